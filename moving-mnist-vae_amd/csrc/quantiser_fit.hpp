// Host side of the pixel quantiser (quantiser_fit.cpp): plain C++, no HIP header, so a host compiler builds it on its own.
#pragma once
#include <stdint.h>

namespace mmvae {

void set_error(const char* fmt, ...);          // runtime.cpp (a stand-alone program that links quantiser_fit.cpp alone brings its own)

// Exact k-means of the 256-bin byte histogram `counts` into q clusters (mmvae_kmeans1d_fit of include/mmvae.h).
int kmeans1d_fit(const uint64_t* counts, int q, double* centres, double* inertia);
// Label of every byte under quantise_normalise_kernel's rule and the label statistics that follow (mmvae_quantiser_stats).
int quantiser_stats(const uint64_t* counts, const float* centres, int q, uint8_t* lut, double* ratios, double* label_mean, double* label_std);

}  // namespace mmvae
