// Host side of the device resize (resample.cpp): plain C++, no HIP header, so a host compiler builds it on its own.
#pragma once
#include <stdint.h>

namespace mmvae {

void set_error(const char* fmt, ...);          // runtime.cpp (a stand-alone program that links resample.cpp alone brings its own)

constexpr int kResampleMaxSize = 128;          // largest side, in or out, of a resized plane

// Taps of one axis of the 8-bit antialiased bilinear resize (mmvae_resample_coeffs of include/mmvae.h).
int resample_coeffs(int in_size, int out_size, int* ksize, int32_t* bounds, int32_t* coeffs);

}  // namespace mmvae
