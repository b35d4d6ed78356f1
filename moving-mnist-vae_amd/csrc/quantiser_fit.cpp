// Host side of the pixel quantiser: the fit and the label statistics the reference gets from scikit-learn and from sampling
// (utils.py:279-309), as exact functions of the 256-bin histogram quantiser.hip takes on the device.  Plain C++: no HIP header.
//
// kmeans1d_fit: k-means in one dimension has an optimum whose clusters are contiguous runs of the sorted points, so it is a
// shortest-path problem over cut positions.  With m <= 256 distinct byte values the O(q m^2) dynamic programme is a few million
// operations; the result is the global optimum (never worse than Lloyd's iterations from random starts, which is what
// sklearn.cluster.KMeans runs) and depends on nothing but the histogram.  Centres come back ASCENDING, so label k is the k-th
// darkest cluster; scikit-learn's label order is an accident of its initialisation.  data_mean / data_std are statistics of the
// LABELS and therefore depend on that order: a quantiser fitted here and one carried over from scikit-learn give the same
// partition (where scikit-learn found the optimum) under different label names, and each must be used with its own statistics.
//
// The segment cost sum c (b - mean)^2 = S2 - S1^2 / W is formed from exact integer prefix sums (W = sum c, S1 = sum c b,
// S2 = sum c b^2, b the integer byte value) as (S2 W - S1^2) / W with the numerator in 128 bits: no cancellation between two
// rounded floating-point sums.  S2 fits 64 bits while W <= 2^64 / 255^2 (2.8e14 pixels); more is rejected.
//
// quantiser_stats: lut[b] repeats quantise_normalise_kernel (latent_loss.hip) operation by operation in f32 -- x = b / 255.0f,
// d = (x - c) * (x - c), strict < so the lowest index wins a tie -- on the f32 centres that kernel would be handed.  Built with
// -ffp-contract=off (Makefile) and the pragma below, never with fast-math: nothing may change one of those comparisons.
#include "quantiser_fit.hpp"

#include <math.h>

#include <vector>

#include "../../include/mmvae.h"

#ifdef __FAST_MATH__
#error "quantiser_fit.cpp repeats a kernel's f32 comparisons: build it without fast-math"
#endif
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace mmvae {

namespace {

typedef unsigned __int128 u128;

inline double u128_to_double(u128 v) { return ldexp((double)(uint64_t)(v >> 64), 64) + (double)(uint64_t)v; }

struct Prefix {
  int m = 0;                                   // non-empty bins
  uint64_t W[257], S1[257], S2[257];           // sums over the first i non-empty bins
  // sum over bins [i, j) of c (b - mean)^2, in byte units squared
  double cost(int i, int j) const {
    const uint64_t w = W[j] - W[i], s1 = S1[j] - S1[i], s2 = S2[j] - S2[i];
    const u128 num = (u128)s2 * w - (u128)s1 * s1;         // >= 0 (Cauchy-Schwarz), exact
    return u128_to_double(num) / (double)w;
  }
  double mean(int i, int j) const { return (double)(S1[j] - S1[i]) / (double)(W[j] - W[i]) / 255.0; }
};

// 0, or an error code with the message set
int build_prefix(const uint64_t* counts, Prefix& P) {
  const uint64_t kMaxPixels = UINT64_MAX / (255ull * 255ull);
  P.W[0] = P.S1[0] = P.S2[0] = 0;
  for (int b = 0; b < 256; ++b) {
    const uint64_t c = counts[b];
    if (!c) continue;
    if (c > kMaxPixels || P.W[P.m] > kMaxPixels - c) {
      set_error("kmeans1d_fit: more than %llu pixels (the exact 64-bit sums would overflow)", (unsigned long long)kMaxPixels);
      return MMVAE_ERR_UNSUPPORTED;
    }
    P.W[P.m + 1] = P.W[P.m] + c;
    P.S1[P.m + 1] = P.S1[P.m] + c * (uint64_t)b;
    P.S2[P.m + 1] = P.S2[P.m] + c * (uint64_t)(b * b);
    ++P.m;
  }
  return MMVAE_OK;
}

}  // namespace

int kmeans1d_fit(const uint64_t* counts, int q, double* centres, double* inertia) {
  if (!counts || !centres) { set_error("kmeans1d_fit: NULL counts or centres"); return MMVAE_ERR_ARG; }
  if (q < 1 || q > 256) { set_error("kmeans1d_fit: q=%d out of range (1..256)", q); return MMVAE_ERR_ARG; }
  Prefix P;
  if (int rc = build_prefix(counts, P)) return rc;
  const int m = P.m;
  if (m == 0) { set_error("kmeans1d_fit: the histogram is empty (all counts are zero)"); return MMVAE_ERR_ARG; }
  if (q > m) { set_error("kmeans1d_fit: q=%d clusters asked of data with %d distinct values", q, m); return MMVAE_ERR_ARG; }

  // best[j]: least cost of the first j bins in k non-empty contiguous clusters; cut[k][j]: where the last of them starts
  // (the smallest such index among equal costs: candidates ascend and only a strictly lower cost replaces)
  std::vector<double> prev(m + 1, 0.0), best(m + 1, 0.0);
  std::vector<int16_t> cut((size_t)q * (m + 1), 0);
  for (int j = 1; j <= m; ++j) prev[j] = P.cost(0, j);
  for (int k = 2; k <= q; ++k) {
    for (int j = k; j <= m; ++j) {
      int arg = k - 1;
      double lo = prev[arg] + P.cost(arg, j);
      for (int i = k; i < j; ++i) {
        const double c = prev[i] + P.cost(i, j);
        if (c < lo) { lo = c; arg = i; }
      }
      best[j] = lo;
      cut[(size_t)(k - 1) * (m + 1) + j] = (int16_t)arg;
    }
    prev.swap(best);
  }
  double total = 0.0;
  int end = m;
  for (int k = q; k >= 1; --k) {
    const int start = k == 1 ? 0 : cut[(size_t)(k - 1) * (m + 1) + end];
    centres[k - 1] = P.mean(start, end);
    total += P.cost(start, end);
    end = start;
  }
  if (inertia) *inertia = total / (255.0 * 255.0);
  return MMVAE_OK;
}

int quantiser_stats(const uint64_t* counts, const float* centres, int q, uint8_t* lut, double* ratios, double* label_mean,
                    double* label_std) {
  if (!counts || !centres || !lut) { set_error("quantiser_stats: NULL counts, centres or lut"); return MMVAE_ERR_ARG; }
  if (q < 1 || q > 256) { set_error("quantiser_stats: q=%d out of range (1..256)", q); return MMVAE_ERR_ARG; }
  uint64_t per_label[256] = {0}, total = 0;
  for (int b = 0; b < 256; ++b) {
    const float x = (float)b / 255.0f;
    int lab = 0;
    float bd = (x - centres[0]) * (x - centres[0]);
    for (int k = 1; k < q; ++k) { const float d = (x - centres[k]) * (x - centres[k]); if (d < bd) { bd = d; lab = k; } }
    lut[b] = (uint8_t)lab;
    if (counts[b] > UINT64_MAX - total) { set_error("quantiser_stats: the counts overflow 64 bits"); return MMVAE_ERR_UNSUPPORTED; }
    total += counts[b];
    per_label[lab] += counts[b];
  }
  if (!total) { set_error("quantiser_stats: the histogram is empty (all counts are zero)"); return MMVAE_ERR_ARG; }
  const double n = (double)total;
  double mean = 0.0;
  for (int k = 0; k < q; ++k) mean += (double)k * ((double)per_label[k] / n);
  double var = 0.0;
  for (int k = 0; k < q; ++k) var += ((double)k - mean) * ((double)k - mean) * ((double)per_label[k] / n);
  if (ratios) for (int k = 0; k < q; ++k) ratios[k] = (double)per_label[k] / n;
  if (label_mean) *label_mean = mean;
  if (label_std) *label_std = sqrt(var);
  return MMVAE_OK;
}

}  // namespace mmvae
