// The panel rule of include/mmvae.h as device functions: how one pixel of a mmvae_panel_col becomes a grey byte.  panels.hip (the contact
// sheet) and frame_quality.hip (MSE / SSIM of two columns) both call panel_byte(), so a metric is of exactly the bytes the sheet shows.
//
// Pick rule.  pick_label() is the one device function that turns the Q logits of a pixel into a label.
//   argmax: strict `>` scan from index 0 against a running maximum that starts at -inf: the lowest index among equal maxima, a NaN never
//           wins, an all-NaN (or all -inf) pixel gives 0.
//   sample: f32 softmax (maximum subtracted, expf, sum in channel order), p_k = e_k / sum, then label = #{k in [0, Q-2] : cdf_k <= u} with
//           cdf accumulated in channel order -- the rule of model.draw_labels and of pixel_head_kernel (pixelcnn.hip).  That kernel keeps
//           its own loop: it sums the exponentials by a lane butterfly, another order of additions than this serial sum, so folding the two
//           together would change its bits.
// Logits are planar [N][Q][HW], so a thread's Q loads are HW apart and neighbouring lanes read neighbouring addresses.  The logits stay in
// registers (the loops over 16 are fully unrolled and predicated on k < Q); no LDS.
#pragma once
#include "common.hpp"

namespace mmvae {

constexpr int kPanelMaxQ = 16;

__device__ __forceinline__ int pick_label(const float* __restrict__ p, long stride, int Q, bool sample, float u) {
  float l[kPanelMaxQ];
#pragma unroll
  for (int k = 0; k < kPanelMaxQ; ++k) l[k] = k < Q ? p[k * stride] : -INFINITY;
  float mx = -INFINITY;
  int best = 0;
#pragma unroll
  for (int k = 0; k < kPanelMaxQ; ++k)
    if (k < Q && l[k] > mx) { mx = l[k]; best = k; }
  if (!sample) return best;
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < kPanelMaxQ; ++k) {
    l[k] = k < Q ? expf(l[k] - mx) : 0.f;
    sum += l[k];
  }
  float cdf = 0.f;
  int label = 0;
#pragma unroll
  for (int k = 0; k < kPanelMaxQ - 1; ++k)
    if (k < Q - 1) {                                                 // inverse CDF: label = #{k <= Q - 2 : cdf_k <= u}
      cdf += l[k] / sum;
      label += cdf <= u;
    }
  return label;
}

__device__ __forceinline__ unsigned lut_byte(const unsigned char* __restrict__ lut, long long label, int Q) {
  return (unsigned long long)label < (unsigned long long)Q ? lut[label] : 0u;
}

// The byte of pixel `pix` of plane `r` of a column of S x S planes (HW = S * S), kinds MMVAE_PANEL_LABELS_U8 .. MMVAE_PANEL_IMAGE_F32.
__device__ __forceinline__ unsigned panel_byte(const mmvae_panel_col& col, long r, int pix, int HW) {
  const long at = r * HW + pix;                                      // index into a [n][S*S] tensor
  switch (col.kind) {
    case MMVAE_PANEL_LABELS_U8:
      return lut_byte(col.lut, static_cast<const unsigned char*>(col.src)[at], col.Q);
    case MMVAE_PANEL_LABELS_I64:
      return lut_byte(col.lut, static_cast<const long long*>(col.src)[at], col.Q);
    case MMVAE_PANEL_LOGITS_ARGMAX:
      return col.lut[pick_label(static_cast<const float*>(col.src) + r * col.Q * HW + pix, HW, col.Q, false, 0.f)];
    case MMVAE_PANEL_LOGITS_SAMPLE:
      return col.lut[pick_label(static_cast<const float*>(col.src) + r * col.Q * HW + pix, HW, col.Q, true, col.uniforms[at])];
    default: {                                                       // MMVAE_PANEL_IMAGE_F32; explicit roundings: no contraction
      const float v = static_cast<const float*>(col.src)[at];
      const float t = __fmul_rn(__fdiv_rn(__fsub_rn(v, col.lo), __fsub_rn(col.hi, col.lo)), 255.f);
      float b = floorf(__fadd_rn(t, 0.5f));
      b = b > 0.f ? b : 0.f;                                         // NaN -> 0
      return (unsigned)(b < 255.f ? b : 255.f);
    }
  }
}

}  // namespace mmvae
