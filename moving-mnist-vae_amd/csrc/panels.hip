// Picture panels of the reference's plot branch (main.py:205-359, utils.py:77-83) on the device: logits, labels or f32 images in,
// class labels or the bytes of an 8-bit greyscale contact sheet out.  The host side (main.py: render_sheet, plot_*) only describes the
// columns; no softmax / argmax / cat / indexing chain in ATen, no f32 tensor crosses to the host.
//
// Pick rule and byte rule.  panel_decode.hpp holds them (pick_label(), panel_byte()): the quality kernel (frame_quality.hip) reduces its
// two sides to bytes through the same functions.  One thread per pixel.
//
// Sheet.  out is uint8 [n * S][ncols * S]; column c holds its n planes stacked vertically in bytes [:, c*S : (c+1)*S].  The grid is
// (pixels of one column, column): the column descriptor, a kernel argument passed by value, is indexed by blockIdx.y only, so it is read
// with wave-uniform loads.  Inside a column the row is padded to Sp = S rounded up to 4 threads, which makes every aligned group of four
// lanes four neighbouring pixels of one output row.  Where the group's first byte is 4-byte aligned and all four pixels exist, its first
// lane collects the bytes by shuffles and issues one 32-bit store; otherwise (odd sheet widths such as S = 9, the ragged end of a row)
// every lane stores its own byte.
#include "common.hpp"
#include "kernels.hpp"
#include "panel_decode.hpp"

namespace mmvae {

namespace {

constexpr int kMaxQ = kPanelMaxQ;
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void logits_to_labels_kernel(const float* __restrict__ logits, long npix, int Q, int HW, int sample,
                                                                   const float* __restrict__ uniforms, long long* __restrict__ labels) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= npix) return;
  const long n = i / HW, p = i - n * HW;
  labels[i] = pick_label(logits + n * Q * HW + p, HW, Q, sample != 0, sample ? uniforms[i] : 0.f);
}

struct PanelCols { mmvae_panel_col c[MMVAE_PANEL_MAX_COLS]; };

__global__ __launch_bounds__(kThreads) void panel_sheet_kernel(PanelCols cols, int ncols, long n, int S, int Sp,
                                                              unsigned char* __restrict__ out) {
  const mmvae_panel_col& col = cols.c[blockIdx.y];
  const long g = (long)blockIdx.x * kThreads + threadIdx.x;
  const int x = (int)(g % Sp);
  const long row = g / Sp;                                           // row of the sheet: plane r = row / S, line y = row % S
  const bool live = x < S && row < n * S;
  unsigned byte = 0;
  if (live) {
    const int HW = S * S;
    const long r = row / S;
    const int pix = (int)(row - r * S) * S + x;
    byte = panel_byte(col, r, pix, HW);
  }
  // the four lanes [q, q + 4) hold pixels x0 .. x0 + 3 of one sheet row (Sp and the block size are multiples of 4); every lane of the
  // wave takes part in the shuffles
  const unsigned b1 = __shfl_down(byte, 1, 64), b2 = __shfl_down(byte, 2, 64), b3 = __shfl_down(byte, 3, 64);
  if (!live) return;
  unsigned char* dst = out + row * ((long)ncols * S) + (long)blockIdx.y * S + x;
  const int x0 = x & ~3;
  const bool packed = x0 + 3 < S && ((reinterpret_cast<uintptr_t>(dst - (x - x0))) & 3) == 0;
  if (!packed) *dst = (unsigned char)byte;
  else if (x == x0) *reinterpret_cast<unsigned*>(dst) = byte | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

}  // namespace

int launch_logits_to_labels(const float* logits, int N, int Q, int HW, int mode, const float* uniforms, long long* labels, hipStream_t s) {
  if (Q < 1 || Q > kMaxQ) { set_error("logits_to_labels: Q=%d unsupported (1..%d)", Q, kMaxQ); return MMVAE_ERR_UNSUPPORTED; }
  if (N < 1 || HW < 1) { set_error("logits_to_labels: N=%d, HW=%d must be positive", N, HW); return MMVAE_ERR_ARG; }
  if (mode != MMVAE_PICK_ARGMAX && mode != MMVAE_PICK_SAMPLE) { set_error("logits_to_labels: mode=%d (0 argmax, 1 sample)", mode); return MMVAE_ERR_ARG; }
  if (!logits || !labels) { set_error("logits_to_labels: NULL logits or labels"); return MMVAE_ERR_ARG; }
  if (mode == MMVAE_PICK_SAMPLE && !uniforms) { set_error("logits_to_labels: sample mode needs uniforms"); return MMVAE_ERR_ARG; }
  const long npix = (long)N * HW;
  if (npix * Q > (1l << 40)) { set_error("logits_to_labels: N * Q * HW too large for one launch"); return MMVAE_ERR_UNSUPPORTED; }
  const long grid = (npix + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(logits_to_labels_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, logits, npix, Q, HW, mode, uniforms, labels);
  return check_launch("logits_to_labels");
}

int launch_panel_sheet(const mmvae_panel_col* cols, int ncols, int n, int S, unsigned char* out, hipStream_t s) {
  if (ncols < 1 || ncols > MMVAE_PANEL_MAX_COLS) { set_error("panel_sheet: ncols=%d out of range (1..%d)", ncols, MMVAE_PANEL_MAX_COLS); return MMVAE_ERR_ARG; }
  if (n < 1 || S < 1 || S > 64) { set_error("panel_sheet: n=%d, S=%d out of range (n >= 1, 1 <= S <= 64)", n, S); return MMVAE_ERR_ARG; }
  if (!cols || !out) { set_error("panel_sheet: NULL cols or out"); return MMVAE_ERR_ARG; }
  PanelCols a{};
  for (int c = 0; c < ncols; ++c) {
    const mmvae_panel_col& k = cols[c];
    if (k.kind < MMVAE_PANEL_LABELS_U8 || k.kind > MMVAE_PANEL_IMAGE_F32) { set_error("panel_sheet: column %d has kind %d", c, k.kind); return MMVAE_ERR_ARG; }
    if (!k.src) { set_error("panel_sheet: column %d has no source", c); return MMVAE_ERR_ARG; }
    if (k.kind == MMVAE_PANEL_IMAGE_F32) {
      if (!(k.hi > k.lo)) { set_error("panel_sheet: column %d needs hi > lo", c); return MMVAE_ERR_ARG; }
    } else {
      if (k.Q < 1 || k.Q > kMaxQ) { set_error("panel_sheet: column %d has Q=%d (1..%d)", c, k.Q, kMaxQ); return MMVAE_ERR_UNSUPPORTED; }
      if (!k.lut) { set_error("panel_sheet: column %d has no lut", c); return MMVAE_ERR_ARG; }
      if (k.kind == MMVAE_PANEL_LOGITS_SAMPLE && !k.uniforms) { set_error("panel_sheet: column %d samples without uniforms", c); return MMVAE_ERR_ARG; }
    }
    a.c[c] = k;
  }
  const int Sp = (S + 3) & ~3;
  const long per_col = (long)n * S * Sp;                             // n < 2^31, S * Sp <= 4096: no overflow
  const long grid = (per_col + kThreads - 1) / kThreads;             // < 2^35 / 2^8: fits grid.x
  hipLaunchKernelGGL(panel_sheet_kernel, dim3((unsigned)grid, (unsigned)ncols), dim3(kThreads), 0, s, a, ncols, (long)n, S, Sp, out);
  return check_launch("panel_sheet");
}

}  // namespace mmvae
