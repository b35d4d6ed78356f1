// The resize branch of the reference's input transform (choose_transformer, main.py:33-38: ToPILImage -> Resize(S) -> ToTensor ->
// kmeans.predict) and the normalisation of main.py:383-387 in one kernel: uint8 planes resident in HBM -> Pillow's bytes at
// out_h x out_w -> k-means labels (int64) and the normalised f32 image.  The bytes are Pillow's exactly: both passes are integer sums
// over the 22-bit taps of resample.cpp, the horizontal one (along W) first, each rounded and clamped to uint8.
//
// Work decomposition.  One block of 256 threads takes whole planes, block b the planes b, b + grid, ...; the grid is one resident
// round (kMaxGrid).  Per plane: global -> LDS (16-byte loads when the host found every plane base 16-byte aligned, bytes otherwise),
// horizontal pass LDS -> LDS (in_h x out_w), vertical pass LDS -> registers, byte -> label and image through two 256-entry tables in
// LDS, stores.  Both coefficient tables are copied to LDS once per block.  The label table is quantise_byte() of every byte value
// and the image table ((float)label - mean) / stdv, the expressions of quantise_normalise_kernel, so for the same resized bytes the
// outputs are that kernel's bit for bit.  With out_h * out_w a multiple of 4 and 16-byte aligned outputs a lane produces 4
// neighbouring pixels and stores them as two 16-byte label vectors, one 16-byte image vector and one 4-byte word of resized bytes.
//
// No atomics; every output element is written by exactly one thread from integer sums in a fixed order: the same bits every run.
#include "common.hpp"
#include "kernels.hpp"
#include "resample.hpp"

namespace mmvae {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxGrid = 2048;                 // 256 CUs x 8 blocks of 256 threads: one resident round
constexpr int kPrecisionBits = 22;

struct ResizeArgs {
  const unsigned char* frames;
  long frame_stride;
  const long long* clip_index;
  int frames_per_clip;
  long n_frames;
  int in_h, in_w, out_h, out_w;
  const int* h_bounds; const int* h_coeffs; int h_ksize;
  const int* v_bounds; const int* v_coeffs; int v_ksize;
  const float* centres; int q;
  float mean, stdv;
  float inv_out_w;                             // 1.0f / out_w (div_small)
  long long* labels; float* image; unsigned char* resized;
};

__host__ __device__ constexpr int align16(int n) { return (n + 15) & ~15; }

// i / w for 0 <= i < 2^14 and 1 <= w <= 128, inv = 1.0f / w.  (i + 0.5) / w is at least 1 / 256 away from every integer and at most
// 128; the two f32 roundings move it by less than 128 * 2^-22, so the truncation is the exact quotient.
__device__ __forceinline__ int div_small(int i, float inv) { return (int)(((float)i + 0.5f) * inv); }

__device__ __forceinline__ unsigned clip8(int acc) { return (unsigned)min(max(acc >> kPrecisionBits, 0), 255); }

// LDS carve-up, shared by the kernel and the host's size arithmetic (every offset a multiple of 16)
struct Carve {
  int src, mid, img_lut, hb, hc, vb, vc, lab_lut, total;
  __host__ __device__ Carve(int in_h, int in_w, int out_h, int out_w, int hk, int vk) {
    src = 0;
    mid = src + align16(in_h * in_w);
    img_lut = mid + align16(in_h * out_w);
    hb = img_lut + 256 * 4;
    hc = hb + align16(2 * out_w * 4);
    vb = hc + align16(out_w * hk * 4);
    vc = vb + align16(2 * out_h * 4);
    lab_lut = vc + align16(out_h * vk * 4);
    total = lab_lut + 256;
  }
};

template <bool kVecIn, bool kVecOut>
__global__ __launch_bounds__(kThreads) void resize_quantise_kernel(const ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int in_px = a.in_h * a.in_w, mid_px = a.in_h * a.out_w, out_px = a.out_h * a.out_w;
  const Carve c(a.in_h, a.in_w, a.out_h, a.out_w, a.h_ksize, a.v_ksize);
  unsigned char* src = smem + c.src;
  unsigned char* mid = smem + c.mid;
  float* img_lut = reinterpret_cast<float*>(smem + c.img_lut);
  int* hb = reinterpret_cast<int*>(smem + c.hb);
  int* hc = reinterpret_cast<int*>(smem + c.hc);
  int* vb = reinterpret_cast<int*>(smem + c.vb);
  int* vc = reinterpret_cast<int*>(smem + c.vc);
  unsigned char* lab_lut = smem + c.lab_lut;

  // once per block (the first barrier of the plane loop publishes them)
  for (int i = tid; i < 2 * a.out_w; i += kThreads) hb[i] = a.h_bounds[i];
  for (int i = tid; i < a.out_w * a.h_ksize; i += kThreads) hc[i] = a.h_coeffs[i];
  for (int i = tid; i < 2 * a.out_h; i += kThreads) vb[i] = a.v_bounds[i];
  for (int i = tid; i < a.out_h * a.v_ksize; i += kThreads) vc[i] = a.v_coeffs[i];
  if (a.centres) {                               // one byte value per thread
    const int lab = quantise_byte((unsigned char)tid, a.centres, a.q);
    lab_lut[tid] = (unsigned char)lab;
    img_lut[tid] = ((float)lab - a.mean) / a.stdv;
  }

  for (long p = blockIdx.x; p < a.n_frames; p += gridDim.x) {
    const long clip = p / a.frames_per_clip;
    const long plane = (a.clip_index ? (long)a.clip_index[clip] : clip) * a.frames_per_clip + (p - clip * a.frames_per_clip);
    const unsigned char* g = a.frames + plane * a.frame_stride;
    if constexpr (kVecIn) {
      const int nvec = in_px >> 4;
      for (int i = tid; i < nvec; i += kThreads) reinterpret_cast<uint4*>(src)[i] = reinterpret_cast<const uint4*>(g)[i];
      for (int i = (nvec << 4) + tid; i < in_px; i += kThreads) src[i] = g[i];
    } else {
      for (int i = tid; i < in_px; i += kThreads) src[i] = g[i];
    }
    __syncthreads();

    // horizontal: mid[y][x] from src[y][first .. first + n)
    for (int i = tid; i < mid_px; i += kThreads) {
      const int y = div_small(i, a.inv_out_w), x = i - y * a.out_w;
      const int first = hb[2 * x], n = hb[2 * x + 1];
      const int* k = hc + x * a.h_ksize;
      const unsigned char* s = src + y * a.in_w + first;
      int acc = 1 << (kPrecisionBits - 1);
      for (int j = 0; j < n; ++j) acc += (int)s[j] * k[j];
      mid[i] = (unsigned char)clip8(acc);
    }
    __syncthreads();

    // vertical: out[y][x] from mid[first .. first + n)[x]; kGroup neighbouring pixels per lane
    constexpr int kGroup = kVecOut ? 4 : 1;
    const long obase = p * out_px;
    for (int g0 = tid * kGroup; g0 < out_px; g0 += kThreads * kGroup) {
      unsigned r[kGroup];
#pragma unroll
      for (int e = 0; e < kGroup; ++e) {
        const int i = g0 + e;
        const int y = div_small(i, a.inv_out_w), x = i - y * a.out_w;
        const int first = vb[2 * y], n = vb[2 * y + 1];
        const int* k = vc + y * a.v_ksize;
        const unsigned char* s = mid + first * a.out_w + x;
        int acc = 1 << (kPrecisionBits - 1);
        for (int j = 0; j < n; ++j) acc += (int)s[j * a.out_w] * k[j];
        r[e] = clip8(acc);
      }
      if constexpr (kVecOut) {
        if (a.resized) *reinterpret_cast<unsigned*>(a.resized + obase + g0) = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
        if (a.labels) {
          longlong2* l = reinterpret_cast<longlong2*>(a.labels + obase + g0);
          l[0] = make_longlong2(lab_lut[r[0]], lab_lut[r[1]]);
          l[1] = make_longlong2(lab_lut[r[2]], lab_lut[r[3]]);
        }
        if (a.image)
          *reinterpret_cast<float4*>(a.image + obase + g0) = make_float4(img_lut[r[0]], img_lut[r[1]], img_lut[r[2]], img_lut[r[3]]);
      } else {
        if (a.resized) a.resized[obase + g0] = (unsigned char)r[0];
        if (a.labels) a.labels[obase + g0] = lab_lut[r[0]];
        if (a.image) a.image[obase + g0] = img_lut[r[0]];
      }
    }
    // no barrier here: the next plane's loads touch only src, which nobody reads behind the barrier above, and its horizontal
    // pass writes mid behind the next barrier, which no thread passes before it has left this loop
  }
}

}  // namespace

int launch_resize_quantise_normalise(const unsigned char* frames, long frame_stride, const long long* clip_index, int frames_per_clip,
                                     long n_frames, int in_h, int in_w, int out_h, int out_w, const int* h_bounds, const int* h_coeffs,
                                     int h_ksize, const int* v_bounds, const int* v_coeffs, int v_ksize, const float* centres, int q,
                                     float mean, float stdv, long long* labels, float* image, unsigned char* resized, hipStream_t s) {
  if (n_frames < 0) { set_error("resize: negative n_frames"); return MMVAE_ERR_ARG; }
  if (!labels && !image && !resized) { set_error("resize: labels, image and resized are all NULL"); return MMVAE_ERR_ARG; }
  const int sizes[4] = {in_h, in_w, out_h, out_w};
  for (int v : sizes)
    if (v < 1 || v > kResampleMaxSize) { set_error("resize: %dx%d -> %dx%d outside [1, %d]", in_h, in_w, out_h, out_w, kResampleMaxSize); return MMVAE_ERR_ARG; }
  // the tap counts resample_coeffs gives these sizes: the kernel trusts the tables' shape
  int hk = 0, vk = 0;
  if (int rc = resample_coeffs(in_w, out_w, &hk, nullptr, nullptr)) return rc;
  if (int rc = resample_coeffs(in_h, out_h, &vk, nullptr, nullptr)) return rc;
  if (h_ksize != hk || v_ksize != vk) {
    set_error("resize: ksize %d / %d given, %d -> %d and %d -> %d have %d / %d", h_ksize, v_ksize, in_w, out_w, in_h, out_h, hk, vk);
    return MMVAE_ERR_ARG;
  }
  if (frames_per_clip < 1) { set_error("resize: frames_per_clip=%d", frames_per_clip); return MMVAE_ERR_ARG; }
  if (frame_stride < (long)in_h * in_w) { set_error("resize: frame stride %ld below the plane's %d bytes", frame_stride, in_h * in_w); return MMVAE_ERR_ARG; }
  if (labels || image) {
    if (!centres) { set_error("resize: labels or image asked for without centres"); return MMVAE_ERR_ARG; }
    if (q < 1 || q > 256) { set_error("resize: q=%d out of range", q); return MMVAE_ERR_ARG; }
  }
  if (n_frames == 0) return MMVAE_OK;
  if (!frames || !h_bounds || !h_coeffs || !v_bounds || !v_coeffs) { set_error("resize: NULL frames or tables"); return MMVAE_ERR_ARG; }

  ResizeArgs a{frames, frame_stride, clip_index, frames_per_clip, n_frames, in_h, in_w, out_h, out_w, h_bounds, h_coeffs, h_ksize,
               v_bounds, v_coeffs, v_ksize, (labels || image) ? centres : nullptr, q, mean, stdv, 1.0f / (float)out_w, labels, image, resized};
  const Carve c(in_h, in_w, out_h, out_w, h_ksize, v_ksize);          // <= 16 K + 16 K + 1 K + 2 * (1 K + 2.5 K) + 256 bytes
  const bool vec_in = reinterpret_cast<uintptr_t>(frames) % 16 == 0 && frame_stride % 16 == 0;
  const long out_px = (long)out_h * out_w;
  const bool vec_out = out_px % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % 16 == 0 && reinterpret_cast<uintptr_t>(image) % 16 == 0 &&
                       reinterpret_cast<uintptr_t>(resized) % 4 == 0;
  const dim3 grid((unsigned)(n_frames < kMaxGrid ? n_frames : kMaxGrid)), block(kThreads);
  note_launch_bytes((double)n_frames * ((double)in_h * in_w + (double)out_px * ((labels ? 8 : 0) + (image ? 4 : 0) + (resized ? 1 : 0))));
  if (vec_in && vec_out) hipLaunchKernelGGL((resize_quantise_kernel<true, true>), grid, block, c.total, s, a);
  else if (vec_in) hipLaunchKernelGGL((resize_quantise_kernel<true, false>), grid, block, c.total, s, a);
  else if (vec_out) hipLaunchKernelGGL((resize_quantise_kernel<false, true>), grid, block, c.total, s, a);
  else hipLaunchKernelGGL((resize_quantise_kernel<false, false>), grid, block, c.total, s, a);
  return check_launch("resize_quantise_normalise");
}

}  // namespace mmvae
