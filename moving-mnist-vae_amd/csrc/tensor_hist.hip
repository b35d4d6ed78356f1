// Per-tensor histograms of a flat f32 buffer: what wandb.hook_torch logs for every parameter (reference main.py:456: min(), max(),
// histc(bins=64) per tensor), for all T tensors of the model's flat gradient / parameter / moment buffer in three launches.
//
// The rule (include/mmvae.h), every operation a correctly rounded f32 operation, written with the explicit _rn intrinsics:
//   lo, hi = min / max of the finite elements (none: lo = hi = 0, no counts); lo == hi: lo - 1 .. hi + 1;
//   bin(x) = min((int)(((x - lo) * 64) / (hi - lo)), 63) for a finite x; NaN / +-inf are counted apart.
//
// Work comes as chunks (segment, start, length), one block each: the largest tensor is spread over many blocks, a 16-element bias
// costs a block that ends after one load.  A chunk starts at any element: its head up to the next 16-byte boundary and its tail go one
// element per thread, the body as 16-byte loads.
//   hist_stats_kernel     per chunk: min, max, the three counts and the f64 sums of its finite elements -> part[chunk][8].  Per thread
//                         in element order, a fixed xor tree over the wave, the waves in order through LDS.
//   hist_finalize_kernel  one wave per segment: lane l takes the chunks l, l + 64, ... of the list that belong to the segment, in that
//                         order, then the same xor tree.  Writes lo, hi (widened), the stats row, and zeroes the segment's 64 counts.
//   hist_bins_kernel      per chunk: 16 copies of the 64 bins in LDS (a copy per lane mod 16: gradients crowd into a few bins around
//                         zero, one copy would serialise the wave on them), integer LDS atomics, then one integer global atomic per
//                         non-empty bin.  Integer sums do not depend on their order.
// No floating-point atomics, no data-dependent launch: the same input gives the same bits, and the three launches can be captured.
#include "common.hpp"
#include "kernels.hpp"

namespace mmvae {

namespace {

constexpr int kBins = MMVAE_TENSOR_HIST_BINS, kStats = MMVAE_TENSOR_HIST_STATS;
constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kCopies = 16, kPitch = kBins + 1;          // (an odd pitch: the same bin of two copies never shares a bank)
constexpr int kPart = 8;                                 // doubles per chunk: min, max, n_finite, n_nonfinite, n_zero, sum, sumsq, -

__device__ __forceinline__ bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// f(x) for every element of p[0 .. n): a thread's elements in increasing address order
template <typename F>
__device__ __forceinline__ void for_each_element(const float* __restrict__ p, long long n, F f) {
  const int tid = threadIdx.x;
  long long head = (long long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
  if (head > n) head = n;
  if (tid < head) f(p[tid]);
  const float4* __restrict__ body = reinterpret_cast<const float4*>(p + head);
  const long long nvec = (n - head) >> 2;
  for (long long v = tid; v < nvec; v += kThreads) {
    const float4 q = body[v];
    f(q.x); f(q.y); f(q.z); f(q.w);
  }
  const long long done = head + 4 * nvec;
  if (tid < n - done) f(p[done + tid]);
}

struct Part {
  float mn, mx;
  long long nf, nn, nz;
  double s, ss;
};

__device__ __forceinline__ long long shfl_xor_ll(long long v, int o) {
  const int lo = __shfl_xor((int)(v & 0xffffffffll), o, 64), hi = __shfl_xor((int)(v >> 32), o, 64);
  return ((long long)hi << 32) | (unsigned int)lo;
}

__device__ __forceinline__ void wave_join(Part& a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.mn = fminf(a.mn, __shfl_xor(a.mn, o, 64));
    a.mx = fmaxf(a.mx, __shfl_xor(a.mx, o, 64));
    a.nf += shfl_xor_ll(a.nf, o);
    a.nn += shfl_xor_ll(a.nn, o);
    a.nz += shfl_xor_ll(a.nz, o);
    a.s += __shfl_xor(a.s, o, 64);
    a.ss += __shfl_xor(a.ss, o, 64);
  }
}

__global__ __launch_bounds__(kThreads) void hist_stats_kernel(const float* __restrict__ flat, const long long* __restrict__ seg,
                                                              const long long* __restrict__ chunk, double* __restrict__ part) {
  __shared__ double red[kWaves][kPart];
  const long long c = blockIdx.x;
  const long long t = chunk[3 * c], start = chunk[3 * c + 1], len = chunk[3 * c + 2];
  Part a{__builtin_inff(), -__builtin_inff(), 0, 0, 0, 0.0, 0.0};
  for_each_element(flat + seg[2 * t] + start, len, [&](float x) {
    if (finite_f32(x)) {
      a.mn = fminf(a.mn, x);
      a.mx = fmaxf(a.mx, x);
      a.nf += 1;
      a.nz += (x == 0.0f);
      const double d = (double)x;
      a.s += d;
      a.ss += d * d;
    } else {
      a.nn += 1;
    }
  });
  wave_join(a);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    red[w][0] = (double)a.mn; red[w][1] = (double)a.mx;
    red[w][2] = (double)a.nf; red[w][3] = (double)a.nn; red[w][4] = (double)a.nz;      // (counts of a chunk: exact in f64 below 2^53)
    red[w][5] = a.s; red[w][6] = a.ss;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r[kPart] = {red[0][0], red[0][1], red[0][2], red[0][3], red[0][4], red[0][5], red[0][6], 0.0};
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
      r[0] = fmin(r[0], red[k][0]);
      r[1] = fmax(r[1], red[k][1]);
#pragma unroll
      for (int q = 2; q < 7; ++q) r[q] += red[k][q];
    }
#pragma unroll
    for (int q = 0; q < kPart; ++q) part[c * kPart + q] = r[q];
  }
}

__global__ __launch_bounds__(kWave) void hist_finalize_kernel(const long long* __restrict__ chunk, long long n_chunks,
                                                              const double* __restrict__ part, int* __restrict__ counts,
                                                              float* __restrict__ lo, float* __restrict__ hi, double* __restrict__ stats) {
  const long long t = blockIdx.x;
  const int lane = threadIdx.x;
  double mn = (double)__builtin_inff(), mx = -(double)__builtin_inff(), nf = 0.0, nn = 0.0, nz = 0.0, s = 0.0, ss = 0.0;
  for (long long c = lane; c < n_chunks; c += kWave)
    if (chunk[3 * c] == t) {
      const double* p = part + c * kPart;
      mn = fmin(mn, p[0]); mx = fmax(mx, p[1]);
      nf += p[2]; nn += p[3]; nz += p[4]; s += p[5]; ss += p[6];
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fmin(mn, __shfl_xor(mn, o, 64));
    mx = fmax(mx, __shfl_xor(mx, o, 64));
    nf += __shfl_xor(nf, o, 64); nn += __shfl_xor(nn, o, 64); nz += __shfl_xor(nz, o, 64);
    s += __shfl_xor(s, o, 64); ss += __shfl_xor(ss, o, 64);
  }
  counts[t * kBins + lane] = 0;
  if (lane == 0) {
    float l = 0.0f, h = 0.0f;
    if (nf > 0.0) {
      l = (float)mn; h = (float)mx;                       // (f32 values widened to f64 and back: exact)
      if (l == h) { l = __fsub_rn(l, 1.0f); h = __fadd_rn(h, 1.0f); }
    }
    lo[t] = l; hi[t] = h;
    double* r = stats + t * kStats;
    r[0] = nf; r[1] = nn; r[2] = nz; r[3] = s; r[4] = ss;
    r[5] = nf > 0.0 ? s / nf : 0.0;
    r[6] = nf > 0.0 ? sqrt(ss / nf) : 0.0;
    r[7] = 0.0;
  }
}

__global__ __launch_bounds__(kThreads) void hist_bins_kernel(const float* __restrict__ flat, const long long* __restrict__ seg,
                                                             const long long* __restrict__ chunk, const float* __restrict__ lo,
                                                             const float* __restrict__ hi, int* __restrict__ counts) {
  __shared__ int bins[kCopies * kPitch];
  const int tid = threadIdx.x;
  for (int i = tid; i < kCopies * kPitch; i += kThreads) bins[i] = 0;
  __syncthreads();
  const long long c = blockIdx.x;
  const long long t = chunk[3 * c], start = chunk[3 * c + 1], len = chunk[3 * c + 2];
  const float l = lo[t], width = __fsub_rn(hi[t], l);
  int* mine = bins + (tid & (kCopies - 1)) * kPitch;
  for_each_element(flat + seg[2 * t] + start, len, [&](float x) {
    if (finite_f32(x)) {
      float q = __fdiv_rn(__fmul_rn(__fsub_rn(x, l), (float)kBins), width);
      q = fminf(fmaxf(q, 0.0f), (float)(kBins - 1));       // NaN (0 / 0, inf / inf of an overflowing range) -> 0; then a safe conversion
      atomicAdd(mine + (int)q, 1);
    }
  });
  __syncthreads();
  if (tid < kBins) {
    int n = 0;
#pragma unroll
    for (int k = 0; k < kCopies; ++k) n += bins[k * kPitch + tid];
    if (n) atomicAdd(counts + t * kBins + tid, n);
  }
}

int check_segments(const char* what, const long long* seg, int T) {
  if (!seg) { set_error("%s: NULL segments", what); return MMVAE_ERR_ARG; }
  if (T <= 0) { set_error("%s: T=%d must be positive", what, T); return MMVAE_ERR_ARG; }
  for (int t = 0; t < T; ++t)
    if (seg[2 * t] < 0 || seg[2 * t + 1] < 0) {
      set_error("%s: segment %d has offset=%lld numel=%lld (neither may be negative)", what, t, seg[2 * t], seg[2 * t + 1]);
      return MMVAE_ERR_ARG;
    }
  return MMVAE_OK;
}

}  // namespace

long long tensor_hist_chunks(const long long* segments, int T, long long chunk_elems, long long* chunks, long long capacity) {
  if (check_segments("tensor_hist_chunks", segments, T) != MMVAE_OK) return MMVAE_ERR_ARG;
  if (chunk_elems <= 0) { set_error("tensor_hist_chunks: chunk_elems=%lld must be positive", chunk_elems); return MMVAE_ERR_ARG; }
  long long n = 0;
  for (int t = 0; t < T; ++t) n += (segments[2 * t + 1] + chunk_elems - 1) / chunk_elems;
  if (!chunks || capacity < n) return n;
  long long c = 0;
  for (int t = 0; t < T; ++t)
    for (long long at = 0; at < segments[2 * t + 1]; at += chunk_elems, ++c) {
      chunks[3 * c] = t;
      chunks[3 * c + 1] = at;
      chunks[3 * c + 2] = segments[2 * t + 1] - at < chunk_elems ? segments[2 * t + 1] - at : chunk_elems;
    }
  return n;
}

size_t tensor_hist_scratch_bytes(int T, long long n_chunks) {
  if (T <= 0 || n_chunks < 0) return 0;
  return (size_t)(n_chunks > 0 ? n_chunks : 1) * kPart * sizeof(double);
}

int launch_tensor_hist(const float* flat, long long flat_numel, const long long* seg_host, const long long* seg_dev, int T,
                       const long long* chunk_host, const long long* chunk_dev, long long n_chunks, int* counts, float* lo, float* hi,
                       double* stats, void* scratch, size_t scratch_bytes, hipStream_t s) {
  const int rc = check_segments("tensor_hist", seg_host, T);
  if (rc != MMVAE_OK) return rc;
  if (n_chunks < 0 || n_chunks > 0x7fffffffll) { set_error("tensor_hist: n_chunks=%lld outside 0..2^31-1", n_chunks); return MMVAE_ERR_ARG; }
  if (!flat || !seg_dev || !counts || !lo || !hi || !stats || !scratch || (n_chunks > 0 && (!chunk_host || !chunk_dev))) {
    set_error("tensor_hist: NULL flat, segments_dev, chunks, chunks_dev, counts, lo, hi, stats or scratch");
    return MMVAE_ERR_ARG;
  }
  if (flat_numel < 0) { set_error("tensor_hist: flat_numel=%lld must not be negative", flat_numel); return MMVAE_ERR_ARG; }
  for (int t = 0; t < T; ++t)
    if (seg_host[2 * t] > flat_numel || seg_host[2 * t + 1] > flat_numel - seg_host[2 * t]) {
      set_error("tensor_hist: segment %d (offset=%lld numel=%lld) leaves the buffer of flat_numel=%lld", t, seg_host[2 * t], seg_host[2 * t + 1],
                flat_numel);
      return MMVAE_ERR_ARG;
    }
  for (long long c = 0; c < n_chunks; ++c) {
    const long long t = chunk_host[3 * c], start = chunk_host[3 * c + 1], len = chunk_host[3 * c + 2];
    if (t < 0 || t >= T) { set_error("tensor_hist: chunk %lld names segment %lld of T=%d", c, t, T); return MMVAE_ERR_ARG; }
    if (start < 0 || len < 0 || start > seg_host[2 * t + 1] || len > seg_host[2 * t + 1] - start) {
      set_error("tensor_hist: chunk %lld (start=%lld length=%lld) leaves segment %lld of numel=%lld", c, start, len, t, seg_host[2 * t + 1]);
      return MMVAE_ERR_ARG;
    }
  }
  const size_t need = tensor_hist_scratch_bytes(T, n_chunks);
  if (scratch_bytes < need) {
    set_error("tensor_hist: scratch_bytes=%zu below the %zu bytes that T=%d, n_chunks=%lld need", scratch_bytes, need, T, n_chunks);
    return MMVAE_ERR_WORKSPACE;
  }
  if ((reinterpret_cast<uintptr_t>(scratch) & 7u) || (reinterpret_cast<uintptr_t>(flat) & 3u)) {
    set_error("tensor_hist: scratch must be 8-byte aligned, flat 4-byte aligned");
    return MMVAE_ERR_ARG;
  }
  double* part = static_cast<double*>(scratch);
  if (n_chunks > 0) {
    hipLaunchKernelGGL(hist_stats_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, s, flat, seg_dev, chunk_dev, part);
    const int e = check_launch("tensor_hist (stats)");
    if (e != MMVAE_OK) return e;
  }
  hipLaunchKernelGGL(hist_finalize_kernel, dim3((unsigned)T), dim3(kWave), 0, s, chunk_dev, n_chunks, part, counts, lo, hi, stats);
  const int e = check_launch("tensor_hist (finalize)");
  if (e != MMVAE_OK || n_chunks == 0) return e;
  hipLaunchKernelGGL(hist_bins_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, s, flat, seg_dev, chunk_dev, lo, hi, counts);
  return check_launch("tensor_hist (bins)");
}

}  // namespace mmvae
