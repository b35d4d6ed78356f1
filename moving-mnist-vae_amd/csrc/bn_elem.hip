// Train-mode BatchNorm pieces and the residual joins, as bandwidth kernels (16-byte NHWC vectors).
//
// Forward BN-apply(+ReLU) is normally fused into the consumer conv's load prologue (conv_gemm.hip);
// what is here: per-channel statistics, the finalize step (scale/shift, running stats), the two-input
// residual join, and the backward reductions / dy materialisation  dy = A*g + B*y + C  per channel.
#include "kernels.hpp"
#include "tile_common.hpp"
#include <cstdlib>

namespace mmvae {

__host__ __device__ inline int block_threads_for(int cvecs) {
  // a block size that is a multiple of cvecs, so a thread's channel group never changes in a grid-stride loop
  int b = 256 - (256 % cvecs);
  return b < cvecs ? cvecs : b;
}

static int elem_blocks(long nvec, int threads) {
  constexpr int cap = kElemMaxBlocks;
  long b = (nvec + (long)threads * 4 - 1) / ((long)threads * 4);
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}

// ---------------------------------------------------------------- channel statistics (NHWC)
template <typename T>
__global__ void chan_stats_nhwc_kernel(const T* __restrict__ y, long nvec, int C, float* __restrict__ partials) {
  constexpr int VE = Elem<T>::kVec;
  extern __shared__ float smem[];
  const int cvecs = C / VE;
  float acc[2][VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) { acc[0][j] = 0.f; acc[1][j] = 0.f; }
  const long stride = (long)gridDim.x * blockDim.x;
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
    float f[VE];
    Elem<T>::unpack(reinterpret_cast<const Vec16*>(y)[v], f);
#pragma unroll
    for (int j = 0; j < VE; ++j) { acc[0][j] += f[j]; acc[1][j] += f[j] * f[j]; }
  }
  block_channel_reduce<2, VE>(acc, cvecs, C, smem, partials + (long)blockIdx.x * 2 * C);
}

int chan_stats_parts(long, int) { return 1024; }   // upper bound on partial rows of every reduction kernel

int launch_chan_stats_nhwc(int dt, const void* y, long npix, int C, float* partials, hipStream_t s) {
  const int VE = dt == DT_F32 ? 4 : 8;
  if (C % VE) { set_error("chan_stats: C=%d not a multiple of %d", C, VE); return MMVAE_ERR_UNSUPPORTED; }
  const int cvecs = C / VE, threads = block_threads_for(cvecs);
  const long nvec = npix * cvecs;
  int blocks = elem_blocks(nvec, threads);
  if (blocks > 1024) blocks = 1024;
  const size_t sm = (size_t)threads * 2 * VE * sizeof(float);
  if (dt == DT_F32) hipLaunchKernelGGL((chan_stats_nhwc_kernel<float>), dim3(blocks), dim3(threads), sm, s, (const float*)y, nvec, C, partials);
  else hipLaunchKernelGGL((chan_stats_nhwc_kernel<bf16_t>), dim3(blocks), dim3(threads), sm, s, (const bf16_t*)y, nvec, C, partials);
  int rc = check_launch("chan_stats_nhwc");
  return rc ? rc : blocks;
}

// ---------------------------------------------------------------- channel statistics (NCHW f32)
// planes = N*C; block handles planes blockIdx.x, +gridDim.x, ...; partials [gridDim.x][NR][C]
template <int NR>
__global__ __launch_bounds__(256) void plane_reduce_nchw_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, int C, int HW,
                                                                 float* __restrict__ partials) {
  // NR=2, b==null: (sum a, sum a^2);  NR=2, b!=null: (sum a, sum a*b).  No barrier per plane: every wave reduces its
  // share of a plane into its OWN per-channel LDS accumulators (single writer, fixed order -> bit-reproducible sums);
  // the four waves are combined once at the end.
  extern __shared__ float sm[];
  float* sAcc = sm;             // [4 waves][NR][C]
  const int wid = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 4 * NR * C; i += blockDim.x) sAcc[i] = 0.f;
  __syncthreads();
  const int planes = N * C;
  for (int p = blockIdx.x; p < planes; p += gridDim.x) {
    const int c = p % C;
    const float* pa = a + (long)p * HW;
    const float* pb = b ? b + (long)p * HW : nullptr;
    float v0 = 0.f, v1 = 0.f;
    if ((HW & 3) == 0) {
      for (int i = threadIdx.x * 4; i < HW; i += 4 * blockDim.x) {
        const float4 x = *reinterpret_cast<const float4*>(pa + i);
        float4 y = x;
        if (pb) y = *reinterpret_cast<const float4*>(pb + i);
        v0 += (x.x + x.y) + (x.z + x.w);
        v1 += (x.x * y.x + x.y * y.y) + (x.z * y.z + x.w * y.w);
      }
    } else {
      for (int i = threadIdx.x; i < HW; i += blockDim.x) {
        const float x = pa[i];
        v0 += x;
        v1 += pb ? x * pb[i] : x * x;
      }
    }
    v0 = wave_sum(v0); v1 = wave_sum(v1);
    if ((threadIdx.x & 63) == 0) { sAcc[wid * NR * C + c] += v0; sAcc[wid * NR * C + C + c] += v1; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NR * C; i += blockDim.x)
    partials[(long)blockIdx.x * NR * C + i] = (sAcc[i] + sAcc[NR * C + i]) + (sAcc[2 * NR * C + i] + sAcc[3 * NR * C + i]);
}

static int nchw_parts(int N, int C) { int p = N * C; return p > 1024 ? 1024 : (p < 1 ? 1 : p); }


int launch_bn_bwd_reduce_nchw(const float* dout, const float* y, int N, int C, int HW, float* partials, hipStream_t s) {
  const int blocks = nchw_parts(N, C);
  const size_t sm = (size_t)4 * 2 * C * sizeof(float);
  hipLaunchKernelGGL((plane_reduce_nchw_kernel<2>), dim3(blocks), dim3(256), sm, s, dout, y, N, C, HW, partials);
  int rc = check_launch("bn_bwd_reduce_nchw");
  return rc ? rc : blocks;
}

// ---------------------------------------------------------------- SyncBN: partial rows -> one row (the all-reduce operand)
// partials [nparts][rows][C] -> out [rows * C]: the finalize kernels take the summed row as a single partial row afterwards.
__global__ __launch_bounds__(256) void partial_rowsum_kernel(const float* __restrict__ partials, int nparts, int stride, float* __restrict__ out) {
  __shared__ double sRed[4];
  const int col = blockIdx.x;
  double s = 0.0;
  for (int p = threadIdx.x; p < nparts; p += 256) s += (double)partials[(long)p * stride + col];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[col] = (float)((sRed[0] + sRed[1]) + (sRed[2] + sRed[3]));
}
int launch_partial_rowsum(const float* partials, int nparts, int width, float* out, hipStream_t s, int row_stride) {
  hipLaunchKernelGGL(partial_rowsum_kernel, dim3(width), dim3(256), 0, s, partials, nparts, row_stride > 0 ? row_stride : width, out);
  return check_launch("partial_rowsum");
}

// ---------------------------------------------------------------- finalize (training)
// Two strided column sums over per-block partial rows (finalize kernels: one block per channel).  The loads of U rows are issued before the
// first add, so a block pays nparts / (U * blockDim) memory latencies instead of nparts / blockDim -- these launches sit between the big
// kernels of the critical stream.  Fixed order per thread -> bit-reproducible.
template <int U>
__device__ __forceinline__ void strided_pair_sum(const float* __restrict__ pa, const float* __restrict__ pb, long stride, int nparts, double& s0, double& s1) {
  const int bd = blockDim.x;
  int p = threadIdx.x;
  for (; p + (U - 1) * bd < nparts; p += U * bd) {
    float va[U], vb[U];
#pragma unroll
    for (int k = 0; k < U; ++k) { va[k] = pa[(long)(p + k * bd) * stride]; vb[k] = pb[(long)(p + k * bd) * stride]; }
#pragma unroll
    for (int k = 0; k < U; ++k) { s0 += (double)va[k]; s1 += (double)vb[k]; }
  }
  for (; p < nparts; p += bd) { s0 += (double)pa[(long)p * stride]; s1 += (double)pb[(long)p * stride]; }
}

__global__ void bn_finalize_kernel(BnFinalizeArgs a) {
  __shared__ double sRed[2 * 4];
  const int c = blockIdx.x;
  double s1 = 0.0, s2 = 0.0;
  strided_pair_sum<8>(a.partials + c, a.partials + a.C + c, 2L * a.C, a.nparts, s1, s2);
  s1 = wave_sum_d(s1); s2 = wave_sum_d(s2);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { sRed[wid] = s1; sRed[4 + wid] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = blockDim.x >> 6;
    s1 = 0.0; s2 = 0.0;
    for (int w = 0; w < nw; ++w) { s1 += sRed[w]; s2 += sRed[4 + w]; }
    const double n = a.count;
    const double mean = s1 / n;
    double var = s2 / n - mean * mean;
    if (var < 0.0) var = 0.0;
    const double isc = (double)a.in_scale;
    const double istd = 1.0 / sqrt(var + (double)a.eps * isc * isc);
    const float g = a.gamma ? a.gamma[c] : 1.f, b = a.beta ? a.beta[c] : 0.f;
    a.mean[c] = (float)mean;
    a.istd[c] = (float)istd;
    const float sc = (float)((double)g * istd);
    a.scale[c] = sc;
    a.shift[c] = (float)((double)b - mean * (double)g * istd);
    if (a.running_mean) {
      const double unbiased = (n > 1.0 ? var * n / (n - 1.0) : var) / (isc * isc);
      a.running_mean[c] = (float)((1.0 - (double)a.momentum) * (double)a.running_mean[c] + (double)a.momentum * mean / isc);
      a.running_var[c] = (float)((1.0 - (double)a.momentum) * (double)a.running_var[c] + (double)a.momentum * unbiased);
    }
    if (c == 0 && a.nbt) *a.nbt += 1;
  }
}

int launch_bn_finalize(const BnFinalizeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(a.C), dim3(256), 0, s, a);
  return check_launch("bn_finalize");
}

// Inference (model.eval(), reference model.py:353-362): every BatchNorm of an entry point folded into its per-channel (scale, shift) pair from the
// running statistics in ONE launch -- the consumers' prologues apply them, no statistics, no per-layer finalize.
__global__ void bn_fold_eval_kernel(BnFoldTable t, const float* __restrict__ params, const float* __restrict__ bnbuf, float* __restrict__ bnws, float eps) {
  const BnFoldEntry e = t.e[blockIdx.x];
  for (int c = threadIdx.x; c < e.C; c += blockDim.x) {
    const float istd = 1.0f / sqrtf(bnbuf[e.rv_off + c] + eps);
    const float sc = params[e.g_off + c] * istd;
    bnws[e.scale_off + c] = sc / e.in_scale;              // the conv output in memory is in_scale * y (fp8 weight scale)
    bnws[e.shift_off + c] = params[e.b_off + c] - bnbuf[e.rm_off + c] * sc;
  }
}
int launch_bn_fold_eval(const BnFoldEntry* entries, int n, const float* params, const float* bnbuf, float* bnws, float eps, hipStream_t s) {
  for (int i = 0; i < n; i += kBnFoldMax) {
    BnFoldTable t;
    const int m = n - i < kBnFoldMax ? n - i : kBnFoldMax;
    for (int j = 0; j < m; ++j) t.e[j] = entries[i + j];
    hipLaunchKernelGGL(bn_fold_eval_kernel, dim3(m), dim3(256), 0, s, t, params, bnbuf, bnws, eps);
  }
  return check_launch("bn_fold_eval");
}

// ---------------------------------------------------------------- forward elementwise
template <typename T, bool TWO>
__global__ void affine_join_kernel(const T* __restrict__ a, const float* __restrict__ sa, const float* __restrict__ ba,
                                   const T* __restrict__ b, const float* __restrict__ sb, const float* __restrict__ bb,
                                   int relu, T* __restrict__ out, long nvec, int C) {
  constexpr int VE = Elem<T>::kVec;
  const int cvecs = C / VE;
  const long stride = (long)gridDim.x * blockDim.x;
  const int cg = (int)(((long)blockIdx.x * blockDim.x + threadIdx.x) % cvecs);   // constant: blockDim % cvecs == 0
  float s0[VE], b0[VE], s1[VE], b1[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) {
    s0[j] = sa[cg * VE + j]; b0[j] = ba[cg * VE + j];
    s1[j] = TWO ? sb[cg * VE + j] : 0.f; b1[j] = TWO ? bb[cg * VE + j] : 0.f;
  }
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
    float fa[VE], fb[VE];
    Elem<T>::unpack(reinterpret_cast<const Vec16*>(a)[v], fa);
    if (TWO) Elem<T>::unpack(reinterpret_cast<const Vec16*>(b)[v], fb);
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      float x = fa[j] * s0[j] + b0[j];
      if (TWO) x += fb[j] * s1[j] + b1[j];
      fa[j] = relu ? fmaxf(x, 0.f) : x;
    }
    reinterpret_cast<Vec16*>(out)[v] = Elem<T>::pack(fa);
  }
}

template <typename T>
static int launch_affine_join_t(const BnSide& a, const BnSide& b, int relu, void* out, long npix, int C, hipStream_t s) {
  constexpr int VE = Elem<T>::kVec;
  if (C % VE) { set_error("affine/join: C=%d not a multiple of %d", C, VE); return MMVAE_ERR_UNSUPPORTED; }
  const int cvecs = C / VE, threads = block_threads_for(cvecs);
  const long nvec = npix * cvecs;
  const int blocks = elem_blocks(nvec, threads);
#define MMVAE_LAUNCH(TWO) hipLaunchKernelGGL((affine_join_kernel<T, TWO>), dim3(blocks), dim3(threads), 0, s, (const T*)a.y, a.fwd.scale, a.fwd.shift, \
    (const T*)b.y, b.fwd.scale, b.fwd.shift, relu, (T*)out, nvec, C)
  if (b.y) MMVAE_LAUNCH(true); else MMVAE_LAUNCH(false);
#undef MMVAE_LAUNCH
  note_launch_bytes((double)npix * C * sizeof(T) * (b.y ? 3 : 2));
  return check_launch("affine_join");
}

int launch_join_fwd(int dt, const BnSide& a, const BnSide& b, void* out, long npix, int C, hipStream_t s) {
  return dt == DT_F32 ? launch_affine_join_t<float>(a, b, 1, out, npix, C, s) : launch_affine_join_t<bf16_t>(a, b, 1, out, npix, C, s);
}
int launch_affine_act(int dt, const BnSide& a, int relu, void* out, long npix, int C, hipStream_t s) {
  return dt == DT_F32 ? launch_affine_join_t<float>(a, BnSide{}, relu, out, npix, C, s) : launch_affine_join_t<bf16_t>(a, BnSide{}, relu, out, npix, C, s);
}

// ---------------------------------------------------------------- backward reductions
// MODE 0: mask from out>0 ; MODE 1: mask from y0*ms+mb>0 ; MODE 2: no mask ;
// MODE 3: mask from (y0*ms+mb) + (y1*ms1+mb1) > 0  (the residual join recomputed -> `out` is not read at all)
static int bn_bwd_mask_mode(const void* out, const BnSide& a, const BnSide& b) {
  return out ? 0 : (a.fwd.scale ? ((b.fwd.scale && b.y) ? 3 : 1) : 2);
}
template <typename T, int NY, int MODE>
__global__ void bn_bwd_reduce_kernel(const T* __restrict__ dout, const T* __restrict__ out, const float* __restrict__ ms,
                                     const float* __restrict__ mb, const float* __restrict__ ms1, const float* __restrict__ mb1,
                                     const T* __restrict__ y0, const T* __restrict__ y1,
                                     long nvec, int C, float* __restrict__ partials) {
  constexpr int VE = Elem<T>::kVec;
  extern __shared__ float smem[];
  const int cvecs = C / VE;
  const int cg = (int)(((long)blockIdx.x * blockDim.x + threadIdx.x) % cvecs);
  float msc[VE], msh[VE], msc1[VE], msh1[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) {
    msc[j] = (MODE == 1 || MODE == 3) ? ms[cg * VE + j] : 0.f; msh[j] = (MODE == 1 || MODE == 3) ? mb[cg * VE + j] : 0.f;
    msc1[j] = MODE == 3 ? ms1[cg * VE + j] : 0.f; msh1[j] = MODE == 3 ? mb1[cg * VE + j] : 0.f;
  }
  float acc[1 + NY][VE];
#pragma unroll
  for (int q = 0; q < 1 + NY; ++q)
#pragma unroll
    for (int j = 0; j < VE; ++j) acc[q][j] = 0.f;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
    float g[VE], o[VE], a0[VE], a1[VE];
    Elem<T>::unpack(reinterpret_cast<const Vec16*>(dout)[v], g);
    Elem<T>::unpack(reinterpret_cast<const Vec16*>(y0)[v], a0);
    if (MODE == 0) Elem<T>::unpack(reinterpret_cast<const Vec16*>(out)[v], o);
    if (NY == 2) Elem<T>::unpack(reinterpret_cast<const Vec16*>(y1)[v], a1);
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      bool on = true;
      if (MODE == 0) on = o[j] > 0.f;
      if (MODE == 1) on = (a0[j] * msc[j] + msh[j]) > 0.f;
      if (MODE == 3) { float x = a0[j] * msc[j] + msh[j]; x += a1[j] * msc1[j] + msh1[j]; on = x > 0.f; }
      const float gg = on ? g[j] : 0.f;
      acc[0][j] += gg;
      acc[1][j] += gg * a0[j];
      if (NY == 2) acc[2][j] += gg * a1[j];
    }
  }
  block_channel_reduce<1 + NY, VE>(acc, cvecs, C, smem, partials + (long)blockIdx.x * (1 + NY) * C);
}

template <typename T>
static int launch_bn_bwd_reduce_t(const void* dout, const void* out, const BnSide& a, const BnSide& b, float* partials, long npix, int C,
                                  hipStream_t s) {
  constexpr int VE = Elem<T>::kVec;
  if (C % VE) { set_error("bn_bwd_reduce: C=%d not a multiple of %d", C, VE); return MMVAE_ERR_UNSUPPORTED; }
  const int cvecs = C / VE, threads = block_threads_for(cvecs);
  const long nvec = npix * cvecs;
  int blocks = elem_blocks(nvec, threads);
  if (blocks > 1024) blocks = 1024;
  const int ny = b.y ? 2 : 1;
  const size_t sm = (size_t)threads * (1 + ny) * VE * sizeof(float);
  const int mode = bn_bwd_mask_mode(out, a, b);
#define MMVAE_LAUNCH(NY, MODE) hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, NY, MODE>), dim3(blocks), dim3(threads), sm, s, \
    (const T*)dout, (const T*)out, a.fwd.scale, a.fwd.shift, b.fwd.scale, b.fwd.shift, (const T*)a.y, (const T*)b.y, nvec, C, partials)
  if (ny == 2) { if (mode == 0) MMVAE_LAUNCH(2, 0); else if (mode == 1) MMVAE_LAUNCH(2, 1); else if (mode == 3) MMVAE_LAUNCH(2, 3); else MMVAE_LAUNCH(2, 2); }
  else { if (mode == 0) MMVAE_LAUNCH(1, 0); else if (mode == 1) MMVAE_LAUNCH(1, 1); else MMVAE_LAUNCH(1, 2); }
#undef MMVAE_LAUNCH
  note_launch_bytes((double)npix * C * sizeof(T) * (1 + ny + (out ? 1 : 0)));
  int rc = check_launch("bn_bwd_reduce");
  return rc ? rc : blocks;
}
int launch_bn_bwd_reduce(int dt, const void* dout, const void* out, const BnSide& a, const BnSide& b, float* partials, long npix, int C,
                         hipStream_t s) {
  return dt == DT_F32 ? launch_bn_bwd_reduce_t<float>(dout, out, a, b, partials, npix, C, s)
                      : launch_bn_bwd_reduce_t<bf16_t>(dout, out, a, b, partials, npix, C, s);
}

// blockIdx.y selects the BatchNorm: the two branches of a residual join (same partials, which = 0 / 1) finalise in one launch
__global__ void bn_bwd_finalize_kernel(BnBwdFinalizeArgs a0, BnBwdFinalizeArgs a1) {
  const BnBwdFinalizeArgs& a = blockIdx.y ? a1 : a0;
  __shared__ double sRed[2 * 4];
  const int c = blockIdx.x;
  const int rows = 1 + a.ny;
  double s0 = 0.0, s1 = 0.0;
  strided_pair_sum<8>(a.partials + c, a.partials + (long)(1 + a.which) * a.C + c, (long)rows * a.C, a.nparts, s0, s1);
  s0 = wave_sum_d(s0); s1 = wave_sum_d(s1);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { sRed[wid] = s0; sRed[4 + wid] = s1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = blockDim.x >> 6;
    s0 = 0.0; s1 = 0.0;
    for (int w = 0; w < nw; ++w) { s0 += sRed[w]; s1 += sRed[4 + w]; }
    const double mean = a.mean[c], istd = a.istd[c], g = a.gamma ? a.gamma[c] : 1.0;
    const double sgy = istd * (s1 - mean * s0);       // sum g * yhat
    if (a.dgamma) a.dgamma[c] += (float)sgy;
    if (a.dbeta) a.dbeta[c] += (float)s0;
    const double m1 = s0 / a.count, m2 = sgy / a.count;
    const double A = g * istd;
    const float Af = (float)A, Bf = (float)(-A * m2 * istd), Cf = (float)(-A * m1 + A * m2 * istd * mean);
    a.coefA[c] = Af;
    a.coefB[c] = Bf;
    a.coefC[c] = Cf;
    if (a.dbias_conv) a.dbias_conv[c] += (float)(((double)Af * s0 + (double)Bf * (mean * a.count) + (double)Cf * a.count) * (double)a.dbias_scale);
  }
}
int launch_bn_bwd_finalize(const BnBwdFinalizeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(a.C), dim3(256), 0, s, a, a);
  return check_launch("bn_bwd_finalize");
}
int launch_bn_bwd_finalize2(const BnBwdFinalizeArgs& a0, const BnBwdFinalizeArgs& a1, hipStream_t s) {
  if (a0.C != a1.C) { set_error("bn_bwd_finalize2: channel counts differ"); return MMVAE_ERR_ARG; }
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(a0.C, 2), dim3(256), 0, s, a0, a1);
  return check_launch("bn_bwd_finalize2");
}

template <typename T, int NY, int MODE>
__global__ void bn_bwd_apply_kernel(const T* __restrict__ dout, const T* __restrict__ out, const float* __restrict__ ms,
                                    const float* __restrict__ mb, const float* __restrict__ ms1, const float* __restrict__ mb1,
                                    const T* __restrict__ y0, const float* __restrict__ A0,
                                    const float* __restrict__ B0, const float* __restrict__ C0, T* __restrict__ dy0,
                                    const T* __restrict__ y1, const float* __restrict__ A1, const float* __restrict__ B1,
                                    const float* __restrict__ C1, T* __restrict__ dy1, long nvec, int C) {
  constexpr int VE = Elem<T>::kVec;
  const int cvecs = C / VE;
  const int cg = (int)(((long)blockIdx.x * blockDim.x + threadIdx.x) % cvecs);
  float msc[VE], msh[VE], msc1[VE], msh1[VE], a0[VE], b0[VE], c0[VE], a1[VE], b1[VE], c1[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) {
    const int ch = cg * VE + j;
    msc[j] = (MODE == 1 || MODE == 3) ? ms[ch] : 0.f; msh[j] = (MODE == 1 || MODE == 3) ? mb[ch] : 0.f;
    msc1[j] = MODE == 3 ? ms1[ch] : 0.f; msh1[j] = MODE == 3 ? mb1[ch] : 0.f;
    a0[j] = A0[ch]; b0[j] = B0[ch]; c0[j] = C0[ch];
    a1[j] = NY == 2 ? A1[ch] : 0.f; b1[j] = NY == 2 ? B1[ch] : 0.f; c1[j] = NY == 2 ? C1[ch] : 0.f;
  }
  const long stride = (long)gridDim.x * blockDim.x;
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
    float g[VE], o[VE], f0[VE], f1[VE], r0[VE], r1[VE];
    Elem<T>::unpack(reinterpret_cast<const Vec16*>(dout)[v], g);
    Elem<T>::unpack(reinterpret_cast<const Vec16*>(y0)[v], f0);
    if (MODE == 0) Elem<T>::unpack(reinterpret_cast<const Vec16*>(out)[v], o);
    if (NY == 2) Elem<T>::unpack(reinterpret_cast<const Vec16*>(y1)[v], f1);
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      bool on = true;
      if (MODE == 0) on = o[j] > 0.f;
      if (MODE == 1) on = (f0[j] * msc[j] + msh[j]) > 0.f;
      if (MODE == 3) { float x = f0[j] * msc[j] + msh[j]; x += f1[j] * msc1[j] + msh1[j]; on = x > 0.f; }
      const float gg = on ? g[j] : 0.f;
      r0[j] = a0[j] * gg + b0[j] * f0[j] + c0[j];
      if (NY == 2) r1[j] = a1[j] * gg + b1[j] * f1[j] + c1[j];
    }
    reinterpret_cast<Vec16*>(dy0)[v] = Elem<T>::pack(r0);
    if (NY == 2) reinterpret_cast<Vec16*>(dy1)[v] = Elem<T>::pack(r1);
  }
}

template <typename T>
static int launch_bn_bwd_apply_t(const void* dout, const void* out, const BnSide& a, const BnSide& b, void* dy0, void* dy1, long npix, int C,
                                 hipStream_t s) {
  constexpr int VE = Elem<T>::kVec;
  if (C % VE) { set_error("bn_bwd_apply: C=%d not a multiple of %d", C, VE); return MMVAE_ERR_UNSUPPORTED; }
  const int cvecs = C / VE, threads = block_threads_for(cvecs);
  const long nvec = npix * cvecs;
  const int blocks = elem_blocks(nvec, threads);
  const int ny = b.y ? 2 : 1;
  const int mode = bn_bwd_mask_mode(out, a, b);
#define MMVAE_LAUNCH(NY, MODE) hipLaunchKernelGGL((bn_bwd_apply_kernel<T, NY, MODE>), dim3(blocks), dim3(threads), 0, s, \
    (const T*)dout, (const T*)out, a.fwd.scale, a.fwd.shift, b.fwd.scale, b.fwd.shift, (const T*)a.y, a.bwd.A, a.bwd.B, a.bwd.C, (T*)dy0, \
    (const T*)b.y, b.bwd.A, b.bwd.B, b.bwd.C, (T*)dy1, nvec, C)
  if (ny == 2) { if (mode == 0) MMVAE_LAUNCH(2, 0); else if (mode == 1) MMVAE_LAUNCH(2, 1); else if (mode == 3) MMVAE_LAUNCH(2, 3); else MMVAE_LAUNCH(2, 2); }
  else { if (mode == 0) MMVAE_LAUNCH(1, 0); else if (mode == 1) MMVAE_LAUNCH(1, 1); else MMVAE_LAUNCH(1, 2); }
#undef MMVAE_LAUNCH
  note_launch_bytes((double)npix * C * sizeof(T) * (1 + 2 * ny + (out ? 1 : 0)));
  return check_launch("bn_bwd_apply");
}
int launch_bn_bwd_apply(int dt, const void* dout, const void* out, const BnSide& a, const BnSide& b, void* dy0, void* dy1, long npix, int C,
                        hipStream_t s) {
  return dt == DT_F32 ? launch_bn_bwd_apply_t<float>(dout, out, a, b, dy0, dy1, npix, C, s)
                      : launch_bn_bwd_apply_t<bf16_t>(dout, out, a, b, dy0, dy1, npix, C, s);
}

// ---------------------------------------------------------------- NCHW f32 elementwise (output BN)
__global__ void affine_nchw_kernel(const float* __restrict__ raw, const float* __restrict__ scale, const float* __restrict__ shift,
                                   float* __restrict__ out, long total, int C, int HW) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)((i / HW) % C);
    out[i] = raw[i] * scale[c] + shift[c];
  }
}
int launch_affine_nchw(const float* raw, Affine bn, float* out, int N, int C, int HW, hipStream_t s) {
  const long total = (long)N * C * HW;
  const int blocks = elem_blocks(total / 4 + 1, 256);
  hipLaunchKernelGGL(affine_nchw_kernel, dim3(blocks), dim3(256), 0, s, raw, bn.scale, bn.shift, out, total, C, HW);
  note_launch_bytes((double)total * 8.0);
  return check_launch("affine_nchw");
}
// ---- Gaussian reconstruction loss fused into the output BatchNorm's backward (reference model.py:193, :403): the loss gradient
//   d[n,c,i] = k * (scale[c] * raw[n,c,i] + shift[c] - target[n,c,i]),  k = coef / sigma^2 (* the upstream gradient, a device scalar)
// is a function of the conv output `raw` and the target alone, so neither d_recon nor a second read of recon is needed: the reduce pass
// sums (d, d * raw) per channel straight from raw and target, the apply pass writes d_raw = A d + B raw + C.  Two passes over the plane
// (2 reads each, 1 write) instead of gauss_nll_bwd + plane_reduce + apply (6 reads, 2 writes).  Same block / summation structure as
// plane_reduce_nchw_kernel (bit-reproducible).
__global__ __launch_bounds__(256) void gauss_tail_reduce_kernel(const float* __restrict__ raw, const float* __restrict__ tgt, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, float k, const float* __restrict__ gs, int N, int C,
                                                                 int HW, float* __restrict__ partials) {
  extern __shared__ float sm[];
  float* sAcc = sm;             // [4 waves][2][C]
  const int wid = threadIdx.x >> 6;
  if (gs) k *= gs[0];
  for (int i = threadIdx.x; i < 4 * 2 * C; i += blockDim.x) sAcc[i] = 0.f;
  __syncthreads();
  const int planes = N * C;
  for (int p = blockIdx.x; p < planes; p += gridDim.x) {
    const int c = p % C;
    const float sc = scale[c], sh = shift[c];
    const float* pa = raw + (long)p * HW;
    const float* pt = tgt + (long)p * HW;
    float v0 = 0.f, v1 = 0.f;
    if ((HW & 3) == 0) {
      for (int i = threadIdx.x * 4; i < HW; i += 4 * blockDim.x) {
        const float4 x = *reinterpret_cast<const float4*>(pa + i);
        const float4 t = *reinterpret_cast<const float4*>(pt + i);
        const float d0 = k * ((sc * x.x + sh) - t.x), d1 = k * ((sc * x.y + sh) - t.y), d2 = k * ((sc * x.z + sh) - t.z), d3 = k * ((sc * x.w + sh) - t.w);
        v0 += (d0 + d1) + (d2 + d3);
        v1 += (d0 * x.x + d1 * x.y) + (d2 * x.z + d3 * x.w);
      }
    } else {
      for (int i = threadIdx.x; i < HW; i += blockDim.x) {
        const float x = pa[i], d = k * ((sc * x + sh) - pt[i]);
        v0 += d; v1 += d * x;
      }
    }
    v0 = wave_sum(v0); v1 = wave_sum(v1);
    if ((threadIdx.x & 63) == 0) { sAcc[wid * 2 * C + c] += v0; sAcc[wid * 2 * C + C + c] += v1; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x)
    partials[(long)blockIdx.x * 2 * C + i] = (sAcc[i] + sAcc[2 * C + i]) + (sAcc[2 * 2 * C + i] + sAcc[3 * 2 * C + i]);
}
int launch_gauss_tail_reduce(const float* raw, Affine bn, const float* target, float sigma, float coef, const float* gscale, float* partials, int N,
                             int C, int HW, hipStream_t s) {
  const int blocks = nchw_parts(N, C);
  const size_t sm = (size_t)4 * 2 * C * sizeof(float);
  hipLaunchKernelGGL(gauss_tail_reduce_kernel, dim3(blocks), dim3(256), sm, s, raw, target, bn.scale, bn.shift, coef / (sigma * sigma), gscale, N, C, HW, partials);
  note_launch_bytes((double)N * C * HW * 8.0);
  const int rc = check_launch("gauss_tail_reduce");
  return rc ? rc : blocks;
}
__global__ __launch_bounds__(256) void gauss_tail_apply_kernel(const float* __restrict__ raw, const float* __restrict__ tgt, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, float k, const float* __restrict__ gs,
                                                                const float* __restrict__ A, const float* __restrict__ B, const float* __restrict__ Cc,
                                                                float* __restrict__ dy, int planes, int C, int HW) {
  if (gs) k *= gs[0];
  for (int p = blockIdx.x; p < planes; p += gridDim.x) {
    const int c = p % C;
    const float sc = scale[c], sh = shift[c], ca = A[c], cb = B[c], cc = Cc[c];
    const long base = (long)p * HW;
    if ((HW & 3) == 0) {
      for (int i = threadIdx.x * 4; i < HW; i += 1024) {
        const float4 x = *reinterpret_cast<const float4*>(raw + base + i);
        const float4 t = *reinterpret_cast<const float4*>(tgt + base + i);
        float4 o;
        o.x = ca * (k * ((sc * x.x + sh) - t.x)) + cb * x.x + cc; o.y = ca * (k * ((sc * x.y + sh) - t.y)) + cb * x.y + cc;
        o.z = ca * (k * ((sc * x.z + sh) - t.z)) + cb * x.z + cc; o.w = ca * (k * ((sc * x.w + sh) - t.w)) + cb * x.w + cc;
        *reinterpret_cast<float4*>(dy + base + i) = o;
      }
    } else {
      for (int i = threadIdx.x; i < HW; i += 256) {
        const float x = raw[base + i];
        dy[base + i] = ca * (k * ((sc * x + sh) - tgt[base + i])) + cb * x + cc;
      }
    }
  }
}
int launch_gauss_tail_apply(const float* raw, Affine bn, BnCoef k, const float* target, float sigma, float coef, const float* gscale, float* dy, int N,
                            int C, int HW, hipStream_t s) {
  if (C > 64) { set_error("gauss_tail_apply: C=%d > 64", C); return MMVAE_ERR_UNSUPPORTED; }
  const int planes = N * C;
  const int blocks = planes < 4096 ? planes : 4096;
  hipLaunchKernelGGL(gauss_tail_apply_kernel, dim3(blocks), dim3(256), 0, s, raw, target, bn.scale, bn.shift, coef / (sigma * sigma), gscale, k.A, k.B, k.C, dy, planes, C, HW);
  note_launch_bytes((double)N * C * HW * 12.0);
  return check_launch("gauss_tail_apply");
}

// dy = A[c]*dout + B[c]*y + C[c] on NCHW f32 planes.  Block = whole planes (n, c).
__global__ __launch_bounds__(256) void bn_bwd_apply_nchw_kernel(const float* __restrict__ dout, const float* __restrict__ y,
                                                                const float* __restrict__ A, const float* __restrict__ B,
                                                                const float* __restrict__ Cc, float* __restrict__ dy, int planes, int C,
                                                                int HW) {
  for (int p = blockIdx.x; p < planes; p += gridDim.x) {
    const int c = p % C;
    const float ca = A[c], cb = B[c], cc = Cc[c];
    const long base = (long)p * HW;
    if ((HW & 3) == 0) {
      for (int i = threadIdx.x * 4; i < HW; i += 1024) {
        const float4 d = *reinterpret_cast<const float4*>(dout + base + i);
        const float4 v = *reinterpret_cast<const float4*>(y + base + i);
        float4 o;
        o.x = ca * d.x + cb * v.x + cc; o.y = ca * d.y + cb * v.y + cc; o.z = ca * d.z + cb * v.z + cc; o.w = ca * d.w + cb * v.w + cc;
        *reinterpret_cast<float4*>(dy + base + i) = o;
      }
    } else {
      for (int i = threadIdx.x; i < HW; i += 256) dy[base + i] = ca * dout[base + i] + cb * y[base + i] + cc;
    }
  }
}
int launch_bn_bwd_apply_nchw(const float* dout, const float* y, BnCoef k, float* dy, int N, int C, int HW, hipStream_t s) {
  if (C > 64) { set_error("bn_bwd_apply_nchw: C=%d > 64", C); return MMVAE_ERR_UNSUPPORTED; }
  const int planes = N * C;
  const int blocks = planes < 4096 ? planes : 4096;
  hipLaunchKernelGGL(bn_bwd_apply_nchw_kernel, dim3(blocks), dim3(256), 0, s, dout, y, k.A, k.B, k.C, dy, planes, C, HW);
  return check_launch("bn_bwd_apply_nchw");
}

}  // namespace mmvae
