// Gradient of the aggregate-posterior densities (posterior_mixture.hip) with respect to the samples and the bank.  In that file's notation,
// with the saved outputs as normalisers and upstream gradients g_joint[i], g_dims[i][d]:
//   r_ij   = exp(s_ij  - (log_qz[i]         + log M)),      rd_ijd = exp(t_ijd - (log_qz_dims[i][d] + log M)),
//   a_ijd  = g_joint[i] r_ij + g_dims[i][d] rd_ijd,         u_ijd  = (z_id - mu_jd) exp(-logvar_jd),
//   d_z[i][d] = -sum_j a u,   d_mu[j][d] = sum_i a u,   d_logvar[j][d] = sum_i a 0.5 ((z_id - mu_jd) u - 1).
// d_z is a sum over the bank for every sample, d_mu / d_logvar are sums over the samples for every bank row: two pair sweeps with the
// roles swapped, so that each sum stays in one lane's registers and nothing is added across lanes.
//
// Dataflow (all on the caller's stream):
//   pmb_bank_prep    the bank in the base-2 domain, by the forward's formulas (w = -0.5 log2(e) exp(-logvar), c = -0.5 log2(e) (logvar +
//                    log 2 pi), formed in f64, rounded once; C[j] = sum_d c_jd in f64), twice: T[g][dd][{mu, w, c}][8 rows], the forward's
//                    layout that a sweep stages through LDS, and row-major R{mu, w, c}[row][dd] padded to 256 rows for the sweep that keeps
//                    a bank row per lane.  Pad rows: w = 0, c = C = -inf (their weights are exp2(-inf) = 0); pad dimensions: zeros.
//   pmb_sample_prep  the samples likewise: Z, LD, GD [row][dd] padded to 256 rows (z, the per-dimension normaliser (log_qz_dims + log M)
//                    log2(e) and g_dims as f32) and S[g][dd][{z, ld, gd}][8 samples]; L2[i] = (log_qz[i] + log M) log2(e) in f64 and
//                    GJ[i] = g_joint[i] as f32.  Pad samples: L2 = ld = +inf and g = 0, so both their weights are exactly 0.
//   pmb_z            one sample per lane, 256 per block, one tile of 16 dimensions per blockIdx.y, one chunk of the bank per blockIdx.z;
//                    the stage of the bank in LDS is shaped as pm_joint's (up to 8 groups of 8 rows, all tiles, at most 48 KB), read by broadcast.
//                    Per group: the 8 joint exponents over ALL dimensions (pm_joint's arithmetic: f32 inside a tile, f64 across tiles,
//                    starting at C[j]), minus L2[i] in f64, one exp2 each, times g_joint[i]; then for each of the lane's 16 dimensions the
//                    8 per-dimension weights, a = gd * rd + gj * r, the 8 products a * ((z - mu) w) summed as an f32 tree and added to the
//                    dimension's f64 sum.  A latent wider than one tile recomputes the joint exponents in every tile's blocks.
//   pmb_bank         the same with the roles swapped: one bank row per lane, a tile of 16 dimensions, chunks of samples staged through
//                    LDS in groups of 8 (S, L2, GJ); two f64 sums per dimension (a * p and a * (-ln 2 * p * (z - mu) - 0.5), p = (z - mu) w).
//   pmb_combine      the chunks' f64 partial sums in chunk order, times the constant that takes (z - mu) w back to u, rounded once to f32.
// Precision: terms in f32; an f32 sum never holds more than the 8 terms of a group (16 inside a tile of the joint exponent; the
// forward's tile is 32); every longer sum is f64.  The chunking is a function of (N, M, d) alone, no atomics: the same bits every run.
#include <math.h>

#include "common.hpp"
#include "kernels.hpp"

namespace mmvae {

namespace {

constexpr int kRows = 8;             // rows (or samples) per group: one f32 tree sum
constexpr int kMinChunk = 64;        // fewest rows of a chunk (but the last), a multiple of kRows
constexpr int kCUs = 256;            // the chip the chunking is sized for; a constant, so that the bits depend on (N, M, d) alone
constexpr int kBlock = 256;          // lanes (threads) per block of a sweep
constexpr int kStageGroups = 8;      // most groups of a stage
constexpr int kStage4 = 3072;        // float4s of a stage: 48 KB = 512 (group, dimension) pairs of 24 floats
constexpr int kDT = 16;              // dimensions per tile of both sweeps: the lane's f64 sums, normalisers and gradients fit 256 VGPRs
constexpr int kMaxD = 512, kMaxN = 16384;
constexpr double kLog2e = 1.4426950408889634074, kLn2 = 0.69314718055994530942, kLog2Pi = 1.8378770664093454836;

struct Plan {
  int ntiles, dpad, Npad, Npad8, Mpad, Mpad8;
  int rows_z, nch_z;                 // pmb_z: bank rows per chunk, chunks
  int rows_b, nch_b;                 // pmb_bank: samples per chunk, chunks
  size_t off_R, off_C, off_S, off_Z, off_L2, off_GJ, off_pz, off_pmu, off_plv, total;
};

// as posterior_mixture.hip: cut `rows` so that the blocks just fill a whole number of rounds of the chip
void chunking(int rows, int units, int slots, int* per, int* nch) {
  const int rounds = (units + slots - 1) / slots;
  const int wanted = rounds * slots / units;                       // >= 1
  int r = ((rows + wanted - 1) / wanted + kRows - 1) / kRows * kRows;
  if (r < kMinChunk) r = kMinChunk;
  *per = r;
  *nch = (rows + r - 1) / r;
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

Plan make_plan(int N, int M, int d) {
  Plan p;
  p.ntiles = (d + kDT - 1) / kDT;
  p.dpad = p.ntiles * kDT;
  p.Npad = (N + kBlock - 1) / kBlock * kBlock;
  p.Mpad = (M + kBlock - 1) / kBlock * kBlock;
  p.Npad8 = (N + kRows - 1) / kRows * kRows;
  p.Mpad8 = (M + kRows - 1) / kRows * kRows;
  chunking(M, p.Npad / kBlock * p.ntiles, kCUs * 2, &p.rows_z, &p.nch_z);                 // both sweeps: 2 blocks per CU (VGPRs)
  chunking(N, p.Mpad / kBlock * p.ntiles, kCUs * 2, &p.rows_b, &p.nch_b);
  const size_t f = sizeof(float), db = sizeof(double);
  size_t at = up16((size_t)p.Mpad8 * p.dpad * 3 * f);                                     // T
  p.off_R = at;   at += up16((size_t)p.Mpad * p.dpad * 3 * f);                            // Rmu, Rw, Rc
  p.off_C = at;   at += up16((size_t)p.Mpad * db);
  p.off_S = at;   at += up16((size_t)p.Npad8 * p.dpad * 3 * f);
  p.off_Z = at;   at += up16((size_t)p.Npad * p.dpad * 3 * f);                            // Z, LD, GD
  p.off_L2 = at;  at += up16((size_t)p.Npad * db);
  p.off_GJ = at;  at += up16((size_t)p.Npad * f);
  p.off_pz = at;  at += up16((size_t)p.nch_z * p.Npad * p.dpad * db);
  p.off_pmu = at; at += up16((size_t)p.nch_b * p.Mpad * p.dpad * db);
  p.off_plv = at; at += up16((size_t)p.nch_b * p.Mpad * p.dpad * db);
  p.total = at;
  return p;
}

// 0, or the error code of a shape the call refuses (what: NULL for the silent size query)
int check_shape(const char* what, int N, int M, int d) {
  if (N < 1 || M < 1 || d < 1) {
    if (what) set_error("%s: N=%d, M=%d and d=%d must be positive", what, N, M, d);
    return MMVAE_ERR_ARG;
  }
  if (d > kMaxD || N > kMaxN || M > kMaxN) {
    if (what) set_error("%s: N=%d, M=%d, d=%d unsupported (N, M <= %d, d <= %d)", what, N, M, d, kMaxN, kMaxD);
    return MMVAE_ERR_UNSUPPORTED;
  }
  return 0;
}

// grid: Mpad * dpad / 256 blocks of 256 threads, one padded bank entry per thread
__global__ __launch_bounds__(256) void pmb_bank_prep_kernel(const float* __restrict__ mu, const float* __restrict__ lv, int M, int d, int dpad,
                                                            int Mpad8, size_t total, float* __restrict__ T, float* __restrict__ Rmu,
                                                            float* __restrict__ Rw, float* __restrict__ Rc, double* __restrict__ C) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int j = (int)(e / dpad), dd = (int)(e - (size_t)j * dpad);
  float m = 0.f, w = 0.f, c = 0.f;
  if (j >= M) c = -INFINITY;
  else if (dd < d) {
    const double l = (double)lv[(size_t)j * d + dd];
    m = mu[(size_t)j * d + dd];
    w = (float)(-0.5 * kLog2e * exp(-l));
    c = (float)(-0.5 * kLog2e * (l + kLog2Pi));
  }
  Rmu[e] = m;
  Rw[e] = w;
  Rc[e] = c;
  if (j < Mpad8) {
    float* at = T + ((size_t)(j / kRows) * dpad + dd) * (3 * kRows) + (j % kRows);
    at[0] = m;
    at[kRows] = w;
    at[2 * kRows] = c;
  }
  if (dd == 0) {
    double a = 0.0;
    if (j < M)
      for (int k = 0; k < d; ++k) a += (double)lv[(size_t)j * d + k];
    C[j] = j < M ? -0.5 * kLog2e * (a + (double)d * kLog2Pi) : -(double)INFINITY;
  }
}

// grid: Npad * dpad / 256 blocks of 256 threads, one padded sample entry per thread
__global__ __launch_bounds__(256) void pmb_sample_prep_kernel(const float* __restrict__ z, const double* __restrict__ log_qz,
                                                              const double* __restrict__ log_qz_dims, const double* __restrict__ g_joint,
                                                              const double* __restrict__ g_dims, int N, int d, int dpad, int Npad8,
                                                              size_t total, double log_m, float* __restrict__ S, float* __restrict__ Z,
                                                              float* __restrict__ LD, float* __restrict__ GD, double* __restrict__ L2,
                                                              float* __restrict__ GJ) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int i = (int)(e / dpad), dd = (int)(e - (size_t)i * dpad);
  const bool real = i < N && dd < d;
  const float zv = real ? z[(size_t)i * d + dd] : 0.f;
  float ld = i < N ? 0.f : INFINITY, gd = 0.f;
  if (real && g_dims) {
    ld = (float)((log_qz_dims[(size_t)i * d + dd] + log_m) * kLog2e);
    gd = (float)g_dims[(size_t)i * d + dd];
  }
  Z[e] = zv;
  LD[e] = ld;
  GD[e] = gd;
  if (i < Npad8) {
    float* at = S + ((size_t)(i / kRows) * dpad + dd) * (3 * kRows) + (i % kRows);
    at[0] = zv;
    at[kRows] = ld;
    at[2 * kRows] = gd;
  }
  if (dd == 0) {
    L2[i] = i < N ? (log_qz[i] + log_m) * kLog2e : (double)INFINITY;
    GJ[i] = (i < N && g_joint) ? (float)g_joint[i] : 0.f;
  }
}

template <int DT>
__device__ __forceinline__ void load_tile(const float* __restrict__ p, float (&zt)[DT]) {
#pragma unroll
  for (int q = 0; q < DT / 4; ++q) {
    const float4 v = reinterpret_cast<const float4*>(p)[q];
    zt[4 * q] = v.x; zt[4 * q + 1] = v.y; zt[4 * q + 2] = v.z; zt[4 * q + 3] = v.w;
  }
}

// the 8 entries of one (group, dimension) pair: two broadcast 16-byte LDS reads
__device__ __forceinline__ void rows8(const float4* __restrict__ p, float (&v)[kRows]) {
  const float4 a = p[0], b = p[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

__device__ __forceinline__ float tree8(const float (&q)[kRows]) { return ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7])); }

// grid (Npad / 256, tiles, chunks of the bank).  ONE_TILE: the lane's tile is the whole latent and stays in registers; otherwise the joint
// pass walks the tiles through `zt` and the lane's own tile is loaded again behind it.  HJ / HD: g_joint / g_dims given.
template <bool ONE_TILE, bool HJ, bool HD>
__global__ __launch_bounds__(kBlock) void pmb_z_kernel(const float* __restrict__ Z, const float* __restrict__ LD, const float* __restrict__ GD,
                                                       const double* __restrict__ L2, const float* __restrict__ GJ,
                                                       const float* __restrict__ T, const double* __restrict__ C, int Npad, int dpad,
                                                       int ntiles, int stage_groups, int groups_per_chunk, int ngroups,
                                                       double* __restrict__ part) {
  constexpr int DT = kDT;
  __shared__ float4 sh[kStage4];
  __shared__ double shC[kStageGroups * kRows];
  const int tid = threadIdx.x, i = blockIdx.x * kBlock + tid, tile = blockIdx.y;
  const int g0 = blockIdx.z * groups_per_chunk, g1 = min(g0 + groups_per_chunk, ngroups);
  const float* zrow = Z + (size_t)i * dpad;
  float zt[DT], ld[DT], gd[DT];
  double acc[DT];
  if (ONE_TILE || !HJ) load_tile<DT>(zrow + tile * DT, zt);
  if (HD) {
    load_tile<DT>(LD + (size_t)i * dpad + tile * DT, ld);
    load_tile<DT>(GD + (size_t)i * dpad + tile * DT, gd);
  }
  const double l2 = HJ ? L2[i] : 0.0;
  const float gj = HJ ? GJ[i] : 0.f;
#pragma unroll
  for (int k = 0; k < DT; ++k) acc[k] = 0.0;
  for (int gs0 = g0; gs0 < g1; gs0 += stage_groups) {                  // (block-uniform trip count)
    const int ns = min(stage_groups, g1 - gs0);
    __syncthreads();                                                   // the previous stage has been read
    const float4* src = reinterpret_cast<const float4*>(T + (size_t)gs0 * dpad * (3 * kRows));
    for (int e = tid; e < ns * dpad * 6; e += kBlock) sh[e] = src[e];  // ns * dpad * 6 <= kStage4: stage_groups * dpad <= 512
    if (tid < ns * kRows) shC[tid] = C[(size_t)gs0 * kRows + tid];
    __syncthreads();
    for (int gs = 0; gs < ns; ++gs) {
      float gr[kRows];                                                 // g_joint[i] * r_ij of the group's rows
#pragma unroll
      for (int r = 0; r < kRows; ++r) gr[r] = 0.f;
      if (HJ) {
        double s2[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) s2[r] = shC[gs * kRows + r];
        for (int t = 0; t < (ONE_TILE ? 1 : ntiles); ++t) {
          if (!ONE_TILE) load_tile<DT>(zrow + t * DT, zt);
          const float4* tp = sh + (gs * ntiles + t) * (DT * 6);
          float a[kRows];
#pragma unroll
          for (int r = 0; r < kRows; ++r) a[r] = 0.f;
#pragma unroll
          for (int k = 0; k < DT; ++k) {
            float mu[kRows], w[kRows];
            rows8(tp + k * 6, mu);
            rows8(tp + k * 6 + 2, w);
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
              const float dl = __fsub_rn(zt[k], mu[r]);
              a[r] = __fmaf_rn(__fmul_rn(dl, w[r]), dl, a[r]);
            }
          }
#pragma unroll
          for (int r = 0; r < kRows; ++r) s2[r] += (double)a[r];
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) gr[r] = __fmul_rn(gj, __builtin_amdgcn_exp2f((float)(s2[r] - l2)));
        if (!ONE_TILE) load_tile<DT>(zrow + tile * DT, zt);
      }
      const float4* tp = sh + (gs * ntiles + tile) * (DT * 6);
#pragma unroll
      for (int k = 0; k < DT; ++k) {
        float mu[kRows], w[kRows], c[kRows], q[kRows];
        rows8(tp + k * 6, mu);
        rows8(tp + k * 6 + 2, w);
        if (HD) rows8(tp + k * 6 + 4, c);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
          const float dl = __fsub_rn(zt[k], mu[r]);
          const float p = __fmul_rn(dl, w[r]);
          float a = gr[r];
          if (HD) a = __fmaf_rn(gd[k], __builtin_amdgcn_exp2f(__fsub_rn(__fmaf_rn(p, dl, c[r]), ld[k])), a);
          q[r] = __fmul_rn(a, p);
        }
        acc[k] += (double)tree8(q);
        __builtin_amdgcn_sched_barrier(0);                             // one dimension at a time: keeps the live LDS reads to 24
      }
    }
  }
  const size_t at = ((size_t)blockIdx.z * Npad + i) * dpad + tile * DT;
#pragma unroll
  for (int k = 0; k < DT; ++k) part[at + k] = acc[k];
}

// grid (Mpad / 256, dpad / 16, chunks of the samples): a bank row per lane, the samples through LDS
template <bool HJ, bool HD>
__global__ __launch_bounds__(kBlock) void pmb_bank_kernel(const float* __restrict__ Rmu, const float* __restrict__ Rw, const float* __restrict__ Rc,
                                                          const double* __restrict__ C, const float* __restrict__ S,
                                                          const double* __restrict__ L2, const float* __restrict__ GJ, int Mpad, int dpad,
                                                          int stage_groups, int groups_per_chunk, int ngroups, double* __restrict__ pmu,
                                                          double* __restrict__ plv) {
  constexpr int DT = kDT;
  __shared__ float4 sh[kStage4];
  __shared__ double shL2[kStageGroups * kRows];
  __shared__ float shGJ[kStageGroups * kRows];
  const int tid = threadIdx.x, j = blockIdx.x * kBlock + tid, tile = blockIdx.y, ntiles = dpad / DT;
  const int g0 = blockIdx.z * groups_per_chunk, g1 = min(g0 + groups_per_chunk, ngroups);
  const size_t row = (size_t)j * dpad;
  float mu[DT], w[DT], c[DT];
  double amu[DT], alv[DT];
  load_tile<DT>(Rmu + row + tile * DT, mu);
  load_tile<DT>(Rw + row + tile * DT, w);
  if (HD) load_tile<DT>(Rc + row + tile * DT, c);
  const double cj = HJ ? C[j] : 0.0;
#pragma unroll
  for (int k = 0; k < DT; ++k) { amu[k] = 0.0; alv[k] = 0.0; }
  for (int gs0 = g0; gs0 < g1; gs0 += stage_groups) {                  // (block-uniform trip count)
    const int ns = min(stage_groups, g1 - gs0);
    __syncthreads();                                                   // the previous stage has been read
    const float4* src = reinterpret_cast<const float4*>(S + (size_t)gs0 * dpad * (3 * kRows));
    for (int e = tid; e < ns * dpad * 6; e += kBlock) sh[e] = src[e];  // ns * dpad * 6 <= kStage4: stage_groups * dpad <= 512
    if (tid < ns * kRows) {
      shL2[tid] = L2[(size_t)gs0 * kRows + tid];
      shGJ[tid] = GJ[(size_t)gs0 * kRows + tid];
    }
    __syncthreads();
    for (int gs = 0; gs < ns; ++gs) {
      float gr[kRows];                                                 // g_joint[i] * r_ij of the group's samples
#pragma unroll
      for (int r = 0; r < kRows; ++r) gr[r] = 0.f;
      if (HJ) {
        double s2[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) s2[r] = cj;
        for (int t = 0; t < ntiles; ++t) {
          float mm[DT], ww[DT];
          load_tile<DT>(Rmu + row + t * DT, mm);
          load_tile<DT>(Rw + row + t * DT, ww);
          const float4* tp = sh + (gs * ntiles + t) * (DT * 6);
          float a[kRows];
#pragma unroll
          for (int r = 0; r < kRows; ++r) a[r] = 0.f;
#pragma unroll
          for (int k = 0; k < DT; ++k) {
            float zz[kRows];
            rows8(tp + k * 6, zz);
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
              const float dl = __fsub_rn(zz[r], mm[k]);
              a[r] = __fmaf_rn(__fmul_rn(dl, ww[k]), dl, a[r]);
            }
          }
#pragma unroll
          for (int r = 0; r < kRows; ++r) s2[r] += (double)a[r];
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r)
          gr[r] = __fmul_rn(shGJ[gs * kRows + r], __builtin_amdgcn_exp2f((float)(s2[r] - shL2[gs * kRows + r])));
      }
      const float4* tp = sh + (gs * ntiles + tile) * (DT * 6);
#pragma unroll
      for (int k = 0; k < DT; ++k) {
        float zz[kRows], ld[kRows], gd[kRows], q[kRows], h[kRows];
        rows8(tp + k * 6, zz);
        if (HD) {
          rows8(tp + k * 6 + 2, ld);
          rows8(tp + k * 6 + 4, gd);
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
          const float dl = __fsub_rn(zz[r], mu[k]);
          const float p = __fmul_rn(dl, w[k]);
          float a = gr[r];
          if (HD) a = __fmaf_rn(gd[r], __builtin_amdgcn_exp2f(__fsub_rn(__fmaf_rn(p, dl, c[k]), ld[r])), a);
          q[r] = __fmul_rn(a, p);
          h[r] = __fmul_rn(a, __fmaf_rn(__fmul_rn(p, dl), -(float)kLn2, -0.5f));      // a * 0.5 ((z - mu) u - 1)
        }
        amu[k] += (double)tree8(q);
        alv[k] += (double)tree8(h);
      }
    }
  }
  const size_t at = ((size_t)blockIdx.z * Mpad + j) * dpad + tile * DT;
#pragma unroll
  for (int k = 0; k < DT; ++k) { pmu[at + k] = amu[k]; plv[at + k] = alv[k]; }
}

// the chunks' partial sums in chunk order; u = (z - mu) exp(-logvar) = -2 ln 2 (z - mu) w.  One output element per thread, d_z first.
__global__ __launch_bounds__(256) void pmb_combine_kernel(const double* __restrict__ pz, const double* __restrict__ pmu, const double* __restrict__ plv,
                                                          int N, int M, int d, int dpad, int Npad, int Mpad, int nch_z, int nch_b,
                                                          float* __restrict__ d_z, float* __restrict__ d_mu, float* __restrict__ d_lv) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, nz = (size_t)N * d, nb = (size_t)M * d;
  if (e < nz) {
    const size_t i = e / d, at = i * dpad + (e - i * d);
    double s = 0.0;
    for (int c = 0; c < nch_z; ++c) s += pz[(size_t)c * Npad * dpad + at];
    d_z[e] = (float)(2.0 * kLn2 * s);
  } else if (e < nz + nb) {
    const size_t b = e - nz, j = b / d, at = j * dpad + (b - j * d);
    double sm = 0.0, sl = 0.0;
    for (int c = 0; c < nch_b; ++c) {
      sm += pmu[(size_t)c * Mpad * dpad + at];
      sl += plv[(size_t)c * Mpad * dpad + at];
    }
    d_mu[b] = (float)(-2.0 * kLn2 * sm);
    d_lv[b] = (float)sl;
  }
}

struct Bufs {
  const float *T, *Rmu, *Rw, *Rc, *S, *Z, *LD, *GD, *GJ;
  const double *C, *L2;
  double *pz, *pmu, *plv;
};

template <bool ONE_TILE, bool HJ, bool HD>
void launch_z(const Plan& p, const Bufs& b, int stage_groups, hipStream_t s) {
  hipLaunchKernelGGL((pmb_z_kernel<ONE_TILE, HJ, HD>), dim3((unsigned)(p.Npad / kBlock), (unsigned)p.ntiles, (unsigned)p.nch_z), dim3(kBlock), 0,
                     s, b.Z, b.LD, b.GD, b.L2, b.GJ, b.T, b.C, p.Npad, p.dpad, p.ntiles, stage_groups, p.rows_z / kRows, p.Mpad8 / kRows, b.pz);
}

template <bool HJ, bool HD>
void launch_sweeps(const Plan& p, const Bufs& b, hipStream_t s) {
  const int stage_groups = 512 / p.dpad < kStageGroups ? 512 / p.dpad : kStageGroups;      // >= 1: dpad <= 512
  if (p.ntiles == 1 || !HJ) launch_z<true, HJ, HD>(p, b, stage_groups, s);                // without g_joint there is no joint pass
  else if constexpr (HJ) launch_z<false, HJ, HD>(p, b, stage_groups, s);
  hipLaunchKernelGGL((pmb_bank_kernel<HJ, HD>), dim3((unsigned)(p.Mpad / kBlock), (unsigned)p.ntiles, (unsigned)p.nch_b), dim3(kBlock), 0,
                     s, b.Rmu, b.Rw, b.Rc, b.C, b.S, b.L2, b.GJ, p.Mpad, p.dpad, stage_groups, p.rows_b / kRows, p.Npad8 / kRows, b.pmu, b.plv);
}

}  // namespace

size_t posterior_mixture_bwd_scratch_bytes(int N, int M, int d) {
  if (check_shape(nullptr, N, M, d) != 0) return 0;
  return make_plan(N, M, d).total;
}

int launch_posterior_mixture_bwd(const float* z, int N, const float* mu, const float* logvar, int M, int d, const double* log_qz,
                                 const double* log_qz_dims, const double* g_joint, const double* g_dims, float* d_z, float* d_mu,
                                 float* d_logvar, void* scratch, size_t scratch_bytes, hipStream_t s) {
  const char* what = "posterior_mixture_bwd";
  const int rc = check_shape(what, N, M, d);
  if (rc != 0) return rc;
  if (!z || !mu || !logvar || !log_qz || !d_z || !d_mu || !d_logvar || !scratch) {
    set_error("%s: NULL %s", what, !z ? "z" : !mu ? "mu" : !logvar ? "logvar" : !log_qz ? "log_qz" : !d_z ? "d_z" : !d_mu ? "d_mu"
                                   : !d_logvar ? "d_logvar" : "scratch");
    return MMVAE_ERR_ARG;
  }
  if (!g_joint && !g_dims) { set_error("%s: g_joint and g_dims are both NULL", what); return MMVAE_ERR_ARG; }
  if (g_dims && !log_qz_dims) { set_error("%s: g_dims needs log_qz_dims", what); return MMVAE_ERR_ARG; }
  if ((uintptr_t)scratch & 15) { set_error("%s: scratch=%p must be 16-byte aligned", what, scratch); return MMVAE_ERR_ARG; }
  const Plan p = make_plan(N, M, d);
  if (scratch_bytes < p.total) {
    set_error("%s: scratch_bytes=%zu below the %zu this shape needs", what, scratch_bytes, p.total);
    return MMVAE_ERR_ARG;
  }
  unsigned char* base = static_cast<unsigned char*>(scratch);
  const size_t nb = (size_t)p.Mpad * p.dpad, ns = (size_t)p.Npad * p.dpad;
  float* T = reinterpret_cast<float*>(base);
  float* R = reinterpret_cast<float*>(base + p.off_R);
  double* C = reinterpret_cast<double*>(base + p.off_C);
  float* S = reinterpret_cast<float*>(base + p.off_S);
  float* Z = reinterpret_cast<float*>(base + p.off_Z);
  double* L2 = reinterpret_cast<double*>(base + p.off_L2);
  float* GJ = reinterpret_cast<float*>(base + p.off_GJ);
  Bufs b;
  b.T = T; b.Rmu = R; b.Rw = R + nb; b.Rc = R + 2 * nb; b.C = C;
  b.S = S; b.Z = Z; b.LD = Z + ns; b.GD = Z + 2 * ns; b.L2 = L2; b.GJ = GJ;
  b.pz = reinterpret_cast<double*>(base + p.off_pz);
  b.pmu = reinterpret_cast<double*>(base + p.off_pmu);
  b.plv = reinterpret_cast<double*>(base + p.off_plv);
  hipLaunchKernelGGL(pmb_bank_prep_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, mu, logvar, M, d, p.dpad, p.Mpad8, nb, T, R, R + nb,
                     R + 2 * nb, C);
  int e = check_launch("posterior_mixture_bwd (bank)");
  if (e != 0) return e;
  hipLaunchKernelGGL(pmb_sample_prep_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, s, z, log_qz, log_qz_dims, g_joint, g_dims, N, d,
                     p.dpad, p.Npad8, ns, log((double)M), S, Z, Z + ns, Z + 2 * ns, L2, GJ);
  e = check_launch("posterior_mixture_bwd (samples)");
  if (e != 0) return e;
  if (g_joint && g_dims) launch_sweeps<true, true>(p, b, s);
  else if (g_joint) launch_sweeps<true, false>(p, b, s);
  else launch_sweeps<false, true>(p, b, s);
  e = check_launch("posterior_mixture_bwd (sweeps)");
  if (e != 0) return e;
  const size_t nout = (size_t)N * d + (size_t)M * d;
  hipLaunchKernelGGL(pmb_combine_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, s, b.pz, b.pmu, b.plv, N, M, d, p.dpad, p.Npad, p.Mpad,
                     p.nch_z, p.nch_b, d_z, d_mu, d_logvar);
  return check_launch("posterior_mixture_bwd (combine)");
}

}  // namespace mmvae
