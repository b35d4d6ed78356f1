// Aggregate-posterior densities for the ELBO split of Hoffman & Johnson 2016: every sample z_i against the whole bank of M diagonal
// Gaussian posteriors N(mu_j, exp(logvar_j)),
//   t_ijd = -0.5 ((z_id - mu_jd)^2 exp(-logvar_jd) + logvar_jd + log 2 pi),   s_ij = sum_d t_ijd,
//   log_qz[i] = logsumexp_j s_ij - log M,   log_qz_dims[i][d] = logsumexp_j t_ijd - log M.
// N * M * d Gaussian terms and, for the per-dimension output, as many exponentials; inputs and outputs are a few MB.
//
// Dataflow (all on the caller's stream):
//   pm_bank_prep   the bank, once, in the base-2 domain and in the order the sweeps read it: group g of 8 rows, tile of DT dimensions,
//                  T[g][tile][k][{mu, w, c}][8 rows],  w = -0.5 log2(e) exp(-logvar),  c = -0.5 log2(e) (logvar + log 2 pi), both formed
//                  in f64 and rounded once to f32; C[j] = sum_d c_jd in f64.  Pad rows (M up to a multiple of 8) get w = 0, c = C = -inf:
//                  their terms are -inf and their exponentials 0, with no test in the sweep; pad dimensions get mu = w = c = 0.
//   pm_z_prep      z padded with zeros to [N up to 256][d up to DT], so the sweeps load whole aligned tiles without a bound test.
//   pm_joint       one sample per lane, 256 samples per block, one bank chunk per blockIdx.y.  The block copies a stage of the re-laid
//                  bank (up to 8 groups, all their tiles: one contiguous piece of at most 48 KB) and its C[j] into LDS; every lane
//                  then reads the same address, an LDS broadcast (ds_read_b128: four rows' mu or w at a time), and a pair-term costs a
//                  subtract, a multiply and an FMA.  Eight rows at a time: f32 partial sums of a tile (DT terms each), added to f64 row
//                  sums that start at C[j]; then one online log-sum-exp step for the group (maximum, one rescale, eight exponentials)
//                  with the running maximum and sum in f64.
//   pm_dims        the same sweep for one tile of DT dimensions (blockIdx.y) and one chunk (blockIdx.z), stages of 8 groups of that
//                  tile (24 KB at DT = 32): z, the running maxima (f32) and the running sums (f64) of the lane's DT dimensions live in
//                  registers, every index a compile-time constant (the loops over k and the 8 rows are fully unrolled).  Per dimension
//                  and group: 8 terms, their maximum with the running one, one rescale, 8 exponentials, an f32 tree sum of those 8,
//                  one f64 FMA into the running sum.
//   pm_*_combine   only when the bank was cut into more than one chunk: the chunks' (max, sum) pairs, which went through scratch, are
//                  merged in chunk order in f64.  With one chunk the sweeps write the outputs themselves, by the same finishing formula.
// Precision: terms in f32 from f32 inputs; no sum of exponentials is ever carried in f32 over more than 8 terms.  The chunking is a
// function of (N, M, d) alone, nothing is accumulated into memory and there are no atomics: the same bits every run.
// log_qz does not depend on whether log_qz_dims is asked for: it comes from its own kernels.
#include <math.h>

#include "common.hpp"
#include "kernels.hpp"

namespace mmvae {

namespace {

constexpr int kRows = 8;             // bank rows per group: one online log-sum-exp step
constexpr int kMinChunk = 64;        // fewest bank rows of a chunk (but the last), a multiple of kRows
constexpr int kCUs = 256;            // the chip the chunking is sized for; a constant, so that the bits depend on (N, M, d) alone
constexpr int kBlock = 256;          // samples (threads) per block of a sweep
constexpr int kStageGroups = 8;      // most groups of a stage
constexpr int kJointStage4 = 3072;   // float4s of the joint sweep's stage: 48 KB = 512 (group, dimension) pairs of 24 floats
constexpr int kMaxD = 512, kMaxN = 1 << 20;
constexpr double kLog2e = 1.4426950408889634074, kLn2 = 0.69314718055994530942, kLog2Pi = 1.8378770664093454836;

struct Plan {
  int DT, ntiles, dpad, Npad, Mpad, nblocks;
  int rows_j, nch_j;                 // joint sweep: bank rows per chunk, chunks
  int rows_d, nch_d;                 // per-dimension sweep
  size_t off_C, off_Z, off_jm, off_js, off_dm, off_ds, total;
};

// units: blocks the sweep has without cutting the bank; slots: blocks the chip holds at once.  The bank is cut so that the blocks
// just fill a whole number of rounds of the chip (one round when units <= slots), in chunks of at least kMinChunk rows.
void chunking(int M, int units, int slots, int* rows, int* nch) {
  const int rounds = (units + slots - 1) / slots;
  const int wanted = rounds * slots / units;                       // >= 1
  int r = ((M + wanted - 1) / wanted + kRows - 1) / kRows * kRows;
  if (r < kMinChunk) r = kMinChunk;
  *rows = r;
  *nch = (M + r - 1) / r;
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

Plan make_plan(int N, int M, int d) {
  Plan p;
  p.DT = d <= 16 ? 16 : 32;
  p.ntiles = (d + p.DT - 1) / p.DT;
  p.dpad = p.ntiles * p.DT;
  p.Npad = (N + kBlock - 1) / kBlock * kBlock;
  p.Mpad = (M + kRows - 1) / kRows * kRows;
  p.nblocks = p.Npad / kBlock;
  chunking(M, p.nblocks, kCUs * 3, &p.rows_j, &p.nch_j);                                   // pm_joint: 48.5 KB of LDS, 3 blocks per CU
  chunking(M, p.nblocks * p.ntiles, kCUs * (p.DT == 32 ? 2 : 4), &p.rows_d, &p.nch_d);     // pm_dims: 198 / 126 VGPRs, 2 / 4 blocks per CU
  size_t at = up16((size_t)p.Mpad * p.dpad * 3 * sizeof(float));
  p.off_C = at;  at += up16((size_t)p.Mpad * sizeof(double));
  p.off_Z = at;  at += up16((size_t)p.Npad * p.dpad * sizeof(float));
  const size_t nj = p.nch_j > 1 ? (size_t)p.nch_j * p.Npad : 0, nd = p.nch_d > 1 ? (size_t)p.nch_d * p.Npad * p.dpad : 0;
  p.off_jm = at; at += up16(nj * sizeof(double));
  p.off_js = at; at += up16(nj * sizeof(double));
  p.off_dm = at; at += up16(nd * sizeof(float));
  p.off_ds = at; at += up16(nd * sizeof(double));
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

// the one finishing formula: base-2 (max, sum) -> natural-log mixture density
__device__ __forceinline__ double finish(double m, double s, double log_m) { return (m + log2(s)) * kLn2 - log_m; }

// grid: Mpad / 8 blocks of 256 threads
__global__ __launch_bounds__(256) void pm_bank_prep_kernel(const float* __restrict__ mu, const float* __restrict__ lv, int M, int d, int DT,
                                                           int ntiles, float* __restrict__ T, double* __restrict__ C) {
  const int g = blockIdx.x, tid = threadIdx.x, dpad = ntiles * DT;
  float* tg = T + (size_t)g * dpad * (3 * kRows);
  for (int e = tid; e < kRows * dpad; e += 256) {
    const int r = e / dpad, dd = e - r * dpad, j = g * kRows + r;
    float m = 0.f, w = 0.f, c = 0.f;
    if (j >= M) c = -INFINITY;
    else if (dd < d) {
      const double l = (double)lv[(size_t)j * d + dd];
      m = mu[(size_t)j * d + dd];
      w = (float)(-0.5 * kLog2e * exp(-l));
      c = (float)(-0.5 * kLog2e * (l + kLog2Pi));
    }
    float* at = tg + (size_t)dd * (3 * kRows) + r;           // [tile][k] is dd: tiles are DT consecutive dimensions
    at[0] = m;
    at[kRows] = w;
    at[2 * kRows] = c;
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int j = g * kRows + wave * 2 + rr;
    double a = 0.0;
    if (j < M)
      for (int dd = lane; dd < d; dd += 64) a += (double)lv[(size_t)j * d + dd];
    a = wave_sum_d(a);
    if (lane == 0) C[j] = j < M ? -0.5 * kLog2e * (a + (double)d * kLog2Pi) : -(double)INFINITY;
  }
}

__global__ __launch_bounds__(256) void pm_z_prep_kernel(const float* __restrict__ z, int N, int d, int dpad, size_t total, float* __restrict__ Z) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const size_t i = e / dpad;
  const int dd = (int)(e - i * dpad);
  Z[e] = (i < (size_t)N && dd < d) ? z[i * d + dd] : 0.f;
}

template <int DT>
__device__ __forceinline__ void load_tile(const float* __restrict__ p, float (&zt)[DT]) {
#pragma unroll
  for (int q = 0; q < DT / 4; ++q) {
    const float4 v = reinterpret_cast<const float4*>(p)[q];
    zt[4 * q] = v.x; zt[4 * q + 1] = v.y; zt[4 * q + 2] = v.z; zt[4 * q + 3] = v.w;
  }
}

// the 8 rows of one (group, dimension) pair: two broadcast 16-byte LDS reads
__device__ __forceinline__ void rows8(const float4* __restrict__ p, float (&v)[kRows]) {
  const float4 a = p[0], b = p[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// grid (Npad / 256, chunks)
template <int DT, bool ONE_TILE>
__global__ __launch_bounds__(kBlock) void pm_joint_kernel(const float* __restrict__ Z, const float* __restrict__ T, const double* __restrict__ C,
                                                          int N, int Npad, int dpad, int ntiles, int stage_groups, int groups_per_chunk,
                                                          int ngroups, int nchunks, double log_m, double* __restrict__ out,
                                                          double* __restrict__ pm, double* __restrict__ ps) {
  __shared__ float4 sh[kJointStage4];
  __shared__ double shC[kStageGroups * kRows];
  const int tid = threadIdx.x, i = blockIdx.x * kBlock + tid;
  const int g0 = blockIdx.y * groups_per_chunk, g1 = min(g0 + groups_per_chunk, ngroups);
  const float* zrow = Z + (size_t)i * dpad;
  float zt[DT];
  if (ONE_TILE) load_tile<DT>(zrow, zt);
  double m = -(double)INFINITY, s = 0.0;
  for (int gs0 = g0; gs0 < g1; gs0 += stage_groups) {                  // (block-uniform trip count)
    const int ns = min(stage_groups, g1 - gs0);
    __syncthreads();                                                   // the previous stage has been read
    const float4* src = reinterpret_cast<const float4*>(T + (size_t)gs0 * dpad * (3 * kRows));
    for (int e = tid; e < ns * dpad * 6; e += kBlock) sh[e] = src[e];  // ns * dpad * 6 <= kJointStage4: stage_groups * dpad <= 512
    if (tid < ns * kRows) shC[tid] = C[(size_t)gs0 * kRows + tid];
    __syncthreads();
    for (int gs = 0; gs < ns; ++gs) {
      double acc[kRows];
#pragma unroll
      for (int r = 0; r < kRows; ++r) acc[r] = shC[gs * kRows + r];
      for (int tile = 0; tile < ntiles; ++tile) {
        if (!ONE_TILE) load_tile<DT>(zrow + tile * DT, zt);
        const float4* tp = sh + (gs * ntiles + tile) * (DT * 6);
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
        for (int r = 0; r < kRows; ++r) acc[r] += (double)a[r];
      }
      double gm = m;
#pragma unroll
      for (int r = 0; r < kRows; ++r) gm = fmax(gm, acc[r]);
      float p[kRows];
#pragma unroll
      for (int r = 0; r < kRows; ++r) p[r] = __builtin_amdgcn_exp2f((float)(acc[r] - gm));
      const float sum = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
      s = fma(s, (double)__builtin_amdgcn_exp2f((float)(m - gm)), (double)sum);
      m = gm;
    }
  }
  if (nchunks == 1) {
    if (i < N) out[i] = finish(m, s, log_m);
  } else {
    pm[(size_t)blockIdx.y * Npad + i] = m;
    ps[(size_t)blockIdx.y * Npad + i] = s;
  }
}

// grid (Npad / 256, tiles, chunks)
template <int DT>
__global__ __launch_bounds__(kBlock) void pm_dims_kernel(const float* __restrict__ Z, const float* __restrict__ T, int N, int Npad, int d,
                                                         int dpad, int ntiles, int groups_per_chunk, int ngroups, int nchunks, double log_m,
                                                         double* __restrict__ out, float* __restrict__ pm, double* __restrict__ ps) {
  __shared__ float4 sh[kStageGroups * DT * 6];
  const int tid = threadIdx.x, i = blockIdx.x * kBlock + tid, tile = blockIdx.y;
  const int g0 = blockIdx.z * groups_per_chunk, g1 = min(g0 + groups_per_chunk, ngroups);
  float zt[DT], m[DT];
  double s[DT];
  load_tile<DT>(Z + (size_t)i * dpad + tile * DT, zt);
#pragma unroll
  for (int k = 0; k < DT; ++k) { m[k] = -INFINITY; s[k] = 0.0; }
  for (int gs0 = g0; gs0 < g1; gs0 += kStageGroups) {                   // (block-uniform trip count)
    const int ns = min(kStageGroups, g1 - gs0);
    __syncthreads();                                                   // the previous stage has been read
    for (int e = tid; e < ns * (DT * 6); e += kBlock) {
      const int piece = e / (DT * 6), at = e - piece * (DT * 6);
      sh[e] = reinterpret_cast<const float4*>(T + ((size_t)(gs0 + piece) * ntiles + tile) * (DT * 3 * kRows))[at];
    }
    __syncthreads();
    for (int gs = 0; gs < ns; ++gs) {
      const float4* tp = sh + gs * (DT * 6);
#pragma unroll
      for (int k = 0; k < DT; ++k) {
        float mu[kRows], w[kRows], c[kRows], t[kRows];
        rows8(tp + k * 6, mu);
        rows8(tp + k * 6 + 2, w);
        rows8(tp + k * 6 + 4, c);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
          const float dl = __fsub_rn(zt[k], mu[r]);
          t[r] = __fmaf_rn(__fmul_rn(dl, w[r]), dl, c[r]);
        }
        const float gm = fmaxf(fmaxf(fmaxf(m[k], t[0]), fmaxf(t[1], t[2])), fmaxf(fmaxf(t[3], t[4]), fmaxf(fmaxf(t[5], t[6]), t[7])));
        float p[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) p[r] = __builtin_amdgcn_exp2f(__fsub_rn(t[r], gm));
        const float sum = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
        s[k] = fma(s[k], (double)__builtin_amdgcn_exp2f(__fsub_rn(m[k], gm)), (double)sum);
        m[k] = gm;
      }
    }
  }
  if (nchunks == 1) {
    if (i < N) {
#pragma unroll
      for (int k = 0; k < DT; ++k)
        if (tile * DT + k < d) out[(size_t)i * d + tile * DT + k] = finish((double)m[k], s[k], log_m);
    }
  } else {
    const size_t at = ((size_t)blockIdx.z * Npad + i) * dpad + tile * DT;
#pragma unroll
    for (int k = 0; k < DT; ++k) { pm[at + k] = m[k]; ps[at + k] = s[k]; }
  }
}

// the chunks' (max, sum) pairs in chunk order: out[e] for e < n; pair c of element e is at c * chunk_stride + (e / d) * dpad + e % d
template <typename TM>
__global__ __launch_bounds__(256) void pm_combine_kernel(const TM* __restrict__ pm, const double* __restrict__ ps, size_t n, int d, int dpad,
                                                         size_t chunk_stride, int nchunks, double log_m, double* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const size_t i = e / d, at = i * dpad + (e - i * d);
  double mm = (double)pm[at];
  for (int c = 1; c < nchunks; ++c) mm = fmax(mm, (double)pm[c * chunk_stride + at]);
  double ss = 0.0;
  for (int c = 0; c < nchunks; ++c) ss += ps[c * chunk_stride + at] * exp2((double)pm[c * chunk_stride + at] - mm);
  out[e] = finish(mm, ss, log_m);
}

template <int DT>
void launch_sweeps(const Plan& p, int N, int d, double log_m, const float* Z, const float* T, const double* C, double* log_qz,
                   double* log_qz_dims, double* jm, double* js, float* dm, double* ds, hipStream_t s) {
  const int ngroups = p.Mpad / kRows, nblocks = p.nblocks;
  const int stage_groups = 512 / p.dpad < kStageGroups ? 512 / p.dpad : kStageGroups;       // >= 1: dpad <= 512
  const dim3 gj((unsigned)nblocks, (unsigned)p.nch_j);
  if (p.ntiles == 1)
    hipLaunchKernelGGL((pm_joint_kernel<DT, true>), gj, dim3(kBlock), 0, s, Z, T, C, N, p.Npad, p.dpad, p.ntiles, stage_groups,
                       p.rows_j / kRows, ngroups, p.nch_j, log_m, log_qz, jm, js);
  else
    hipLaunchKernelGGL((pm_joint_kernel<DT, false>), gj, dim3(kBlock), 0, s, Z, T, C, N, p.Npad, p.dpad, p.ntiles, stage_groups,
                       p.rows_j / kRows, ngroups, p.nch_j, log_m, log_qz, jm, js);
  if (log_qz_dims)
    hipLaunchKernelGGL((pm_dims_kernel<DT>), dim3((unsigned)nblocks, (unsigned)p.ntiles, (unsigned)p.nch_d), dim3(kBlock), 0, s, Z, T, N,
                       p.Npad, d, p.dpad, p.ntiles, p.rows_d / kRows, ngroups, p.nch_d, log_m, log_qz_dims, dm, ds);
}

}  // namespace

size_t posterior_mixture_scratch_bytes(int N, int M, int d) {
  if (check_shape(nullptr, N, M, d) != 0) return 0;
  return make_plan(N, M, d).total;
}

int launch_posterior_mixture(const float* z, int N, const float* mu, const float* logvar, int M, int d, double* log_qz, double* log_qz_dims,
                             void* scratch, size_t scratch_bytes, hipStream_t s) {
  const int rc = check_shape("posterior_mixture", N, M, d);
  if (rc != 0) return rc;
  if (!z || !mu || !logvar || !log_qz || !scratch) {
    set_error("posterior_mixture: NULL %s", !z ? "z" : !mu ? "mu" : !logvar ? "logvar" : !log_qz ? "log_qz" : "scratch");
    return MMVAE_ERR_ARG;
  }
  if ((uintptr_t)scratch & 15) { set_error("posterior_mixture: scratch=%p must be 16-byte aligned", scratch); return MMVAE_ERR_ARG; }
  const Plan p = make_plan(N, M, d);
  if (scratch_bytes < p.total) {
    set_error("posterior_mixture: scratch_bytes=%zu below the %zu this shape needs", scratch_bytes, p.total);
    return MMVAE_ERR_ARG;
  }
  unsigned char* base = static_cast<unsigned char*>(scratch);
  float* T = reinterpret_cast<float*>(base);
  double* C = reinterpret_cast<double*>(base + p.off_C);
  float* Z = reinterpret_cast<float*>(base + p.off_Z);
  double* jm = reinterpret_cast<double*>(base + p.off_jm);
  double* js = reinterpret_cast<double*>(base + p.off_js);
  float* dm = reinterpret_cast<float*>(base + p.off_dm);
  double* ds = reinterpret_cast<double*>(base + p.off_ds);
  const double log_m = log((double)M);
  hipLaunchKernelGGL(pm_bank_prep_kernel, dim3((unsigned)(p.Mpad / kRows)), dim3(256), 0, s, mu, logvar, M, d, p.DT, p.ntiles, T, C);
  int e = check_launch("posterior_mixture (bank)");
  if (e != 0) return e;
  const size_t nz = (size_t)p.Npad * p.dpad;
  hipLaunchKernelGGL(pm_z_prep_kernel, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, s, z, N, d, p.dpad, nz, Z);
  e = check_launch("posterior_mixture (samples)");
  if (e != 0) return e;
  if (p.DT == 16) launch_sweeps<16>(p, N, d, log_m, Z, T, C, log_qz, log_qz_dims, jm, js, dm, ds, s);
  else launch_sweeps<32>(p, N, d, log_m, Z, T, C, log_qz, log_qz_dims, jm, js, dm, ds, s);
  e = check_launch("posterior_mixture (sweep)");
  if (e != 0) return e;
  if (p.nch_j > 1) {
    hipLaunchKernelGGL((pm_combine_kernel<double>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, jm, js, (size_t)N, 1, 1, (size_t)p.Npad,
                       p.nch_j, log_m, log_qz);
    e = check_launch("posterior_mixture (combine)");
    if (e != 0) return e;
  }
  if (log_qz_dims && p.nch_d > 1) {
    const size_t n = (size_t)N * d;
    hipLaunchKernelGGL((pm_combine_kernel<float>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dm, ds, n, d, p.dpad,
                       (size_t)p.Npad * p.dpad, p.nch_d, log_m, log_qz_dims);
    e = check_launch("posterior_mixture (combine dims)");
    if (e != 0) return e;
  }
  return 0;
}

}  // namespace mmvae
