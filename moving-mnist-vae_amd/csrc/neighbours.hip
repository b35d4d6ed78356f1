// Nearest training frames of a sample: exact k-NN of M uint8 query planes over F resident uint8 frames of D bytes (mmvae_nearest_frames).
//
//   d(m, f) = sum_i (q[m][i] - t(x[f][i]))^2, t = identity or a 256-byte table; all integer, no floating point anywhere.
//   With a' = a ^ 0x80 read as int8 (= a - 128) on both sides:  d = sum a'^2 + sum b'^2 - 2 sum a' b'.  The cross term is a
//   [M_p x D] x [D x 16 frames] product on v_mfma_i32_16x16x64_i8 (M_p = M rounded up to 16); every term and partial sum stays below 2^31.
//
// Three launches:
//   nn_prep_kernel   queries -> signed bytes in the A-operand fragment order [row tile][k step][lane][16 B], zero rows / zero bytes where
//                    M_p > M or the last 64-byte k step passes D (zeros add nothing to the product), and the query norms qn[64].
//   nn_scan_kernel   the pass over `frames`.  The 16-frame tiles are cut into contiguous, equal (+-1 tile) ranges, one per wave; a wave walks
//                    its range in walks of up to four tiles.  A k step is 64 bytes of every frame of the tile, the frames as B and the
//                    query rows as A.  Loaded in the operand order an instruction would touch 64 bytes of 16 rows, half a line each;
//                    instead two k steps are read as whole 128-byte lines (8 rows an instruction) and pass through a per-wave LDS stage
//                    into the operand order (measured: 3.8 against 3.0 TB/s at M = 6).
//                    Frame norms come from the bytes in registers (v_dot4_i32_i8).
//                    Selection (knn_select.hpp): lane l of a wave owns query row l; the 4 x RT x CNT keys of a lane are tested against
//                    their rows' k-th keys, one ballot per four rows rejects them (the common case).  The first k of every list go
//                    to scratch at the end, unused slots as ~0.
//   nn_merge_kernel  a block per query: the k merge rounds over all lists, then out_dist / out_index.  ~0 is never reached because F >= k.
// Operand order, key, list and tie rule are defined in knn_select.hpp; the same bits every run, for any partition of the frames.
#include "common.hpp"
#include "kernels.hpp"
#include "knn_select.hpp"

namespace mmvae {

namespace {

constexpr int kMaxM = 64;
constexpr int kScanThreads = 256, kScanWaves = kScanThreads / 64;
constexpr int kMaxBlocks = 512;                      // two blocks of four waves per CU
constexpr int kNT = 4;                               // 16-frame tiles a wave carries through one walk over D

struct Plan {
  int Mp, RT, KS;                                     // query rows padded to 16, row tiles, 64-byte k steps
  long tiles;                                         // 16-frame tiles
  int blocks, lists;                                  // scan grid; k-best lists (one per wave)
  size_t qn_off, lists_off, total;
};

Plan make_plan(int M, long F, int D, int k) {
  Plan p;
  p.Mp = (M + 15) / 16 * 16;
  p.RT = p.Mp / 16;
  p.KS = (D + 63) / 64;
  p.tiles = (F + 15) / 16;
  const long want = (p.tiles + kScanWaves - 1) / kScanWaves;
  p.blocks = (int)(want < kMaxBlocks ? want : kMaxBlocks);
  p.lists = p.blocks * kScanWaves;
  p.qn_off = (size_t)p.RT * p.KS * 1024;              // in front: the queries, [RT][KS][64 lanes][16 B]
  p.lists_off = p.qn_off + kMaxM * sizeof(int);
  p.total = p.lists_off + (size_t)p.lists * M * k * sizeof(u64);
  return p;
}

// ---- queries -> fragment order, norms.  grid RT, 256 threads; a thread per (lane, k step) fragment
__global__ __launch_bounds__(256) void nn_prep_kernel(const unsigned char* __restrict__ q, int M, int D, int KS, uint4* __restrict__ qs,
                                                      int* __restrict__ qn) {
  __shared__ int norm[16];
  const int rt = blockIdx.x, tid = threadIdx.x;
  if (tid < 16) norm[tid] = 0;
  __syncthreads();
  for (int t = tid; t < KS * 64; t += 256) {
    const int s = t >> 6, l = t & 63, row = rt * 16 + (l & 15), off = s * 64 + (l >> 4) * 16;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row < M && off < D) {
      v = *reinterpret_cast<const uint4*>(q + (long)row * D + off);
      atomicAdd(&norm[l & 15], signed_norm16(v, 0));  // integer adds in LDS: any order, the same sum
    }
    qs[((long)rt * KS + s) * 64 + l] = v;
  }
  __syncthreads();
  if (tid < 16) qn[rt * 16 + tid] = norm[tid];
}

// table lookup of the four bytes of a dword; the table already holds t(b) ^ 0x80
__device__ __forceinline__ uint32_t lut4(const unsigned char* t, uint32_t w) {
  return (uint32_t)t[w & 255u] | ((uint32_t)t[(w >> 8) & 255u] << 8) | ((uint32_t)t[(w >> 16) & 255u] << 16) | ((uint32_t)t[w >> 24] << 24);
}

template <int RT, bool LUT, int CNT, bool TAIL>
__device__ __forceinline__ void nn_step(const unsigned char* const (&fp)[CNT], const uint4* __restrict__ qa, int KS, int s, bool live,
                                        const unsigned char* tab, i32x4 (&acc)[RT][CNT], int (&fn)[CNT]) {
  i32x4 a[RT], b[CNT];
#pragma unroll
  for (int nt = 0; nt < CNT; ++nt) {                     // each byte of `frames` is needed once: non-temporal
    const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(fp[nt] + (long)s * 64));
    b[nt] = i32x4{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const uint4 v = qa[((long)rt * KS + s) * 64];
    a[rt] = i32x4{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
  }
#pragma unroll
  for (int nt = 0; nt < CNT; ++nt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t w = (uint32_t)b[nt][j];
      w = LUT ? lut4(tab, w) : (w ^ 0x80808080u);
      if (TAIL && !live) w = 0u;                        // past D: zero in the signed space, for the product and for the norm
      b[nt][j] = (int)w;
      fn[nt] = __builtin_amdgcn_sdot4((int)w, (int)w, fn[nt], false);
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[rt], b[nt], acc[rt][nt], 0, 0, 0);
  }
}

// CNT 16-frame tiles from tile0 on, through all of D, then the selection
template <int RT, bool LUT, int CNT>
__device__ __forceinline__ void nn_unit(const unsigned char* __restrict__ frames, long F, int D, int KS, long tile0,
                                        const uint4* __restrict__ qa, const unsigned char* tab, const int* qn, u32x4_t* stage, u64* list, u64& thr,
                                        int M, int k) {
  const int lane = threadIdx.x & 63, col = lane & 15, grp = lane >> 4;
  i32x4 acc[RT][CNT];
  int fn[CNT];
#pragma unroll
  for (int nt = 0; nt < CNT; ++nt) {
    fn[nt] = 0;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt][nt] = i32x4{0, 0, 0, 0};
  }
  const int full = D / 64;
  // Two k steps at a time, one 128-byte line of every frame row, read as whole lines: a load instruction takes 8 rows x 128 bytes (lane l:
  // row l >> 3, piece l & 7), two of them a tile.  The pieces pass through the wave's own LDS stage into the operand order (lane (c, g),
  // step u: piece 4 u + g of row c).  The next line's loads are issued before this line's products.  The walk starts at a line that
  // differs from walk to walk and wraps around -- a sum does not care -- so that the waves do not sweep the same address bits together.
  const int lines = full / 2;
  if (lines > 0) {
    const unsigned char* lp[CNT][2];
#pragma unroll
    for (int nt = 0; nt < CNT; ++nt)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        long f = (tile0 + nt) * 16 + h * 8 + (lane >> 3);
        if (f > F - 1) f = F - 1;                       // a frame past the end reads the last frame; its keys are dropped
        lp[nt][h] = frames + f * (long)D + (lane & 7) * 16;
      }
    int p = (int)((((unsigned)tile0 * 2654435761u) >> 16) % (unsigned)lines);
    u32x4_t cur[CNT][2];
#pragma unroll
    for (int nt = 0; nt < CNT; ++nt)
#pragma unroll
      for (int h = 0; h < 2; ++h) cur[nt][h] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(lp[nt][h] + (long)p * 128));
    const int rd = (col >> 3) * 64 + (col & 7) * 8 + grp;   // + 4 u: where lane (c, g) finds its piece of step u in a tile's stage
    for (int i = 0; i < lines; ++i) {
#pragma unroll
      for (int nt = 0; nt < CNT; ++nt)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          u32x4_t v = cur[nt][h];
          if (LUT) { v.x = lut4(tab, v.x); v.y = lut4(tab, v.y); v.z = lut4(tab, v.z); v.w = lut4(tab, v.w); }
          else v ^= 0x80808080u;
          stage[(nt * 2 + h) * 64 + lane] = v;
        }
      const int pn = p + 1 == lines ? 0 : p + 1;
      if (i + 1 < lines) {
#pragma unroll
        for (int nt = 0; nt < CNT; ++nt)
#pragma unroll
          for (int h = 0; h < 2; ++h) cur[nt][h] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(lp[nt][h] + (long)pn * 128));
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        i32x4 a[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const uint4 v = qa[((long)rt * KS + 2 * p + u) * 64];
          a[rt] = i32x4{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
        }
#pragma unroll
        for (int nt = 0; nt < CNT; ++nt) {
          const u32x4_t v = stage[nt * 128 + rd + 4 * u];
          const i32x4 b = i32x4{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) fn[nt] = __builtin_amdgcn_sdot4(b[j], b[j], fn[nt], false);
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc[rt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[rt], b, acc[rt][nt], 0, 0, 0);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      p = pn;
    }
  }
  // what is left of D: a single 64-byte step and / or the partial one, straight into the operand order
  const unsigned char* fp[CNT];
#pragma unroll
  for (int nt = 0; nt < CNT; ++nt) {
    long f = (tile0 + nt) * 16 + col;
    if (f > F - 1) f = F - 1;                           // a frame past the end reads the last frame; its keys are dropped
    fp[nt] = frames + f * (long)D + grp * 16;
  }
  for (int s = lines * 2; s < full; ++s) nn_step<RT, LUT, CNT, false>(fp, qa, KS, s, true, tab, acc, fn);
  if (full < KS) {                                      // D = 64 full + 16, 32 or 48: the lanes whose 16 bytes lie past D read the row's last 16
    const bool live = full * 64 + grp * 16 < D;
    const unsigned char* tp[CNT];
#pragma unroll
    for (int nt = 0; nt < CNT; ++nt) tp[nt] = live ? fp[nt] : fp[nt] - grp * 16 + (D - 16) - (long)full * 64;
    nn_step<RT, LUT, CNT, true>(tp, qa, KS, full, live, tab, acc, fn);
  }
  // frame norms: the four 16-lane groups hold the four quarters of every k step
#pragma unroll
  for (int nt = 0; nt < CNT; ++nt) {
    fn[nt] += __shfl_xor(fn[nt], 16, 64);
    fn[nt] += __shfl_xor(fn[nt], 32, 64);
  }
  auto key_of = [&](int rt, int nt, int r) -> u64 {
    const int row = rt * 16 + grp * 4 + r;
    const long f = (tile0 + nt) * 16 + col;
    const int d = qn[row] + fn[nt] - 2 * acc[rt][nt][r];
    return row < M && f < F ? knn_key(d, (u64)f) : kNoKey;
  };
  // almost every frame fails against its row's k-th best: one compare per key and one ballot per four rows is the common path
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const u64 last = shfl64(thr, rt * 16 + grp * 4 + r);
      u64 cand[CNT];
      bool hit = false;
#pragma unroll
      for (int nt = 0; nt < CNT; ++nt) {
        cand[nt] = key_of(rt, nt, r);
        hit |= cand[nt] < last;
      }
      if (__ballot(hit)) knn_insert<CNT, kScanThreads>(cand, rt, r, list, thr, k);
    }
}

template <int RT, bool LUT>
__global__ __launch_bounds__(kScanThreads, 2) void nn_scan_kernel(const unsigned char* __restrict__ frames, long F, int D, int KS, long tiles,
                                                                  const uint4* __restrict__ qs, const int* __restrict__ qn_g,
                                                                  const unsigned char* __restrict__ lut, int M, int k, u64* __restrict__ lists) {
  __shared__ u64 s_list[kMaxK][kScanThreads];             // [j][thread]: the j-th best key of the query row that thread's lane owns
  __shared__ u32x4_t s_stage[kScanWaves][kNT * 2 * 64];   // a wave's own: two 8-row x 128-byte images per tile
  __shared__ int s_qn[kMaxM];
  __shared__ unsigned char s_tab[256];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // in a scalar register: what follows from it is uniform to the compiler too
  if (tid < kMaxM) s_qn[tid] = tid < RT * 16 ? qn_g[tid] : 0;
  if (LUT) s_tab[tid] = lut[tid] ^ 0x80;
  u64* list = &s_list[0][tid];
  knn_list_init<kScanThreads>(list);
  __syncthreads();
  u64 thr = kNoKey;                                       // list[k - 1] of this lane's row
  const long w = (long)blockIdx.x * kScanWaves + wave, nw = (long)gridDim.x * kScanWaves;
  const long t0 = w * tiles / nw, t1 = (w + 1) * tiles / nw;       // tiles < 2^27, nw <= 2048: no overflow
  const uint4* qa = qs + lane;
  // the wave's tiles in ceil(n / kNT) walks of equal size (+-1 tile)
  const int n = (int)(t1 - t0), walks = (n + kNT - 1) / kNT;
  long t = t0;
  for (int u = 0; u < walks; ++u) {
    const int cnt = n / walks + (u < n % walks ? 1 : 0);
    switch (cnt) {
      case 1: nn_unit<RT, LUT, 1>(frames, F, D, KS, t, qa, s_tab, s_qn, s_stage[wave], list, thr, M, k); break;
      case 2: nn_unit<RT, LUT, 2>(frames, F, D, KS, t, qa, s_tab, s_qn, s_stage[wave], list, thr, M, k); break;
      case 3: nn_unit<RT, LUT, 3>(frames, F, D, KS, t, qa, s_tab, s_qn, s_stage[wave], list, thr, M, k); break;
      default: nn_unit<RT, LUT, 4>(frames, F, D, KS, t, qa, s_tab, s_qn, s_stage[wave], list, thr, M, k); break;
    }
    t += cnt;
  }
  if (lane < M) knn_list_store<kScanThreads>(lists + (w * M + lane) * (long)k, list, k);
}

// ---- merge.  grid M, 256 threads
__global__ __launch_bounds__(256) void nn_merge_kernel(const u64* __restrict__ lists, int nlists, int M, int k, int* __restrict__ out_dist,
                                                       long long* __restrict__ out_index) {
  __shared__ u64 red[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  u64 prev = 0;
  for (int j = 0; j < k; ++j) {
    u64 best = wave_min64(knn_merge_pick(lists, nlists, M, m, k, j, prev, tid, 256));
    __syncthreads();                                    // the previous round's red[] has been read
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    best = red[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) if (red[i] < best) best = red[i];
    if (tid == 0) {
      out_dist[m * k + j] = knn_key_dist(best);
      out_index[m * k + j] = knn_key_index(best);
    }
    prev = best;
  }
}

template <int RT>
void launch_scan(bool with_lut, const Plan& p, const unsigned char* frames, long F, int D, const uint4* qs, const int* qn,
                 const unsigned char* lut, int M, int k, u64* lists, hipStream_t s) {
  if (with_lut)
    hipLaunchKernelGGL((nn_scan_kernel<RT, true>), dim3((unsigned)p.blocks), dim3(kScanThreads), 0, s, frames, F, D, p.KS, p.tiles, qs, qn, lut, M,
                       k, lists);
  else
    hipLaunchKernelGGL((nn_scan_kernel<RT, false>), dim3((unsigned)p.blocks), dim3(kScanThreads), 0, s, frames, F, D, p.KS, p.tiles, qs, qn, lut, M,
                       k, lists);
}

// the shape contract of both entry points; 0 when the shape is served
int check_shape(const char* who, int M, long F, int D, int k) {
  if (M < 1) { set_error("%s: M=%d must be positive", who, M); return MMVAE_ERR_ARG; }
  if (F < 1) { set_error("%s: F=%ld must be positive", who, F); return MMVAE_ERR_ARG; }
  if (const int rc = knn_check_signs(who, D, k, 1)) return rc;
  if (M > kMaxM) { set_error("%s: M=%d unsupported (1..%d queries)", who, M, kMaxM); return MMVAE_ERR_UNSUPPORTED; }
  if (const int rc = knn_check_limits(who, D, k, 1)) return rc;
  if (F > 2147483647L) { set_error("%s: F=%ld unsupported (at most 2^31 - 1 frames)", who, F); return MMVAE_ERR_UNSUPPORTED; }
  if (k > F) { set_error("%s: k=%d exceeds F=%ld", who, k, F); return MMVAE_ERR_ARG; }
  return 0;
}

}  // namespace

size_t nearest_frames_scratch_bytes(int M, long F, int D, int k) {
  if (check_shape("nearest_frames_scratch_bytes", M, F, D, k) != 0) return 0;
  return make_plan(M, F, D, k).total;
}

int launch_nearest_frames(const unsigned char* queries, int M, const unsigned char* frames, long F, int D, const unsigned char* lut, int k,
                          int* out_dist, long long* out_index, void* scratch, size_t scratch_bytes, hipStream_t s) {
  int rc = check_shape("nearest_frames", M, F, D, k);
  if (rc != 0) return rc;
  const Plan p = make_plan(M, F, D, k);
  rc = knn_check_buffers("nearest_frames", {{"queries", queries}, {"frames", frames}, {"out_dist", out_dist}, {"out_index", out_index},
                                            {"scratch", scratch}}, scratch_bytes, p.total);
  if (rc != 0) return rc;
  uint4* qs = knn_carve<uint4>(scratch, 0);
  int* qn = knn_carve<int>(scratch, p.qn_off);
  u64* lists = knn_carve<u64>(scratch, p.lists_off);
  hipLaunchKernelGGL(nn_prep_kernel, dim3((unsigned)p.RT), dim3(256), 0, s, queries, M, D, p.KS, qs, qn);
  int e = check_launch("nearest_frames (prep)");
  if (e != 0) return e;
  switch (p.RT) {
    case 1: launch_scan<1>(lut != nullptr, p, frames, F, D, qs, qn, lut, M, k, lists, s); break;
    case 2: launch_scan<2>(lut != nullptr, p, frames, F, D, qs, qn, lut, M, k, lists, s); break;
    case 3: launch_scan<3>(lut != nullptr, p, frames, F, D, qs, qn, lut, M, k, lists, s); break;
    default: launch_scan<4>(lut != nullptr, p, frames, F, D, qs, qn, lut, M, k, lists, s); break;
  }
  note_launch_bytes((double)F * D);
  e = check_launch("nearest_frames (scan)");
  if (e != 0) return e;
  hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)M), dim3(256), 0, s, lists, p.lists, M, k, out_dist, out_index);
  return check_launch("nearest_frames (merge)");
}

}  // namespace mmvae
