// Set-to-set exact k-NN and ball counts: every row of a [Na][D] uint8 against every row of b [Nb][D] uint8 (mmvae_knn_cross).
//
//   d(i, j) = sum_t (a[i][t] - b[j][t])^2 in exact integers.  With x' = x ^ 0x80 read as int8 on both sides,
//   d = |a'|^2 + |b'|^2 - 2 a'.b', and the cross term is a tiled int8 GEMM on v_mfma_i32_16x16x64_i8; every term stays below 2^31.
//
// Three launches:
//   kc_norm_kernel   |a'|^2 and |b'|^2 of every row (v_dot4_i32_i8), a wave per row, into scratch.
//   kc_sweep_kernel  a block of four waves owns a tile of kTile = 128 rows of `a` and a contiguous range of 128-column tiles of `b`
//                    (dealt out so that the blocks of one XCD share tiles in its L2, see the kernel).  Per column tile it walks D in chunks of 128 bytes: every thread
//                    loads 4 + 4 16-byte pieces into registers (the next chunk's loads are in flight during this chunk's products), turns
//                    them to signed bytes (zeros past D) and stores them to LDS in the operand fragment order (knn_select.hpp), 16-row
//                    tile t and k step u at [t][u][lane].  Stores and loads are lane-contiguous 16-byte accesses: no bank conflicts.
//                    A wave owns a 64 x 64 quarter of the block tile, 4 x 4 accumulator tiles: per k step it reads 4 A and 4 B fragments
//                    for 16 MFMAs.
//                    Epilogue per column tile: d from the norms; the ball test d <= col_radius[j] adds to 16 per-lane counters (one per
//                    (row tile, reg)); the selection (knn_select.hpp): lane l of a wave owns row l of the wave's 64, one ballot per four
//                    rows rejects the common case.  At the end of the range every wave writes one list and one count per row to
//                    scratch: `parts` = 2 x ranges partial results per row (the two waves side by side in a block keep separate lists).
//   kc_merge_kernel  a wave per row: the k merge rounds over the row's parts x k keys, and the integer sum of its partial counts.
// Operand order, key, list and tie rule are defined in knn_select.hpp; the counts are integer sums: the same bits every run, for any
// split of the columns.
#include "common.hpp"
#include "kernels.hpp"
#include "knn_select.hpp"

namespace mmvae {

namespace {

constexpr long kMaxN = 1L << 20;
constexpr int kTile = 128;                             // rows of a and columns of b in a block tile
constexpr int kThreads = 256;
constexpr int kTargetBlocks = 2048;                    // a few rounds of two blocks per CU: the tail round stays small
constexpr int kMaxRanges = 128;

struct Plan {
  int row_tiles, col_tiles, ranges, parts;
  size_t bn_off, lists_off, counts_off, total;
};

Plan make_plan(long Na, long Nb, int k, bool want_count) {
  Plan p;
  p.row_tiles = (int)((Na + kTile - 1) / kTile);
  p.col_tiles = (int)((Nb + kTile - 1) / kTile);
  int r = (kTargetBlocks + p.row_tiles - 1) / p.row_tiles;
  r = r < kMaxRanges ? r : kMaxRanges;
  p.ranges = r < p.col_tiles ? r : p.col_tiles;
  p.parts = 2 * p.ranges;
  auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
  p.bn_off = up16((size_t)Na * sizeof(int));
  p.lists_off = p.bn_off + up16((size_t)Nb * sizeof(int));
  p.counts_off = p.lists_off + (size_t)p.parts * Na * k * sizeof(u64);
  p.total = p.counts_off + (want_count ? up16((size_t)p.parts * Na * sizeof(int)) : 0);
  return p;
}

// ---- row norms of a and b in the signed space.  A wave per row; grid ceil((Na + Nb) / 4), 256 threads
__global__ __launch_bounds__(256) void kc_norm_kernel(const unsigned char* __restrict__ a, long Na, const unsigned char* __restrict__ b, long Nb,
                                                      int D, int* __restrict__ an, int* __restrict__ bn) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= Na + Nb) return;
  const unsigned char* src = row < Na ? a + row * D : b + (row - Na) * D;
  int n = 0;
  for (int off = lane * 16; off < D; off += 64 * 16) {
    uint4 v = *reinterpret_cast<const uint4*>(src + off);
    n = signed_norm16(v, n);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if (lane == 0) {
    if (row < Na) an[row] = n;
    else bn[row - Na] = n;
  }
}

// 16-byte piece `off` of a row as it lies in memory; at and past D the row's last piece stands in (kc_signed drops it).  The load is
// unconditional and its value is not touched before the LDS store of the next chunk, so it stays in flight during this chunk's products.
__device__ __forceinline__ u32x4_t kc_piece(const unsigned char* row, int off, int D) {
  return *reinterpret_cast<const u32x4_t*>(row + (off < D ? off : D - 16));
}
// ... as signed bytes; zeros at and past D (they add nothing to the product)
__device__ __forceinline__ u32x4_t kc_signed(u32x4_t v, int off, int D) {
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  return off < D ? (v ^ 0x80808080u) : zero;
}

__global__ __launch_bounds__(kThreads, 2) void kc_sweep_kernel(const unsigned char* __restrict__ a, int Na, const unsigned char* __restrict__ b,
                                                               int Nb, int D, int row_tiles, int col_tiles, int ranges, const int* __restrict__ an,
                                                               const int* __restrict__ bn, const int* __restrict__ col_radius, int k,
                                                               int exclude_diagonal, u64* __restrict__ lists, int* __restrict__ counts) {
  __shared__ u64 s_list[kMaxK][kThreads];                 // [j][thread]: the j-th best key of the row that thread's lane owns
  __shared__ u32x4_t s_a[16 * 64], s_b[16 * 64];           // [16-row tile t][k step u][lane]: 8 x 2 fragments a side
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, grp = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wave >> 1, wc = wave & 1;
  // Which (row tile, column range) this block owns.  Blocks go to the 8 XCDs round-robin by their index, and each XCD has an L2 of its
  // own: the longer of the two axes is dealt out over the XCDs (index & 7), the other one runs fastest inside an XCD, so that the blocks
  // resident on an XCD together share a few row tiles and a few column tiles and most of their loads hit its L2.
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const bool deal_rows = row_tiles >= ranges;
  const int fast = deal_rows ? ranges : row_tiles, dealt = (slot / fast) * 8 + xcd;
  const int row_tile = deal_rows ? dealt : slot % fast, range = deal_rows ? slot % fast : dealt;
  if (row_tile >= row_tiles || range >= ranges) return;   // the padding of the dealt axis to a multiple of 8 (uniform over the block)
  const int row0 = row_tile * kTile + wr * 64;            // the first row of this wave's quarter
  u64* list = &s_list[0][tid];
  knn_list_init<kThreads>(list);
  u64 thr = kNoKey;                                       // list[k - 1] of this lane's row
  int cnt[4][4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) cnt[rt][r] = 0;
  // staging: wave w fills fragments 4 w .. 4 w + 3 of either side, i.e. 16-row tiles 2 w and 2 w + 1, both k steps: whole 128-byte lines
  const unsigned char* ap[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    long r = (long)row_tile * kTile + (2 * wave + h) * 16 + col;
    if (r > Na - 1) r = Na - 1;                           // a row past the end reads the last row; its keys are dropped
    ap[h] = a + r * (long)D;
  }
  const int chunks = (D + 127) / 128;
  const int t0 = (int)((long)range * col_tiles / ranges), t1 = (int)((long)(range + 1) * col_tiles / ranges);
  for (int ct = t0; ct < t1; ++ct) {
    const unsigned char* bp[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      long r = (long)ct * kTile + (2 * wave + h) * 16 + col;
      if (r > Nb - 1) r = Nb - 1;
      bp[h] = b + r * (long)D;
    }
    i32x4 acc[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[rt][nt] = i32x4{0, 0, 0, 0};
    u32x4_t pa[4], pb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      pa[q] = kc_piece(ap[q >> 1], (q & 1) * 64 + grp * 16, D);
      pb[q] = kc_piece(bp[q >> 1], (q & 1) * 64 + grp * 16, D);
    }
    for (int c = 0; c < chunks; ++c) {
      __syncthreads();                                    // the previous chunk's fragments have been read
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int off = c * 128 + (q & 1) * 64 + grp * 16;
        s_a[(4 * wave + q) * 64 + lane] = kc_signed(pa[q], off, D);
        s_b[(4 * wave + q) * 64 + lane] = kc_signed(pb[q], off, D);
      }
      __syncthreads();
      if (c + 1 < chunks) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          pa[q] = kc_piece(ap[q >> 1], (c + 1) * 128 + (q & 1) * 64 + grp * 16, D);
          pb[q] = kc_piece(bp[q >> 1], (c + 1) * 128 + (q & 1) * 64 + grp * 16, D);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (u == 1 && c * 128 + 64 >= D) break;           // the whole second step lies past D (uniform)
        i32x4 fa[4], fb[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
          const u32x4_t v = s_a[((wr * 4 + rt) * 2 + u) * 64 + lane];
          fa[rt] = i32x4{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const u32x4_t v = s_b[((wc * 4 + nt) * 2 + u) * 64 + lane];
          fb[nt] = i32x4{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) acc[rt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[rt], fb[nt], acc[rt][nt], 0, 0, 0);
      }
    }
    // ---- epilogue: distances, ball test, selection.  This lane's columns are j0 + 16 nt, its rows row0 + 16 rt + 4 grp + r
    const int j0 = ct * kTile + wc * 64 + col;
    int bnorm[4], rad[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int j = j0 + 16 * nt;
      bnorm[nt] = j < Nb ? bn[j] : 0;
      rad[nt] = (col_radius && j < Nb) ? col_radius[j] : -1;      // d >= 0: a column past the end is in nobody's ball
    }
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = row0 + rt * 16 + grp * 4 + r;
        const int anorm = i < Na ? an[i] : 0;
        const u64 last = shfl64(thr, rt * 16 + grp * 4 + r);
        u64 cand[4];
        bool hit = false;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int j = j0 + 16 * nt;
          const int d = anorm + bnorm[nt] - 2 * acc[rt][nt][r];
          const bool live = i < Na && j < Nb && !(exclude_diagonal && i == j);
          cnt[rt][r] += (live && d <= rad[nt]) ? 1 : 0;
          cand[nt] = live ? knn_key(d, (uint32_t)j) : kNoKey;
          hit |= cand[nt] < last;
        }
        if (k > 0 && __ballot(hit)) knn_insert<4, kThreads>(cand, rt, r, list, thr, k);
      }
    }
  }
  // ---- one list and one count per row of this wave's quarter; part = 2 range + wave column
  const long part = (long)range * 2 + wc;
  if (k > 0 && row0 + lane < Na) knn_list_store<kThreads>(lists + (part * Na + row0 + lane) * (long)k, list, k);
  if (counts) {
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int v = cnt[rt][r];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);          // over the 16 columns of the lane group
        const int i = row0 + rt * 16 + grp * 4 + r;
        if (col == 0 && i < Na) counts[part * Na + i] = v;
      }
  }
}

// ---- merge.  A wave per row; grid ceil(Na / 4), 256 threads
__global__ __launch_bounds__(256) void kc_merge_kernel(const u64* __restrict__ lists, const int* __restrict__ counts, int parts, int Na, int k,
                                                       int* __restrict__ out_dist, long long* __restrict__ out_index,
                                                       int* __restrict__ out_count) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= Na) return;
  u64 prev = 0;
  for (int j = 0; j < k; ++j) {
    const u64 best = wave_min64(knn_merge_pick(lists, parts, Na, i, k, j, prev, lane, 64));
    if (lane == 0) {
      out_dist[(long)i * k + j] = knn_key_dist(best);
      out_index[(long)i * k + j] = knn_key_index(best);
    }
    prev = best;
  }
  if (out_count) {
    int n = 0;
    for (int p = lane; p < parts; p += 64) n += counts[(long)p * Na + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) out_count[i] = n;
  }
}

// the shape contract of both entry points; 0 when the shape is served
int check_shape(const char* who, long Na, long Nb, int D, int k) {
  if (Na < 1) { set_error("%s: Na=%ld must be positive", who, Na); return MMVAE_ERR_ARG; }
  if (Nb < 1) { set_error("%s: Nb=%ld must be positive", who, Nb); return MMVAE_ERR_ARG; }
  if (const int rc = knn_check_signs(who, D, k, 0)) return rc;
  if (Na > kMaxN) { set_error("%s: Na=%ld unsupported (1..%ld rows)", who, Na, kMaxN); return MMVAE_ERR_UNSUPPORTED; }
  if (Nb > kMaxN) { set_error("%s: Nb=%ld unsupported (1..%ld rows)", who, Nb, kMaxN); return MMVAE_ERR_UNSUPPORTED; }
  if (const int rc = knn_check_limits(who, D, k, 0)) return rc;
  if (k > Nb) { set_error("%s: k=%d exceeds Nb=%ld", who, k, Nb); return MMVAE_ERR_ARG; }
  return 0;
}

}  // namespace

size_t knn_cross_scratch_bytes(long Na, long Nb, int D, int k, int want_count) {
  if (check_shape("knn_cross_scratch_bytes", Na, Nb, D, k) != 0) return 0;
  if (k == 0 && !want_count) { set_error("knn_cross_scratch_bytes: k=0 and no count: nothing is asked for"); return 0; }
  return make_plan(Na, Nb, k, want_count != 0).total;
}

int launch_knn_cross(const unsigned char* a, long Na, const unsigned char* b, long Nb, int D, int k, int exclude_diagonal, int* out_dist,
                     long long* out_index, const int* col_radius, int* out_count, void* scratch, size_t scratch_bytes, hipStream_t s) {
  int rc = check_shape("knn_cross", Na, Nb, D, k);
  if (rc != 0) return rc;
  if (exclude_diagonal && k > Nb - 1) { set_error("knn_cross: k=%d exceeds the Nb-1=%ld columns left without the diagonal", k, Nb - 1); return MMVAE_ERR_ARG; }
  if ((col_radius != nullptr) != (out_count != nullptr)) {
    set_error("knn_cross: col_radius=%p and out_count=%p go together", (const void*)col_radius, (void*)out_count);
    return MMVAE_ERR_ARG;
  }
  if (k > 0 ? (!out_dist || !out_index) : (out_dist || out_index)) {
    set_error("knn_cross: out_dist=%p and out_index=%p are both given with k > 0 and both NULL with k=0 (k=%d)", (void*)out_dist, (void*)out_index, k);
    return MMVAE_ERR_ARG;
  }
  if (k == 0 && !out_count) { set_error("knn_cross: k=0 and no out_count: nothing is asked for"); return MMVAE_ERR_ARG; }
  const Plan p = make_plan(Na, Nb, k, out_count != nullptr);
  rc = knn_check_buffers("knn_cross", {{"a", a}, {"b", b}, {"scratch", scratch}}, scratch_bytes, p.total);
  if (rc != 0) return rc;
  int* an = knn_carve<int>(scratch, 0);
  int* bn = knn_carve<int>(scratch, p.bn_off);
  u64* lists = knn_carve<u64>(scratch, p.lists_off);
  int* counts = out_count ? knn_carve<int>(scratch, p.counts_off) : nullptr;
  hipLaunchKernelGGL(kc_norm_kernel, dim3((unsigned)((Na + Nb + 3) / 4)), dim3(256), 0, s, a, Na, b, Nb, D, an, bn);
  int e = check_launch("knn_cross (norms)");
  if (e != 0) return e;
  const int dealt = p.row_tiles >= p.ranges ? p.row_tiles : p.ranges, fast = p.row_tiles >= p.ranges ? p.ranges : p.row_tiles;
  const unsigned blocks = 8u * (unsigned)((dealt + 7) / 8) * (unsigned)fast;             // at most 8 * 1024 * 128
  hipLaunchKernelGGL(kc_sweep_kernel, dim3(blocks), dim3(kThreads), 0, s, a, (int)Na, b, (int)Nb, D, p.row_tiles, p.col_tiles, p.ranges, an, bn,
                     col_radius, k, exclude_diagonal, lists, counts);
  note_launch_bytes((double)(Na + Nb) * D);
  e = check_launch("knn_cross (sweep)");
  if (e != 0) return e;
  hipLaunchKernelGGL(kc_merge_kernel, dim3((unsigned)((Na + 3) / 4)), dim3(256), 0, s, lists, counts, p.parts, (int)Na, k, out_dist, out_index,
                     out_count);
  return check_launch("knn_cross (merge)");
}

}  // namespace mmvae
