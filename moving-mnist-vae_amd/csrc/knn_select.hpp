// What the two exact k-NN paths share (neighbours.hip: a few queries over all frames; knn_cross.hip: set against set): the key, the
// k-best list and its insertion, the merge round, the signed-byte norm and the tail of the argument contract.  Included by those two only.
//
// Operand fragment order (v_mfma_i32_16x16x64_i8), the same for A and B: the fragment of (16-row tile t, 64-byte k step u) holds, for
// lane l, bytes [64 u + 16 (l >> 4), +16) of row 16 t + (l & 15) -- one lane -> (row, k) map on both sides, so the k order inside a
// step, whatever the hardware makes of it, is the same for both operands (a sum over k does not care).  C/D: col = l & 15,
// row = 4 (l >> 4) + reg.  Bytes are compared as x' = x ^ 0x80 read as int8 (= x - 128): d = |a'|^2 + |b'|^2 - 2 a'.b'.
//
// Key, list, tie rule: a candidate is the key (d << 32) | index, so one unsigned compare is the order (d, index) and equal distances go
// to the lower index; keys are distinct (each holds its index), kNoKey = ~0 is above all of them and marks an unused slot.  A wave keeps,
// per row, a sorted list of the k smallest keys it has seen; the lists of all parts of a row lie in scratch as
// lists[(part * rows + row) * k + j], and the merge takes the k smallest of their union in k rounds of "smallest key above the last one
// chosen".  The outputs are therefore a function of the inputs alone, for any split of the columns.
#pragma once
#include <initializer_list>

#include "common.hpp"

namespace mmvae {

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef unsigned long long u64;

constexpr int kMaxK = 8, kMaxD = 16384;
constexpr u64 kNoKey = ~0ull;

__device__ __forceinline__ u64 knn_key(int d, u64 index) { return ((u64)(uint32_t)d << 32) | index; }
__device__ __forceinline__ int knn_key_dist(u64 key) { return (int)(key >> 32); }
__device__ __forceinline__ long long knn_key_index(u64 key) { return (long long)(key & 0xffffffffull); }

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  return ((u64)(uint32_t)__shfl((int)(v >> 32), src, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src, 64);
}
__device__ __forceinline__ u64 wave_min64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 other = ((u64)(uint32_t)__shfl_xor((int)(v >> 32), o, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
    if (other < v) v = other;
  }
  return v;
}

// 16 bytes of a row to signed bytes, in place; returns acc + the sum of their squares (v_dot4_i32_i8)
__device__ __forceinline__ int signed_norm16(uint4& v, int acc) {
  v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
  acc = __builtin_amdgcn_sdot4((int)v.x, (int)v.x, acc, false);
  acc = __builtin_amdgcn_sdot4((int)v.y, (int)v.y, acc, false);
  acc = __builtin_amdgcn_sdot4((int)v.z, (int)v.z, acc, false);
  return __builtin_amdgcn_sdot4((int)v.w, (int)v.w, acc, false);
}

// A thread's list is a column of a [kMaxK][STRIDE] LDS array (no bank conflicts, nobody else touches it): list[j * STRIDE].
template <int STRIDE>
__device__ __forceinline__ void knn_list_init(u64* list) {
#pragma unroll
  for (int j = 0; j < kMaxK; ++j) list[j * STRIDE] = kNoKey;
}
template <int STRIDE>
__device__ __forceinline__ void knn_list_store(u64* __restrict__ dst, const u64* list, int k) {
  for (int j = 0; j < k; ++j) dst[j] = list[j * STRIDE];
}

// The k-best lists of a wave that owns up to 64 rows: lane l owns row l, its sorted keys in `list`, the k-th of them also in the
// register `thr`.  The keys cand[nt] of (row tile rt, accumulator register r) -- the row of lane group g is 16 rt + 4 g + r, so the four
// groups hold four different rows -- go in, one per group and turn: the first lane of a group with a key below its row's `thr` offers
// its smallest, the row's owner fetches it and shifts its list.  `thr` is fetched afresh every turn: an insertion may have lowered it.
template <int CNT, int STRIDE>
__device__ __forceinline__ void knn_insert(u64 (&cand)[CNT], int rt, int r, u64* list, u64& thr, int k) {
  const int lane = threadIdx.x & 63, grp = lane >> 4, row = rt * 16 + grp * 4 + r;
  const int og = (lane >> 2) & 3;                         // the lane group whose row this lane owns, if it owns one of these four rows
  const bool owner = (lane >> 4) == rt && (lane & 3) == r;
  for (;;) {
    const u64 t = shfl64(thr, row);
    u64 best = cand[0];
#pragma unroll
    for (int nt = 1; nt < CNT; ++nt) best = cand[nt] < best ? cand[nt] : best;
    const bool c = best < t;
    const u64 m = __ballot(c);
    if (!m) break;
    const unsigned mine = (unsigned)(m >> (16 * grp)) & 0xffffu, theirs = (unsigned)(m >> (16 * og)) & 0xffffu;
    const u64 nk = shfl64(best, 16 * og + (theirs ? __builtin_ctz(theirs) : 0));
    if (mine && (lane & 15) == __builtin_ctz(mine)) {     // the offered key leaves its lane (keys are distinct)
#pragma unroll
      for (int nt = 0; nt < CNT; ++nt) cand[nt] = cand[nt] == best ? kNoKey : cand[nt];
    }
    if (owner && theirs) {                                // nk is below list[k - 1]: it goes in, the last key drops out
      u64 e[kMaxK];
#pragma unroll
      for (int j = 0; j < kMaxK; ++j) e[j] = list[j * STRIDE];
#pragma unroll
      for (int j = kMaxK - 1; j > 0; --j) e[j] = e[j] < nk ? e[j] : (e[j - 1] < nk ? nk : e[j - 1]);
      e[0] = e[0] < nk ? e[0] : nk;
#pragma unroll
      for (int j = 0; j < kMaxK; ++j) {
        list[j * STRIDE] = e[j];
        thr = j == k - 1 ? e[j] : thr;
      }
    }
  }
}

// Round j of a merge, one thread's share: the smallest of `row`'s parts * k keys above `prev`, the key round j - 1 chose.  The caller
// takes the minimum over its threads; kNoKey is never chosen because at least k columns are in reach of every row.
__device__ __forceinline__ u64 knn_merge_pick(const u64* __restrict__ lists, int parts, int rows, int row, int k, int j, u64 prev, int tid,
                                              int nthreads) {
  u64 best = kNoKey;
  for (int i = tid; i < parts * k; i += nthreads) {
    const u64 v = lists[((long)(i / k) * rows + row) * k + i % k];
    if ((j == 0 || v > prev) && v < best) best = v;
  }
  return best;
}

// ---- host: what both argument contracts share, worded by the entry point's name `who`.  0 when served.
// D and k in the order both report them: signs first (kmin, 0 or 1, is the least k served), then, behind the row counts, the limits.
int knn_check_signs(const char* who, int D, int k, int kmin) {
  if (D < 1) { set_error("%s: D=%d must be positive", who, D); return MMVAE_ERR_ARG; }
  if (k < kmin) { set_error("%s: k=%d must %s", who, k, kmin ? "be positive" : "not be negative"); return MMVAE_ERR_ARG; }
  return 0;
}
int knn_check_limits(const char* who, int D, int k, int kmin) {
  if (k > kMaxK) { set_error("%s: k=%d unsupported (%d..%d neighbours)", who, k, kmin, kMaxK); return MMVAE_ERR_UNSUPPORTED; }
  if (D % 16 != 0 || D > kMaxD) { set_error("%s: D=%d unsupported (a multiple of 16 in 16..%d)", who, D, kMaxD); return MMVAE_ERR_UNSUPPORTED; }
  return 0;
}
// The buffers: the first NULL of `ptrs` is named; the first two (the row operands) and the last (scratch) are 16-byte aligned; scratch
// holds the `need` bytes of the plan.
struct NamedPtr { const char* name; const void* p; };
int knn_check_buffers(const char* who, std::initializer_list<NamedPtr> ptrs, size_t scratch_bytes, size_t need) {
  for (const NamedPtr& a : ptrs)
    if (!a.p) { set_error("%s: NULL %s", who, a.name); return MMVAE_ERR_ARG; }
  const NamedPtr *x = ptrs.begin(), *y = x + 1, *scratch = ptrs.end() - 1;
  if (((uintptr_t)x->p | (uintptr_t)y->p | (uintptr_t)scratch->p) & 15) {
    set_error("%s: %s=%p, %s=%p and scratch=%p must be 16-byte aligned", who, x->name, x->p, y->name, y->p, scratch->p);
    return MMVAE_ERR_ARG;
  }
  if (scratch_bytes < need) { set_error("%s: scratch_bytes=%zu below the %zu this shape needs", who, scratch_bytes, need); return MMVAE_ERR_WORKSPACE; }
  return 0;
}
template <typename T>
T* knn_carve(void* scratch, size_t off) { return reinterpret_cast<T*>(static_cast<unsigned char*>(scratch) + off); }

}  // namespace

}  // namespace mmvae
