// Byte histogram of the resident uint8 dataset: the one device pass behind fit_quantiser (main.py).  Everything the reference
// derives by sampling in utils.save_kmeans_file (utils.py:279-309) -- the k-means fit, the label mean / std, the class ratios --
// is an exact function of these 256 counts (quantiser_fit.cpp).
//
// Work decomposition.  The input is n_clips ranges of clip_bytes bytes (the contiguous form is ONE range of all the bytes); each
// range is cut into `parts` pieces of `piece` bytes (a multiple of 16, so every piece of a clip has the clip's alignment) and the
// blocks stride over the (clip, part) items.  Inside an item the bytes up to the first 16-byte boundary and behind the last one
// are counted one byte per thread; the body is read as 16-byte vectors, four in flight per thread.
//
// Skew.  Moving-MNIST is > 90 % background: with one atomicAdd(&lds[b], 1) per byte all 64 lanes of a wave hit the word of bin 0
// and the LDS serialises them.  What this kernel does instead, chosen by measurement (the table of DESIGN.md 4.14: variants timed
// against each other in one process on 819 MB; tools/quantiser_bench.py times the shipped kernel against torch.bincount):
//   - zeros never reach the LDS: a 32-bit word that is zero adds 4 to a per-thread register, a zero byte in a mixed word adds 1;
//     the registers are summed over the wave by shuffles and reach bin 0 once per wave at the end;
//   - a non-zero word of four equal bytes (saturated strokes, constant images) is ONE atomic of 4;
//   - the block's histogram is kept in kReplicas copies, lane l using copy l % kReplicas, interleaved ([bin][copy]) so the copies of
//     one bin sit on neighbouring banks: the same-address serialisation left for a constant non-zero image drops from 64 lanes to
//     64 / kReplicas, and on uniform bytes two lanes collide on a bank only when their bins agree modulo 4 AND their copies agree.
// Measured against (GB/s of input, Moving-MNIST-like 92 % zeros / uniform bytes / all 255): the naive per-byte LDS atomic with one
// copy 329 / 3803 / 303 and with 8 copies 2384 / 5186 / 2391; the register + equal-word aggregation with one copy 4361 / 3282 / 1197,
// with 8 copies (this kernel) 4278 / 4117 / 5694, with 16 the same within 1 %, with 32 slower (3623 / 3597 / 5606).  One copy is 2 %
// ahead on the skewed data and far behind elsewhere; 8 is the fewest copies that repairs that.
//
// Counters.  LDS counters and the zero registers are 32-bit.  A block counts at most ceil(n_items / grid) * piece bytes, which the
// launch arithmetic below keeps <= 2^31, so none can wrap.  Each block flushes once: thread b adds the copies of bin b and, if the
// sum is non-zero, issues one 64-bit vector atomicAdd to counts[b].  Integer adds commute: the result is the same bits every run.
#include "common.hpp"
#include "kernels.hpp"

namespace mmvae {

namespace {

constexpr int kHistThreads = 256;              // one thread per bin in the flush
constexpr int kReplicas = 8;                   // copies of the block histogram (a power of two)
constexpr long kMaxPiece = 64 << 10;           // bytes of one work item (a multiple of 16)
constexpr long kBlockShare = 1l << 31;         // most bytes one block may count (32-bit counters)

__device__ __forceinline__ void count_byte(unsigned* hist, unsigned b, unsigned rep, unsigned& zeros) {
  if (b == 0) ++zeros;
  else atomicAdd(&hist[b * kReplicas + rep], 1u);
}

__device__ __forceinline__ void count_word(unsigned* hist, unsigned w, unsigned rep, unsigned& zeros) {
  if (w == 0) { zeros += 4; return; }
  const unsigned b0 = w & 0xffu;
  if (w == b0 * 0x01010101u) { atomicAdd(&hist[b0 * kReplicas + rep], 4u); return; }
  count_byte(hist, b0, rep, zeros);
  count_byte(hist, (w >> 8) & 0xffu, rep, zeros);
  count_byte(hist, (w >> 16) & 0xffu, rep, zeros);
  count_byte(hist, w >> 24, rep, zeros);
}

__device__ __forceinline__ void count_vec(unsigned* hist, const uint4& v, unsigned rep, unsigned& zeros) {
  if ((v.x | v.y | v.z | v.w) == 0) { zeros += 16; return; }
  count_word(hist, v.x, rep, zeros);
  count_word(hist, v.y, rep, zeros);
  count_word(hist, v.z, rep, zeros);
  count_word(hist, v.w, rep, zeros);
}

// clip_index == nullptr: clip i starts at frames + i * clip_bytes
__global__ __launch_bounds__(kHistThreads) void u8_histogram_kernel(const unsigned char* __restrict__ frames, long clip_bytes,
                                                                     const long long* __restrict__ clip_index, long n_items, long parts,
                                                                     long piece, unsigned long long* __restrict__ counts) {
  __shared__ unsigned hist[256 * kReplicas];
  const int tid = threadIdx.x;
  for (int i = tid; i < 256 * kReplicas; i += kHistThreads) hist[i] = 0;
  __syncthreads();
  const unsigned rep = (unsigned)tid & (kReplicas - 1);
  unsigned zeros = 0;
  for (long item = blockIdx.x; item < n_items; item += gridDim.x) {
    const long clip = item / parts, lo = (item - clip * parts) * piece;
    const long nbytes = min(piece, clip_bytes - lo);
    if (nbytes <= 0) continue;
    const unsigned char* p = frames + (clip_index ? (long)clip_index[clip] : clip) * clip_bytes + lo;
    const long head = min((long)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15), nbytes);
    const long nvec = (nbytes - head) >> 4;
    const long tail = nbytes - head - (nvec << 4);
    if (tid < head) count_byte(hist, p[tid], rep, zeros);
    if (tid < tail) count_byte(hist, p[head + (nvec << 4) + tid], rep, zeros);
    const uint4* v = reinterpret_cast<const uint4*>(p + head);
    long i = tid;
    for (; i + 3 * kHistThreads < nvec; i += 4 * kHistThreads) {
      const uint4 a = v[i], b = v[i + kHistThreads], c = v[i + 2 * kHistThreads], d = v[i + 3 * kHistThreads];
      count_vec(hist, a, rep, zeros);
      count_vec(hist, b, rep, zeros);
      count_vec(hist, c, rep, zeros);
      count_vec(hist, d, rep, zeros);
    }
    for (; i < nvec; i += kHistThreads) count_vec(hist, v[i], rep, zeros);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) zeros += __shfl_xor(zeros, o, 64);
  if ((tid & 63) == 0 && zeros) atomicAdd(&hist[(tid >> 6) & (kReplicas - 1)], zeros);        // bin 0, one copy per wave
  __syncthreads();
  unsigned sum = 0;
#pragma unroll
  for (int r = 0; r < kReplicas; ++r) sum += hist[tid * kReplicas + r];
  if (sum) atomicAdd(&counts[tid], (unsigned long long)sum);
}

}  // namespace

int launch_u8_histogram(const unsigned char* frames, long clip_bytes, const long long* clip_index, long n_clips,
                        unsigned long long* counts, hipStream_t s) {
  if (n_clips < 0 || clip_bytes < 0) { set_error("u8_histogram: negative size"); return MMVAE_ERR_ARG; }
  if (n_clips == 0 || clip_bytes == 0) return MMVAE_OK;
  if (!frames || !counts) { set_error("u8_histogram: NULL frames or counts"); return MMVAE_ERR_ARG; }
  if (clip_bytes > INT64_MAX / n_clips) { set_error("u8_histogram: n_clips * clip_bytes overflows 64 bits"); return MMVAE_ERR_ARG; }
  if (!clip_index) { clip_bytes *= n_clips; n_clips = 1; }          // contiguous: one range
  // pieces of equal size, a multiple of 16, at most kMaxPiece
  const long parts = (clip_bytes + kMaxPiece - 1) / kMaxPiece;
  const long piece = ((clip_bytes + parts - 1) / parts + 15) & ~15l;
  if (parts > INT64_MAX / n_clips) { set_error("u8_histogram: too many work items"); return MMVAE_ERR_ARG; }
  const long n_items = n_clips * parts;
  // A block counts at most ceil(n_items / grid) * piece bytes.  per_block = floor(kBlockShare / piece) items (>= 32768) keep that
  // <= kBlockShare = 2^31 < 2^32, so no 32-bit counter can wrap; the grid is the larger of what fills the chip and what the
  // bound asks for.
  const long per_block = kBlockShare / piece;
  const long need = (n_items + per_block - 1) / per_block;
  const long grid = max(min(n_items, 2048l), need);
  if (grid > 0x7fffffffl) { set_error("u8_histogram: input too large for one launch"); return MMVAE_ERR_UNSUPPORTED; }
  note_launch_bytes((double)n_items * (double)piece);
  hipLaunchKernelGGL(u8_histogram_kernel, dim3((unsigned)grid), dim3(kHistThreads), 0, s, frames, clip_bytes, clip_index, n_items, parts,
                     piece, counts);
  return check_launch("u8_histogram");
}

}  // namespace mmvae
