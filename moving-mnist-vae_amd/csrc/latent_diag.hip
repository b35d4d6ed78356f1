// Latent diagnostics: the density panel behind the reference's scatter plot of q(z|x) against p(z) (scatter_plot, main.py:166-183) and
// per-dimension f64 sums over the images of a batch (which latent dimensions carry information, which have collapsed to the prior).
//
// scatter_panel_kernel.  n 2-D points -> side x side bytes, one launch, no global atomics, no zeroed global buffer.
//   Sub-pixel position (f32, an add then a multiply: nothing an fma could contract, explicit roundings all the same):
//     qx = (int)floorf((x + xlim) * sx),  qy = (int)floorf((ylim - y) * sy)        16 sub-positions per pixel, y points up
//   Pixel (row i, column j) is covered iff (16 j + 8 - qx)^2 + (16 i + 8 - qy)^2 <= radius16^2 (integers); the byte is
//   tone[min(#covering points, 255)].
//   A block owns a 32 x 32 tile (clipped at the panel's edge: side is a multiple of 16).  In a row of pixels a disc covers a span of
//   columns, so the block keeps per-row DIFFERENCES in LDS: +1 where a span starts, -1 behind its end; a running sum along each row at
//   the end gives the counts.  That is two LDS integer atomics per row of a disc instead of one per covered pixel (18 against ~50 at
//   radius 4, 34 against ~200 at radius 8): the block in the middle of the cloud, which the launch waits for, is bound by its LDS atomics.
//   The span of row i is |16 j + 8 - qx| <= half[|16 i + 8 - qy|], half[t] = floor(sqrt(r^2 - t^2)) from an exact integer-root table
//   the block builds first -- the same pixels as the rule above.
//   The block walks ALL n points, 1024 at a time, one per thread; a thread turns its point into the pixel box of its disc clipped to
//   the tile and rejects it when the box is empty (jlo <= jhi, ilo <= ihi after the four clips).  The survivors of a wave are stamped
//   four at a time, one per 16-lane group, a lane per row of the box (at most 17 rows: the 17th is a second turn of lane 0).
//   Typically a few lanes of a wave survive, so a per-lane loop over the box would idle the rest of the wave.  Integer sums do not
//   depend on the order of the adds: the same bytes every run, for any order of the points.
//   Tile side (DESIGN.md "Latent diagnostics"): every block re-reads all points, so smaller tiles multiply the reads ((side / T)^2 n
//   points); the critical path is the block that owns the middle of the cloud, whose stamping does not get shorter once the cloud
//   (sigma ~ 15 pixels at the defaults) spans several tiles.  T = 32 is the largest tile at which it still does; 1024 threads = 16
//   waves keep that block's stamping spread over all four SIMDs.
//   A non-finite coordinate, or one whose disc cannot reach the panel, fails the f32 range test in front of the int conversion (NaN
//   compares false), so no conversion overflows.
//
// latent_stats_kernel.  acc[6][d] f64: sums over the N images of mu, mu^2, 0.5 (exp(lv) + mu^2 - lv - 1), exp(lv), enc, enc^2, every
//   term formed in double from the f32 inputs.  A block owns 8 neighbouring dimensions (one 32-byte segment of a row) and 64 row
//   groups: thread (g, k) adds rows g, g + 64, ... of dimension k in that order, a fixed shuffle tree joins the 8 row groups of a wave,
//   the 8 wave sums meet in LDS and are added in wave order.  No atomics: the bits depend on the inputs only (as eval_loss.hip).
#include "common.hpp"
#include "kernels.hpp"

namespace mmvae {

namespace {

constexpr int kTile = 32;
constexpr int kScatterThreads = kTile * kTile;      // one thread per pixel of the tile
constexpr int kPitch = kTile + 1;                   // a spare column takes the span ends of the tile's last column
constexpr int kMaxSide = 512, kMinRadius16 = 12, kMaxRadius16 = 128;

__global__ __launch_bounds__(kScatterThreads) void scatter_panel_kernel(const float* __restrict__ pts, long n, int stride, int col_x, int col_y,
                                                                        const float* __restrict__ xform, int side, int r,
                                                                        const unsigned char* __restrict__ tone, unsigned char* __restrict__ out,
                                                                        long out_row_stride) {
  __shared__ int diff[kTile * kPitch];              // diff[i][j]: discs whose span in row i starts at column j, minus those that ended at j - 1
  __shared__ int half[kMaxRadius16 + 1];           // half[|dy|] = floor(sqrt(r^2 - dy^2)): the disc's half-width, in sub-pixels, |dy| away from its centre
  const int tid = threadIdx.x, lane = tid & 63, grp = lane >> 4, sub = lane & 15;
  const int r2 = r * r;
  for (int t = tid; t < kTile * kPitch; t += kScatterThreads) diff[t] = 0;
  if (tid <= r) {
    const int v = r2 - tid * tid;
    int s = (int)sqrtf((float)v);                  // v <= 2^14 is exact in f32; the two loops make s the integer root whatever sqrtf rounds to
    while (s * s > v) --s;
    while ((s + 1) * (s + 1) <= v) ++s;
    half[tid] = s;
  }
  __syncthreads();
  const int tj0 = blockIdx.x * kTile, ti0 = blockIdx.y * kTile;
  const int tj1 = min(tj0 + kTile, side) - 1, ti1 = min(ti0 + kTile, side) - 1;       // last column / row of the tile inside the panel
  const float xlim = xform[0], ylim = xform[1], sx = xform[2], sy = xform[3];
  const float qmin = -(float)(r + 8), qmax = (float)(16 * side + r + 8);                // outside: the disc cannot reach a pixel centre
  for (long base = 0; base < n; base += kScatterThreads) {                             // (wave-uniform trip count)
    const long p = base + tid;
    int qx = 0, qy = 0, ilo = 0, h = 0;
    if (p < n) {
      const float x = pts[p * stride + col_x], y = pts[p * stride + col_y];
      const float fx = floorf(__fmul_rn(__fadd_rn(x, xlim), sx)), fy = floorf(__fmul_rn(__fsub_rn(ylim, y), sy));
      if (fx >= qmin && fx <= qmax && fy >= qmin && fy <= qmax) {                       // NaN / inf / far away: skipped before the conversion
        qx = (int)fx;
        qy = (int)fy;
        // pixels with |16 j + 8 - qx| <= r: ceil((qx - r - 8) / 16) .. floor((qx + r - 8) / 16) (arithmetic shifts: floor), clipped to the tile
        const int jlo = max((qx - r - 8 + 15) >> 4, tj0), jhi = min((qx + r - 8) >> 4, tj1);
        const int ihi = min((qy + r - 8) >> 4, ti1);
        ilo = max((qy - r - 8 + 15) >> 4, ti0);
        if (jlo <= jhi && ilo <= ihi) h = ihi - ilo + 1;
      }
    }
    unsigned long long live = __ballot(h > 0);
    while (live) {                                                                     // wave-uniform: four surviving points per turn
      int src = -1;                                                                    // the lane whose point this 16-lane group stamps
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (live) {
          const int l = __builtin_ctzll(live);
          live &= live - 1;
          if (grp == k) src = l;
        }
      const int from = src < 0 ? lane : src;
      const int bx = __shfl(qx, from, 64), by = __shfl(qy, from, 64), bi = __shfl(ilo, from, 64), bh = __shfl(h, from, 64);
      if (src >= 0)
        for (int di = sub; di < bh; di += 16) {                                        // a lane per row of the box (at most 17)
          const int i = bi + di;
          const int s = half[min(abs(16 * i + 8 - by), r)];                            // (|dy| <= r for every row of the box)
          const int jl = max((bx - s - 8 + 15) >> 4, tj0), jr = min((bx + s - 8) >> 4, tj1);      // |16 j + 8 - bx| <= s, clipped
          if (jl <= jr) {
            const int row = (i - ti0) * kPitch - tj0;
            atomicAdd(&diff[row + jl], 1);
            atomicAdd(&diff[row + jr + 1], -1);                                        // column jr + 1 <= tj0 + kTile: the spare one
          }
        }
    }
  }
  __syncthreads();
  // counts = running sums of a row's differences: a row is half a wave
  int k = diff[(tid >> 5) * kPitch + (tid & 31)];
#pragma unroll
  for (int o = 1; o < kTile; o <<= 1) {
    const int below = __shfl_up(k, o, kTile);
    if ((tid & (kTile - 1)) >= o) k += below;
  }
  const int i = ti0 + tid / kTile, j = tj0 + tid % kTile;
  if (i < side && j < side) out[(long)i * out_row_stride + j] = tone[min((unsigned)k, 255u)];
}

constexpr int kStatDims = 8, kStatGroups = 64, kStatThreads = kStatDims * kStatGroups, kStatWaves = kStatThreads / 64, kStatRows = 6;

__global__ __launch_bounds__(kStatThreads) void latent_stats_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                                    const float* __restrict__ enc, int N, int d, int accumulate,
                                                                    double* __restrict__ acc) {
  __shared__ double red[kStatWaves][kStatRows][kStatDims];
  const int tid = threadIdx.x, k = tid & (kStatDims - 1), g = tid / kStatDims;
  const int dim = blockIdx.x * kStatDims + k;
  double s[kStatRows] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (dim < d) {
    for (int row = g; row < N; row += kStatGroups) {
      const long at = (long)row * d + dim;
      const double m = (double)mu[at];
      s[0] += m;
      s[1] += m * m;
      if (lv) {
        const double l = (double)lv[at], e = exp(l);
        s[2] += 0.5 * (e + m * m - l - 1.0);
        s[3] += e;
      }
      if (enc) {
        const double z = (double)enc[at];
        s[4] += z;
        s[5] += z * z;
      }
    }
  }
  // lanes k, k + 8, ..., k + 56 of a wave hold the same dimension: a fixed xor tree over the row groups
#pragma unroll
  for (int q = 0; q < kStatRows; ++q) {
#pragma unroll
    for (int o = 32; o >= kStatDims; o >>= 1) s[q] += __shfl_xor(s[q], o, 64);
  }
  if ((tid & 63) < kStatDims) {
#pragma unroll
    for (int q = 0; q < kStatRows; ++q) red[tid >> 6][q][k] = s[q];
  }
  __syncthreads();
  if (tid < kStatRows * kStatDims) {
    const int q = tid / kStatDims, kk = tid % kStatDims, dd = blockIdx.x * kStatDims + kk;
    if (dd < d) {
      double t = 0.0;
#pragma unroll
      for (int wv = 0; wv < kStatWaves; ++wv) t += red[wv][q][kk];
      double* dst = acc + (long)q * d + dd;
      *dst = accumulate ? *dst + t : t;
    }
  }
}

}  // namespace

int launch_scatter_panel(const float* pts, long n, int stride, int col_x, int col_y, const float* xform, int side, int radius16,
                         const unsigned char* tone, unsigned char* out, long out_row_stride, hipStream_t s) {
  if (side < 16 || side > kMaxSide || side % 16 != 0) {
    set_error("scatter_panel: side=%d unsupported (a multiple of 16 in 16..%d)", side, kMaxSide);
    return MMVAE_ERR_UNSUPPORTED;
  }
  if (radius16 < kMinRadius16 || radius16 > kMaxRadius16) {
    set_error("scatter_panel: radius16=%d unsupported (%d..%d sixteenths of a pixel)", radius16, kMinRadius16, kMaxRadius16);
    return MMVAE_ERR_UNSUPPORTED;
  }
  if (n < 0) { set_error("scatter_panel: n=%ld must not be negative", n); return MMVAE_ERR_ARG; }
  if (stride < 1 || col_x < 0 || col_x >= stride || col_y < 0 || col_y >= stride) {
    set_error("scatter_panel: columns (%d, %d) outside a row of stride=%d", col_x, col_y, stride);
    return MMVAE_ERR_ARG;
  }
  if (out_row_stride < side) { set_error("scatter_panel: out_row_stride=%ld below side=%d", out_row_stride, side); return MMVAE_ERR_ARG; }
  if (!xform || !tone || !out || (n > 0 && !pts)) { set_error("scatter_panel: NULL pts, xform, tone or out"); return MMVAE_ERR_ARG; }
  const unsigned tiles = (unsigned)((side + kTile - 1) / kTile);
  hipLaunchKernelGGL(scatter_panel_kernel, dim3(tiles, tiles), dim3(kScatterThreads), 0, s, pts, n, stride, col_x, col_y, xform, side, radius16,
                     tone, out, out_row_stride);
  return check_launch("scatter_panel");
}

int launch_latent_stats(const float* mu, const float* logvar, const float* enc, int N, int d, int accumulate, double* acc, hipStream_t s) {
  if (d < 1 || d > 512) { set_error("latent_stats: d=%d unsupported (1..512)", d); return MMVAE_ERR_UNSUPPORTED; }
  if (N < 1) { set_error("latent_stats: N=%d must be positive", N); return MMVAE_ERR_ARG; }
  if (accumulate != 0 && accumulate != 1) { set_error("latent_stats: accumulate=%d (0 write, 1 add)", accumulate); return MMVAE_ERR_ARG; }
  if (!mu || !acc) { set_error("latent_stats: NULL mu or acc"); return MMVAE_ERR_ARG; }
  hipLaunchKernelGGL(latent_stats_kernel, dim3((unsigned)((d + kStatDims - 1) / kStatDims)), dim3(kStatThreads), 0, s, mu, logvar, enc, N, d,
                     accumulate, acc);
  return check_launch("latent_stats");
}

}  // namespace mmvae
