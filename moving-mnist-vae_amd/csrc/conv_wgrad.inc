// Patch-tile weight-gradient kernel (included by conv_wgrad_bf16.hip / conv_wgrad_f32.hip with WG_T defined).
//
//   dW[tap][a][b] = sum over pixels p of P[p][a] * G[shift_tap(p)][b]
//
// The reduction runs over pixels, so both MFMA operands need pixel-major fragments; they come from natural-layout
// (NHWC) LDS images through ds_read_b64_tr_b16 (hardware transpose, bf16) or plain ds_read_b32 (f32 mode).  A tile is
// up to 128 P-pixels (rows of one image, or several whole images); the G patch every tap of the tile touches is staged
// ONCE (zero-filled padding, optional fused BN+ReLU) and each tap reuses it through a constant byte offset.
//
// These launches are bound by per-tile latency (global round trip + two barriers for only ~16 MFMAs per wave), not
// by HBM or MFMA throughput, so the tile loop is software-pipelined: the loads of tile i+1 are issued into registers
// before the MFMA phase of tile i and committed to LDS afterwards.  The staging slots of a thread are tile-invariant
// (element offset + one range check each, decoded once), its channel vector is fixed, and so the BN scale/shift of
// the prologue sit in registers.
//
// Accumulators persist in registers across the block's tiles.  Flush: every block stores its partial image
// [part = blockIdx.x][tap][a][b] with plain coalesced stores and wgrad_reduce_kernel sums the parts into the PyTorch
// weight layout (no atomics, grid sized by occupancy).
//
// LDS carve: [P tile: TP x TA][G patch: npatch x TB][sToff: 32 ints]; the flush staging image aliases the front.
// Work split over the 4 waves of a block:
//   TS = true  (>= 4 taps): wave w owns taps w, w+4, ... of the block's tap group and runs every 32-pixel k-step;
//   TS = false (1x1 convs): wave w owns k-step w of the tile and every tap.

namespace mmvae {

template <int TA16, int TB16> struct Wgrad2Cfg {
  static constexpr int kUnits = TA16 * TB16;
  static constexpr int kMaxT = (12 / kUnits) < 1 ? 1 : ((12 / kUnits) > 4 ? 4 : (12 / kUnits));
};

constexpr int kSlotInvalid = 0x40000000;

template <typename T, int VE>
__device__ __forceinline__ Vec16 apply_pro(const Vec16& q, const float* sc, const float* sh, int relu) {
  float f[VE];
  Elem<T>::unpack(q, f);
#pragma unroll
  for (int j = 0; j < VE; ++j) {
    const float x = f[j] * sc[j] + sh[j];
    f[j] = relu ? fmaxf(x, 0.f) : x;
  }
  return Elem<T>::pack(f);
}

// NW = waves per block.  4: the default.  9 / 16 (deep layers, 3x3 / 4x4 kernels): ONE tap per wave, so the block covers every
// tap of its (a, b) tile and the P tile / G patch are staged once instead of once per tap group.
template <typename T, int TA16, int TB16, bool TS, int MAXG, bool PPL, int NW = 4>
__global__ __launch_bounds__(64 * NW, NW == 16 ? 4 : (NW == 9 ? 3 : (NW == 8 ? 2 : (MAXG <= 8 ? 3 : 2) - (TA16 * TB16 > 2 ? 1 : 0)))) void wgrad2_kernel(Wgrad2Args a) {
  static_assert(NW == 4 || TS, "one-tap-per-wave blocks are tap-split");
  constexpr int NT = 64 * NW;
  constexpr int VE = Elem<T>::kVec;
  constexpr int ES = sizeof(T);
  constexpr int TA = TA16 * 16, TB = TB16 * 16;
  constexpr int MAXT = NW > 4 ? (NW == 8 ? 2 : 1) : Wgrad2Cfg<TA16, TB16>::kMaxT;     // NW = 8: two taps per wave (64x64 tiles, 16 taps)
  constexpr int NKS = TS ? 4 : 1;
  constexpr int CVG = TB / VE, PSG = NT / CVG;          // 16-byte vectors per G pixel; patch pixels per slot round
  constexpr int CVP = TA / VE, PSP = NT / CVP;
  constexpr int MAXP = (128 + PSP - 1) / PSP;       // P-tile slots per thread (TP <= 128)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const TileGeom g = a.g;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, gq = lane >> 4, r = lane & 15;
  const int nb_tiles = a.Cb / TB;
  const int a0 = (blockIdx.y / nb_tiles) * TA, b0 = (blockIdx.y % nb_tiles) * TB;
  const int tap0 = blockIdx.z * a.TG;
  const int tg_n = min(a.TG, a.ntaps - tap0);
  const int npatch = g.segs * g.PR * g.PW;
  char* sP = smem;                                                     // [TP][TA]
  char* sG = sP + g.TP * TA * ES;                                      // [npatch][TB]
  int* sToff = reinterpret_cast<int*>(sG + npatch * TB * ES);
  const T* __restrict__ Pp = reinterpret_cast<const T*>(a.P);
  const T* __restrict__ Gp = reinterpret_cast<const T*>(a.G);
  const bool proP = a.proP_scale != nullptr, proG = a.proG_scale != nullptr;
  const bool multi = g.tiles_per_img == 0;
  if (t < tg_n) {
    const int tap = tap0 + t, kh = tap / a.ksz, kw = tap - kh * a.ksz;
    sToff[t] = (kh * g.PW + kw) * TB * ES;          // patch origin is (q*SI - pad): tap (kh,kw) sits at +kh rows, +kw cols
  }
  // ---- this thread's staging slots (tile-invariant)
  const int cvp = t % CVP, pp0 = t / CVP, cvg = t % CVG, gp0 = t / CVG;
  float xsc[VE], xsh[VE];      // BN scale / shift of the ONE operand that has a load prologue (never both: see the launcher)
#pragma unroll
  for (int j = 0; j < VE; ++j) {
    xsc[j] = proP ? a.proP_scale[a0 + cvp * VE + j] : (proG ? a.proG_scale[b0 + cvg * VE + j] : 1.f);
    xsh[j] = proP ? a.proP_shift[a0 + cvp * VE + j] : (proG ? a.proG_shift[b0 + cvg * VE + j] : 0.f);
  }
  int goff[MAXG], gchk[MAXG];
#pragma unroll
  for (int k = 0; k < MAXG; ++k) {
    const int pp = gp0 + k * PSG;
    goff[k] = 0; gchk[k] = kSlotInvalid;
    if (pp < npatch) {
      const int row = pp / g.PW, pc = pp - row * g.PW;
      const int seg = row / g.PR, pr = row - seg * g.PR;
      const int wi = g.ow + pc;
      bool ok = wi >= 0 && wi < g.Wi;
      if (multi) ok = ok && g.oh + pr >= 0 && g.oh + pr < g.Hi;       // whole-image tiles: the row check is static too
      goff[k] = ((seg * g.Hi + pr) * g.Wi + wi) * a.Cb + b0 + cvg * VE;
      if (ok) gchk[k] = multi ? seg : pr;
    }
  }
  const unsigned lim = multi ? g.N : g.Hi;
  f32x4 acc[MAXT][TA16][TB16];
#pragma unroll
  for (int tl = 0; tl < MAXT; ++tl)
#pragma unroll
    for (int ta = 0; ta < TA16; ++ta)
#pragma unroll
      for (int tb = 0; tb < TB16; ++tb) acc[tl][ta][tb] = (f32x4){0, 0, 0, 0};
  const int npix_tile = g.segs * g.qr * g.Wq;       // pixel slots of one tile
  // tile-independent LDS offsets of this lane's fragment pixels (bf16: 2 four-pixel blocks per k-step)
  int offP[NKS][2], offG[NKS][2];
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int i = 0; i < NKS; ++i)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        int p = 32 * (TS ? i : wv) + 16 * b + 4 * gq + (r >> 2);
        offP[i][b] = p * TA * ES + (r & 3) * 8;
        if (p >= npix_tile) p = 0;                  // P rows beyond the tile are zero; any finite G value will do
        offG[i][b] = patch_index(g, p) * TB * ES + (r & 3) * 8;
      }
  }
  int my_tap[MAXT];
#pragma unroll
  for (int tl = 0; tl < MAXT; ++tl) my_tap[tl] = TS ? wv + NW * tl : tl;

  // ---- software pipeline state: the staged registers of the NEXT tile
  Vec16 gv[MAXG], pv[MAXP];
  int tb_c = 0, nv_c = 0;                           // range-check base / valid P pixels of the tile held in gv/pv
  long m0_c = 0;                                    // first P pixel of that tile (planar P only)
  const long pplane = (long)g.Hq * g.Wq;
  auto issue = [&](int tile) {
    int n, hq0;
    tile_origin(g, tile, 0, n, hq0);
    const long m0 = ((long)n * g.Hq + hq0) * g.Wq;
    const long mend = !multi ? ((long)n * g.Hq + min(g.Hq, hq0 + g.qr)) * g.Wq : (long)min(g.N, n + g.segs) * g.Hq * g.Wq;
    nv_c = (int)(mend - m0);
    const int h_base = hq0 * g.SI + g.oh;
    tb_c = multi ? n : h_base;
    const T* gsrc = Gp + ((long)n * g.Hi + h_base) * g.Wi * a.Cb;
#pragma unroll
    for (int k = 0; k < MAXG; ++k) {
      gv[k] = Vec16{{0, 0, 0, 0}};
      if ((unsigned)(tb_c + gchk[k]) < lim) gv[k] = *reinterpret_cast<const Vec16*>(gsrc + goff[k]);
    }
    if constexpr (!PPL) {
      const T* psrc = Pp + m0 * a.Ca + a0 + cvp * VE;
#pragma unroll
      for (int k = 0; k < MAXP; ++k) {
        const int pix = pp0 + k * PSP;
        pv[k] = Vec16{{0, 0, 0, 0}};
        if (pix < nv_c) pv[k] = *reinterpret_cast<const Vec16*>(psrc + (long)pix * a.Ca);
      }
    } else {
      // planar f32 P ([N][P_planes][Hq][Wq], the reconstruction gradient): up to 2 planes are prefetched as raw floats
      m0_c = m0;
#pragma unroll
      for (int k = 0; k < MAXP; ++k) {
        const int pix = pp0 + k * PSP;
        pv[k] = Vec16{{0, 0, 0, 0}};
        if (pix < nv_c && cvp == 0 && a.P_planes <= 2) {
          long nn = n, rem = (long)hq0 * g.Wq + pix;                  // row tiles stay inside image n
          if (multi) { const long m = m0 + pix; nn = m / pplane; rem = m - nn * pplane; }
          const float* src = reinterpret_cast<const float*>(a.P) + nn * a.P_planes * pplane + rem;
          pv[k].w[0] = __float_as_uint(src[0]);
          if (a.P_planes > 1) pv[k].w[1] = __float_as_uint(src[pplane]);
        }
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < MAXG; ++k) {
      const int pp = gp0 + k * PSG;
      if (pp < npatch) {
        Vec16 q = gv[k];
        if (proG && (unsigned)(tb_c + gchk[k]) < lim) q = apply_pro<T, VE>(q, xsc, xsh, a.proG_relu);   // padding stays exactly zero
        reinterpret_cast<Vec16*>(sG)[pp * CVG + cvg] = q;
      }
    }
#pragma unroll
    for (int k = 0; k < MAXP; ++k) {
      const int pix = pp0 + k * PSP;
      if (pix < g.TP) {
        Vec16 q = pv[k];
        if constexpr (PPL) {
          // channels >= P_planes of the 16-channel LDS pixel are zero
          float f[VE];
#pragma unroll
          for (int j = 0; j < VE; ++j) f[j] = 0.f;
          if (pix < nv_c && cvp * VE < a.P_planes) {
            if (a.P_planes <= 2) { f[0] = __uint_as_float(q.w[0]); f[1] = __uint_as_float(q.w[1]); }
            else {
              const long m = m0_c + pix, nn = m / pplane, rem = m - nn * pplane;
              const float* src = reinterpret_cast<const float*>(a.P) + nn * a.P_planes * pplane + rem;
#pragma unroll
              for (int j = 0; j < VE; ++j) if (cvp * VE + j < a.P_planes) f[j] = src[(long)(cvp * VE + j) * pplane];
            }
          }
          q = Elem<T>::pack(f);
        } else { if (proP && pix < nv_c) q = apply_pro<T, VE>(q, xsc, xsh, a.proP_relu); }
        reinterpret_cast<Vec16*>(sP)[pix * CVP + cvp] = q;
      }
    }
  };

  const int nks_tile = g.TP >> 5;                   // 32-pixel k-steps per tile (TS mode: 4, 2 or 1)
  // values loaded before the tile loop must have arrived before it (see conv_patch.inc): a pending load at loop entry
  // costs a vmcnt(0) wait -- covering the next tile's prefetch -- at its first use in every iteration
#pragma unroll
  for (int j = 0; j < VE; ++j) {
    asm volatile("" ::"v"(xsc[j])); asm volatile("" ::"v"(xsh[j]));
  }
  const TileWalk walk = xcd_tile_walk(g.ntiles);
  int tile = walk.first;
  if (tile < walk.end) issue(tile);
  for (; tile < walk.end; tile += walk.step) {
    __syncthreads();                                // every wave is done reading the previous tile
    commit();
    __syncthreads();
    if (tile + walk.step < walk.end) issue(tile + walk.step);     // in flight during the MFMA phase
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int i = 0; i < NKS; ++i) {
        if (TS && i >= nks_tile) break;
        Vec16 af[TA16];
#pragma unroll
        for (int ta = 0; ta < TA16; ++ta) af[ta] = FragOps<bf16_t>::load(sP, offP[i][0] + ta * 32, offP[i][1] + ta * 32);
#pragma unroll
        for (int tl = 0; tl < MAXT; ++tl) {
          if (my_tap[tl] < tg_n) {
            const int toff = sToff[my_tap[tl]];
#pragma unroll
            for (int tb = 0; tb < TB16; ++tb) {
              const Vec16 bf = FragOps<bf16_t>::load(sG, offG[i][0] + toff + tb * 32, offG[i][1] + toff + tb * 32);
#pragma unroll
              for (int ta = 0; ta < TA16; ++ta) acc[tl][ta][tb] = mma_bf16(af[ta], bf, acc[tl][ta][tb]);
            }
          }
        }
      }
    } else {
      // ---- f32 (validation mode): 8 MFMA 16x16x4 steps per 32-pixel k-step; pixel of (step j, group gq): 32ks + 4j + gq
      for (int i = 0; i < NKS; ++i) {
        if (TS && i >= nks_tile) break;
        const int ks = TS ? i : wv;
        for (int j = 0; j < 8; ++j) {
          int p = 32 * ks + 4 * j + gq;
          const int oP = p * TA * ES + r * 4;
          if (p >= npix_tile) p = 0;
          const int oG = patch_index(g, p) * TB * ES + r * 4;
          float av[TA16];
#pragma unroll
          for (int ta = 0; ta < TA16; ++ta) av[ta] = *reinterpret_cast<const float*>(sP + oP + ta * 64);
#pragma unroll
          for (int tl = 0; tl < MAXT; ++tl) {
            if (my_tap[tl] < tg_n) {
              const int toff = sToff[my_tap[tl]];
#pragma unroll
              for (int tb = 0; tb < TB16; ++tb) {
                const float bv = *reinterpret_cast<const float*>(sG + oG + toff + tb * 64);
#pragma unroll
                for (int ta = 0; ta < TA16; ++ta)
                  acc[tl][ta][tb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ta], bv, acc[tl][ta][tb], 0, 0, 0);
              }
            }
          }
        }
      }
    }
  }
  // ---- flush
  if (TS && a.partial) {
    // every (part, tap, a, b) has exactly one owner wave: plain stores, 64 contiguous bytes per 16 lanes
#pragma unroll
    for (int tl = 0; tl < MAXT; ++tl) {
      if (my_tap[tl] < tg_n) {
        float* dst = a.dW + (((long)blockIdx.x * a.ntaps + tap0 + my_tap[tl]) * a.Ca + a0) * a.Cb + b0;
#pragma unroll
        for (int ta = 0; ta < TA16; ++ta)
#pragma unroll
          for (int tb = 0; tb < TB16; ++tb)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) dst[(long)(16 * ta + 4 * gq + jj) * a.Cb + 16 * tb + r] = acc[tl][ta][tb][jj];
      }
    }
    return;
  }
  // tap by tap through an LDS image [a_l][b_l]: combines the k-split waves, makes the global accesses contiguous
  __syncthreads();
  float* sAcc = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int tl = 0; tl < MAXT; ++tl) {
    for (int w = 0; w < (TS ? NW : 1); ++w) {
      const int tap_l = TS ? w + NW * tl : tl;          // uniform over the block
      if (tap_l >= tg_n) continue;
      // the k-split waves of a tap (!TS) add in wave order: every LDS element has one writer per round -> the same bits every run
      for (int src = 0; src < (TS ? 1 : NW); ++src) {
        if (TS ? (wv == w) : (wv == src)) {
#pragma unroll
          for (int ta = 0; ta < TA16; ++ta)
#pragma unroll
            for (int tb = 0; tb < TB16; ++tb)
#pragma unroll
              for (int jj = 0; jj < 4; ++jj) {
                float* q = &sAcc[(16 * ta + 4 * gq + jj) * TB + 16 * tb + r];
                *q = (src == 0 ? 0.f : *q) + acc[tl][ta][tb][jj];
              }
        }
        __syncthreads();
      }
      float* dst = a.dW + (((long)blockIdx.x * a.ntaps + tap0 + tap_l) * a.Ca + a0) * a.Cb + b0;
      for (int i = t; i < TA * TB; i += NT) dst[(long)(i / TB) * a.Cb + (i % TB)] = sAcc[i];
      __syncthreads();
    }
  }
}

template <typename T>
static int launch_wgrad2_t(Wgrad2Args a, int dt, dim3 grid, int ta16, int tb16, int maxg, hipStream_t s) {
  const size_t lds = wgrad2_lds_bytes(a, dt, ta16 * 16, tb16 * 16);
  dim3 block(64 * a.nw);
  const bool ts = a.ntaps >= 4;
  if (a.nw != 4) {
    // one tap per wave (deep layers): 64x64, 64x32, 32x64 tiles, 9 or 16 waves
    if (a.nw == 8) {
      if (ta16 != 4 || tb16 != 4 || a.P_planar || !ts || maxg > 8) { set_error("wgrad2: nw=8 needs the 64x64 tile"); return MMVAE_ERR_UNSUPPORTED; }
      if (maxg <= 4) hipLaunchKernelGGL((wgrad2_kernel<T, 4, 4, true, 4, false, 8>), grid, block, lds, s, a);
      else hipLaunchKernelGGL((wgrad2_kernel<T, 4, 4, true, 8, false, 8>), grid, block, lds, s, a);
      return check_launch("wgrad2");
    }
    if (a.P_planar || !ts || maxg > 8 || (a.nw != 9 && a.nw != 16)) { set_error("wgrad2: nw=%d unsupported here", a.nw); return MMVAE_ERR_UNSUPPORTED; }
#define MMVAE_W2N(A_, B_) do { \
    if (a.nw == 9) { if (maxg <= 4) hipLaunchKernelGGL((wgrad2_kernel<T, A_, B_, true, 4, false, 9>), grid, block, lds, s, a); \
                     else hipLaunchKernelGGL((wgrad2_kernel<T, A_, B_, true, 8, false, 9>), grid, block, lds, s, a); } \
    else { if (maxg <= 4) hipLaunchKernelGGL((wgrad2_kernel<T, A_, B_, true, 4, false, 16>), grid, block, lds, s, a); \
           else hipLaunchKernelGGL((wgrad2_kernel<T, A_, B_, true, 8, false, 16>), grid, block, lds, s, a); } } while (0)
    if (ta16 == 4 && tb16 == 4) MMVAE_W2N(4, 4);
    else if (ta16 == 4 && tb16 == 2) MMVAE_W2N(4, 2);
    else if (ta16 == 2 && tb16 == 4) MMVAE_W2N(2, 4);
    else if (ta16 == 2 && tb16 == 2) MMVAE_W2N(2, 2);
    else { set_error("wgrad2: tile %dx%d unsupported with nw=%d", ta16, tb16, a.nw); return MMVAE_ERR_UNSUPPORTED; }
#undef MMVAE_W2N
    return check_launch("wgrad2");
  }
#define MMVAE_W2G(A_, B_, G_) do { if (ts) hipLaunchKernelGGL((wgrad2_kernel<T, A_, B_, true, G_, false>), grid, block, lds, s, a); \
                                   else hipLaunchKernelGGL((wgrad2_kernel<T, A_, B_, false, G_, false>), grid, block, lds, s, a); } while (0)
#define MMVAE_W2(A_, B_) do { if (maxg <= 8) MMVAE_W2G(A_, B_, 8); else MMVAE_W2G(A_, B_, 16); } while (0)
  if (a.P_planar) {
    if (ta16 != 1 || tb16 != 1 || !ts) { set_error("wgrad2: planar P needs the 16x16 tap-split tile"); return MMVAE_ERR_UNSUPPORTED; }
    if (maxg <= 8) hipLaunchKernelGGL((wgrad2_kernel<T, 1, 1, true, 8, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((wgrad2_kernel<T, 1, 1, true, 16, true>), grid, block, lds, s, a);
  } else if (ta16 == 1 && tb16 == 1) MMVAE_W2(1, 1);
  else if (ta16 == 1 && tb16 == 2) MMVAE_W2(1, 2);
  else if (ta16 == 2 && tb16 == 1) MMVAE_W2(2, 1);
  else if (ta16 == 2 && tb16 == 2) MMVAE_W2(2, 2);
  else if (ta16 == 4 && tb16 == 2) MMVAE_W2(4, 2);
  else if (ta16 == 2 && tb16 == 4) MMVAE_W2(2, 4);
  else if (ta16 == 4 && tb16 == 4) MMVAE_W2(4, 4);
  else if (ta16 == 4 && tb16 == 1) MMVAE_W2(4, 1);
  else if (ta16 == 1 && tb16 == 4) MMVAE_W2(1, 4);
  else { set_error("wgrad2: tile %dx%d unsupported", ta16, tb16); return MMVAE_ERR_UNSUPPORTED; }
#undef MMVAE_W2
#undef MMVAE_W2G
  return check_launch("wgrad2");
}

}  // namespace mmvae
