// patch_conv_kernel: pipelined patch-tile convolution for the thin, pixel-heavy layers (Conv2d fwd, ConvT fwd, dgrads)
// whose complete weight set (all stride-phases) fits LDS.
//
// A tile = up to 128 q-pixels (rows of one image or several whole images); q is the coarse grid: the output grid of a
// strided Conv2d / ConvT-dgrad, the input-resolution grid of a ConvT / strided-conv dgrad (each q-pixel then owns
// SO x SO output pixels, one per stride-phase).  Per tile the block
//   1. commits the input patch (prefetched into registers during the previous tile's MFMA phase) to LDS in natural
//      NHWC layout, zero-filled padding, fused BN+ReLU applied ONCE per element;
//   2. issues the global loads of the next tile;
//   3. runs every stride-phase from the one staged patch: B fragment = 8 consecutive channels of one tap
//      (ds_read_b128 at pixel base + per-k-vector offset), A fragment = LDS copy of the phase's weight matrix,
//      D[cout][pixel] so that a lane ends with 4 consecutive output channels of one pixel (8/16-byte NHWC stores);
//      per-channel sum / sum^2 for BatchNorm are accumulated from the f32 results.
// The staging slots of a thread are tile-invariant (element offset + one range check), its channel vector is fixed,
// so the BN scale/shift of the prologue sit in registers and the per-tile index arithmetic is a handful of VALU ops --
// these layers are bound by per-tile latency and index VALU, not by HBM or MFMA.
//
// LDS carve: [weights of all phases: CT rows x (kvp_p+1) vec16 each][patch][sKoff: sum kvp_p ints][sStat: 8*CT floats]
#include "kernels.hpp"
#include "tile_common.hpp"

namespace mmvae {

template <typename TO> __device__ __forceinline__ void pstore4(TO* p, const float* v, bool acc);
template <> __device__ __forceinline__ void pstore4<float>(float* p, const float* v, bool acc) {
  float4 o = make_float4(v[0], v[1], v[2], v[3]);
  if (acc) { const float4 e = *reinterpret_cast<const float4*>(p); o.x += e.x; o.y += e.y; o.z += e.z; o.w += e.w; }
  *reinterpret_cast<float4*>(p) = o;
}
template <> __device__ __forceinline__ void pstore4<bf16_t>(bf16_t* p, const float* v, bool acc) {
  float f[4] = {v[0], v[1], v[2], v[3]};
  if (acc) {
    const uint2 e = *reinterpret_cast<const uint2*>(p);
    f[0] += __uint_as_float(e.x << 16); f[1] += __uint_as_float(e.x & 0xffff0000u);
    f[2] += __uint_as_float(e.y << 16); f[3] += __uint_as_float(e.y & 0xffff0000u);
  }
  uint2 o;
  o.x = pack2_bf16(f[0], f[1]);
  o.y = pack2_bf16(f[2], f[3]);
  *reinterpret_cast<uint2*>(__builtin_assume_aligned(p, 8)) = o;
}

constexpr int kPatchSlotInvalid = 0x40000000;
constexpr int kPlanarPrefetch = 2;      // planar inputs with <= 2 planes are prefetched like NHWC ones

// NPT = 16-pixel MFMA column tiles per wave and tile (tile = 64*NPT q-pixels).  NPT == 2: any geometry (per-lane pixel
// decode).  NPT > 2: row tiles whose q-width is a power of two >= 16 -- a column tile is then 16 consecutive pixels of
// one q-row, its row / column origin are wave-uniform and only `r` is per-lane.
//
// UNI epilogue: 8-byte-per-lane stores of an MFMA column tile touch 16 half-filled lines and the store instruction
// count, not HBM, bounds these layers (measured: 155 of 250 us at decoder.uplayer5).  So the wave stages the results
// of one output row-phase in a private LDS buffer laid out like the output run ([16 q][SO pw][Cout], contiguous in
// memory) and writes it back with 16-byte-per-lane stores of whole lines.
// ACC (y += result) is a template parameter: its read-modify-write loads share registers with the accumulators, and a
// load anywhere in the loop makes the compiler's in-order vmcnt waits cover the next tile's prefetch as well.
// SOT (uniform geometry only) = output stride of the phases: the (ph, pw) loops are unrolled, because an inner loop with
// memory operations makes the compiler flush vmcnt in its preheader -- i.e. wait for the prefetch just issued.
// X2 (0, 2, 4) = staging slots of the optional SECOND source: a tensor on the q grid itself ([N][Hq][Wq][Cin2], no halo) whose 1x1
// convolution is added into one phase -- the shortcut's data gradient merged into the main path's (see GatherArgs).
template <typename T, typename TO, int CT16, int MAXG, bool PLANAR, int NPT, bool UNI, bool ACC, int SOT, int X2 = 0>
__global__ __launch_bounds__(256, (MAXG <= 4 ? (CT16 == 1 ? 4 : (CT16 == 2 ? 3 : 2)) : ((MAXG <= 8 && CT16 == 1) ? 3 : 2)) - ((NPT >= 4 && MAXG <= 4) ? 1 : 0) - ((X2 > 0 && MAXG <= 4 && CT16 == 1) ? 1 : 0)) void patch_conv_kernel(PatchArgs a) {
  static_assert(UNI || NPT == 2, "general pixel decode only with 2 column tiles per wave");
  constexpr int VE = Elem<T>::kVec;
  constexpr int ES = sizeof(T);
  constexpr int CT = CT16 * 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const TileGeom g = a.g;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, gq = lane >> 4, r = lane & 15;
  const int cin_vecs = a.Cin / VE;
  const int npatch = g.segs * g.PR * g.PW;
  Vec16* sW = reinterpret_cast<Vec16*>(smem);
  Vec16* sPatch = sW + a.w_vecs;
  int* sKoff = reinterpret_cast<int*>(sPatch + npatch * cin_vecs);
  float* sStat = reinterpret_cast<float*>(sKoff + a.koff_total);
  char* sOut = reinterpret_cast<char*>(sStat + 8 * CT);          // UNI: 4 wave-private output staging buffers (16-byte aligned)
  Vec16* sW2 = sW + a.w2_vec0;                                   // X2: weights [CT][kvp2 + 1] and the tile of the second source
  Vec16* sX2 = sW + a.x2_vec0;
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  TO* __restrict__ Y = reinterpret_cast<TO*>(a.y);
  const bool has_pro = a.pro_scale != nullptr, has_bias = a.bias != nullptr, has_stats = a.stats != nullptr;
  const bool multi = g.tiles_per_img == 0;
  constexpr bool planar = PLANAR;
  const bool planar_pf = planar && a.x_planes <= kPlanarPrefetch;

  // ---- block prologue: weight matrices and k-offset tables of every phase
  for (int p = 0; p < a.nphase; ++p) {
    const PatchPhase P = a.phases[p];
    const int kvecs = P.ntaps * cin_vecs, kvp = (kvecs + 3) & ~3, wrow = kvp + 1;
    const T* Wt = reinterpret_cast<const T*>(a.w) + P.w_off;
    Vec16* sWp = sW + P.w_vec0;
    for (int v = t; v < CT * kvp; v += 256) {
      const int row = v / kvp, kv = v - row * kvp;
      sWp[row * wrow + kv] = (kv < kvecs && row < a.Cout) ? *reinterpret_cast<const Vec16*>(Wt + ((long)row * kvecs + kv) * VE) : Vec16{{0, 0, 0, 0}};
    }
    for (int v = t; v < kvp; v += 256) {
      int off = 0;
      if (v < kvecs) {
        const int tap = v / cin_vecs, cv = v - tap * cin_vecs;
        const Tap tp = a.taps[P.tap0 + tap];
        off = (((tp.dh - g.oh) * g.PW + (tp.dw - g.ow)) * a.Cin + cv * VE) * ES;
      }
      sKoff[P.koff0 + v] = off;
    }
  }
  const int cin2_vecs = X2 > 0 ? a.Cin2 / VE : 1;
  if constexpr (X2 > 0) {
    const T* W2g = reinterpret_cast<const T*>(a.w2);
    const int wrow2 = a.kvp2 + 1;
    for (int v = t; v < CT * a.kvp2; v += 256) {
      const int row = v / a.kvp2, kv = v - row * a.kvp2;
      sW2[row * wrow2 + kv] = (kv < cin2_vecs && row < a.Cout) ? *reinterpret_cast<const Vec16*>(W2g + ((long)row * cin2_vecs + kv) * VE) : Vec16{{0, 0, 0, 0}};
    }
    for (int v = t; v < g.segs * g.qr * g.Wq * cin2_vecs + 8; v += 256) sX2[v] = Vec16{{0, 0, 0, 0}};     // incl. the read-past pad
  }
  // ---- this thread's staging slots (tile-invariant)
  //  NHWC:   slot k = 16-byte vector `cv` of patch pixel pix0 + k*PS
  //  planar: slot k = patch pixel t + 256k (x_planes scalars, expanded to Cin zero-padded channels in LDS)
  const int cv = planar ? 0 : t % cin_vecs, pix0 = planar ? t : t / cin_vecs, PS = planar ? 256 : 256 / cin_vecs;
  float psc[VE], psh[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) {
    psc[j] = has_pro ? a.pro_scale[cv * VE + j] : 1.f;
    psh[j] = has_pro ? a.pro_shift[cv * VE + j] : 0.f;
  }
  unsigned goff[MAXG]; int gchk[MAXG];     // element offset from the tile's source origin (valid slots: >= 0)
  const long plane = (long)g.Hi * g.Wi;
#pragma unroll
  for (int k = 0; k < MAXG; ++k) {
    const int pp = pix0 + k * PS;
    goff[k] = 0; gchk[k] = kPatchSlotInvalid;
    if (pp < npatch) {
      const int row = pp / g.PW, pc = pp - row * g.PW;
      const int seg = row / g.PR, pr = row - seg * g.PR;
      const int wi = g.ow + pc;
      bool ok = wi >= 0 && wi < g.Wi;
      if (multi) ok = ok && g.oh + pr >= 0 && g.oh + pr < g.Hi;
      if (ok) {
        goff[k] = planar ? (unsigned)((int)(seg * a.x_planes * plane) + pr * g.Wi + wi) : (unsigned)(((seg * g.Hi + pr) * g.Wi + wi) * a.Cin + cv * VE);
        gchk[k] = multi ? seg : pr;
      }
    }
  }
  const unsigned lim = multi ? g.N : g.Hi;
  const float relu_lo = a.pro_relu ? 0.f : -__builtin_inff();
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, a.x_bytes, 0x00020000);
  if constexpr (!planar) {                         // statically padded patch slots stay zero for the block's lifetime
    for (int v = t; v < npatch * cin_vecs; v += 256) sPatch[v] = Vec16{{0, 0, 0, 0}};
  }
  // ---- tile-independent decode of this lane's q-pixels
  const int npix_tile = g.segs * g.qr * g.Wq;
  const int wvu = __builtin_amdgcn_readfirstlane(wv);
  int pbase[2], pseg[2], pj[2], pwq[2];
  if constexpr (!UNI) {
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
      const int p = 32 * wv + 16 * pt + r;
      const int pc = p < npix_tile ? p : 0;
      pbase[pt] = patch_index(g, pc) * a.Cin * ES;
      const int per_seg = g.qr * g.Wq;
      pseg[pt] = pc / per_seg;
      const int rem = pc - pseg[pt] * per_seg;
      pj[pt] = rem / g.Wq;
      pwq[pt] = rem - pj[pt] * g.Wq;
      if (p >= npix_tile) pseg[pt] = -1;
    }
  }
  const int lane_pb = r * g.SI * a.Cin * ES;       // NPT > 2: per-lane part of the patch byte offset
  // column tile pt of this wave: q-row jrow(pt), first q-column wq0(pt) (both wave-uniform)
  auto col_row = [&](int pt) { return ((wv * NPT + pt) * 16) >> a.wq_shift; };
  auto col_wq0 = [&](int pt) { return ((wv * NPT + pt) * 16) & (g.Wq - 1); };
  float st1[CT16][4], st2[CT16][4];
#pragma unroll
  for (int c = 0; c < CT16; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) { st1[c][j] = 0.f; st2[c][j] = 0.f; }
  const char* patch_bytes = reinterpret_cast<const char*>(sPatch);
  // UNI epilogue: LDS staging geometry and this lane's tile-invariant read-back offsets (see the epilogue below)
  constexpr int kOutPitch = 16 * 4 * (int)sizeof(TO) + 16;       // bytes between channel-quad planes (16 q x 4 channels + skew)
  // read-back rounds of 64 x 16 bytes per column-tile run: run16 = SO*Cout*sizeof(TO) <= SOT*CT*sizeof(TO) chunks
  constexpr int kOutIters = (SOT * CT * (int)sizeof(TO) + 63) / 64;
  const int run16 = (16 * a.SO * a.Cout * (int)sizeof(TO)) >> 4; // 16-byte chunks of one column-tile run [16 q][SO pw][Cout]
  int rb_off[kOutIters];
  if constexpr (UNI) {
    const int cpp = (a.Cout * (int)sizeof(TO)) >> 4;             // chunks per output pixel
#pragma unroll
    for (int it = 0; it < kOutIters; ++it) {
      const int j = lane + 64 * it;
      const int q = j / (a.SO * cpp), rem = j - q * (a.SO * cpp);
      const int pw = rem / cpp, k = rem - pw * cpp;
      const int quad = sizeof(TO) == 2 ? 2 * k : k;              // first channel quad of the chunk (bf16: 8 channels, f32: 4)
      rb_off[it] = ((pw * CT16 + (quad >> 2)) * 4 + (quad & 3)) * kOutPitch + q * 4 * (int)sizeof(TO);
    }
  }
  // bias of this lane's output channels, in registers: a global load inside the tile loop would make the epilogue wait
  // (vmcnt is in-order) for the next tile's prefetch as well
  float bv[CT16][4];
#pragma unroll
  for (int c = 0; c < CT16; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = 16 * c + 4 * gq + j;
      bv[c][j] = (a.bias && co < (a.y_planes > 0 ? a.y_planes : a.Cout)) ? a.bias[co] : 0.f;
    }

  // ---- software pipeline: registers of the NEXT tile
  Vec16 gv[MAXG];
  Vec16 gv2[X2 > 0 ? X2 : 1];
  const __amdgpu_buffer_rsrc_t x2rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(X2 > 0 ? a.x2 : a.x), 0, X2 > 0 ? a.x2_bytes : 0u, 0x00020000);
  const int x2_tile_vecs = g.segs * g.qr * g.Wq * cin2_vecs;
  int tb_c = 0;
  auto issue = [&](int tile) {
    int n, hq0;
    tile_origin(g, tile, 0, n, hq0);
    const int h_base = hq0 * g.SI + g.oh;
    tb_c = multi ? n : h_base;
    if constexpr (X2 > 0) {
      // the tile's q-pixels are one contiguous run of the second source; pixels beyond the image / batch read as zero
      const int nv2 = (multi ? min(g.segs, g.N - n) * g.Hq : min(g.qr, g.Hq - hq0)) * g.Wq * cin2_vecs;
      const unsigned toff2 = (unsigned)((((long)n * g.Hq + hq0) * g.Wq * a.Cin2) * ES);
#pragma unroll
      for (int k = 0; k < X2; ++k) {
        const int v = t + 256 * k;
        const unsigned off = v < nv2 ? toff2 + (unsigned)v * 16u : 0x80000000u;
        gv2[k] = __builtin_bit_cast(Vec16, __builtin_amdgcn_raw_buffer_load_b128(x2rs, off, 0, 0));
      }
    }
    if constexpr (!planar) {
      // buffer loads: an out-of-range offset returns zeros, so padding costs one select instead of a branch
      const unsigned toff = (unsigned)((((long)n * g.Hi + h_base) * g.Wi * a.Cin) * ES);      // wraps for top padding rows
#pragma unroll
      for (int k = 0; k < MAXG; ++k) {
        const unsigned off = (unsigned)(tb_c + gchk[k]) < lim ? toff + goff[k] * ES : 0x80000000u;
        gv[k] = __builtin_bit_cast(Vec16, __builtin_amdgcn_raw_buffer_load_b128(xrs, off, 0, 0));
      }
    } else if (planar_pf) {
      const long base = (long)n * a.x_planes * plane + (long)h_base * g.Wi;
#pragma unroll
      for (int k = 0; k < MAXG; ++k) {
        gv[k] = Vec16{{0, 0, 0, 0}};
        if ((unsigned)(tb_c + gchk[k]) < lim) {
#pragma unroll
          for (int c = 0; c < kPlanarPrefetch; ++c) {
            if (c < a.x_planes) {
              const long idx = base + goff[k] + c * plane;
              const float f = a.x_planar == 1 ? reinterpret_cast<const float*>(a.x)[idx] : Elem<T>::load(X + idx);
              gv[k].w[c] = __float_as_uint(f);
            }
          }
        }
      }
    }
  };
  auto commit = [&](int tile) {
    if constexpr (X2 > 0) {
#pragma unroll
      for (int k = 0; k < X2; ++k) { const int v = t + 256 * k; if (v < x2_tile_vecs) sX2[v] = gv2[k]; }
    }
    if constexpr (!planar) {
#pragma unroll
      for (int k = 0; k < MAXG; ++k) {
        const int pp = pix0 + k * PS;
        if (pp < npatch && gchk[k] != kPatchSlotInvalid) {       // static padding was zeroed once, before the loop
          Vec16 q = gv[k];
          if (has_pro && (unsigned)(tb_c + gchk[k]) < lim) {       // padding stays exactly zero
            float f[VE];
            Elem<T>::unpack(q, f);
#pragma unroll
            for (int j = 0; j < VE; ++j) f[j] = fmaxf(f[j] * psc[j] + psh[j], relu_lo);
            q = Elem<T>::pack(f);
          }
          sPatch[pp * cin_vecs + cv] = q;
        }
      }
    } else {
      // planar source: every patch pixel becomes a Cin-channel NHWC LDS pixel whose channels >= x_planes are zero
      int n, hq0;
      tile_origin(g, tile, 0, n, hq0);
      const long base = (long)n * a.x_planes * plane + (long)(hq0 * g.SI + g.oh) * g.Wi;
#pragma unroll
      for (int k = 0; k < MAXG; ++k) {
        const int pp = pix0 + k * PS;
        if (pp < npatch) {
          if (planar_pf) {
            float f[VE];
#pragma unroll
            for (int c = 0; c < VE; ++c) f[c] = c < kPlanarPrefetch ? __uint_as_float(gv[k].w[c]) : 0.f;
            sPatch[pp * cin_vecs] = Elem<T>::pack(f);
            for (int q = 1; q < cin_vecs; ++q) sPatch[pp * cin_vecs + q] = Vec16{{0, 0, 0, 0}};
          } else {
            const bool ok = (unsigned)(tb_c + gchk[k]) < lim;
            for (int q = 0; q < cin_vecs; ++q) {
              float f[VE];
#pragma unroll
              for (int c = 0; c < VE; ++c) {
                f[c] = 0.f;
                if (ok && q * VE + c < a.x_planes) {
                  const long idx = base + goff[k] + (long)(q * VE + c) * plane;
                  f[c] = a.x_planar == 1 ? reinterpret_cast<const float*>(a.x)[idx] : Elem<T>::load(X + idx);
                }
              }
              sPatch[pp * cin_vecs + q] = Elem<T>::pack(f);
            }
          }
        }
      }
    }
  };

  // Every value loaded from global memory before the tile loop must have ARRIVED before the loop: a load still pending at
  // loop entry makes the compiler wait with vmcnt(0) at its first use in EVERY iteration, and that wait (in-order
  // counter) also covers the next tile's prefetch.
#pragma unroll
  for (int c = 0; c < CT16; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(bv[c][j]));
#pragma unroll
  for (int j = 0; j < VE; ++j) { asm volatile("" ::"v"(psc[j])); asm volatile("" ::"v"(psh[j])); }
  const TileWalk walk = xcd_tile_walk(g.ntiles);
  // An always-true uniform test the compiler cannot see through, between the prefetch and the MFMA phase: the MFMA phase and the
  // epilogue then do not count as executed on every trip, and their tile-invariant values are not hoisted out of the tile loop --
  // hoisted, they stay live across it and the larger instantiations spill (second-source SO = 2 form: 5 -> 35 spilled VGPRs; 4x12: 20 -> 114)
  int live = 1;
  asm volatile("" : "+s"(live));
  int tile = walk.first;
  if (tile < walk.end) issue(tile);
  for (; tile < walk.end; tile += walk.step) {
    __syncthreads();                 // previous tile's fragment reads are done (also orders the block prologue)
    commit(tile);
    __syncthreads();
    if (tile + walk.step < walk.end) issue(tile + walk.step);     // in flight during the MFMA phase
    if (!live) continue;
    int n_t, hq0_t;
    tile_origin(g, tile, 0, n_t, hq0_t);
    const unsigned cmul = a.y_planes > 0 ? 1u : (unsigned)a.Cout;
    // one phase: acc[c][pt] = W_phase x patch
    auto run_phase = [&](const PatchPhase& P, f32x4 (&acc)[CT16][NPT], bool with_x2) {
      const int kvp = (P.ntaps * cin_vecs + 3) & ~3, wrow = kvp + 1, nks = kvp >> 2;
      const Vec16* sWp = sW + P.w_vec0;
      const int* sK = sKoff + P.koff0;
#pragma unroll
      for (int c = 0; c < CT16; ++c)
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) acc[c][pt] = (f32x4){0, 0, 0, 0};
      for (int ks = 0; ks < nks; ++ks) {
        const int kv = 4 * ks + gq;
        const int koff = sK[kv];
        Vec16 af[CT16];
#pragma unroll
        for (int c = 0; c < CT16; ++c) af[c] = sWp[(16 * c + r) * wrow + kv];
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) {
          int pb;
          if constexpr (!UNI) pb = pbase[pt];
          else pb = (col_row(pt) * g.SI * g.PW + col_wq0(pt) * g.SI) * a.Cin * ES + lane_pb;
          const Vec16 b = *reinterpret_cast<const Vec16*>(patch_bytes + pb + koff);
#pragma unroll
          for (int c = 0; c < CT16; ++c) acc[c][pt] = mma_vec<T>(af[c], b, acc[c][pt]);
        }
      }
      if constexpr (X2 > 0) {
        if (with_x2) {
          // the second source: its tile is stored by tile pixel index, K = Cin2 (zero weights beyond it)
          const int wrow2 = a.kvp2 + 1;
          for (int ks = 0; ks < (a.kvp2 >> 2); ++ks) {
            const int kv = 4 * ks + gq;
            Vec16 af[CT16];
#pragma unroll
            for (int c = 0; c < CT16; ++c) af[c] = sW2[(16 * c + r) * wrow2 + kv];
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt) {
              const int pl = (UNI ? (wv * NPT + pt) * 16 : 32 * wv + 16 * pt) + r;
              const Vec16 b = sX2[pl * cin2_vecs + kv];
#pragma unroll
              for (int c = 0; c < CT16; ++c) acc[c][pt] = mma_vec<T>(af[c], b, acc[c][pt]);
            }
          }
        }
      }
    };
    if constexpr (!UNI) {
      // ---- general geometry: per-lane output offsets (32-bit: the launcher guarantees the tensor fits), direct stores
      unsigned obase[2]; int ohq[2];
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) {
        int n, hq0;
        tile_origin(g, tile, pseg[pt] < 0 ? 0 : pseg[pt], n, hq0);
        ohq[pt] = (pseg[pt] >= 0 && n < g.N) ? hq0 + pj[pt] : (1 << 29);
        const unsigned hq = pseg[pt] >= 0 ? (unsigned)(hq0 + pj[pt]) : 0u;
        obase[pt] = a.y_planes > 0 ? ((unsigned)n * a.y_planes * a.Ho + hq * a.SO) * a.Wo + pwq[pt] * a.SO
                                   : (((unsigned)n * a.Ho + hq * a.SO) * a.Wo + pwq[pt] * a.SO) * cmul + 4 * gq;
      }
#pragma unroll
      for (int p = 0; p < kMaxPhases; ++p) {
        if (p >= a.nphase) break;
        const PatchPhase P = a.phases[p];
        f32x4 acc[CT16][NPT];
        run_phase(P, acc, p == a.x2_phase);
        // lane holds couts 16c + 4gq + j of its q-pixel of column tile pt, output pixel (hq*SO+ph, wq*SO+pw)
        const unsigned ph_off = ((unsigned)P.ph * a.Wo + P.pw) * cmul;
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) {
          const int hq = ohq[pt], wq = pwq[pt];
          const unsigned ob = obase[pt] + ph_off;
          if (hq < P.Hq && wq < P.Wq) {
            if (a.y_planes > 0) {
              // NCHW f32 output with y_planes (<= 16) real channels: the reconstruction layout of the reference
              if (gq * 4 < a.y_planes) {
                float* Yp = reinterpret_cast<float*>(a.y);
                const unsigned hw = (unsigned)a.Ho * a.Wo;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                  const int co = 4 * gq + jj;
                  if (co < a.y_planes) {
                    const float v = acc[0][pt][jj] + bv[0][jj];
                    st1[0][jj] += v;
                    st2[0][jj] += v * v;
                    Yp[ob + co * hw] = v;
                  }
                }
              }
            } else {
#pragma unroll
              for (int c = 0; c < CT16; ++c) {
                const int co = 16 * c + 4 * gq;
                if (co < a.Cout) {
                  float v[4];
#pragma unroll
                  for (int jj = 0; jj < 4; ++jj) {
                    v[jj] = acc[c][pt][jj] + bv[c][jj];
                    st1[c][jj] += v[jj];
                    st2[c][jj] += v[jj] * v[jj];
                  }
                  pstore4<TO>(Y + (ob + 16u * c), v, ACC);
                }
              }
            }
          }
        }
      }
    } else {
      // ---- uniform geometry: stage one output row-phase per wave in LDS, write whole lines
      char* sOutW = sOut + wvu * a.out_wave_bytes;
#pragma unroll
      for (int ph = 0; ph < SOT; ++ph) {
#pragma unroll
        for (int pw = 0; pw < SOT; ++pw) {
          const PatchPhase P = a.phases[a.phase_of[ph * SOT + pw]];
          f32x4 acc[CT16][NPT];
          run_phase(P, acc, a.phase_of[ph * SOT + pw] == a.x2_phase);
#pragma unroll
          for (int pt = 0; pt < NPT; ++pt) {
            if (a.y_planes > 0) {
              // planes [y_planes][NPT*16 pixels] f32 (SO == 1)
              if (gq * 4 < a.y_planes) {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                  const int co = 4 * gq + jj;
                  if (co < a.y_planes) {
                    const float v = acc[0][pt][jj] + bv[0][jj];
                    if (hq0_t + col_row(pt) < g.Hq) { st1[0][jj] += v; st2[0][jj] += v * v; }
                    reinterpret_cast<float*>(sOutW)[co * (NPT * 16) + pt * 16 + r] = v;
                  }
                }
              }
            } else {
              // channel-quad planes [pt][pw][c][gq] of 16 q x 4 channels: the 16 lanes of one gq write 16 consecutive
              // quads (conflict-free), the 16-byte skew of the plane pitch spreads the read-back over the banks
              TO* dst = reinterpret_cast<TO*>(sOutW + (((pt * a.SO + pw) * CT16) * 4 + gq) * kOutPitch) + r * 4;
              const bool rowok = has_stats && hq0_t + col_row(pt) < g.Hq;
#pragma unroll
              for (int c = 0; c < CT16; ++c) {
                if (16 * c < a.Cout) {                     // Cout is a multiple of 16 here: uniform
                  float v[4];
#pragma unroll
                  for (int jj = 0; jj < 4; ++jj) v[jj] = acc[c][pt][jj];
                  if (has_bias) {
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) v[jj] += bv[c][jj];
                  }
                  if (rowok) {
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) { st1[c][jj] += v[jj]; st2[c][jj] += v[jj] * v[jj]; }
                  }
                  pstore4<TO>(reinterpret_cast<TO*>(reinterpret_cast<char*>(dst) + c * 4 * kOutPitch), v, false);
                }
              }
            }
          }
        }
        // ---- wave-private LDS -> global, 16 bytes per lane (LDS operations of one wave complete in order)
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (a.y_planes > 0) {
          // the wave's NPT*16 pixels are consecutive in memory (whole rows of one image plane)
          float* Yp = reinterpret_cast<float*>(a.y);
          const unsigned hw = (unsigned)a.Ho * a.Wo;
          const unsigned pix0o = ((unsigned)n_t * a.y_planes * a.Ho + (unsigned)(hq0_t + col_row(0))) * a.Wo + col_wq0(0);
          const int nrows_ok = g.Hq - (hq0_t + col_row(0));                         // rows of this wave inside the image
          const int npx = min(NPT * 16, nrows_ok * g.Wq);
          // (no real loop here: a loop with stores would make the compiler wait for the prefetch in its preheader)
          const int i = lane * 4;                   // NPT*16 <= 128 pixels: one float4 per lane covers the run
#pragma unroll
          for (int pl = 0; pl < 16; ++pl) {
            if (pl < a.y_planes && i < npx)
              *reinterpret_cast<float4*>(Yp + pix0o + pl * hw + i) = *reinterpret_cast<const float4*>(sOutW + (pl * (NPT * 16) + i) * 4);
          }
        } else {
          const int pt_bytes = a.SO * CT16 * 4 * kOutPitch;                          // LDS bytes of one column tile
#pragma unroll
          for (int pt = 0; pt < NPT; ++pt) {
            const int hq = hq0_t + col_row(pt);
            if (hq < g.Hq) {
              const unsigned ob = (((unsigned)n_t * a.Ho + (unsigned)(hq * a.SO + ph)) * a.Wo + (unsigned)col_wq0(pt) * a.SO) * (unsigned)a.Cout;
              char* gdst = reinterpret_cast<char*>(Y + ob);
              const char* lsrc = sOutW + pt * pt_bytes;
#pragma unroll
              for (int it = 0; it < kOutIters; ++it) {
                const int i = lane + 64 * it;
                if (i < run16) {
                  Vec16 q;
                  if constexpr (sizeof(TO) == 2) {
                    const uint2 lo = *reinterpret_cast<const uint2*>(lsrc + rb_off[it]);
                    const uint2 hi = *reinterpret_cast<const uint2*>(lsrc + rb_off[it] + kOutPitch);
                    q.w[0] = lo.x; q.w[1] = lo.y; q.w[2] = hi.x; q.w[3] = hi.y;
                  } else {
                    q = *reinterpret_cast<const Vec16*>(lsrc + rb_off[it]);
                  }
                  if constexpr (ACC) {
                    const Vec16 e = *reinterpret_cast<const Vec16*>(gdst + i * 16);
                    constexpr int VO = 16 / sizeof(TO);
                    float fa[VO], fb[VO];
                    Elem<TO>::unpack(q, fa); Elem<TO>::unpack(e, fb);
#pragma unroll
                    for (int j = 0; j < VO; ++j) fa[j] += fb[j];
                    q = Elem<TO>::pack(fa);
                  }
                  *reinterpret_cast<Vec16*>(gdst + i * 16) = q;
                }
              }
            }
          }
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
    }
  }
  if (a.stats) {
#pragma unroll
    for (int c = 0; c < CT16; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          st1[c][j] += __shfl_xor(st1[c][j], o, 64);
          st2[c][j] += __shfl_xor(st2[c][j], o, 64);
        }
      }
    __syncthreads();
    if (r == 0) {
#pragma unroll
      for (int c = 0; c < CT16; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sStat[wv * 2 * CT + 16 * c + 4 * gq + j] = st1[c][j];
          sStat[wv * 2 * CT + CT + 16 * c + 4 * gq + j] = st2[c][j];
        }
    }
    __syncthreads();
    if (t < 2 * CT) {
      const float s = sStat[t] + sStat[2 * CT + t] + sStat[4 * CT + t] + sStat[6 * CT + t];
      const int which = t / CT, cl = t - which * CT;
      const int cs = a.y_planes > 0 ? a.y_planes : a.Cout;      // channel count of the statistics rows
      if (cl < cs) a.stats[(long)blockIdx.x * 2 * cs + (long)which * cs + cl] = s;
    }
  }
}

template <typename T, typename TO>
static int launch_patch_t(const PatchArgs& a, int dt, int gx, hipStream_t s) {
  int ct16 = (a.Cout + 15) / 16;
  if (ct16 == 3) ct16 = 4;
  const size_t lds = patch_conv_lds_bytes(a, dt);
  const int slots = patch_conv_slots(a, dt);
  dim3 grid(gx), block(256);
  // instances: general geometry NPT = 2; uniform geometry (LDS epilogue) CT16 = 1 -> NPT 2/4/8, 2 -> 2/4, 4 -> 2
#define MMVAE_PCK0(C_, G_, PL_, N_, U_, A_, S_, X_) hipLaunchKernelGGL((patch_conv_kernel<T, TO, C_, G_, PL_, N_, U_, A_, S_, X_>), grid, block, lds, s, a)
  // second source: only without accumulate / planar input, and only where the network uses it (C <= 32 main paths)
#define MMVAE_PCK(C_, G_, PL_, N_, U_, A_, S_) do { \
    if constexpr (!(PL_) && !(A_) && (C_) <= 2 && (N_) == 2 && sizeof(TO) == sizeof(T)) { \
      if (a.x2_slots > 2) MMVAE_PCK0(C_, G_, PL_, N_, U_, A_, S_, 4); else if (a.x2_slots > 0) MMVAE_PCK0(C_, G_, PL_, N_, U_, A_, S_, 2); else MMVAE_PCK0(C_, G_, PL_, N_, U_, A_, S_, 0); \
    } else { if (a.x2_slots > 0) { set_error("patch_conv: second source not available for this variant"); return MMVAE_ERR_UNSUPPORTED; } MMVAE_PCK0(C_, G_, PL_, N_, U_, A_, S_, 0); } } while (0)
  // planar inputs (stem, tail dgrad): SO = 1, no accumulate; general geometry: phases unrolled with guards (SOT unused)
#define MMVAE_PCL(C_, G_, PL_, N_, U_) do { \
    if (PL_) { if (a.accumulate || (U_ && a.SO != 1)) { set_error("patch_conv: planar input with accumulate / SO=%d", a.SO); return MMVAE_ERR_UNSUPPORTED; } \
               MMVAE_PCK(C_, G_, PL_, N_, U_, false, 1); } \
    else if (!U_ || a.SO == 1) { if (a.accumulate) MMVAE_PCK(C_, G_, false, N_, U_, true, 1); else MMVAE_PCK(C_, G_, false, N_, U_, false, 1); } \
    else { if (a.accumulate) MMVAE_PCK(C_, G_, false, N_, U_, true, 2); else MMVAE_PCK(C_, G_, false, N_, U_, false, 2); } } while (0)
#define MMVAE_PC(C_, N_, U_) do { \
    if (a.x_planar) { if (slots <= 4) MMVAE_PCL(C_, 4, true, N_, U_); else MMVAE_PCL(C_, 12, true, N_, U_); } \
    else { if (slots <= 4) MMVAE_PCL(C_, 4, false, N_, U_); else if (slots <= 8 && C_ == 1) MMVAE_PCL(C_, 8, false, N_, U_); else MMVAE_PCL(C_, 12, false, N_, U_); } } while (0)
  if (slots > 12) { set_error("patch_conv: %d staging slots > 12", slots); return MMVAE_ERR_UNSUPPORTED; }
  const int key = (ct16 * 16 + a.npt) * 2 + (a.uni ? 1 : 0);
  switch (key) {
    case (1 * 16 + 2) * 2: MMVAE_PC(1, 2, false); break;
    case (2 * 16 + 2) * 2: MMVAE_PC(2, 2, false); break;
    case (4 * 16 + 2) * 2: MMVAE_PC(4, 2, false); break;
    case (1 * 16 + 2) * 2 + 1: MMVAE_PC(1, 2, true); break;
    case (1 * 16 + 4) * 2 + 1: MMVAE_PC(1, 4, true); break;
    case (1 * 16 + 8) * 2 + 1: MMVAE_PC(1, 8, true); break;
    case (2 * 16 + 2) * 2 + 1: MMVAE_PC(2, 2, true); break;
    case (2 * 16 + 4) * 2 + 1: MMVAE_PC(2, 4, true); break;
    case (4 * 16 + 2) * 2 + 1: MMVAE_PC(4, 2, true); break;
    default: set_error("patch_conv: Cout=%d npt=%d uni=%d unsupported", a.Cout, a.npt, a.uni); return MMVAE_ERR_UNSUPPORTED;
  }
#undef MMVAE_PCL
#undef MMVAE_PCK
#undef MMVAE_PCK0
#undef MMVAE_PC
  const int rc = check_launch("patch_conv");
  return rc ? rc : gx;
}

#if PATCH_TU == 0
int launch_patch_conv_f32(const PatchArgs& a, int gx, hipStream_t s) { return launch_patch_t<float, float>(a, DT_F32, gx, s); }
#elif PATCH_TU == 1
int launch_patch_conv_bf16(const PatchArgs& a, int gx, hipStream_t s) { return launch_patch_t<bf16_t, bf16_t>(a, DT_BF16, gx, s); }
#else
int launch_patch_conv_bf16_f32(const PatchArgs& a, int gx, hipStream_t s) { return launch_patch_t<bf16_t, float>(a, DT_BF16, gx, s); }
#endif

}  // namespace mmvae
