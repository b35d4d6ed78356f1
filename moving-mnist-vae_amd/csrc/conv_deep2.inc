// deep2_conv_kernel: barrier-free implicit GEMM for the channel-heavy layers (Cin, Cout >= 32, one of them >= 64, on 1x1 .. 8x8 feature
// maps): Conv2d fwd, ConvT fwd and both dgrads in gather form,
//     y[n, hq*SO+ph, wq*SO+pw, co] (+)= bias[co] + sum_{tap, ci} pro(x[n, hq*SI+dh, wq*SI+dw, ci]) * w[co][tap][ci].
//
// Measured on its round-1 predecessor (deep_conv_kernel, deleted in round 4; in-kernel cycle stamps): its K-step -- weights through a double-buffered
// LDS tile, ONE block barrier per 64 k-values -- takes 1000 cycles plus the MFMA time whatever the tile, because the 8
// waves of the single resident block run their LDS phase and their MFMA phase in lock step, and ~10 us per block go to
// set-up, staging and the epilogue with nobody to hide them behind: 7-14 % of the MFMA peak on every layer.
//
// Here the weights never touch LDS.  A wave owns 32 output channels and ALL pixels of the tile:
//   * the A operand (weights, [cout][tap][cin], 64-byte row chunks) is loaded from L2 straight into MFMA fragment
//     registers, 16 rows x 64 B per instruction, one K-loop unit (up to 4 chunks) ahead -- private to the wave, so there is no
//     barrier in the K loop and waves drift apart (one wave's MFMAs cover another's loads);
//   * the B operand (activations) is the staged patch of `ipt` whole images in LDS, as before: unpadded pixels, fused
//     BN+ReLU applied once per element, taps reach their pixels through tab[tap][q-pixel] (out-of-range -> zero pixel);
//     a B fragment is reused by both of the wave's cout fragments: per 64-byte K chunk 2 global loads + NPT LDS reads
//     feed 2*NPT MFMAs (NPT = 8: L1 and LDS both at half of what the MFMA pipe consumes);
//   * a block is Cout/32 (at most 8) such waves sharing one patch, so the patch is staged once per tile for all output
//     channels, small enough (18-70 KB) for 2-8 blocks per CU, and the only barriers are the two around staging;
//   * BatchNorm statistics come from the f32 accumulators; a wave owns its channels, so no cross-wave reduction.
//
// LDS carve: [patch: (npix_in + 1) x pitch][opix: TPX u32][stat: 2 x 32*nw f32][tab: ntaps_all x TPX u16]
#include "kernels.hpp"
#include "tile_common.hpp"

namespace mmvae {

// LITE: 2-chunk units, two register sets (<= 168 VGPRs at NPT = 8): three waves per SIMD, so that 640 4-wave tiles run in ONE round.
// Measured (tools/deep_probe.py): 10-25 % faster where a block is 4 or 8 waves (Cout >= 128), 5-15 % slower for the 1-2 wave blocks of
// the 32/64-cout layers, which keep the 4-chunk units and three register sets.
// F8 (bf16 storage, forward convs of the fp8 mode): the staged activations are quantised to e4m3 behind the fused BN+ReLU (one byte per
// element in LDS, pixel pitch Cin + 16), the fragment-major weights are e4m3 bytes (static per-layer scale); a 64-byte chunk of a weight
// row is 64 k-values = two v_mfma_f32_16x16x32_fp8_fp8, a lane's 16 bytes = its 8 bytes of each.
template <typename T, typename TO, int NPT, int CPT, bool ACC, bool LITE, bool F8 = false>
__device__ __forceinline__ void deep2_conv_body(const DeepArgs& a) {
  static_assert(!F8 || (sizeof(T) == 2 && !ACC), "fp8 MFMA: bf16 storage, forward convolutions");
  constexpr int VE = Elem<T>::kVec;
  constexpr int ES = sizeof(T);
  constexpr int TPX = NPT * 16;
  constexpr int kSV = 8;
  constexpr int G = CPT < (LITE ? 2 : 4) ? CPT : (LITE ? 2 : 4);   // chunks per K-loop unit (CPT = 64-byte chunks per tap of a weight row)
  constexpr int NB = LITE ? 2 : NPT >= 8 ? 3 : 4;    // register sets of G weight chunks per cout fragment
  constexpr int UPT = CPT / G;                       // units per tap: 1, 2 (bf16 Cin = 256, f32 Cin = 128) or 4 (f32 Cin = 256)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, nthr = blockDim.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6), gq = lane >> 4, r = lane & 15;
  const int c0 = (blockIdx.y * a.nw + wv) * 32;     // this wave's first output channel
  const int cin_vecs = a.Cin / VE;
  constexpr int LES = F8 ? 1 : ES;                   // bytes per element in LDS and in the weight matrix
  const int pitch = F8 ? a.Cin + 16 : a.Cin * ES + 32;   // bytes per staged pixel: (pitch / 16) % 4 == 2 keeps the ds_read_b128 lane groups of a
                                                    // B fragment (16 pixels x 4 k-slices) on 16 distinct 16-byte bank slots
  const int npix_in = a.ipt * a.Hi * a.Wi;
  char* sPatch = smem;
  unsigned* sOpix = reinterpret_cast<unsigned*>(sPatch + (size_t)(npix_in + 1) * pitch);
  float* sStat = reinterpret_cast<float*>(sOpix + TPX) + wv * 64;      // this wave's [2][32]: sum, sum of squares of its couts
  unsigned short* sTab = reinterpret_cast<unsigned short*>(sOpix + TPX + 64 * a.nw);
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  TO* __restrict__ Y = reinterpret_cast<TO*>(a.y);
  const bool has_pro = a.pro_scale != nullptr, has_bias = a.bias != nullptr, has_stats = a.stats != nullptr;
  const float relu_lo = a.pro_relu ? 0.f : -__builtin_inff();
  const int HqWq = a.Hq * a.Wq;

  const int cv = t % cin_vecs, pix0 = t / cin_vecs, PS = nthr / cin_vecs;
  // ---- per-block tables (tile-invariant), one pass over the q-pixel slots:
  //   opix[slot] = (image in tile) << 16 | hq << 8 | wq of the slot's output pixel, or ~0u
  //   tab[tap][slot] -> staged pixel index of the tap's input pixel (npix_in = the zero pixel)
  // The tap loop is unrolled over the kernel-argument array so its (dh, dw) arrive by a few wide scalar loads.
  for (int p = t; p < TPX; p += nthr) {
    unsigned o = ~0u;
    int img = 0, hq = 0, wq = 0;
    const bool live = p < a.ipt * HqWq;
    if (live) {
      img = p / HqWq;
      const int rem = p - img * HqWq;
      hq = rem / a.Wq; wq = rem - hq * a.Wq;
      o = ((unsigned)img << 16) | ((unsigned)hq << 8) | (unsigned)wq;
    }
    sOpix[p] = o;
    const int hb = hq * a.SI, wb = wq * a.SI, ib = img * a.Hi;
#pragma unroll
    for (int tap = 0; tap < kMaxTaps; ++tap)
      if (tap < a.ntaps_all) {
        const int hi = hb + a.taps[tap].dh, wi = wb + a.taps[tap].dw;
        const bool in = live && hi >= 0 && hi < a.Hi && wi >= 0 && wi < a.Wi;
        sTab[tap * TPX + p] = (unsigned short)(in ? (ib + hi) * a.Wi + wi : npix_in);
      }
  }
  for (int i = t; i < pitch / 16; i += nthr) reinterpret_cast<Vec16*>(sPatch + (size_t)npix_in * pitch)[i] = Vec16{{0, 0, 0, 0}};
  sStat[lane] = 0.f;

  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int n0 = tile * a.ipt;
    const int nimg = min(a.ipt, a.N - n0);
    __syncthreads();                                 // the previous tile's fragment reads are done (first: tables written)
    // ---- stage the input pixels of the tile's images (contiguous in memory), BN+ReLU applied once per element
    {
      const T* src = X + (long)n0 * a.Hi * a.Wi * a.Cin + cv * VE;
      const int nvalid = nimg * a.Hi * a.Wi;
      float psc[VE], psh[VE];                        // re-read per tile (L1/L2 hits): 16 registers the K loop keeps free
#pragma unroll
      for (int j = 0; j < VE; j += 4) {
        const float4 sc = has_pro ? *reinterpret_cast<const float4*>(a.pro_scale + cv * VE + j) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 sh = has_pro ? *reinterpret_cast<const float4*>(a.pro_shift + cv * VE + j) : make_float4(0.f, 0.f, 0.f, 0.f);
        psc[j] = sc.x; psc[j + 1] = sc.y; psc[j + 2] = sc.z; psc[j + 3] = sc.w;
        psh[j] = sh.x; psh[j + 1] = sh.y; psh[j + 2] = sh.z; psh[j + 3] = sh.w;
      }
      for (int p0 = pix0; p0 < npix_in; p0 += kSV * PS) {      // kSV vectors in flight per thread: one memory round trip for most tiles
        Vec16 q[kSV];
#pragma unroll
        for (int k = 0; k < kSV; ++k) {
          const int p = p0 + k * PS;
          q[k] = Vec16{{0, 0, 0, 0}};
          if (p < nvalid) q[k] = *reinterpret_cast<const Vec16*>(src + (long)p * a.Cin);
        }
#pragma unroll
        for (int k = 0; k < kSV; ++k) {
          const int p = p0 + k * PS;
          if (p < npix_in) {
            if (has_pro && p < nvalid) {
              float f[VE];
              Elem<T>::unpack(q[k], f);
#pragma unroll
              for (int j = 0; j < VE; ++j) f[j] = fmaxf(f[j] * psc[j] + psh[j], relu_lo);
              q[k] = Elem<T>::pack(f);
            }
            if constexpr (F8) {
              float f[VE];
              Elem<T>::unpack(q[k], f);
              *reinterpret_cast<uint2*>(sPatch + (size_t)p * pitch + cv * 8) = pack8_fp8(f);
            } else {
              *reinterpret_cast<Vec16*>(sPatch + (size_t)p * pitch + cv * 16) = q[k];
            }
          }
        }
      }
    }
    __syncthreads();
    for (int ph = 0; ph < a.nphase; ++ph) {
      const DeepPhase P = a.phases[ph];
      const long rowbytes = (long)P.ntaps * a.Cin * LES;
      // this lane's 16 bytes of chunk 0 of the wave's two A fragments (couts c0.. and c0 + 16..), chunk j at + j * cstride:
      //   row-major [cout][tap][cin]: row c0 + r, bytes gq*16 of each 64-byte chunk;  fragment-major: 1 KB per (16 couts, chunk)
      // Row r of fragment m is cout c0 + 8*(r/4) + 4*m + r%4, so that a lane's 2 x 4 results are 8 CONSECUTIVE couts of its pixel
      // (one 16-byte store); the fragment-major pack (frag_index, conv_gemm.hip) applies the same permutation.
      const int cstride = a.wfrag ? 1024 : 64;
      const char* wl0 = reinterpret_cast<const char*>(a.w) + P.w_off * LES +
                        (a.wfrag ? (long)c0 * rowbytes + lane * 16 : (long)(c0 + 8 * (r >> 2) + (r & 3)) * rowbytes + gq * 16);
      const char* wl1 = wl0 + (a.wfrag ? 16 : 4) * rowbytes;
      f32x4 acc[2][NPT];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) acc[m][pt] = (f32x4){0, 0, 0, 0};
      // The K loop walks units of G chunks (a tap, or part of one).  Every load is unconditional (the tail re-reads the last unit), so
      // the compiler counts vmcnt exactly; the sched_barriers keep it from sinking the prefetch down to its use.
      const int nunits = P.ntaps * UPT;
      auto load_unit = [&](Vec16 (&buf)[G][2], int unit) {
        const int jb = min(unit, nunits - 1) * G * cstride;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          buf[g][0] = *reinterpret_cast<const Vec16*>(wl0 + jb + g * cstride);
          buf[g][1] = *reinterpret_cast<const Vec16*>(wl1 + jb + g * cstride);
        }
      };
      auto tap_pixels = [&](unsigned (&pb)[NPT], int tap) {
        const unsigned short* tb = sTab + (P.tap0 + tap) * TPX + r;
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) pb[pt] = __umul24((unsigned)tb[pt * 16], (unsigned)pitch) + gq * (F8 ? 8 : 16);
      };
      auto mul_unit = [&](const Vec16 (&buf)[G][2], const unsigned (&pb)[NPT], int cc0) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if constexpr (F8) {
            // two 32-k-value MFMAs per chunk: the lane's 8 bytes of k-block 0 (bytes 8gq ..) and of k-block 1 (32 + 8gq ..)
            long bl[NPT], bh[NPT];
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt) {
              bl[pt] = *reinterpret_cast<const long*>(sPatch + pb[pt] + (cc0 + g) * 64);
              bh[pt] = *reinterpret_cast<const long*>(sPatch + pb[pt] + (cc0 + g) * 64 + 32);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
              const long al = (long)(((unsigned long)buf[g][m].w[1] << 32) | buf[g][m].w[0]);
              const long ah = (long)(((unsigned long)buf[g][m].w[3] << 32) | buf[g][m].w[2]);
#pragma unroll
              for (int pt = 0; pt < NPT; ++pt) {
                acc[m][pt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(al, bl[pt], acc[m][pt], 0, 0, 0);
                acc[m][pt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(ah, bh[pt], acc[m][pt], 0, 0, 0);
              }
            }
          } else {
            Vec16 bf[NPT];
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt) bf[pt] = *reinterpret_cast<const Vec16*>(sPatch + pb[pt] + (cc0 + g) * 64);
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt) {
              acc[0][pt] = mma_vec<T>(buf[g][0], bf[pt], acc[0][pt]);
              acc[1][pt] = mma_vec<T>(buf[g][1], bf[pt], acc[1][pt]);
            }
          }
        }
      };
      // NB register sets rotate: while unit u is multiplied, units u + 1 .. u + NB - 1 are in flight (an L2 round trip under load is
      // ~1.2 us, a unit's MFMAs 0.2-0.8 us)
      Vec16 buf[NB][G][2];
      unsigned pb[NPT];
#pragma unroll
      for (int b = 0; b < NB - 1; ++b) load_unit(buf[b], b);
      for (int u = 0; u < nunits; u += NB) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const int uu = u + b;
          load_unit(buf[(b + NB - 1) % NB], uu + NB - 1);
          __builtin_amdgcn_sched_barrier(0);
          if (uu < nunits) {
            if (UPT == 1 || (uu & (UPT - 1)) == 0) tap_pixels(pb, uu / UPT);
            mul_unit(buf[b], pb, (uu & (UPT - 1)) * G);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // ---- epilogue of this phase: lane holds couts c0 + 8gq + 4m + j of its q-pixel of column tile pt
      float bv[8], st1[8], st2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        bv[j] = has_bias ? a.bias[c0 + 8 * gq + j] : 0.f;
        st1[j] = 0.f; st2[j] = 0.f;
      }
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt) {
        const unsigned op = sOpix[pt * 16 + r];
        const int img = (int)(op >> 16), hq = (int)((op >> 8) & 255u), wq = (int)(op & 255u);
        if (op != ~0u && img < nimg && hq < P.Hq && wq < P.Wq) {
          const unsigned ob = ((((unsigned)(n0 + img) * a.Ho + (unsigned)(hq * a.SO + P.ph)) * a.Wo + (unsigned)(wq * a.SO + P.pw)) * (unsigned)a.Cout) +
                              (unsigned)(c0 + 8 * gq);
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = acc[j >> 2][pt][j & 3] + bv[j];
#pragma unroll
          for (int j = 0; j < 8; ++j) { st1[j] += v[j]; st2[j] += v[j] * v[j]; }
          dstore8<TO>(Y + ob, v, ACC);
        }
      }
      if (has_stats) {
        // sum over the 16 pixel-lanes that share gq (DPP row rotations and quad permutes: every lane of the row ends with the row's
        // sum) and park it in the wave's LDS row (the wave owns its 32 channels)
#pragma unroll
        for (int j = 0; j < 8; ++j) { st1[j] = row16_sum(st1[j]); st2[j] = row16_sum(st2[j]); }
        if (r == 0) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            sStat[8 * gq + j] += st1[j];
            sStat[32 + 8 * gq + j] += st2[j];
          }
        }
      }
    }
  }
  if (has_stats) {
    // lane l: sum (l < 32) or sum of squares of channel c0 + (l & 31); parked by lanes r == 0 of this wave only
    a.stats[(long)blockIdx.x * 2 * a.Cout + (long)(lane >> 5) * a.Cout + c0 + (lane & 31)] = sStat[lane];
  }
}

template <typename T, typename TO, int NPT, int CPT, bool ACC>
__global__ __launch_bounds__(512, 2) void deep2_conv_kernel(DeepArgs a) { deep2_conv_body<T, TO, NPT, CPT, ACC, false>(a); }
template <typename T, typename TO, int NPT, int CPT, bool ACC>
__global__ __launch_bounds__(512, 3) void deep2_conv_lite_kernel(DeepArgs a) { deep2_conv_body<T, TO, NPT, CPT, ACC, true>(a); }
template <typename T, typename TO, int NPT, int CPT, bool ACC>
__global__ __launch_bounds__(512, 2) void deep2_conv_f8_kernel(DeepArgs a) { deep2_conv_body<T, TO, NPT, CPT, false, false, true>(a); }
template <typename T, typename TO, int NPT, int CPT, bool ACC>
__global__ __launch_bounds__(512, 3) void deep2_conv_f8_lite_kernel(DeepArgs a) { deep2_conv_body<T, TO, NPT, CPT, false, true, true>(a); }

template <typename T, typename TO>
static int launch_deep2_t(const DeepArgs& a, int dt, int gx, hipStream_t s) {
  const size_t lds = deep2_conv_lds_bytes(a, dt);
  dim3 grid(gx, a.Cout / (32 * a.nw)), block(64 * a.nw);
#define MMVAE_D2K(K_, N_, C_, A_) do { \
    static bool attr_set = false; \
    if (!attr_set) { \
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&K_<T, TO, N_, C_, A_>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
      if (e != hipSuccess) { set_error("deep2_conv: hipFuncSetAttribute: %s", hipGetErrorString(e)); return MMVAE_ERR_HIP; } \
      attr_set = true; \
    } \
    hipLaunchKernelGGL((K_<T, TO, N_, C_, A_>), grid, block, lds, s, a); } while (0)
#define MMVAE_D2(N_, C_, A_) do { if (a.nw >= 4) MMVAE_D2K(deep2_conv_lite_kernel, N_, C_, A_); else MMVAE_D2K(deep2_conv_kernel, N_, C_, A_); } while (0)
#define MMVAE_D2C(N_, C_) do { if (a.accumulate) MMVAE_D2(N_, C_, true); else MMVAE_D2(N_, C_, false); } while (0)
#define MMVAE_D2N(N_) do { \
    constexpr int kC0 = sizeof(T) == 2 ? 1 : 2;      /* Cin = 32 */ \
    if (cpt == kC0) MMVAE_D2C(N_, kC0); else if (cpt == 2 * kC0) MMVAE_D2C(N_, 2 * kC0); else if (cpt == 4 * kC0) MMVAE_D2C(N_, 4 * kC0); \
    else if (cpt == 8 * kC0) MMVAE_D2C(N_, 8 * kC0); \
    else { set_error("deep2_conv: Cin=%d unsupported", a.Cin); return MMVAE_ERR_UNSUPPORTED; } } while (0)
  const int cpt = 1 << a.cpt_log2;
  if (a.fp8) {
    // e4m3 weights and LDS bytes: chunks per tap = Cin / 64
    if constexpr (sizeof(T) == 2 && sizeof(TO) == 2) {
      if (a.accumulate || !a.wfrag) { set_error("deep2_conv: fp8 needs fragment-major weights and no accumulate"); return MMVAE_ERR_UNSUPPORTED; }
      /* the 8-tile fp8 form keeps 2 x 8 B-operand pairs live: it spills under the 168-register cap, so only the 2- and 4-tile forms run 3 waves per SIMD */
#define MMVAE_D2F(N_, C_) do { if (a.nw >= 4 && N_ < 8) MMVAE_D2K(deep2_conv_f8_lite_kernel, N_, C_, false); else MMVAE_D2K(deep2_conv_f8_kernel, N_, C_, false); } while (0)
#define MMVAE_D2FN(N_) do { if (cpt == 1) MMVAE_D2F(N_, 1); else if (cpt == 2) MMVAE_D2F(N_, 2); else if (cpt == 4) MMVAE_D2F(N_, 4); \
      else { set_error("deep2_conv: fp8 Cin=%d unsupported", a.Cin); return MMVAE_ERR_UNSUPPORTED; } } while (0)
      if (a.npt == 8) MMVAE_D2FN(8); else if (a.npt == 4) MMVAE_D2FN(4); else if (a.npt == 2) MMVAE_D2FN(2);
      else { set_error("deep2_conv: npt=%d unsupported", a.npt); return MMVAE_ERR_UNSUPPORTED; }
#undef MMVAE_D2FN
#undef MMVAE_D2F
      const int rc8 = check_launch("deep2_conv_f8");
      return rc8 ? rc8 : gx;
    } else { set_error("deep2_conv: fp8 needs bf16 storage"); return MMVAE_ERR_UNSUPPORTED; }
  }
  if (a.npt == 8) MMVAE_D2N(8);
  else if (a.npt == 4) MMVAE_D2N(4);
  else if (a.npt == 2) MMVAE_D2N(2);
  else { set_error("deep2_conv: npt=%d unsupported", a.npt); return MMVAE_ERR_UNSUPPORTED; }
#undef MMVAE_D2N
#undef MMVAE_D2C
#undef MMVAE_D2
#undef MMVAE_D2K
  const int rc = check_launch("deep2_conv");
  return rc ? rc : gx;
}

#if DEEP_TU == 0
int launch_deep2_conv_f32(const DeepArgs& a, int gx, hipStream_t s) { return launch_deep2_t<float, float>(a, DT_F32, gx, s); }
#elif DEEP_TU == 1
int launch_deep2_conv_bf16(const DeepArgs& a, int gx, hipStream_t s) { return launch_deep2_t<bf16_t, bf16_t>(a, DT_BF16, gx, s); }
#else
int launch_deep2_conv_bf16_f32(const DeepArgs& a, int gx, hipStream_t s) { return launch_deep2_t<bf16_t, float>(a, DT_BF16, gx, s); }
#endif

}  // namespace mmvae
