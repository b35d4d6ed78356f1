"""Op-level bit and float64 tests of the three MFMA kernels a bf16 64x64 training step launches around encoder.layer1, through the C ABI:
  mmvae_conv2d_fwd_pair       conv3_stream_kernel<2, SC = true, PRO>: layer1.conv1 (3x3 s2) and the block's 1x1 s2 shortcut from one read of
                              the stem activation -- the shortcut accumulators, the second store and the second statistics rows;
  mmvae_conv2d_dgrad_bn_sums  conv3_stream_kernel<1, false, false, BS = true> (launch_conv3_stream_bwd): layer1.conv2's data gradient with bn1's
                              backward sums from the same pass -- the masked sums, the `yv` prefetch, g = the bf16-rounded result;
  mmvae_stem_bwd_dg           stem_bwd_kernel<bf16_t, 0, DG = true> (launch_stem_bwd_dg): the stem backward with its incoming gradient recomputed
                              row by row from dy1 / dys (conv1's nine taps in four stride phases plus the shortcut).
Conventions and helpers of test_conv_lattice_gpu.py, test_conv_join_ops_f64_gpu.py, test_stem_ops_f64_gpu.py and test_upblock_ops_f64_gpu.py
(imported, not rewritten): every device buffer is a window of its documented size in a pattern-filled arena with the guards checked; y, y_sc
and dx start as 0xFF bytes; statistics and sums buffers are pattern-filled to their macro capacity (MMVAE_FWD_PAIR_MAX_ROWS = 512,
MMVAE_DGRAD_BN_SUMS_MAX_ROWS = 768) and rows past the returned count must still hold the pattern; two runs give the same bits.

Lattice regime (bit equality, the argument of test_conv_lattice_gpu.py): operands are small integers, every majorant (the absolute-value
convolutions, per-channel sum |v|, sum v^2, sum |g|, sum |g y|, per-tap sum |gm| |patch|, sum |gm y0|) is asserted <= 2^23 on the CPU (first
test, no GPU) and again in front of each GPU comparison, so every f32 sum has one possible value under any order.  Generator ladder: weight
density 1/4, 1/8, 1/16, then amplitude 1 (at most 10 % of the cases may leave the first rung: one of 19 does, the pair at N = 37 with the ReLU prologue, to density 1/8).  The mask operands bn_scale / bn_shift
are integers, shift = -scale * t with t in the value range of y, so y * scale + shift is exactly 0 on about 1/7 of the elements of every case
(`>` against `>=` shows) and a negative scale occurs in every case.
  pair    y and y_sc = rbf(exact integer) bit for bit; the float64 sum of the first `rows` rows of each statistics tensor = the exact sums of the
          f32 accumulators; rows of blocks without work are zeros; three prologue forms with a positive shift (a prologue applied to the zero
          padding shows).  Wide regime: a dense patch of amplitude 60 in image 0 on a sparse background (weights of density 1/16 and 1/4), so that some |y| and some |y_sc| pass
          256 (they round in the store; the statistics must not) while sum v^2 stays under the cap: asserted on the CPU for every case.
  dgrad   dx bits; both sum rows exact with g taken from the ROUNDED dx; the same dense patch in dy: the sums over rounded and over exact dx
          differ in both rows in every case (asserted on the CPU), so sums taken from the accumulator fail.
  stem    g = rbf(exact integer data gradient of conv1 plus shortcut) on the host (one accumulator, one rounding in the kernel);
          mmvae_stem_bwd_dg must give the bits of mmvae_stem_bwd fed that g for dweight, dgamma, dbeta from the same nonzero starting values:
          both routes' partial sums are exact integers, stem_bwd_finalize adds them in double, so any grid gives the same sums (N = 97: 768
          blocks against 776).  That comparison cannot see what the two routes share (the mask line), so the outputs are also checked on the
          host: dbeta = pre + (float) sum gm is one f32 addition of known numbers (bits), dweight and dgamma are the finalize formula in
          double plus that addition (u of the term and of the result, 2^-46 of the term magnitudes).  dy1 and dys are nonzero in row 0, column 0, the last row and the last column of their maps (asserted).

Real-valued regime: inputs rounded to bf16, weights handed over in f32 and rounded by the pack.
  Bit contracts, no tolerance: the pair's y, returned rows and stats = mmvae_conv2d_fwd's (stride 2, same prologue); mmvae_conv2d_dgrad_bn_sums's
  dx = mmvae_conv2d_dgrad's.  (dx is also gated against float64 with the slab rule, 9 slabs.)
  y_sc against the float64 conv of the bf16 prologue output with the bf16 weights: the MFMA slab rule of test_conv_join_ops_f64_gpu.py (K = 32
  is one slab: 32 u A) plus the prologue's midpoint uncertainty carried through |w|, plus half a bf16 ulp.
  stats_sc and the two backward sum rows against the float64 sums of the same terms (backward: g from the device's OWN dx, so a one-ulp
  disagreement in dx is not counted twice).  Summation bound: the ORDER-FREE MAJORANT was used, not the rebuilt walk -- u x (additions on the
  longest chain) x sum |terms|, the chain being 8 rows per unit x the units of the busiest wave (sequential f32 sum per lane) + 4 (row16_sum)
  + 2 (the four waves), one more u for a product; the test's own sum over rows is float64.  SLOP = 1.01.
  Mask ambiguity: y_pre (dgrad) and y0 (stem) are resampled until no element has |y s + b| <= 4u (|y s| + |b|); the count is asserted zero on
  the CPU and nothing is excluded from a gate.
  Stem DG: dweight, dgamma, dbeta against ref_stem_bwd_rq and stem_bwd_bounds of test_stem_ops_f64_gpu.py (imported) evaluated at g =
  rbf(g64), g64 the float64 data gradient with bf16 weights, plus the first-order term sum_i |d out / d g_i| e_i for g's own uncertainty (the
  outputs are affine in gm given mask and statistics; the three terms of d dW / d g_i are bounded separately): e_i = 0 unless a bf16 rounding
  midpoint lies within the slab bound of element i (32 u x {2, 2, 2, 4} slabs by stride phase x A), then one bf16 step.  |Rq - R64| is
  printed and gates nothing.

Cases (the launchers' grid arithmetic, rebuilt on the host and asserted by test_walks_are_what_the_cases_claim):
  pair and dgrad, N in {1, 3, 5, 37}: two 8-row units per image.  N = 1: 2 units for 32 wave slots, 6 of 8 blocks write zero rows; N = 3: 6
  units for 8 XCD groups, two groups empty; N = 5: per = 2, groups 5 - 7 empty, the last used group full; N = 37: 74 units on 16 blocks, two
  waves per group walk a second unit (ring reuse, `yv` carried across a unit boundary), group 7 has four units.
  stem DG, N in {1, 3, 97}: 32 one-row slabs per image; N = 97 is the smallest at which a wave walks a second slab (3104 slabs, 3072 waves).
Refusals (f32; H = 32 for the dgrad; S = 32 for the stem; the pair off its shape; a null y_pre / sums / weight_sc; N = 0; dtype 7): a negative
code, every output and scratch byte untouched, and an empty census segment -- not even a packing launch.  launch_conv3_stream_bwd used to
refuse after its caller's pack; the entry point checks first.
Census (last test): one child process under MMVAE_LAUNCH_STATS / MMVAE_LAUNCH_SEQ, an 8-element mmvae_convert between calls; the families must be
exactly LAUNCHES'.

mmvae_stem_bwd_dg takes `dtype` and `S` like mmvae_stem_bwd (the refusals of f32 and of S = 32 need them).

Measured on the MI355X: all 45 tests pass at the first device run; the file takes 5.6 - 6.0 s (40 GPU tests, the census child 2.1 s of it, the
slowest other test 0.3 s: the real-valued stem at N = 97), the five CPU self-checks 3.6 s.  Every lattice case bit-exact, every bit contract
holds.  Worst err / bound: y_sc 0.9992 (rounding ties: the half ulp is then the whole bound), stats_sc 0.24 (0.004 - 0.02 but for the affine
prologue at N = 5 and 37), dx 0.987, the backward sum rows 0.012; stem DG real-valued dweight 0.010, dgamma 0.017, dbeta 0.005 (the bound is
dominated by the one-bf16-step term of the 3.7 % of g's elements that sit near a rounding midpoint; the lattice regime is what pins this kernel),
stem DG lattice against the host: dbeta bits, dweight 0.90, dgamma 0.76.  Largest majorants, fractions of the 2^23 cap: sum y^2 0.67 (small),
0.47 (wide), sum y_sc^2 0.37, per-tap sum |gm| |patch| 0.053.  LAUNCHES and PACKS were filled from the code and the first device run
corrected nothing.
Mutation check (each in a scratch copy of the kernel, built and run once, not committed) -- the tests that failed:
  * the `hq + 1 < Hs` zero row dropped (the next image's row 0 read instead): test_stem_dg_lattice and test_stem_dg_real at N = 3 and 97 (at
    N = 1 the row read is guard bytes, 0xA5A5 = -2.9e-16 as bf16, and nothing shows);
  * slot 9's weights (the shortcut) on row buffer 0 (dy1): all six stem tests;
  * `>=` in stem_bwd_kernel's mask: test_stem_dg_lattice, every N, at the dbeta bits (the comparison with mmvae_stem_bwd passes: it runs the same line);
  * `>=` in conv3_stream_kernel's mask: test_dgrad_bn_sums_lattice, every N;
  * sums from `v` instead of `vr`: test_dgrad_bn_sums_lattice and test_dgrad_bn_sums_real, every N;
  * stats_sc not stored by blocks without work: all 24 pair tests (a zero row expected, the fill pattern found).
"""
import collections
import ctypes
import functools
import json
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_stem_ops_f64_gpu as ST  # noqa: E402
from test_conv_join_ops_f64_gpu import Case as JCase, main_term, second_term  # noqa: E402
from test_conv_lattice_gpu import (CAP, PROS, RUNGS, _ints, _masked, act, assert_exact, equal_or_explain, nchw64, nhwc)  # noqa: E402
from test_upblock_ops_f64_gpu import (ERR_ARG, ERR_UNSUPPORTED, F64, SLOP, U, Dev, P, _header_macro, _L, _ratio, _spacing, affine_pre,  # noqa: E402
                                      conv_g, gate, gpu, half_ulp_bf16, plane_slices, rbf, rbf_e, relu_e, same_bits, stream, stream_grid,
                                      stream_walk, v4)

BF = torch.bfloat16
PAIR_ROWS, DGRAD_ROWS = 512, 768                                            # MMVAE_FWD_PAIR_MAX_ROWS, MMVAE_DGRAD_BN_SUMS_MAX_ROWS (checked below)
PAIR_SCRATCH, DGRAD_SCRATCH, BN_SCRATCH = 20480, 18432, 16 << 20
FWD_STATS_ROWS = 4096                                                       # MMVAE_CONV_STATS_MAX_ROWS: mmvae_conv2d_fwd's capacity
CONV_NS = (1, 3, 5, 37)
STEM_NS = (1, 3, 97)
JC = lambda N: JCase("enc", 0, 32, 32, 3, 2, 1, 32, N)                      # layer1.conv1 + its 1x1 shortcut, as test_conv_join_ops_f64_gpu.py writes them


# ================================================================ launch geometry (rebuilt from the launchers)
def conv_geo(N, cap):
    """launch_conv3_stream (stride 2: cap 512) / launch_conv3_stream_bwd (cap 768): two 8-row units per image, 4 waves a block, never below
    8 blocks; the XCD-aware walk.  depth: additions on the longest chain of a statistics sum."""
    nunits = 2 * N
    gx = stream_grid(nunits, cap, 4, 8)
    walk = stream_walk(nunits, gx, 4)
    most = max(len(v) for v in walk.values())
    idle = [b for b in range(gx) if not any(walk[(b, s)] for s in range(4))]
    return dict(nunits=nunits, gx=gx, walk=walk, most=most, idle=idle, depth=8 * most + 6)


def dg_geo(N):
    """launch_stem_bwd_dg: 32 one-row slabs per image, wave gw takes slabs gw, gw + 4 gx, ...; at most 768 blocks."""
    nslabs = 32 * N
    gx = min(768, (nslabs + 3) // 4)
    return dict(nslabs=nslabs, gx=gx, spw=-(-nslabs // (4 * gx)), L=16, NS=2)


def pix(t):
    """NCHW -> [pixels, channels] in NHWC order."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ================================================================ lattice generators
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _spiky(g, shape, bg, r0, r1, amp=32):
    """`bg` with rows / columns r0 .. r1 - 1 of image 0 replaced by dense integers in [-amp, amp]: results pass 256 there and only there."""
    t = bg.clone()
    t[0, :, r0:r1, r0:r1] = _ints(g, -amp, amp, (shape[1], r1 - r0, r1 - r0))
    return t


def _mask_pair(g, C, lo, hi):
    """Integer (scale, shift) with scale in {1, 2, -1} and shift = -scale * t, t in [lo, hi]: y * scale + shift == 0 wherever y == t."""
    s = torch.tensor([1.0, 2.0, -1.0], dtype=F64)[torch.randint(0, 3, (C,), generator=g)]
    if not bool((s < 0).any()):
        s[int(torch.randint(0, C, (1,), generator=g))] = -1.0
    return s, -s * _ints(g, lo, hi, (C,))


def _pro_pos(g, C):
    """Prologue coefficients with a POSITIVE shift: relu(0 * scale + shift) > 0, so a prologue applied to the zero padding shows."""
    return torch.tensor([1.0, 2.0, -1.0], dtype=F64)[torch.randint(0, 3, (C,), generator=g)], _ints(g, 1, 2, (C,))


def _pair_terms(x, w, wsc, ps, pb, pro, tag):
    a = act(x, ps, pb, pro)
    y, ysc = F.conv2d(a, w, None, 2, 1), F.conv2d(a, wsc, None, 2, 0)
    cond = {f"{tag} conv(|a|,|w|)": float(F.conv2d(a.abs(), w.abs(), None, 2, 1).max()), f"{tag} conv(|a|,|w_sc|)": float(F.conv2d(a.abs(), wsc.abs(), None, 2, 0).max())}
    for n, v in (("y", y), ("y_sc", ysc)):
        cond[f"{tag} sum|{n}|"], cond[f"{tag} sum {n}^2"] = float(v.abs().sum((0, 2, 3)).max()), float((v * v).sum((0, 2, 3)).max())
    return dict(x=x, w=w, wsc=wsc, ps=ps, pb=pb, y=y, ysc=ysc), cond


def _pair_small(N, pro, rung):
    one_in, xm = RUNGS[rung]
    g = _gen(1000 * N + 7 * PROS.index(pro) + 1)
    x, w, wsc = _ints(g, -xm, xm, (N, 32, 32, 32)), _masked(g, (32, 32, 3, 3), one_in), _masked(g, (32, 32, 1, 1), one_in)
    return _pair_terms(x, w, wsc, *_pro_pos(g, 32), pro, "small")


def _pair_wide(N, pro):
    g = _gen(1000 * N + 7 * PROS.index(pro) + 500001)
    bg = _masked(g, (N, 32, 32, 32), 8)
    x = _spiky(g, bg.shape, bg, 8, 16, 60)
    # sparse weights: under a prologue the background is the shift, a constant per output channel whose square is summed over every pixel
    wsc = _masked(g, (32, 32, 1, 1), 4) * _ints(g, 1, 2, (32, 32, 1, 1))
    return _pair_terms(x, _masked(g, (32, 32, 3, 3), 16), wsc, *_pro_pos(g, 32), pro, "wide")


@functools.lru_cache(maxsize=4)
def pair_lattice(N, pro):
    """(small regime, its rung, wide regime, the exactness conditions' values)."""
    for rung in range(len(RUNGS)):
        small, cond = _pair_small(N, pro, rung)
        if max(cond.values()) <= CAP:
            break
    wide, cw = _pair_wide(N, pro)
    cond.update(cw)
    return small, rung, wide, cond


def _dgrad_lat(N, rung):
    one_in, xm = RUNGS[rung]
    g = _gen(77000 + N)
    bg = _ints(g, -xm, xm, (N, 32, 16, 16))
    dy = _spiky(g, bg.shape, bg, 4, 8)
    w = _masked(g, (32, 32, 3, 3), one_in)
    y = _ints(g, -3, 3, (N, 32, 16, 16))
    s, b = _mask_pair(g, 32, -2, 2)
    dx = conv_g(dy, w, taps=False)
    mask = (y * v4(s) + v4(b)) > 0
    gr, ge = rbf(dx) * mask, dx * mask
    d = dict(dy=dy, w=w, y=y, s=s, b=b, dx=dx, zero_share=float(((y * v4(s) + v4(b)) == 0).double().mean()),
             sums=torch.stack([gr.sum((0, 2, 3)), (gr * y).sum((0, 2, 3))]), sums_exact_dx=torch.stack([ge.sum((0, 2, 3)), (ge * y).sum((0, 2, 3))]))
    cond = {"conv(|dy|,|w|)": float(conv_g(dy.abs(), w.abs(), taps=False).max()), "sum|g|": float(gr.abs().sum((0, 2, 3)).max()),
            "sum|g y|": float((gr * y).abs().sum((0, 2, 3)).max())}
    return d, cond


@functools.lru_cache(maxsize=4)
def dgrad_lattice(N):
    for rung in range(len(RUNGS)):
        d, cond = _dgrad_lat(N, rung)
        if max(cond.values()) <= CAP:
            break
    return d, rung, cond


def _edges_nonzero(t):
    return all(bool((e != 0).any()) for e in (t[:, :, 0], t[:, :, -1], t[:, :, :, 0], t[:, :, :, -1]))


def _stem_lat(N, rung):
    one_in, xm = RUNGS[rung]
    g = _gen(99000 + N)
    bg1, bgs = _ints(g, -xm, xm, (N, 32, 16, 16)), _ints(g, -xm, xm, (N, 32, 16, 16))
    dy1, dys = _spiky(g, bg1.shape, bg1, 4, 8), _spiky(g, bgs.shape, bgs, 4, 8)
    w1, wsc = _masked(g, (32, 32, 3, 3), one_in), _masked(g, (32, 32, 1, 1), one_in)
    y0, x = _ints(g, -3, 3, (N, 32, 32, 32)), _ints(g, -2, 2, (N, 64, 64))
    s, b = _mask_pair(g, 32, -2, 2)
    jc = JC(N)
    gex = main_term(dy1, w1, jc) + second_term(dys, wsc, jc)
    gq = rbf(gex)
    gm = pix(gq * ((y0 * v4(s) + v4(b)) > 0))
    Pm = ST.patches(x)
    d = dict(dy1=dy1, dys=dys, w1=w1, wsc=wsc, y0=y0, x=x, s=s, b=b, g=gq, rounds=int((gq != gex).sum()),
             zero_share=float(((y0 * v4(s) + v4(b)) == 0).double().mean()),
             w=torch.randn(32, 25, generator=g) * 0.2, gamma=torch.rand(32, generator=g) + 0.5, mean=torch.randn(32, generator=g) * 0.3,
             istd=torch.rand(32, generator=g) + 0.5, pre=[torch.randn(32, 25, generator=g), torch.randn(32, generator=g), torch.randn(32, generator=g)])
    cond = {"dgrad(|dy1|,|w1|)+(|dys|,|w_sc|)": float((main_term(dy1.abs(), w1.abs(), jc) + second_term(dys.abs(), wsc.abs(), jc)).max()),
            "sum|gm|": float(gm.abs().sum(0).max()), "sum|gm y0|": float((gm * pix(y0)).abs().sum(0).max()),
            "per-tap sum|gm||patch|": float((gm.abs().t() @ Pm.abs()).max())}
    return d, cond


@functools.lru_cache(maxsize=2)
def stem_lattice(N):
    for rung in range(len(RUNGS)):
        d, cond = _stem_lat(N, rung)
        if max(cond.values()) <= CAP:
            break
    return d, rung, cond


# ================================================================ real-valued generators and float64 references
def _rb(t):
    return t.to(BF).float()


def _span(g, n):
    return torch.exp2(torch.rand(n, generator=g) * 4 - 2).view(1, -1, 1, 1)


def ambiguous(y, s, b):
    """Elements whose float64 pre-activation is within 4u (|y s| + |b|) of zero: the f32 mask could fall on either side."""
    ys = y.double() * v4(s)
    return (ys + v4(b)).abs() <= 4 * U * (ys.abs() + v4(b).abs())


def resample_unambiguous(y, s, b, g):
    """y (bf16 values, NCHW) with every ambiguous element drawn again until none is left."""
    y = y.clone()
    for _ in range(64):
        amb = ambiguous(y, s, b)
        n = int(amb.sum())
        if n == 0:
            return y
        y[amb] = _rb(torch.randn(n, generator=g))
    raise AssertionError("ambiguous elements left after 64 draws")


def prologue_q(x, ps, pb, pro):
    """(bf16 value the kernel stages, bound on the device's difference from it): bf16(max(x ps + pb, lo)) under the midpoint rule."""
    x = x.double()
    if pro == "none":
        return x, torch.zeros_like(x)
    p, m, _ = affine_pre([x * v4(ps), v4(pb).expand_as(x)])
    v, e = relu_e(p, 2 * U * m) if pro == "relu" else (p, 2 * U * m)
    return rbf_e(v, e)


@functools.lru_cache(maxsize=4)
def pair_real(N, pro):
    g = _gen(31000 + 10 * N + PROS.index(pro))
    x = _rb(torch.randn(N, 32, 32, 32, generator=g) * _span(g, 32))
    w, wsc = torch.randn(32, 32, 3, 3, generator=g) / 288 ** 0.5, torch.randn(32, 32, 1, 1, generator=g) / 32 ** 0.5
    ps = (torch.rand(32, generator=g) + 0.5) * (torch.randint(0, 2, (32,), generator=g) * 2 - 1).float()
    pb = torch.randn(32, generator=g) * 0.5
    a, ea = prologue_q(x, ps, pb, pro)
    wq = rbf(wsc.double())
    Y, A = F.conv2d(a, wq, None, 2, 0), F.conv2d(a.abs(), wq.abs(), None, 2, 0)
    E = F.conv2d(ea, wq.abs(), None, 2, 0) + SLOP * 32 * U * A              # one K = 32 slab
    r64 = F.conv2d(act(x.double(), ps.double(), pb.double(), pro), wsc.double(), None, 2, 0)
    return dict(x=x, w=w, wsc=wsc, ps=ps, pb=pb, Y=Y, E=E, r64=r64)


@functools.lru_cache(maxsize=4)
def dgrad_real(N):
    g = _gen(41000 + N)
    dy = _rb(torch.randn(N, 32, 16, 16, generator=g) * _span(g, 32))
    w = torch.randn(32, 32, 3, 3, generator=g) / 288 ** 0.5
    s = (torch.rand(32, generator=g) + 0.5) * (torch.randint(0, 2, (32,), generator=g) * 2 - 1).float()
    b = torch.randn(32, generator=g) * 0.3
    y = resample_unambiguous(_rb(torch.randn(N, 32, 16, 16, generator=g)), s, b, g)
    wq = rbf(w.double())
    T, A = conv_g(dy.double(), wq, taps=False), conv_g(dy.double().abs(), wq.abs(), taps=False)
    return dict(dy=dy, w=w, y=y, s=s, b=b, T=T, E=SLOP * 32 * U * 9 * A, r64=conv_g(dy.double(), w.double(), taps=False))


@functools.lru_cache(maxsize=2)
def stem_real(N):
    """test_stem_ops_f64_gpu.make_bwd_case (x, stem weights, y0, statistics, starting values) + encoder.layer1's dy tensors and weights."""
    c = ST.make_bwd_case(64, N, "bf16")
    g = _gen(51000 + N)
    c["dy1"] = _rb(torch.randn(N, 32, 16, 16, generator=g) * _span(g, 32))
    c["dys"] = _rb(torch.randn(N, 32, 16, 16, generator=g) * _span(g, 32))
    c["w1"], c["wsc"] = torch.randn(32, 32, 3, 3, generator=g) / 72 ** 0.5, torch.randn(32, 32, 1, 1, generator=g) / 32 ** 0.5
    y0 = c["y0"].float().view(N, 32, 32, 32).permute(0, 3, 1, 2)
    c["y0n"] = resample_unambiguous(y0, c["scale"], c["shift"], g)           # NCHW, bf16 values
    jc = JC(N)
    d = lambda t: t.double()
    w1q, wsq = rbf(d(c["w1"])), rbf(d(c["wsc"]))
    c["G"] = main_term(d(c["dy1"]), w1q, jc) + second_term(d(c["dys"]), wsq, jc)
    A = main_term(d(c["dy1"]).abs(), w1q.abs(), jc) + second_term(d(c["dys"]).abs(), wsq.abs(), jc)
    slabs = torch.tensor([[2.0, 2.0], [2.0, 4.0]], dtype=F64).repeat(16, 16)  # MFMA steps of stride phase (h & 1, w & 1)
    c["E"] = SLOP * 32 * U * slabs * A
    c["G64"] = main_term(d(c["dy1"]), d(c["w1"]), jc) + second_term(d(c["dys"]), d(c["wsc"]), jc)
    return c


# ================================================================ CPU self-checks
def test_macros_and_prototypes():
    assert _header_macro("MMVAE_FWD_PAIR_MAX_ROWS") == PAIR_ROWS and _header_macro("MMVAE_DGRAD_BN_SUMS_MAX_ROWS") == DGRAD_ROWS
    assert _header_macro("MMVAE_FWD_PAIR_SCRATCH_BYTES") == PAIR_SCRATCH and _header_macro("MMVAE_DGRAD_BN_SUMS_SCRATCH_BYTES") == DGRAD_SCRATCH
    assert _header_macro("MMVAE_BN_SCRATCH_BYTES") == BN_SCRATCH and _header_macro("MMVAE_CONV_STATS_MAX_ROWS") == FWD_STATS_ROWS
    # the two packs of the DG form sit behind the 768 partial rows of the backward pass
    pack = _header_macro("MMVAE_STEM_DG_PACK_BYTES")
    assert pack >= (32 * 9 * 32 + 32 * 32) * 2 and 1024 * 8 + (1024 + 768) * (64 + 32 * 32) * 4 + pack <= BN_SCRATCH
    assert PAIR_ROWS >= max(conv_geo(N, 512)["gx"] for N in (1, 37, 5120)) and DGRAD_ROWS >= max(conv_geo(N, 768)["gx"] for N in (1, 37, 5120))
    assert _L().lib().mmvae_abi_version() == 3


def test_walks_are_what_the_cases_claim():
    for cap in (512, 768):
        g = conv_geo(1, cap)
        assert (g["nunits"], g["gx"], len(g["idle"])) == (2, 8, 6) and sum(1 for v in g["walk"].values() if not v) == 30
        g = conv_geo(3, cap)
        groups = lambda g: [sorted(u for (b, s), v in g["walk"].items() if b % 8 == q for u in v) for q in range(8)]
        assert g["gx"] == 8 and [len(q) for q in groups(g)] == [1, 1, 1, 1, 1, 1, 0, 0]
        g = conv_geo(5, cap)
        assert g["gx"] == 8 and [len(q) for q in groups(g)] == [2, 2, 2, 2, 2, 0, 0, 0]
        g = conv_geo(37, cap)
        assert (g["nunits"], g["gx"], g["most"], g["idle"]) == (74, 16, 2, [15])     # group 7's second block has no unit: a zero row here too
        assert [len(q) for q in groups(g)] == [10] * 7 + [4]
        for q in range(7):                                                  # two waves of every full group walk a second unit
            assert sorted(len(g["walk"][(b, s)]) for b in (q, q + 8) for s in range(4)) == [1] * 6 + [2] * 2
        assert sorted(u for v in g["walk"].values() for u in v) == list(range(74))
    assert (dg_geo(1)["gx"], dg_geo(3)["gx"], dg_geo(3)["spw"]) == (8, 24, 1)
    assert (dg_geo(96)["gx"], dg_geo(96)["spw"]) == (768, 1)
    g = dg_geo(97)
    assert (g["nslabs"], g["gx"], g["spw"]) == (3104, 768, 2) and g["nslabs"] - 4 * g["gx"] == 32
    assert ST.stem_bwd_geometry(97, 64, "bf16")["gx"] == 776                # mmvae_stem_bwd's grid differs: the sums must not depend on it


def test_exactness_conditions_ladder_and_regimes():
    left, total, worst = [], 0, collections.defaultdict(float)

    def note(cond, rung, what):
        nonlocal total
        assert_exact(cond, what)
        total += 1
        if rung:
            left.append((what, rung))
        for k, v in cond.items():
            worst[k] = max(worst[k], v / CAP)

    both = 0
    for N in CONV_NS:
        for pro in PROS:
            small, rung, wide, cond = pair_lattice(N, pro)
            note(cond, rung, ("pair", N, pro))
            assert bool((rbf(small["y"]) == small["y"]).all())
            big = [bool(((v.abs() > 256) & (rbf(v) != v)).any()) for v in (wide["y"], wide["ysc"])]
            print(f"WIDE pair N={N} {pro}: max |y| {float(wide['y'].abs().max()):.0f}, max |y_sc| {float(wide['ysc'].abs().max()):.0f}, rounding {big}")
            assert all(big), ("wide regime: no |y| or no |y_sc| above 256 that rounds", N, pro)
            both += all(big)
    assert both >= 1, "no wide case in which some |y| and some |y_sc| exceed 256"
    differ = 0
    for N in CONV_NS:
        d, rung, cond = dgrad_lattice(N)
        note(cond, rung, ("dgrad", N))
        assert d["zero_share"] > 0 and bool((d["s"] < 0).any()), N
        assert bool((d["sums"] != d["sums_exact_dx"]).any(1).all()), ("the sums over the rounded and over the exact dx agree in a row", N)
        differ += 1
    assert differ >= 1, "no case whose sums over the rounded and over the exact dx differ in both rows"
    for N in STEM_NS:
        d, rung, cond = stem_lattice(N)
        note(cond, rung, ("stem", N))
        assert d["zero_share"] > 0 and bool((d["s"] < 0).any()) and d["rounds"] > 0, N
        assert _edges_nonzero(d["dy1"]) and _edges_nonzero(d["dys"]), N
    print(f"LADDER {len(left)} of {total} cases left the first rung: {left}; both-tensors-round pair cases {both}, dgrad cases whose sums differ {differ}")
    print("WORST majorants, fractions of the cap:", {k: round(v, 4) for k, v in worst.items()})
    assert len(left) <= 0.10 * total, left


def test_no_ambiguous_mask_element_and_reference_plumbing():
    for N in CONV_NS:
        d = dgrad_real(N)
        assert int(ambiguous(d["y"], d["s"], d["b"]).sum()) == 0
    c = stem_real(3)
    assert int(ambiguous(c["y0n"], c["scale"], c["shift"]).sum()) == 0
    # the data gradient written by phases is autograd's
    N = 2
    g = _gen(5)
    x = torch.zeros(N, 32, 32, 32, dtype=F64, requires_grad=True)
    w1, ws = torch.randn(32, 32, 3, 3, generator=g, dtype=F64), torch.randn(32, 32, 1, 1, generator=g, dtype=F64)
    dy1, dys = torch.randn(N, 32, 16, 16, generator=g, dtype=F64), torch.randn(N, 32, 16, 16, generator=g, dtype=F64)
    ((F.conv2d(x, w1, None, 2, 1) * dy1).sum() + (F.conv2d(x, ws, None, 2, 0) * dys).sum()).backward()
    assert float((main_term(dy1, w1, JC(N)) + second_term(dys, ws, JC(N)) - x.grad).abs().max()) < 1e-12
    x = torch.zeros(N, 32, 16, 16, dtype=F64, requires_grad=True)
    (F.conv2d(x, w1, None, 1, 1) * dy1).sum().backward()
    assert float((conv_g(dy1, w1, taps=False) - x.grad).abs().max()) < 1e-12
    # prologue_q: exact where nothing is near a midpoint, one step where something is
    v, e = prologue_q(torch.tensor([[[[1.0]]]]), torch.tensor([1.0]), torch.tensor([2.0 ** -8]), "affine")
    assert float(v) in (1.0, 1.0 + 2.0 ** -7) and float(e) > 2.0 ** -7


# ================================================================ device side
class Ctx:
    def __init__(self):
        self.L = _L()
        self.lib = self.L.lib()
        self.D = Dev()
        self.n = 0

    def out(self, name, shape, dtype, fill):
        self.n += 1
        return self.D.put(f"{name}{self.n}", (tuple(shape), dtype), fill)

    def f32(self, name, t):
        return None if t is None else self.D.put(name, t.float())


def tail_holds_pattern(t, rows, what):
    assert bool((t[rows:].contiguous().view(torch.uint8) == 0xA5).all()), ("rows past the returned count were written", what, rows)


def run_pair(o, d, N, pro, what, twice=True):
    """Two calls of mmvae_conv2d_fwd_pair on guarded windows: [(y, y_sc, stats, stats_sc, rows)]."""
    D = o.D
    x, w, wsc = D.put("x" + what, nhwc(d["x"], "bf16")), o.f32("w" + what, d["w"]), o.f32("wsc" + what, d["wsc"])
    ps, pb = (None, None) if pro == "none" else (o.f32("ps" + what, d["ps"]), o.f32("pb" + what, d["pb"]))
    sc = D.scratch("scratch" + what, PAIR_SCRATCH)
    res = []
    for rep in range(2 if twice else 1):
        y, ysc = o.out("y", (N, 16, 16, 32), BF, 0xFF), o.out("ysc", (N, 16, 16, 32), BF, 0xFF)
        st, stsc = o.out("stats", (PAIR_ROWS, 2, 32), torch.float32, 0xA5), o.out("stats_sc", (PAIR_ROWS, 2, 32), torch.float32, 0xA5)
        rows = o.L.check(o.lib.mmvae_conv2d_fwd_pair(1, P(x), P(w), P(wsc), P(y), P(ysc), N, 32, 32, 32, 32, P(ps), P(pb), 1 if pro == "relu" else 0,
                                                     P(st), P(stsc), sc, stream()), "conv2d_fwd_pair " + what)
        res.append((y, ysc, st, stsc, rows))
    torch.cuda.synchronize()
    D.check(what)
    geo = conv_geo(N, 512)
    for y, ysc, st, stsc, rows in res:
        assert rows == geo["gx"] and 0 < rows <= PAIR_ROWS, (what, rows, geo["gx"])
        tail_holds_pattern(st, rows, what + " stats"), tail_holds_pattern(stsc, rows, what + " stats_sc")
        assert bool(torch.isfinite(st[:rows]).all()) and bool(torch.isfinite(stsc[:rows]).all()), what
        if geo["idle"]:
            assert bool((st[geo["idle"]] == 0).all()) and bool((stsc[geo["idle"]] == 0).all()), ("a block without work did not write a row of zeros", what)
    if twice:
        assert all(same_bits(a, b) for a, b in zip(res[0][:4], res[1][:4])), ("not bit-reproducible", what)     # (the untouched tails included)
    o.h = dict(x=x, w=w, ps=ps, pb=pb)
    return res[0]


@gpu
@pytest.mark.parametrize("pro", PROS)
@pytest.mark.parametrize("N", CONV_NS)
def test_pair_lattice(N, pro):
    small, _, wide, cond = pair_lattice(N, pro)
    assert_exact(cond, ("pair", N, pro))
    for regime, d in (("small", small), ("wide", wide)):
        what = f"pair N{N} {pro} {regime}"
        y, ysc, st, stsc, rows = run_pair(Ctx(), d, N, pro, what)
        equal_or_explain(nchw64(y), rbf(d["y"]), ("image", "channel", "row", "column"), (what, "y"))
        equal_or_explain(nchw64(ysc), rbf(d["ysc"]), ("image", "channel", "row", "column"), (what, "y_sc"))
        for name, t, v in (("stats", st, d["y"]), ("stats_sc", stsc, d["ysc"])):
            got = t[:rows].cpu().double().sum(0)
            equal_or_explain(got, torch.stack([v.sum((0, 2, 3)), (v * v).sum((0, 2, 3))]), ("sum / sum of squares", "channel"), (what, name, "over", rows, "rows"))


@gpu
@pytest.mark.parametrize("pro", PROS)
@pytest.mark.parametrize("N", CONV_NS)
def test_pair_real(N, pro):
    d = pair_real(N, pro)
    what = f"pair real N{N} {pro}"
    o = Ctx()
    y, ysc, st, stsc, rows = run_pair(o, d, N, pro, what)
    # bit contract: mmvae_conv2d_fwd on the same input (the same MFMA sequence without the shortcut's)
    D = o.D
    x, w, ps, pb = (o.h[k] for k in ("x", "w", "ps", "pb"))
    y1, st1 = o.out("y_fwd", (N, 16, 16, 32), BF, 0xFF), o.out("stats_fwd", (FWD_STATS_ROWS, 2, 32), torch.float32, 0xA5)
    sc1 = D.scratch("scratch_fwd", 2 * 32 * 32 * 9 * 2 + 64)
    rows1 = o.L.check(o.lib.mmvae_conv2d_fwd(1, 0, P(x), P(w), P(y1), N, 32, 32, 32, 32, 3, 2, 1, P(ps), P(pb), 1 if pro == "relu" else 0, P(st1), sc1, stream()),
                      "conv2d_fwd " + what)
    torch.cuda.synchronize()
    D.check(what)
    assert rows1 == rows and same_bits(y, y1) and same_bits(st[:rows], st1[:rows]), ("the pair's y / rows / stats are not mmvae_conv2d_fwd's", what, rows, rows1)
    # y_sc: float64 reference, the slab rule + half a bf16 ulp
    Y, E = d["Y"], d["E"]
    got = nchw64(ysc)
    assert bool(torch.isfinite(got).all()), what
    bound = E + half_ulp_bf16(Y.abs() + E)
    gate(f"pair_ysc_{pro}", plane_slices(_ratio((got - Y).abs(), bound)), what, lambda: (rbf(Y) - d["r64"]).abs())
    print(f"STORAGE {what}: max |Rq - R64| of y_sc {float((rbf(Y) - d['r64']).abs().max()):.3e}")
    # stats_sc: sums of the f32 accumulators; order-free majorant of the summation
    depth = conv_geo(N, 512)["depth"]
    sums = stsc[:rows].cpu().double().sum(0)
    ref = torch.stack([Y.sum((0, 2, 3)), (Y * Y).sum((0, 2, 3))])
    bnd = torch.stack([E.sum((0, 2, 3)) + SLOP * U * depth * Y.abs().sum((0, 2, 3)),
                       (2 * Y.abs() * E + E * E).sum((0, 2, 3)) + SLOP * U * (depth + 1) * (Y * Y).sum((0, 2, 3))])
    gate(f"pair_stats_sc_{pro}", _ratio((sums - ref).abs(), bnd), what)


def run_dgrad(o, d, N, what):
    D = o.D
    dy, w, y = D.put("dy", nhwc(d["dy"], "bf16")), o.f32("w", d["w"]), D.put("y_pre", nhwc(d["y"], "bf16"))
    s, b = o.f32("bn_scale", d["s"]), o.f32("bn_shift", d["b"])
    sc = D.scratch("scratch", DGRAD_SCRATCH)
    res = []
    for rep in range(2):
        dx, sums = o.out("dx", (N, 16, 16, 32), BF, 0xFF), o.out("sums", (DGRAD_ROWS, 2, 32), torch.float32, 0xA5)
        rows = o.L.check(o.lib.mmvae_conv2d_dgrad_bn_sums(1, P(dy), P(w), P(dx), P(y), P(s), P(b), P(sums), N, 16, sc, stream()), "conv2d_dgrad_bn_sums " + what)
        res.append((dx, sums, rows))
    torch.cuda.synchronize()
    D.check(what)
    geo = conv_geo(N, 768)
    for dx, sums, rows in res:
        assert rows == geo["gx"] and 0 < rows <= DGRAD_ROWS, (what, rows, geo["gx"])
        tail_holds_pattern(sums, rows, what)
        assert bool(torch.isfinite(sums[:rows]).all()), what
        if geo["idle"]:
            assert bool((sums[geo["idle"]] == 0).all()), ("a block without work did not write a row of zeros", what)
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1][:res[0][2]], res[1][1][:res[0][2]]), ("not bit-reproducible", what)
    return res[0] + (dy, w)


@gpu
@pytest.mark.parametrize("N", CONV_NS)
def test_dgrad_bn_sums_lattice(N):
    d, _, cond = dgrad_lattice(N)
    what = f"dgrad lattice N{N}"
    assert_exact(cond, what)
    dx, sums, rows, _, _ = run_dgrad(Ctx(), d, N, what)
    equal_or_explain(nchw64(dx), rbf(d["dx"]), ("image", "channel", "row", "column"), (what, "dx"))
    equal_or_explain(sums[:rows].cpu().double().sum(0), d["sums"], ("sum g / sum g y", "channel"), (what, "sums over", rows, "rows; g = the rounded dx under the mask"))


@gpu
@pytest.mark.parametrize("N", CONV_NS)
def test_dgrad_bn_sums_real(N):
    d = dgrad_real(N)
    what = f"dgrad real N{N}"
    assert int(ambiguous(d["y"], d["s"], d["b"]).sum()) == 0
    o = Ctx()
    dx, sums, rows, dy, w = run_dgrad(o, d, N, what)
    dx1 = o.out("dx_dgrad", (N, 16, 16, 32), BF, 0xFF)
    sc1 = o.D.scratch("scratch_dgrad", 2 * 32 * 32 * 9 * 2 + 64)
    o.L.check(o.lib.mmvae_conv2d_dgrad(1, 0, P(dy), P(w), P(dx1), N, 16, 16, 32, 32, 3, 1, 1, sc1, stream()), "conv2d_dgrad " + what)
    torch.cuda.synchronize()
    o.D.check(what)
    assert same_bits(dx, dx1), ("dx is not mmvae_conv2d_dgrad's", what)
    got = nchw64(dx)
    assert bool(torch.isfinite(got).all()), what
    T, E = d["T"], d["E"]
    gate("dgrad_dx", plane_slices(_ratio((got - T).abs(), E + half_ulp_bf16(T.abs() + E))), what, lambda: (rbf(T) - d["r64"]).abs())
    # the sums of the device's own dx under the float64 mask (no element is ambiguous)
    y = d["y"].double()
    g = got * ((y * v4(d["s"]) + v4(d["b"])) > 0)
    depth = conv_geo(N, 768)["depth"]
    ref = torch.stack([g.sum((0, 2, 3)), (g * y).sum((0, 2, 3))])
    bnd = SLOP * U * torch.stack([depth * g.abs().sum((0, 2, 3)), (depth + 1) * (g * y).abs().sum((0, 2, 3))])
    gate("dgrad_sums", _ratio((sums[:rows].cpu().double().sum(0) - ref).abs(), bnd), what)


def run_stem(o, c, N, g_host, y0_nchw, scale, shift, what):
    """mmvae_stem_bwd_dg twice and, where g_host is given, mmvae_stem_bwd on it once: [(dweight, dgamma, dbeta)] -- from the same starting values."""
    D = o.D
    dy1, dys = D.put("dy1", nhwc(c["dy1"], "bf16")), D.put("dys", nhwc(c["dys"], "bf16"))
    w1, wsc = o.f32("w1", c["w1"]), o.f32("wsc", c["wsc"])
    y0, x = D.put("y0", nhwc(y0_nchw, "bf16")), D.put("x", c["x"].to(BF))
    w, gamma, mean, istd = (o.f32(k, c[k]) for k in ("w", "gamma", "mean", "istd"))
    s, b = o.f32("bn_scale", scale), o.f32("bn_shift", shift)
    sc = D.scratch("scratch", BN_SCRATCH)
    res = []
    for rep in range(3 if g_host is not None else 2):
        dw, dg, db = o.f32(f"dweight{rep}", c["pre"][0]), o.f32(f"dgamma{rep}", c["pre"][1]), o.f32(f"dbeta{rep}", c["pre"][2])
        if rep < 2:
            o.L.check(o.lib.mmvae_stem_bwd_dg(1, P(dy1), P(dys), P(w1), P(wsc), P(y0), P(x), P(w), P(gamma), P(s), P(b), P(mean), P(istd), P(dw), P(dg), P(db),
                                              N, 64, sc, stream()), "stem_bwd_dg " + what)
        else:
            gd = D.put("g", nhwc(g_host, "bf16"))
            sc2 = D.scratch("scratch_stem_bwd", BN_SCRATCH)
            o.L.check(o.lib.mmvae_stem_bwd(1, P(gd), P(y0), P(x), P(w), P(gamma), P(s), P(b), P(mean), P(istd), P(dw), P(dg), P(db), N, 64, sc2, stream()),
                      "stem_bwd " + what)
        res.append((dw, dg, db))
    torch.cuda.synchronize()
    D.check(what)
    assert all(same_bits(a, b_) for a, b_ in zip(res[0], res[1])), ("not bit-reproducible", what)
    assert all(bool(torch.isfinite(t).all()) for t in res[0]), what
    return res


@gpu
@pytest.mark.parametrize("N", STEM_NS)
def test_stem_dg_lattice(N):
    d, _, cond = stem_lattice(N)
    what = f"stem lattice N{N}"
    assert_exact(cond, what)
    assert _edges_nonzero(d["dy1"]) and _edges_nonzero(d["dys"])
    res = run_stem(Ctx(), d, N, d["g"], d["y0"], d["s"], d["b"], what)
    for name, a, b in zip(("dweight", "dgamma", "dbeta"), res[0], res[2]):
        got, want = a.double().cpu(), b.double().cpu()
        assert same_bits(a, b), (what, name, "mmvae_stem_bwd_dg differs from mmvae_stem_bwd fed g = rbf(exact data gradient)",
                                 f"{int((got != want).sum())} of {got.numel()} differ, largest difference {float((got - want).abs().max())}")
        assert not torch.equal(got, d["pre"][("dweight", "dgamma", "dbeta").index(name)].double()), (what, name, "unchanged")
    # Absolute, on the host: the two routes share the mask line, so the comparison above cannot see `>=` for `>`.  The sums are exact integers:
    # dbeta = pre + (float)S0 is ONE f32 addition of two known numbers (bits); dgamma and dweight are the finalize formula in double (a few
    # double roundings: 2^-46 of the term magnitudes) and the same single f32 addition (u of the term and of the result).
    dd = lambda t: t.double()
    r = ST.ref_stem_bwd_rq(pix(d["g"]), pix(d["y0"]), ST.patches(d["x"]), dd(d["w"]), dd(d["gamma"]), d["s"], d["b"], dd(d["mean"]), dd(d["istd"]))
    want_db = d["pre"][2].float() + r["S0"].float()
    equal_or_explain(res[0][2].cpu().double(), want_db.double(), ("channel",), (what, "dbeta = pre + sum gm, the mask strict"))
    istd, mean = dd(d["istd"]), dd(d["mean"])
    mag_g = istd * (r["S1"].abs() + (mean * r["S0"]).abs())
    mag_w = r["A"].abs()[:, None] * (r["W1"].abs() + (r["m2"] * istd).abs()[:, None] * (r["W2"].abs() + (mean[:, None] * r["W3"]).abs()) + r["m1"].abs()[:, None] * r["W3"].abs())
    for name, k, got, pre, mag in (("dweight", "dW", res[0][0], d["pre"][0], mag_w), ("dgamma", "dgamma", res[0][1], d["pre"][1], mag_g)):
        ref = dd(pre) + r[k]
        bound = SLOP * U * (r[k].abs() + ref.abs()) + 2.0 ** -46 * mag
        gate(f"stemdg_lattice_{name}", _ratio((got.cpu().double() - ref).abs(), bound), what)


@gpu
@pytest.mark.parametrize("N", STEM_NS)
def test_stem_dg_real(N):
    c = stem_real(N)
    what = f"stem real N{N}"
    assert int(ambiguous(c["y0n"], c["scale"], c["shift"]).sum()) == 0
    res = run_stem(Ctx(), c, N, None, c["y0n"], c["scale"], c["shift"], what)
    cu, d = (lambda t: t.cuda()), (lambda t: t.double())
    gq, eflag = rbf_e(c["G"], c["E"])
    e = torch.where(eflag > 0, _spacing(c["G"].abs() + c["E"]), torch.zeros_like(eflag))     # one bf16 step where a midpoint is within the slab bound
    g2, y0, e2 = cu(pix(gq)), cu(pix(d(c["y0n"]))), cu(pix(e))
    Pm = cu(ST.patches(d(c["x"])))
    w, gamma, scale, shift, mean, istd = (cu(d(c[k])) for k in ("w", "gamma", "scale", "shift", "mean", "istd"))
    r = ST.ref_stem_bwd_rq(g2, y0, Pm, w, gamma, scale, shift, mean, istd)
    assert int(r["amb"].sum()) == 0
    pre = [cu(d(t)) for t in c["pre"]]
    bW, bG, bB = ST.stem_bwd_bounds(r, g2, y0, Pm, w, mean, istd, pre[0], pre[1], pre[2], dg_geo(N), "bf16")
    # first order in g's own uncertainty: dbeta = sum gm; dgamma = istd sum gm (y0 - mean); dW = A (W1 - m2 istd (W2 - mean W3) - m1 W3)
    n = y0.shape[0]
    em = e2 * ((y0 * scale + shift) > 0)
    eS0, eS1 = em.sum(0), (em * (y0 - mean).abs()).sum(0)
    bB = bB + SLOP * eS0
    bG = bG + SLOP * istd * eS1
    bW = bW + SLOP * r["A"].abs()[:, None] * (em.t() @ Pm.abs() + (istd * istd * eS1 / n)[:, None] * (r["W2"] - mean[:, None] * r["W3"]).abs()
                                              + (eS0 / n)[:, None] * r["W3"].abs()[None, :])
    r64 = ST.ref_stem_bwd_r64(cu(pix(c["G64"])), y0, Pm, gamma, scale, shift, mean, istd)
    for name, k, got, p, bnd in (("dweight", "dW", res[0][0], pre[0], bW), ("dgamma", "dgamma", res[0][1], pre[1], bG), ("dbeta", "dbeta", res[0][2], pre[2], bB)):
        print(f"STORAGE {what}: max |Rq - R64| of {name} {float((r[k] - r64[k]).abs().max()):.3e}; elements of g near a midpoint {int((e > 0).sum())}")
        gate(f"stemdg_{name}", _ratio((got.double() - (p + r[k])).abs(), bnd).cpu(), what, lambda k=k: (r[k] - r64[k]).abs())


# ================================================================ refusals
def refusal_calls(lib, b, st=None):
    """name -> return code of every refused call on `b` = dict of pointers; each must be refused before anything is enqueued."""
    pair = lambda dt=1, H=32, C=32, N=1, wsc=b["w2"]: lib.mmvae_conv2d_fwd_pair(dt, b["x"], b["w"], wsc, b["y"], b["y2"], N, H, H, C, C, None, None, 0, b["st"], b["st2"],
                                                                              b["sc"], st)
    dg = lambda dt=1, H=16, N=1, y=b["x2"], sums=b["st"]: lib.mmvae_conv2d_dgrad_bn_sums(dt, b["x"], b["w"], b["y"], y, b["v"], b["v"], sums, N, H, b["sc"], st)
    stem = lambda dt=1, S=64, N=1, wsc=b["w2"]: lib.mmvae_stem_bwd_dg(dt, b["x"], b["x2"], b["w"], wsc, b["y"], b["y2"], b["w3"], b["v"], b["v"], b["v"], b["v"], b["v"],
                                                                      b["dw"], b["dg"], b["db"], N, S, b["sc"], st)
    U_, A_ = ERR_UNSUPPORTED, ERR_ARG
    return {"pair f32": (pair(dt=0), U_), "dgrad f32": (dg(dt=0), U_), "stem f32": (stem(dt=0), U_),
            "dgrad H = 32": (dg(H=32), U_), "stem S = 32": (stem(S=32), U_), "pair on 16x16 maps": (pair(H=16), U_), "pair 64 channels": (pair(C=64), U_),
            "dgrad y_pre NULL": (dg(y=None), A_), "dgrad sums NULL": (dg(sums=None), A_), "pair weight_sc NULL": (pair(wsc=None), A_),
            "stem weight_sc NULL": (stem(wsc=None), A_), "pair N = 0": (pair(N=0), A_), "dgrad N = 0": (dg(N=0), A_), "stem N = 0": (stem(N=0), A_),
            "pair dtype 7": (pair(dt=7), A_), "dgrad dtype 7": (dg(dt=7), A_), "stem dtype 7": (stem(dt=7), A_)}


REFUSAL_BUFS = ("x", "x2", "w", "w2", "w3", "y", "y2", "st", "st2", "v", "dw", "dg", "db", "sc")


def test_refusals_need_no_device(pkg):
    """Every refusal returns before anything is enqueued: where there is no device, host buffers stand in for the device ones and stay as
    they are.  Where there is one, the guarded device variant below is the test and this one leaves the calls to it."""
    if torch.cuda.is_available():
        return test_refusals_leave_everything_untouched()
    lib = _L().lib()
    host = {n: (ctypes.c_uint8 * 64)(*([0xA5] * 64)) for n in REFUSAL_BUFS}
    got = refusal_calls(lib, {n: ctypes.addressof(v) for n, v in host.items()})
    assert all(rc == want for rc, want in got.values()), got
    assert lib.mmvae_last_error()
    assert all(bytes(v) == b"\xa5" * 64 for v in host.values())


@gpu
def test_refusals_leave_everything_untouched():
    lib = _L().lib()
    D = Dev()
    bufs = {n: D.scratch(n, BN_SCRATCH if n == "sc" else 1 << 20) for n in REFUSAL_BUFS}
    got = refusal_calls(lib, bufs, stream())
    torch.cuda.synchronize()
    assert all(rc == want for rc, want in got.values()), got
    wrote = [n for n, a in D.arenas.items() if not a.untouched()]
    assert not wrote, ("a refused call wrote", wrote)


# ================================================================ census (keep last)
# Launcher families per entry point, packing launches left out.  Filled from the code (capi.cpp, conv_fstream.hip, stem_bwd.hip).
LAUNCHES = {"pair": ("conv3_stream",), "dgrad": ("conv3_stream_bwd",), "stem": ("stem_gram", "stem_gram_sum", "stem_bwd_dg", "stem_bwd_finalize"), "refusals": ()}
PACKS = {"pair": 2, "dgrad": 1, "stem": 5, "refusals": 0}                    # [cout][tap][cin] + [32][32]; the flipped taps; four stride phases + the shortcut


def census_plan():
    return [("pair", N) for N in (1, 37)] + [("dgrad", N) for N in (1, 37)] + [("stem", N) for N in (1, 3)] + [("refusals", 0)]


def census_child():
    lib = _L().lib()
    a, b = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    v, done = z(32), []
    for op, N in census_plan():
        assert lib.mmvae_convert(0, 0, P(a), P(b), 8, stream()) == 0
        if op == "pair":
            rc = lib.mmvae_conv2d_fwd_pair(1, P(z((N, 32, 32, 32), BF)), P(z((32, 32, 3, 3))), P(z((32, 32, 1, 1))), P(z((N, 16, 16, 32), BF)), P(z((N, 16, 16, 32), BF)),
                                           N, 32, 32, 32, 32, P(v), P(v), 1, P(z((PAIR_ROWS, 2, 32))), P(z((PAIR_ROWS, 2, 32))), P(z(PAIR_SCRATCH, torch.uint8)), stream())
        elif op == "dgrad":
            rc = lib.mmvae_conv2d_dgrad_bn_sums(1, P(z((N, 16, 16, 32), BF)), P(z((32, 32, 3, 3))), P(z((N, 16, 16, 32), BF)), P(z((N, 16, 16, 32), BF)), P(v), P(v),
                                                P(z((DGRAD_ROWS, 2, 32))), N, 16, P(z(DGRAD_SCRATCH, torch.uint8)), stream())
        elif op == "stem":
            rc = lib.mmvae_stem_bwd_dg(1, P(z((N, 16, 16, 32), BF)), P(z((N, 16, 16, 32), BF)), P(z((32, 32, 3, 3))), P(z((32, 32, 1, 1))), P(z((N, 32, 32, 32), BF)),
                                       P(z((N, 64, 64), BF)), P(z((32, 25))), P(v), P(v), P(v), P(v), P(v), P(z((32, 25))), P(z(32)), P(z(32)), N, 64,
                                       P(z(BN_SCRATCH, torch.uint8)), stream())
        else:
            big = lambda: z(1 << 18).data_ptr()
            rcs = refusal_calls(lib, {n: (z(BN_SCRATCH, torch.uint8).data_ptr() if n == "sc" else big()) for n in REFUSAL_BUFS}, stream())
            rc = max(r for r, _ in rcs.values())
        torch.cuda.synchronize()
        done.append([op, N, rc])
    print("CENSUS_PLAN " + json.dumps(done))


@gpu
def test_launch_census(tmp_path):
    prefix = str(tmp_path / "census")
    env = dict(os.environ, MMVAE_LAUNCH_STATS=prefix, MMVAE_LAUNCH_SEQ="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--census-child"], capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    done = json.loads(re.search(r"^CENSUS_PLAN (.*)$", r.stdout, re.M).group(1))
    seqs = [f for f in os.listdir(tmp_path) if f.endswith(".seq")]
    assert len(seqs) == 1, seqs
    names = [ln.split()[0] for ln in open(tmp_path / seqs[0]) if ln.strip()]
    segs, cur = [], None
    for n in names:
        if n == "convert":
            cur = []
            segs.append(cur)
        else:
            assert cur is not None, names[:4]
            cur.append(n)
    assert len(segs) == len(done), (len(segs), len(done))
    wrong, seen = [], set()
    for (op, N, rc), seg in zip(done, segs):
        print(f"CENSUS {op} N={N} rc={rc}: {' '.join(seg)}")
        packs = [n for n in seg if n in ("pack", "pack_multi")]
        rest = tuple(n for n in seg if n not in ("pack", "pack_multi"))
        if rest != LAUNCHES[op] or len(packs) != PACKS[op] or (rc < 0) != (op == "refusals"):
            wrong.append((op, N, rc, seg))
        seen.update(rest)
    assert not wrong, wrong
    assert seen == {f for v in LAUNCHES.values() for f in v}, seen


if __name__ == "__main__":
    if sys.argv[1:] == ["--census-child"]:
        census_child()
    else:
        for fn in (test_macros_and_prototypes, test_walks_are_what_the_cases_claim, test_exactness_conditions_ladder_and_regimes,
                   test_no_ambiguous_mask_element_and_reference_plumbing):
            fn()
            print("ok", fn.__name__)
