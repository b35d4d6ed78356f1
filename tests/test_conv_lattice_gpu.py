"""Bit equality of the generic convolution entry points on integer-lattice inputs, through the C ABI: mmvae_conv2d_fwd (y, the returned row
count, the statistics rows), mmvae_conv2d_wgrad, mmvae_conv2d_wgrad_pair and mmvae_convT_bwd_fused (dw, dx, dw2).

Why bits: every operand is a small integer, so every product is an integer, exact in bf16 and in f32, and an f32 sum of integers whose
absolute sum stays below 2^24 is exact under any order.  A convolution, a statistics row or a weight gradient whose terms have an absolute
sum below the cap has ONE possible f32 result -- whatever the tap order, K-slab order, the split across waves, blocks or partial images and
the tree of wgrad_reduce_kernel -- and the device must give the float64 reference bit for bit.  A missing, doubled or misplaced term (a wrong
tap or padding rule, a prologue applied to the zero padding, a partial image left unwritten, `dW =` for `dW +=`) changes it; there is no
tolerance.  The cap used is 2^23: one bit is left for the MFMA's internal accumulation, which nobody has measured to be exact right up to
2^24.  Loss of precision is what this file cannot see; tests/test_conv_wgrad_f64_gpu.py gates the weight gradients on real-valued data.

Cases: test_ops_gpu.CONFIGS (imported, so the two lists stay in step) in {f32, bf16} x {no prologue, prologue with ReLU, affine-only
prologue}; N = 1 on every stream shape (wstream_kind 1 - 4, conv3_stream at both strides, convT4_stream at both sizes: 1 - 2 work units for
32 wave slots); N in {1, 37, 70} on the position-major weight-gradient shapes (ragged last image chunk, one split, two splits); non-square
maps; channel counts off the network that reach the fallback families (wgrad_kernel, gather_gemm_kernel, gather3_kernel); the pair and the
fused entry points on the shapes of their tests in test_ops_gpu.py with N in {1, 5, 37}.

Inputs, seeded per case.  Small regime: x, dy integers in [-2, 2]; weights +-1 under a mask of density 1/4; prologue scale from {1, 2, -1}
(a negative scale meets the ReLU), shift an integer in [-1, 2]; dw_old integers in +-[1, 4] (never zero: `=` for `+=` shows on every
element); x2, w2, dy_sc by the same rules.  Where a case misses a condition below, its generator goes down a fixed ladder: density 1/8,
1/16, then x in [-1, 1] (asserted: at most 10 % of the cases leave the first rung).  In this regime no y rounds: the largest |y| over all
cases is 180, every y is a bf16 number, so it cannot tell the accumulator from the stored value.  Wide regime (forward y and the fused dx
only): dense integers in [-3, 3] on both sides; on the channel-heavy layers |y| passes 256 by far, so a bf16 store really rounds -- y must
be the round-to-nearest-even bf16 of the exact integer -- and the statistics are gated here as well wherever sum |y| and sum y^2 of the case
meet the cap (the deep layers on small maps: 256 -> 256 on 2x2 has 473 rounded elements at 0.38 of the cap).  Rounding regime (forward, the
cases with at most 1024 output pixels per channel, statistics gated): dense integers of the largest amplitude of 12, 8, 6, 4 at which every
condition holds, so that |y| passes 256 on the thin layers too (16 channels, 1x1 kernels).  The first test asserts that every forward
family (gather_gemm, gather3, patch_conv, deep2_conv, pos_conv, conv3_stream, convT4_stream) has at least one statistics-gated bf16 case
whose y rounds and whose sums over the rounded y differ from the exact ones in both rows: a kernel that took its statistics from the stored
y instead of the f32 accumulators fails there.

Exactness conditions, from the float64 reference of absolute values, each <= 2^23, asserted on the CPU for every case (first test) and again
by each GPU test before it trusts bit equality: conv(|a|, |w|) per output element; sum |y| and sum y^2 per channel over the whole tensor
(wherever the statistics are gated); |dw_old| + sum |a| |dy| per weight element; likewise dx, dw2 and the pair's second image.

Asserted per case: every device buffer is a window of its documented size in a pattern-filled arena and the guards are intact; y and dx
start as 0xFF bytes (NaN in both storage types); the weight-gradient scratch is MMVAE_WGRAD_SCRATCH_BYTES of 0xFF bytes (a partial image
left unwritten is then a NaN in dw, not a lucky zero).  Forward: bits of y (bf16: rbf of the exact integer); 0 < rows <=
MMVAE_CONV_STATS_MAX_ROWS; per channel the float64 host sum of the first `rows` rows of sum and of sum of squares equals the reference exactly
(the sums come from the f32 accumulators, as mmvae.h says: the gated wide and rounding regimes are where that shows); rows past `rows` still hold the fill pattern; a second call with weight = NULL on the same scratch gives the same bits.  Weight
gradients: dw == dw_old + R64 exactly; a second run from the same dw_old gives the same bits.  Pair and fused: the same for both weight images
and dx.  Refusals (k = 7, channel counts off the vector width, the fused entry point on 8x8 maps, the pair off its shape, dtype 7, and the
fallback weight gradient whose image is no multiple of 256 elements): a negative code, every output and scratch byte untouched, and (census)
nothing enqueued, not even the packing launch.

What guards the out-of-range lanes of the shapes that had never run (non-square maps, off-network channel counts), read before their first
device run:
  * every stream and position-major kernel requires a square map in its dispatcher (conv3_stream_ok / convT4_stream_ok: Hin == Win;
    wstream_kind: Hp == Wp; try_wgrad_pos: Hp == Wp and Hg == Wg; try_pos: Hi == Wi and Ho == Wo), so none of them takes a non-square map;
  * gather_gemm_kernel and gather3_kernel decode (n, hq, wq) from P.Hq / P.Wq and test every tap against a.Hi and a.Wi separately; pixels
    past M load nothing (gather3: offset 0, result discarded) and store nothing; weight rows past Cout are zero-filled, stores need co < Cout
    (4 channels at a time, Cout % 4 == 0 is a dispatcher condition);
  * patch_conv_kernel reads x through a buffer resource of exactly x_bytes (out of range reads as zero), its staging slots test wi against
    g.Wi statically and the row against g.Hi per tile; LDS writes need pp < npatch; the general epilogue stores need hq < P.Hq, wq < P.Wq,
    n < N and co < Cout, the uniform one hq < g.Hq (whole rows of a power-of-two width);
  * deep2_conv_kernel stages whole images (p < nvalid) and resolves taps through a table built from a.Hi and a.Wi separately;
  * wgrad_kernel (the fallback): P loads need m < m_end and a0 + ch < Ca, G loads hg in [0, Hg), wg in [0, Wg) and b0 + ch < Cb (channel
    counts are multiples of the vector, a dispatcher condition); the partial image is written under aa < Ca, bb < Cb_valid and the launcher
    caps the number of parts by the scratch;
  * wgrad2_kernel (make_tile_geom with Hq, Wq, Hi, Wi separate): G loads need the static column test against g.Wi and the per-tile row test
    against g.Hi (whole-image tiles: n < N), P loads pix < nv_c.
Reading found no form that indexes out of range, so no dispatcher refusal was added for them; all of them are computed, none refused.
The one refusal among the new shapes is the f32 4 -> 16 3x3 weight gradient (576 elements: launch_wgrad_reduce takes multiples of 256),
which used to arrive AFTER wgrad_kernel had been enqueued and now comes first.

Census (last test): one child process with MMVAE_LAUNCH_STATS / MMVAE_LAUNCH_SEQ runs every case and entry point once, an 8-element
mmvae_convert between them, and the launcher families of every segment must be LAUNCHES'.  Families seen, each at least once: wgrad_stream,
wgrad_pos, wgrad2, wgrad, wgrad_reduce, gather_gemm, gather3, patch_conv, deep2_conv, pos_conv, conv3_stream, convT4_stream -- every family
is reached through these entry points at a small shape.  The refusals run in the same child and their segment must be empty.
LAUNCHES was filled from the dispatch code and the first device run corrected 20 of its 78 rows:
  * f32 weight gradients of the 1x1 stride-2 layers (32 -> 32 on 16x16, 7x7 and 16x8, 32 -> 64 and 64 -> 128 on 8x8, 128 -> 256 on 4x4) and
    of 128 -> 128 k4 s2 ConvT on 2x2: wgrad (the fallback), not wgrad2 -- try_wgrad2 declines them at its LDS / staging-slot fit, which
    the hand evaluation left out (the k-split form cannot shrink its 128-pixel tile).  So the fallback kernel IS reached by network shapes, in f32;
  * bf16 forward of 64 -> 128 3x3 s2 on 8x8 (every N), 64 -> 128 1x1 s2 on 8x8, 64 -> 64 3x3 on 5x5 and 32 -> 128 k2 s2 ConvT on 1x1:
    deep2_conv, not pos_conv (launch_pos_conv has no instantiation of these geometries);
  * forward of bf16 32 -> 32 3x3 s2 on 7x7 and of f32 32 -> 32 3x3 s1 on 16x16 (N 1 and 5) and on 32x16: gather_gemm, not patch_conv (weights
    + patch exceed the patch-tile kernel's LDS; on 16x32 the f32 form does fit).

Measured on the MI355X: every case bit-exact at the first run, in both storage types and all three prologue forms, the non-square and the
off-network shapes included; no exact sum came back inexact on any MFMA form at the 2^23 cap (largest majorants: 0.95 of the cap for sum y^2,
0.13 for sum |y|, 0.066 for a weight-gradient element, 5.7e3 for a wide-regime accumulator), the statistics of the gated wide and rounding regimes included.  This file and
test_conv_wgrad_f64_gpu.py together: 584 GPU tests in 19.7 s (0.03 s a test; this file's census child 2.4 s of it, the slowest case 0.9 s: 16 -> 16 ConvT on 32x32, N = 70); the CPU
self-checks in 12 s (the float64 references of all 234 case x prologue combinations).
"""
import collections
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

from test_ops_gpu import CONFIGS  # noqa: E402
from test_upblock_ops_f64_gpu import DTI, F64, TDT, Arena, Dev, P, _header_macro, _L, gpu, rbf, same_bits, stream  # noqa: E402

CAP = float(1 << 23)
PROS = ("none", "relu", "affine")
DTS = ("bf16", "f32")
WSCRATCH_BYTES = 64 << 20                                                   # MMVAE_WGRAD_SCRATCH_BYTES (checked against the header below)
STATS_ROWS = 4096                                                           # MMVAE_CONV_STATS_MAX_ROWS

Case = collections.namedtuple("Case", "group Cin Cout k s p tr H W N dts")


def _cases():
    out = [Case("net", ci, co, k, s, p, tr, H, H, N, DTS) for ci, co, k, s, p, tr, H, N in CONFIGS]
    sq = lambda grp, ci, co, k, s, p, tr, H, N, dts=DTS: Case(grp, ci, co, k, s, p, tr, H, H, N, dts)
    # N = 1 on each stream shape: weight-gradient stream kinds 1 - 4 (kind 1 at 16 channels is CONFIGS' 16x16x4x2x1x1x32x1), conv3_stream at
    # both strides (the same two shapes as kinds 3 and 4), convT4_stream at both sizes
    out += [sq("one", 32, 16, 4, 2, 1, 1, 32, 1), sq("one", 16, 16, 4, 2, 1, 1, 16, 1), sq("one", 32, 16, 4, 2, 1, 1, 16, 1),
            sq("one", 32, 32, 3, 1, 1, 0, 16, 1), sq("one", 32, 32, 3, 2, 1, 0, 32, 1)]
    # position-major weight gradients: KI = 32 on 64x64 tiles, the 64x32-tile form, the banded form; ragged chunk, one split, two splits
    for N in (1, 37, 70):
        out += [sq("pos", 256, 256, 3, 1, 1, 0, 2, N), sq("pos", 128, 64, 4, 2, 1, 1, 4, N), sq("pos", 64, 128, 3, 2, 1, 0, 8, N)]
    ns = lambda ci, co, k, s, p, tr, H, W, N: Case("nonsq", ci, co, k, s, p, tr, H, W, N, DTS)
    out += [ns(32, 32, 3, 1, 1, 0, 16, 32, 3), ns(32, 32, 3, 1, 1, 0, 32, 16, 3), ns(16, 16, 4, 2, 1, 1, 32, 16, 3), ns(64, 64, 3, 1, 1, 0, 8, 4, 5),
            ns(128, 128, 3, 1, 1, 0, 4, 2, 9), ns(32, 32, 1, 2, 0, 0, 16, 8, 3)]
    out += [sq("off", 48, 48, 3, 1, 1, 0, 8, 5), sq("off", 96, 32, 1, 1, 0, 0, 8, 5), sq("off", 8, 32, 3, 1, 1, 0, 8, 5, ("bf16",)),
            sq("off", 4, 16, 3, 1, 1, 0, 8, 5, ("f32",)), sq("off", 32, 8, 4, 2, 1, 1, 8, 5)]
    return out


CASES = _cases()
# the fallback weight gradient of this case is refused (its image is no multiple of 256 elements), before anything is enqueued
WGRAD_REFUSED = {("off-4x16k3s1-8x8-N5", "f32")}
PAIR_NS = (1, 5, 37)
FUSED = [(C, H, N, second) for C, H in ((16, 32), (16, 16), (32, 16), (32, 32)) for N in (1, 5, 37) for second in (False, True)]


def case_id(c):
    return f"{c.group}-{c.Cin}x{c.Cout}k{c.k}s{c.s}{'T' if c.tr else ''}-{c.H}x{c.W}-N{c.N}"


def out_hw(c):
    f = (lambda h: (h - 1) * c.s - 2 * c.p + c.k) if c.tr else (lambda h: (h + 2 * c.p - c.k) // c.s + 1)
    return f(c.H), f(c.W)


def w_shape(c):
    return (c.Cin, c.Cout, c.k, c.k) if c.tr else (c.Cout, c.Cin, c.k, c.k)


# ================================================================ float64 references
def act(x, ps, pb, pro):
    """What the kernels multiply: x, or the prologue of x (the zero padding comes after it)."""
    if pro == "none":
        return x
    a = x * ps.view(1, -1, 1, 1) + pb.view(1, -1, 1, 1)
    return a.clamp_min(0) if pro == "relu" else a


def conv_ref(a, w, c):
    return F.conv_transpose2d(a, w, None, c.s, c.p) if c.tr else F.conv2d(a, w, None, c.s, c.p)


def wgrad_ref(a, dy, c):
    """dL/dw of conv_ref(a, w, c) under the output gradient dy; the ConvTranspose2d one is the Conv2d one with the operands' roles swapped."""
    if c.tr:
        return torch.nn.grad.conv2d_weight(dy, w_shape(c), a, stride=c.s, padding=c.p)
    return torch.nn.grad.conv2d_weight(a, w_shape(c), dy, stride=c.s, padding=c.p)


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _signs(g, shape):
    return _ints(g, 0, 1, shape) * 2 - 1


def _nonzero(g, m, shape):
    return _ints(g, 1, m, shape) * _signs(g, shape)


def _masked(g, shape, one_in):
    return _signs(g, shape) * (torch.randint(0, one_in, shape, generator=g) == 0).to(F64)


def _pro_pair(g, C):
    return torch.tensor([1.0, 2.0, -1.0], dtype=F64)[torch.randint(0, 3, (C,), generator=g)], _ints(g, -1, 2, (C,))


RUNGS = ((4, 2), (8, 2), (16, 2), (16, 1))                                  # (weights: one in, |x| <=): the ladder


def _seed(c, pro, extra=0):
    return (((((c.Cin * 521 + c.Cout) * 7 + c.k) * 3 + c.s) * 131 + c.H) * 131 + c.W) * 401 + c.N + 7919 * PROS.index(pro) + (1 << 24) * c.tr + extra


def _small(c, pro, rung):
    one_in, xm = RUNGS[rung]
    g = torch.Generator().manual_seed(_seed(c, pro))
    Ho, Wo = out_hw(c)
    d = collections.OrderedDict()
    d["x"] = _ints(g, -xm, xm, (c.N, c.Cin, c.H, c.W))
    d["w"] = _masked(g, w_shape(c), one_in)
    d["dy"] = _ints(g, -2, 2, (c.N, c.Cout, Ho, Wo))
    d["ps"], d["pb"] = _pro_pair(g, c.Cin)
    d["dw_old"] = _nonzero(g, 4, w_shape(c))
    a = act(d["x"], d["ps"], d["pb"], pro)
    d["y"] = conv_ref(a, d["w"], c)
    d["dw"] = d["dw_old"] + wgrad_ref(a, d["dy"], c)
    cond = {"conv(|a|,|w|)": float(conv_ref(a.abs(), d["w"].abs(), c).max()), "sum|y|": float(d["y"].abs().sum((0, 2, 3)).max()),
            "sum y^2": float((d["y"] * d["y"]).sum((0, 2, 3)).max()),
            "|dw_old|+sum|a||dy|": float((d["dw_old"].abs() + wgrad_ref(a.abs(), d["dy"].abs(), c)).max())}
    return d, cond


def _dense(c, pro, m, extra):
    """Dense integers in [-m, m] on both sides: (tensors, the three forward conditions' values)."""
    g = torch.Generator().manual_seed(_seed(c, pro, extra))
    x, w = _ints(g, -m, m, (c.N, c.Cin, c.H, c.W)), _ints(g, -m, m, w_shape(c))
    ps, pb = _pro_pair(g, c.Cin)
    a = act(x, ps, pb, pro)
    y = conv_ref(a, w, c)
    cond = {"conv(|a|,|w|)": float(conv_ref(a.abs(), w.abs(), c).max()), "sum|y|": float(y.abs().sum((0, 2, 3)).max()),
            "sum y^2": float((y * y).sum((0, 2, 3)).max())}
    return dict(x=x, w=w, ps=ps, pb=pb, y=y), cond


def _wide(c, pro):
    """The wide regime; its statistics are gated too wherever their own conditions hold (the deep layers on small maps)."""
    d, cond = _dense(c, pro, 3, 1 << 28)
    d["gate_stats"] = cond["sum|y|"] <= CAP and cond["sum y^2"] <= CAP
    return d, {"wide " + k: v for k, v in cond.items() if d["gate_stats"] or k == "conv(|a|,|w|)"}


ROUND_AMPS = (12, 8, 6, 4)
ROUND_PIXELS = 1024


def _round(c, pro):
    """The rounding regime, statistics gated: on the cases with at most ROUND_PIXELS output pixels per channel, dense integers of the
    largest amplitude of ROUND_AMPS at which every forward condition holds -- large enough for |y| to pass 256 on the thin layers as well,
    so that a bf16 y differs from the accumulator the statistics must be taken from.  None where no amplitude fits."""
    Ho, Wo = out_hw(c)
    if c.N * Ho * Wo > ROUND_PIXELS:
        return None, {}
    for m in ROUND_AMPS:
        d, cond = _dense(c, pro, m, (1 << 27) + m)
        if max(cond.values()) <= CAP:
            d["gate_stats"] = True
            return d, {"round " + k: v for k, v in cond.items()}
    return None, {}


@functools.lru_cache(maxsize=2)
def case_data(c, pro):
    """(small-regime tensors, its rung, the dense regimes as (name, tensors), the exactness conditions' values) of a case; the same
    integers serve both dtypes."""
    for rung in range(len(RUNGS)):
        small, cond = _small(c, pro, rung)
        if max(cond.values()) <= CAP:
            break
    small["gate_stats"] = True
    wide, condw = _wide(c, pro)
    rnd, condr = _round(c, pro)
    cond.update(condw)
    cond.update(condr)
    return small, rung, (("wide", wide),) + ((("round", rnd),) if rnd is not None else ()), cond


def assert_exact(cond, what):
    bad = {k: v for k, v in cond.items() if not v <= CAP}
    assert not bad, ("exactness condition missed (cap 2^23)", what, bad)


def _pair_data(N, pro):
    c = Case("pair", 32, 32, 3, 2, 1, 0, 32, 32, N, ("bf16",))
    cs = c._replace(k=1, p=0)
    g = torch.Generator().manual_seed(_seed(c, pro, 1 << 29))
    d = dict(x=_ints(g, -2, 2, (N, 32, 32, 32)), dy=_ints(g, -2, 2, (N, 32, 16, 16)), dys=_ints(g, -2, 2, (N, 32, 16, 16)),
             old=_nonzero(g, 4, (32, 32, 3, 3)), olds=_nonzero(g, 4, (32, 32, 1, 1)))
    d["ps"], d["pb"] = _pro_pair(g, 32)
    a = act(d["x"], d["ps"], d["pb"], pro)
    d["dw"], d["dws"] = d["old"] + wgrad_ref(a, d["dy"], c), d["olds"] + wgrad_ref(a, d["dys"], cs)
    cond = {"pair dw": float((d["old"].abs() + wgrad_ref(a.abs(), d["dy"].abs(), c)).max()),
            "pair dw_sc": float((d["olds"].abs() + wgrad_ref(a.abs(), d["dys"].abs(), cs)).max())}
    return d, cond


@functools.lru_cache(maxsize=2)
def pair_data(N, pro):
    return _pair_data(N, pro)


def _fused_terms(C, H, N, second, pro, wide, g):
    c = Case("fused", C, 16, 4, 2, 1, 1, H, H, N, ("bf16",))
    m = 3 if wide else 2
    d = dict(c=c, x=_ints(g, -2, 2, (N, C, H, H)), dy=_ints(g, -m, m, (N, 16, 2 * H, 2 * H)),
             w=_ints(g, -3, 3, w_shape(c)) if wide else _masked(g, w_shape(c), 4), old=_nonzero(g, 4, w_shape(c)))
    d["ps"], d["pb"] = _pro_pair(g, C)
    a = act(d["x"], d["ps"], d["pb"], pro)
    dx, adx = F.conv2d(d["dy"], d["w"], None, 2, 1), F.conv2d(d["dy"].abs(), d["w"].abs(), None, 2, 1)
    cond = {}
    if second:
        d["x2"] = _ints(g, -m, m, (N, 16, H, H))
        d["w2"] = _ints(g, -3, 3, (C, 16)) if wide else _masked(g, (C, 16), 4)
        d["old2"] = _nonzero(g, 4, (16, C))
        dx = dx + torch.einsum("nkhw,ak->nahw", d["x2"], d["w2"])
        adx = adx + torch.einsum("nkhw,ak->nahw", d["x2"].abs(), d["w2"].abs())
        d["dw2"] = d["old2"] + torch.einsum("nkhw,nahw->ka", d["x2"], a)
        cond["fused dw2"] = float((d["old2"].abs() + torch.einsum("nkhw,nahw->ka", d["x2"].abs(), a.abs())).max())
    d["dx"], d["dw"] = dx, d["old"] + wgrad_ref(a, d["dy"], c)
    cond["fused dx"] = float(adx.max())
    cond["fused dw"] = float((d["old"].abs() + wgrad_ref(a.abs(), d["dy"].abs(), c)).max())
    return d, cond


@functools.lru_cache(maxsize=2)
def fused_data(C, H, N, second, pro):
    c = Case("fused", C, 16, 4, 2, 1, 1, H, H, N, ("bf16",))
    small, cond = _fused_terms(C, H, N, second, pro, False, torch.Generator().manual_seed(_seed(c, pro, (1 << 30) + int(second))))
    wide, cw = _fused_terms(C, H, N, second, pro, True, torch.Generator().manual_seed(_seed(c, pro, (1 << 30) + 2 + int(second))))
    cond["wide fused dx"] = cw["fused dx"]                                  # the wide regime gates dx alone
    return small, wide, cond


# ================================================================ CPU: conditions, ladder, reference
def test_exactness_conditions_and_ladder():
    """Every case of the file satisfies the exactness conditions (first, and with no GPU); the ladder's caps: density never below 1/16 (the
    last rungs), at most 10 % of the cases leave the first rung."""
    left, total, rounds = [], 0, collections.Counter()
    for c in CASES:
        for pro in PROS:
            _, rung, dense, cond = case_data(c, pro)
            assert_exact(cond, (case_id(c), pro))
            total += 1
            # where the statistics are gated and a bf16 y is not the accumulator: sums of the rounded y would be other numbers
            for name, d in dense:
                y, yr = d["y"], rbf(d["y"])
                if "bf16" in c.dts and d["gate_stats"] and bool((yr != y).any()) and bool((yr.sum((0, 2, 3)) != y.sum((0, 2, 3))).any()) and \
                        bool(((yr * yr).sum((0, 2, 3)) != (y * y).sum((0, 2, 3))).any()):
                    rounds[LAUNCHES[case_id(c)]["bf16"]["fwd"][0]] += 1
            if rung:
                left.append((case_id(c), pro, rung))
    print(f"LADDER {len(left)} of {total} cases left the first rung: {left}")
    assert min(one_in for one_in, _ in RUNGS) == 4 and max(one_in for one_in, _ in RUNGS) == 16
    assert len(left) <= 0.10 * total, left
    print("ROUNDING statistics-gated bf16 cases whose y rounds and whose rounded sums differ, per forward family:", dict(rounds))
    assert all(rounds[f] > 0 for f in (_G, _G3, _PC, _D2, _Q, _S3, _T4)), dict(rounds)
    worst = collections.defaultdict(float)
    for N in PAIR_NS:
        for pro in PROS:
            _, cond = pair_data(N, pro)
            assert_exact(cond, ("pair", N, pro))
            for k, v in cond.items():
                worst[k] = max(worst[k], v / CAP)
    for C, H, N, second in FUSED:
        for pro in PROS:
            _, _, cond = fused_data(C, H, N, second, pro)
            assert_exact(cond, ("fused", C, H, N, second, pro))
            for k, v in cond.items():
                worst[k] = max(worst[k], v / CAP)
    print("WORST pair / fused majorants, fractions of the cap:", dict(worst))


def test_reference_is_autograd():
    """wgrad_ref (torch.nn.grad.conv2d_weight, roles swapped for the ConvTranspose2d) and the fused references against torch.autograd in
    float64, on one case per distinct geometry with N = 2, prologue included; integers, so equality is exact."""
    seen = set()
    for c in CASES:
        key = c._replace(N=0, group="", dts=())
        if key in seen:
            continue
        seen.add(key)
        c = c._replace(N=2)
        for pro in ("relu", "affine"):
            d, _ = _small(c, pro, 0)
            w = d["w"].clone().requires_grad_(True)
            y = conv_ref(act(d["x"], d["ps"], d["pb"], pro), w, c)
            assert torch.equal(y.detach(), d["y"]) and y.shape[2:] == out_hw(c), case_id(c)
            (y * d["dy"]).sum().backward()
            assert torch.equal(d["dw"], d["dw_old"] + w.grad), (case_id(c), pro)
    for second in (False, True):
        d, _ = _fused_terms(32, 16, 2, second, "relu", False, torch.Generator().manual_seed(5))
        a = act(d["x"], d["ps"], d["pb"], "relu").requires_grad_(True)
        w = d["w"].clone().requires_grad_(True)
        loss = (F.conv_transpose2d(a, w, None, 2, 1) * d["dy"]).sum()
        if second:                                                          # the 1x1 conv (16, C) beside it, its output gradient x2
            w1 = d["w2"].t().contiguous().clone().requires_grad_(True)
            loss = loss + (torch.einsum("nahw,ka->nkhw", a, w1) * d["x2"]).sum()
        loss.backward()
        assert torch.equal(a.grad, d["dx"]) and torch.equal(d["old"] + w.grad, d["dw"]), second
        if second:
            assert torch.equal(d["old2"] + w1.grad, d["dw2"])
    d, _ = _pair_data(2, "relu")
    a = act(d["x"], d["ps"], d["pb"], "relu")
    w1, ws = torch.zeros(32, 32, 3, 3, dtype=F64, requires_grad=True), torch.zeros(32, 32, 1, 1, dtype=F64, requires_grad=True)
    ((F.conv2d(a, w1, None, 2, 1) * d["dy"]).sum() + (F.conv2d(a, ws, None, 2, 0) * d["dys"]).sum()).backward()
    assert torch.equal(d["old"] + w1.grad, d["dw"]) and torch.equal(d["olds"] + ws.grad, d["dws"])


def test_lattice_values_are_exact_in_both_storage_types():
    """The operands survive the storage types, and the wide regime really rounds: some |y| is not a bf16 number."""
    v = torch.arange(-9, 10, dtype=F64)                                     # the largest prologue'd operand is 3 * 2 + 2
    assert torch.equal(v.to(torch.bfloat16).double(), v) and torch.equal(v.float().double(), v)
    c = next(c for c in CASES if c.Cin == 256)
    _, _, dense, _ = case_data(c, "none")
    y = dict(dense)["wide"]["y"]
    assert float(y.abs().max()) > 256 and int((rbf(y) != y).sum()) > 0
    assert torch.equal(rbf(y).to(torch.bfloat16).double(), rbf(y)) and torch.equal(y.float().to(torch.bfloat16).double(), rbf(y))
    assert _header_macro("MMVAE_WGRAD_SCRATCH_BYTES") == WSCRATCH_BYTES and _header_macro("MMVAE_CONV_STATS_MAX_ROWS") == STATS_ROWS
    assert len({case_id(c) for c in CASES}) == len(CASES)
    assert {(case_id(c), dt) for c in CASES for dt in c.dts} >= WGRAD_REFUSED


# ================================================================ device side
def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(TDT[dt])


def nchw64(t):
    return t.double().permute(0, 3, 1, 2).cpu()


def store(t, dt):
    """What a storage type holds of an exact integer result."""
    return rbf(t) if dt == "bf16" else t


def first_diff(got, want, names):
    """The first mismatching index with the integer difference: it usually names the missing term."""
    bad = (got != want) | (got != got)
    idx = bad.nonzero()[0].tolist()
    g, w = float(got[tuple(idx)]), float(want[tuple(idx)])
    return f"{int(bad.sum())} of {bad.numel()} differ; first at {dict(zip(names, idx))}: device {g}, reference {w}, difference {g - w}"


def equal_or_explain(got, want, names, what):
    assert torch.equal(got, want), (what, first_diff(got, want, names))


_WS = []


def wscratch():
    """MMVAE_WGRAD_SCRATCH_BYTES of 0xFF bytes in a guarded arena, one per process, refilled in front of every call."""
    if not _WS:
        _WS.append(Arena(WSCRATCH_BYTES, 0xFF))
    _WS[0].buf.fill_(0xFF)
    return _WS[0]


def es_of(dt):
    return 2 if dt == "bf16" else 4


def call_fwd(lib, c, dt, relu, x, w, y, ps, pb, stats, sc):
    return lib.mmvae_conv2d_fwd(DTI[dt], c.tr, P(x), P(w), P(y), c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.s, c.p, P(ps), P(pb), relu, P(stats), sc, stream())


def call_wgrad(lib, c, dt, relu, x, dy, dw, ps, pb, ws):
    return lib.mmvae_conv2d_wgrad(DTI[dt], c.tr, P(x), P(dy), P(dw), c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.s, c.p, P(ps), P(pb), relu, ws, stream())


class Ops:
    """A case's operands on the device, each a guarded window, and the entry points as calls on them."""

    def __init__(self, c, dt, pro):
        self.c, self.dt, self.pro = c, dt, pro
        self.L = _L()
        self.lib = self.L.lib()
        self.D = Dev()
        self.n = 0
        self.put, self.scratch = self.D.put, self.D.scratch

    def vec(self, name, v):
        return None if self.pro == "none" else self.put(name, v.float())

    def new(self, name, shape, dtype, fill):
        self.n += 1
        return self.put(f"{name}{self.n}", (tuple(shape), dtype), fill)

    def relu(self):
        return 1 if self.pro == "relu" else 0

    def fwd(self, x, w, y, ps, pb, stats, sc):
        return call_fwd(self.lib, self.c, self.dt, self.relu(), x, w, y, ps, pb, stats, sc)

    def wgrad(self, x, dy, dw, ps, pb, ws):
        return call_wgrad(self.lib, self.c, self.dt, self.relu(), x, dy, dw, ps, pb, ws)


def check_fwd(o, d, regime, what):
    """One forward regime: y's bits, the rows, the statistics, the tail of the statistics buffer, the weight = NULL repeat."""
    c, dt = o.c, o.dt
    Ho, Wo = out_hw(c)
    x, w = o.put(f"x_{regime}", nhwc(d["x"], dt)), o.put(f"w_{regime}", d["w"].float())
    ps, pb = o.vec(f"ps_{regime}", d["ps"]), o.vec(f"pb_{regime}", d["pb"])
    sc = o.scratch(f"scratch_{regime}", 2 * d["w"].numel() * es_of(dt) + 64)
    gate_stats = d["gate_stats"]
    ys, sts, rows = [], [], []
    for rep in range(2):
        y = o.new("y", (c.N, Ho, Wo, c.Cout), TDT[dt], 0xFF)
        st = o.new("stats", (STATS_ROWS, 2, c.Cout), torch.float32, 0xA5) if gate_stats else None
        rc = o.fwd(x, w if rep == 0 else None, y, ps, pb, st, sc)
        if rc < 0:
            return rc
        ys.append(y), sts.append(st), rows.append(rc)
    torch.cuda.synchronize()
    o.D.check(what)
    equal_or_explain(nchw64(ys[0]), store(d["y"], dt), ("image", "channel", "row", "column"), (what, regime, "y"))
    assert same_bits(ys[0], ys[1]), ("the call with weight = NULL differs", what, regime)
    assert rows[0] == rows[1] and 0 < rows[0] <= STATS_ROWS, (what, rows)
    if gate_stats:
        r = rows[0]
        got = sts[0][:r].cpu().double().sum(0)                              # on the host, in float64
        want = torch.stack([d["y"].sum((0, 2, 3)), (d["y"] * d["y"]).sum((0, 2, 3))])
        equal_or_explain(got, want, ("sum / sum of squares", "channel"), (what, "statistics over", r, "rows"))
        assert same_bits(sts[0][:r], sts[1][:r]), ("statistics of the weight = NULL call differ", what)
        tail = sts[0][r:].contiguous().view(torch.uint8)
        assert bool((tail == 0xA5).all()), ("statistics rows past the returned count were written", what, r)
    return rows[0]


def check_wgrad(o, d, what):
    c, dt = o.c, o.dt
    x, dy = o.put("x_wg", nhwc(d["x"], dt)), o.put("dy", nhwc(d["dy"], dt))
    ps, pb = o.vec("ps_wg", d["ps"]), o.vec("pb_wg", d["pb"])
    dws = []
    for rep in range(2):
        dw = o.put(f"dw{rep}", d["dw_old"].float())
        ws = wscratch()
        rc = o.wgrad(x, dy, dw, ps, pb, ws.ptr())
        if rc < 0:
            torch.cuda.synchronize()
            assert torch.equal(dw.double().cpu(), d["dw_old"]) and ws.untouched(), ("a refused weight gradient wrote", what)
            return rc
        torch.cuda.synchronize()
        assert ws.intact(), ("guard bytes changed around the weight-gradient scratch", what)
        dws.append(dw)
    o.D.check(what)
    equal_or_explain(dws[0].double().cpu(), d["dw"], ("out" if not c.tr else "in", "in" if not c.tr else "out", "kh", "kw"), (what, "dw = dw_old + R64"))
    assert same_bits(dws[0], dws[1]), ("not bit-reproducible", what)
    return 0


CONV_PARAMS = [pytest.param(c, pro, dt, id=f"{case_id(c)}-{pro}-{dt}") for c in CASES for pro in PROS for dt in c.dts]


@gpu
@pytest.mark.parametrize("c,pro,dt", CONV_PARAMS)
def test_conv_lattice(c, pro, dt):
    small, _, dense, cond = case_data(c, pro)
    what = f"{case_id(c)} {dt} {pro}"
    assert_exact(cond, what)
    o = Ops(c, dt, pro)
    free = c.group == "nonsq"                                               # may be refused instead: untouched outputs then
    for regime, d in (("small", small),) + dense:
        rc = check_fwd(o, d, regime, what)
        if rc < 0:
            assert free, (what, "forward refused", rc, o.lib.mmvae_last_error())
            torch.cuda.synchronize()
            assert all(a.untouched() for n, a in o.D.arenas.items() if n.startswith(("y", "stats", "scratch"))), ("a refused forward wrote", what)
    rc = check_wgrad(o, small, what)
    if rc < 0:
        assert free or (case_id(c), dt) in WGRAD_REFUSED, (what, "weight gradient refused", rc, o.lib.mmvae_last_error())
    else:
        assert (case_id(c), dt) not in WGRAD_REFUSED, (what, "expected the refusal")


@gpu
@pytest.mark.parametrize("pro", PROS)
@pytest.mark.parametrize("N", PAIR_NS)
def test_wgrad_pair_lattice(N, pro):
    d, cond = pair_data(N, pro)
    what = f"pair N{N} {pro}"
    assert_exact(cond, what)
    c = Case("pair", 32, 32, 3, 2, 1, 0, 32, 32, N, ("bf16",))
    o = Ops(c, "bf16", pro)
    x, dy, dys = o.put("x", nhwc(d["x"], "bf16")), o.put("dy", nhwc(d["dy"], "bf16")), o.put("dys", nhwc(d["dys"], "bf16"))
    ps, pb = o.vec("ps", d["ps"]), o.vec("pb", d["pb"])
    res = []
    for rep in range(2):
        dw, dws = o.put(f"dw{rep}", d["old"].float()), o.put(f"dws{rep}", d["olds"].float())
        ws = wscratch()
        o.L.check(o.lib.mmvae_conv2d_wgrad_pair(1, P(x), P(dy), P(dys), P(dw), P(dws), N, 32, 32, 32, 32, P(ps), P(pb), o.relu(), ws.ptr(), stream()), what)
        torch.cuda.synchronize()
        assert ws.intact(), what
        res.append((dw, dws))
    o.D.check(what)
    equal_or_explain(res[0][0].double().cpu(), d["dw"], ("out", "in", "kh", "kw"), (what, "dw"))
    equal_or_explain(res[0][1].double().cpu(), d["dws"], ("out", "in", "kh", "kw"), (what, "dw_sc"))
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]), ("not bit-reproducible", what)


def run_fused(o, d, second, dw2_too=True):
    c = o.c
    x, dy, w = o.put("x", nhwc(d["x"], "bf16")), o.put("dy", nhwc(d["dy"], "bf16")), o.put("w", d["w"].float())
    ps, pb = o.vec("ps", d["ps"]), o.vec("pb", d["pb"])
    x2 = o.put("x2", nhwc(d["x2"], "bf16")) if second else None
    w2 = o.put("w2", d["w2"].float()) if second else None
    sc = o.scratch("scratch", (d["w"].numel() + (d["w2"].numel() if second else 0)) * 2)
    res = []
    for rep in range(2):
        dw = o.put(f"dw{rep}", d["old"].float())
        dw2 = o.put(f"dw2{rep}", d["old2"].float()) if second and dw2_too else None
        dx = o.new("dx", (c.N, c.H, c.H, c.Cin), torch.bfloat16, 0xFF)
        ws = wscratch()
        rc = o.lib.mmvae_convT_bwd_fused(1, P(x), P(dy), P(w), P(dw), P(dx), c.N, c.H, c.H, c.Cin, 16, 4, 2, 1, P(ps), P(pb), o.relu(), P(x2), P(w2), P(dw2),
                                         sc, ws.ptr(), stream())
        o.L.check(rc, "convT_bwd_fused")
        torch.cuda.synchronize()
        assert ws.intact()
        res.append((dw, dx, dw2))
    return res


@gpu
@pytest.mark.parametrize("pro", PROS)
@pytest.mark.parametrize("C,H,N,second", FUSED, ids=lambda v: str(int(v)))
def test_convT_bwd_fused_lattice(C, H, N, second, pro):
    small, wide, cond = fused_data(C, H, N, second, pro)
    what = f"fused C{C} H{H} N{N} second={second} {pro}"
    assert_exact(cond, what)
    for regime, d in (("small", small), ("wide", wide)):
        o = Ops(d["c"], "bf16", pro)
        res = run_fused(o, d, second)
        o.D.check(what)
        equal_or_explain(nchw64(res[0][1]), rbf(d["dx"]), ("image", "channel", "row", "column"), (what, regime, "dx"))
        assert same_bits(res[0][1], res[1][1]), ("dx not bit-reproducible", what, regime)
        if regime == "small":
            equal_or_explain(res[0][0].double().cpu(), d["dw"], ("in", "out", "kh", "kw"), (what, "dw"))
            assert same_bits(res[0][0], res[1][0]), ("dw not bit-reproducible", what)
            if second:
                equal_or_explain(res[0][2].double().cpu(), d["dw2"], ("out", "in"), (what, "dw2"))
                assert same_bits(res[0][2], res[1][2]), ("dw2 not bit-reproducible", what)


# ================================================================ refusals
def refusal_calls(lib, bufs, st=None):
    """name -> return code of every refused call, on `bufs` = dict of pointers (x, w, y, dy, dy2, dw, dw2, dx, stats, sc, ws)."""
    b = bufs
    fwd = lambda dt=1, tr=0, Cin=32, Cout=32, k=3, s=1, p=1: lib.mmvae_conv2d_fwd(dt, tr, b["x"], b["w"], b["y"], 1, 8, 8, Cin, Cout, k, s, p, None, None, 0,
                                                                                   b["stats"], b["sc"], st)
    wg = lambda dt=1, tr=0, Cin=32, Cout=32, k=3, s=1, p=1: lib.mmvae_conv2d_wgrad(dt, tr, b["x"], b["dy"], b["dw"], 1, 8, 8, Cin, Cout, k, s, p, None, None,
                                                                                   0, b["ws"], st)
    pair = lambda dt=1, H=32, C=32: lib.mmvae_conv2d_wgrad_pair(dt, b["x"], b["dy"], b["dy2"], b["dw"], b["dw2"], 1, H, H, C, C, None, None, 0, b["ws"], st)
    fused = lambda dt=1, H=32, C=16: lib.mmvae_convT_bwd_fused(dt, b["x"], b["dy"], b["w"], b["dw"], b["dx"], 1, H, H, C, 16, 4, 2, 1, None, None, 0, None, None,
                                                               None, b["sc"], b["ws"], st)
    return {"fwd k = 7": fwd(k=7, p=3), "fwd k = 7 transposed": fwd(tr=1, k=7, s=2, p=3), "wgrad k = 7": wg(k=7, p=3),
            "fwd bf16 Cin = 12": fwd(Cin=12), "fwd f32 Cin = 6": fwd(dt=0, Cin=6), "fwd Cout = 6": fwd(Cout=6), "fwd transposed Cin = 12": fwd(tr=1, Cin=12, k=4, s=2),
            "wgrad bf16 Cin = 12": wg(Cin=12), "wgrad f32 Cout = 6": wg(dt=0, Cout=6),
            "wgrad bf16 8 -> 8 1x1 (64 elements)": wg(Cin=8, Cout=8, k=1, p=0), "wgrad f32 4 -> 4 3x3 (144 elements)": wg(dt=0, Cin=4, Cout=4),
            "wgrad f32 4 -> 16 3x3 (576 elements)": wg(dt=0, Cin=4, Cout=16),
            "fused on 8x8 maps": fused(H=8), "fused 48 channels": fused(C=48), "fused f32": fused(dt=0),
            "pair on 16x16 maps": pair(H=16), "pair 64 channels": pair(C=64), "pair f32": pair(dt=0),
            "fwd dtype 7": fwd(dt=7), "wgrad dtype 7": wg(dt=7), "pair dtype 7": pair(dt=7), "fused dtype 7": fused(dt=7)}


def test_refusals_need_no_device(pkg):
    """Every refusal returns before anything is enqueued: where there is no device, host buffers stand in for the device ones and stay as
    they are.  Where there is one, a refusal that regressed would hand these host pointers to a kernel, so the guarded device variant below
    is the test there and this one leaves the calls to it."""
    import ctypes
    if torch.cuda.is_available():
        return test_refusals_leave_outputs_untouched()
    lib = _L().lib()
    names = ("x", "w", "y", "dy", "dy2", "dw", "dw2", "dx", "stats", "sc", "ws")
    host = {n: (ctypes.c_uint8 * 64)(*([0xA5] * 64)) for n in names}
    got = refusal_calls(lib, {n: ctypes.addressof(v) for n, v in host.items()})
    assert all(rc < 0 for rc in got.values()), got
    assert lib.mmvae_last_error()
    assert all(bytes(v) == b"\xa5" * 64 for v in host.values())


@gpu
def test_refusals_leave_outputs_untouched():
    lib = _L().lib()
    D = Dev()
    sizes = dict(x=1 << 20, w=1 << 20, y=1 << 20, dy=1 << 20, dy2=1 << 20, dw=1 << 20, dw2=1 << 16, dx=1 << 20, stats=1 << 20, sc=1 << 20)
    bufs = {n: D.scratch(n, nb) for n, nb in sizes.items()}
    ws = wscratch()
    bufs["ws"] = ws.ptr()
    got = refusal_calls(lib, bufs, stream())
    torch.cuda.synchronize()
    assert all(rc < 0 for rc in got.values()), got
    wrote = [n for n, a in D.arenas.items() if not a.untouched()]
    assert not wrote and ws.untouched(), ("a refused call wrote", wrote)


# ================================================================ census (keep last)
_G, _G3, _PC, _D2, _Q, _S3, _T4 = "gather_gemm", "gather3", "patch_conv", "deep2_conv", "pos_conv", "conv3_stream", "convT4_stream"
_WS_, _WP, _W2, _WF, _WR = "wgrad_stream", "wgrad_pos", "wgrad2", "wgrad", "wgrad_reduce"
FAMILIES = (_WS_, _WP, _W2, _WF, _WR, _G, _G3, _PC, _D2, _Q, _S3, _T4)
_CODE = {"G": _G, "3": _G3, "P": _PC, "D": _D2, "Q": _Q, "S": _S3, "T": _T4, "s": _WS_, "p": _WP, "2": _W2, "f": _WF, "-": None}
# Launcher family per case and storage type: forward, then the weight gradient's first kernel (wgrad_reduce follows it in every taken case;
# "-": refused, nothing launched; ".": not a case of that storage type), bf16 then f32.  Filled from the dispatch code (launch_gather_gemm,
# launch_wgrad, conv3_stream_ok, convT4_stream_ok in csrc/), corrected from the device: see the docstring.
_TABLE = """
net-32x32k3s2-16x16-N3 P2G2
net-32x32k3s1-8x8-N3 P2G2
net-32x32k1s2-16x16-N3 P23f
net-32x64k3s2-8x8-N5 DpD2
net-64x64k3s1-8x8-N2 D2D2
net-32x64k1s2-8x8-N5 D2Df
net-64x128k3s2-8x8-N3 DpD2
net-128x128k3s1-4x4-N7 QpD2
net-64x128k1s2-8x8-N3 D2Df
net-128x256k3s2-4x4-N9 QpD2
net-256x256k3s1-2x2-N11 QpD2
net-128x256k1s2-4x4-N9 Q2Df
net-32x32k3s2-7x7-N3 G2G2
net-32x32k1s2-7x7-N3 P23f
net-64x64k3s1-5x5-N3 D2D2
net-128x128k1s1-2x2-N9 Q2D2
net-128x64k1s1-4x4-N5 Q2D2
net-64x32k1s1-8x8-N3 D2D2
net-32x16k1s1-16x16-N3 P2P2
net-16x16k1s1-32x32-N2 P2P2
net-128x128k4s2T-2x2-N9 QpDf
net-128x64k4s2T-4x4-N5 QpD2
net-64x64k4s2T-4x4-N5 QpD2
net-64x32k4s2T-8x8-N3 D2D2
net-32x32k4s2T-8x8-N3 P232
net-32x16k4s2T-16x16-N2 PsP2
net-16x16k4s2T-16x16-N2 TsP2
net-16x16k4s2T-32x32-N1 TsP2
net-32x128k2s2T-1x1-N37 D2D2
net-128x128k2s2T-1x1-N300 Q2D2
net-16x16k1s1-64x64-N40 P2P2
net-16x16k4s2T-32x32-N36 TsP2
net-16x16k3s1-64x64-N2 P2P2
net-32x32k4s2T-16x16-N4 P232
net-16x32k3s2-64x64-N2 P2P2
net-32x16k3s1-32x32-N3 P2P2
net-16x16k4s2-64x64-N2 PsP2
net-32x16k4s2T-32x32-N5 PsP2
net-16x16k4s2T-32x32-N70 TsP2
net-32x32k3s2-32x32-N3 SsG2
net-32x32k3s1-16x16-N5 SsG2
net-32x32k3s2-32x32-N41 SsG2
net-128x128k3s1-4x4-N37 QpD2
net-256x256k3s1-2x2-N70 QpD2
net-128x256k3s2-4x4-N45 QpD2
net-64x128k3s2-8x8-N19 DpD2
net-128x128k4s2T-2x2-N50 QpDf
net-128x64k4s2T-4x4-N21 QpD2
net-64x64k4s2T-4x4-N33 QpD2
net-128x256k1s2-4x4-N40 Q2Df
net-128x128k1s1-2x2-N41 Q2D2
net-128x64k1s1-4x4-N18 Q2D2
net-128x128k2s2T-1x1-N100 Q2D2
one-32x16k4s2T-32x32-N1 PsP2
one-16x16k4s2T-16x16-N1 TsP2
one-32x16k4s2T-16x16-N1 PsP2
one-32x32k3s1-16x16-N1 SsG2
one-32x32k3s2-32x32-N1 SsG2
pos-256x256k3s1-2x2-N1 QpD2
pos-128x64k4s2T-4x4-N1 QpD2
pos-64x128k3s2-8x8-N1 DpD2
pos-256x256k3s1-2x2-N37 QpD2
pos-128x64k4s2T-4x4-N37 QpD2
pos-64x128k3s2-8x8-N37 DpD2
pos-256x256k3s1-2x2-N70 QpD2
pos-128x64k4s2T-4x4-N70 QpD2
pos-64x128k3s2-8x8-N70 DpD2
nonsq-32x32k3s1-16x32-N3 P2G2
nonsq-32x32k3s1-32x16-N3 P2G2
nonsq-16x16k4s2T-32x16-N3 P2P2
nonsq-64x64k3s1-8x4-N5 D2D2
nonsq-128x128k3s1-4x2-N9 D2D2
nonsq-32x32k1s2-16x8-N3 P23f
off-48x48k3s1-8x8-N5 GfGf
off-96x32k1s1-8x8-N5 3f3f
off-8x32k3s1-8x8-N5 Pf..
off-4x16k3s1-8x8-N5 ..P-
off-32x8k4s2T-8x8-N5 PfPf
"""


def _parse_table():
    out = {}
    for ln in _TABLE.strip().splitlines():
        cid, codes = ln.split()
        row = {}
        for dt, (f, g) in zip(DTS, (codes[0:2], codes[2:4])):
            if f != ".":
                row[dt] = {"fwd": (_CODE[f],), "wgrad": (_CODE[g], _WR) if _CODE[g] else ()}
        out[cid] = row
    return out


LAUNCHES = _parse_table()
PAIR_LAUNCHES = (_WS_, _WR, _WR)
FUSED_LAUNCHES = {False: (_WS_, _WR), True: (_WS_, _WR, _WR)}


def census_plan():
    plan = [(case_id(c), dt, op) for c in CASES for dt in c.dts for op in ("fwd", "wgrad")]
    plan += [(f"pair N{N}", "bf16", "pair") for N in PAIR_NS]
    plan += [(f"fused {C} {H} {N} {int(second)}", "bf16", "fused") for C, H, N, second in FUSED]
    return plan + [("refusals", "bf16", "refusals")]


def census_child():
    """Every case and entry point once (zero operands: the dispatch does not look at the data), an 8-element mmvae_convert in front of each."""
    lib = _L().lib()
    a, b = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    by_id = {case_id(c): c for c in CASES}
    ws = torch.zeros(WSCRATCH_BYTES, dtype=torch.uint8, device="cuda")
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    done = []
    for label, dt, op in census_plan():
        assert lib.mmvae_convert(0, 0, P(a), P(b), 8, stream()) == 0
        tdt = TDT[dt]
        if op in ("fwd", "wgrad"):
            c = by_id[label]
            Ho, Wo = out_hw(c)
            x, ps, pb = z((c.N, c.H, c.W, c.Cin), tdt), z(c.Cin), z(c.Cin)
            if op == "fwd":
                rc = call_fwd(lib, c, dt, 1, x, z(w_shape(c)), z((c.N, Ho, Wo, c.Cout), tdt), ps, pb, z((STATS_ROWS, 2, c.Cout)),
                              z(2 * c.Cin * c.Cout * c.k * c.k + 64).data_ptr())
            else:
                rc = call_wgrad(lib, c, dt, 1, x, z((c.N, Ho, Wo, c.Cout), tdt), z(w_shape(c)), ps, pb, ws.data_ptr())
        elif op == "pair":
            N = int(label.split("N")[1])
            rc = lib.mmvae_conv2d_wgrad_pair(1, P(z((N, 32, 32, 32), tdt)), P(z((N, 16, 16, 32), tdt)), P(z((N, 16, 16, 32), tdt)), P(z((32, 32, 3, 3))),
                                             P(z((32, 32, 1, 1))), N, 32, 32, 32, 32, None, None, 0, ws.data_ptr(), stream())
        elif op == "fused":
            C, H, N, second = (int(v) for v in label.split()[1:])
            x2, w2, dw2 = (z((N, H, H, 16), tdt), z((C, 16)), z((16, C))) if second else (None, None, None)
            rc = lib.mmvae_convT_bwd_fused(1, P(z((N, H, H, C), tdt)), P(z((N, 2 * H, 2 * H, 16), tdt)), P(z((C, 16, 4, 4))), P(z((C, 16, 4, 4))),
                                           P(z((N, H, H, C), tdt)), N, H, H, C, 16, 4, 2, 1, None, None, 0, P(x2), P(w2), P(dw2), z(1 << 16).data_ptr(),
                                           ws.data_ptr(), stream())
        else:
            big = lambda: z(1 << 18).data_ptr()
            rcs = refusal_calls(lib, dict(x=big(), w=big(), y=big(), dy=big(), dy2=big(), dw=big(), dw2=big(), dx=big(), stats=big(), sc=big(), ws=ws.data_ptr()),
                                stream())
            rc = max(rcs.values())
        torch.cuda.synchronize()
        done.append([label, dt, op, rc])
    print("CENSUS_PLAN " + json.dumps(done))


def census_segments(tmp_path, script=os.path.abspath(__file__)):
    """Run `script --census-child` under the launch census: (what the child says it ran, the launcher names of every segment)."""
    prefix = str(tmp_path / "census")
    env = dict(os.environ, MMVAE_LAUNCH_STATS=prefix, MMVAE_LAUNCH_SEQ="1")
    r = subprocess.run([sys.executable, script, "--census-child"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
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
    return done, segs


@gpu
def test_launch_census(tmp_path):
    done, segs = census_segments(tmp_path)
    wrong, seen = [], collections.Counter()
    for (label, dt, op, rc), seg in zip(done, segs):
        print(f"CENSUS {label} {dt} {op} rc={rc}: {' '.join(seg)}")
        if op == "refusals":
            assert rc < 0 and seg == [], ("a refused call enqueued something", rc, seg)   # not even the packing launch
            continue
        seg = tuple(n for n in seg if n not in ("pack", "pack_multi"))
        want = PAIR_LAUNCHES if op == "pair" else FUSED_LAUNCHES[label.endswith("1")] if op == "fused" else LAUNCHES[label][dt][op]
        if seg != want or (rc < 0) != (want == ()):
            wrong.append((label, dt, op, rc, seg, want))
        seen.update(seg)
    assert not wrong, wrong
    missing = [f for f in FAMILIES if not seen[f]]
    assert not missing, (missing, dict(seen))


if __name__ == "__main__":
    if sys.argv[1:] == ["--census-child"]:
        census_child()
    else:
        for fn in (test_exactness_conditions_and_ladder, test_reference_is_autograd, test_lattice_values_are_exact_in_both_storage_types):
            fn()
            print("ok", fn.__name__)
