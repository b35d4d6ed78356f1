"""Float64 gates of the weight gradients on real-valued data, through mmvae_conv2d_wgrad and mmvae_conv2d_wgrad_pair: what the lattice file
(test_conv_lattice_gpu.py: bit equality on integer inputs) cannot see -- loss of precision -- at sizes where a single lost product is still
visible.  Conventions and helpers of test_upblock_ops_f64_gpu.py; the cases' launcher families are those the lattice file's census pins
(looked up in its LAUNCHES by geometry, asserted on the CPU) and, since this file's N are not that file's, a census of its own (last test)
pins on the device that every case runs on the family its bound is built for: the stream kinds 1 - 4, the position-major kernel, the patch-tile kernel
(wgrad2_kernel) in both storage types -- a 1x1 (k-split form), a 9-wave and a 16-wave form, a non-square map -- and the fallback
(wgrad_kernel) in both.  Every case runs with and without the prologue, which sits on x: the G side of a Conv2d, the P side of a
ConvTranspose2d.

Data: randn times per-channel magnitudes spread over 2^+-2 (span); prologue scale and shift as bn_pair draws them (scale * x is O(1), the
shift is not negligible); dw_old = randn, never zero.

References, float64, built on the CPU from the exact tensors handed to the device (x, dy already rounded to the storage type):
  R64  autograd's weight gradient of the layer on relu(x * scale + shift) (torch.nn.grad.conv2d_weight, tied to autograd on the CPU), + dw_old;
  Rq   the same with a rounding wherever the code rounds (read off the .hip files):
       - the prologue is evaluated in f32 on load -- `f * scale + shift`, fused or not as compiled, then fmaxf(., 0) -- in wgrad_kernel's
         staging loops (conv_gemm.hip), apply_pro (conv_wgrad.inc) and the stream / position kernels' loaders; its result is rounded to bf16
         on its way into LDS in bf16 mode (Elem<T>::store / pack).  Rq takes the float64 pre-activation; the f32 evaluation is 2 u of the
         terms' magnitudes away, and where a bf16 rounding midpoint (or the ReLU's zero) lies within that, the device may land on the
         neighbour: one bf16 step (prologue / relu_e / rbf_e of the sibling file), propagated through |dy| into the bound;
       - bf16 x bf16 products are exact in the MFMA's f32; f32 mode (v_mfma_f32_16x16x4f32) rounds every product: u per product;
       - no other rounding before the f32 accumulation: partial images are f32, wgrad_reduce_kernel adds them in f32, `dW +=` is one f32 add.
The device is gated against Rq; |Rq - R64| is printed and gates nothing.

Bound per weight element, units of u = 2^-24, derived (K = N Hp Wp, the pixel axis; A = sum |products| of the element):
  * the K-slab rule of test_conv_join_ops_f64_gpu.py on each partial image p, order-free: an accumulator pays one rounding of at most
    |C| + sum |products| <= A_p per product slot and per slab; slots that hold a zero (padding, ragged tiles) add nothing, so a partial
    image with K_p real pixels pays u (K_p + 32) A_p in bf16 (its last slab may be ragged) and u (K_p + 1) A_p + u A_p in f32; summed over
    the partial images with K_p <= K, sum A_p = A: u (K + 32 nparts) A, resp. u (K + 1 + nparts) A;
  * the reduce: nparts - 1 real additions, each result at most A: u (nparts - 1) A whatever the order and the tree (LANES = 8 .. 64; the
    walk of wgrad_reduce_kernel is modelled for every LANES by reduce_err below -- wgrad_reduce_err of the sibling file extended -- and the
    CPU self-check holds the order-free majorant against it);
  * nparts from the launchers' grid rules, as an upper bound where the exact value needs the LDS fit: the stream kernels' `while (gx > 8 &&
    gx * nw > nunits) gx -= 8` exactly; position-major ceil(N / 32) (a split holds at least two 16-image chunks); patch-tile 176; fallback
    ceil(K / 64) in bf16, ceil(K / 32) in f32 (one part per K-step at most);
  * u (|result| + incoming) for the `+=`;
  * SLOP = 1.01.
The gate is per (out, in, tap) element, nothing excluded.  Sharpness, asserted on the CPU per case: the median over elements of
bound / (A / K) is below 1 -- one lost average product would exceed the bound.  Mutants the gate must fail, on the CPU: one pixel's
contribution removed, kh and kw swapped on a non-square map, the prologue applied to the zero padding, `=` for `+=`; Rq itself passes.

Measured on the MI355X: the whole file, 39 GPU tests, in about 5 s (its census child 2.1 s of it); the CPU self-checks in 4 s.  Worst err / bound per family (plain / prologue):
  wgrad_stream  bf16 0.0002 / 0.0004      pair: dw 0.0008 / 0.0010, dw_sc 0.0006 / 0.0010
  wgrad_pos     bf16 0.0090 / 0.91
  wgrad2        bf16 0.0001 / 0.0011      f32 0.0018 / 0.0025
  wgrad         bf16 0.0015 / 0.0059      f32 0.0031 / 0.0062
The 0.91 is 256 -> 256 on 2x2 maps with the prologue: one of its 38 000 prologue'd values sits within 2 u of a bf16 rounding midpoint and
the device landed on the other side -- one bf16 step times |dy| against a chain bound of only 213 u A (K = 148); the same case without
the prologue is at 0.009.  Everything else sits at 1e-3 .. 1e-2 by construction: the order-free majorant charges every product slot a
rounding of the element's whole magnitude A, the hardware's errors add up like sqrt(K) of the typical partial sum.  The bounds are
nevertheless below one average product (median bound / (A / K): 0.002 .. 0.42 over the cases).
"""
import collections
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_conv_lattice_gpu as LAT  # noqa: E402
from test_conv_lattice_gpu import Case, case_id, out_hw, w_shape, wgrad_ref, wscratch  # noqa: E402
from test_upblock_ops_f64_gpu import (DTI, F64, SLOP, TDT, U, Dev, P, _L, _ratio, gate, gpu, prologue, sgn, span, stream,  # noqa: E402
                                      wgrad_reduce_err)

DTS = ("bf16", "f32")
_B, _BF = ("bf16",), DTS
CASES = [
    # (family, case): K = N Hp Wp <= 2048 for the stream and position kernels, <= 1024 for the patch-tile kernel
    ("wgrad_stream", Case("kind1", 16, 16, 4, 2, 1, 1, 32, 32, 2, _B)), ("wgrad_stream", Case("kind2", 32, 16, 4, 2, 1, 1, 16, 16, 5, _B)),
    ("wgrad_stream", Case("kind3", 32, 32, 3, 1, 1, 0, 16, 16, 5, _B)), ("wgrad_stream", Case("kind4", 32, 32, 3, 2, 1, 0, 32, 32, 5, _B)),
    ("wgrad_pos", Case("pos", 256, 256, 3, 1, 1, 0, 2, 2, 37, _B)), ("wgrad_pos", Case("pos", 64, 128, 3, 2, 1, 0, 8, 8, 37, _B)),
    ("wgrad2", Case("ksplit", 16, 16, 1, 1, 0, 0, 32, 32, 1, _BF)), ("wgrad2", Case("nine", 64, 64, 3, 1, 1, 0, 8, 8, 7, _BF)),
    ("wgrad2", Case("sixteen", 64, 32, 4, 2, 1, 1, 8, 8, 5, _BF)), ("wgrad2", Case("nonsq", 32, 32, 3, 1, 1, 0, 16, 32, 1, _BF)),
    ("wgrad", Case("fallback", 48, 48, 3, 1, 1, 0, 8, 8, 5, _BF)), ("wgrad", Case("fallback", 32, 8, 4, 2, 1, 1, 8, 8, 5, _BF)),
]
PAIR = Case("pair", 32, 32, 3, 2, 1, 0, 32, 32, 2, _B)
PAIR_SC = PAIR._replace(k=1, p=0)
PARAMS = [pytest.param(fam, c, dt, pro, id=f"{case_id(c)}-{dt}-{'pro' if pro else 'plain'}") for fam, c in CASES for dt in c.dts for pro in (False, True)]


def p_grid(c):
    """The small side's map (the K axis of the weight gradient is N x this): x for a ConvTranspose2d, dy for a Conv2d."""
    return (c.H, c.W) if c.tr else out_hw(c)


def K_of(c):
    hp, wp = p_grid(c)
    return c.N * hp * wp


def nparts_bound(fam, c, dt):
    """Partial images of the launch (an upper bound), from the launchers' grid rules: see the docstring."""
    if fam == "wgrad_stream":
        hp = p_grid(c)[0]
        nunits = c.N * (hp // 16 if hp % 16 == 0 else 1)
        kind4 = not c.tr and c.s == 2
        gx, nw = (768, 2) if kind4 else (512, 4)
        while gx > 8 and gx * nw > nunits:
            gx -= 8
        return gx
    if fam == "wgrad_pos":
        return -(-c.N // 32)
    if fam == "wgrad2":
        return 176
    return -(-K_of(c) // (64 if dt == "bf16" else 32))


def reduce_err(parts, lanes=8):
    """wgrad_reduce_kernel<LANES>'s walk on parts [nb, F]: RG = 256 / LANES row groups, thread (rg, l) adds parts rg, rg + RG, ... into four
    accumulators while four are left, the rest into the first; (s0 + s1) + (s2 + s3); binary tree over the row groups.  -> (sum, error bound).
    lanes = 8 is wgrad_reduce_err of test_upblock_ops_f64_gpu.py (asserted below)."""
    nb, F_ = parts.shape
    RG = 256 // lanes
    acc = parts.new_zeros(RG, 4, F_)
    e = parts.new_zeros(F_)
    for rg in range(RG):
        p = rg
        while p + 3 * RG < nb:
            for k in range(4):
                acc[rg, k] += parts[p + k * RG]
                e += acc[rg, k].abs()
            p += 4 * RG
        while p < nb:
            acc[rg, 0] += parts[p]
            e += acc[rg, 0].abs()
            p += RG
    a, b = acc[:, 0] + acc[:, 1], acc[:, 2] + acc[:, 3]
    s = a + b
    e += a.abs().sum(0) + b.abs().sum(0) + s.abs().sum(0)
    st = RG // 2
    while st >= 1:
        s = s[:st] + s[st:2 * st]
        e += s.abs().sum(0)
        st //= 2
    return s[0], SLOP * U * e


def reduce_lanes(wsize):
    """launch_wgrad_reduce: elements per block 256 .. 32, aiming at >= 256 blocks."""
    lanes = 64
    while lanes > 8 and wsize // (4 * lanes) < 256:
        lanes >>= 1
    return lanes


def bn_pair_c(g, mag):
    """bn_pair of test_upblock_ops_f64_gpu.py (written for its 16 channels) for any channel count."""
    n = mag.numel()
    return sgn(g, n) * (0.5 + torch.rand(n, generator=g)) / mag, torch.randn(n, generator=g) * 0.5


def make_case(c, dt, pro, second=False):
    g = torch.Generator().manual_seed(LAT._seed(c, "relu" if pro else "none", (1 << 26) + DTS.index(dt)))
    r = lambda t: t.to(TDT[dt]).float()
    lo = math.log10(0.25)
    mx, my = span(g, c.Cin, lo, -lo), span(g, c.Cout, lo, -lo)
    Ho, Wo = out_hw(c)
    t = dict(x=r(torch.randn(c.N, c.Cin, c.H, c.W, generator=g) * mx.view(1, -1, 1, 1)),
             dy=r(torch.randn(c.N, c.Cout, Ho, Wo, generator=g) * my.view(1, -1, 1, 1)), old=torch.randn(w_shape(c), generator=g))
    t["old"] = torch.where(t["old"] == 0, torch.ones_like(t["old"]), t["old"])
    t["ps"], t["pb"] = bn_pair_c(g, mx) if pro else (None, None)
    if second:
        t["dys"] = r(torch.randn(c.N, c.Cout, Ho, Wo, generator=g) * my.view(1, -1, 1, 1))
        t["olds"] = torch.randn(c.Cout, c.Cin, 1, 1, generator=g)
    assert bool((t["old"] != 0).all())
    return t


def reference(c, dt, a, dy, old, nparts):
    """(target T = dw_old + Rq's gradient, bound on |device - T|, A / K) for the operand a = prologue(x, ...) (value, its bound) and dy."""
    d = lambda v: v.double()
    K = K_of(c)
    grad = wgrad_ref(a.v, d(dy), c)
    A = wgrad_ref(a.v.abs(), d(dy).abs(), c)
    flip = wgrad_ref(a.e, d(dy).abs(), c)
    chain = (K + 32 * nparts) if dt == "bf16" else (K + 1 + nparts)
    e = flip + SLOP * U * (chain + nparts - 1) * A
    T = d(old) + grad
    return T, e + SLOP * U * (T.abs() + e), A / K


def operand(t, dt):
    return prologue(t["x"], t["ps"], t["pb"], dt == "bf16")


def r64(c, t):
    x = t["x"].double()
    a = x if t["ps"] is None else (x * t["ps"].double().view(1, -1, 1, 1) + t["pb"].double().view(1, -1, 1, 1)).clamp_min(0)
    return t["old"].double() + wgrad_ref(a, t["dy"].double(), c)


def family_of(c, dt):
    """The weight gradient's launcher family as the lattice file's census pins it, by geometry (N aside)."""
    geo = lambda q: (q.Cin, q.Cout, q.k, q.s, q.p, q.tr, q.H, q.W)
    fams = {LAT.LAUNCHES[case_id(q)][dt]["wgrad"][0] for q in LAT.CASES if geo(q) == geo(c) and dt in q.dts}
    assert len(fams) == 1, (case_id(c), dt, fams)
    return fams.pop()


# ================================================================ CPU self-checks
def test_cases_reach_their_families_and_bounds_are_sharp():
    seen = collections.Counter()
    for fam, c in CASES:
        for dt in c.dts:
            assert family_of(c, dt) == fam, (case_id(c), dt, family_of(c, dt), fam)
            seen[(fam, dt)] += 1
            K, nparts = K_of(c), nparts_bound(fam, c, dt)
            assert K <= (1024 if fam == "wgrad2" else 2048) and nparts >= 1, (case_id(c), K, nparts)
            for pro in (False, True):
                t = make_case(c, dt, pro)
                T, bound, unit = reference(c, dt, operand(t, dt), t["dy"], t["old"], nparts)
                assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all()), case_id(c)
                sharp = float((bound / unit).median())
                print(f"SHARP {case_id(c)} {dt} pro={pro}: K {K} nparts <= {nparts} median bound / (A / K) {sharp:.3f}; |Rq - R64| max {float((T - r64(c, t)).abs().max()):.3e}")
                assert sharp < 1, ("one lost average product would pass", case_id(c), dt, pro, sharp)
    assert {("wgrad2", "bf16"), ("wgrad2", "f32"), ("wgrad", "bf16"), ("wgrad", "f32"), ("wgrad_stream", "bf16"), ("wgrad_pos", "bf16")} <= set(seen)
    assert family_of(PAIR, "bf16") == "wgrad_stream"
    for cc in (PAIR, PAIR_SC):
        t = make_case(PAIR, "bf16", True, second=True)
        dy, old = (t["dy"], t["old"]) if cc is PAIR else (t["dys"], t["olds"])
        T, bound, unit = reference(cc, "bf16", operand(t, "bf16"), dy, old, nparts_bound("wgrad_stream", PAIR, "bf16"))
        assert float((bound / unit).median()) < 1, cc


def test_reference_is_autograd():
    for fam, c in CASES + [("pair", PAIR), ("pair", PAIR_SC)]:
        t = make_case(c, "f32", True)
        x = t["x"].double()
        a = (x * t["ps"].double().view(1, -1, 1, 1) + t["pb"].double().view(1, -1, 1, 1)).clamp_min(0)
        w = torch.zeros(w_shape(c), dtype=F64, requires_grad=True)
        (LAT.conv_ref(a, w, c) * t["dy"].double()).sum().backward()
        ours = r64(c, t)
        assert float((ours - (t["old"].double() + w.grad)).abs().max()) <= 1e-12 * float(ours.abs().max()), case_id(c)
        # Rq of f32 mode is R64 (the f32 evaluation of the prologue is inside the bound); of bf16 mode at most the operand's half ulp away
        T, bound, _ = reference(c, "f32", operand(t, "f32"), t["dy"], t["old"], 1)
        assert float((T - ours).abs().max()) <= 1e-12 * float(ours.abs().max()), case_id(c)


def _fails(dev, T, bound):
    return bool((_ratio((dev - T).abs(), bound) > 1).any())


def test_mutants_fail_the_gate():
    """The gate applied to a deliberately wrong 'device' result must fail; to Rq itself it passes."""
    for fam, c in CASES:
        for dt in c.dts:
            t = make_case(c, dt, True)
            a = operand(t, dt)
            T, bound, _ = reference(c, dt, a, t["dy"], t["old"], nparts_bound(fam, c, dt))
            assert not _fails(T, T, bound)
            assert not _fails(T.float().double(), T, bound), ("the f32 rounding of Rq itself fails", case_id(c), dt)
            # `=` for `+=`
            assert _fails(T - t["old"].double(), T, bound), ("dW = passes", case_id(c), dt)
            # one pixel's contribution removed (the K axis' pixel: of x for a ConvTranspose2d, of dy for a Conv2d)
            av, dy = a.v.clone(), t["dy"].double().clone()
            (av if c.tr else dy)[c.N - 1, :, 1, 0] = 0
            assert _fails(t["old"].double() + wgrad_ref(av, dy, c), T, bound), ("a lost pixel passes", case_id(c), dt)
            if c.H != c.W:                                                  # kh and kw swapped
                assert _fails(t["old"].double() + wgrad_ref(a.v, t["dy"].double(), c).transpose(-1, -2), T, bound), ("swapped taps pass", case_id(c), dt)
            if not c.tr and c.p > 0:                                        # the prologue applied to the zero padding (x is the padded side)
                xp = F.pad(t["x"].double(), (c.p,) * 4)
                ap = prologue(xp, t["ps"], t["pb"], dt == "bf16").v
                wrong = torch.nn.grad.conv2d_weight(ap, w_shape(c), t["dy"].double(), stride=c.s, padding=0)
                assert _fails(t["old"].double() + wrong, T, bound), ("a prologue'd padding passes", case_id(c), dt)
    assert any(c.H != c.W for _, c in CASES) and any(not c.tr and c.p > 0 for _, c in CASES)


def test_reduce_model_for_every_lanes():
    """reduce_err at LANES = 8 is the sibling file's wgrad_reduce_err.  For every LANES the walk, carried out in f32, lands within the modelled
    bound AND within the order-free majorant u (nparts - 1) sum |parts| that the gates use (the model also counts the exact additions onto
    empty accumulators, so it is the larger of the two at few parts); launch_wgrad_reduce's choice of LANES by image size."""
    g = torch.Generator().manual_seed(3)
    for nb in (1, 2, 8, 31, 37, 176, 512):
        parts = torch.randn(nb, 64, generator=g).double()                   # f32 values, as the partial images are
        s0, e0 = wgrad_reduce_err(parts.clone())
        s8, e8 = reduce_err(parts.clone(), 8)
        assert torch.equal(s0, s8) and torch.equal(e0, e8), nb
        for lanes in (8, 16, 32, 64):
            s, e = reduce_err(parts.clone(), lanes)
            assert float((s - parts.sum(0)).abs().max()) < 1e-12 * nb
            walked = reduce_err(parts.float(), lanes)[0].double()           # the same walk in f32 arithmetic
            err = (walked - s).abs()
            assert bool((err <= e).all()), (nb, lanes)
            assert bool((err <= SLOP * U * max(nb - 1, 0) * parts.abs().sum(0)).all()), (nb, lanes)
    assert [reduce_lanes(n) for n in (256, 4096, 9216, 32768, 65536, 589824)] == [8, 8, 8, 32, 64, 64]


# ================================================================ GPU
def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(TDT[dt])


@gpu
@pytest.mark.parametrize("fam,c,dt,pro", PARAMS)
def test_conv_wgrad_f64(fam, c, dt, pro):
    t = make_case(c, dt, pro)
    what = f"{case_id(c)} {dt} {'prologue' if pro else 'plain'}"
    L = _L()
    D = Dev()
    x, dy, dw = D.put("x", nhwc(t["x"], dt)), D.put("dy", nhwc(t["dy"], dt)), D.put("dw", t["old"])
    ps, pb = D.put("ps", t["ps"]), D.put("pb", t["pb"])
    ws = wscratch()
    L.check(L.lib().mmvae_conv2d_wgrad(DTI[dt], c.tr, P(x), P(dy), P(dw), c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.s, c.p, P(ps), P(pb), 1, ws.ptr(), stream()), what)
    torch.cuda.synchronize()
    D.check(what)
    assert ws.intact(), what
    got = dw.double().cpu()
    assert bool(torch.isfinite(got).all()), ("non-finite dw", what)
    T, bound, _ = reference(c, dt, operand(t, dt), t["dy"], t["old"], nparts_bound(fam, c, dt))
    gate(f"{fam}_{dt}", _ratio((got - T).abs(), bound), what, lambda: (T - r64(c, t)).abs())


@gpu
@pytest.mark.parametrize("pro", (False, True), ids=("plain", "pro"))
def test_conv_wgrad_pair_f64(pro):
    c = PAIR
    t = make_case(c, "bf16", pro, second=True)
    what = f"pair N{c.N} {'prologue' if pro else 'plain'}"
    L = _L()
    D = Dev()
    x, dy, dys = D.put("x", nhwc(t["x"], "bf16")), D.put("dy", nhwc(t["dy"], "bf16")), D.put("dys", nhwc(t["dys"], "bf16"))
    dw, dws = D.put("dw", t["old"]), D.put("dws", t["olds"])
    ps, pb = D.put("ps", t["ps"]), D.put("pb", t["pb"])
    ws = wscratch()
    L.check(L.lib().mmvae_conv2d_wgrad_pair(1, P(x), P(dy), P(dys), P(dw), P(dws), c.N, 32, 32, 32, 32, P(ps), P(pb), 1, ws.ptr(), stream()), what)
    torch.cuda.synchronize()
    D.check(what)
    assert ws.intact(), what
    a, nparts = operand(t, "bf16"), nparts_bound("wgrad_stream", c, "bf16")
    for name, cc, out, dyy, old in (("dw", PAIR, dw, t["dy"], t["old"]), ("dw_sc", PAIR_SC, dws, t["dys"], t["olds"])):
        T, bound, _ = reference(cc, "bf16", a, dyy, old, nparts)
        gate(f"pair_{name}", _ratio((out.double().cpu() - T).abs(), bound), f"{what} {name}")


# ================================================================ GPU: census of this file's own cases (keep last)
def census_plan():
    return [(case_id(c), dt, int(pro), fam) for fam, c in CASES for dt in c.dts for pro in (False, True)] + [("pair", "bf16", 1, "pair")]


def census_child():
    """This file's cases once each (zero operands), an 8-element mmvae_convert in front of each: their N are not the lattice file's."""
    lib = _L().lib()
    a, b = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    ws = torch.zeros(LAT.WSCRATCH_BYTES, dtype=torch.uint8, device="cuda")
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    by_id = {case_id(c): c for _, c in CASES}
    done = []
    for label, dt, pro, fam in census_plan():
        assert lib.mmvae_convert(0, 0, P(a), P(b), 8, stream()) == 0
        tdt = TDT[dt]
        if fam == "pair":
            c = PAIR
            rc = lib.mmvae_conv2d_wgrad_pair(1, P(z((c.N, 32, 32, 32), tdt)), P(z((c.N, 16, 16, 32), tdt)), P(z((c.N, 16, 16, 32), tdt)), P(z((32, 32, 3, 3))),
                                             P(z((32, 32, 1, 1))), c.N, 32, 32, 32, 32, P(z(32)), P(z(32)), 1, ws.data_ptr(), stream())
        else:
            c = by_id[label]
            Ho, Wo = out_hw(c)
            ps, pb = (z(c.Cin), z(c.Cin)) if pro else (None, None)
            rc = LAT.call_wgrad(lib, c, dt, 1, z((c.N, c.H, c.W, c.Cin), tdt), z((c.N, Ho, Wo, c.Cout), tdt), z(w_shape(c)), ps, pb, ws.data_ptr())
        torch.cuda.synchronize()
        done.append([label, dt, pro, rc])
    print("CENSUS_PLAN " + LAT.json.dumps(done))


@gpu
def test_launch_census(tmp_path):
    """The family a case's bound is built for (nparts_bound) is the family the device runs it on, at this file's own N."""
    done, segs = LAT.census_segments(tmp_path, os.path.abspath(__file__))
    plan = census_plan()
    assert [d[:3] for d in done] == [list(p[:3]) for p in plan]
    wrong = []
    for (label, dt, pro, rc), (_, _, _, fam), seg in zip(done, plan, segs):
        seg = tuple(n for n in seg if n not in ("pack", "pack_multi"))
        print(f"CENSUS {label} {dt} pro={pro} rc={rc}: {' '.join(seg)}")
        want = ("wgrad_stream", "wgrad_reduce", "wgrad_reduce") if fam == "pair" else (fam, "wgrad_reduce")
        if rc != 0 or seg != want:
            wrong.append((label, dt, pro, rc, seg, want))
    assert not wrong, wrong


if __name__ == "__main__":
    if sys.argv[1:] == ["--census-child"]:
        census_child()
        sys.exit(0)
    for fn in (test_cases_reach_their_families_and_bounds_are_sharp, test_reference_is_autograd, test_mutants_fail_the_gate, test_reduce_model_for_every_lanes):
        fn()
        print("ok", fn.__name__)
