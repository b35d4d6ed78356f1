"""Float64 per-slice parity of the convolution data gradients as the network's backward pass launches them, through mmvae_conv2d_dgrad_ex:
plain, accumulating onto a buffer that already holds the shortcut's share (the identity blocks of the deeper variant), and with a second
source (the 1x1 branch of a residual join: encoder downsample.0 beside conv1, decoder conv1 beside upsample.0), merged into the patch-tile
kernel or run as a second, accumulating launch (launch_x2_separately, csrc/conv_gemm.hip).  Conventions of test_upblock_ops_f64_gpu.py,
whose helpers are imported: every device buffer is a window of its documented size inside a pattern-filled allocation, dx of a
non-accumulating call starts NaN-filled, gates are per slice with bounds built from term magnitudes, nothing is excluded.

References, float64, built on the CPU from the exact tensors handed to the device (dy, dy2, dx_old already rounded to the storage type; the
weights are handed over in f32 and rounded by the packing kernels):
  R64  conv_transpose2d / conv2d of dy with the weights + dx_old + the second source's term, written with its phase placement
       (dx[:, :, ::s, ::s] += dy2 (x) w2 for the stride-s 1x1 conv of the encoder, dx += dy2 (x) w2 on dx's own grid in the decoder);
  Rq   the same with a rounding wherever the code rounds (read off the .hip files):
       - weights to bf16 in bf16 mode (pack_kernel: Elem<bf16_t>::store, nearest-even), f32 weights as they are;
       - one f32 accumulator per output element in every kernel (gather_gemm, gather3, patch_conv, deep2_conv, pos_conv): no split K;
       - a launch's output to the storage type; an accumulating launch adds the stored value in f32 before that rounding (store4 /
         dstore4 / dstore8 / pstore4 with acc);
       - patch_conv_kernel's UNIFORM epilogue (whole rows, power-of-two width >= 16: every patch-tile case here) stages the result in LDS
         in the storage type and the accumulating form adds dx_old to the STAGED value: bf16 `dx +=` there is rbf(rbf(M) + dx_old), two
         roundings (conv_patch.inc, `if constexpr (ACC)` behind the LDS read-back); the general epilogue and every other kernel have one;
       - the two-launch second source: bf16 dx is stored after the main launch, re-read, added to and stored again (two roundings); the
         merged patch-tile launch continues the same accumulator over the second source's K range (one rounding); f32 dx has none.
The device is gated against Rq; |Rq - R64| is printed in failure messages and gates nothing.  Which numerics a case has (merged or two
launches, staged accumulate) follows from the launcher families in LAUNCHES below, which the census test pins to what the device runs.

Bounds, units of u = 2^-24, derived:
  * MFMA K-slab rule.  bf16: 32 roundings per K = 32 slab of |C| + sum |products| (products exact).  f32 (v_mfma_f32_16x16x4f32 in every
    kernel): 4 roundings per K = 4 slab of the same, plus u per product.  The five kernels walk taps and channel chunks in different
    orders, so the order-free majorant is used: |C| + sum |products of the slab| <= A = sum |all products of the element|, hence
    32 u nslabs A (bf16, nslabs = taps x ceil(channels / 32)) and u (K + 1) A (f32, K = taps x channels); taps = the most any output
    element has (ceil(k / s)^2 for the Conv2d data gradient, k^2 for the ConvTranspose2d one).  The merged second source extends the same
    chain: slabs and A of both sources together.
  * u (|result| + incoming bound) for the f32 `+=`.
  * a bf16 store: half a bf16 ulp on top of the incoming bound; at the FIRST store of a two-store form the midpoint rule (rbf_e): Rq's
    rounding and bound 0 unless a rounding midpoint lies within the incoming bound, then incoming bound + one bf16 step.
  * SLOP = 1.01.
Slices: per (image, channel) x {border ring, interior}; on 2x2 and 4x4 maps per (image, channel, position).

Contracts asserted besides the gates: accumulate onto zeros gives the bits of the plain call (every case: a form's plain and accumulating
launches are the same kernel family, and mmvae_conv2d_dgrad_ex has no stream form: see the census); where the second source takes two launches the call gives the bits of the plain call followed by an accumulating call of the 1x1 layer alone;
two runs give the same bits; guard bytes intact with the scratch at MMVAE_DGRAD_EX_SCRATCH_BYTES; the refusals return MMVAE_ERR_ARG
before anything is enqueued.

Census (last test): one child process with MMVAE_LAUNCH_STATS / MMVAE_LAUNCH_SEQ runs every case and form once, an 8-element mmvae_convert
between them, and the launcher families of every segment must be LAUNCHES' (packing launches left out).  mmvae_conv2d_dgrad runs on two
cases in the same child and must show what it launched before it became a call of the new entry point: pos_conv for the 64 -> 128 encoder
conv, conv3_stream for the bf16 32 -> 32 3x3 on 16x16 maps (the one shape it keeps for itself; the network reaches that kernel through
launch_conv3_stream_bwd, never through run_up, so the new entry point runs patch_conv there).

Launcher families the device showed (LAUNCHES, all N): bf16 -- patch_conv for the 32- and 16-channel layers (second source merged: one
launch), deep2_conv for 32 -> 64 @ 16, 64 -> 32 @ 8 and 64 @ 8x8, pos_conv for everything on 2x2 / 4x4 maps and for 64 -> 128 @ 8 (second
source: two launches each).  f32 -- deep2_conv where bf16 has pos_conv or deep2_conv;
gather_gemm for 32 -> 16 @ 16 (ConvT) and the 32-channel 3x3 on 16x16 (weights + patch exceed the patch-tile kernel's 60 KB of LDS, 16 x 16 /
9 x 32 values a tap row exceed gather3's 160); patch_conv for 32 -> 32 @ 32, 16 -> 16 @ 32 and the 16-channel 1x1, but with a second source
TWO launches (f32 operands are twice as wide: the merged form's second-source weights and tile no longer fit the 60 KB), the second an
accumulating patch_conv.  So the merged second source is a bf16 form; gather3 is reached by none of the joins at these sizes.

Measured on the MI355X: the whole file, 62 GPU tests, in 5.9 s (the census child 2.7 s of it); the CPU self-checks in 4 s.  Worst err / bound
per case family (plain / accumulate / second source):
  encoder joins     bf16 0.996 / 1.000 / 0.998    f32 0.038 / 0.056 / 0.052
  decoder joins     bf16 0.974 / 1.000 / 0.999    f32 0.020 / 0.020 / 0.020
  3x3 s1 identity   bf16 0.982 / 1.000            f32 0.016 / 0.016
  1x1 s1 identity   bf16 0.999 / 1.000            f32 0.226 / 0.242
  odd map (7x7)     bf16 0.991                    f32 0.029
bf16 outputs reach ~1 on rounding ties (the half ulp is then the whole bound), exactly 1 where dx_old + the re-read value is a tie itself; f32
outputs sit lower by construction (the order-free majorant of the slab rule), highest where K is smallest (16 products: the bound is 17 u A).
"""
import collections
import ctypes
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

from test_upblock_ops_f64_gpu import (DTI, ERR_ARG, F64, SLOP, TDT, U, Dev, P, _L, _ratio, gate, gpu, half_ulp_bf16, plane_slices, rbf,  # noqa: E402
                                      rbf_e, same_bits, stream)

Case = collections.namedtuple("Case", "fam tr Cin Cout k s p H N")


def _cases():
    out = []
    for Cin, Cout, H, Ns in ((32, 32, 32, (1, 3)), (32, 64, 16, (1, 5)), (64, 128, 8, (1, 37)), (128, 256, 4, (1, 37))):
        out += [Case("enc", 0, Cin, Cout, 3, 2, 1, H, N) for N in Ns]                 # conv1 (3x3 s2) + downsample.0 (1x1 s2)
    for Cin, Cout, H, Ns in ((128, 128, 2, (1, 37)), (128, 64, 4, (1, 37)), (64, 32, 8, (1, 5)), (32, 16, 16, (1, 3)), (16, 16, 32, (1, 3))):
        out += [Case("dec", 1, Cin, Cout, 4, 2, 1, H, N) for N in Ns]                 # upsample.0 (ConvT k4 s2) + conv1 (1x1)
    for C, H, Ns in ((32, 16, (1, 5)), (64, 8, (1, 37)), (128, 4, (1, 37)), (256, 2, (1, 37))):
        out += [Case("acc3", 0, C, C, 3, 1, 1, H, N) for N in Ns]                     # identity blocks: 3x3 s1
    for C, H, Ns in ((128, 2, (1, 37)), (16, 32, (1, 3))):
        out += [Case("acc1", 0, C, C, 1, 1, 0, H, N) for N in Ns]                     # identity blocks: 1x1 s1
    return out


CASES = _cases()
DTS = ("bf16", "f32")


def key(c):
    return f"{c.fam} {c.Cin}->{c.Cout}@{c.H}"


def case_id(c):
    return f"{c.fam}-{c.Cin}-{c.Cout}-H{c.H}-N{c.N}"


def forms(c):
    return ("plain", "acc", "x2") if c.fam in ("enc", "dec") else ("plain", "acc")


# Launcher families per case (any N), storage type and form, in launch order -- what launch_gather_gemm's dispatch gives; the census test
# asserts it on the device.  In bf16 the 64 -> 128 and 128 -> 256 encoder joins and the 128 -> 128 and 128 -> 64 decoder joins are two
# pos_conv launches with a second source (the only launches of POS_CASE(1, 2, 0, true, 4, 8, 128, 1) / (1, 2, 0, true, 2, 4, 256, 2)).
_P, _Q, _D, _G3, _GG, _S3 = "patch_conv", "pos_conv", "deep2_conv", "gather3", "gather_gemm", "conv3_stream"


def _row(plain, acc=None, x2=None):
    r = {"plain": tuple(plain), "acc": tuple(acc if acc is not None else plain)}
    if x2 is not None:
        r["x2"] = tuple(x2)
    return r


LAUNCHES = {
    "enc 32->32@32": {"bf16": _row([_P], x2=[_P]), "f32": _row([_P], x2=[_P, _P])},
    "enc 32->64@16": {"bf16": _row([_D], x2=[_D, _D]), "f32": _row([_D], x2=[_D, _D])},
    "enc 64->128@8": {"bf16": _row([_Q], x2=[_Q, _Q]), "f32": _row([_D], x2=[_D, _D])},
    "enc 128->256@4": {"bf16": _row([_Q], x2=[_Q, _Q]), "f32": _row([_D], x2=[_D, _D])},
    "dec 128->128@2": {"bf16": _row([_Q], x2=[_Q, _Q]), "f32": _row([_D], x2=[_D, _D])},
    "dec 128->64@4": {"bf16": _row([_Q], x2=[_Q, _Q]), "f32": _row([_D], x2=[_D, _D])},
    "dec 64->32@8": {"bf16": _row([_D], x2=[_D, _D]), "f32": _row([_D], x2=[_D, _D])},
    "dec 32->16@16": {"bf16": _row([_P], x2=[_P]), "f32": _row([_GG], x2=[_GG, _P])},
    "dec 16->16@32": {"bf16": _row([_P], x2=[_P]), "f32": _row([_P], x2=[_P, _P])},
    "acc3 32->32@16": {"bf16": _row([_P]), "f32": _row([_GG])},
    "acc3 64->64@8": {"bf16": _row([_D]), "f32": _row([_D])},
    "acc3 128->128@4": {"bf16": _row([_Q]), "f32": _row([_D])},
    "acc3 256->256@2": {"bf16": _row([_Q]), "f32": _row([_D])},
    "acc1 128->128@2": {"bf16": _row([_Q]), "f32": _row([_D])},
    "acc1 16->16@32": {"bf16": _row([_P]), "f32": _row([_P])},
}
# mmvae_conv2d_dgrad, bf16: the launch of the plain form, but for the one shape it has always run as a per-wave stream
DGRAD_CENSUS = ((Case("enc", 0, 64, 128, 3, 2, 1, 8, 37), (_Q,)), (Case("acc3", 0, 32, 32, 3, 1, 1, 16, 5), (_S3,)))


# ================================================================ geometry and the documented scratch size
def out_size(c):
    return (c.H - 1) * c.s - 2 * c.p + c.k if c.tr else (c.H + 2 * c.p - c.k) // c.s + 1


def w_shape(c):
    return (c.Cin, c.Cout, c.k, c.k) if c.tr else (c.Cout, c.Cin, c.k, c.k)


def second_grid(c):
    """Map size of dy2: the main layer's small side for the encoder's stride-s 1x1 conv, dx's grid for the decoder's stride-1 one."""
    return c.H if c.tr else out_size(c)


def w2_offset(numel_w, es):
    return (numel_w * es + 255) // 256 * 256                                # MMVAE_DGRAD_EX_W2_OFFSET


def scratch_bytes(numel_w, numel_w2, es):
    return w2_offset(numel_w, es) + numel_w2 * es if numel_w2 > 0 else numel_w * es     # MMVAE_DGRAD_EX_SCRATCH_BYTES


def patch_uniform(c):
    """try_patch's uni_ok for the data-gradient launch of case c (conv_gemm.hip): whole rows of a power-of-two width >= 16, >= 128 q pixels,
    every stride phase present and full-size, output channels a multiple of 16.  Then patch_conv_kernel stages its results in LDS."""
    q = c.H if c.tr else c.H // c.s
    every_phase = c.tr or (c.k >= c.s and c.H % c.s == 0)
    return q >= 16 and q & (q - 1) == 0 and q * q >= 128 and every_phase and c.Cin % 16 == 0


def numerics(c, dt, form):
    fam = LAUNCHES[key(c)][dt][form]
    if form == "x2":
        return "merged" if len(fam) == 1 else "two"
    if form == "acc":
        return "staged" if dt == "bf16" and fam == (_P,) and patch_uniform(c) else "one"
    return "one"


# ================================================================ float64 references and bounds
def main_term(dy, w, c):
    """The main layer's data gradient on NCHW float64 tensors."""
    if c.tr:
        return F.conv2d(dy, w, stride=c.s, padding=c.p)
    opad = c.H - ((dy.shape[2] - 1) * c.s - 2 * c.p + c.k)
    return F.conv_transpose2d(dy, w, stride=c.s, padding=c.p, output_padding=opad)


def second_term(dy2, w2, c):
    """The 1x1 conv's data gradient, placed by hand: every s-th pixel (stride phase (0, 0)) beside a Conv2d, dx's own grid beside a ConvT."""
    t = torch.einsum("nchw,ci->nihw", dy2, w2[:, :, 0, 0])
    if c.tr:
        return t
    out = t.new_zeros(t.shape[0], t.shape[1], c.H, c.H)
    out[:, :, ::c.s, ::c.s] = t
    return out


def chain_err(A, ntaps, kc, dt):
    """One MFMA accumulator over ntaps x kc products of absolute sum A (order-free majorant of the K-slab rule, see the docstring)."""
    if dt == "bf16":
        return SLOP * 32 * U * (ntaps * -(-kc // 32)) * A
    return SLOP * U * (ntaps * kc + 1) * A


def main_taps(c):
    return c.k * c.k if c.tr else (-(-c.k // c.s)) ** 2


def two_round(m, s):
    """bf16 dx of the two-launch form and of the staged accumulate: stored, re-read, added to, stored again."""
    return rbf(rbf(m) + s)


def make_case(c, dt):
    g = torch.Generator().manual_seed(((c.Cin * 257 + c.Cout) * 64 + c.H) * 64 + c.N + 7919 * c.k + (1 << 20) * c.tr)
    Ho, H2 = out_size(c), second_grid(c)
    r = lambda t: t.to(TDT[dt]).float()
    span = lambda n: torch.exp2(torch.rand(n, generator=g) * 4 - 2).view(1, -1, 1, 1)
    t = collections.namedtuple("T", "c dt dy w old dy2 w2")
    dy = r(torch.randn(c.N, c.Cout, Ho, Ho, generator=g) * span(c.Cout))
    w = torch.randn(w_shape(c), generator=g) / (c.Cout * main_taps(c)) ** 0.5
    old = r(torch.randn(c.N, c.Cin, c.H, c.H, generator=g) * span(c.Cin))
    dy2 = r(torch.randn(c.N, c.Cout, H2, H2, generator=g) * span(c.Cout))
    w2 = torch.randn(c.Cout, c.Cin, 1, 1, generator=g) / c.Cout ** 0.5
    return t(c, dt, dy, w, old, dy2, w2)


def reference(t, form, how):
    """(target in front of the last store, bound on |device - target|, Rq, R64), NCHW float64."""
    c, dt = t.c, t.dt
    q = dt == "bf16"
    d = lambda x: x.double()
    wq, w2q = (rbf(d(t.w)), rbf(d(t.w2))) if q else (d(t.w), d(t.w2))
    M, A1 = main_term(d(t.dy), wq, c), main_term(d(t.dy).abs(), wq.abs(), c)
    r64 = main_term(d(t.dy), d(t.w), c)
    nt, kc = main_taps(c), c.Cout
    E1 = chain_err(A1, nt, kc, dt)
    if form == "plain":
        T, e = M, E1
    elif form == "acc":
        r1, e1 = rbf_e(M, E1, q and how == "staged")
        T = r1 + d(t.old)
        e = e1 + SLOP * U * (T.abs() + e1)
        r64 = r64 + d(t.old)
    else:
        S, A2 = second_term(d(t.dy2), w2q, c), second_term(d(t.dy2).abs(), w2q.abs(), c)
        r64 = r64 + second_term(d(t.dy2), d(t.w2), c)
        if how == "merged":
            T = M + S
            slabs = nt * -(-kc // 32) + -(-c.Cout // 32)
            e = SLOP * 32 * U * slabs * (A1 + A2) if q else SLOP * U * (nt * kc + c.Cout + 1) * (A1 + A2)
        else:
            r1, e1 = rbf_e(M, E1, q)
            E2 = chain_err(A2, 1, c.Cout, dt)
            T = r1 + S
            e = e1 + E2 + SLOP * U * (T.abs() + e1 + E2)
    bound = e + half_ulp_bf16(T.abs() + e) if q else e
    return T, bound, (rbf(T) if q else T), r64


def slices(ratio):
    """[N, C, H, W] -> per (image, channel) x {border ring, interior}; per position on 2x2 and 4x4 maps."""
    return ratio.flatten(2) if ratio.shape[-1] <= 4 else plane_slices(ratio)


# ================================================================ device side
def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(TDT[dt])


class Run:
    """A case's inputs on the device (guarded windows) and its forms as calls of mmvae_conv2d_dgrad_ex."""

    def __init__(self, t, guarded=True):
        self.t, c, dt = t, t.c, t.dt
        self.L = _L()
        self.lib = self.L.lib()
        self.D = Dev()
        put = self.D.put if guarded else (lambda name, x: x.cuda())
        self.dy, self.dy2 = put("dy", nhwc(t.dy, dt)), put("dy2", nhwc(t.dy2, dt))
        self.w, self.w2 = put("w", t.w), put("w2", t.w2)
        es = 2 if dt == "bf16" else 4
        self.sc = self.D.scratch("scratch", scratch_bytes(t.w.numel(), t.w2.numel(), es))
        self.sc1 = self.D.scratch("scratch1", scratch_bytes(t.w2.numel(), 0, es))
        self.n = 0

    def out(self, init=None):
        """A guarded dx window: NaN-filled (every byte 0xFF is a NaN in both storage types), or holding `init`."""
        c = self.t.c
        self.n += 1
        if init is None:
            return self.D.put(f"dx{self.n}", ((c.N, c.H, c.H, c.Cin), TDT[self.t.dt]), 0xFF)
        return self.D.put(f"dx{self.n}", nhwc(init, self.t.dt))

    def call(self, form, dx, check=True):
        c = self.t.c
        x2 = form == "x2"
        rc = self.lib.mmvae_conv2d_dgrad_ex(DTI[self.t.dt], c.tr, P(self.dy), P(self.w), P(dx), c.N, c.H, c.H, c.Cin, c.Cout, c.k, c.s, c.p,
                                            1 if form == "acc" else 0, P(self.dy2) if x2 else None, P(self.w2) if x2 else None,
                                            c.Cout if x2 else 0, self.sc, stream())
        return self.L.check(rc, f"conv2d_dgrad_ex {case_id(c)} {self.t.dt} {form}") if check else rc

    def call_1x1_alone(self, dx):
        """The second source's layer on its own, accumulating: Conv2d (C2, Cin, 1, 1) with the encoder's stride / stride 1 in the decoder."""
        c = self.t.c
        rc = self.lib.mmvae_conv2d_dgrad_ex(DTI[self.t.dt], 0, P(self.dy2), P(self.w2), P(dx), c.N, c.H, c.H, c.Cin, c.Cout, 1, 1 if c.tr else c.s, 0,
                                            1, None, None, 0, self.sc1, stream())
        return self.L.check(rc, f"conv2d_dgrad_ex {case_id(c)} {self.t.dt} 1x1 alone")

    def legacy(self, dx):
        c = self.t.c
        return self.L.check(self.lib.mmvae_conv2d_dgrad(DTI[self.t.dt], c.tr, P(self.dy), P(self.w), P(dx), c.N, c.H, c.H, c.Cin, c.Cout, c.k, c.s, c.p,
                                                        self.sc, stream()), "conv2d_dgrad")


def nchw64(t):
    return t.cpu().double().permute(0, 3, 1, 2)


# ================================================================ CPU self-checks
def test_reference_is_autograd():
    """R64 as written (phase placement of the second source by hand) against torch.autograd of conv(x, W) + conv1x1(x, W2) in float64."""
    seen = set()
    for c in CASES:
        if key(c) in seen:
            continue
        seen.add(key(c))
        c = c._replace(N=2)
        t = make_case(c, "f32")
        d = lambda x: x.double()
        x = torch.zeros(c.N, c.Cin, c.H, c.H, dtype=F64, requires_grad=True)
        y = F.conv_transpose2d(x, d(t.w), stride=c.s, padding=c.p) if c.tr else F.conv2d(x, d(t.w), stride=c.s, padding=c.p)
        y2 = F.conv2d(x, d(t.w2), stride=1 if c.tr else c.s)
        assert y.shape == t.dy.shape and y2.shape == t.dy2.shape, (c, y.shape, y2.shape)
        ((y * d(t.dy)).sum() + (y2 * d(t.dy2)).sum()).backward()
        ours = main_term(d(t.dy), d(t.w), c) + second_term(d(t.dy2), d(t.w2), c)
        scale = float(x.grad.abs().max())
        assert float((ours - x.grad).abs().max()) <= 1e-13 * scale, c
        # ... and the reference() plumbing: R64 of every form, Rq of f32 = the target, bounds positive and small against the values
        for form in forms(c):
            T, b, rq, r64 = reference(t, form, numerics(c, "f32", form))
            want = main_term(d(t.dy), d(t.w), c) + (d(t.old) if form == "acc" else 0) + (second_term(d(t.dy2), d(t.w2), c) if form == "x2" else 0)
            assert torch.equal(r64, want) and torch.equal(rq, T), (c, form)
            assert float((T - r64).abs().max()) <= 1e-12 * scale and bool((b > 0).all()) and float(b.max()) < 1e-2 * scale, (c, form)
            Tb, bb, rqb, _ = reference(make_case(c, "bf16"), form, numerics(c, "bf16", form))
            # (a bound of exactly 0 is right where a re-read bf16 value cancels dx_old exactly: both roundings are then exact)
            assert bool((bb[Tb != 0] > 0).all()) and bool((bb >= 0).all()) and float((rqb - Tb).abs().max()) <= float(half_ulp_bf16(Tb).max()), (c, form)


def test_two_rounding_form_is_the_literal_two_steps():
    g = torch.Generator().manual_seed(7)
    draw = lambda: (0.5 + 3.5 * torch.rand(1 << 16, generator=g)) * (torch.randint(0, 2, (1 << 16,), generator=g) * 2 - 1)
    m = draw()                                                              # f32 in +-[0.5, 4): exact in float64
    s = draw().to(torch.bfloat16)
    first = m.to(torch.bfloat16)                                            # the first store
    f = first.float() + s.float()                                           # re-read and added in f32 ...
    assert torch.equal(f.double(), first.double() + s.double())             # ... exactly, for operands this close in magnitude
    literal = f.to(torch.bfloat16).double()                                 # the second store
    assert torch.equal(two_round(m.double(), s.double()), literal)
    once = rbf(m.double() + s.double())
    assert 0 < int((once != literal).sum()) < m.numel()                      # the single rounding is another function


def test_bound_helpers_by_hand():
    one = torch.ones(1, dtype=F64)
    assert float(chain_err(one, 4, 64, "bf16")) == SLOP * 32 * U * 8         # 4 taps x 2 slabs of 32
    assert float(chain_err(one, 4, 16, "bf16")) == SLOP * 32 * U * 4         # a 16-channel tap is still a slab
    assert float(chain_err(one, 4, 64, "f32")) == SLOP * U * 257             # 64 slabs of 4, 4 roundings each, + the products
    assert float(half_ulp_bf16(one)) == 2.0 ** -8 and float(half_ulp_bf16(one * 0.75)) == 2.0 ** -9
    # midpoint rule: bf16 neighbours of 1 are 1 and 1 + 2^-7, the midpoint is 1 + 2^-8
    near, far, e = one + 2.0 ** -8 - 2.0 ** -22, one + 2.0 ** -10, one * 2.0 ** -20
    r, b = rbf_e(near, e)
    assert float(r) == 1.0 and float(b) == 2.0 ** -20 + 2.0 ** -7
    r, b = rbf_e(far, e)
    assert float(r) == 1.0 and float(b) == 0.0
    # slices: ring and interior of an 8x8 plane, positions of a 2x2 one
    x = torch.zeros(1, 1, 8, 8, dtype=F64)
    x[0, 0, 0, 3], x[0, 0, 4, 4] = 2.0, 3.0
    assert slices(x).tolist() == [[[2.0, 3.0]]] and slices(torch.arange(4.0).view(1, 1, 2, 2)).tolist() == [[[0.0, 1.0, 2.0, 3.0]]]
    # the uniform (LDS-staged) epilogue of the patch-tile kernel: 16-wide q grids and up, not the deep layers' small maps
    uni = {key(c) for c in CASES if patch_uniform(c)}
    assert uni == {"enc 32->32@32", "dec 32->16@16", "dec 16->16@32", "acc3 32->32@16", "acc1 16->16@32"}, uni


def test_launch_table_and_scratch_formula():
    for c in CASES:
        for dt in DTS:
            row = LAUNCHES[key(c)][dt]
            assert set(row) == set(forms(c)), (key(c), dt)
            if "x2" in row:
                assert row["x2"][:1] == row["plain"] or len(row["x2"]) == 1, (key(c), dt)
    assert {key(c) for c in CASES} == set(LAUNCHES)
    bf = {k: v["bf16"] for k, v in LAUNCHES.items()}
    for k in ("enc 64->128@8", "enc 128->256@4", "dec 128->128@2", "dec 128->64@4"):
        assert bf[k]["x2"] == (_Q, _Q) and bf[k]["plain"] == (_Q,) and bf[k]["acc"] == (_Q,), k
    for k in ("enc 32->32@32", "dec 32->16@16", "dec 16->16@32"):
        assert bf[k]["x2"] == (_P,), k
    allacc = {f for v in LAUNCHES.values() for d in v.values() for f in d["acc"] + d.get("x2", ())[1:]}
    assert {_P, _Q, _D} <= allacc and allacc & {_G3, _GG}, allacc           # every family the joins reach accumulates somewhere
    src = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    flat = re.sub(r"\s+", " ", src.replace("\\\n", " "))
    assert "#define MMVAE_DGRAD_EX_W2_OFFSET(numel_w, esize) ((((size_t)(numel_w) * (esize) + 255) / 256) * 256)" in flat
    assert ("#define MMVAE_DGRAD_EX_SCRATCH_BYTES(numel_w, numel_w2, esize) ((numel_w2) > 0 ? MMVAE_DGRAD_EX_W2_OFFSET(numel_w, esize) + "
            "(size_t)(numel_w2) * (esize) : (size_t)(numel_w) * (esize))") in flat
    assert scratch_bytes(1000, 0, 2) == 2000 and scratch_bytes(1000, 10, 2) == 2048 + 20 and scratch_bytes(128, 16, 4) == 512 + 64


def test_refusals_need_no_device(pkg):
    """Every refusal returns before anything is enqueued: host buffers stand in for the device ones and stay as they are."""
    lib = _L().lib()
    buf = lambda: (ctypes.c_uint8 * 64)(*([0xA5] * 64))
    dy, w, dx, dy2, w2, sc = (buf() for _ in range(6))
    p = lambda b: ctypes.addressof(b)

    def call(tr=0, H=8, W=8, k=3, s=2, pad=1, acc=0, dy_=p(dy), w_=p(w), dx_=p(dx), dy2_=p(dy2), w2_=p(w2), C2=32, sc_=p(sc), dt=1, N=1):
        return lib.mmvae_conv2d_dgrad_ex(dt, tr, dy_, w_, dx_, N, H, W, 32, 32, k, s, pad, acc, dy2_, w2_, C2, sc_, None)

    got = {"accumulate with a second source": call(acc=1), "dy2 without w2": call(w2_=None), "w2 without dy2": call(dy2_=None),
           "odd H": call(H=7), "odd W": call(W=7), "odd H, accumulate": call(H=7, acc=1), "C2 = 0": call(C2=0),
           "dy NULL": call(dy_=None, dy2_=None, w2_=None), "weight NULL": call(w_=None, dy2_=None, w2_=None),
           "dx NULL": call(dx_=None, dy2_=None, w2_=None), "scratch NULL": call(sc_=None, dy2_=None, w2_=None),
           "N = 0": call(N=0, dy2_=None, w2_=None), "dtype 2": call(dt=2, dy2_=None, w2_=None),
           "transposed, accumulate with a second source": call(tr=1, k=4, acc=1)}
    assert all(rc == ERR_ARG for rc in got.values()), got
    assert lib.mmvae_last_error()
    assert all(bytes(b) == b"\xa5" * 64 for b in (dy, w, dx, dy2, w2, sc))


# ================================================================ GPU: the gates and the contracts
@gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_conv_join_f64(c, dt):
    t = make_case(c, dt)
    R = Run(t)
    what = f"{case_id(c)} {dt}"
    res = {}
    for form in forms(c):
        res[form] = []
        for rep in range(2):
            dx = R.out(t.old if form == "acc" else None)
            R.call(form, dx)
            res[form].append(dx)
    zero = R.out(torch.zeros_like(t.old))
    R.call("acc", zero)
    two = "x2" in res and numerics(c, dt, "x2") == "two"
    if two:
        steps = R.out()
        R.call("plain", steps)
        R.call_1x1_alone(steps)
    torch.cuda.synchronize()
    R.D.check(what)
    for form, (a, b) in res.items():
        assert same_bits(a, b), ("not bit-reproducible", what, form)
        got = nchw64(a)
        assert bool(torch.isfinite(got).all()), ("non-finite dx", what, form)
        T, bound, rq, r64 = reference(t, form, numerics(c, dt, form))
        gate(f"{c.fam}_{form}_{dt}", slices(_ratio((got - T).abs(), bound)), f"{what} {form} ({numerics(c, dt, form)})", lambda: (rq - r64).abs())
    assert same_bits(zero, res["plain"][0]), ("accumulate onto zeros differs from the plain call", what)
    if two:
        assert same_bits(steps, res["x2"][0]), ("the second source is not the plain call followed by the accumulating 1x1 call", what)


@gpu
def test_refusals_leave_dx_untouched():
    c = Case("enc", 0, 32, 32, 3, 2, 1, 8, 2)
    odd = c._replace(H=7)
    for dt in DTS:
        R, Ro = Run(make_case(c, dt)), Run(make_case(odd, dt))
        dx, dxo = R.out(), Ro.out()
        lib, st = R.lib, stream()
        a = lambda r, x, cc: (DTI[dt], cc.tr, P(r.dy), P(r.w), P(x), cc.N, cc.H, cc.H, cc.Cin, cc.Cout, cc.k, cc.s, cc.p)
        got = {"accumulate with a second source": lib.mmvae_conv2d_dgrad_ex(*a(R, dx, c), 1, P(R.dy2), P(R.w2), c.Cout, R.sc, st),
               "dy2 without w2": lib.mmvae_conv2d_dgrad_ex(*a(R, dx, c), 0, P(R.dy2), None, c.Cout, R.sc, st),
               "w2 without dy2": lib.mmvae_conv2d_dgrad_ex(*a(R, dx, c), 0, None, P(R.w2), c.Cout, R.sc, st),
               "odd H and W": lib.mmvae_conv2d_dgrad_ex(*a(Ro, dxo, odd), 0, P(Ro.dy2), P(Ro.w2), odd.Cout, Ro.sc, st)}
        torch.cuda.synchronize()
        assert all(rc == ERR_ARG for rc in got.values()), (dt, got)
        for r, names in ((R, ("dx1", "scratch")), (Ro, ("dx1", "scratch"))):
            assert all(r.D.arenas[n].untouched() for n in names), ("a refused call wrote", dt)
            r.D.check("refusals")
        # the odd map itself is fine without the second source
        Ro.call("plain", dxo)
        torch.cuda.synchronize()
        T, bound, _, _ = reference(Ro.t, "plain", "one")
        gate(f"odd_plain_{dt}", slices(_ratio((nchw64(dxo) - T).abs(), bound)), f"{case_id(odd)} {dt} plain")
        Ro.D.check("odd map")


# ================================================================ GPU: census (keep last)
def census_plan():
    plan = [(key(c), dt, form, c) for c in CASES for dt in DTS for form in forms(c)]
    return plan + [("dgrad " + key(c), "bf16", "plain", c) for c, _ in DGRAD_CENSUS]


def census_child():
    """Every case and form once, an 8-element mmvae_convert in front of each: the launch sequence file is cut at the `convert` lines."""
    lib = _L().lib()
    a, b = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    done = []
    for label, dt, form, c in census_plan():
        t = make_case(c, dt)
        R = Run(t, guarded=False)
        dx = nhwc(t.old, dt).cuda()
        assert lib.mmvae_convert(0, 0, P(a), P(b), 8, stream()) == 0
        if label.startswith("dgrad "):
            R.legacy(dx)
        else:
            R.call(form, dx)
        done.append([label, dt, form, c.N])
    torch.cuda.synchronize()
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
        elif n not in ("pack", "pack_multi"):
            assert cur is not None, names[:4]
            cur.append(n)
    assert len(segs) == len(done), (len(segs), len(done))
    wrong, seen = [], collections.defaultdict(set)
    for (label, dt, form, N), seg in zip(done, segs):
        print(f"CENSUS {label} N={N} {dt} {form}: {' '.join(seg)}")
        want = dict((key(c), w) for c, w in DGRAD_CENSUS)[label[6:]] if label.startswith("dgrad ") else LAUNCHES[label][dt][form]
        if tuple(seg) != want:
            wrong.append((label, N, dt, form, seg, want))
        for i, f in enumerate(seg):
            if label.startswith("dgrad "):
                continue
            seen[f].add("accumulating" if form == "acc" or i > 0 else "merged second source" if form == "x2" else "plain")
    assert not wrong, wrong
    for f in (_Q, _D, _P):
        assert "accumulating" in seen[f], (f, dict(seen))
    assert "merged second source" in seen[_P], dict(seen)
    assert "accumulating" in seen[_G3] | seen[_GG], dict(seen)


if __name__ == "__main__":
    if sys.argv[1:] == ["--census-child"]:
        census_child()
    else:
        for fn in (test_reference_is_autograd, test_two_rounding_form_is_the_literal_two_steps, test_bound_helpers_by_hand,
                   test_launch_table_and_scratch_formula):
            fn()
            print("ok", fn.__name__)
