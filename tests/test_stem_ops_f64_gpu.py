"""Float64 parity of the stem entry points: mmvae_stem_fwd (the bf16 stream kernel at S = 64 / 32 / 16, the packed gather path at every other
size and for f32) per image x {outer output ring, interior}, and mmvae_stem_bwd (stem_bwd_kernel "grad" and "gram" modes, stem_gram_sum,
stem_bwd_finalize of csrc/stem_bwd.hip) per channel x tap, plus the += contract, determinism, the refusal paths and the documented buffer
sizes (every buffer is a window of the documented size inside a pattern-filled allocation: an overrun shows as changed guard bytes).

References (float64, from the exact tensors handed to the device):
  R64  conv2d(x, w, stride 2, pad 2) and the autograd of relu(bn(.)) with respect to weight, gamma, beta: dW = sum dy (x) patch with
       dy = A (gm - m1 - m2 yhat) evaluated on the stored y0;
  Rq   the kernels' algorithm: forward weights rounded to the storage type; backward dW = A (W1 - m2 istd (W2 - mean W3) - m1 W3) with
       W1 = sum gm (x) patch, W2 = w_f32 x R (R the 25 x 25 gram matrix of the batch's patches -- NOT the stored y0), W3 = sum patch, the mask
       from y0 bn_scale + bn_shift > 0.
The device is gated against Rq; |Rq - R64| (what storing y0 costs) is printed in failure messages only.

Bounds, in units of u = 2^-24 (times 1.01 for second-order terms):
  * forward: 25 products (exact for bf16 operands, u each for f32) summed in f32 in an order the MFMA owns: any order is within
    25u sum |x w|; a bf16 store adds half a bf16 ulp (2^-9 of the value's binade top).  The statistics rows: each element's own error, plus
    a block's f32 sum of its row -- every lane adds its own pixels in sequence, then four shuffle steps and the four waves: depth
    d = 2 ceil(npix / (32 rows)) + 8 additions, d u sum |y| (one more u for the squares);
  * backward: W1, S0 (the ones column), R and W3 are sums over pixels inside the MFMA accumulators of one wave (32-pixel slabs, wave
    4 block + wv takes slabs gw, gw + 4 gridDim, ...), then the four waves of a block in order in f32, then double.  The bound follows
    that order with running partial sums (mfma_sum_err): for f32 the 16x16x4 MFMA is a k-ordered fma chain, so u of every partial sum of
    the wave's pixel-ordered chain; for bf16 the products are exact and the order inside a 16x16x32 MFMA is unspecified, so 32 roundings of
    at most |C| + max(positive part, negative part) of the slab.  S1 = sum gm y0 is added per lane, then by xor shuffles, then over the waves
    (lane_sum_err).  These propagate through the finalize formula term by term (W2 = w x R takes |w| x dR: the entries of dR are
    independent roundings); the f32 `+=` into the outputs adds u of the gradient and of the result.  The bf16 gates sit lower than the f32
    ones for the reason given: 32 u per slab where the chain of known order pays u per step.
  * mask ties: an element whose float64 pre-activation is within 4u (|y0 scale| + |shift|) of zero may fall on either side: its |g| widens
    the sums of its channel.  At most 0.1 % of a case, asserted on the CPU before device output is looked at.
"""
import importlib
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U = 2.0 ** -24
SLOP = 1.01
EPS = float(np.float32(1e-5))
GUARD = 1 << 16
PATTERN = 0xA5
ERR_UNSUPPORTED = -4
STATS_ROWS = 1024                    # kGatherMaxGridX / the stream kernels' grid cap: the most partial rows a call returns
gpu = pytest.mark.gpu
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
DTI = {"f32": 0, "bf16": 1}


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _header_macro(name):
    src = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    m = re.search(r"#define\s+" + name + r"\s+\(?\s*(\d+)u?\s*(?:<<\s*(\d+))?\s*\)?", src)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


def half_ulp_bf16(v):
    _, ex = torch.frexp(v.abs())
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), ex - 9))


def rnd(t, dt):
    return t.to(torch.bfloat16).float() if dt == "bf16" else t


class Arena:
    """A window of exactly `nbytes` inside a larger allocation filled with a byte pattern: an overrun changes guard bytes, never faults."""

    def __init__(self, nbytes, fill=PATTERN):
        self.n = nbytes
        self.buf = torch.full((GUARD + nbytes + (-nbytes) % 256 + GUARD,), fill, dtype=torch.uint8, device="cuda")
        self.fill = fill

    def view(self, dtype, shape):
        return self.buf[GUARD:GUARD + self.n].view(dtype).view(shape)

    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def window(t, fill=PATTERN):
    if isinstance(t, tuple):
        shape, dtype = t
        a = Arena(int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size(), fill)
        return a, a.view(dtype, shape)
    a = Arena(t.numel() * t.element_size(), fill)
    v = a.view(t.dtype, tuple(t.shape))
    v.copy_(t)
    return a, v


_RATIOS = {}


def gate(name, ratio, what, storage=None):
    """ratio = err / bound per slice; every slice must be <= 1."""
    worst = float(ratio.max())
    _RATIOS[name] = max(_RATIOS.get(name, 0.0), worst)
    print(f"RATIO {name} {worst:.4f} (so far {_RATIOS[name]:.4f}) {what}")
    bad = (ratio > 1).nonzero().tolist()
    assert not bad, (name, what, "slices", bad[:8], "worst err/bound", worst, "storage error |Rq - R64| max", None if storage is None else float(storage.max()))


def _ratio(err, bound):
    return torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


# ================================================================ references (pure CPU, float64)
def out_side(S):
    return (S + 4 - 5) // 2 + 1


def ref_stem_fwd(x, w):
    """x [N, S, S], w [32, 25] float64 -> y [N, H1, H1, 32] and sum |x w| per element."""
    xx = x[:, None]
    ww = w.view(32, 1, 5, 5)
    y = F.conv2d(xx, ww, None, 2, 2)
    mag = F.conv2d(xx.abs(), ww.abs(), None, 2, 2)
    return y.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous()


def patches(x):
    """x [N, S, S] float64 -> [N * H1 * H1, 25] (tap = kh * 5 + kw)."""
    return F.unfold(x[:, None], 5, padding=2, stride=2).permute(0, 2, 1).reshape(-1, 25)


def ref_stem_bwd_r64(g, y0, P, gamma, scale, shift, mean, istd):
    """The mathematical backward on the stored y0: dy = A (gm - m1 - m2 yhat), dW = dy^T patch."""
    n = y0.shape[0]
    gm = g * ((y0 * scale + shift) > 0)
    yhat = (y0 - mean) * istd
    m1, m2 = gm.sum(0) / n, (gm * yhat).sum(0) / n
    dy = gamma * istd * (gm - m1 - m2 * yhat)
    return dict(dW=dy.t() @ P, dgamma=(gm * yhat).sum(0), dbeta=gm.sum(0))


def ref_stem_bwd_rq(g, y0, P, w, gamma, scale, shift, mean, istd):
    """The kernels' algorithm (header of csrc/stem_bwd.hip).  g, y0 [npix, 32], P [npix, 25], w [32, 25]; all float64."""
    n = y0.shape[0]
    pre = y0 * scale + shift
    amb = pre.abs() <= 4 * U * ((y0 * scale).abs() + shift.abs())
    gm = g * (pre > 0)
    S0, S1 = gm.sum(0), (gm * y0).sum(0)
    W1 = gm.t() @ P
    R = P.t() @ P
    W3 = P.sum(0)
    W2 = w @ R
    sgy = istd * (S1 - mean * S0)
    m1, m2, A = S0 / n, sgy / n, gamma * istd
    dW = A[:, None] * (W1 - (m2 * istd)[:, None] * (W2 - mean[:, None] * W3) - m1[:, None] * W3)
    return dict(amb=amb, gm=gm, S0=S0, S1=S1, W1=W1, R=R, W2=W2, W3=W3, sgy=sgy, m1=m1, m2=m2, A=A, dW=dW, dgamma=sgy, dbeta=S0)


def stem_bwd_geometry(N, S, dt):
    """launch_stem_bwd / launch_stem_gram: 32-pixel slabs, one per wave and pass, 4 waves a block, at most 1024 blocks."""
    Wo = S // 2
    nslabs = N * (Wo // (32 // Wo))
    gx = min(1024, (nslabs + 3) // 4)
    spw = -(-nslabs // (4 * gx))                    # slabs of the busiest wave
    CV = 8 if dt == "f32" else 4                    # 16-byte vectors per pixel of g / y0
    NS = 32 * CV // 64
    return dict(nslabs=nslabs, gx=gx, spw=spw, L=64 // CV, NS=NS)


def _by_wave(terms, geo):
    """terms [nslabs * 32, F] -> [waves = 4 gx, spw, 32, F]: wave gw = 4 block + wv takes slabs gw, gw + 4 gx, ... (zero slabs pad the tail)."""
    F_ = terms.shape[1]
    W, spw = 4 * geo["gx"], geo["spw"]
    pad = spw * W * 32 - terms.shape[0]
    t = torch.cat([terms, terms.new_zeros(pad, F_)]) if pad else terms
    return t.view(spw, W, 32, F_).permute(1, 0, 2, 3)


def _waves_err(wave_tot):
    """The flush adds the four waves of a block in order into a zeroed f32 row (the first addition is exact); blocks are summed in double."""
    wt = wave_tot.view(-1, 4, wave_tot.shape[-1]).cumsum(1)
    return wt[:, 1:].abs().sum((0, 1))


def mfma_sum_err(a, b, geo, dt, chunk=128):
    """Bound [Fa * Fb] on the error of the kernels' sum over pixels of the products a[p, i] b[p, j] (a [npix, Fa], b [npix, Fb] or None for
    ones; float64) that runs through the MFMA accumulators.  (The outer product is formed a few waves at a time: 131 200 x 800 at the largest.)
    f32: v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain, and the kernel feeds pixel 4 j + k of the slab in step j: the wave's accumulator is
    one fma chain over its slabs' pixels in ascending order, one rounding per fma, each at most u of the partial sum it produces.
    bf16: one 16x16x32 MFMA per slab; the products are exact in f32 and the order in which the hardware adds the 32 of them and C is not
    specified, so: 32 roundings, each of a partial sum that is C plus a subset of the products -- at most |C| + max(sum of the positive,
    sum of the negative products) -- per slab.  Then the four waves in order, then double."""
    ta, tb = _by_wave(a, geo), None if b is None else _by_wave(b, geo)
    W, F_ = ta.shape[0], a.shape[1] * (1 if b is None else b.shape[1])
    e = a.new_zeros(F_)
    for w0 in range(0, W, chunk):
        tc = ta[w0:w0 + chunk]
        if tb is not None:
            tc = (tc[..., :, None] * tb[w0:w0 + chunk][..., None, :]).reshape(*tc.shape[:3], F_)
        if dt == "f32":
            chain = tc.reshape(tc.shape[0], -1, F_).cumsum(1)
            e += chain.abs().sum((0, 1))
            tot = chain[:, -1]
        else:
            pos, neg = tc.clamp_min(0).sum(2), (-tc).clamp_min(0).sum(2)
            s = pos - neg
            before = s.cumsum(1) - s
            e += 32 * (before.abs() + torch.maximum(pos, neg)).sum((0, 1))
            tot = s.sum(1)
        e += _waves_err(tot)
    return SLOP * U * e


def lane_sum_err(terms, geo):
    """Bound [32] on the error of S1 = sum gm y0, terms [npix, 32]: lane l of a wave's channel group adds pixels l + L k (k < NS) of every slab
    of the wave in order (a product and an addition, or one fma: u of the product and u of the partial sum), the L lanes are combined by xor
    shuffles (pairs, pairs of pairs, ...: u of every node of that tree), then the four waves in order, then double."""
    L, NS = geo["L"], geo["NS"]
    t = _by_wave(terms, geo)                                              # [W, spw, 32, C]
    W, spw, C = t.shape[0], t.shape[1], t.shape[3]
    t = t.reshape(W, spw, NS, L, C).permute(0, 3, 1, 2, 4).reshape(W, L, spw * NS, C)
    chain = t.cumsum(2)
    e = terms.abs().sum(0) + chain[:, :, 1:].abs().sum((0, 1, 2))
    x = chain[:, :, -1]                                                  # [W, L, C]
    while x.shape[1] > 1:
        x = x.reshape(W, x.shape[1] // 2, 2, C).sum(2)
        e = e + x.abs().sum((0, 1))
    return SLOP * U * (e + _waves_err(x[:, 0]))


def stem_bwd_bounds(r, g, y0, P, w, mean, istd, pre_dw, pre_dg, pre_db, geo, dt):
    n = y0.shape[0]
    ga = (g * r["amb"]).abs()
    gm = r["gm"]
    dS0 = mfma_sum_err(gm, None, geo, dt) + ga.sum(0)                          # the ones column of the tap operand
    dS1 = lane_sum_err(gm * y0, geo) + (ga * y0.abs()).sum(0)
    dW1 = mfma_sum_err(gm, P, geo, dt).view(32, 25) + ga.t() @ P.abs()
    dR = mfma_sum_err(P, P, geo, dt).view(25, 25)
    dW3 = mfma_sum_err(P, None, geo, dt)
    dW2 = w.abs() @ dR                                                   # the entries of dR are independent roundings: no cancellation to claim
    dsgy = istd * (dS1 + mean.abs() * dS0)
    dm1, dm2 = dS0 / n, dsgy / n
    A, m1, m2 = r["A"].abs()[:, None], r["m1"].abs()[:, None], r["m2"].abs()[:, None]
    i_, mu = istd[:, None], mean.abs()[:, None]
    core = dW1 + m2 * i_ * (dW2 + mu * dW3) + dm2[:, None] * i_ * (r["W2"] - mean[:, None] * r["W3"]).abs() + m1 * dW3 + dm1[:, None] * r["W3"].abs()
    bW = SLOP * (A * core + U * r["dW"].abs() + U * (pre_dw + r["dW"]).abs())
    bG = SLOP * (dsgy + U * r["sgy"].abs() + U * (pre_dg + r["sgy"]).abs())
    bB = SLOP * (dS0 + U * r["S0"].abs() + U * (pre_db + r["S0"]).abs())
    return bW, bG, bB


# ================================================================ cases
FWD_S = [9, 10, 15, 16, 28, 31, 32, 33, 56, 63, 64]
BWD_CASES = [(S, N) for S in (16, 32, 64) for N in (1, 2, 5)] + [(16, 2050)]      # 4100 slabs > 4096 waves of the capped grid: a second pass


def make_x(N, S, kind, dt, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "binary":
        x = (torch.rand(N, S, S, generator=g) < 0.15).float() * 4.3 - 0.23
    else:
        x = torch.randn(N, S, S, generator=g)
    return rnd(x, dt), g


def make_bwd_case(S, N, dt):
    """Host tensors of one backward case: y0 = the float64 forward rounded to the storage type, statistics from that stored y0 (f32)."""
    x, g = make_x(N, S, "binary", dt, S * 1000 + N)
    w = torch.randn(32, 25, generator=g) * 0.2
    gamma, beta = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.2
    H1 = S // 2
    gout = rnd(torch.randn(N * H1 * H1, 32, generator=g), dt)
    y64, _ = ref_stem_fwd(x.double(), rnd(w, dt).double())
    y0 = y64.reshape(-1, 32).to(TDT[dt])
    yd = y0.double()
    mean = yd.mean(0).float()
    istd = (1.0 / torch.sqrt(((yd - yd.mean(0)) ** 2).mean(0) + EPS)).float()
    scale = (gamma.double() * istd.double()).float()
    shift = (beta.double() - mean.double() * gamma.double() * istd.double()).float()
    pre = [torch.randn(32, 25, generator=g), torch.randn(32, generator=g), torch.randn(32, generator=g)]
    return dict(S=S, N=N, dt=dt, x=x.to(TDT[dt]), w=w, gamma=gamma, g=gout.to(TDT[dt]), y0=y0, mean=mean, istd=istd, scale=scale, shift=shift, pre=pre)


def bwd_refs(c):
    d = lambda t: t.double()
    P = patches(d(c["x"]))
    r = ref_stem_bwd_rq(d(c["g"]), d(c["y0"]), P, d(c["w"]), d(c["gamma"]), d(c["scale"]), d(c["shift"]), d(c["mean"]), d(c["istd"]))
    n_amb = int(r["amb"].sum())
    assert n_amb <= 1e-3 * c["y0"].numel(), (n_amb, c["y0"].numel())
    return P, r


# ================================================================ CPU self-checks
@pytest.mark.parametrize("S", [9, 16, 31])
def test_r64_forward_is_conv2d(S):
    g = torch.Generator().manual_seed(S)
    x = torch.randn(2, S, S, generator=g, dtype=torch.float64)
    w = torch.randn(32, 25, generator=g, dtype=torch.float64)
    y, mag = ref_stem_fwd(x, w)
    H1 = out_side(S)
    assert y.shape == (2, H1, H1, 32)
    # the same sum spelled out through the patches (tap = kh * 5 + kw, offsets kh - 2, kw - 2 around pixel (2 ho, 2 wo))
    torch.testing.assert_close(y.reshape(-1, 32), patches(x) @ w.t(), rtol=0, atol=1e-12)
    xp = F.pad(x, (2, 2, 2, 2))
    ho, wo, c = H1 - 1, 1, 7
    direct = sum(xp[1, 2 * ho + kh, 2 * wo + kw] * w[c, kh * 5 + kw] for kh in range(5) for kw in range(5))
    assert abs(float(y[1, ho, wo, c] - direct)) < 1e-12
    assert (mag >= y.abs() - 1e-12).all()


@pytest.mark.parametrize("S,N", [(16, 2), (32, 1)])
def test_r64_backward_is_autograd_and_rq_equals_r64_unrounded(S, N):
    """float64 inputs, y0 = the exact convolution: R64 is autograd of relu(batch_norm(conv2d)); Rq's w x R identity then gives the same dW."""
    g = torch.Generator().manual_seed(S + N)
    x = ((torch.rand(N, S, S, generator=g) < 0.15).double() * 4.3 - 0.23)
    w = (torch.randn(32, 25, generator=g, dtype=torch.float64) * 0.2).requires_grad_(True)
    gamma = (torch.rand(32, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (torch.randn(32, generator=g, dtype=torch.float64) * 0.2).requires_grad_(True)
    H1 = S // 2
    gout = torch.randn(N * H1 * H1, 32, generator=g, dtype=torch.float64)
    y0 = F.conv2d(x[:, None], w.view(32, 1, 5, 5), None, 2, 2)
    a = F.relu(F.batch_norm(y0, None, None, gamma, beta, True, 0.1, EPS))
    a.backward(gout.view(N, H1, H1, 32).permute(0, 3, 1, 2))
    yd = y0.detach().permute(0, 2, 3, 1).reshape(-1, 32)
    mean = yd.mean(0)
    istd = 1.0 / torch.sqrt(((yd - mean) ** 2).mean(0) + EPS)
    scale = gamma.detach() * istd
    shift = beta.detach() - mean * scale
    P = patches(x)
    r64 = ref_stem_bwd_r64(gout, yd, P, gamma.detach(), scale, shift, mean, istd)
    rq = ref_stem_bwd_rq(gout, yd, P, w.detach(), gamma.detach(), scale, shift, mean, istd)
    tol = dict(rtol=1e-12, atol=1e-11)
    torch.testing.assert_close(r64["dW"], w.grad, **tol)
    torch.testing.assert_close(r64["dgamma"], gamma.grad, **tol)
    torch.testing.assert_close(r64["dbeta"], beta.grad, **tol)
    for k in ("dW", "dgamma", "dbeta"):
        torch.testing.assert_close(rq[k], r64[k], **tol)


def test_ambiguous_share_within_cap_and_geometry():
    for dt in ("f32", "bf16"):
        for S, N in BWD_CASES:
            bwd_refs(make_bwd_case(S, N, dt))
    g = stem_bwd_geometry(1, 16, "bf16")
    assert (g["nslabs"], g["gx"], g["spw"]) == (2, 1, 1)                     # fewer slabs than one block's four waves
    g = stem_bwd_geometry(2050, 16, "bf16")
    assert (g["nslabs"], g["gx"], g["spw"]) == (4100, 1024, 2)               # more slabs than the capped grid has waves
    assert stem_bwd_geometry(5, 64, "f32")["nslabs"] == 160


def test_scratch_macros():
    """mmvae_stem_fwd packs 32 columns x 25 taps x one 16-byte vector; mmvae_stem_bwd carves R (1024 doubles), 1024 gram partial rows and at
    least as many backward partial rows of 64 + 32 * 32 floats out of the BatchNorm scratch."""
    L = _L()
    assert _header_macro("MMVAE_STEM_SCRATCH_BYTES") >= 32 * 25 * 16
    assert L.STEM_SCRATCH_BYTES == _header_macro("MMVAE_STEM_SCRATCH_BYTES") and L.BN_SCRATCH_BYTES == _header_macro("MMVAE_BN_SCRATCH_BYTES")
    assert _header_macro("MMVAE_BN_SCRATCH_BYTES") >= 1024 * 8 + 2 * 1024 * (64 + 32 * 32) * 4


# ================================================================ GPU: forward
@gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["binary", "gauss"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("S", FWD_S)
def test_stem_fwd_f64(S, N, kind, dt):
    L = _L(); lib = L.lib()
    what = f"{dt} S={S} N={N} {kind}"
    x, g = make_x(N, S, kind, dt, S * 100 + N)
    w = torch.randn(32, 25, generator=g) * 0.2
    H1 = out_side(S)
    y64, mag = ref_stem_fwd(x.double(), rnd(w, dt).double())             # both paths round the weights to the storage type
    y_exact, _ = ref_stem_fwd(x.double(), w.double())
    st = torch.cuda.current_stream().cuda_stream
    ax, xd = window(x.to(TDT[dt]).cuda())
    aw, wd = window(w.cuda())
    ay, yd = window(((N, H1, H1, 32), TDT[dt]), 0xFF)
    ast, stats = window(((STATS_ROWS, 2, 32), torch.float32), 0xFF)
    scratch = Arena(_header_macro("MMVAE_STEM_SCRATCH_BYTES"))
    rows = L.check(lib.mmvae_stem_fwd(DTI[dt], L.ptr(xd), L.ptr(wd), L.ptr(yd), N, S, L.ptr(stats), scratch.ptr(), st), "stem_fwd")
    torch.cuda.synchronize()
    for name, a in (("x", ax), ("weight", aw), ("y", ay), ("stats", ast), ("scratch", scratch)):
        assert a.intact(), ("guard bytes changed around", name, what)
    assert 1 <= rows <= STATS_ROWS, rows
    assert torch.equal(xd.cpu(), x.to(TDT[dt])) and torch.equal(wd.cpu(), w)
    y_dev = yd.cpu().double()
    assert not torch.isnan(y_dev).any(), what
    eb = SLOP * 25 * U * mag
    bound = eb + half_ulp_bf16(y64.abs() + eb) if dt == "bf16" else eb
    ratio = _ratio((y_dev - y64).abs(), bound).amax(3)                   # [N, H1, H1]
    ring = torch.zeros(H1, H1, dtype=torch.bool)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
    per_slice = torch.stack([ratio[:, ring].amax(1), ratio[:, ~ring].amax(1)], 1)          # [N, {ring, interior}]
    gate("stem_y", per_slice, what, storage=(rnd(y64.float(), dt).double() - y_exact).abs())
    # statistics rows, summed in float64 per channel, against the sums of the reference y (the kernels sum their f32 accumulators)
    sd = stats[:rows].cpu().double().sum(0)                              # [2, 32]
    assert not torch.isnan(sd).any(), what
    npix = N * H1 * H1
    d = 2 * -(-npix // (32 * rows)) + 8
    yf, mf = y64.reshape(-1, 32), mag.reshape(-1, 32)
    b1 = SLOP * U * (25 * mf.sum(0) + d * yf.abs().sum(0))
    b2 = SLOP * U * (2 * 25 * (yf.abs() * mf).sum(0) + (d + 1) * (yf * yf).sum(0))
    gate("stem_stats", torch.stack([_ratio((sd[0] - yf.sum(0)).abs(), b1), _ratio((sd[1] - (yf * yf).sum(0)).abs(), b2)]), what)


# ================================================================ GPU: backward
@gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("S,N", BWD_CASES)
def test_stem_bwd_f64(S, N, dt):
    L = _L(); lib = L.lib()
    what = f"{dt} S={S} N={N}"
    c = make_bwd_case(S, N, dt)
    P, r = bwd_refs(c)                                                   # asserts the ambiguous-share cap on the CPU first
    d = lambda t: t.double()
    geo = stem_bwd_geometry(N, S, dt)
    pre = [d(t) for t in c["pre"]]
    # the running sums behind the bounds are ordinary float64 tensor arithmetic, 131 200 x 800 terms at the largest case: done on the device
    cu = lambda t: t.cuda()
    bW, bG, bB = (b.cpu() for b in stem_bwd_bounds({k: cu(v) for k, v in r.items()}, cu(d(c["g"])), cu(d(c["y0"])), cu(P), cu(d(c["w"])),
                                                   cu(d(c["mean"])), cu(d(c["istd"])), cu(pre[0]), cu(pre[1]), cu(pre[2]), geo, dt))
    r64 = ref_stem_bwd_r64(d(c["g"]), d(c["y0"]), P, d(c["gamma"]), d(c["scale"]), d(c["shift"]), d(c["mean"]), d(c["istd"]))
    H1 = S // 2
    st = torch.cuda.current_stream().cuda_stream
    arenas = {"scratch": Arena(_header_macro("MMVAE_BN_SCRATCH_BYTES"))}

    def dev(name, t):
        arenas[name], v = window(t.cuda())
        return v
    gd, y0d, xd = dev("g", c["g"].view(N, H1, H1, 32)), dev("y0", c["y0"].view(N, H1, H1, 32)), dev("x", c["x"])
    wd, gmd, scd, shd, md, isd = (dev(k, c[k]) for k in ("w", "gamma", "scale", "shift", "mean", "istd"))
    res = []
    for rep in range(2):
        dw, dg, db = dev(f"dW{rep}", c["pre"][0]), dev(f"dgamma{rep}", c["pre"][1]), dev(f"dbeta{rep}", c["pre"][2])
        L.check(lib.mmvae_stem_bwd(DTI[dt], L.ptr(gd), L.ptr(y0d), L.ptr(xd), L.ptr(wd), L.ptr(gmd), L.ptr(scd), L.ptr(shd), L.ptr(md), L.ptr(isd), L.ptr(dw),
                                   L.ptr(dg), L.ptr(db), N, S, arenas["scratch"].ptr(), st), "stem_bwd")
        res.append((dw, dg, db))
    torch.cuda.synchronize()
    for name, a in arenas.items():
        assert a.intact(), ("guard bytes changed around", name, what)
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), ("backward is not bit-reproducible", what)
    assert torch.equal(gd.cpu().view(-1, 32), c["g"]) and torch.equal(y0d.cpu().view(-1, 32), c["y0"]) and torch.equal(xd.cpu(), c["x"])
    dw, dg, db = (d(t.cpu()) for t in res[0])
    gate("stem_dW", _ratio((dw - (pre[0] + r["dW"])).abs(), bW), what, storage=(r["dW"] - r64["dW"]).abs())
    gate("stem_dgamma", _ratio((dg - (pre[1] + r["dgamma"])).abs(), bG), what, storage=(r["dgamma"] - r64["dgamma"]).abs())
    gate("stem_dbeta", _ratio((db - (pre[2] + r["dbeta"])).abs(), bB), what, storage=(r["dbeta"] - r64["dbeta"]).abs())


@gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("S", [28, 48, 8])
def test_stem_bwd_refuses_other_sizes(S, dt):
    L = _L(); lib = L.lib()
    N, H1 = 2, out_side(S)
    st = torch.cuda.current_stream().cuda_stream
    t = lambda *shape: torch.ones(*shape, device="cuda", dtype=TDT[dt])
    g, y0, x = t(N, H1, H1, 32), t(N, H1, H1, 32), t(N, S, S)
    v, w = torch.ones(32, device="cuda"), torch.ones(32, 25, device="cuda")
    outs = [window(((32, 25), torch.float32))[0], window(((32,), torch.float32))[0], window(((32,), torch.float32))[0]]
    scratch = Arena(_header_macro("MMVAE_BN_SCRATCH_BYTES"))
    rc = lib.mmvae_stem_bwd(DTI[dt], L.ptr(g), L.ptr(y0), L.ptr(x), L.ptr(w), L.ptr(v), L.ptr(v), L.ptr(v), L.ptr(v), L.ptr(v), outs[0].ptr(), outs[1].ptr(),
                            outs[2].ptr(), N, S, scratch.ptr(), st)
    torch.cuda.synchronize()
    assert rc == ERR_UNSUPPORTED, rc
    assert all(a.untouched() for a in outs) and scratch.untouched()
