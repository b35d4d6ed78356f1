"""Float64 per-slice parity of the last up-block's fused kernels and the tail conv through the C ABI: mmvae_tail_join_fwd (f32, bf16),
mmvae_tail_join_fwd_stream, mmvae_tail_join_bwd_reduce / _apply (VALU and MFMA forms of csrc/tail_join.hip), mmvae_upblock_tail_fwd
(up5_tail_fwd_kernel), mmvae_upblock_bwd_fused + mmvae_conv1x1_bwd_fused (csrc/conv_joinbwd.hip) and mmvae_join_conv1x1_fwd
(csrc/conv_joinfwd.hip), plus the += contract, determinism, the refusal paths and the documented buffer sizes (every output and scratch
buffer is a window of the documented size inside a pattern-filled allocation: an overrun shows as changed guard bytes).

References, both float64, both built on the CPU from the exact tensors handed to the device (already rounded to the storage type), with
torch float64 ops only (reference model.py:70-88, :193 and their autograd):
  R64  the mathematical graph: join -> tail conv; g = convT(d_raw, w) [x > 0]; dy = A g + B y + C; both ConvTranspose2d weight and data
       gradients; dy1 = A1 (d_a1 [bn1(y1) > 0]) + B1 y1 + C1; g_in = dys' data gradient + dy1 (x) W1; dW1 = dy1^T (x) pro(xin);
       bn1_sums = (sum gm, sum gm y1);
  Rq   the same graph with a rounding wherever the kernel sources round (read off the .hip files, not off the older test):
       - weights to bf16 where they feed a bf16 MFMA or the bf16 VALU tables (TailW<bf16_t>, op_pack_up / op_pack_down);
       - the joined activation to bf16 in tail_fwd_stream_kernel and up5_tail_fwd_kernel;
       - relu(bn1(y1)) and the optional relu(bn(xin)) prologue to bf16 on their way into the rings;
       - up5_tail_fwd_kernel's recomputed branch outputs are NOT rounded: the file's header comment says "rounded to bf16 like the
         stored tensors", the code joins the f32 MFMA accumulators (acc2 * s2 + (b2 + bs) + accS * ss), and Rq follows the code;
       - the dy rows to bf16 in the LDS rings of join_bwd_stream_kernel; dy1 and pro(xin) to bf16 in conv1_bwd_stream_kernel;
       - d_raw as hi + lo bf16 halves in the MFMA producers of g (hi = RNE; lo = RNE of d - hi in join_bwd_stream and tail_apply_mfma,
         lo CUT to bf16 in tail_reduce_mfma, whose weight gradient is xh dh + xh dl + xl dh with x = hi + lo likewise);
       - outputs to their storage type.
The device is gated against Rq; |Rq - R64| is printed in failure messages and gates nothing.  mmvae_conv1x1_bwd_fused takes the d_a1 and
g_in that mmvae_upblock_bwd_fused left on the device (each gated against Rq first), so its reference is built from those exact tensors.

Gates are per slice: plane-shaped outputs per image x {border ring, interior} (x channel), sums per channel, weight gradients per
(output channel, input channel, tap).  Bounds are in units of u = 2^-24 and are built from the magnitudes of the terms, not of the result:
  * every Rq value v carries a bound e on what the device may hold instead.  A rounding to bf16 of such a value gives Rq's rounding and
    e' = 0, unless a rounding midpoint lies within e of v: then the device may land on the neighbour, e' = e + one bf16 step.  Linear
    operations propagate e through |weights| (the data gradients and weight gradients see the rare one-step differences of their inputs);
  * f32 VALU chains (the dot products and tap sums of tail_join_fwd_kernel, the g of tail_join_bwd_kernel, the per-thread sums) are followed
    step by step in their k order: u of every partial sum and of every product;
  * a bf16 MFMA pays 32 roundings per K = 32 slab of (|C| + sum |products|) -- for the weight gradients |C| is the running float64 partial sum
    of the wave's slabs in walk order and the slab's own part is max(positive, negative products), the bound test_stem_ops_f64_gpu.py uses;
  * partial images: the two wave pairs of a block in order, then launch_wgrad_reduce's order (32 row groups x 4 accumulators, binary tree),
    rebuilt from the launchers' grid sizes; launch_partial_rowsum sums in double and rounds once; the f32 `+=` adds u of the gradient and of
    the result.  Per-block partial rows the entry points return are summed in float64 by the test;
  * a bf16 store adds half a bf16 ulp (2^-9 of the value's binade top);
  * ReLU masks: an element whose float64 pre-activation is within 4u (sum |terms|) of zero is ambiguous: it is excluded from elementwise
    gates and adds its |g| to every sum it enters.  At most 0.1 % of a case, asserted on the CPU before device output is looked at.
bf16-stored outputs reach err / bound ~ 1 whenever a value sits on a rounding tie (the half ulp is the whole bound there); f32 outputs of
bf16 MFMAs sit lower by construction (32 u per slab, where the hardware's internal order is unspecified).

Steady state (the grid caps of the three stream kernels): N = 769 for tail_fwd_stream, N = 1025 for up5_tail_fwd and join_bwd_stream +
conv1_bwd_stream.  Their inputs are drawn on the device and both references are evaluated there in float64, in chunks of images, with
plain tensor arithmetic (the convolutions as einsums over shifted slices; a CPU self-check ties that form to torch's float64 convolutions
and the chunked evaluation to the whole one).  Measured on the MI355X: 0.53 s, 0.22 s and 0.52 s per test -- all three are kept.

Worst err / bound per output on the MI355X (every case, the steady-state ones included; the whole file: 96 GPU tests in 8.4 s, the CPU
self-checks in 5 s):
  tail_join_fwd          r_raw 0.13   stats 0.025 (against the device's own r_raw, accumulation bound alone: 0.21)
  tail_join_fwd_stream   r_raw 0.995  stats 0.017 (own: 0.020)
  upblock_tail_fwd       r_raw 0.998  stats 0.0023 (own: 0.008)
  tail_join_bwd_reduce   sums 0.030 VALU / 0.0015 MFMA   tail dW 0.025 VALU / 0.038 MFMA
  tail_join_bwd_apply    dy2 / dys 1.000 bf16 (VALU and MFMA), 0.47 f32
  upblock_bwd_fused      d_a1 0.992  g_in 0.991  bn1_sums 0.0052  dw_conv2 0.62  dw_up 0.44
  conv1x1_bwd_fused      g_in 1.000  dw_conv1 0.63
  join_conv1x1_fwd       out 0.9999  y1 0.9995  stats 0.030
The r_raw of the two stream forms reach ~1 through joined elements that did land on the other side of a bf16 rounding midpoint (one bf16
step times a weight is then the whole bound of the pixels it feeds); everything stored in bf16 reaches ~1 on rounding ties.
Why the sums sit at 0.002 .. 0.03 and are left there: a sum's bound is the SUM of its n elements' bounds (each element may be off by its
whole bound in the same direction: for g out of a bf16 MFMA that is 32 u of the slab's magnitude, ~50 times what the hardware does on
average) plus the accumulation order's, and grows like n, while the device's rounding errors add up like sqrt(n).  Nothing rigorous is
smaller: the MFMA's internal order is unspecified and g is never stored, so there is no per-element device value to sum instead (where there
is one -- the forward statistics -- the "own" gates above do exactly that and are limited by the same n against sqrt(n) of the
accumulation chain).  The smallest shapes carry these gates; they are still tight enough to catch a dropped lo half of d_raw (2^-9
relative per element), an unmasked sum or a swapped operand: see the mutants in the commit message.
"""
import importlib
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U = 2.0 ** -24
SLOP = 1.01
GUARD = 1 << 16
PATTERN = 0xA5
ERR_ARG = -1
ERR_UNSUPPORTED = -4
gpu = pytest.mark.gpu
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
DTI = {"f32": 0, "bf16": 1}
F64 = torch.float64


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
    """ratio = err / bound per slice; every slice must be <= 1.  storage: a callable giving |Rq - R64| (evaluated on failure only)."""
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _RATIOS[name] = max(_RATIOS.get(name, 0.0), worst)
    print(f"RATIO {name} {worst:.4f} (so far {_RATIOS[name]:.4f}) {what}")
    bad = (ratio > 1).nonzero().tolist()
    if bad:
        st = None if storage is None else float(storage().max())
        raise AssertionError((name, what, "slices", bad[:8], "worst err/bound", worst, "storage error |Rq - R64| max", st))


def _ratio(err, bound):
    return torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


def plane_slices(ratio):
    """ratio [N, C, H, W] -> [N, C, {border ring, interior}]."""
    H, W = ratio.shape[-2:]
    ring = torch.zeros(H, W, dtype=torch.bool, device=ratio.device)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
    return torch.stack([ratio[..., ring].amax(-1), ratio[..., ~ring].amax(-1)], -1)


# ================================================================ float64 building blocks
def rbf(v):
    """Round a float64 tensor to the bf16 grid (nearest, ties to even), staying in float64."""
    m, ex = torch.frexp(v)
    return torch.ldexp(torch.round(m * 256.0), ex - 8)


def cut_bf(v):
    """Cut (toward zero) to the bf16 grid: the upper half of an f32 word."""
    m, ex = torch.frexp(v)
    return torch.ldexp(torch.trunc(m * 256.0), ex - 8)


def _spacing(v):
    _, ex = torch.frexp(v.abs())
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), ex - 8))


def rbf_e(v, e, q=True):
    """(Rq's bf16 rounding of v, bound on |device's rounding - it|) for a device value within e of v."""
    if not q:
        return v, e
    r = rbf(v)
    sv = _spacing(v)
    dist = sv / 2 - (v - r).abs()                                        # to the nearest rounding midpoint
    flip = (e > 0) & ((dist <= e) | (v == 0))
    return r, torch.where(flip, e + _spacing(v.abs() + e), torch.zeros_like(e))


def relu_e(p, e):
    """relu of a pre-activation known to e: exact zero where p < -e."""
    return p.clamp_min(0), torch.where(p < -e, torch.zeros_like(e), e)


def v4(t):
    return t.double().view(1, -1, 1, 1)


def affine_pre(terms):
    """terms: list of float64 tensors whose sum is a pre-activation -> (p, sum |terms|, ambiguous)."""
    p = sum(terms)
    m = sum(t.abs() for t in terms)
    return p, m, p.abs() <= 4 * U * m


def join_pre(c):
    y2, ys = c.y2.double(), c.ys.double()
    return affine_pre([y2 * v4(c.s2), v4(c.b2).expand_as(y2), ys * v4(c.ss), v4(c.bs).expand_as(y2)])


def prologue(y, s, b, q=True):
    """bf16(relu(y s + b)) with its bound, the mask, the ambiguity; s None: y itself."""
    y = y.double()
    if s is None:
        z = torch.zeros_like(y)
        return types.SimpleNamespace(v=y, e=z, pre=y, amb=z.bool(), m=y.abs())
    p, m, amb = affine_pre([y * v4(s), v4(b).expand_as(y)])
    v, e = relu_e(p, 2 * U * m)
    v, e = rbf_e(v, e, q)
    return types.SimpleNamespace(v=v, e=e, pre=p, amb=amb, m=m)


def conv_g(d, w, taps=None):
    """g[n, ci, h, w] = sum_{oc, kh, kw} d[n, oc, h + 1 - kh, w + 1 - kw] w[oc, ci, kh, kw].  On the device (the steady-state cases) the
    convolutions below run tap by tap as float64 einsums over shifted slices -- plain tensor arithmetic; the CPU self-check ties both forms."""
    if not (d.is_cuda if taps is None else taps):
        return F.conv_transpose2d(d, w, padding=1)
    H, W = d.shape[2:]
    dp = F.pad(d, (1, 1, 1, 1))
    return sum(torch.einsum("nohw,oi->nihw", dp[:, :, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W], w[:, :, kh, kw]) for kh in range(3) for kw in range(3))


def up(a, w, taps=None):
    """ConvTranspose2d(k4 s2 p1): out[co, 2h - 1 + kh, 2w - 1 + kw] += a[ci, h, w] w[ci, co, kh, kw]."""
    if not (a.is_cuda if taps is None else taps):
        return F.conv_transpose2d(a, w, stride=2, padding=1)
    n, _, h, wd = a.shape
    out = a.new_zeros(n, w.shape[1], 2 * h + 2, 2 * wd + 2)
    for kh in range(4):
        for kw in range(4):
            out[:, :, kh:kh + 2 * h:2, kw:kw + 2 * wd:2] += torch.einsum("nihw,io->nohw", a, w[:, :, kh, kw])
    return out[:, :, 1:-1, 1:-1]


def up_dgrad(dy, w, taps=None):
    """Its data gradient: d_a[ci, h, w] = sum dy[co, 2h - 1 + kh, 2w - 1 + kw] w[ci, co, kh, kw]."""
    if not (dy.is_cuda if taps is None else taps):
        return F.conv2d(dy, w, stride=2, padding=1)
    H, W = dy.shape[2:]
    dp = F.pad(dy, (1, 1, 1, 1))
    return sum(torch.einsum("nohw,io->nihw", dp[:, :, kh:kh + H:2, kw:kw + W:2], w[:, :, kh, kw]) for kh in range(4) for kw in range(4))


def col_conv(J, wc, taps=None):
    """D[kw][h, col] = sum_{c, kh} wc[kw, c, kh] J[c, h + kh - 1, col]."""
    if not (J.is_cuda if taps is None else taps):
        return F.conv2d(J, wc, padding=(1, 0))
    H = J.shape[2]
    Jp = F.pad(J, (0, 0, 1, 1))
    return sum(torch.einsum("nchw,kc->nkhw", Jp[:, :, kh:kh + H], wc[:, :, kh, 0]) for kh in range(3))


def up_wgrad_slabs(a, dy):
    """[N, 32 rows, Cin, Cout, 4, 4]: per input row h, sum_w a[n, ci, h, w] dy[n, co, 2h - 1 + kh, 2w - 1 + kw]."""
    dg = F.pad(dy, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)          # [N, Co, 32, 32, 4, 4]
    return torch.einsum("nihw,nohwkl->nhiokl", a, dg)


# ================================================================ launch geometry (rebuilt from the launchers)
def stream_grid(nunits, cap, per_block, floor):
    """`int gx = cap; while (gx > floor && gx * per_block > nunits) gx -= gx > 8 ? 8 : 1` with floor 8 (never below 8) or 1."""
    gx = cap
    while gx > floor and gx * per_block > nunits:
        gx -= 8 if gx > 8 else 1
    return gx


def stream_walk(nunits, gx, slots_per_block):
    """Units of every (block, slot): the XCD-aware walk of the stream kernels (eight chunks of ceil(nunits / 8) when gx % 8 == 0)."""
    out = {}
    for b in range(gx):
        for s in range(slots_per_block):
            if gx % 8 == 0:
                per = (nunits + 7) >> 3
                lo = (b & 7) * per
                first, step, end = lo + (b >> 3) * slots_per_block + s, (gx >> 3) * slots_per_block, min(nunits, lo + per)
            else:
                first, step, end = b * slots_per_block + s, gx * slots_per_block, nunits
            out[(b, s)] = list(range(first, end, step))
    return out


def tail_fwd_stream_grid(N):
    return stream_grid(4 * N, 768, 4, 1)                                   # launch_tail_fwd_stream: 64 / 16 = 4 units per image


def up5_grid(N):
    return stream_grid(2 * N, 512, 4, 1)                                   # launch_up5_tail_fwd: 32 / 16 = 2 units per image


def join_bwd_grid(N):
    return stream_grid(N, 512, 2, 8)                                       # launch_join_bwd_stream: one image per unit, two pairs per block


def conv1_bwd_grid(rows):
    return stream_grid(rows, 1024, 4, 8)                                   # launch_conv1_bwd_stream: one row per wave and step


def join_conv1_grid(npix):
    return stream_grid(npix // 32, 1024, 4, 8)


def tail_bwd_path(dt, OC, W, wgrad, apply_):
    if apply_:
        return "mfma" if dt == "bf16" and OC == 1 and W >= 32 else "valu"
    return "mfma" if wgrad and dt == "bf16" and OC == 1 and W >= 32 else "valu"


def tail_bwd_geometry(N, H, W, dt, path, apply_):
    pt = 64 if dt == "f32" else 128
    ntiles = N * H * W // pt
    cap = 768 if apply_ and path == "mfma" else 1024
    blocks = min(ntiles, cap)
    return dict(pt=pt, ntiles=ntiles, blocks=blocks, T=-(-ntiles // blocks))


def tail_supported(H, W, dt):
    pt = 64 if dt == "f32" else 128
    return W <= pt and (W & (W - 1)) == 0 and (H * W) % pt == 0


# ================================================================ summation-order bounds
def valu_sum_err(terms, geo, products=False):
    """tail_join_bwd_kernel's per-channel sums, terms [npix, C] in NHWC pixel order: pixel (k blocks + b) PT + j is added in pass k by thread
    j of block b's channel group (f32 chain over k), block_channel_reduce adds the PT threads in order (f32 chain over j); blocks in double."""
    npix, C = terms.shape
    K, blocks, T = geo["pt"], geo["blocks"], geo["T"]
    pad = T * blocks * K - npix
    t = torch.cat([terms, terms.new_zeros(pad, C)]) if pad else terms
    t = t.view(T, blocks, K, C)
    c1 = t.cumsum(0)
    e = c1[1:].abs().sum((0, 1, 2))
    c2 = c1[-1].cumsum(1)
    e = e + c2[:, 1:].abs().sum((0, 1))
    if products:
        e = e + terms.abs().sum(0)
    return SLOP * U * e


def mfma_lane_sum_err(terms, geo, products=False):
    """tail_reduce_mfma_kernel's sums: lane (wave wv, pixel lane r) adds pixel 32 wv + 16 pt + r of tile b + k blocks in the order (k, pt),
    row16_sum combines the 16 pixel lanes (r ^ 8, ^ 4, ^ 2, ^ 1), then (w0 + w1) + (w2 + w3); blocks in double."""
    npix, C = terms.shape
    blocks, T = geo["blocks"], geo["T"]
    pad = T * blocks * 128 - npix
    t = torch.cat([terms, terms.new_zeros(pad, C)]) if pad else terms
    t = t.view(T, blocks, 4, 2, 16, C).permute(1, 2, 4, 0, 3, 5).reshape(blocks, 4, 16, 2 * T, C)
    chain = t.cumsum(3)
    e = chain[:, :, :, 1:].abs().sum((0, 1, 2, 3))
    x = chain[:, :, :, -1]                                                # [blocks, 4, 16, C]
    for half in (8, 4, 2, 1):
        x = x.view(blocks, 4, -1, 2, half, C).sum(3).reshape(blocks, 4, -1, C)
        e = e + x.abs().sum((0, 1, 2))
    w = x[:, :, 0]                                                        # [blocks, 4, C]
    pair = w.view(blocks, 2, 2, C).sum(2)
    e = e + pair.abs().sum((0, 1)) + pair.sum(1).abs().sum(0)
    if products:
        e = e + terms.abs().sum(0)
    return SLOP * U * e


def slab_chain_err(pos, neg, dim=0):
    """bf16 MFMA accumulator over slabs in order along `dim`, pos / neg = sums of the positive / negative products of each slab: 32 roundings
    per slab of at most |C| + max(pos, neg)."""
    s = pos - neg
    before = s.cumsum(dim) - s
    return 32 * U * (before.abs() + torch.maximum(pos, neg)).sum(dim)


def wgrad_reduce_err(parts):
    """wgrad_reduce_kernel<8> (the 4096- and 256-element images here: 32 row groups): thread (rg, l) adds parts rg, rg + 32, ... into four
    accumulators while four are left, the rest into the first; (s0 + s1) + (s2 + s3); binary tree over the row groups.  parts [nb, F]."""
    nb, F_ = parts.shape
    RG = 32
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


# ================================================================ cases
def span(g, n=16, lo=-1.0, hi=1.0):
    """Per-channel magnitudes over two decades."""
    return 10.0 ** (torch.rand(n, generator=g) * (hi - lo) + lo)


def sgn(g, n=16):
    return (torch.rand(n, generator=g) < 0.5).float() * 2 - 1


def bn_pair(g, mag):
    """(scale, shift) of a BatchNorm over a tensor of per-channel magnitude `mag`: scale * y is O(1), the shift is not negligible."""
    return sgn(g) * (0.5 + torch.rand(16, generator=g)) / mag, torch.randn(16, generator=g) * 0.5


def bwd_coefs(g, mag):
    """(A, B, C) of a BatchNorm backward: A over two decades, B y and C of the size of A g."""
    A = sgn(g) * span(g)
    return A, sgn(g) * A.abs() * (0.3 + 0.7 * torch.rand(16, generator=g)) / mag, sgn(g) * A.abs() * (0.2 + 0.8 * torch.rand(16, generator=g))


def make_join(N, H, W, OC, dt, seed=0, dev=False):
    """dev: the steady-state cases draw their large tensors on the device (a CUDA generator) and keep the whole case there."""
    g = torch.Generator().manual_seed(1000 * N + 10 * H + OC + seed + (7 if dt == "bf16" else 0))
    c = types.SimpleNamespace(N=N, H=H, W=W, OC=OC, dt=dt)
    if dev:
        gd = torch.Generator(device="cuda").manual_seed(g.initial_seed())
        c.rn = lambda *shape: torch.randn(*shape, generator=gd, device="cuda")
        c.to = lambda t: t.cuda()
    else:
        c.rn = lambda *shape: torch.randn(*shape, generator=g)
        c.to = lambda t: t
    m2, ms = span(g), span(g)
    c.y2 = rnd(c.rn(N, 16, H, W) * c.to(m2.view(1, 16, 1, 1)), dt)
    c.ys = rnd(c.rn(N, 16, H, W) * c.to(ms.view(1, 16, 1, 1)), dt)
    (c.s2, c.b2), (c.ss, c.bs) = bn_pair(g, m2), bn_pair(g, ms)
    c.w = (torch.rand(OC, 16, 3, 3, generator=g) + 0.5) * ((torch.rand(OC, 16, 3, 3, generator=g) < 0.5).float() * 2 - 1) / 6.0
    c.bias = torch.randn(OC, generator=g)
    d = c.rn(N, OC, H, W)
    d[:, :, 0], d[:, :, -1], d[:, :, :, 0], d[:, :, :, -1] = d[:, :, 0] * 2, d[:, :, -1] * 2, d[:, :, :, 0] * 2, d[:, :, :, -1] * 2
    c.d_raw = d
    (c.A2, c.B2, c.C2), (c.As, c.Bs, c.Cs) = bwd_coefs(g, m2), bwd_coefs(g, ms)
    c.gen = g
    return on_device(c) if dev else c


def on_device(c):
    for k, v in vars(c).items():
        if isinstance(v, torch.Tensor):
            setattr(c, k, v.cuda())
        elif isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
            setattr(c, k, [t.cuda() for t in v])
    return c


def make_upblock(N, pro_x, seed=0, dev=False):
    """The whole block: y1, xin [N, 16, 32, 32] bf16 next to independent y2 / ys [N, 16, 64, 64] (the backward entry points take all four)."""
    c = make_join(N, 64, 64, 1, "bf16", seed=seed + 31 + int(pro_x), dev=dev)
    g = c.gen
    m1, mx = span(g), span(g)
    c.y1 = rnd(c.rn(N, 16, 32, 32) * c.to(m1.view(1, 16, 1, 1)), "bf16")
    c.s1, c.b1 = bn_pair(g, m1)
    if pro_x:
        c.xin = rnd(c.rn(N, 16, 32, 32) * c.to(mx.view(1, 16, 1, 1)), "bf16")
        c.sx, c.bx = bn_pair(g, mx)
    else:
        c.xin = rnd(c.rn(N, 16, 32, 32).clamp_min(0) * c.to(mx.view(1, 16, 1, 1)), "bf16")      # an activation
        c.sx, c.bx = None, None
    c.w2 = torch.randn(16, 16, 4, 4, generator=g) / 8.0
    c.wu = torch.randn(16, 16, 4, 4, generator=g) / 8.0 / mx.view(16, 1, 1, 1)
    c.w1 = torch.randn(16, 16, 1, 1, generator=g) / 4.0
    c.A1, c.B1, c.C1 = bwd_coefs(g, m1)
    c.pre = [torch.randn(16, 16, 4, 4, generator=g), torch.randn(16, 16, 4, 4, generator=g), torch.randn(16, 16, 1, 1, generator=g)]
    c.pro_x = pro_x
    return on_device(c) if dev else c


def sub(c, n0, n1):
    """Images [n0, n1) of a case (the per-channel parameters are shared)."""
    s = types.SimpleNamespace(**vars(c))
    for k in ("y2", "ys", "d_raw", "y1", "xin"):
        if hasattr(c, k):
            setattr(s, k, getattr(c, k)[n0:n1])
    s.N = n1 - n0
    return s


def amb_cap(amb, what):
    n = int(amb.sum())
    assert n <= 1e-3 * amb.numel(), ("ambiguous ReLU elements above 0.1 %", what, n, amb.numel())


# ================================================================ references: tail conv forward
def ref_tail_fwd_valu(c, q=True):
    """tail_join_fwd_kernel: x in f32 (never rounded), weights of the storage type; a thread's dot product over its VE channels in order, the
    CV lanes of a pixel by xor shuffles, the nine tap partials added onto the bias in (kh, kw) order.  -> r [N, H, W], bound, stats."""
    N, H, W, dt = c.N, c.H, c.W, c.dt
    VE = 4 if dt == "f32" else 8
    CV = 16 // VE
    p, m, amb = join_pre(c)
    x, ex = relu_e(p, 4 * U * m)
    wq = (rbf(c.w.double()) if (q and dt == "bf16") else c.w.double()).view(16, 9)
    bias = float(c.bias[0])
    out, eo = [], []
    for n0 in range(0, N, 4):
        xs, es = x[n0:n0 + 4], ex[n0:n0 + 4]
        n = xs.shape[0]
        t = (xs[:, :, None] * wq.view(1, 16, 9, 1, 1)).view(n, CV, VE, 9, H, W)
        cum = t.cumsum(2)
        e = (t.abs().sum(2) + cum.abs().sum(2)).sum(1)                     # [n, 9, H, W]
        part = cum[:, :, -1]
        while part.shape[1] > 1:
            part = part.view(n, part.shape[1] // 2, 2, 9, H, W).sum(2)
            e = e + part.abs().sum(1)
        T = part[:, 0]
        eT = SLOP * U * e + (es[:, :, None] * wq.abs().view(1, 16, 9, 1, 1)).sum(1)
        Tp, eTp = F.pad(T, (1, 1, 1, 1)), F.pad(eT, (1, 1, 1, 1))
        v = torch.full((n, H, W), bias, dtype=F64)
        ev = torch.zeros(n, H, W, dtype=F64)
        for kh in range(3):
            for kw in range(3):
                v = v + Tp[:, kh * 3 + kw, kh:kh + H, kw:kw + W]
                ev = ev + eTp[:, kh * 3 + kw, kh:kh + H, kw:kw + W] + SLOP * U * v.abs()
        out.append(v)
        eo.append(ev)
    r, er = torch.cat(out), torch.cat(eo)
    pt = 64 if dt == "f32" else 128
    depth = H // (pt // W) + 1 + 6 + 2                                     # a thread's passes, wave_sum, the four waves
    return types.SimpleNamespace(r=r, e=er, amb=amb, depth=depth, stats=stats_ref(r.view(N, -1), er.view(N, -1), depth))


def stats_ref(v, ev, depth):
    """(sum, sum of squares) over the last axis with the bound of an f32 accumulation of the given depth."""
    s, q = v.sum(-1), (v * v).sum(-1)
    bs = ev.sum(-1) + SLOP * U * depth * v.abs().sum(-1)
    bq = (2 * v.abs() * ev + ev * ev).sum(-1) + SLOP * U * (depth + 1) * q
    return torch.stack([s, q], -1), torch.stack([bs, bq], -1)


def tail_from_joined(J, eJ, w, bias, q=True):
    """The per-tap-column MFMA form of tail_fwd_stream_kernel / up5_tail_fwd_kernel on a joined activation J [N, 16, 64, 64] (bf16 values with
    bound eJ): D[kw][col] = rows kh = 0, 1 in one K = 32 slab, kh = 2 in a second; out[p] = (D0[p - 1] + D1[p]) + D2[p + 1] + bias."""
    wq = rbf(w.double()) if q else w.double()
    wc = wq[0].permute(2, 0, 1).unsqueeze(-1).contiguous()                 # [kw, c, kh, 1]
    Dk = col_conv(J, wc)                                                  # [N, 3, H, W]: no horizontal shift yet
    w01, w2_ = wc.abs().clone(), wc.abs().clone()
    w01[:, :, 2], w2_[:, :, :2] = 0, 0
    m01, m2_ = col_conv(J.abs(), w01), col_conv(J.abs(), w2_)
    eD = col_conv(eJ, wc.abs()) + SLOP * 32 * U * (2 * m01 + m2_)
    Dp, eDp = F.pad(Dk, (1, 1)), F.pad(eD, (1, 1))
    W = J.shape[-1]
    a = Dp[:, 0, :, 0:W] + Dp[:, 1, :, 1:W + 1]
    b = a + Dp[:, 2, :, 2:W + 2]
    r = b + float(bias[0])
    e = eDp[:, 0, :, 0:W] + eDp[:, 1, :, 1:W + 1] + eDp[:, 2, :, 2:W + 2] + SLOP * U * (a.abs() + b.abs() + r.abs())
    return r, e


def stream_stats_depth(nunits, gx):
    """A gq = 0 lane adds its 4 columns of the 16 rows of every unit of its wave, then row16_sum (4) and the four waves (2)."""
    most = max(len(v) for v in stream_walk(nunits, gx, 4).values())
    return most * 64 + 6


def ref_tail_fwd_stream(c, q=True, total=None):
    """total: the whole case's image count when c is a chunk of it (the statistics' depth follows the whole launch)."""
    p, m, amb = join_pre(c)
    x, ex = relu_e(p, 4 * U * m)
    J, eJ = rbf_e(x, ex, q)
    r, e = tail_from_joined(J, eJ, c.w, c.bias, q)
    gx = tail_fwd_stream_grid(total or c.N)
    depth = stream_stats_depth(4 * (total or c.N), gx)
    return types.SimpleNamespace(r=r, e=e, amb=amb, rows=gx, depth=depth, stats=stats_ref(r.reshape(-1), e.reshape(-1), depth))


def ref_up5_tail_fwd(c, q=True, total=None):
    a1, ax = prologue(c.y1, c.s1, c.b1, q), prologue(c.xin, c.sx, c.bx, q)
    w2q, wuq = (rbf(c.w2.double()), rbf(c.wu.double())) if q else (c.w2.double(), c.wu.double())
    # two K = 32 slabs (th = 0, 1) per output pixel and branch; the accumulators are joined in f32, not rounded
    y2, ys = up(a1.v, w2q), up(ax.v, wuq)
    e2 = up(a1.e, w2q.abs()) + SLOP * 64 * U * up(a1.v.abs(), w2q.abs())
    es = up(ax.e, wuq.abs()) + SLOP * 64 * U * up(ax.v.abs(), wuq.abs())
    jb = v4(c.b2) + v4(c.bs)
    terms = [y2 * v4(c.s2), jb.expand_as(y2), ys * v4(c.ss)]
    p, m, amb = affine_pre(terms)
    x, ex = relu_e(p, 4 * U * m + e2 * v4(c.s2).abs() + es * v4(c.ss).abs())
    J, eJ = rbf_e(x, ex, q)
    r, e = tail_from_joined(J, eJ, c.w, c.bias, q)
    gx = up5_grid(total or c.N)
    most = max(len(v) for v in stream_walk(2 * (total or c.N), gx, 4).values())
    amb_all = torch.cat([a1.amb.reshape(-1), ax.amb.reshape(-1), amb.reshape(-1)])
    depth = most * 128 + 6                                                 # 4 columns of 32 output rows per unit, row16_sum, the four waves
    return types.SimpleNamespace(r=r, e=e, amb=amb_all, rows=gx, depth=depth, stats=stats_ref(r.reshape(-1), e.reshape(-1), depth))


# ================================================================ references: tail conv backward (reduce / apply)
def ref_g(c, path, lo_cut, q=True):
    """g = convT(d_raw, w) before the mask, with its bound.  valu: an f32 fma chain over (oc, kh, kw); mfma: one bf16 slab over the nine taps
    of the hi and of the lo half of d_raw."""
    d, w = c.d_raw.double(), c.w.double()
    if not q:
        g = conv_g(d, w)
        return g, torch.zeros_like(g)
    wq = rbf(w) if c.dt == "bf16" else w
    if path == "mfma":
        dh = rbf(d)
        dl = cut_bf(d - dh) if lo_cut else rbf(d - dh)
        g = conv_g(dh, wq) + conv_g(dl, wq)
        return g, SLOP * 32 * U * conv_g(dh.abs() + dl.abs(), wq.abs())
    N, OC, H, W = d.shape
    dp = F.pad(d, (1, 1, 1, 1))
    cum = torch.zeros(N, 16, H, W, dtype=F64)
    e = torch.zeros_like(cum)
    for oc in range(OC):
        for kh in range(3):
            for kw in range(3):
                t = dp[:, oc, None, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W] * wq[oc, :, kh, kw].view(1, 16, 1, 1)
                cum = cum + t
                e = e + t.abs() + cum.abs()
    return cum, SLOP * U * e


def masked(g, eg, p, amb):
    """(g [p > 0], bound): an ambiguous element may hold either value."""
    mask = p > 0
    return g * mask, torch.where(amb, g.abs() + eg, eg * mask)


def pix(t):
    """[N, C, H, W] -> [npix, C] in NHWC order."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def ref_tail_reduce(c, wgrad, q=True):
    path = tail_bwd_path(c.dt, c.OC, c.W, wgrad, False)
    geo = tail_bwd_geometry(c.N, c.H, c.W, c.dt, path, False)
    p, m, amb = join_pre(c)
    g, eg = ref_g(c, path, True, q)
    gm, em = masked(g, eg, p, amb)
    y2, ys = c.y2.double(), c.ys.double()
    terms = [gm, gm * y2, gm * ys]
    errs = [em, em * y2.abs(), em * ys.abs()]
    sums, bounds = [], []
    for k, (t, e) in enumerate(zip(terms, errs)):
        tp = pix(t)
        order = (mfma_lane_sum_err if path == "mfma" else valu_sum_err)(tp, geo, products=k > 0)
        sums.append(tp.sum(0))
        bounds.append(pix(e).sum(0) + order)
    r = types.SimpleNamespace(sums=torch.stack(sums), bsums=torch.stack(bounds), amb=amb, rows=geo["blocks"], path=path, geo=geo)
    if wgrad:
        x, ex = relu_e(p, 4 * U * m)
        d = c.d_raw.double()[:, 0]
        N, H, W = d.shape
        if path == "mfma" and q:
            xh, exh = rbf_e(x, ex)
            xl, exl = rbf_e(x - xh, ex + exh)
            dh = rbf(d)
            dl = cut_bf(d - dh)
            prods = [(xh, dh), (xh, dl), (xl, dh)]
            flip = [(exh, dh.abs() + dl.abs()), (exl, dh.abs())]
        else:
            prods, flip = [(x, d)], [(ex, d.abs())]

        def tapsum(a, b):                                               # [16, 9]: sum_pix a[ci](h, w) b(h + 1 - kh, w + 1 - kw)
            bp = F.pad(b, (1, 1, 1, 1))
            return torch.stack([(a * bp[:, None, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W]).sum((0, 2, 3)) for kh in range(3) for kw in range(3)], 1)
        dw = sum(tapsum(a, b) for a, b in prods)
        mag = tapsum(x.abs(), d.abs())
        bw = sum(tapsum(a, b) for a, b in flip)
        if path == "mfma":
            bw = bw + SLOP * U * (32 * 3 * geo["T"] + 2) * mag                 # three slabs per tile, each at most the wave's whole magnitude; the waves
        else:
            CV = 4 if c.dt == "f32" else 2
            depth = 2 * geo["T"] + int(math.log2(64 // CV)) + 4           # product + add per pass, the butterfly, the four waves
            bw = bw + SLOP * U * depth * mag
        r.dw, r.bdw = dw, bw
    return r


def ref_tail_apply(c, q=True):
    path = tail_bwd_path(c.dt, c.OC, c.W, False, True)
    p, m, amb = join_pre(c)
    g, eg = ref_g(c, path, False, q)
    gm, em = masked(g, eg, p, amb)
    out = []
    for A, B, C, y in ((c.A2, c.B2, c.C2, c.y2), (c.As, c.Bs, c.Cs, c.ys)):
        t = [v4(A) * gm, v4(B) * y.double(), v4(C).expand_as(gm)]
        v = sum(t)
        e = v4(A).abs() * em + SLOP * 3 * U * sum(x.abs() for x in t)
        out.append((v, e))
    return types.SimpleNamespace(dy2=out[0], dys=out[1], amb=amb, path=path)


# ================================================================ references: the block's backward in one pass
def upblock_bwd_chunk(c, q=True):
    """Everything of the one-pass backward that is local to the images of c (a whole case or a chunk): the elementwise outputs with their
    bounds, and per image what the walk-ordered sums need (bn1's lane totals and chain errors, the weight gradients' totals and slab errors)."""
    N = c.N
    p, m, amb = join_pre(c)
    g, eg = ref_g(c, "mfma", False, q)
    gm, em = masked(g, eg, p, amb)
    dy = []
    for A, B, C, y in ((c.A2, c.B2, c.C2, c.y2), (c.As, c.Bs, c.Cs, c.ys)):
        t = [v4(A) * gm, v4(B) * y.double(), v4(C).expand_as(gm)]
        v = sum(t)
        e = v4(A).abs() * em + SLOP * 2 * U * sum(x.abs() for x in t)
        dy.append(rbf_e(v, e, q))
    a1, ax = prologue(c.y1, c.s1, c.b1, q), prologue(c.xin, c.sx, c.bx, q)
    w2q, wuq = (rbf(c.w2.double()), rbf(c.wu.double())) if q else (c.w2.double(), c.wu.double())
    r = types.SimpleNamespace(amb=torch.cat([amb.reshape(-1), a1.amb.reshape(-1), ax.amb.reshape(-1)]), dy2=dy[0][0], dys=dy[1][0])
    # data gradients: eight K = 32 slabs per pixel chained in one accumulator
    dx = []
    for (d, ed), wq in ((dy[0], w2q), (dy[1], wuq)):
        v = up_dgrad(d, wq)
        e = up_dgrad(ed, wq.abs()) + SLOP * 32 * 8 * U * up_dgrad(d.abs(), wq.abs())
        dx.append((v, e))
    r.da1, r.gin0 = dx
    # bn1's sums from the f32 data gradient: a lane's chain over the (h, pt) steps of an image, its total, the sums of the element bounds
    gm1, em1 = masked(dx[0][0], dx[0][1], a1.pre, a1.amb)
    y1 = c.y1.double()
    r.bn = []
    for k, (t, e) in enumerate(((gm1, em1), (gm1 * y1, em1 * y1.abs()))):
        cs = t.permute(0, 2, 3, 1).reshape(N, 64, 16, 16).cumsum(1)       # [n, (h, pt), r, C]
        r.bn.append(dict(chain=cs[:, 1:].abs().sum((1, 2)).cpu(), lane=cs[:, -1].cpu(), elem=e.sum((2, 3)).cpu(),
                         prod=(t.abs().sum((2, 3)) if k else torch.zeros_like(e.sum((2, 3)))).cpu(), val=t.sum((2, 3)).cpu()))
    # weight gradients: one slab per P row
    r.wg = []
    for a, (d, ed) in ((a1, dy[0]), (ax, dy[1])):
        ap, an, dp, dn = a.v.clamp_min(0), (-a.v).clamp_min(0), d.clamp_min(0), (-d).clamp_min(0)
        pos = (up_wgrad_slabs(ap, dp) + up_wgrad_slabs(an, dn)).reshape(N, 32, 4096)
        neg = (up_wgrad_slabs(ap, dn) + up_wgrad_slabs(an, dp)).reshape(N, 32, 4096)
        flip = (up_wgrad_slabs(a.e, d.abs() + ed) + up_wgrad_slabs(a.v.abs(), ed)).sum((0, 1)).reshape(-1)
        r.wg.append(dict(err=slab_chain_err(pos, neg, 1).cpu(), tot=(pos - neg).sum(1).cpu(), flip=flip.cpu()))
    return r


def upblock_bwd_assemble(N, bn, wg, pre):
    """The walk-ordered part: bn1_sums and the two weight gradients from the per-image pieces (bn, wg: lists over chunks of what
    upblock_bwd_chunk leaves).  A pair's second image continues the chains of its first: every step's partial sum moves by the first image's
    total (64 lane steps, 32 slabs)."""
    gx = join_bwd_grid(N)
    walk = stream_walk(N, gx, 2)
    cat = lambda lst, k: torch.cat([x[k] for x in lst])
    sums, bs = [], []
    for k in range(2):
        chain, lane, elem, prod, val = (cat([b[k] for b in bn], key) for key in ("chain", "lane", "elem", "prod", "val"))
        order = torch.zeros(16, dtype=F64)
        for b in range(gx):
            tot = []
            for s_ in range(2):
                x = torch.zeros(16, 16, dtype=F64)
                for u in walk[(b, s_)]:
                    order += chain[u] + 64 * x.abs().sum(0)
                    x = x + lane[u]
                while x.shape[0] > 1:
                    x = x.view(2, x.shape[0] // 2, 16).sum(0)
                    order += x.abs().sum(0)
                tot.append(x[0])
            order += (tot[0] + tot[1]).abs()
        v = val.sum(0)
        sums.append(v)
        bs.append(elem.sum(0) + SLOP * U * (order + prod.sum(0) + v.abs()))
    dw = []
    for i in range(2):
        err, tot, flip = cat([w[i] for w in wg], "err"), cat([w[i] for w in wg], "tot"), sum(w[i]["flip"] for w in wg)
        e = torch.zeros(4096, dtype=F64)
        parts = torch.zeros(gx, 4096, dtype=F64)
        for b in range(gx):
            for s_ in range(2):
                x = torch.zeros(4096, dtype=F64)
                for u in walk[(b, s_)]:
                    e += err[u] + 32 * 32 * U * x.abs()
                    x = x + tot[u]
                if s_ == 1:
                    e += U * (parts[b] + x).abs()                         # pair 0 + pair 1
                parts[b] += x
        grad, er = wgrad_reduce_err(parts)
        res = pre[i].double().cpu().reshape(-1) + grad
        dw.append((res.view(16, 16, 4, 4), (SLOP * (flip + e + er + U * grad.abs() + U * res.abs())).view(16, 16, 4, 4), grad.view(16, 16, 4, 4)))
    return torch.stack(sums), torch.stack(bs), dw, gx


def ref_upblock_bwd(c, q=True):
    r = upblock_bwd_chunk(c, q)
    r.sums, r.bsums, r.dw, r.gx = upblock_bwd_assemble(c.N, [r.bn], [r.wg], c.pre)
    return r


def ref_conv1x1_bwd(c, da1, gin0, pre_dw, q=True):
    """conv1_bwd_stream_kernel on the given d_a1 / g_in (bf16 values as float64, [N, 16, H, W]-shaped rows of 32 pixels)."""
    a1 = prologue(c.y1, c.s1, c.b1, q)
    y1 = c.y1.double()
    t = [v4(c.A1) * da1 * (a1.pre > 0), v4(c.B1) * y1, v4(c.C1).expand_as(y1)]
    v = sum(t)
    e = SLOP * 3 * U * sum(x.abs() for x in t) + torch.where(a1.amb, (v4(c.A1) * da1).abs(), torch.zeros_like(v))
    dy1, e1 = rbf_e(v, e, q)
    x = prologue(c.xin, c.sx, c.bx, q)
    w1q = (rbf(c.w1.double()) if q else c.w1.double()).view(16, 16)        # [co, cin]
    dg = torch.einsum("nohw,oi->nihw", dy1, w1q)
    mg = torch.einsum("nohw,oi->nihw", dy1.abs(), w1q.abs())
    gin = dg + gin0
    eg = torch.einsum("nohw,oi->nihw", e1, w1q.abs()) + SLOP * U * (32 * mg + gin.abs())
    # dW1[co][cin]: one slab per row of 32 pixels; wave 4 b + wv takes rows b 4 + wv + k 4 gx; the four waves in order; launch_wgrad_reduce; +=
    rows = dy1.shape[0] * dy1.shape[2]
    gx = conv1_bwd_grid(rows)
    dr = dy1.permute(0, 2, 1, 3).reshape(rows, 16, -1)                    # [row, co, w]
    xr = x.v.permute(0, 2, 1, 3).reshape(rows, 16, -1)                    # [row, cin, w]
    prod = lambda a, b: torch.einsum("row,riw->roi", a, b).reshape(rows, 256)
    dp, dn, xp, xn = dr.clamp_min(0), (-dr).clamp_min(0), xr.clamp_min(0), (-xr).clamp_min(0)
    pos, neg = prod(dp, xp) + prod(dn, xn), prod(dp, xn) + prod(dn, xp)
    e1r = e1.permute(0, 2, 1, 3).reshape(rows, 16, -1)
    exr = x.e.permute(0, 2, 1, 3).reshape(rows, 16, -1)
    flip = (prod(e1r, xr.abs() + exr) + prod(dr.abs(), exr)).sum(0)
    W_ = 4 * gx
    k = -(-rows // W_)
    pad = k * W_ - rows
    if pad:
        pos, neg = torch.cat([pos, pos.new_zeros(pad, 256)]), torch.cat([neg, neg.new_zeros(pad, 256)])
    pos, neg = pos.view(k, W_, 256), neg.view(k, W_, 256)
    e = slab_chain_err(pos, neg).sum(0)
    wt = (pos - neg).sum(0).view(gx, 4, 256).cumsum(1)
    e = e + U * wt[:, 1:].abs().sum((0, 1))
    grad, er = wgrad_reduce_err(wt[:, -1])
    res = pre_dw.double().reshape(-1) + grad
    bw = SLOP * (flip + e + er + U * grad.abs() + U * res.abs())
    return types.SimpleNamespace(gin=gin, egin=eg, dw=res.view(16, 16), bdw=bw.view(16, 16), grad=grad.view(16, 16), amb=torch.cat([a1.amb.reshape(-1), x.amb.reshape(-1)]), gx=gx)


def ref_join_conv1(y2, s2, b2, ys, ss, bs, w, q=True):
    """join_conv1_fwd_kernel; y2, ys [npix, C] bf16, w [16, C].  out = bf16(relu((y2 s2 + b2) + (ys ss + bs))); y1 = one slab of out w^T."""
    d = lambda t: t.double()
    p, m, amb = affine_pre([d(y2) * d(s2), d(b2).expand(y2.shape), d(ys) * d(ss), d(bs).expand(y2.shape)])
    x, ex = relu_e(p, 4 * U * m)
    o, eo = rbf_e(x, ex, q)
    wq = rbf(d(w)) if q else d(w)
    y1 = o @ wq.t()
    mag = o.abs() @ wq.abs().t()
    e1 = eo @ wq.abs().t() + SLOP * 32 * U * mag
    return types.SimpleNamespace(out=x, eout=ex, y1=y1, e1=e1, amb=amb, outq=o)


# ================================================================ case lists
# tail_join_fwd / bwd_reduce / bwd_apply.  64x64 bf16 is 4096 / 128 = 32 tiles an image: N = 25 gives 800 tiles, one past the 768-block cap of
# tail_apply_mfma (a block takes a second tile); N = 33 gives 1056, past the 1024-block cap of tail_reduce_mfma and of the VALU reduce.
# f32 (8, 8) x 1100: 64-pixel tiles, 1100 tiles > 1024 (the VALU cap case; refused in bf16: 64 pixels are no multiple of 128).
TAIL_SHAPES = [(1, 64, 64, 1), (3, 64, 64, 1), (2, 32, 32, 1), (2, 16, 16, 1), (1, 128, 128, 1), (2, 32, 32, 3), (1100, 8, 8, 1)]
TAIL_CASES = [(s, dt) for s in TAIL_SHAPES for dt in ("f32", "bf16")] + [((25, 64, 64, 1), "bf16"), ((33, 64, 64, 1), "bf16")]
# tail_fwd_stream: 4 units an image.  N = 1, 3: grids 1, 3 (plain walk); N = 9: 36 units, 8 x 4 = 32 <= 36 -> grid 8, chunks of ceil(36 / 8) = 5:
# the last chunk holds unit 35 alone and wave 0 of the others walks two units; N = 17: 68 units -> grid 16, chunks of 9, two blocks a chunk.
STREAM_N = [1, 3, 9, 17]
# up5_tail_fwd: 2 units an image.  N = 17: 34 units -> grid 8, chunks of ceil(34 / 8) = 5, chunk 7 starts at unit 35 >= 34: an empty block that
# must still leave a zero statistics row; N = 19: 38 units, chunk 7 holds 35 .. 37.
UP5_N = [1, 3, 17, 19]
# join_bwd_stream: one unit an image, at least 8 blocks of two pairs.  N = 1: 15 idle pairs; N = 2: both pairs of block 0;
# N = 17: chunks of 3 images -> pair 0 of blocks 0 .. 4 walks two images (its rings are reused across the image boundary), blocks 6, 7 idle;
# N = 19: chunks of 3, block 6 holds image 18 alone.
BWD_N = [1, 2, 17, 19]
JC_CASES = [(16, 1, 32), (16, 3, 32), (32, 5, 16), (32, 257, 16)]


def tail_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ================================================================ CPU self-checks
def test_bf16_grid_helpers():
    g = torch.Generator().manual_seed(1)
    v = torch.randn(4096, generator=g) * 10.0 ** torch.randint(-6, 6, (4096,), generator=g).float()
    assert torch.equal(rbf(v.double()).float(), v.to(torch.bfloat16).float())
    cut = (v.view(torch.int32) & -65536).view(torch.float32)
    assert torch.equal(cut_bf(v.double()).float(), cut)
    assert torch.equal(half_ulp_bf16(torch.tensor([1.0, 1.5, 2.0], dtype=F64)), torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -7], dtype=F64))
    # a value on a midpoint may round either way; one well inside a cell may not
    r, e = rbf_e(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 0.0, 0.0], dtype=F64), torch.tensor([1e-9, 1e-9, 1e-9, 0.0], dtype=F64))
    assert e[0] > 2.0 ** -7 and e[1] == 0 and 0 < e[2] < 2e-9 and e[3] == 0 and r[1] == 1.0


def test_launch_geometry():
    assert [tail_fwd_stream_grid(n) for n in STREAM_N] == [1, 3, 8, 16]
    w = stream_walk(36, 8, 4)
    assert w[(7, 0)] == [35] and w[(7, 1)] == [] and w[(0, 0)] == [0, 4] and sorted(sum(w.values(), [])) == list(range(36))
    assert sorted(sum(stream_walk(68, 16, 4).values(), [])) == list(range(68))
    assert [up5_grid(n) for n in UP5_N] == [1, 1, 8, 8]
    w = stream_walk(34, 8, 4)
    assert all(w[(7, s)] == [] for s in range(4)) and sorted(sum(w.values(), [])) == list(range(34))       # the empty chunk
    assert [join_bwd_grid(n) for n in BWD_N] == [8, 8, 8, 8] and join_bwd_grid(1025) == 512
    w = stream_walk(17, 8, 2)
    assert w[(0, 0)] == [0, 2] and w[(0, 1)] == [1] and w[(5, 0)] == [15] and w[(5, 1)] == [16] and w[(6, 0)] == [] and w[(7, 1)] == []
    assert sum(1 for v in stream_walk(1, 8, 2).values() if not v) == 15
    assert conv1_bwd_grid(32) == 8 and conv1_bwd_grid(17 * 32) == 136 and conv1_bwd_grid(129 * 32) == 1024 and 129 * 32 > 4 * 1024
    assert join_conv1_grid(257 * 256) == 512 and 257 * 256 // 32 > 4 * 512 and join_conv1_grid(1024) == 8        # 2056 steps: eight waves walk two
    g = tail_bwd_geometry(25, 64, 64, "bf16", "mfma", True)
    assert (g["ntiles"], g["blocks"], g["T"]) == (800, 768, 2)
    g = tail_bwd_geometry(33, 64, 64, "bf16", "mfma", False)
    assert (g["ntiles"], g["blocks"], g["T"]) == (1056, 1024, 2)
    g = tail_bwd_geometry(1100, 8, 8, "f32", "valu", False)
    assert (g["ntiles"], g["blocks"], g["T"]) == (1100, 1024, 2)
    assert not tail_supported(8, 8, "bf16") and tail_supported(128, 128, "bf16") and not tail_supported(128, 128, "f32")
    assert _header_macro("MMVAE_WGRAD_SCRATCH_BYTES") >= 16384 + (2 * 1024 * 4096 + 1024 * 32) * 4      # packed weights, two images a block, bn rows


def test_tapwise_convolutions_are_the_torch_ones():
    """The device form of the reference convolutions (einsums over shifted slices) against torch's float64 convolutions."""
    g = torch.Generator().manual_seed(11)
    r = lambda *sh: torch.randn(*sh, generator=g, dtype=F64)
    d, w = r(2, 3, 8, 8), r(3, 16, 3, 3)
    torch.testing.assert_close(conv_g(d, w, taps=True), conv_g(d, w, taps=False), rtol=1e-12, atol=1e-12)
    a, wt = r(2, 16, 6, 6), r(16, 16, 4, 4)
    torch.testing.assert_close(up(a, wt, taps=True), up(a, wt, taps=False), rtol=1e-12, atol=1e-12)
    dy = r(2, 16, 12, 12)
    torch.testing.assert_close(up_dgrad(dy, wt, taps=True), up_dgrad(dy, wt, taps=False), rtol=1e-12, atol=1e-12)
    J, wc = r(2, 16, 8, 8), r(3, 16, 3, 1)
    torch.testing.assert_close(col_conv(J, wc, taps=True), col_conv(J, wc, taps=False), rtol=1e-12, atol=1e-12)


def test_chunked_block_backward_is_the_whole_one():
    """The steady-state case evaluates the block's backward reference in chunks of images: the same sums, gradients and bounds."""
    c = make_upblock(3, True)
    whole = ref_upblock_bwd(c)
    chunks = [upblock_bwd_chunk(sub(c, a, b)) for a, b in ((0, 1), (1, 3))]
    sums, bsums, dw, gx = upblock_bwd_assemble(3, [x.bn for x in chunks], [x.wg for x in chunks], c.pre)
    torch.testing.assert_close(sums, whole.sums, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(bsums, whole.bsums, rtol=1e-9, atol=0)
    for a, b in zip(dw, whole.dw):
        torch.testing.assert_close(a[0], b[0], rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(a[1], b[1], rtol=1e-9, atol=0)
    torch.testing.assert_close(torch.cat([x.da1[0] for x in chunks]), whole.da1[0], rtol=0, atol=0)


def test_wgrad_reduce_order_sums_every_part_once():
    g = torch.Generator().manual_seed(3)
    for nb in (8, 136, 512, 1024):
        parts = torch.randn(nb, 8, generator=g, dtype=F64)
        s, e = wgrad_reduce_err(parts)
        torch.testing.assert_close(s, parts.sum(0), rtol=1e-12, atol=1e-12)
        assert (e > 0).all() and (e < U * 64 * parts.abs().sum(0)).all()


def test_r64_is_autograd():
    """With every rounding switched off the reference functions are the autograd of reference model.py:70-88, :193 in float64."""
    c = make_upblock(2, True)
    d = lambda t: t.double()
    y1, xin = d(c.y1), d(c.xin)
    w2 = d(c.w2).requires_grad_(True)
    wu = d(c.wu).requires_grad_(True)
    w1 = d(c.w1).requires_grad_(True)
    tw = d(c.w).requires_grad_(True)
    a1 = F.relu(y1 * v4(c.s1) + v4(c.b1)).requires_grad_(True)
    ax = F.relu(xin * v4(c.sx) + v4(c.bx)).requires_grad_(True)
    y2, ys = up(a1, w2), up(ax, wu)
    y2.retain_grad(), ys.retain_grad()
    x = F.relu(y2 * v4(c.s2) + v4(c.b2) + ys * v4(c.ss) + v4(c.bs))
    r = F.conv2d(x, tw, d(c.bias), padding=1)
    r.backward(d(c.d_raw))
    # forward: the three forward entry points compute r from (their inputs for) y2, ys
    cc = types.SimpleNamespace(**vars(c))
    cc.y2, cc.ys = y2.detach(), ys.detach()
    for ref in (ref_tail_fwd_valu(cc, q=False).r, ref_tail_fwd_stream(cc, q=False).r, ref_up5_tail_fwd(c, q=False).r):
        torch.testing.assert_close(ref, r.detach()[:, 0], rtol=1e-11, atol=1e-11)
    # backward of the join: g = dL/dx masked; the reduce sums and the tail conv's weight gradient
    g = (y2.grad / v4(c.s2))
    red = ref_tail_reduce(cc, True, q=False)
    torch.testing.assert_close(red.sums[0], g.sum((0, 2, 3)), rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(red.sums[1], (g * y2.detach()).sum((0, 2, 3)), rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(red.dw, tw.grad[0].reshape(16, 9), rtol=1e-10, atol=1e-10)
    # the block's backward with A = s, B = C = 0 is plain autograd: dy2 = s2 g, dys = ss g
    z = torch.zeros(16)
    cc.A2, cc.B2, cc.C2, cc.As, cc.Bs, cc.Cs = c.s2, z, z, c.ss, z, z
    cc.pre = [torch.zeros_like(p) for p in c.pre]
    ap = ref_tail_apply(cc, q=False)
    torch.testing.assert_close(ap.dy2[0], y2.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(ap.dys[0], ys.grad, rtol=1e-10, atol=1e-10)
    ub = ref_upblock_bwd(cc, q=False)
    torch.testing.assert_close(ub.da1[0], a1.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(ub.gin0[0], ax.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(ub.dw[0][0], w2.grad, rtol=1e-10, atol=1e-9)
    torch.testing.assert_close(ub.dw[1][0], wu.grad, rtol=1e-10, atol=1e-9)
    gm = a1.grad * (a1.detach() > 0)
    torch.testing.assert_close(ub.sums, torch.stack([gm.sum((0, 2, 3)), (gm * y1).sum((0, 2, 3))]), rtol=1e-10, atol=1e-10)
    # conv1 (1x1): y1 = conv2d(pro(xin), w1); with A1 = 1, B1 = C1 = 0, dy1 = d_a1 [bn1(y1) > 0]
    xa = ax.detach().clone().requires_grad_(True)
    yc = F.conv2d(xa, w1)
    yc.backward(gm)
    cc.A1, cc.B1, cc.C1 = torch.ones(16), z, z
    r1 = ref_conv1x1_bwd(cc, a1.grad, ax.grad, torch.zeros(16, 16), q=False)
    torch.testing.assert_close(r1.gin, ax.grad + xa.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(r1.dw, w1.grad.view(16, 16), rtol=1e-10, atol=1e-9)
    # join + conv1 forward
    jc = ref_join_conv1(pix(y2.detach()), c.s2, c.b2, pix(ys.detach()), c.ss, c.bs, c.w1.view(16, 16), q=False)
    torch.testing.assert_close(jc.y1, pix(F.conv2d(x.detach(), d(c.w1))), rtol=1e-10, atol=1e-10)


def test_rq_stays_close_to_r64_and_bounds_are_positive():
    """Rq differs from R64 by bf16 roundings only (percent level of each slice's scale), and every bound is finite and positive."""
    c = make_upblock(2, True)
    rq, r64 = ref_upblock_bwd(c), ref_upblock_bwd(c, q=False)
    for a, b in ((rq.da1, r64.da1), (rq.gin0, r64.gin0), (rq.dw[0], r64.dw[0]), (rq.dw[1], r64.dw[1])):
        assert torch.isfinite(a[1]).all() and (a[1] > 0).all()
        assert float((a[0] - b[0]).abs().max()) < 0.05 * float(b[0].abs().max())
    assert (rq.bsums > 0).all() and torch.isfinite(rq.bsums).all()
    f, f64_ = ref_up5_tail_fwd(c), ref_up5_tail_fwd(c, q=False)
    assert float((f.r - f64_.r).abs().max()) < 0.05 * float(f64_.r.abs().max()) and (f.e > 0).all()
    c2 = make_join(2, 32, 32, 1, "bf16")
    for wg in (False, True):
        r = ref_tail_reduce(c2, wg)
        assert (r.bsums > 0).all() and torch.isfinite(r.bsums).all()
        assert r.path == ("mfma" if wg else "valu")
    assert (ref_tail_reduce(c2, True).bdw > 0).all()


def test_ambiguous_share_within_cap():
    """Every case's ambiguous ReLU elements (join mask, bn1's mask, the sx / bx prologue) from the reference alone: at most 0.1 %."""
    for shape, dt in TAIL_CASES:
        if tail_supported(shape[1], shape[2], dt):
            amb_cap(join_pre(make_join(*shape, dt))[2], (shape, dt))
    for N in sorted(set(STREAM_N)):
        amb_cap(join_pre(make_join(N, 64, 64, 1, "bf16"))[2], ("stream", N))
    for N in sorted(set(UP5_N + BWD_N)):
        for pro_x in (False, True):
            c = make_upblock(N, pro_x)
            amb_cap(join_pre(c)[2], ("upblock join", N, pro_x))
            amb_cap(prologue(c.y1, c.s1, c.b1).amb, ("bn1", N, pro_x))
            amb_cap(prologue(c.xin, c.sx, c.bx).amb, ("pro_x", N, pro_x))
            if N <= 3:
                amb_cap(ref_up5_tail_fwd(c).amb, ("up5", N, pro_x))
    for C, N, H in JC_CASES:
        amb_cap(make_jc(C, N, H)[-1].amb, ("join_conv1", C, N, H))


# ================================================================ GPU helpers
def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(TDT[dt])


def nchw(t):
    return t.double().permute(0, 3, 1, 2)


class Dev:
    """Device copies of a case's tensors, each a guarded window; outputs are registered the same way."""

    def __init__(self):
        self.arenas = {}

    def put(self, name, t, fill=PATTERN):
        if t is None:
            return None
        self.arenas[name], v = window(t.cuda() if isinstance(t, torch.Tensor) else t, fill)
        return v

    def scratch(self, name, nbytes):
        self.arenas[name] = Arena(nbytes)
        return self.arenas[name].ptr()

    def check(self, what):
        for name, a in self.arenas.items():
            assert a.intact(), ("guard bytes changed around", name, what)


def P(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def join_dev(D, c):
    d = types.SimpleNamespace()
    d.y2, d.ys = D.put("y2", nhwc(c.y2, c.dt)), D.put("ys", nhwc(c.ys, c.dt))
    for k in ("s2", "b2", "ss", "bs", "w", "bias", "d_raw", "A2", "B2", "C2", "As", "Bs", "Cs"):
        setattr(d, k, D.put(k, getattr(c, k)))
    return d


def own_stats_gate(name, got, r_dev, depth, what):
    """The kernels add the very f32 values they store: the returned sums against the float64 sums of the device's own r_raw, with the f32
    accumulation bound alone (the elementwise gate ties r_raw to Rq; this one is not widened by the sum of the per-element bounds)."""
    v = r_dev.double().reshape(got.shape[0] if got.dim() > 1 else 1, -1)
    own = torch.stack([v.sum(-1), (v * v).sum(-1)], -1).reshape(got.shape)
    bound = SLOP * U * torch.stack([depth * v.abs().sum(-1), (depth + 1) * (v * v).sum(-1)], -1).reshape(got.shape)
    gate(name + "_own", _ratio((got - own).abs(), bound), what)


def check_stats_rows(name, stats, rows, total_rows, ref, what, r_dev, depth):
    """Rows [0, rows) finite and summing (float64) to Rq's sums within the bound; rows beyond untouched (still the fill pattern)."""
    host = stats.cpu()
    assert torch.isfinite(host[:rows]).all(), ("non-finite statistics row", what)
    rest = stats[rows:total_rows].contiguous().view(torch.uint8)
    assert bool((rest == 0xFF).all()), ("statistics rows beyond the returned count were written", what)
    got = host[:rows].double().sum(0)
    gate(name, _ratio((got - ref[0]).abs(), ref[1]), what)
    own_stats_gate(name, got, r_dev, depth, what)


# ================================================================ GPU: tail conv forward
@gpu
@pytest.mark.parametrize("shape,dt", [(s, dt) for s, dt in TAIL_CASES if s[3] == 1], ids=tail_id)
def test_tail_join_fwd_f64(shape, dt):
    L = _L(); lib = L.lib()
    N, H, W, OC = shape
    what = f"tail_join_fwd {dt} {shape}"
    c = make_join(*shape, dt)
    D = Dev()
    d = join_dev(D, c)
    res = []
    for rep in range(2):
        r = D.put(f"r{rep}", ((N, H, W), torch.float32), 0xFF)
        stats = D.put(f"stats{rep}", ((N, 2), torch.float32), 0xFF)
        rc = lib.mmvae_tail_join_fwd(DTI[dt], P(d.y2), P(d.s2), P(d.b2), P(d.ys), P(d.ss), P(d.bs), P(d.w), P(d.bias), P(r), P(stats), N, H, W, stream())
        res.append((r, stats))
    torch.cuda.synchronize()
    D.check(what)
    if not tail_supported(H, W, dt):
        assert rc == ERR_UNSUPPORTED, rc
        assert all(D.arenas[k].untouched() for k in ("r0", "r1", "stats0", "stats1")), what
        return
    assert rc == N, rc
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]), ("not bit-reproducible", what)
    ref = ref_tail_fwd_valu(c)
    amb_cap(ref.amb, what)
    got = res[0][0].cpu().double()
    assert torch.isfinite(got).all(), what
    gate("tail_fwd_r", plane_slices(_ratio((got - ref.r).abs(), ref.e)[:, None]), what, lambda: (ref.r - ref_tail_fwd_valu(c, q=False).r).abs())
    st = res[0][1].cpu().double()
    gate("tail_fwd_stats", _ratio((st - ref.stats[0]).abs(), ref.stats[1]), what)
    own_stats_gate("tail_fwd_stats", st, got, ref.depth, what)


@gpu
@pytest.mark.parametrize("N", STREAM_N)
def test_tail_join_fwd_stream_f64(N):
    L = _L(); lib = L.lib()
    what = f"tail_join_fwd_stream N={N}"
    c = make_join(N, 64, 64, 1, "bf16")
    ref = ref_tail_fwd_stream(c)
    amb_cap(ref.amb, what)
    D = Dev()
    d = join_dev(D, c)
    res = []
    for rep in range(2):
        r = D.put(f"r{rep}", ((N, 64, 64), torch.float32), 0xFF)
        stats = D.put(f"stats{rep}", ((N + 4, 2), torch.float32), 0xFF)      # the contract is [N][2]; four more rows to see that they stay
        rows = L.check(lib.mmvae_tail_join_fwd_stream(1, P(d.y2), P(d.s2), P(d.b2), P(d.ys), P(d.ss), P(d.bs), P(d.w), P(d.bias), P(r), P(stats), N, 64, 64,
                                                      stream()), what)
        res.append((r, stats))
    torch.cuda.synchronize()
    D.check(what)
    assert rows == ref.rows and rows <= N, (rows, ref.rows)
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]), ("not bit-reproducible", what)
    got = res[0][0].cpu().double()
    assert torch.isfinite(got).all(), what
    gate("stream_fwd_r", plane_slices(_ratio((got - ref.r).abs(), ref.e)[:, None]), what, lambda: (ref.r - ref_tail_fwd_stream(c, q=False).r).abs())
    check_stats_rows("stream_fwd_stats", res[0][1], rows, N + 4, ref.stats, what, got, ref.depth)


@gpu
@pytest.mark.parametrize("pro_x", [False, True])
@pytest.mark.parametrize("N", UP5_N)
def test_upblock_tail_fwd_f64(N, pro_x):
    L = _L(); lib = L.lib()
    what = f"upblock_tail_fwd N={N} pro_x={pro_x}"
    c = make_upblock(N, pro_x)
    ref = ref_up5_tail_fwd(c)
    amb_cap(ref.amb, what)
    D = Dev()
    d = join_dev(D, c)
    y1, xin = D.put("y1", nhwc(c.y1, "bf16")), D.put("xin", nhwc(c.xin, "bf16"))
    s1, b1, sx, bx, w2, wu = (D.put(k, getattr(c, k)) for k in ("s1", "b1", "sx", "bx", "w2", "wu"))
    sc = D.scratch("scratch", 16 << 10)
    res = []
    for rep in range(2):
        r = D.put(f"r{rep}", ((N, 64, 64), torch.float32), 0xFF)
        stats = D.put(f"stats{rep}", ((max(N, 8) + 4, 2), torch.float32), 0xFF)
        rows = L.check(lib.mmvae_upblock_tail_fwd(P(y1), P(s1), P(b1), P(w2), P(xin), P(sx), P(bx), P(wu), P(d.s2), P(d.b2), P(d.ss), P(d.bs), P(d.w), P(d.bias),
                                                  P(r), P(stats), N, sc, stream()), what)
        res.append((r, stats))
    torch.cuda.synchronize()
    D.check(what)
    assert rows == ref.rows, (rows, ref.rows)
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]), ("not bit-reproducible", what)
    got = res[0][0].cpu().double()
    assert torch.isfinite(got).all(), what
    gate("up5_fwd_r", plane_slices(_ratio((got - ref.r).abs(), ref.e)[:, None]), what, lambda: (ref.r - ref_up5_tail_fwd(c, q=False).r).abs())
    check_stats_rows("up5_fwd_stats", res[0][1], rows, max(N, 8) + 4, ref.stats, what, got, ref.depth)
    if N == 17:
        assert bool((res[0][1][7] == 0).all()), "the block without work must leave a zero statistics row"


# ================================================================ GPU: tail conv backward
@gpu
@pytest.mark.parametrize("wgrad", [False, True])
@pytest.mark.parametrize("shape,dt", TAIL_CASES, ids=tail_id)
def test_tail_join_bwd_reduce_f64(shape, dt, wgrad):
    L = _L(); lib = L.lib()
    N, H, W, OC = shape
    what = f"tail_join_bwd_reduce {dt} {shape} wgrad={wgrad}"
    c = make_join(*shape, dt)
    D = Dev()
    d = join_dev(D, c)
    res = []
    for rep in range(2):
        part = D.put(f"partials{rep}", ((1024, 3, 16), torch.float32), 0xFF)
        wpart = D.put(f"wpartials{rep}", ((1024, 16, 9), torch.float32), 0xFF) if wgrad else None
        rows = lib.mmvae_tail_join_bwd_reduce(DTI[dt], P(d.d_raw), P(d.w), OC, P(d.y2), P(d.s2), P(d.b2), P(d.ys), P(d.ss), P(d.bs), P(part), P(wpart), N, H, W,
                                              stream())
        res.append((part, wpart))
    torch.cuda.synchronize()
    D.check(what)
    if not tail_supported(H, W, dt) or (wgrad and OC != 1):
        assert rows == ERR_UNSUPPORTED, rows
        assert all(a.untouched() for k, a in D.arenas.items() if "partials" in k), what
        return
    ref = ref_tail_reduce(c, wgrad)
    amb_cap(ref.amb, what)
    assert rows == ref.rows, (rows, ref.rows)
    for a, b in zip(res[0], res[1]):
        assert a is None or same_bits(a, b), ("not bit-reproducible", what)
    for t in res[0]:
        if t is not None:
            assert torch.isfinite(t[:rows]).all() and bool((t[rows:].contiguous().view(torch.uint8) == 0xFF).all()), ("rows beyond the returned count", what)
    sums = res[0][0][:rows].cpu().double().sum(0)
    gate(f"reduce_sums_{ref.path}", _ratio((sums - ref.sums).abs(), ref.bsums), what, lambda: (ref.sums - ref_tail_reduce(c, wgrad, q=False).sums).abs())
    if wgrad:
        dw = res[0][1][:rows].cpu().double().sum(0)
        gate(f"reduce_dw_{ref.path}", _ratio((dw - ref.dw).abs(), ref.bdw), what, lambda: (ref.dw - ref_tail_reduce(c, wgrad, q=False).dw).abs())


@gpu
@pytest.mark.parametrize("shape,dt", TAIL_CASES, ids=tail_id)
def test_tail_join_bwd_apply_f64(shape, dt):
    L = _L(); lib = L.lib()
    N, H, W, OC = shape
    what = f"tail_join_bwd_apply {dt} {shape}"
    c = make_join(*shape, dt)
    D = Dev()
    d = join_dev(D, c)
    res = []
    for rep in range(2):
        dy2, dys = D.put(f"dy2_{rep}", ((N, H, W, 16), TDT[dt]), 0xFF), D.put(f"dys_{rep}", ((N, H, W, 16), TDT[dt]), 0xFF)
        rc = lib.mmvae_tail_join_bwd_apply(DTI[dt], P(d.d_raw), P(d.w), OC, P(d.y2), P(d.s2), P(d.b2), P(d.ys), P(d.ss), P(d.bs), P(d.A2), P(d.B2), P(d.C2),
                                           P(d.As), P(d.Bs), P(d.Cs), P(dy2), P(dys), N, H, W, stream())
        res.append((dy2, dys))
    torch.cuda.synchronize()
    D.check(what)
    if not tail_supported(H, W, dt):
        assert rc == ERR_UNSUPPORTED, rc
        assert all(a.untouched() for k, a in D.arenas.items() if k.startswith("dy")), what
        return
    assert rc == 0, rc
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]), ("not bit-reproducible", what)
    ref = ref_tail_apply(c)
    amb_cap(ref.amb, what)
    r64 = lambda k: (lambda: (getattr(ref, k)[0] - getattr(ref_tail_apply(c, q=False), k)[0]).abs())
    for k, got in (("dy2", res[0][0]), ("dys", res[0][1])):
        v, e = getattr(ref, k)
        gd = nchw(got.cpu())
        assert torch.isfinite(gd).all(), what
        bound = e + half_ulp_bf16(v.abs() + e) if dt == "bf16" else e
        ratio = torch.where(ref.amb, torch.zeros_like(v), _ratio((gd - v).abs(), bound))
        gate(f"apply_{k}_{ref.path}", plane_slices(ratio), what, r64(k))


# ================================================================ GPU: the block's backward in one pass
def run_upblock_bwd(L, D, c, d, rep):
    lib = L.lib()
    o = types.SimpleNamespace()
    N = c.N
    o.dw2, o.dwu, o.dw1 = D.put(f"dw2_{rep}", c.pre[0]), D.put(f"dwu_{rep}", c.pre[1]), D.put(f"dw1_{rep}", c.pre[2])
    o.da1 = D.put(f"da1_{rep}", ((N, 32, 32, 16), torch.bfloat16), 0xFF)
    o.gin = D.put(f"gin_{rep}", ((N, 32, 32, 16), torch.bfloat16), 0xFF)
    o.sums = D.put(f"sums_{rep}", ((2, 16), torch.float32), 0xFF)
    L.check(lib.mmvae_upblock_bwd_fused(P(d.d_raw), P(d.w), P(d.y2), P(d.s2), P(d.b2), P(d.ys), P(d.ss), P(d.bs), P(d.A2), P(d.B2), P(d.C2), P(d.As), P(d.Bs),
                                        P(d.Cs), P(d.y1), P(d.s1), P(d.b1), P(d.w2), P(o.dw2), P(o.da1), P(o.sums), P(d.xin), P(d.sx), P(d.bx), P(d.wu),
                                        P(o.dwu), P(o.gin), N, d.scratch, stream()), "upblock_bwd_fused")
    o.gin0 = o.gin.clone()
    L.check(lib.mmvae_conv1x1_bwd_fused(P(o.da1), P(d.y1), P(d.s1), P(d.b1), P(d.A1), P(d.B1), P(d.C1), P(d.xin), P(d.sx), P(d.bx), P(d.w1), P(o.dw1), P(o.gin),
                                        N * 32, d.scratch, stream()), "conv1x1_bwd_fused")
    return o


@gpu
@pytest.mark.parametrize("pro_x", [False, True])
@pytest.mark.parametrize("N", BWD_N)
def test_upblock_bwd_fused_f64(N, pro_x):
    L = _L()
    what = f"upblock_bwd N={N} pro_x={pro_x}"
    c = make_upblock(N, pro_x)
    ref = ref_upblock_bwd(c)
    amb_cap(ref.amb, what)
    D = Dev()
    d = join_dev(D, c)
    d.y1, d.xin = D.put("y1", nhwc(c.y1, "bf16")), D.put("xin", nhwc(c.xin, "bf16"))
    for k in ("s1", "b1", "sx", "bx", "w2", "wu", "w1", "A1", "B1", "C1"):
        setattr(d, k, D.put(k, getattr(c, k)))
    d.scratch = D.scratch("scratch", _header_macro("MMVAE_WGRAD_SCRATCH_BYTES"))
    o, o2 = run_upblock_bwd(L, D, c, d, 0), run_upblock_bwd(L, D, c, d, 1)
    torch.cuda.synchronize()
    D.check(what)
    for k in ("dw2", "dwu", "dw1", "da1", "gin", "gin0", "sums"):
        assert same_bits(getattr(o, k), getattr(o2, k)), ("not bit-reproducible", k, what)
    r64 = {}

    def storage(f):
        def go():
            if "r" not in r64:
                r64["r"] = ref_upblock_bwd(c, q=False)
            return f(r64["r"])
        return go
    # data gradients (bf16 stores of the f32 accumulators)
    for name, got, (v, e), k in (("upbwd_d_a1", o.da1, ref.da1, "da1"), ("upbwd_g_in_up", o.gin0, ref.gin0, "gin0")):
        gd = nchw(got.cpu())
        assert torch.isfinite(gd).all(), (name, what)
        gate(name, plane_slices(_ratio((gd - v).abs(), e + half_ulp_bf16(v.abs() + e))), what, storage(lambda r, k=k, v=v: (v - getattr(r, k)[0]).abs()))
    gate("upbwd_bn1_sums", _ratio((o.sums.cpu().double() - ref.sums).abs(), ref.bsums), what, storage(lambda r: (ref.sums - r.sums).abs()))
    for name, got, (v, e, _), i in (("upbwd_dw_conv2", o.dw2, ref.dw[0], 0), ("upbwd_dw_up", o.dwu, ref.dw[1], 1)):
        gate(name, _ratio((got.cpu().double() - v).abs(), e), what, storage(lambda r, i=i, v=v: (v - r.dw[i][0]).abs()))
    # conv1 (1x1) from the d_a1 / g_in the first call left on the device
    r1 = ref_conv1x1_bwd(c, nchw(o.da1.cpu()), nchw(o.gin0.cpu()), c.pre[2])
    amb_cap(r1.amb, what)
    gd = nchw(o.gin.cpu())
    assert torch.isfinite(gd).all(), what
    gate("conv1_g_in", plane_slices(_ratio((gd - r1.gin).abs(), r1.egin + half_ulp_bf16(r1.gin.abs() + r1.egin))), what)
    gate("conv1_dw", _ratio((o.dw1.cpu().double().view(16, 16) - r1.dw).abs(), r1.bdw), what)


@gpu
@pytest.mark.parametrize("pro_x", [False, True])
def test_conv1x1_bwd_second_row_round(pro_x):
    """rows = 129 * 32 = 4128 > 4 x 1024: the first 32 waves walk a second row.  d_a1 / g_in are synthetic."""
    L = _L(); lib = L.lib()
    N = 129
    what = f"conv1x1_bwd rows={N * 32} pro_x={pro_x}"
    c = make_upblock(1, pro_x, seed=5)
    g = c.gen
    m1 = span(g)
    c.y1 = rnd(torch.randn(N, 16, 32, 32, generator=g) * m1.view(1, 16, 1, 1), "bf16")
    c.s1, c.b1 = bn_pair(g, m1)
    c.A1, c.B1, c.C1 = bwd_coefs(g, m1)
    c.xin = rnd(torch.randn(N, 16, 32, 32, generator=g) * (1 if pro_x else 0.5) + (0 if pro_x else 0.5), "bf16")
    if pro_x:
        c.sx, c.bx = bn_pair(g, torch.ones(16))
    da1 = rnd(torch.randn(N, 16, 32, 32, generator=g) * span(g).view(1, 16, 1, 1), "bf16")
    gin0 = rnd(torch.randn(N, 16, 32, 32, generator=g), "bf16")
    ref = ref_conv1x1_bwd(c, da1.double(), gin0.double(), c.pre[2])
    amb_cap(ref.amb, what)
    assert ref.gx == 1024
    D = Dev()
    y1, xin, da1d = D.put("y1", nhwc(c.y1, "bf16")), D.put("xin", nhwc(c.xin, "bf16")), D.put("da1", nhwc(da1, "bf16"))
    s1, b1, A1, B1, C1, sx, bx, w1 = (D.put(k, getattr(c, k)) for k in ("s1", "b1", "A1", "B1", "C1", "sx", "bx", "w1"))
    sc = D.scratch("scratch", _header_macro("MMVAE_WGRAD_SCRATCH_BYTES"))
    res = []
    for rep in range(2):
        gin, dw1 = D.put(f"gin{rep}", nhwc(gin0, "bf16")), D.put(f"dw1_{rep}", c.pre[2])
        L.check(lib.mmvae_conv1x1_bwd_fused(P(da1d), P(y1), P(s1), P(b1), P(A1), P(B1), P(C1), P(xin), P(sx), P(bx), P(w1), P(dw1), P(gin), N * 32, sc, stream()), what)
        res.append((gin, dw1))
    torch.cuda.synchronize()
    D.check(what)
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]), ("not bit-reproducible", what)
    gd = nchw(res[0][0].cpu())
    gate("conv1_g_in", plane_slices(_ratio((gd - ref.gin).abs(), ref.egin + half_ulp_bf16(ref.gin.abs() + ref.egin))), what)
    gate("conv1_dw", _ratio((res[0][1].cpu().double().view(16, 16) - ref.dw).abs(), ref.bdw), what)


# ================================================================ GPU: steady state of the three stream kernels (capped grids)
def _chunks(N, n):
    return [(i, min(N, i + n)) for i in range(0, N, n)]


@gpu
def test_tail_join_fwd_stream_steady_state():
    """N = 769: 3076 units, 768 x 4 = 3072 <= 3076: the capped grid of 768 blocks, eight chunks of 385 units over 96 blocks each -- every wave
    walks one unit, one wave of each chunk a second.  Inputs are drawn on the device and the float64 reference is evaluated there in chunks of
    images (plain tensor arithmetic, see conv_g), so the ambiguity cap of this case is asserted here and not in the CPU self-check."""
    L = _L(); lib = L.lib()
    N = 769
    what = f"tail_join_fwd_stream N={N}"
    assert tail_fwd_stream_grid(N) == 768
    c = make_join(N, 64, 64, 1, "bf16", dev=True)
    D = Dev()
    d = join_dev(D, c)
    res = []
    for rep in range(2):
        r = D.put(f"r{rep}", ((N, 64, 64), torch.float32), 0xFF)
        stats = D.put(f"stats{rep}", ((N + 4, 2), torch.float32), 0xFF)
        rows = L.check(lib.mmvae_tail_join_fwd_stream(1, P(d.y2), P(d.s2), P(d.b2), P(d.ys), P(d.ss), P(d.bs), P(d.w), P(d.bias), P(r), P(stats), N, 64, 64,
                                                      stream()), what)
        res.append((r, stats))
    torch.cuda.synchronize()
    D.check(what)
    assert rows == 768
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]), ("not bit-reproducible", what)
    namb, sv, sb, depth = 0, 0, 0, None
    for n0, n1 in _chunks(N, 64):
        ref = ref_tail_fwd_stream(sub(c, n0, n1), total=N)
        namb += int(ref.amb.sum())
        got = res[0][0][n0:n1].double()
        gate("stream_fwd_r", plane_slices(_ratio((got - ref.r).abs(), ref.e)[:, None]), f"{what} images {n0}..{n1 - 1}")
        sv, sb, depth = sv + ref.stats[0].cpu(), sb + ref.stats[1].cpu(), ref.depth
    assert namb <= 1e-3 * c.y2.numel(), namb
    check_stats_rows("stream_fwd_stats", res[0][1], rows, N + 4, (sv, sb), what, res[0][0].cpu(), depth)


@gpu
def test_upblock_tail_fwd_steady_state():
    """N = 1025: 2050 units, 512 x 4 = 2048 <= 2050: the capped grid of 512 blocks, chunks of 257 units over 64 blocks (256 waves) each."""
    L = _L(); lib = L.lib()
    N = 1025
    what = f"upblock_tail_fwd N={N}"
    assert up5_grid(N) == 512
    c = make_upblock(N, True, dev=True)
    D = Dev()
    d = join_dev(D, c)
    y1, xin = D.put("y1", nhwc(c.y1, "bf16")), D.put("xin", nhwc(c.xin, "bf16"))
    s1, b1, sx, bx, w2, wu = (D.put(k, getattr(c, k)) for k in ("s1", "b1", "sx", "bx", "w2", "wu"))
    sc = D.scratch("scratch", 16 << 10)
    res = []
    for rep in range(2):
        r = D.put(f"r{rep}", ((N, 64, 64), torch.float32), 0xFF)
        stats = D.put(f"stats{rep}", ((N + 4, 2), torch.float32), 0xFF)
        rows = L.check(lib.mmvae_upblock_tail_fwd(P(y1), P(s1), P(b1), P(w2), P(xin), P(sx), P(bx), P(wu), P(d.s2), P(d.b2), P(d.ss), P(d.bs), P(d.w), P(d.bias),
                                                  P(r), P(stats), N, sc, stream()), what)
        res.append((r, stats))
    torch.cuda.synchronize()
    D.check(what)
    assert rows == 512
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]), ("not bit-reproducible", what)
    namb, nel, sv, sb, depth = 0, 0, 0, 0, None
    for n0, n1 in _chunks(N, 64):
        ref = ref_up5_tail_fwd(sub(c, n0, n1), total=N)
        namb, nel = namb + int(ref.amb.sum()), nel + ref.amb.numel()
        got = res[0][0][n0:n1].double()
        gate("up5_fwd_r", plane_slices(_ratio((got - ref.r).abs(), ref.e)[:, None]), f"{what} images {n0}..{n1 - 1}")
        sv, sb, depth = sv + ref.stats[0].cpu(), sb + ref.stats[1].cpu(), ref.depth
    assert namb <= 1e-3 * nel, namb
    check_stats_rows("up5_fwd_stats", res[0][1], rows, N + 4, (sv, sb), what, res[0][0].cpu(), depth)


@gpu
def test_upblock_bwd_fused_steady_state():
    """N = 1025: the capped grid of 512 blocks x 2 pairs, chunks of ceil(1025 / 8) = 129 images over 128 pair slots: one pair of every chunk
    walks two images.  conv1_bwd_stream: 32 800 rows, 1024 blocks, eight or nine rows a wave."""
    L = _L()
    N = 1025
    what = f"upblock_bwd N={N}"
    assert join_bwd_grid(N) == 512 and conv1_bwd_grid(N * 32) == 1024
    c = make_upblock(N, True, dev=True)
    D = Dev()
    d = join_dev(D, c)
    d.y1, d.xin = D.put("y1", nhwc(c.y1, "bf16")), D.put("xin", nhwc(c.xin, "bf16"))
    for k in ("s1", "b1", "sx", "bx", "w2", "wu", "w1", "A1", "B1", "C1"):
        setattr(d, k, D.put(k, getattr(c, k)))
    d.scratch = D.scratch("scratch", _header_macro("MMVAE_WGRAD_SCRATCH_BYTES"))
    o, o2 = run_upblock_bwd(L, D, c, d, 0), run_upblock_bwd(L, D, c, d, 1)
    torch.cuda.synchronize()
    D.check(what)
    for k in ("dw2", "dwu", "dw1", "da1", "gin", "gin0", "sums"):
        assert same_bits(getattr(o, k), getattr(o2, k)), ("not bit-reproducible", k, what)
    namb, nel, bn, wg = 0, 0, [], []
    for n0, n1 in _chunks(N, 32):
        ch = upblock_bwd_chunk(sub(c, n0, n1))
        namb, nel = namb + int(ch.amb.sum()), nel + ch.amb.numel()
        for name, got, (v, e) in (("upbwd_d_a1", o.da1, ch.da1), ("upbwd_g_in_up", o.gin0, ch.gin0)):
            gd = nchw(got[n0:n1])
            gate(name, plane_slices(_ratio((gd - v).abs(), e + half_ulp_bf16(v.abs() + e))), f"{what} images {n0}..{n1 - 1}")
        bn.append(ch.bn)
        wg.append(ch.wg)
    assert namb <= 1e-3 * nel, namb
    sums, bsums, dw, gx = upblock_bwd_assemble(N, bn, wg, c.pre)
    gate("upbwd_bn1_sums", _ratio((o.sums.cpu().double() - sums).abs(), bsums), what)
    for name, got, (v, e, _) in (("upbwd_dw_conv2", o.dw2, dw[0]), ("upbwd_dw_up", o.dwu, dw[1])):
        gate(name, _ratio((got.cpu().double() - v).abs(), e), what)
    r1 = ref_conv1x1_bwd(c, nchw(o.da1), nchw(o.gin0), c.pre[2])
    amb_cap(r1.amb, what)
    gate("conv1_g_in", plane_slices(_ratio((nchw(o.gin) - r1.gin).abs(), r1.egin + half_ulp_bf16(r1.gin.abs() + r1.egin))), what)
    gate("conv1_dw", _ratio((o.dw1.double().view(16, 16) - r1.dw).abs(), r1.bdw), what)


# ================================================================ GPU: join + the next block's conv1
def make_jc(C, N, H):
    g = torch.Generator().manual_seed(C * 1000 + N)
    npix = N * H * H
    m2, ms = span(g, C), span(g, C)
    y2 = (torch.randn(npix, C, generator=g) * m2).to(torch.bfloat16)
    ys = (torch.randn(npix, C, generator=g) * ms).to(torch.bfloat16)
    sg = lambda: (torch.rand(C, generator=g) < 0.5).float() * 2 - 1
    s2, ss = sg() * (0.5 + torch.rand(C, generator=g)) / m2, sg() * (0.5 + torch.rand(C, generator=g)) / ms
    b2, bs = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.5
    w = torch.randn(16, C, generator=g) * 0.2 * span(g, C)
    return y2, s2, b2, ys, ss, bs, w, ref_join_conv1(y2, s2, b2, ys, ss, bs, w)


@gpu
@pytest.mark.parametrize("with_stats", [True, False])
@pytest.mark.parametrize("C,N,H", JC_CASES)
def test_join_conv1x1_fwd_f64(C, N, H, with_stats):
    L = _L(); lib = L.lib()
    what = f"join_conv1x1_fwd C={C} N={N} H={H} stats={with_stats}"
    y2, s2, b2, ys, ss, bs, w, ref = make_jc(C, N, H)
    amb_cap(ref.amb, what)
    npix = N * H * H
    D = Dev()
    y2d, ysd = D.put("y2", y2), D.put("ys", ys)
    s2d, b2d, ssd, bsd, wd = (D.put(k, t) for k, t in (("s2", s2), ("b2", b2), ("ss", ss), ("bs", bs), ("w", w.view(16, C, 1, 1))))
    sc = D.scratch("scratch", 2 << 10)
    res = []
    for rep in range(2):
        out = D.put(f"out{rep}", ((npix, C), torch.bfloat16), 0xFF)
        y1 = D.put(f"y1_{rep}", ((npix, 16), torch.bfloat16), 0xFF)
        stats = D.put(f"stats{rep}", ((1024, 2, 16), torch.float32), 0xFF)
        rows = L.check(lib.mmvae_join_conv1x1_fwd(P(y2d), P(s2d), P(b2d), P(ysd), P(ssd), P(bsd), P(wd), C, P(out), P(y1), P(stats) if with_stats else None, npix,
                                                  sc, stream()), what)
        res.append((out, y1, stats))
    torch.cuda.synchronize()
    D.check(what)
    assert rows == join_conv1_grid(npix), rows
    for a, b in zip(res[0], res[1]):
        assert same_bits(a, b), ("not bit-reproducible", what)
    out, y1, stats = res[0]
    planes = lambda t, ch: plane_slices(t.view(N, H, H, ch).permute(0, 3, 1, 2))        # per image x channel x {border ring, interior}
    go = out.cpu().double()
    assert torch.isfinite(go).all(), what
    ro = _ratio((go - ref.out).abs(), ref.eout + half_ulp_bf16(ref.out.abs() + ref.eout))
    gate("joinconv_out", planes(ro, C), what)
    g1 = y1.cpu().double()
    r1 = _ratio((g1 - ref.y1).abs(), ref.e1 + half_ulp_bf16(ref.y1.abs() + ref.e1))
    gate("joinconv_y1", planes(r1, 16), what)
    if not with_stats:
        assert D.arenas["stats0"].untouched(), what
        return
    host = stats.cpu()
    assert torch.isfinite(host[:rows]).all() and bool((stats[rows:].contiguous().view(torch.uint8) == 0xFF).all()), what
    got = host[:rows].double().sum(0)                                      # [2, 16]
    depth = 2 * -(-(npix // 32) // (4 * rows)) + 4 + 3                     # a lane's two pixels per step, row16_sum, the four waves in order
    v, e = ref.y1, ref.e1
    b0 = e.sum(0) + SLOP * U * depth * v.abs().sum(0)
    b1 = (2 * v.abs() * e + e * e).sum(0) + SLOP * U * (depth + 1) * (v * v).sum(0)
    gate("joinconv_stats", torch.stack([_ratio((got[0] - v.sum(0)).abs(), b0), _ratio((got[1] - (v * v).sum(0)).abs(), b1)]), what)


# ================================================================ GPU: refusals
@gpu
def test_refusals_leave_outputs_untouched():
    """NULL for each pointer an entry point checks, N = 0, rows = 0, sx without bx, npix not a multiple of 32, C = 24, unsupported tail geometry:
    a negative code, nothing enqueued, guarded outputs untouched.  Every other argument is a valid buffer."""
    L = _L(); lib = L.lib()
    c = make_upblock(1, True)
    D = Dev()
    d = join_dev(D, c)
    d.y1, d.xin = D.put("y1", nhwc(c.y1, "bf16")), D.put("xin", nhwc(c.xin, "bf16"))
    for k in ("s1", "b1", "sx", "bx", "w2", "wu", "w1", "A1", "B1", "C1"):
        setattr(d, k, D.put(k, getattr(c, k)))
    outs = Dev()
    o = types.SimpleNamespace()
    o.dw2, o.dwu, o.dw1 = outs.put("dw2", ((16, 16, 4, 4), torch.float32)), outs.put("dwu", ((16, 16, 4, 4), torch.float32)), outs.put("dw1", ((16, 16), torch.float32))
    o.da1, o.gin = outs.put("da1", ((1, 32, 32, 16), torch.bfloat16)), outs.put("gin", ((1, 32, 32, 16), torch.bfloat16))
    o.sums, o.r, o.stats = outs.put("sums", ((2, 16), torch.float32)), outs.put("r", ((1, 64, 64), torch.float32)), outs.put("stats", ((1024, 2, 16), torch.float32))
    o.out, o.y1o = outs.put("out", ((1024, 32), torch.bfloat16)), outs.put("y1o", ((1024, 16), torch.bfloat16))
    o.dy2, o.dys = outs.put("dy2", ((1, 64, 64, 16), torch.float32)), outs.put("dys", ((1, 64, 64, 16), torch.float32))
    o.part = outs.put("part", ((1024, 3, 16), torch.float32))
    sc = outs.scratch("scratch", _header_macro("MMVAE_WGRAD_SCRATCH_BYTES"))
    st = stream()

    def ubwd(N=1, **kw):
        a = dict(d_raw=P(d.d_raw), w=P(d.w), y2=P(d.y2), s2=P(d.s2), b2=P(d.b2), ys=P(d.ys), ss=P(d.ss), bs=P(d.bs), A2=P(d.A2), B2=P(d.B2), C2=P(d.C2), As=P(d.As),
                 Bs=P(d.Bs), Cs=P(d.Cs), y1=P(d.y1), s1=P(d.s1), b1=P(d.b1), w2=P(d.w2), dw2=P(o.dw2), da1=P(o.da1), sums=P(o.sums), xin=P(d.xin), sx=P(d.sx),
                 bx=P(d.bx), wu=P(d.wu), dwu=P(o.dwu), gin=P(o.gin), N=N, scratch=sc)
        a.update(kw)
        return lib.mmvae_upblock_bwd_fused(*a.values(), st)

    def c1(rows=32, **kw):
        a = dict(da1=P(d.y1), y1=P(d.y1), s1=P(d.s1), b1=P(d.b1), A1=P(d.A1), B1=P(d.B1), C1=P(d.C1), xin=P(d.xin), sx=P(d.sx), bx=P(d.bx), w1=P(d.w1), dw1=P(o.dw1),
                 gin=P(o.gin), rows=rows, scratch=sc)
        a.update(kw)
        return lib.mmvae_conv1x1_bwd_fused(*a.values(), st)

    def utf(N=1, **kw):
        a = dict(y1=P(d.y1), s1=P(d.s1), b1=P(d.b1), w2=P(d.w2), xin=P(d.xin), sx=P(d.sx), bx=P(d.bx), wu=P(d.wu), s2=P(d.s2), b2=P(d.b2), ss=P(d.ss), bs=P(d.bs),
                 tw=P(d.w), tb=P(d.bias), r=P(o.r), stats=P(o.stats), N=N, scratch=sc)
        a.update(kw)
        return lib.mmvae_upblock_tail_fwd(*a.values(), st)

    def jc(C=16, npix=1024, **kw):
        a = dict(y2=P(d.y2), s2=P(d.s2), b2=P(d.b2), ys=P(d.ys), ss=P(d.ss), bs=P(d.bs), w=P(d.w1), C=C, out=P(o.out), y1=P(o.y1o), stats=P(o.stats), npix=npix, scratch=sc)
        a.update(kw)
        return lib.mmvae_join_conv1x1_fwd(*a.values(), st)

    calls = []
    for k in ("scratch", "d_raw", "w", "y2", "ys", "y1", "xin", "w2", "wu", "dw2", "dwu", "da1", "gin", "sums"):
        calls.append((f"upblock_bwd_fused {k}=NULL", ubwd(**{k: None}), ERR_ARG))
    calls += [("upblock_bwd_fused N=0", ubwd(N=0), ERR_ARG), ("upblock_bwd_fused sx without bx", ubwd(bx=None), ERR_ARG),
              ("upblock_bwd_fused bx without sx", ubwd(sx=None), ERR_ARG)]
    for k in ("scratch", "da1", "y1", "s1", "b1", "A1", "B1", "C1", "xin", "w1", "dw1", "gin"):
        calls.append((f"conv1x1_bwd_fused {k}=NULL", c1(**{k: None}), ERR_ARG))
    calls += [("conv1x1_bwd_fused rows=0", c1(rows=0), ERR_ARG), ("conv1x1_bwd_fused sx without bx", c1(bx=None), ERR_ARG)]
    for k in ("scratch", "y1", "s1", "b1", "w2", "xin", "wu", "s2", "b2", "ss", "bs", "tw", "r"):
        calls.append((f"upblock_tail_fwd {k}=NULL", utf(**{k: None}), ERR_ARG))
    calls += [("upblock_tail_fwd N=0", utf(N=0), ERR_ARG), ("upblock_tail_fwd sx without bx", utf(bx=None), ERR_ARG)]
    for k in ("y2", "s2", "b2", "ys", "ss", "bs", "w", "out", "y1", "scratch"):
        calls.append((f"join_conv1x1_fwd {k}=NULL", jc(**{k: None}), ERR_ARG))
    calls += [("join_conv1x1_fwd npix=1000", jc(npix=1000), ERR_UNSUPPORTED), ("join_conv1x1_fwd npix=0", jc(npix=0), ERR_UNSUPPORTED),
              ("join_conv1x1_fwd C=24", jc(C=24), ERR_UNSUPPORTED)]
    # tail_join_*: W no power of two, W above the tile, H * W no multiple of the tile, a stream form off 64x64, wpartials with three planes
    tj = lambda fn, dt, H, W, *mid: fn(dt, *mid, 1, H, W, st)
    fwd_a = (P(d.y2), P(d.s2), P(d.b2), P(d.ys), P(d.ss), P(d.bs), P(d.w), P(d.bias), P(o.r), P(o.stats))
    red_a = lambda oc, wp: (P(d.d_raw), P(d.w), oc, P(d.y2), P(d.s2), P(d.b2), P(d.ys), P(d.ss), P(d.bs), P(o.part), wp)
    app_a = (P(d.d_raw), P(d.w), 1, P(d.y2), P(d.s2), P(d.b2), P(d.ys), P(d.ss), P(d.bs), P(d.A2), P(d.B2), P(d.C2), P(d.As), P(d.Bs), P(d.Cs), P(o.dy2), P(o.dys))
    for dt, H, W in ((1, 24, 24), (0, 4, 128), (1, 4, 8), (0, 2, 8)):
        calls.append((f"tail_join_fwd dt={dt} {H}x{W}", tj(lib.mmvae_tail_join_fwd, dt, H, W, *fwd_a), ERR_UNSUPPORTED))
        calls.append((f"tail_join_bwd_reduce dt={dt} {H}x{W}", tj(lib.mmvae_tail_join_bwd_reduce, dt, H, W, *red_a(1, None)), ERR_UNSUPPORTED))
        calls.append((f"tail_join_bwd_apply dt={dt} {H}x{W}", tj(lib.mmvae_tail_join_bwd_apply, dt, H, W, *app_a), ERR_UNSUPPORTED))
    calls.append(("tail_join_fwd_stream 32x32", tj(lib.mmvae_tail_join_fwd_stream, 1, 32, 32, *fwd_a), ERR_UNSUPPORTED))
    calls.append(("tail_join_fwd_stream f32", tj(lib.mmvae_tail_join_fwd_stream, 0, 64, 64, *fwd_a), ERR_UNSUPPORTED))
    calls.append(("tail_join_bwd_reduce wpartials with 3 planes", tj(lib.mmvae_tail_join_bwd_reduce, 1, 16, 16, *red_a(3, P(o.stats))), ERR_UNSUPPORTED))
    torch.cuda.synchronize()
    wrong = [(name, rc) for name, rc, want in calls if rc != want]
    assert not wrong, wrong
    touched = [k for k, a in outs.arenas.items() if not a.untouched()]
    assert not touched, ("a refused call wrote to", touched)
    D.check("refusals")


if __name__ == "__main__":
    for fn in (test_bf16_grid_helpers, test_launch_geometry, test_tapwise_convolutions_are_the_torch_ones, test_chunked_block_backward_is_the_whole_one,
               test_wgrad_reduce_order_sums_every_part_once, test_r64_is_autograd,
               test_rq_stays_close_to_r64_and_bounds_are_positive, test_ambiguous_share_within_cap):
        fn()
        print("ok", fn.__name__)
