"""GPU: the last up-block's forward with the branch outputs stored by the tail kernel (through the C ABI).

The training step used to run decoder.uplayer5's two ConvTranspose2d(16 -> 16, k4 s2 p1) as storing launches (mmvae_conv2d_fwd ->
convT4_stream_kernel: y2 / ys + their batch statistics) and then up5_tail_fwd_kernel, which recomputes both outputs for the join.  Now
  mmvae_convT4_stats             the same launch without its output: only the partial statistics rows
  mmvae_upblock_tail_fwd_store   mmvae_upblock_tail_fwd that also stores y2 / ys
Nothing numerical may change: the same accumulation in the same order, the same rounding.  So every comparison here is BIT equality against
the launches the step used until now (mmvae_conv2d_fwd, mmvae_upblock_tail_fwd) on the same device tensors -- no tolerances.

Shapes: N = 1 (almost every wave without a unit), 17 (34 tail units on a grid of 8 blocks, one of them empty), 1025 (2050 tail units on
512 x 4 wave slots, 4100 ConvTranspose2d units on 1024 x 4: a wave runs a second unit, so the rings are re-primed and the owned-row rule is
exercised across units), each with and without the block-input prologue.  y2 / ys sit between two guard images of a sentinel bit pattern
(a bf16 NaN no finite input can produce): the guards must survive and no element inside may keep the sentinel.
"""
import functools
import importlib
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

BF16, F32 = 1, 0
ERR_ARG, ERR_UNSUPPORTED = -1, -4
SENTINEL = 0x7FA5                   # as int16: a bf16 NaN with a payload
CASES = [(N, pro_x) for N in (1, 17, 1025) for pro_x in (False, True)]


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _guarded(N):
    """[N + 2][64][64][16] int16 of the sentinel; the window is images 1 .. N"""
    return torch.full((N + 2, 64, 64, 16), SENTINEL, dtype=torch.int16, device="cuda")


@functools.lru_cache(maxsize=None)
def _case(N, pro_x):
    """Inputs on the device and the outputs of the launches the step used until now (computed once per case, never written again)."""
    L = _L(); lib = L.lib(); P = L.ptr
    g = torch.Generator(device="cuda").manual_seed(7700 + 2 * N + int(pro_x))
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")
    vec = lambda lo, hi: torch.rand(16, generator=g, device="cuda") * (hi - lo) + lo
    c = types.SimpleNamespace(N=N, pro_x=pro_x)
    c.y1, c.xin = rnd(N, 32, 32, 16).to(torch.bfloat16), rnd(N, 32, 32, 16).to(torch.bfloat16)
    c.s1, c.b1 = vec(0.5, 1.5), vec(-0.3, 0.3)
    c.sx, c.bx = (vec(0.5, 1.5), vec(-0.3, 0.3)) if pro_x else (None, None)
    c.w2, c.wu = rnd(16, 16, 4, 4) / 8.0, rnd(16, 16, 4, 4) / 8.0
    c.s2, c.ss, c.b2, c.bs = vec(0.5, 1.5), vec(0.5, 1.5), vec(-0.3, 0.3), vec(-0.3, 0.3)
    c.tw, c.tb = rnd(1, 16, 3, 3) / 12.0, rnd(1)
    c.scratch = torch.empty(65536, dtype=torch.uint8, device="cuda")
    # the storing ConvTranspose2d launches
    c.y2 = torch.empty(N, 64, 64, 16, dtype=torch.bfloat16, device="cuda")
    c.ys = torch.empty_like(c.y2)
    c.st2 = torch.full((1024, 2, 16), float("nan"), device="cuda")
    c.sts = torch.full((1024, 2, 16), float("nan"), device="cuda")
    c.rows2 = L.check(lib.mmvae_conv2d_fwd(BF16, 1, P(c.y1), P(c.w2), P(c.y2), N, 32, 32, 16, 16, 4, 2, 1, P(c.s1), P(c.b1), 1, P(c.st2),
                                           P(c.scratch), _stream()), "conv2d_fwd conv2")
    c.rowss = L.check(lib.mmvae_conv2d_fwd(BF16, 1, P(c.xin), P(c.wu), P(c.ys), N, 32, 32, 16, 16, 4, 2, 1, P(c.sx), P(c.bx), 1 if pro_x else 0,
                                           P(c.sts), P(c.scratch), _stream()), "conv2d_fwd upsample")
    # the tail kernel that stores nothing
    c.r = torch.full((N, 64, 64), float("nan"), device="cuda")
    c.str = torch.full((512, 2), float("nan"), device="cuda")
    c.rowsr = L.check(lib.mmvae_upblock_tail_fwd(P(c.y1), P(c.s1), P(c.b1), P(c.w2), P(c.xin), P(c.sx), P(c.bx), P(c.wu), P(c.s2), P(c.b2), P(c.ss),
                                                 P(c.bs), P(c.tw), P(c.tb), P(c.r), P(c.str), N, P(c.scratch), _stream()), "upblock_tail_fwd")
    torch.cuda.synchronize()
    assert 0 < c.rows2 <= 1024 and 0 < c.rowss <= 1024 and 0 < c.rowsr <= 512
    return c


def _store(c):
    L = _L(); lib = L.lib(); P = L.ptr
    o = types.SimpleNamespace(y2=_guarded(c.N), ys=_guarded(c.N), r=torch.full((c.N, 64, 64), float("nan"), device="cuda"),
                              stats=torch.full((512, 2), float("nan"), device="cuda"))
    o.rows = L.check(lib.mmvae_upblock_tail_fwd_store(P(c.y1), P(c.s1), P(c.b1), P(c.w2), P(c.xin), P(c.sx), P(c.bx), P(c.wu), P(c.s2), P(c.b2),
                                                      P(c.ss), P(c.bs), P(c.tw), P(c.tb), P(o.r), P(o.stats), P(o.y2[1]), P(o.ys[1]), c.N,
                                                      P(c.scratch), _stream()), "upblock_tail_fwd_store")
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("N,pro_x", CASES)
def test_statistics_only_convT_rows_are_those_of_the_storing_launch(N, pro_x):
    """mmvae_convT4_stats: the row count and the partial rows of mmvae_conv2d_fwd, bit for bit (conv2 always has its BatchNorm + ReLU prologue;
    the upsample has one with pro_x)."""
    L = _L(); lib = L.lib(); P = L.ptr
    c = _case(N, pro_x)
    for what, x, w, ps, pb, rows_ref, st_ref in (("conv2", c.y1, c.w2, c.s1, c.b1, c.rows2, c.st2), ("upsample", c.xin, c.wu, c.sx, c.bx, c.rowss, c.sts)):
        st = torch.full((1024, 2, 16), float("nan"), device="cuda")
        rows = L.check(lib.mmvae_convT4_stats(BF16, P(x), P(w), P(ps), P(pb), P(st), N, 0, P(c.scratch), _stream()), "convT4_stats " + what)
        torch.cuda.synchronize()
        assert rows == rows_ref, (what, rows, rows_ref)
        assert not torch.isnan(st[:rows]).any(), what
        assert same_bits(st[:rows], st_ref[:rows]), what
        assert torch.isnan(st[rows:]).all(), (what, "rows past the returned count were written")


@pytest.mark.parametrize("N,pro_x", CASES)
def test_storing_tail_writes_the_branch_outputs_bit_exactly(N, pro_x):
    """mmvae_upblock_tail_fwd_store: y2 / ys are those of mmvae_conv2d_fwd, r_raw and its statistics those of mmvae_upblock_tail_fwd, the guard
    images keep the sentinel, no element inside does, and a second launch gives the same bits."""
    c = _case(N, pro_x)
    a, b = _store(c), _store(c)
    for o in (a, b):
        assert o.rows == c.rowsr
        for name, got, ref in (("y2", o.y2, c.y2), ("ys", o.ys, c.ys)):
            assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), (name, "guard image overwritten")
            assert not (got[1:-1] == SENTINEL).any(), (name, "an owned row was not written")
            bad = (got[1:-1] != _bits(ref)).flatten(1).any(1).nonzero().flatten()[:8].tolist()
            assert same_bits(got[1:-1], ref), (name, "first differing images", bad)
        assert same_bits(o.r, c.r), "r_raw"
        assert same_bits(o.stats[:o.rows], c.str[:o.rows]), "statistics rows"
        assert torch.isnan(o.stats[o.rows:]).all()
    assert same_bits(a.y2, b.y2) and same_bits(a.ys, b.ys) and same_bits(a.r, b.r) and same_bits(a.stats[:a.rows], b.stats[:b.rows]), "not bit-reproducible"


def test_refusals_launch_nothing():
    """The statistics-only form exists for bf16 without e4m3 storage only; the storing tail needs both outputs.  Each refusal is an error code and
    leaves the output buffers untouched."""
    L = _L(); lib = L.lib(); P = L.ptr
    c = _case(1, True)
    st = torch.full((1024, 2, 16), float("nan"), device="cuda")
    xf = c.y1.float()
    calls = [("e4m3", lib.mmvae_convT4_stats(BF16, P(c.y1), P(c.w2), P(c.s1), P(c.b1), P(st), 1, 1, P(c.scratch), _stream()), ERR_UNSUPPORTED),
             ("f32", lib.mmvae_convT4_stats(F32, P(xf), P(c.w2), P(c.s1), P(c.b1), P(st), 1, 0, P(c.scratch), _stream()), ERR_UNSUPPORTED),
             ("dtype 7", lib.mmvae_convT4_stats(7, P(c.y1), P(c.w2), P(c.s1), P(c.b1), P(st), 1, 0, P(c.scratch), _stream()), ERR_UNSUPPORTED),
             ("stats NULL", lib.mmvae_convT4_stats(BF16, P(c.y1), P(c.w2), P(c.s1), P(c.b1), None, 1, 0, P(c.scratch), _stream()), ERR_ARG),
             ("scale without shift", lib.mmvae_convT4_stats(BF16, P(c.y1), P(c.w2), P(c.s1), None, P(st), 1, 0, P(c.scratch), _stream()), ERR_ARG)]
    y2, ys = _guarded(1), _guarded(1)
    r = torch.full((1, 64, 64), float("nan"), device="cuda")
    for k in ("y2", "ys"):
        py2, pys = (None if k == "y2" else P(y2[1])), (None if k == "ys" else P(ys[1]))
        calls.append((k + " NULL", lib.mmvae_upblock_tail_fwd_store(P(c.y1), P(c.s1), P(c.b1), P(c.w2), P(c.xin), P(c.sx), P(c.bx), P(c.wu), P(c.s2),
                                                                    P(c.b2), P(c.ss), P(c.bs), P(c.tw), P(c.tb), P(r), None, py2, pys, 1,
                                                                    P(c.scratch), _stream()), ERR_ARG))
    torch.cuda.synchronize()
    for what, rc, want in calls:
        assert rc == want, (what, rc, want)
    assert torch.isnan(st).all() and torch.isnan(r).all() and (y2 == SENTINEL).all() and (ys == SENTINEL).all()
