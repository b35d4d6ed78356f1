"""No GPU: the host side of the latent diagnostics -- scatter_tone, the C ABI declarations / bindings of mmvae_scatter_panel and
mmvae_latent_stats, the argument errors both refuse before anything is launched, and the torch reference of the coverage rule that
tests/test_latent_diag_gpu.py compares the kernel with, checked here against a brute-force double loop in Python integers."""
import importlib
import math
import os
import re
import struct

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -4


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


# ================================================================ the reference of the coverage rule
def scatter_q(x, y, xform):
    """The two f32 expressions of mmvae_scatter_panel on the CPU (every torch f32 operation is correctly rounded, an add then a
    multiply), then int64: (qx, qy, keep).  A point whose f32 result is not finite is dropped; a finite one is clamped to +-2^40
    before the conversion (far outside every panel, so the coverage rule below drops it by itself)."""
    x, y, xform = x.float(), y.float(), xform.float().cpu()
    fx = torch.floor((x + xform[0]) * xform[2])
    fy = torch.floor((xform[1] - y) * xform[3])
    assert fx.dtype == torch.float32 and fy.dtype == torch.float32
    keep = torch.isfinite(fx) & torch.isfinite(fy)
    big = float(2 ** 40)
    return fx[keep].clamp(-big, big).to(torch.int64), fy[keep].clamp(-big, big).to(torch.int64), keep


def scatter_counts_ref(x, y, xform, side, r):
    """k(i, j) of the rule (16 j + 8 - qx)^2 + (16 i + 8 - qy)^2 <= r^2 as an int64 (side, side) tensor: every kept point offers
    the pixels of a box that contains its disc, the rule is tested in int64 and the covered pixels are counted with bincount."""
    qx, qy, _ = scatter_q(x, y, xform)
    w = torch.arange(2 * r // 16 + 2, dtype=torch.int64)                       # a disc touches at most 2r / 16 + 1 pixel columns
    j = (torch.div(qx - r - 8 + 15, 16, rounding_mode="floor"))[:, None, None] + w[None, None, :]
    i = (torch.div(qy - r - 8 + 15, 16, rounding_mode="floor"))[:, None, None] + w[None, :, None]
    dx, dy = 16 * j + 8 - qx[:, None, None], 16 * i + 8 - qy[:, None, None]
    cover = (dx * dx + dy * dy <= r * r) & (i >= 0) & (i < side) & (j >= 0) & (j < side)
    return torch.bincount((i * side + j).expand(cover.shape)[cover], minlength=side * side).view(side, side)


def scatter_ref(x, y, xform, side, r, tone):
    return tone.cpu()[scatter_counts_ref(x, y, xform, side, r).clamp(max=255)]


def _brute_counts(x, y, xform, side, r):
    xlim, ylim, sx, sy = (struct.unpack("f", struct.pack("f", float(v)))[0] for v in xform)

    def f32(v):
        try:
            return struct.unpack("f", struct.pack("f", v))[0]
        except OverflowError:                                                   # beyond f32's range: the rounded result is an infinity
            return math.copysign(math.inf, v)

    counts = [[0] * side for _ in range(side)]
    for px, py in zip(x.tolist(), y.tolist()):
        fx, fy = f32(f32(px + xlim) * sx), f32(f32(ylim - py) * sy)          # a double sum / product of two floats, rounded once to f32
        if not (math.isfinite(fx) and math.isfinite(fy)):
            continue
        qx, qy = math.floor(fx), math.floor(fy)
        for i in range(side):
            for j in range(side):
                counts[i][j] += (16 * j + 8 - qx) ** 2 + (16 * i + 8 - qy) ** 2 <= r * r
    return torch.tensor(counts, dtype=torch.int64)


@pytest.mark.parametrize("r", [12, 40, 128])
def test_reference_is_the_rule_on_a_16_by_16_panel(r):
    side = 16
    g = torch.Generator().manual_seed(r)
    lim = torch.tensor([3.0, 2.5])
    xform = torch.cat([lim, float(8 * side) / lim])
    x, y = torch.randn(60, generator=g) * 1.5, torch.randn(60, generator=g) * 1.5
    # the border, just outside it, far away, not finite, huge; and exact sub-pixel integers ((x + 3) * 128/3 lands on or next to one)
    extra_x = torch.tensor([-3.0, 3.0, 3.2, -3.3, 100.0, float("inf"), float("nan"), 3e38, -3e38, 0.0, 0.75, -1.5, 0.0])
    extra_y = torch.tensor([2.5, -2.5, 0.0, 2.7, 0.0, 0.0, 0.0, 0.0, 1.0, float("-inf"), 1.25, 0.0, 0.0])
    x, y = torch.cat([x, extra_x]), torch.cat([y, extra_y])
    got = scatter_counts_ref(x, y, xform, side, r)
    want = _brute_counts(x, y, xform, side, r)
    assert torch.equal(got, want)
    assert int(want.sum()) > 0 and int(want.max()) >= 2
    tone = torch.arange(255, -1, -1, dtype=torch.uint8)
    assert torch.equal(scatter_ref(x, y, xform, side, r, tone), tone[want.clamp(max=255)])


def test_reference_saturates_and_floors_the_f32_product():
    side, r = 16, 12
    xform = torch.tensor([8.0, 8.0, 16.0, 16.0])                                # q = (x + 8) * 16 exactly for multiples of 1/16
    x = torch.full((300,), -8.0 + 40 / 16.0)                                    # qx = 40: pixel column 2 (centre 40)
    y = torch.full((300,), 8.0 - 24 / 16.0)                                     # qy = 24: pixel row 1
    c = scatter_counts_ref(x, y, xform, side, r)
    assert int(c[1, 2]) == 300 and int(c.sum()) == 300
    tone = torch.arange(256, dtype=torch.uint8)
    assert int(scatter_ref(x, y, xform, side, r, tone)[1, 2]) == 255
    below = torch.nextafter(torch.tensor(-8.0 + 40 / 16.0), torch.tensor(-9.0))
    qx, _, _ = scatter_q(torch.stack([torch.tensor(-8.0 + 40 / 16.0), below]), torch.zeros(2), xform)
    assert qx.tolist() == [40, 39]


# ================================================================ scatter_tone
def test_scatter_tone(pkg):
    tone = pkg.scatter_tone()
    assert tone.dtype == torch.uint8 and tuple(tone.shape) == (256,) and not tone.is_cuda
    t = tone.tolist()
    assert t[0] == 255 and t[1] == 230
    assert all(a >= b for a, b in zip(t, t[1:])), "monotone"
    assert t[255] == round(255 * 0.9 ** 255)
    assert t[:6] == [round(255 * 0.9 ** k) for k in range(6)]
    assert pkg.scatter_tone(0.0).tolist() == [255] * 256
    assert pkg.scatter_tone(1.0).tolist() == [255] + [0] * 255
    assert pkg.scatter_tone(0.5).tolist()[:4] == [255, 128, 64, 32]
    with pytest.raises(ValueError):
        pkg.scatter_tone(1.5)


# ================================================================ C ABI
def test_header_declares_and_binding_binds_both_entry_points(pkg):
    L = _L()
    txt = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for name in ("mmvae_scatter_panel", "mmvae_latent_stats"):
        assert re.search(r"MMVAE_API\s+int\s+" + name + r"\s*\(", txt), name
        assert name in L.PROTOTYPES
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1]
    assert len(L.PROTOTYPES["mmvae_scatter_panel"][1]) == 12 and len(L.PROTOTYPES["mmvae_latent_stats"][1]) == 8
    assert L.lib().mmvae_abi_version() == 3 and "#define MMVAE_ABI_VERSION 3" in txt
    src = open(os.path.join(ROOT, "moving-mnist-vae_amd", "csrc", "Makefile")).read()
    assert "latent_diag.hip" in src


def _scatter_rc(n=10, stride=2, col_x=0, col_y=1, side=16, radius16=64, out_row_stride=None, pts=0x1000, xform=0x1000, tone=0x1000,
                out=0x1000):
    """mmvae_scatter_panel with made-up device addresses: every call here must be refused before they could be used."""
    L = _L()
    rc = L.lib().mmvae_scatter_panel(pts, n, stride, col_x, col_y, xform, side, radius16, tone, out,
                                     side if out_row_stride is None else out_row_stride, None)
    return rc, (L.lib().mmvae_last_error() or b"").decode()


def test_scatter_panel_refuses_bad_arguments_before_any_launch(pkg):
    for side in (8, 24, 528, 0, -16):
        rc, msg = _scatter_rc(side=side)
        assert rc == ERR_UNSUPPORTED and "side=%d" % side in msg, side
    for radius16 in (11, 129, 0):
        rc, msg = _scatter_rc(radius16=radius16)
        assert rc == ERR_UNSUPPORTED and "radius16=%d" % radius16 in msg, radius16
    assert _scatter_rc(col_x=2)[0] == ERR_ARG                                   # col_x >= stride
    assert _scatter_rc(col_y=2)[0] == ERR_ARG
    assert _scatter_rc(col_x=-1)[0] == ERR_ARG
    assert _scatter_rc(stride=0, col_x=0, col_y=0)[0] == ERR_ARG
    rc, msg = _scatter_rc(side=32, out_row_stride=31)
    assert rc == ERR_ARG and "out_row_stride" in msg
    assert _scatter_rc(n=-1)[0] == ERR_ARG
    for null in ("pts", "xform", "tone", "out"):
        assert _scatter_rc(**{null: None})[0] == ERR_ARG, null


def test_latent_stats_refuses_bad_arguments_before_any_launch(pkg):
    lib = _L().lib()
    A = 0x1000                                                                  # never dereferenced
    for d in (0, 513, -8):
        assert lib.mmvae_latent_stats(A, A, A, 4, d, 0, A, None) == ERR_UNSUPPORTED, d
        assert ("d=%d" % d) in lib.mmvae_last_error().decode()
    assert lib.mmvae_latent_stats(A, A, A, 0, 8, 0, A, None) == ERR_ARG         # N = 0
    assert lib.mmvae_latent_stats(A, A, A, -1, 8, 0, A, None) == ERR_ARG
    assert lib.mmvae_latent_stats(None, A, A, 4, 8, 0, A, None) == ERR_ARG      # no mu
    assert lib.mmvae_latent_stats(A, None, None, 4, 8, 0, None, None) == ERR_ARG        # no accumulator
    assert lib.mmvae_latent_stats(A, A, A, 4, 8, 2, A, None) == ERR_ARG         # accumulate is 0 or 1


# ================================================================ Python surface
def test_python_surface_refuses_before_any_launch(pkg):
    pts = torch.zeros(8, 4)
    with pytest.raises(ValueError, match="GPU"):
        pkg.scatter_panel(pts)
    with pytest.raises(ValueError, match="GPU"):
        pkg.scatter_plot(pts, "unused", 0, 0, save=False)
    m = importlib.import_module("moving-mnist-vae_amd.model").VAE(1, 32, 1, 2, 8, False, False)
    with pytest.raises(ValueError):
        pkg.latent_stats(m, None, None, None)


def test_new_names_are_exported_and_documented(pkg):
    for name in ("scatter_tone", "scatter_panel", "scatter_plot", "latent_stats"):
        assert callable(getattr(pkg, name)), name
    main = importlib.import_module("moving-mnist-vae_amd.main")
    assert "scatter_plot" in main.__doc__ and "the scatter plot and wandb stay" not in main.__doc__
    assert "matplotlib" in pkg.scatter_panel.__doc__
    import inspect
    for fn in (pkg.plot_vae, pkg.plot_pixelvae, pkg.make_plot_callback):
        assert inspect.signature(fn).parameters["scatter"].default is False
    assert inspect.signature(pkg.evaluate).parameters["latent_stats"].default is False
