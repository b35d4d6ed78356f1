"""GPU: the latent diagnostics -- mmvae_scatter_panel, mmvae_latent_stats and the Python surface on top of them (scatter_panel,
scatter_plot, the ``scatter=True`` sheets of the plot callback, latent_stats, evaluate(..., latent_stats=True)).

Scatter panel: EXACT byte equality with the torch reference of tests/test_latent_diag_cpu.py (the two f32 expressions in f32 on the
CPU, everything else in int64; that file checks it against a brute-force loop), both sides reading the same four xform floats.  The
tone table of the op tests is a permutation of 0..255, so every count up to the saturation at 255 shows in the byte.  The kernel's tile
is 32 x 32: side = 16 and 48 have a ragged last tile, side = 256 / 512 have 8 / 16 tiles per axis, and the constructed points sit on
every internal tile boundary.

Latent stats: per entry |device - reference| <= 1e-12 * sum over the images of the magnitudes of the entry's terms before any
cancellation (|mu|; mu^2; 0.5 (exp(lv) + mu^2 + |lv| + 1); exp(lv); |enc|; enc^2), the reference being the f64 formulas in torch on the
same f32 inputs.  Derivation: at most 5120 terms, each a few f64 roundings (2^-53 = 1.1e-16) of its magnitude, the device exp within a
couple of ulps, and a sum of n terms adds at most n 2^-53 times the sum of magnitudes: below 5120 * 1.1e-16 + ~1e-15 < 1e-12.  The gates
of tests/test_eval_ops_gpu.py for the per-image KL have the same form.  Worst error / bound ratio measured on the MI355X: 0.0008
((5120, 512), the encoding rows)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_latent_diag_cpu import scatter_counts_ref, scatter_ref  # noqa: E402
from test_panels_cpu import _decode_png_gray  # noqa: E402

gpu = pytest.mark.gpu
TILE = 32                      # the kernel's tile side (csrc/latent_diag.hip)


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _tone():
    """A permutation of 0..255: no two counts share a byte."""
    return torch.tensor([(k * 37 + 11) % 256 for k in range(256)], dtype=torch.uint8)


def _xform(xlim, ylim, side):
    lim = torch.tensor([xlim, ylim], dtype=torch.float32)
    return torch.cat([lim, float(8 * side) / lim])


def _embed(x, y, stride, col_x, col_y):
    """(n, stride) f32 rows holding the points in two columns and NaN everywhere else (a read of another column would drop the point)."""
    pts = torch.full((x.numel(), stride), float("nan"), dtype=torch.float32)
    pts[:, col_x], pts[:, col_y] = x, y
    return pts


def _panel(pts, col_x, col_y, xform, side, r, tone, out=None, row_stride=None):
    """One mmvae_scatter_panel launch through the C ABI on device copies; returns the (side, side) device tensor it wrote."""
    L = _L()
    n, stride = pts.shape
    d_pts, d_x, d_t = pts.cuda().contiguous(), xform.cuda().contiguous(), tone.cuda().contiguous()
    if out is None:
        out = torch.full((side, side), 0x5A, dtype=torch.uint8, device="cuda")
    rc = L.lib().mmvae_scatter_panel(d_pts.data_ptr() if n else None, n, stride, col_x, col_y, d_x.data_ptr(), side, r, d_t.data_ptr(),
                                     out.data_ptr(), side if row_stride is None else row_stride, _st())
    assert rc == 0, L.lib().mmvae_last_error()
    torch.cuda.synchronize()
    return out


def _pool(side, r, xlim, ylim, seed):
    """5000 points for a panel: a Gaussian cloud around the middle, a wide one that reaches past the border, and the special values."""
    g = torch.Generator().manual_seed(seed)
    n = 5000
    x = torch.randn(n, generator=g) * (xlim / 4)
    y = torch.randn(n, generator=g) * (ylim / 4)
    wide = torch.arange(n) % 5 == 0
    x[wide], y[wide] = x[wide] * 5, y[wide] * 5                                 # sigma 1.25 lim: a good share outside the panel
    special = torch.tensor([float("inf"), float("-inf"), float("nan"), 3e38, -3e38, 1e9, -1e9, xlim, -xlim, 0.0])
    for k, v in enumerate(special.tolist()):                                    # at 11 k + 3: inside n = 63 from k = 5 on, all inside n = 257
        x[11 * k + 3] = v
        y[11 * k + 7] = v
    return x, y


# ------------------------------------------------------------------------------------------ sizes and strides
#          n     side (stride, col_x, col_y) radius16
SWEEP = [(0, 16, (2, 0, 1), 12), (1, 16, (2, 0, 1), 12), (63, 48, (8, 0, 1), 64), (64, 48, (32, 5, 2), 128), (65, 16, (8, 0, 1), 128),
         (257, 48, (2, 0, 1), 12), (5000, 256, (32, 5, 2), 64), (5000, 256, (2, 0, 1), 128), (5000, 48, (8, 0, 1), 12),
         (257, 256, (8, 0, 1), 64), (1, 256, (32, 5, 2), 128), (0, 256, (8, 0, 1), 64), (63, 16, (32, 5, 2), 64), (64, 256, (2, 0, 1), 12),
         (65, 48, (2, 0, 1), 64), (257, 16, (32, 5, 2), 12), (5000, 16, (2, 0, 1), 64), (64, 16, (8, 0, 1), 12), (63, 256, (2, 0, 1), 128),
         (65, 256, (32, 5, 2), 12), (257, 512, (8, 1, 0), 128), (1025, 48, (2, 1, 0), 64)]


@gpu
@pytest.mark.parametrize("n,side,cols,r", SWEEP)
def test_scatter_panel_sweep(pkg, n, side, cols, r):
    stride, col_x, col_y = cols
    xlim, ylim = 8.5, 7.25
    xform = _xform(xlim, ylim, side)
    x, y = _pool(side, r, xlim, ylim, seed=side + r)
    if n > x.numel():
        x, y = x.repeat(2), y.repeat(2)
    x, y = x[:n], y[:n]
    tone = _tone()
    got = _panel(_embed(x, y, stride, col_x, col_y), col_x, col_y, xform, side, r, tone).cpu()
    counts = scatter_counts_ref(x, y, xform, side, r)
    want = tone[counts.clamp(max=255)]
    bad = int((got != want).sum())
    print(f"scatter n={n} side={side} cols={cols} r={r}: max count {int(counts.max()) if n else 0}, {bad} bytes differ")
    assert torch.equal(got, want)
    if n == 0:
        assert (got == tone[0]).all()
    if n >= 257:
        assert int(counts.max()) >= 2                                           # discs overlap: the counts are not just 0 / 1


# ------------------------------------------------------------------------------------------ constructed inputs
def _constructed(side, r, xlim, ylim):
    """Points named by their sub-pixel position (qx, qy): with power-of-two limits and side, (x + xlim) * sx is exact."""
    sx, sy = 8.0 * side / xlim, 8.0 * side / ylim
    full = 16 * side
    edge = [0, 1, 7, 8, 15, 16, full - 16, full - 8, full - 1, full]            # on the border (0 and 16 side) and just inside it
    outside = [-r - 9, -r - 8, -r - 7, -r, -r // 2, -1, full + 1, full + r // 2, full + r + 7, full + r + 8, full + r + 9]
    tiles = [16 * TILE * k + o for k in range(1, side // TILE + 1) for o in (-r - 8, -r - 7, -9, -8, -1, 0, 7, 8, r + 7, r + 8)
             if 16 * TILE * k < full]
    qs = sorted(set(edge + outside + tiles))
    mid = [full // 2 + 3, full // 2 - 8]
    q = [(a, b) for a in qs for b in mid] + [(b, a) for a in qs for b in mid]
    q += [(a, b) for a in edge[:3] + outside + edge[-3:] for b in edge[:3] + outside + edge[-3:]]            # every corner
    q += [(a, a) for a in tiles] + [(a, full - a) for a in tiles]                                          # tile corners
    qx = torch.tensor([a for a, _ in q], dtype=torch.float64)
    qy = torch.tensor([b for _, b in q], dtype=torch.float64)
    x, y = (qx / sx - xlim).float(), (ylim - qy / sy).float()
    return x, y, qx.long(), qy.long()


@gpu
@pytest.mark.parametrize("side,r", [(16, 12), (48, 64), (256, 128), (256, 12), (512, 40)])
def test_scatter_panel_constructed_points(pkg, side, r):
    """Discs cut by every edge and corner of the panel and by every internal tile boundary; points far outside; inf, nan, +-3e38; 300
    coincident points (the count saturates at 255); sub-pixel coordinates that are exact integers, and their f32 neighbours below."""
    xlim, ylim = 8.0, 4.0                                                       # side / lim is a power of two at side 16, 256, 512
    xform = _xform(xlim, ylim, side)
    x, y, qx, qy = _constructed(side, r, xlim, ylim)
    if side != 48:                                                              # exact arithmetic: the reference's q is the constructed one
        fx = torch.floor((x + xform[0]) * xform[2]).long()
        fy = torch.floor((xform[1] - y) * xform[3]).long()
        assert torch.equal(fx, qx) and torch.equal(fy, qy)
    below_x = torch.nextafter(x, torch.full_like(x, -1e9))                      # an ulp to the left: q drops by one where x sits on an integer
    far = torch.tensor([1e6, -1e6, 1e30, -1e30, 3e38, -3e38, float("inf"), float("-inf"), float("nan"), 0.0, 0.0, 0.0, 0.0, 0.0])
    far_y = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 3e38, -3e38, float("inf"), float("-inf"), float("nan")])
    cx = torch.full((300,), (8 * side + 3) / (8.0 * side / xlim) - xlim)        # 300 coincident points at qx = 8 side + 3, mid-panel
    cy = torch.zeros(300)
    X = torch.cat([x, below_x, far, cx])
    Y = torch.cat([y, y, far_y, cy])
    tone = _tone()
    got = _panel(_embed(X, Y, 3, 2, 0), 2, 0, xform, side, r, tone).cpu()
    counts = scatter_counts_ref(X, Y, xform, side, r)
    assert int(counts.max()) >= 300
    assert torch.equal(got, tone[counts.clamp(max=255)])
    # the non-finite and far points alone leave an empty panel
    empty = _panel(_embed(far, far_y, 2, 0, 1), 0, 1, xform, side, r, tone).cpu()
    assert (empty == tone[0]).all()


@gpu
def test_scatter_panel_saturates_at_255(pkg):
    side, r = 16, 12
    xform = torch.tensor([8.0, 8.0, 16.0, 16.0])
    for n, byte in ((254, 254), (255, 255), (256, 255), (300, 255), (1500, 255)):
        x, y = torch.full((n,), -5.5), torch.full((n,), 6.5)                    # qx = 40, qy = 24: pixel (1, 2) and no other
        got = _panel(_embed(x, y, 2, 0, 1), 0, 1, xform, side, r, torch.arange(256, dtype=torch.uint8)).cpu()
        assert int(got[1, 2]) == byte and int(got.long().sum()) == byte, n


@gpu
@pytest.mark.parametrize("side", [48, 256])
def test_scatter_panel_writes_the_panel_and_nothing_else(pkg, side):
    """out_row_stride = 2 side + 32: the panel sits at an odd column offset inside a buffer pre-filled with 0xA5, 256 guard bytes in
    front of its first row and behind its last; every byte outside the panel must keep its value."""
    r, row_stride, col0, guard = 64, 2 * side + 32, side + 7, 256
    xform = _xform(8.5, 7.25, side)
    x, y = _pool(side, r, 8.5, 7.25, seed=3)
    tone = _tone()
    buf = torch.full((guard + side * row_stride + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    body = buf[guard:guard + side * row_stride].view(side, row_stride)
    view = body[:, col0:col0 + side]
    assert view.data_ptr() == buf.data_ptr() + guard + col0
    _panel(_embed(x, y, 2, 0, 1), 0, 1, xform, side, r, tone, out=view, row_stride=row_stride)
    assert torch.equal(view.cpu(), scatter_ref(x, y, xform, side, r, tone))
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[guard:guard + side * row_stride].view(side, row_stride)[:, col0:col0 + side] = False
    assert int(outside.sum()) == buf.numel() - side * side
    assert (buf[outside] == 0xA5).all()


@gpu
def test_scatter_panel_is_deterministic_and_order_free(pkg):
    side, r = 256, 64
    xform = _xform(8.5, 7.25, side)
    x, y = _pool(side, r, 8.5, 7.25, seed=9)
    tone = _tone()
    pts = _embed(x, y, 8, 0, 1)
    a = _panel(pts, 0, 1, xform, side, r, tone)
    b = _panel(pts, 0, 1, xform, side, r, tone)
    perm = torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(1))
    c = _panel(pts[perm], 0, 1, xform, side, r, tone)
    assert torch.equal(a, b) and torch.equal(a, c)


# ------------------------------------------------------------------------------------------ latent stats
def _stats_ref(mu, lv, enc):
    """(reference [6][d], magnitude [6][d]) in f64 on the CPU from the f32 inputs; absent inputs give zero rows."""
    d = mu.shape[1]
    z = torch.zeros(d, dtype=torch.float64)
    m = mu.double()
    ref, mag = [m.sum(0), (m * m).sum(0)], [m.abs().sum(0), (m * m).sum(0)]
    if lv is not None:
        l = lv.double()
        e = l.exp()
        ref += [(0.5 * (e + m * m - l - 1.0)).sum(0), e.sum(0)]
        mag += [(0.5 * (e + m * m + l.abs() + 1.0)).sum(0), e.sum(0)]
    else:
        ref += [z, z]
        mag += [z, z]
    if enc is not None:
        c = enc.double()
        ref += [c.sum(0), (c * c).sum(0)]
        mag += [c.abs().sum(0), (c * c).sum(0)]
    else:
        ref += [z, z]
        mag += [z, z]
    return torch.stack(ref), torch.stack(mag)


def _stats_call(mu, lv, enc, accumulate, acc):
    L = _L()
    N, d = mu.shape
    keep = [t.cuda().contiguous() if t is not None else None for t in (mu, lv, enc)]
    rc = L.lib().mmvae_latent_stats(L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(keep[2]), N, d, accumulate, acc.data_ptr(), _st())
    assert rc == 0, L.lib().mmvae_last_error()
    torch.cuda.synchronize()
    return acc


def _stats_inputs(N, d, seed):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(N, d, generator=g) * 1.5 + 0.3
    lv = torch.randn(N, d, generator=g) * 0.8 - 0.5
    lv[0, 0] = 0.0                                                              # exp(0) - 0 - 1 = 0: the KL term's cancellation
    enc = mu + torch.randn(N, d, generator=g) * (0.5 * lv).exp()
    return mu, lv, enc


def _stats_gate(name, got, ref, mag):
    err, bound = (got.cpu() - ref).abs(), 1e-12 * mag
    ratio = (err / bound.clamp_min(1e-300)).max().item() if bool((bound > 0).any()) else 0.0
    print(f"RATIO {name} {ratio:.4f}")
    assert (err <= bound).all(), (name, ratio)


@gpu
@pytest.mark.parametrize("N,d", [(1, 8), (3, 8), (64, 32), (257, 64), (5120, 512), (7, 13), (70, 1)])
@pytest.mark.parametrize("with_lv,with_enc", [(True, True), (True, False), (False, True), (False, False)])
def test_latent_stats_against_f64(pkg, N, d, with_lv, with_enc):
    mu, lv, enc = _stats_inputs(N, d, seed=N + d)
    lv, enc = (lv if with_lv else None), (enc if with_enc else None)
    acc = torch.full((6, d), float("nan"), dtype=torch.float64, device="cuda")  # accumulate = 0 overwrites
    got = _stats_call(mu, lv, enc, 0, acc)
    ref, mag = _stats_ref(mu, lv, enc)
    _stats_gate(f"latent_stats[{N}x{d} lv={with_lv} enc={with_enc}]", got, ref, mag)
    if not with_lv:
        assert (got[2:4] == 0).all()
    if not with_enc:
        assert (got[4:6] == 0).all()
    again = _stats_call(mu, lv, enc, 0, torch.empty_like(acc))
    assert torch.equal(got, again)                                              # the bits depend on the inputs only


@gpu
@pytest.mark.parametrize("Na,Nb,d", [(3, 2, 8), (257, 64, 64), (100, 157, 13)])
def test_latent_stats_accumulates(pkg, Na, Nb, d):
    mu, lv, enc = _stats_inputs(Na + Nb, d, seed=5)
    acc = torch.zeros((6, d), dtype=torch.float64, device="cuda")
    _stats_call(mu[:Na], lv[:Na], enc[:Na], 1, acc)
    _stats_call(mu[Na:], lv[Na:], enc[Na:], 1, acc)
    one = _stats_call(mu, lv, enc, 0, torch.full((6, d), float("nan"), dtype=torch.float64, device="cuda"))
    ref, mag = _stats_ref(mu, lv, enc)
    _stats_gate("accumulated", acc, ref, mag)
    _stats_gate("one call", one, ref, mag)
    assert ((acc - one).abs().cpu() <= 1e-12 * mag).all()
    # accumulate = 0 overwrites whatever was there, NaN included; a missing input adds nothing to its rows
    before = acc.clone()
    _stats_call(mu[:Na], None, None, 1, acc)
    assert torch.equal(acc[2:], before[2:]) and not torch.equal(acc[:2], before[:2])
    wrote = _stats_call(mu[:Na], lv[:Na], enc[:Na], 0, torch.full((6, d), float("nan"), dtype=torch.float64, device="cuda"))
    assert torch.isfinite(wrote).all()


# ------------------------------------------------------------------------------------------ Python level
@gpu
def test_scatter_panel_python_surface(pkg):
    g = torch.Generator().manual_seed(4)
    enc = (torch.randn(128, 32, 1, 1, generator=g) * 1.3).cuda()
    panel = pkg.scatter_panel(enc)
    assert panel.dtype == torch.uint8 and panel.is_cuda and tuple(panel.shape) == (256, 256)
    flat = enc.view(128, 32).cpu()
    lim = flat[:, :2].abs().amax(0) + 4.0                                       # main.py:170-171
    xform = torch.cat([lim, float(8 * 256) / lim])
    tone = pkg.scatter_tone()
    assert torch.equal(panel.cpu(), scatter_ref(flat[:, 0], flat[:, 1], xform, 256, 64, tone))
    assert int(panel.min()) < 255 and int(panel[0, 0]) == 255                   # ink in the middle, white in the corner
    # other dimensions, explicit limits, a smaller panel and radius, a custom tone, rendering into half of a sheet
    sheet = torch.zeros((64, 128), dtype=torch.uint8, device="cuda")
    t2 = torch.arange(255, -1, -1, dtype=torch.uint8)
    out = pkg.scatter_panel(enc.view(128, 32), dims=(7, 3), lims=(6.0, 5.0), side=64, radius=1.5, tone=t2, out=sheet[:, 64:])
    assert out.data_ptr() == sheet[:, 64:].data_ptr() and (sheet[:, :64] == 0).all()
    want = scatter_ref(flat[:, 7], flat[:, 3], _xform(6.0, 5.0, 64), 64, 24, t2)
    assert torch.equal(sheet[:, 64:].cpu(), want)
    empty = pkg.scatter_panel(torch.zeros((0, 2), device="cuda"), side=16)
    assert (empty == 255).all()
    for bad in (dict(side=24), dict(side=528), dict(radius=0.5), dict(radius=9.0), dict(dims=(0, 32)), dict(tone=torch.zeros(16, dtype=torch.uint8)),
                dict(out=torch.zeros((256, 256), device="cuda")), dict(lims=(1.0, 2.0, 3.0))):
        with pytest.raises(ValueError):
            pkg.scatter_panel(enc, **bad)
    with pytest.raises(ValueError):
        pkg.scatter_panel(enc.double())


@gpu
def test_scatter_plot(pkg, tmp_path):
    """(N = 128, z = 32, 1, 1): the right half is scatter_panel(encoding), the left half scatter_panel of the returned prior points
    under the same limits, the PNG decodes to the sheet, the sheet is a function of the generator seed, save=False writes nothing."""
    enc = (torch.randn(128, 32, 1, 1, generator=torch.Generator().manual_seed(8)) * 0.7 + 0.2).cuda()
    gen = lambda s: torch.Generator(device="cuda").manual_seed(s)
    sheet, T = pkg.scatter_plot(enc, str(tmp_path), 3, 5, generator=gen(1), return_tensors=True)
    assert sheet.dtype == torch.uint8 and sheet.is_cuda and tuple(sheet.shape) == (256, 512)
    assert torch.equal(sheet[:, 256:], pkg.scatter_panel(enc))
    assert tuple(T["prior"].shape) == (128, 2) and tuple(T["xform"].shape) == (4,) and T["xform"].is_cuda
    assert torch.equal(sheet[:, :256], pkg.scatter_panel(T["prior"], lims=T["xform"][:2]))
    flat = enc.view(128, 32)
    assert torch.equal(T["xform"][:2], flat[:, :2].abs().amax(0) + 4.0)
    # ... and both are the reference's bytes
    xf = T["xform"].cpu()
    assert torch.equal(sheet[:, :256].cpu(), scatter_ref(T["prior"][:, 0].cpu(), T["prior"][:, 1].cpu(), xf, 256, 64, pkg.scatter_tone()))
    path = tmp_path / "scatter-3-5.png"
    assert path.is_file() and [p.name for p in tmp_path.iterdir()] == ["scatter-3-5.png"]
    assert (_decode_png_gray(path.read_bytes()) == sheet.cpu().numpy()).all()
    quiet = tmp_path / "quiet"
    quiet.mkdir()
    same = pkg.scatter_plot(enc, str(quiet), 0, 0, generator=gen(1), save=False)
    other = pkg.scatter_plot(enc, str(quiet), 0, 0, generator=gen(2), save=False)
    assert not list(quiet.iterdir()), "save=False wrote a file"
    assert torch.equal(same, sheet)
    assert torch.equal(other[:, 256:], sheet[:, 256:]) and not torch.equal(other[:, :256], sheet[:, :256])
    # given prior points, a smaller sheet
    prior = torch.randn(128, 2, generator=torch.Generator().manual_seed(3)).cuda()
    small, T2 = pkg.scatter_plot(flat, str(quiet), 0, 0, prior=prior, side=64, radius=2.0, save=False, return_tensors=True)
    assert tuple(small.shape) == (64, 128) and torch.equal(T2["prior"], prior)
    assert torch.equal(small[:, :64], pkg.scatter_panel(prior, lims=T2["xform"][:2], side=64, radius=2.0))
    assert torch.equal(small[:, 64:], pkg.scatter_panel(flat, side=64, radius=2.0))


@gpu
@pytest.mark.parametrize("name", ["cat_vae", "cat_pixelvae"])
def test_plot_callback_with_scatter(pkg, oracle, tmp_path, name):
    """One plot_vae / plot_pixelvae call through make_plot_callback(..., scatter=True): 'scatter' is the last sheet and its file exists;
    every other sheet equals the scatter=False run from the same seed (the prior draw is the last one taken from the generator)."""
    P = importlib.import_module("test_panels_gpu")
    m = P._model(name)
    image, encoding, reconstruction = P._train_forward(oracle, m)
    sheets = {}
    for flag in (True, False):
        cb = pkg.make_plot_callback(P.MEAN, P.STD, rows=P.ROWS, generator=torch.Generator(device="cuda").manual_seed(1), scatter=flag)
        directory = tmp_path / str(flag)
        sheets[flag] = cb(model=m, image=image, reconstruction=reconstruction, encoding=encoding, epoch=2, index=0, directory=str(directory),
                          running={})
        assert cb.last["sheets"] is sheets[flag] and m.training
        names = sorted(p.name for p in directory.iterdir())
        assert names == sorted(f"{stem}-2-0.png" for stem in sheets[flag])
    assert tuple(sheets[False]) == P.STEMS[name]
    assert tuple(sheets[True]) == P.STEMS[name] + ("scatter",)
    for stem in P.STEMS[name]:
        assert torch.equal(sheets[True][stem], sheets[False][stem]), stem
    scatter = sheets[True]["scatter"]
    assert tuple(scatter.shape) == (256, 512) and scatter.dtype == torch.uint8
    assert torch.equal(scatter[:, 256:], pkg.scatter_panel(encoding.detach().float()))
    assert (_decode_png_gray((tmp_path / "True" / "scatter-2-0.png").read_bytes()) == scatter.cpu().numpy()).all()


@gpu
def test_plot_functions_return_the_scatter_tensors(pkg, oracle, tmp_path):
    P = importlib.import_module("test_panels_gpu")
    m = P._model("normal_vae")
    image, encoding, reconstruction = P._train_forward(oracle, m)
    sheets, T = P._plot(pkg, "normal_vae", m, image, encoding, reconstruction, str(tmp_path), seed=5, save=False, scatter=True)
    assert tuple(sheets) == ("recon", "normal_sampling", "scatter")
    assert torch.equal(sheets["scatter"][:, :256], pkg.scatter_panel(T["scatter_prior"], lims=T["scatter_xform"][:2]))
    plain, _ = P._plot(pkg, "normal_vae", m, image, encoding, reconstruction, str(tmp_path), seed=5, save=False)
    assert tuple(plain) == ("recon", "normal_sampling")
    # a PixelCNN on its own has no latent: the callback's flag changes nothing there
    p = P._model("pixelcnn")
    pimage, pencoding, preconstruction = P._train_forward(oracle, p)
    cb = pkg.make_plot_callback(P.MEAN, P.STD, rows=P.ROWS, generator=torch.Generator(device="cuda").manual_seed(1), save=False, scatter=True)
    out = cb(model=p, image=pimage, reconstruction=preconstruction, encoding=pencoding, epoch=0, index=0, directory=str(tmp_path), running={})
    assert tuple(out) == P.STEMS["pixelcnn"]


@gpu
def test_latent_stats_python_surface(pkg, oracle):
    E = importlib.import_module("test_evaluate_gpu")
    m, N = E._model(oracle, "gauss28_f32")
    with torch.no_grad():
        _, _, mu, lv, enc, _ = E._forward(m, E._labels(oracle, m, N))
    z = m.z_dimensions
    acc = pkg.latent_stats(m, mu, lv, enc)
    assert acc.dtype == torch.float64 and tuple(acc.shape) == (6, z) and acc.is_cuda
    ref, mag = _stats_ref(mu.cpu().view(N, z), lv.cpu().view(N, z), enc.cpu().view(N, z))
    _stats_gate("latent_stats()", acc, ref, mag)
    first = acc.clone()
    again = pkg.latent_stats(m, mu, lv, enc, acc)
    assert again is acc
    assert ((acc - 2 * first).abs().cpu() <= 2e-12 * mag).all()
    only_mu = pkg.latent_stats(m, mu, None, None)
    assert torch.equal(only_mu[:2], first[:2]) and (only_mu[2:] == 0).all()
    for bad in (torch.zeros((6, z), device="cuda"), torch.zeros((5, z), dtype=torch.float64, device="cuda"), torch.zeros((6, z), dtype=torch.float64)):
        with pytest.raises(ValueError):
            pkg.latent_stats(m, mu, lv, enc, bad)
    with pytest.raises(ValueError):
        pkg.latent_stats(m, mu[:, :8], lv, enc)


@gpu
@pytest.mark.parametrize("name", ["gauss28_f32", "cat_q2"])
def test_evaluate_latent_stats(pkg, oracle, name):
    """Two small batches (3 + 2 images): 'latent' against the f64 formulas on the concatenated mu / logvar / encoding of a replay with
    the same generator (means over the 5 images, gate 1e-12 of the mean magnitudes); sum(kl_per_dim) against the returned kl to 1e-12
    relative; that kl against the one without the flag within the f32 bound of the per-image kernel's terms (0.5 * 8 * 2^-24 of the
    magnitudes, tests/test_evaluate_gpu.py); and without the flag the key set is what it was."""
    import types
    E = importlib.import_module("test_evaluate_gpu")
    m, _ = E._model(oracle, name)
    loader = E._two_batches(oracle, m)
    dev = torch.device("cuda")
    args = types.SimpleNamespace(data_ratio_of_labels=None)
    gen = lambda: torch.Generator(device="cuda").manual_seed(7)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    res = pkg.evaluate(m, loader, dev, args, E.MEAN, E.STD, generator=gen(), latent_stats=True)
    plain = pkg.evaluate(m, loader, dev, args, E.MEAN, E.STD, generator=gen())
    assert set(plain) == {"n_images", "nll", "kl", "elbo", "iw_bound", "bits_per_dim"}
    assert set(res) == set(plain) | {"latent"}
    for k, v in before.items():
        assert torch.equal(m.state_dict()[k], v), k
    assert res["n_images"] == 5 and res["nll"] == plain["nll"] and res["bits_per_dim"] == plain["bits_per_dim"]
    z, g = m.z_dimensions, gen()
    mus, lvs, encs = [], [], []
    with torch.no_grad():
        for labels in loader:
            n = labels.shape[0]
            eps = torch.randn((n, z, 1, 1), device="cuda", dtype=torch.float32, generator=g)
            _, _, mu, lv, enc, _ = E._forward(m, labels, eps)
            mus.append(mu.cpu().view(n, z)); lvs.append(lv.cpu().view(n, z)); encs.append(enc.cpu().view(n, z))
    ref, mag = _stats_ref(torch.cat(mus), torch.cat(lvs), torch.cat(encs))
    ref, mag = (ref / 5).numpy(), (mag / 5).numpy()
    lat = res["latent"]
    assert set(lat) == {"kl_per_dim", "mu_mean", "mu_var", "active_units", "mean_posterior_var", "z_mean", "z_var"}
    for key, row in (("mu_mean", 0), ("kl_per_dim", 2), ("mean_posterior_var", 3), ("z_mean", 4)):
        assert lat[key].dtype == np.float64 and lat[key].shape == (z,)
        assert (np.abs(lat[key] - ref[row]) <= 1e-12 * mag[row]).all(), key
    # variances: E[x^2] - E[x]^2 from the same sums; both terms carry the gate
    for key, r1, r2 in (("mu_var", 0, 1), ("z_var", 4, 5)):
        want = np.maximum(ref[r2] - ref[r1] ** 2, 0.0)
        assert (np.abs(lat[key] - want) <= 1e-12 * (mag[r2] + 2 * np.abs(ref[r1]) * mag[r1]) + 4e-16 * mag[r2]).all(), key
    want_var = np.maximum(ref[1] - ref[0] ** 2, 0.0)
    assert (np.abs(want_var - 0.01) > 1e-9).all(), "a dimension sits on the threshold: change the seed"
    assert lat["active_units"] == int((want_var > 0.01).sum()) and isinstance(lat["active_units"], int)
    total = float(lat["kl_per_dim"].sum())
    print(f"evaluate_latent[{name}]: kl {res['kl']!r}, sum(kl_per_dim) {total!r}, kl without the flag {plain['kl']!r}, active {lat['active_units']}")
    assert abs(total - res["kl"]) <= 1e-12 * abs(res["kl"])
    assert res["elbo"] == -(res["nll"] + res["kl"])
    assert abs(res["kl"] - plain["kl"]) <= 0.5 * 8 * E.U * float(mag[2].sum()) * 2
    # a PixelCNN on its own has no latent
    p, _ = E._model(oracle, "pixelcnn")
    pres = pkg.evaluate(p, E._two_batches(oracle, p), dev, args, E.MEAN, E.STD, latent_stats=True)
    assert pres["latent"] is None and pres["kl"] is None
