"""GPU: per-frame quality -- mmvae_frame_quality through ``frame_quality`` and the C ABI against the float64 references of
tests/test_frame_quality_cpu.py, and the surface on top of it (``reconstruction_quality``, ``evaluate(quality=True)``, graph capture).

Op test.  Sides S in {11, 12, 27, 64} (one valid position, two per row, an odd size, the maximum) x n in {1, 3, 70} (one pair, a
ragged few, more pairs than one block's share).  Every case runs the six contents (random bytes, a against a, a against 255 - a,
constant 255 against constant 254, all zeros, sparse 0 / 255 planes) through the 'bytes' and 'image' kinds, and its share of the 49
ordered pairings of source kinds (u8 labels, i64 labels, argmax Q = 3, argmax Q = 16, sample, image, bytes) on random data.  The bytes
each side stands for come from ``render_sheet`` on the same column spec (pinned by its own tests), or are the tensor itself for 'bytes'.

Gates.  sse: torch.equal to the int64 reference.  ssim: |device - ssim_ref| <= 1e-9 for every pair -- a window sum of 121 non-negative
terms <= 65025 errs by < 1e-9 absolute in f64 (121 * 65025 * 2^-53 = 8.7e-10, and only when every term is at its maximum); every
denominator factor is >= C1 = 6.5 or C2 = 58.5, so a map value errs by <~ 1e-10; the 2-D and the separable summation order of the
reference differ by at most 7.5e-13 over these contents and sizes.  mse: equal to sse_ref / S^2 in f64.  psnr: 1e-12 relative, inf
where mse = 0.  The same bits on a second call; the words around out[2][n] untouched.

Worst ssim error / gate measured on the MI355X (every case prints its own as `frame_quality[...] worst ssim error`): 1.12e-3 over the
op test (1.1e-12 absolute, on the constant 255 against 254 planes; 2e-6 on every other content), 2.8e-8 over the surface test."""
import ctypes
import importlib
import itertools
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_frame_quality_cpu import sse_ref, ssim_ref  # noqa: E402

gpu = pytest.mark.gpu
SSIM_GATE = 1e-9
MEAN, STD = 0.0521, 0.2222
KINDS = ("u8", "i64", "argmax3", "argmax16", "sample", "image", "bytes")
SHAPES = [(S, n) for S in (11, 12, 27, 64) for n in (1, 3, 70)]
PAIRINGS = list(itertools.product(KINDS, KINDS))                       # 49 ordered pairings, dealt out over the 12 shapes


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _Q():
    return importlib.import_module("moving-mnist-vae_amd.quality")


def _side(pkg, kind, n, S, gen):
    """A random side of the given kind: (column spec, the (n, S, S) uint8 planes it stands for)."""
    col = pkg.column
    if kind == "bytes":
        t = torch.randint(0, 256, (n, S, S), dtype=torch.uint8, generator=gen).cuda()
        return col("bytes", t), t
    if kind == "image":                                               # values beyond [lo, hi] too: the clamp is part of the rule
        spec = col("image", (torch.rand((n, S, S), generator=gen) * 1.4 - 0.2).cuda(), lo=0.0, hi=1.0)
    elif kind in ("u8", "i64"):
        Q = 16 if kind == "u8" else 5
        lut = torch.randint(0, 256, (Q,), dtype=torch.uint8, generator=gen)
        lab = torch.randint(0, Q, (n, S * S), generator=gen)
        spec = col("labels", (lab.to(torch.uint8) if kind == "u8" else lab).cuda(), lut)
    else:
        Q = 16 if kind == "argmax16" else 3
        logits = torch.randn((n, Q, S, S), generator=gen).cuda()
        lut = torch.randint(0, 256, (Q,), dtype=torch.uint8, generator=gen) if kind == "argmax16" else None
        spec = col("sample", logits, lut, torch.rand((n, S * S), generator=gen).cuda()) if kind == "sample" else col("argmax", logits, lut)
    return spec, pkg.render_sheet([spec], n).view(n, S, S)


def _contents(n, S, gen):
    """The six contents as byte planes, dealt cyclically over a whole number of launches of n pairs: (a, b) uint8 (T, S, S)."""
    rnd = lambda: torch.randint(0, 256, (S, S), dtype=torch.uint8, generator=gen)
    sparse = lambda: ((torch.rand((S, S), generator=gen) < 0.06) * 255).to(torch.uint8)
    a, b = [], []
    for p in range(n * -(-6 // n)):
        x = rnd()
        pa, pb = [(x, rnd()), (x, x), (x, 255 - x), (torch.full_like(x, 255), torch.full_like(x, 254)), (x * 0, x * 0),
                  (sparse(), sparse())][p % 6]
        a.append(pa); b.append(pb)
    return torch.stack(a), torch.stack(b)


def _check(tag, q, a_bytes, b_bytes, S):
    """Every gate of the module docstring on one result dict; returns the worst ssim error."""
    n = a_bytes.shape[0]
    sse, ssim = sse_ref(a_bytes, b_bytes), ssim_ref(a_bytes, b_bytes)
    for key in ("sse", "ssim", "mse", "psnr"):
        assert q[key].dtype == torch.float64 and q[key].shape == (n,) and q[key].is_cuda, (tag, key)
    assert torch.equal(q["sse"].cpu(), sse.double()), tag
    err = (q["ssim"].cpu() - ssim).abs()
    print(f"frame_quality[{tag}] worst ssim error {err.max().item():.3e} = {err.max().item() / SSIM_GATE:.2e} of the gate")
    assert (err <= SSIM_GATE).all(), (tag, err.max().item())
    mse = sse.double() / float(S * S)
    assert torch.equal(q["mse"].cpu(), mse), tag
    psnr, got = 10.0 * torch.log10(65025.0 / mse), q["psnr"].cpu()
    same = mse == 0
    assert torch.isposinf(got[same]).all() and ((got[~same] - psnr[~same]).abs() <= 1e-12 * psnr[~same].abs()).all(), tag
    return err.max().item()


def _c_call(spec_a, spec_b, n, S):
    """One launch through the C ABI into the middle of a guarded buffer: (out (2, n), guards untouched?)."""
    L, Q = _L(), _Q()
    descs = (Q._side(spec_a, "a")[0], Q._side(spec_b, "b")[0])        # (kept: they hold the device copies whose addresses are passed)
    cols = [L.PanelCol(code, L.ptr(t), q, L.ptr(u), L.ptr(lut), lo, hi) for code, t, q, u, lut, lo, hi in descs]
    buf = torch.full((2 * n + 16,), -7.25, dtype=torch.float64, device="cuda")
    L.check(L.lib().mmvae_frame_quality(ctypes.addressof(cols[0]), ctypes.addressof(cols[1]), n, S, buf.data_ptr() + 64,
                                        torch.cuda.current_stream().cuda_stream), "mmvae_frame_quality")
    torch.cuda.synchronize()
    return buf[8:8 + 2 * n].view(2, n), bool((buf[:8] == -7.25).all() and (buf[8 + 2 * n:] == -7.25).all())


@gpu
@pytest.mark.parametrize("S,n", SHAPES)
def test_frame_quality_op(pkg, S, n):
    case = SHAPES.index((S, n))
    gen = torch.Generator().manual_seed(100 + case)
    col = pkg.column
    # the six contents through the two kinds that can hold any byte
    a, b = _contents(n, S, gen)
    for k in range(a.shape[0] // n):
        pa, pb = a[k * n:(k + 1) * n].cuda(), b[k * n:(k + 1) * n].cuda()
        as_image = lambda t: col("image", t.float(), lo=0.0, hi=255.0)             # (v - 0) / 255 * 255 in f32 is the byte itself
        for form, (sa, sb) in {"bytes,bytes": (col("bytes", pa), col("bytes", pb)), "image,bytes": (as_image(pa), col("bytes", pb)),
                               "bytes,image": (col("bytes", pa.view(n, -1)), as_image(pb))}.items():
            q = pkg.frame_quality(sa, sb)
            _check(f"S={S},n={n},contents {k},{form}", q, pa, pb, S)
            again = pkg.frame_quality(sa, sb)
            assert all(torch.equal(q[key], again[key]) for key in q)
        if k == 0:
            out, guards = _c_call(sa, sb, n, S)
            assert guards and torch.equal(out[0], q["sse"]) and torch.equal(out[1], q["ssim"])
            if n >= 3:
                assert q["ssim"][1].item() == pytest.approx(1.0, abs=1e-12) and q["sse"][1].item() == 0.0      # a against a
                assert q["ssim"][2].item() < 0.0                                                             # a against 255 - a
    # this shape's share of the 49 ordered pairings of kinds
    for ka, kb in PAIRINGS[case::len(SHAPES)]:
        (sa, pa), (sb, pb) = _side(pkg, ka, n, S, gen), _side(pkg, kb, n, S, gen)
        q = pkg.frame_quality(sa, sb)
        _check(f"S={S},n={n},{ka},{kb}", q, pa, pb, S)
        again = pkg.frame_quality(sa, sb)
        assert all(torch.equal(q[key], again[key]) for key in q)
        out, guards = _c_call(sa, sb, n, S)
        assert guards and torch.equal(out[0], q["sse"]) and torch.equal(out[1], q["ssim"])


def test_every_ordered_pairing_of_kinds_is_dealt_out():
    assert sorted(p for c in range(len(SHAPES)) for p in PAIRINGS[c::len(SHAPES)]) == sorted(PAIRINGS) and len(PAIRINGS) == 49


# ------------------------------------------------------------------------------------------ the surface
# name -> (VAE's positional constructor arguments, compute dtype)
#         in mid dec_out pix_out z  pixelcnn only layers                     sigma S
MODELS = {
    "gauss16": ((1, 32, 1, 2, 8, False, False, 4, "ReLu", 1, 1, 0, True, 0.1, 16), "bf16"),
    "cat16": ((1, 32, 2, 2, 8, False, False, 4, "ReLu", 1, 1, 0, True, 0.1, 16), "bf16"),
    "pixelvae32": ((1, 16, 2, 2, 32, True, False, 3, "ReLu", 1, 1, 0, True, 0.0, 32), "bf16"),
    "gauss27": ((1, 32, 1, 2, 8, False, False, 4, "ReLu", 1, 1, 0, True, 0.1, 27), "f32"),
}


def _model(oracle, name):
    ctor, dt = MODELS[name]
    torch.manual_seed(3)
    m = importlib.import_module("moving-mnist-vae_amd.model").VAE(*ctor, compute_dtype=dt)
    if m.pixelcnn is None:       # well-conditioned weights and non-trivial BatchNorm running statistics (the default ones are 0 / 1)
        m.load_state_dict(oracle.filled_state(oracle.state_spec(ctor[0], ctor[4], ctor[2], ctor[14], ctor[12]), seed=5))
    return m.to("cuda").eval()


def _categorical(m):
    return m.pixelcnn is not None or m.decoder_out_channels > m.in_channels


def _replay(pkg, m, loader, seed):
    """What evaluate() does batch by batch, with the same generator: [(image, encoding, reconstruction, reconstruction_quality)]."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    with torch.no_grad():
        for labels in loader:
            image, _ = m.prepare_batch(labels, torch.device("cuda"), MEAN, STD, _categorical(m))
            m.injected_eps = torch.randn((labels.shape[0], m.z_dimensions, 1, 1), device="cuda", dtype=torch.float32, generator=gen)
            try:
                _, _, enc, rec = m(image, sample=image)
            finally:
                m.injected_eps = None
            out.append((image, enc, rec, pkg.reconstruction_quality(m, image, rec, MEAN, STD)))
    return out


@gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_reconstruction_quality_and_evaluate(pkg, oracle, name):
    m = _model(oracle, name)
    S, dev = m.input_image_size, torch.device("cuda")
    loader = [oracle.synthetic_labels(3, S, seed=31, p=0.05).view(3, -1), oracle.synthetic_labels(2, S, seed=32, p=0.35).view(2, -1)]
    args = types.SimpleNamespace(data_ratio_of_labels=None)
    batches = _replay(pkg, m, loader, 7)
    # (taken after a forward: a PixelCNN's forward multiplies its stored weights by their masks, as the reference's does)
    before = {k: v.clone() for k, v in m.state_dict().items()}

    # the very columns the plot functions draw, and the bytes of the sheet they render
    image, enc, rec, q = batches[0]
    kw = dict(rows=3, generator=torch.Generator(device="cuda").manual_seed(1), save=False, return_tensors=True)
    if m.pixelcnn is None:
        sheets, T = pkg.plot_vae(m, dev, image, rec, enc, None, 0, 0, data_mean=MEAN, data_std=STD, **kw)
        sheet, theirs = sheets["recon"], 1
    else:
        sheets, T = pkg.plot_pixelvae(m, dev, image, rec, enc, None, 0, 0, MEAN, STD, **kw)
        sheet, theirs = sheets["recon_z_"], 1 + m.decoder_out_channels
    col_a = pkg.column("image", T["image"], lo=T["lo"], hi=T["hi"])
    col_b = (pkg.column("argmax", T["reconstruction"], T["lut"]) if _categorical(m)
             else pkg.column("image", T["reconstruction"].float(), lo=T["lo"], hi=T["hi"]))
    fq = pkg.frame_quality(col_a, col_b)
    assert sorted(q) == sorted(fq) == ["mse", "psnr", "sse", "ssim"] and all(torch.equal(q[k], fq[k]) for k in q)
    planes = sheet.view(3, S, -1)
    _check(f"{name},sheet", q, planes[:, :, :S], planes[:, :, theirs * S:(theirs + 1) * S], S)
    assert (q["sse"] > 0).all()                                        # an untrained model does not reproduce its input

    if S % 2:                      # the decoder's crop leaves an odd size one row and column too many: the quality columns fit them
        return                     # (_fit_planes), the likelihood terms of evaluate() refuse that reconstruction with or without the flag
    # evaluate(quality=True): means per image over a 3 + 2 loader, the other keys untouched, the model unchanged
    m.train()
    g = lambda: torch.Generator(device="cuda").manual_seed(7)
    res = pkg.evaluate(m, loader, dev, args, MEAN, STD, generator=g(), return_per_image=True, quality=True)
    plain = pkg.evaluate(m, loader, dev, args, MEAN, STD, generator=g(), return_per_image=True)
    assert m.training is True
    m.eval()
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], v) for k, v in before.items())
    assert "quality" not in plain and sorted(plain["per_image"]) == ["iw_bound", "kl", "nll"]
    assert sorted(res) == sorted(list(plain) + ["quality"]) and sorted(res["per_image"]) == ["iw_bound", "kl", "mse", "nll", "ssim"]
    for k, v in plain.items():
        if k != "per_image":
            assert res[k] == v, k
    for k, v in plain["per_image"].items():
        assert (res["per_image"][k] is None and v is None) or torch.equal(res["per_image"][k], v), k
    want = {k: torch.cat([b[3][k] for b in batches]) for k in ("mse", "ssim")}
    for k, v in want.items():
        got = res["per_image"][k]
        assert got.dtype == torch.float64 and got.shape == (5,) and torch.equal(got, v), k
        mean = v.sum().item() / 5                                      # (3 + 2 summed batch-wise against all five at once: f64 roundings)
        assert abs(res["quality"][k] - mean) <= 8 * 2.0 ** -53 * v.abs().sum().item() / 5, k
    assert res["quality"]["psnr"] == pytest.approx(10.0 * torch.log10(torch.tensor(65025.0 / res["quality"]["mse"], dtype=torch.float64)).item(),
                                                   rel=1e-12)
    assert sorted(res["quality"]) == ["mse", "psnr", "ssim"]


@gpu
def test_reconstruction_quality_averages_the_channels_of_a_gaussian_model(pkg):
    """in_channels = 3, nothing but the model's attributes is read: planes compared one by one, averaged back per image."""
    m = types.SimpleNamespace(pixelcnn=None, decoder_out_channels=3, in_channels=3, pixelcnn_out_channels=2)
    gen = torch.Generator().manual_seed(5)
    x, y = torch.rand((2, 3, 16, 16), generator=gen).cuda(), torch.rand((2, 3, 16, 16), generator=gen).cuda()
    lo, hi = (0.0 - MEAN) / STD, (1.0 - MEAN) / STD
    q = pkg.reconstruction_quality(m, x * (hi - lo) + lo, y * (hi - lo) + lo, MEAN, STD)
    col = lambda t: pkg.column("image", (t * (hi - lo) + lo).reshape(6, 16, 16), lo=lo, hi=hi)
    flat = pkg.frame_quality(col(x), col(y))
    assert torch.equal(q["sse"], flat["sse"].view(2, 3).sum(1)) and torch.equal(q["ssim"], flat["ssim"].view(2, 3).mean(1))
    assert torch.equal(q["mse"].cpu(), q["sse"].cpu() / (3 * 256.0)) and torch.equal(q["psnr"], 10.0 * torch.log10(65025.0 / q["mse"]))


@gpu
def test_frame_quality_replays_in_a_graph(pkg):
    """One frame_quality call captured with torch.cuda.graph and replayed on new contents equals the eager call, to the bit."""
    gen = torch.Generator().manual_seed(9)
    n, S = 5, 27
    a = torch.randint(0, 256, (n, S, S), dtype=torch.uint8, generator=gen).cuda()
    b = torch.rand((n, S, S), generator=gen).cuda()
    call = lambda: pkg.frame_quality(pkg.column("bytes", a), pkg.column("image", b, lo=0.0, hi=1.0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                         # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(2):
        a.copy_(torch.randint(0, 256, (n, S, S), dtype=torch.uint8, generator=gen))
        b.copy_(torch.rand((n, S, S), generator=gen))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager = call()
        assert all(torch.equal(captured[k], eager[k]) for k in eager)
    _check("graph", captured, a, pkg.render_sheet([pkg.column("image", b, lo=0.0, hi=1.0)], n).view(n, S, S), S)
