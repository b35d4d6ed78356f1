"""GPU: the picture-panel kernels through the C ABI (mmvae_logits_to_labels, mmvae_panel_sheet) against numpy in float64, at the
smallest shapes where they can go wrong: S = 9 (odd sheet width: the packed 4-byte store must fall back on every other row, and the
last pixel of each row is a ragged group) and S = 16, one plane and six, one column and all eight, Q from 1 to 16, more than one block.

Tolerances.  argmax and label columns are exact.  A sampled label can only differ from the float64 draw where u is within the f32
error of a cdf value: with |logit| <= 8 the rounding of l - max adds at most about 16 * 2^-24 ~ 1e-6 relative to each term, expf and
the Q-term sums a few 2^-23 more, so a cdf value is off by less than 4e-6; pixels with some |u - cdf_k| <= delta = 1e-5 are left out,
and their share is asserted (<= 1 %; the float64 side alone leaves out about (Q - 1) * 2 * delta <= 3e-4).  An IMAGE_F32 byte is exact
wherever the float64 value of x = (v - lo) / (hi - lo) * 255 is farther than 1e-3 from a .5 boundary (the f32 error of x is about
255 * 3 * 2^-24 ~ 5e-5) and within one grey level elsewhere; the left-out share is asserted (<= 1 %; random inputs leave out ~0.2 %)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DELTA = 1e-5
SHAPES = [(1, 2, 81), (6, 3, 81), (6, 16, 256), (5, 1, 81)]


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _labels(logits, mode, u=None):
    L = _L()
    N, Q, HW = logits.shape
    out = torch.full((N, HW), -7, dtype=torch.int64, device="cuda")
    L.check(L.lib().mmvae_logits_to_labels(L.ptr(logits), N, Q, HW, mode, L.ptr(u), L.ptr(out), torch.cuda.current_stream().cuda_stream),
            "mmvae_logits_to_labels")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _ref_draw(logits, u):
    """float64 softmax, then model.draw_labels; also the mask of pixels whose u is farther than DELTA from every cdf value.
    logits (N, Q, HW), u (N, HW), numpy."""
    M = importlib.import_module("moving-mnist-vae_amd.model")
    x = torch.from_numpy(np.ascontiguousarray(logits.astype(np.float64).transpose(0, 2, 1)))           # (N, HW, Q)
    probs = torch.softmax(x, dim=-1)
    ud = torch.from_numpy(u.astype(np.float64))
    ref = M.draw_labels(probs, ud).numpy()
    cdf = torch.cumsum(probs, dim=-1)[..., :-1]
    clear = ((cdf - ud.unsqueeze(-1)).abs() > DELTA).all(dim=-1).numpy()
    return ref, clear


def _random_logits(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_argmax_is_numpy_argmax(shape):
    logits = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)))
    got = _labels(logits.cuda(), 0)
    assert (got == logits.numpy().astype(np.float64).argmax(axis=1)).all()


@gpu
def test_argmax_ties_and_nan():
    N, Q, HW = 2, 5, 81
    assert (_labels(torch.zeros(N, Q, HW, device="cuda"), 0) == 0).all()                 # all equal: the lowest index
    x = torch.full((N, Q, HW), -1.0)
    x[:, 1], x[:, 3] = 2.5, 2.5                                                          # two equal maxima: the lower one
    x[1, 4, :40] = 2.5
    assert (_labels(x.cuda(), 0) == 1).all()
    x = torch.zeros(N, Q, HW)
    x[:, 0], x[:, 2] = float("nan"), 1.0                                                 # a NaN never wins, wherever it sits
    x[1, 4] = float("nan")
    assert (_labels(x.cuda(), 0) == 2).all()
    assert (_labels(torch.full((N, Q, HW), float("nan"), device="cuda"), 0) == 0).all()  # all NaN: 0
    assert (_labels(torch.full((N, Q, HW), -float("inf"), device="cuda"), 0) == 0).all()


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_sample_is_the_float64_draw(shape):
    N, Q, HW = shape
    logits = _random_logits(shape, 100 + sum(shape), 8.0)
    u = torch.rand((N, HW), generator=torch.Generator().manual_seed(7 + sum(shape)))
    got = _labels(logits.cuda(), 1, u.cuda())
    ref, clear = _ref_draw(logits.numpy(), u.numpy())
    left_out = 1.0 - clear.mean()
    print(f"sample {shape}: left out {left_out:.2e}, mismatches among them {(got != ref)[~clear].sum()}")
    assert left_out <= 0.01
    assert (got[clear] == ref[clear]).all()
    assert got.min() >= 0 and got.max() <= Q - 1
    # u = 0 gives label 0; u just below 1 stays inside [0, Q - 1]
    assert (_labels(logits.cuda(), 1, torch.zeros(N, HW, device="cuda")) == 0).all()
    top = _labels(logits.cuda(), 1, torch.full((N, HW), float(np.nextafter(np.float32(1.0), np.float32(0.0))), device="cuda"))
    assert top.min() >= 0 and top.max() <= Q - 1
    ref_top, clear_top = _ref_draw(logits.numpy(), np.full((N, HW), np.nextafter(np.float32(1.0), np.float32(0.0)), dtype=np.float32))
    assert (top[clear_top] == ref_top[clear_top]).all()


# ------------------------------------------------------------------------------------------------------------- the sheet
LO, HI = -0.2345, 4.266
KINDS = ("u8", "i64", "argmax", "sample", "image")
LAYOUTS = {"1-" + k: (k,) for k in KINDS}
LAYOUTS["8-mixed"] = ("u8", "i64", "argmax", "sample", "image", "argmax16", "i64", "image")


def _column(kind, n, S, seed):
    """One column: (descriptor fields holding the device tensors, expected bytes (n*S, S) uint8, mask (n*S, S) of pixels that must be exact)."""
    L = _L()
    g = torch.Generator().manual_seed(seed)
    HW = S * S
    exact = np.ones((n * S, S), dtype=bool)
    if kind in ("u8", "i64"):
        Q = 4 if kind == "u8" else 16
        lut = torch.randint(1, 256, (Q,), dtype=torch.uint8, generator=g)
        lab = torch.randint(0, Q, (n, HW), generator=g)
        lab[0, HW // 2] = Q                                                    # out of range: renders as 0
        if kind == "i64":
            lab[n - 1, 0], lab[n - 1, HW - 1] = -1, 1 << 40
        lab = lab.to(torch.uint8 if kind == "u8" else torch.int64)
        lv = lab.to(torch.int64).numpy()
        inside = (lv >= 0) & (lv < Q)
        want = np.where(inside, lut.numpy()[np.where(inside, lv, 0)], 0)
        src, lutd = lab.cuda(), lut.cuda()
        code = L.PANEL_LABELS_U8 if kind == "u8" else L.PANEL_LABELS_I64
        return (code, src, Q, None, lutd, 0.0, 1.0), want.reshape(n * S, S).astype(np.uint8), exact
    if kind in ("argmax", "argmax16", "sample"):
        Q = 16 if kind == "argmax16" else 3
        lut = torch.randint(0, 256, (Q,), dtype=torch.uint8, generator=g)
        logits = (torch.rand((n, Q, HW), generator=g) * 2 - 1) * 8.0
        if kind == "sample":
            u = torch.rand((n, HW), generator=g)
            ref, clear = _ref_draw(logits.numpy(), u.numpy())
            return ((L.PANEL_LOGITS_SAMPLE, logits.cuda(), Q, u.cuda(), lut.cuda(), 0.0, 1.0), lut.numpy()[ref].reshape(n * S, S),
                    clear.reshape(n * S, S))
        ref = logits.numpy().astype(np.float64).argmax(axis=1)
        return (L.PANEL_LOGITS_ARGMAX, logits.cuda(), Q, None, lut.cuda(), 0.0, 1.0), lut.numpy()[ref].reshape(n * S, S), exact
    v = LO + (torch.rand((n, HW), generator=g) * 1.4 - 0.2) * (HI - LO)         # a fifth of the values beyond either end
    v[0, :5] = torch.tensor([LO - 1.0, HI + 1.0, float("nan"), float("inf"), -float("inf")])
    lo32, hi32 = np.float32(LO), np.float32(HI)
    with np.errstate(invalid="ignore"):
        x = (v.numpy().astype(np.float64) - float(lo32)) / float(np.float32(hi32 - lo32)) * 255.0
        want = np.clip(np.floor(x + 0.5), 0, 255)
        want[np.isnan(x)] = 0
        exact = ~(np.abs(x - (np.floor(x) + 0.5)) <= 1e-3) | np.isnan(x) | (x < -1) | (x > 256)
    assert want.reshape(-1)[:5].tolist() == [0, 255, 0, 255, 0]                 # below lo, above hi, NaN, +inf, -inf
    return ((L.PANEL_IMAGE_F32, v.cuda(), 0, None, None, float(lo32), float(hi32)), want.reshape(n * S, S).astype(np.uint8),
            exact.reshape(n * S, S))


def _render(descs, n, S, offset):
    """The sheet written `offset` bytes into a buffer of guard bytes; checks the guards; returns the sheet as numpy."""
    L = _L()
    ncols = len(descs)
    total = n * S * ncols * S
    buf = torch.full((offset + total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    arr = (L.PanelCol * ncols)(*[L.PanelCol(code, L.ptr(src), Q, L.ptr(u), L.ptr(lut), lo, hi) for code, src, Q, u, lut, lo, hi in descs])
    L.check(L.lib().mmvae_panel_sheet(ctypes.addressof(arr), ncols, n, S, buf.data_ptr() + offset, torch.cuda.current_stream().cuda_stream),
            "mmvae_panel_sheet")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:offset] == 0xA5).all() and (host[offset + total:] == 0xA5).all(), "guard bytes were written"
    return host[offset:offset + total].reshape(n * S, ncols * S)


@gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [1, 6])
@pytest.mark.parametrize("S", [9, 16])
def test_sheet(S, n, layout):
    kinds = LAYOUTS[layout]
    cols = [_column(k, n, S, 1000 * S + 10 * n + i) for i, k in enumerate(kinds)]
    descs = [c[0] for c in cols]
    sheet = _render(descs, n, S, 64)
    assert (_render(descs, n, S, 64) == sheet).all(), "a second call gives other bytes"
    for offset in (61, 62):                                 # another alignment of `out`: other groups take the packed store
        assert (_render(descs, n, S, offset) == sheet).all()
    for c, (kind, (_, want, exact)) in enumerate(zip(kinds, cols)):
        got = sheet[:, c * S:(c + 1) * S]
        left_out = 1.0 - exact.mean()
        print(f"S={S} n={n} column {c} ({kind}): left out {left_out:.2e}")
        if kind in ("sample", "image"):
            assert left_out <= 0.01                         # (the mask depends on the inputs and the float64 side alone)
        else:
            assert exact.all()
        assert (got[exact] == want[exact]).all(), kind
        if kind == "image":
            assert (np.abs(got.astype(int) - want.astype(int))[~exact] <= 1).all()


@gpu
def test_sheet_more_than_one_block_per_column():
    """n = 40 planes of S = 16: 10240 threads per column, 40 blocks; argmax and labels side by side."""
    n, S = 40, 16
    cols = [_column(k, n, S, 77 + i) for i, k in enumerate(("argmax16", "i64"))]
    sheet = _render([c[0] for c in cols], n, S, 64)
    for c, (_, want, _) in enumerate(cols):
        assert (sheet[:, c * S:(c + 1) * S] == want).all()
