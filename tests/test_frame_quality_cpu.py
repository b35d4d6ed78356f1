"""No GPU: the host side of the per-frame quality measures -- the float64 references the GPU tests compare against (``sse_ref``,
``ssim_ref``: a valid 2-D convolution with the 11 x 11 window, checked here against a brute-force double loop), the C ABI declaration
/ binding of mmvae_frame_quality, and the argument errors both layers raise before anything is launched."""
import ctypes
import importlib
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def window():
    """g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)) / sum, float64 (11,)."""
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    return g / g.sum()


def sse_ref(a, b):
    """Sum of squared byte differences per plane: uint8 (n, S, S) -> int64 (n,)."""
    d = a.cpu().long() - b.cpu().long()
    return (d * d).flatten(1).sum(1)


def ssim_ref(a, b):
    """Mean SSIM per plane pair by the rule of include/mmvae.h in float64 on the CPU: uint8 (n, S, S) -> float64 (n,).  The five maps
    are valid 2-D convolutions with w = g g^T (the 121 products of one window summed by conv2d)."""
    a, b = a.cpu().double().unsqueeze(1), b.cpu().double().unsqueeze(1)
    g = window()
    w = (g[:, None] * g[None, :]).view(1, 1, 11, 11)
    E = lambda t: torch.nn.functional.conv2d(t, w)
    mu_a, mu_b = E(a), E(b)
    va, vb, cab = E(a * a) - mu_a * mu_a, E(b * b) - mu_b * mu_b, E(a * b) - mu_a * mu_b
    m = ((2 * mu_a * mu_b + C1) * (2 * cab + C2)) / ((mu_a * mu_a + mu_b * mu_b + C1) * (va + vb + C2))
    return m.flatten(1).mean(1)


def _brute(a, b):
    """One plane pair (lists of lists of ints) by plain Python floats, position by position."""
    S = len(a)
    g = [math.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2)) for k in range(11)]
    g = [v / sum(g) for v in g]
    total = 0.0
    for y in range(S - 10):
        for x in range(S - 10):
            ma = mb = eaa = ebb = eab = 0.0
            for i in range(11):
                for j in range(11):
                    w, p, q = g[i] * g[j], a[y + i][x + j], b[y + i][x + j]
                    ma += w * p; mb += w * q; eaa += w * p * p; ebb += w * q * q; eab += w * p * q
            va, vb, cab = eaa - ma * ma, ebb - mb * mb, eab - ma * mb
            total += ((2 * ma * mb + C1) * (2 * cab + C2)) / ((ma * ma + mb * mb + C1) * (va + vb + C2))
    return total / (S - 10) ** 2


@pytest.mark.parametrize("S", [11, 12])
def test_references_match_a_brute_force_loop(S):
    gen = torch.Generator().manual_seed(S)
    a = torch.randint(0, 256, (4, S, S), dtype=torch.uint8, generator=gen)
    b = torch.randint(0, 256, (4, S, S), dtype=torch.uint8, generator=gen)
    b[1] = a[1]
    b[2] = 255 - a[2]
    a[3], b[3] = 255, 254
    got, sse = ssim_ref(a, b), sse_ref(a, b)
    for p in range(4):
        want = _brute(a[p].tolist(), b[p].tolist())
        assert abs(got[p].item() - want) <= 1e-12, (S, p)          # two summation orders of 121 terms; far inside the GPU gate of 1e-9
        assert sse[p].item() == sum((x - y) ** 2 for ra, rb in zip(a[p].tolist(), b[p].tolist()) for x, y in zip(ra, rb))
    assert abs(got[1].item() - 1.0) <= 1e-12 and got[2].item() < 0 and sse[1].item() == 0 and sse[3].item() == S * S


def test_header_declares_and_binding_binds_the_entry_point(pkg):
    L = _L()
    txt = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    m = re.search(r"MMVAE_API\s+int\s+mmvae_frame_quality\s*\(([^)]*)\)", txt)
    assert m and len(m.group(1).split(",")) == 6 == len(L.PROTOTYPES["mmvae_frame_quality"][1])
    assert L.PROTOTYPES["mmvae_frame_quality"][0] is ctypes.c_int
    assert L.lib().mmvae_frame_quality.argtypes == L.PROTOTYPES["mmvae_frame_quality"][1]
    assert "#define MMVAE_FRAME_BYTES_U8 5" in txt and L.FRAME_BYTES_U8 == 5
    assert (L.FRAME_MIN_S, L.FRAME_MAX_S) == (11, 64)
    assert L.lib().mmvae_abi_version() == 3 and "#define MMVAE_ABI_VERSION 3" in txt
    assert "Wang et al. 2004" in txt                         # the rule is part of the interface


def _rc(a, b, n=1, S=16, out=0x1000):
    """mmvae_frame_quality with made-up device addresses: every call here must be refused before they could be used."""
    L = _L()
    rc = L.lib().mmvae_frame_quality(None if a is None else ctypes.addressof(a), None if b is None else ctypes.addressof(b), n, S, out, None)
    return rc, (L.lib().mmvae_last_error() or b"").decode()


def test_c_abi_refuses_bad_arguments_before_any_launch(pkg):
    L = _L()
    A = 0x1000                                                # never dereferenced
    good = L.PanelCol(L.FRAME_BYTES_U8, A, 0, None, None, 0.0, 0.0)
    lab = L.PanelCol(L.PANEL_LABELS_U8, A, 2, None, A, 0.0, 1.0)
    for S in (10, 65, 0, -1):
        rc, msg = _rc(good, lab, S=S)
        assert rc == -4 and f"S={S}" in msg                   # MMVAE_ERR_UNSUPPORTED
    assert _rc(good, lab, n=0)[0] == -1 and _rc(good, lab, n=-3)[0] == -1
    assert _rc(good, lab, out=None)[0] == -1
    assert _rc(None, lab)[0] == -1 and _rc(good, None)[0] == -1
    bad = [L.PanelCol(L.FRAME_BYTES_U8, None, 0, None, None, 0.0, 0.0),            # no source
           L.PanelCol(L.PANEL_LABELS_I64, None, 2, None, A, 0.0, 1.0),
           L.PanelCol(L.PANEL_LABELS_I64, A, 2, None, None, 0.0, 1.0),             # no lut
           L.PanelCol(L.PANEL_LOGITS_ARGMAX, A, 2, None, None, 0.0, 1.0),
           L.PanelCol(L.PANEL_LOGITS_SAMPLE, A, 2, None, A, 0.0, 1.0),             # no uniforms
           L.PanelCol(L.PANEL_LOGITS_ARGMAX, A, 0, None, A, 0.0, 1.0),             # Q outside 1..16
           L.PanelCol(L.PANEL_LOGITS_ARGMAX, A, 17, None, A, 0.0, 1.0),
           L.PanelCol(L.PANEL_LABELS_U8, A, 17, None, A, 0.0, 1.0),
           L.PanelCol(L.PANEL_IMAGE_F32, A, 0, None, None, 1.0, 1.0),              # hi <= lo
           L.PanelCol(L.PANEL_IMAGE_F32, A, 0, None, None, 1.0, 0.5),
           L.PanelCol(L.PANEL_IMAGE_F32, A, 0, None, None, 0.0, float("nan")),
           L.PanelCol(6, A, 2, None, A, 0.0, 1.0),                                 # unknown kinds
           L.PanelCol(-1, A, 2, None, A, 0.0, 1.0)]
    for i, col in enumerate(bad):
        assert _rc(col, good)[0] == -1, i
        rc, msg = _rc(good, col)
        assert rc == -1 and "side b" in msg, i
    # the raw-byte kind is this entry point's alone: the sheet keeps refusing it
    arr = (L.PanelCol * 1)(good)
    assert L.lib().mmvae_panel_sheet(ctypes.addressof(arr), 1, 1, 16, A, None) == -1
    arr = (L.PanelCol * 1)(L.PanelCol(5, A, 2, None, A, 0.0, 1.0))
    assert L.lib().mmvae_panel_sheet(ctypes.addressof(arr), 1, 1, 9, A, None) == -1


class _OnGpu(torch.Tensor):
    """A host tensor that claims to live on the GPU: lets the checks behind the device check run without one.  Nothing here may reach
    a launch -- every call below must raise first."""
    @property
    def is_cuda(self):
        return True


def _fake(t):
    return t.as_subclass(_OnGpu)


def test_frame_quality_refuses_bad_arguments(pkg):
    col = pkg.column
    by = lambda *shape: col("bytes", _fake(torch.zeros(shape, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="GPU"):              # a CPU tensor
        pkg.frame_quality(col("bytes", torch.zeros(2, 16, 16, dtype=torch.uint8)), by(2, 16, 16))
    with pytest.raises(ValueError, match="kind"):
        pkg.frame_quality(col("picture", _fake(torch.zeros(2, 16, 16))), by(2, 16, 16))
    with pytest.raises(ValueError, match="tensor"):
        pkg.frame_quality(col("bytes", None), by(2, 16, 16))
    with pytest.raises(ValueError, match="uint8"):
        pkg.frame_quality(col("bytes", _fake(torch.zeros(2, 16, 16))), by(2, 16, 16))
    with pytest.raises(ValueError, match="square"):
        pkg.frame_quality(by(2, 16, 12), by(2, 16, 16))
    with pytest.raises(ValueError, match="2 planes against 3"):
        pkg.frame_quality(by(2, 16, 16), by(3, 16, 16))
    with pytest.raises(ValueError, match="side 16 against planes of side 12"):
        pkg.frame_quality(by(2, 256), by(2, 12, 12))
    for S in (10, 65):
        with pytest.raises(ValueError, match=f"side {S} unsupported"):
            pkg.frame_quality(by(2, S, S), by(2, S, S))
    with pytest.raises(ValueError, match="one channel"):
        pkg.frame_quality(by(2, 3, 16, 16), by(2, 16, 16))
    with pytest.raises(ValueError, match="3 columns"):        # a (n, C, S, S) image is the caller's to reshape
        pkg.frame_quality(col("image", _fake(torch.zeros(2, 3, 16, 16)), lo=0.0, hi=1.0), by(2, 16, 16))
    # the checks of render_sheet's columns are reused as they are
    with pytest.raises(ValueError, match="lo < hi"):
        pkg.frame_quality(col("image", _fake(torch.zeros(2, 16, 16)), lo=1.0, hi=1.0), by(2, 16, 16))
    with pytest.raises(ValueError, match="float32"):
        pkg.frame_quality(col("image", _fake(torch.zeros(2, 16, 16, dtype=torch.float64)), lo=0.0, hi=1.0), by(2, 16, 16))
    with pytest.raises(ValueError, match="lut"):
        pkg.frame_quality(col("labels", _fake(torch.zeros(2, 16, 16, dtype=torch.int64))), by(2, 16, 16))
    with pytest.raises(ValueError, match="Q = 17"):
        pkg.frame_quality(col("argmax", _fake(torch.zeros(2, 17, 16, 16))), by(2, 16, 16))
    with pytest.raises(ValueError, match="uniforms"):
        pkg.frame_quality(col("sample", _fake(torch.zeros(2, 2, 16, 16))), by(2, 16, 16))
    # render_sheet does not learn the raw-byte kind
    with pytest.raises(ValueError, match="kind"):
        pkg.render_sheet([by(2, 16, 16)], 2)


def test_reconstruction_quality_refuses_a_categorical_model_with_channels(pkg):
    import types
    m = types.SimpleNamespace(pixelcnn=None, decoder_out_channels=6, in_channels=3, pixelcnn_out_channels=2)
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(ValueError, match="in_channels > 1"):
        pkg.reconstruction_quality(m, x, torch.zeros(2, 6, 16, 16), 0.05, 0.22)
    with pytest.raises(ValueError, match=r"\(N, C, S, S\)"):
        pkg.reconstruction_quality(m, x[0], torch.zeros(2, 6, 16, 16), 0.05, 0.22)


def test_new_names_are_exported(pkg):
    main = importlib.import_module("moving-mnist-vae_amd.main")
    for name in ("frame_quality", "reconstruction_quality"):
        assert callable(getattr(pkg, name)) and getattr(pkg, name) is getattr(main, name), name
    import inspect
    sig = inspect.signature(pkg.evaluate)
    assert sig.parameters["quality"].default is False and sig.parameters["centres"].default is None
