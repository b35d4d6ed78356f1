"""No GPU: the host side of the picture panels -- the PNG writer (decoded by a decoder written here from zlib, and by PIL when it
imports), gray_lut, the C ABI declarations / bindings of mmvae_logits_to_labels and mmvae_panel_sheet, and the argument errors both
layers refuse before anything is launched."""
import ctypes
import importlib
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _decode_png_gray(data):
    """Strict decoder of what write_png_gray may emit: 8-bit greyscale, no interlace, filter type 0 on every row."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        (length,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        assert crc == zlib.crc32(tag + body) & 0xffffffff, tag
        chunks.append((tag, body))
        pos += 12 + length
    assert pos == len(data)
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filt, interlace) == (8, 0, 0, 0, 0)
    assert all(t in (b"IHDR", b"IDAT", b"IEND") for t, _ in chunks)
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    assert len(raw) == h * (w + 1)
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, w + 1)
    assert (rows[:, 0] == 0).all(), "filter bytes"
    return rows[:, 1:]


@pytest.mark.parametrize("shape", [(9, 9), (54, 72)])
def test_write_png_gray_round_trips(pkg, tmp_path, shape):
    sheet = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(shape[0]))
    sheet[0, 0], sheet[-1, -1] = 0, 255
    path = str(tmp_path / "sheet.png")
    assert pkg.write_png_gray(path, sheet) == path
    with open(path, "rb") as f:
        got = _decode_png_gray(f.read())
    assert got.shape == shape and (got == sheet.numpy()).all()
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.mode == "L" and im.size == (shape[1], shape[0])
        assert (np.array(im) == sheet.numpy()).all()


def test_write_png_gray_refuses_other_input(pkg, tmp_path):
    with pytest.raises(ValueError):
        pkg.write_png_gray(str(tmp_path / "a.png"), torch.zeros(4, 4))
    with pytest.raises(ValueError):
        pkg.write_png_gray(str(tmp_path / "a.png"), torch.zeros(2, 4, 4, dtype=torch.uint8))


def test_gray_lut(pkg):
    assert pkg.gray_lut(2).tolist() == [0, 255]
    assert pkg.gray_lut(3).tolist() == [0, 128, 255]
    assert pkg.gray_lut(16).tolist() == [17 * k for k in range(16)]
    assert pkg.gray_lut(1).tolist() == [0]
    lut = pkg.gray_lut(4, [0.0, 0.1, 0.5, 1.2])            # 25.5 rounds up to 26, 127.5 up to 128, 306 clamps
    assert lut.dtype == torch.uint8 and lut.tolist() == [0, 26, 128, 255]
    assert pkg.gray_lut(2, np.array([[0.002], [0.9]])).tolist() == [1, 230]       # cluster_centers_ has shape (q, 1)
    with pytest.raises(ValueError):
        pkg.gray_lut(3, [0.0, 1.0])
    with pytest.raises(ValueError):
        pkg.gray_lut(0)


def test_header_declares_and_binding_binds_both_entry_points(pkg):
    L = _L()
    txt = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for name in ("mmvae_logits_to_labels", "mmvae_panel_sheet"):
        assert re.search(r"MMVAE_API\s+int\s+" + name + r"\s*\(", txt), name
        assert name in L.PROTOTYPES
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1]
    assert L.lib().mmvae_abi_version() == 3 and "#define MMVAE_ABI_VERSION 3" in txt
    # the ctypes mirror of mmvae_panel_col: field order of the header, natural alignment
    fields = re.search(r"typedef struct mmvae_panel_col \{(.*?)\} mmvae_panel_col;", txt, re.S).group(1)
    names = [n for decl in fields.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in L.PanelCol._fields_] == ["kind", "src", "Q", "uniforms", "lut", "lo", "hi"]
    assert ctypes.sizeof(L.PanelCol) == 48 and L.PanelCol.lo.offset == 40
    for k, name in enumerate(("LABELS_U8", "LABELS_I64", "LOGITS_ARGMAX", "LOGITS_SAMPLE", "IMAGE_F32")):
        assert "#define MMVAE_PANEL_%s %d" % (name, k) in txt and getattr(L, "PANEL_" + name) == k


def _sheet_rc(cols, ncols, n=1, S=9, out=0x1000):
    """mmvae_panel_sheet with made-up device addresses: every call here must be refused before they could be used."""
    L = _L()
    arr = (L.PanelCol * len(cols))(*cols)
    rc = L.lib().mmvae_panel_sheet(ctypes.addressof(arr), ncols, n, S, out, None)
    return rc, (L.lib().mmvae_last_error() or b"").decode()


def test_c_abi_refuses_bad_arguments_before_any_launch(pkg):
    L = _L()
    A = 0x1000                                              # never dereferenced
    good = L.PanelCol(L.PANEL_LABELS_U8, A, 2, None, A, 0.0, 1.0)
    assert _sheet_rc([good] * 9, 9)[0] == -1                # ncols = 9
    assert _sheet_rc([good], 0)[0] == -1
    assert _sheet_rc([good], 1, S=65)[0] == -1
    assert _sheet_rc([good], 1, n=0)[0] == -1
    assert _sheet_rc([good], 1, out=None)[0] == -1
    rc, msg = _sheet_rc([L.PanelCol(L.PANEL_LOGITS_ARGMAX, A, 17, None, A, 0.0, 1.0)], 1)
    assert rc == -4 and "Q=17" in msg                       # MMVAE_ERR_UNSUPPORTED
    assert _sheet_rc([L.PanelCol(L.PANEL_LOGITS_ARGMAX, A, 0, None, A, 0.0, 1.0)], 1)[0] == -4
    for lo, hi in ((1.0, 1.0), (1.0, 0.5), (0.0, float("nan"))):
        rc, msg = _sheet_rc([L.PanelCol(L.PANEL_IMAGE_F32, A, 0, None, None, lo, hi)], 1)
        assert rc == -1 and "hi > lo" in msg
    assert _sheet_rc([L.PanelCol(L.PANEL_LOGITS_SAMPLE, A, 2, None, A, 0.0, 1.0)], 1)[0] == -1      # no uniforms
    assert _sheet_rc([L.PanelCol(L.PANEL_LABELS_I64, A, 2, None, None, 0.0, 1.0)], 1)[0] == -1      # no lut
    assert _sheet_rc([L.PanelCol(L.PANEL_LABELS_I64, None, 2, None, A, 0.0, 1.0)], 1)[0] == -1      # no source
    assert _sheet_rc([L.PanelCol(5, A, 2, None, A, 0.0, 1.0)], 1)[0] == -1                          # unknown kind
    lib = L.lib()
    assert lib.mmvae_logits_to_labels(A, 1, 17, 81, 0, None, A, None) == -4
    assert lib.mmvae_logits_to_labels(A, 1, 0, 81, 0, None, A, None) == -4
    assert lib.mmvae_logits_to_labels(A, 1, 2, 81, 1, None, A, None) == -1                          # sample mode without uniforms
    assert lib.mmvae_logits_to_labels(A, 1, 2, 81, 2, None, A, None) == -1
    assert lib.mmvae_logits_to_labels(None, 1, 2, 81, 0, None, A, None) == -1
    assert lib.mmvae_logits_to_labels(A, 0, 2, 81, 0, None, A, None) == -1


def test_render_sheet_refuses_bad_arguments(pkg):
    img = torch.zeros(6, 9, 9)
    with pytest.raises(ValueError, match="GPU"):            # a CPU tensor
        pkg.render_sheet([pkg.column("image", img, lo=0.0, hi=1.0)], 6)
    with pytest.raises(ValueError, match="exactly 6 planes"):          # mismatched plane counts
        pkg.render_sheet([pkg.column("image", torch.zeros(5, 9, 9), lo=0.0, hi=1.0)], 6)
    with pytest.raises(ValueError, match="kind"):
        pkg.render_sheet([pkg.column("picture", img)], 6)
    with pytest.raises(ValueError):
        pkg.render_sheet([], 6)
    with pytest.raises(ValueError):
        pkg.render_sheet([pkg.column("image", img, lo=0.0, hi=1.0)], 0)
    with pytest.raises(ValueError):
        importlib.import_module("moving-mnist-vae_amd.model").decode_labels(torch.zeros(1, 2, 9, 9))      # a CPU tensor
    with pytest.raises(ValueError):
        pkg.sample_from_reconstruction(torch.zeros(1, 2, 9, 9))


def test_new_names_are_exported(pkg):
    for name in ("column", "gray_lut", "render_sheet", "write_png_gray", "plot_vae", "plot_pixelcnn", "plot_pixelvae", "latent_slide",
                 "make_plot_callback", "sample_from_reconstruction", "decode_labels"):
        assert callable(getattr(pkg, name)), name
    assert "plot_callback" in importlib.import_module("moving-mnist-vae_amd.main").__doc__


def test_main_carries_every_name_the_package_imports(pkg):
    """The drop-in promise is "swap the import": the reference's main.py holds the input pipeline and the plot functions too, so
    ``main`` re-exports what ``data`` and ``panels`` define -- the very objects the package hands out."""
    import types
    main = importlib.import_module("moving-mnist-vae_amd.main")
    names = [n for n, v in vars(pkg).items() if not n.startswith("_") and not isinstance(v, types.ModuleType)]
    assert len(names) >= 33 and {"train", "plot_vae", "scatter_plot", "quantise_frames", "MovingMNISTClips"} <= set(names)
    for name in names:
        assert getattr(pkg, name) is getattr(main, name), name
