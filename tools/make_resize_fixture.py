"""Writes tests/golden/pil_resize.npz: uint8 planes and what PIL makes of them with
``Image.fromarray(a, "L").resize((S_w, S_h), Image.BILINEAR)`` -- the call ``transforms.Resize(S)`` makes for a square mode-L image
(the reference's input transform, main.py:33-36).  The tests compare the library's coefficient tables and the device resize against
these bytes, so neither needs PIL.  Needs only numpy and PIL; reads nothing of the reference.

File layout: ``pil_version`` (str), ``cases`` (n, 4) int32 rows (in_h, in_w, out_h, out_w), and for row i ``x{i}`` (3, in_h, in_w) /
``y{i}`` (3, out_h, out_w) uint8: random bytes, a sparse 0/255 pattern, a bright block on black.

    python tools/make_resize_fixture.py
"""
import os

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE = [(64, 32), (64, 56), (64, 28), (64, 9), (64, 33), (64, 63), (64, 64), (28, 14), (28, 20), (28, 9)]
CASES = [(i, i, o, o) for i, o in SQUARE] + [(40, 64, 20, 32)]


def inputs(h, w, rng):
    random = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    sparse = np.where(rng.random((h, w)) < 0.08, 255, 0).astype(np.uint8)
    block = np.zeros((h, w), dtype=np.uint8)
    block[h // 4:h // 4 + max(h // 3, 2), w // 5:w // 5 + max(w // 2, 2)] = 255
    block[h // 4 + 1, w // 5 + 1] = 200                      # (one softer pixel inside the block)
    return np.stack([random, sparse, block])


def main():
    rng = np.random.default_rng(20240607)
    out = {"pil_version": np.str_(PIL.__version__), "cases": np.asarray(CASES, dtype=np.int32)}
    for i, (ih, iw, oh, ow) in enumerate(CASES):
        x = inputs(ih, iw, rng)
        y = np.stack([np.asarray(Image.fromarray(a, "L").resize((ow, oh), Image.BILINEAR)) for a in x])
        assert y.dtype == np.uint8 and y.shape == (3, oh, ow)
        out[f"x{i}"], out[f"y{i}"] = x, y
    path = os.path.join(ROOT, "tests", "golden", "pil_resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, PIL", PIL.__version__)


if __name__ == "__main__":
    main()
