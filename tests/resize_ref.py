"""Integer restatement of PIL's 8-bit antialiased bilinear resize (precompute_coeffs / normalize_coeffs_8bpc and the two passes)
in Python / numpy: the reference the resize tests compare the library against.  Python floats are f64 and int() truncates, as the
C casts do; nothing here calls the library."""
import math

import numpy as np

PRECISION_BITS = 22


def coeffs(in_size, out_size):
    """(ksize, bounds int32 [out, 2] = (first, count), coeffs int32 [out, ksize])."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / fs
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = []
        ww = 0.0
        for x in range(n):
            t = abs((x + xmin - center + 0.5) * ss)
            v = 1.0 - t if t < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * 4194304.0) if v < 0 else int(0.5 + v * 4194304.0)
        bounds[xx] = (xmin, n)
    return ksize, bounds, kk


def one_pass(planes, bounds, kk):
    """Resample the LAST axis of uint8 `planes` [..., in] -> [..., out] with the tables of coeffs()."""
    p = planes.astype(np.int64)
    out = np.empty(planes.shape[:-1] + (bounds.shape[0],), dtype=np.uint8)
    for xx, (first, n) in enumerate(bounds):
        acc = (1 << (PRECISION_BITS - 1)) + (p[..., first:first + n] * kk[xx, :n].astype(np.int64)).sum(axis=-1)
        assert acc.max(initial=0) < 2 ** 31 and acc.min(initial=0) >= 0                   # int32 suffices
        out[..., xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize_with(planes, h_tables, v_tables):
    """Horizontal pass (along W) first, then the vertical one, uint8 behind each; tables = (bounds, coeffs)."""
    mid = one_pass(planes, *h_tables)                                                    # [..., H, out_w]
    return np.ascontiguousarray(np.swapaxes(one_pass(np.swapaxes(mid, -1, -2), *v_tables), -1, -2))


def resize(planes, size):
    """uint8 [..., H, W] -> [..., out_h, out_w]; size an int or (h, w)."""
    out_h, out_w = (size, size) if isinstance(size, int) else size
    H, W = planes.shape[-2:]
    return resize_with(planes, coeffs(W, out_w)[1:], coeffs(H, out_h)[1:])


def label_table(centres):
    """Label of every byte under the quantise kernel's f32 rule (x = b / 255, squared distance, lowest index wins ties)."""
    c = np.asarray(centres, dtype=np.float32).reshape(-1)
    x = np.arange(256, dtype=np.float32) / np.float32(255.0)
    d = (x[:, None] - c[None, :]) * (x[:, None] - c[None, :])
    assert d.dtype == np.float32
    return np.argmin(d, axis=1).astype(np.int64)
