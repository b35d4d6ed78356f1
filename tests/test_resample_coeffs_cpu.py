"""CPU: mmvae_resample_coeffs, the host half of the device resize -- the taps of PIL's 8-bit antialiased bilinear resample --
through ctypes, exactly: against a Python restatement of the algorithm (tests/resize_ref.py) and, applied in a plain numpy two-pass
resize, against PIL's own bytes (tests/golden/pil_resize.npz, written by tools/make_resize_fixture.py)."""
import ctypes
import importlib

import numpy as np
import pytest

import resize_ref as R
from conftest import load_golden

FIXTURE_PAIRS = [(64, 32), (64, 56), (64, 28), (64, 9), (64, 33), (64, 63), (64, 64), (28, 14), (28, 20), (28, 9), (40, 20)]
PAIRS = FIXTURE_PAIRS + [(128, 1), (1, 128), (128, 128), (5, 7), (7, 5)]


@pytest.fixture(scope="module")
def L(pkg):
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _tables(L, in_size, out_size):
    """(rc, ksize, bounds, coeffs) through the two-call protocol: size first, then fill."""
    ksize = ctypes.c_int(-7)
    rc = L.lib().mmvae_resample_coeffs(in_size, out_size, ctypes.byref(ksize), None, None)
    if rc != 0:
        return rc, ksize.value, None, None
    bounds = np.full((out_size, 2), -1, dtype=np.int32)
    coeffs = np.full((out_size, ksize.value), -1, dtype=np.int32)
    k2 = ctypes.c_int(-7)
    rc = L.lib().mmvae_resample_coeffs(in_size, out_size, ctypes.byref(k2), bounds.ctypes.data, coeffs.ctypes.data)
    assert k2.value == ksize.value
    return rc, ksize.value, bounds, coeffs


@pytest.mark.parametrize("in_size,out_size", PAIRS)
def test_tables_equal_the_restated_algorithm(L, in_size, out_size):
    rc, ksize, bounds, coeffs = _tables(L, in_size, out_size)
    assert rc == 0
    want_ksize, want_bounds, want_coeffs = R.coeffs(in_size, out_size)
    assert ksize == want_ksize
    assert np.array_equal(bounds, want_bounds)
    assert np.array_equal(coeffs, want_coeffs)
    first, count = bounds[:, 0], bounds[:, 1]
    assert (first >= 0).all() and (count >= 1).all() and (count <= ksize).all() and (first + count <= in_size).all()
    for xx in range(out_size):                                          # zero behind the tap count
        assert not coeffs[xx, count[xx]:].any()
    # the int32 bound of the kernel: 255 * sum + 2^21 < 2^31
    assert 255 * int(coeffs.sum(axis=1).max()) + (1 << 21) < 2 ** 31


def test_numpy_resize_from_the_library_tables_equals_pil(L):
    g = load_golden("pil_resize")
    cases = g["cases"]
    assert len(cases) == 11 and str(g["pil_version"])
    seen = set()
    for i, (ih, iw, oh, ow) in enumerate(cases.tolist()):
        x, y = g[f"x{i}"], g[f"y{i}"]
        assert x.shape == (3, ih, iw) and y.shape == (3, oh, ow)
        _, _, hb, hc = _tables(L, iw, ow)
        _, _, vb, vc = _tables(L, ih, oh)
        assert np.array_equal(R.resize_with(x, (hb, hc), (vb, vc)), y), (ih, iw, oh, ow)
        seen.add((ih, oh))
    assert seen == set(FIXTURE_PAIRS)


@pytest.mark.parametrize("n", [1, 9, 28, 64, 128])
def test_equal_sizes_give_the_identity(L, n):
    rc, ksize, bounds, coeffs = _tables(L, n, n)
    assert rc == 0 and ksize == 3
    x = np.random.default_rng(n).integers(0, 256, size=(2, n), dtype=np.uint8)
    assert np.array_equal(R.one_pass(x, bounds, coeffs), x)
    for xx in range(n):                                                 # one tap of weight 1 on the pixel itself
        row = np.zeros(n, dtype=np.int64)
        row[bounds[xx, 0]:bounds[xx, 0] + bounds[xx, 1]] = coeffs[xx, :bounds[xx, 1]]
        assert row[xx] == 1 << 22 and row.sum() == 1 << 22


@pytest.mark.parametrize("in_size,out_size", [(0, 8), (8, 0), (129, 8), (8, 129), (-1, 4)])
def test_sizes_out_of_range_are_argument_errors(L, in_size, out_size):
    rc, _, _, _ = _tables(L, in_size, out_size)
    assert rc == -1                                                     # MMVAE_ERR_ARG
    msg = L.lib().mmvae_last_error()
    assert msg and str(in_size).encode() in msg


def test_null_tables_return_only_ksize(L):
    for (i, o), want in {(64, 32): 5, (64, 9): 17, (28, 32): 3, (128, 1): 257}.items():
        ksize = ctypes.c_int(0)
        assert L.lib().mmvae_resample_coeffs(i, o, ctypes.byref(ksize), None, None) == 0
        assert ksize.value == want == R.coeffs(i, o)[0]
    # one table without the other is an error, and writes nothing
    bounds = np.full((32, 2), -1, dtype=np.int32)
    ksize = ctypes.c_int(0)
    assert L.lib().mmvae_resample_coeffs(64, 32, ctypes.byref(ksize), bounds.ctypes.data, None) == -1
    assert (bounds == -1).all()
