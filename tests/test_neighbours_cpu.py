"""No GPU: the host side of the nearest-frames search -- the torch reference the GPU tests compare against (checked here against a
brute-force integer loop), the C argument contract of mmvae_nearest_frames / mmvae_nearest_frames_scratch_bytes (every refusal happens
before anything is enqueued, so made-up device addresses are never used), and the ValueErrors of nearest_frames / neighbour_sheet."""
import importlib
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from knn_ref import knn_cross_brute, knn_cross_ref, tie_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -3, -4


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


# ================================================================ the reference (tests/knn_ref.py), under the names the GPU tests import
def nearest_ref(queries, frames, k, lut=None, chunk=8192):
    return knn_cross_ref(queries, frames, k, lut=lut, chunk=chunk)


def nearest_brute(queries, frames, k, lut=None):
    return knn_cross_brute(queries, frames, k, lut=lut)[:2]


@pytest.mark.parametrize("with_lut", [False, True])
def test_reference_matches_the_brute_force_loop(with_lut):
    q, f = tie_case()                                       # a tie between two frames, four identical frames, a query's copy at two indices
    lut = torch.randperm(256, generator=torch.Generator().manual_seed(4)).to(torch.uint8) if with_lut else None
    if with_lut:
        f[3], f[30] = 0, 0
        q[2] = lut[0]
    for k in (1, 8, 37):
        rd, ri = nearest_ref(q, f, k, lut)
        bd, bi = nearest_brute(q, f, k, lut)
        assert torch.equal(rd, bd) and torch.equal(ri, bi), k
        assert rd.dtype == torch.int32 and ri.dtype == torch.int64
    rd, ri = nearest_ref(q, f, 8, lut)
    assert rd[2, 0] == 0 and rd[2, 1] == 0 and ri[2, :2].tolist() == [3, 30]
    assert torch.equal(nearest_ref(q, f, 8, lut, chunk=7)[1], ri)


def test_reference_reaches_the_largest_distance():
    q = torch.zeros((1, 16384), dtype=torch.uint8)
    f = torch.full((2, 16384), 255, dtype=torch.uint8)
    f[1] = 0
    d, i = nearest_ref(q, f, 2)
    assert d.tolist() == [[0, 1065369600]] and i.tolist() == [[1, 0]]


# ================================================================ C ABI
def test_header_declares_and_binding_binds_both_entry_points(pkg):
    L = _L()
    txt = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    assert re.search(r"MMVAE_API\s+size_t\s+mmvae_nearest_frames_scratch_bytes\s*\(", txt)
    assert re.search(r"MMVAE_API\s+int\s+mmvae_nearest_frames\s*\(", txt)
    for name, nargs in (("mmvae_nearest_frames_scratch_bytes", 4), ("mmvae_nearest_frames", 12)):
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1] and len(L.PROTOTYPES[name][1]) == nargs
    assert L.lib().mmvae_abi_version() == 3 and "#define MMVAE_ABI_VERSION 3" in txt
    assert "neighbours.hip" in open(os.path.join(ROOT, "moving-mnist-vae_amd", "csrc", "Makefile")).read()


A = 0x1000                                                  # a made-up, 16-byte aligned device address: never dereferenced


def _rc(M=4, F=100, D=64, k=5, queries=A, frames=A, lut=None, out_dist=A, out_index=A, scratch=A, scratch_bytes=None):
    lib = _L().lib()
    if scratch_bytes is None:
        scratch_bytes = lib.mmvae_nearest_frames_scratch_bytes(M, F, D, k) or (1 << 20)
    rc = lib.mmvae_nearest_frames(queries, M, frames, F, D, lut, k, out_dist, out_index, scratch, scratch_bytes, None)
    return rc, (lib.mmvae_last_error() or b"").decode()


def test_nearest_frames_refuses_bad_arguments_before_any_launch(pkg):
    for name in ("M", "F", "D", "k"):
        for v in (0, -1):
            rc, msg = _rc(**{name: v})
            assert rc == ERR_ARG and "%s=%d" % (name, v) in msg, (name, v, msg)
    rc, msg = _rc(F=3, k=5)
    assert rc == ERR_ARG and "k=5" in msg and "F=3" in msg
    for null in ("queries", "frames", "out_dist", "out_index", "scratch"):
        rc, msg = _rc(**{null: None})
        assert rc == ERR_ARG and null in msg, (null, msg)
    for odd in ("queries", "frames", "scratch"):
        rc, msg = _rc(**{odd: A + 8})
        assert rc == ERR_ARG and "aligned" in msg, (odd, msg)
    rc, msg = _rc(M=65)
    assert rc == ERR_UNSUPPORTED and "M=65" in msg
    rc, msg = _rc(k=9, F=100)
    assert rc == ERR_UNSUPPORTED and "k=9" in msg
    for D in (8, 24, 1000, 16400, 32768):
        rc, msg = _rc(D=D)
        assert rc == ERR_UNSUPPORTED and "D=%d" % D in msg, (D, msg)
    rc, msg = _rc(F=2 ** 31)
    assert rc == ERR_UNSUPPORTED and "F=2147483648" in msg
    need = _L().lib().mmvae_nearest_frames_scratch_bytes(4, 100, 64, 5)
    for have in (0, need - 1):
        rc, msg = _rc(scratch_bytes=have)
        assert rc == ERR_WORKSPACE and "scratch_bytes=%d" % have in msg and str(need) in msg, (have, msg)
    assert _rc(lut=None, M=0)[0] == ERR_ARG                  # a NULL lut is no error of its own


def test_scratch_bytes_is_positive_and_grows_with_the_frames(pkg):
    fn = _L().lib().mmvae_nearest_frames_scratch_bytes
    for (M, D, k) in ((1, 16, 1), (6, 784, 5), (64, 4096, 8), (16, 16384, 8)):
        last = 0
        for F in (k, 16, 17, 64, 65, 1000, 4096, 32768, 32769, 200000, 10 ** 7, 2 ** 31 - 1):
            if F < k:
                continue
            b = fn(M, F, D, k)
            assert b > 0 and b >= last, (M, D, k, F, b, last)
            assert b >= M * k * 8 and b < (64 << 20)
            last = b
    for bad in ((0, 100, 64, 5), (65, 100, 64, 5), (4, 100, 24, 5), (4, 100, 64, 9), (4, 3, 64, 5), (4, 2 ** 31, 64, 5), (4, 100, 64, 0)):
        assert fn(*bad) == 0, bad


# ================================================================ Python surface
def test_python_surface_refuses_before_any_launch(pkg):
    q, f = torch.zeros((4, 8, 8), dtype=torch.uint8), torch.zeros((30, 8, 8), dtype=torch.uint8)
    for fn in (pkg.nearest_frames, pkg.neighbour_sheet):
        with pytest.raises(ValueError, match="GPU"):
            fn(q, f)                                        # host tensors (everything else about them is fine)
        with pytest.raises(ValueError, match="GPU"):
            fn(q.view(4, 64), f.view(3, 10, 8, 8), k=3, lut=torch.arange(256, dtype=torch.uint8))
        with pytest.raises(ValueError, match="uint8"):
            fn(q.float(), f)
        with pytest.raises(ValueError, match="uint8"):
            fn(q, f.to(torch.int64))
        with pytest.raises(ValueError, match="uint8"):
            fn(q.numpy(), f)
        with pytest.raises(ValueError, match="do not match"):
            fn(torch.zeros((4, 4, 16), dtype=torch.uint8), f)
        with pytest.raises(ValueError, match="do not match"):
            fn(torch.zeros((4, 48), dtype=torch.uint8), f)
        with pytest.raises(ValueError, match="queries must have shape"):
            fn(torch.zeros((4, 2, 8, 8), dtype=torch.uint8), f)
        with pytest.raises(ValueError, match="k=0"):
            fn(q, f, k=0)
        with pytest.raises(ValueError, match="k=9"):
            fn(q, f, k=9)
        with pytest.raises(ValueError, match="M=65"):
            fn(torch.zeros((65, 8, 8), dtype=torch.uint8), f)
        with pytest.raises(ValueError, match="M=0"):
            fn(torch.zeros((0, 8, 8), dtype=torch.uint8), f)
        with pytest.raises(ValueError, match="D=24"):
            fn(torch.zeros((4, 4, 6), dtype=torch.uint8), torch.zeros((30, 4, 6), dtype=torch.uint8))
        with pytest.raises(ValueError, match="F=3"):
            fn(q, f[:3], k=5)
        with pytest.raises(ValueError, match="lut"):
            fn(q, f, lut=torch.zeros(255, dtype=torch.uint8))
        with pytest.raises(ValueError, match="lut"):
            fn(q, f, lut=torch.zeros(256, dtype=torch.int64))
    with pytest.raises(ValueError, match="D=20480"):
        pkg.nearest_frames(torch.zeros((1, 128, 160), dtype=torch.uint8), torch.zeros((9, 128, 160), dtype=torch.uint8))
    with pytest.raises(ValueError, match="k=8"):
        pkg.neighbour_sheet(q, f, k=8)                      # a sheet has 8 columns, one of them the queries
    with pytest.raises(ValueError, match="display_lut"):
        pkg.neighbour_sheet(q, f, display_lut=torch.zeros(17, dtype=torch.uint8))
    with pytest.raises(ValueError, match="display_lut"):
        pkg.neighbour_sheet(q, f, display_lut=torch.zeros(4))
    with pytest.raises(ValueError, match="GPU"):
        pkg.plot_neighbours(q, f, "unused", 0, 0, k=3)
    assert not os.path.exists("unused")


def test_new_names_are_exported(pkg):
    neighbours = importlib.import_module("moving-mnist-vae_amd.neighbours")
    panels = importlib.import_module("moving-mnist-vae_amd.panels")
    main = importlib.import_module("moving-mnist-vae_amd.main")
    assert callable(neighbours.nearest_frames) and callable(panels.neighbour_sheet) and callable(panels.plot_neighbours)
    for name, home in (("nearest_frames", neighbours), ("neighbour_sheet", panels), ("plot_neighbours", panels)):
        assert getattr(pkg, name) is getattr(home, name) and getattr(main, name) is getattr(home, name), name
    import inspect
    assert inspect.signature(pkg.nearest_frames).parameters["k"].default == 5
    assert list(inspect.signature(pkg.neighbour_sheet).parameters) == ["queries", "frames", "k", "lut", "display_lut"]
    assert list(inspect.signature(pkg.plot_neighbours).parameters)[:5] == ["queries", "frames", "directory", "epoch", "plot_count"]
    L = _L()
    assert (L.NEAREST_MAX_M, L.NEAREST_MAX_K, L.NEAREST_MAX_D) == (64, 8, 16384)
