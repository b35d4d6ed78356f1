"""No GPU: the host side of the set-to-set sweep and of the sample-quality scores -- the references of tests/knn_ref.py (checked here
against an int64 brute-force double loop and on sets with known answers), the C argument contract of mmvae_knn_cross /
mmvae_knn_cross_scratch_bytes (every refusal happens before anything is enqueued, so made-up device addresses are never used), and the
ValueErrors of cross_neighbours / ball_counts / sample_quality / sample_frames."""
import importlib
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from knn_ref import ball_counts_ref, dist_matrix, knn_cross_brute, knn_cross_ref, sample_quality_ref, tie_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -3, -4


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


# ================================================================ the references
@pytest.mark.parametrize("exclude", [False, True])
def test_reference_matches_the_brute_force_loop(exclude):
    a, b = tie_case()
    d = dist_matrix(a, b)
    radius = d[torch.arange(37) % 5, torch.arange(37)].clone()           # drawn from the matrix: equality is hit in every column
    radius[4] = 0
    for k in (1, 3, 8, 36):
        rd, ri = knn_cross_ref(a, b, k, exclude)
        bd, bi, bc = knn_cross_brute(a, b, k, exclude, radius)
        assert torch.equal(rd, bd) and torch.equal(ri, bi), k
        assert rd.dtype == torch.int32 and ri.dtype == torch.int64
        assert torch.equal(ball_counts_ref(a, b, radius, exclude), bc)
    rd, ri = knn_cross_ref(a, b, 8, exclude)
    assert rd[2, :2].tolist() == [0, 0] and ri[2, :2].tolist() == [3, 30]           # a row equal to two columns: the lower index first
    order = knn_cross_ref(a, b, 36 if exclude else 37, exclude)[1][0].tolist()          # every column row 0 may see
    assert order.index(20) == order.index(11) + 1                                       # the planted tie: the lower index first
    if exclude:
        assert not bool((ri == torch.arange(5)[:, None]).any())
    every = torch.full((37,), int(d.max()), dtype=torch.int64)
    assert ball_counts_ref(a, b, every, exclude).tolist() == [36 if exclude else 37] * 5


def test_reference_scores_on_sets_with_known_answers():
    g = torch.Generator().manual_seed(9)
    real = torch.randint(0, 64, (40, 64), dtype=torch.uint8, generator=g)
    assert len({tuple(r) for r in real.tolist()}) == 40                 # all rows distinct
    same = sample_quality_ref(real, real.clone(), 3)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0 and same["accuracy"] == 0.0
    assert same["accuracy_real"] == 0.0 and same["accuracy_fake"] == 0.0 and same["density"] >= 1.0 / 3.0
    far = sample_quality_ref(real, torch.full((30, 64), 255, dtype=torch.uint8), 3)
    assert far["precision"] == far["recall"] == far["coverage"] == far["density"] == 0.0
    assert far["accuracy"] == far["accuracy_real"] == far["accuracy_fake"] == 1.0
    assert all(isinstance(v, np.float64) for v in far.values())


# ================================================================ C ABI
def test_header_declares_and_binding_binds_both_entry_points(pkg):
    L = _L()
    txt = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    assert re.search(r"MMVAE_API\s+size_t\s+mmvae_knn_cross_scratch_bytes\s*\(", txt)
    assert re.search(r"MMVAE_API\s+int\s+mmvae_knn_cross\s*\(", txt)
    for name, nargs in (("mmvae_knn_cross_scratch_bytes", 5), ("mmvae_knn_cross", 14)):
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1] and len(L.PROTOTYPES[name][1]) == nargs
    assert L.lib().mmvae_abi_version() == 3 and "#define MMVAE_ABI_VERSION 3" in txt
    assert "knn_cross.hip" in open(os.path.join(ROOT, "moving-mnist-vae_amd", "csrc", "Makefile")).read()
    assert (L.KNN_CROSS_MAX_N, L.KNN_CROSS_MAX_K, L.KNN_CROSS_MAX_D) == (1 << 20, 8, 16384)


A = 0x1000                                                  # a made-up, 16-byte aligned device address: never dereferenced
_DEFAULT = object()


def _rc(Na=300, Nb=100, D=64, k=3, exclude=0, a=A, b=A, out_dist=_DEFAULT, out_index=_DEFAULT, col_radius=None, out_count=None, scratch=A,
        scratch_bytes=None):
    lib = _L().lib()
    if out_dist is _DEFAULT:
        out_dist = A if k > 0 else None
    if out_index is _DEFAULT:
        out_index = A if k > 0 else None
    if scratch_bytes is None:
        scratch_bytes = lib.mmvae_knn_cross_scratch_bytes(Na, Nb, D, k, int(out_count is not None)) or (1 << 24)
    rc = lib.mmvae_knn_cross(a, Na, b, Nb, D, k, exclude, out_dist, out_index, col_radius, out_count, scratch, scratch_bytes, None)
    return rc, (lib.mmvae_last_error() or b"").decode()


def test_knn_cross_refuses_bad_arguments_before_any_launch(pkg):
    for name in ("Na", "Nb", "D"):
        for v in (0, -1):
            rc, msg = _rc(**{name: v})
            assert rc == ERR_ARG and "%s=%d" % (name, v) in msg, (name, v, msg)
    rc, msg = _rc(k=-1, out_dist=None, out_index=None)
    assert rc == ERR_ARG and "k=-1" in msg
    rc, msg = _rc(Nb=3, k=5)
    assert rc == ERR_ARG and "k=5" in msg and "Nb=3" in msg
    rc, msg = _rc(Nb=5, k=5, exclude=1)                     # the diagonal is gone: four columns are left
    assert rc == ERR_ARG and "k=5" in msg and "4" in msg
    assert _rc(Nb=5, k=4, exclude=1, a=None)[0] == ERR_ARG and "NULL a" in _rc(Nb=5, k=4, exclude=1, a=None)[1]     # k itself passes
    for null in ("a", "b", "scratch"):
        rc, msg = _rc(**{null: None})
        assert rc == ERR_ARG and "NULL " + null in msg, (null, msg)
    for odd in ("a", "b", "scratch"):
        rc, msg = _rc(**{odd: A + 8})
        assert rc == ERR_ARG and "aligned" in msg, (odd, msg)
    # inconsistent pointer pairs
    for kw in (dict(out_dist=None), dict(out_index=None), dict(k=0, out_dist=A, out_index=None, col_radius=A, out_count=A),
               dict(k=0, out_dist=None, out_index=A, col_radius=A, out_count=A)):
        rc, msg = _rc(**kw)
        assert rc == ERR_ARG and "out_dist" in msg and "out_index" in msg, (kw, msg)
    for kw in (dict(col_radius=A), dict(out_count=A)):
        rc, msg = _rc(**kw)
        assert rc == ERR_ARG and "col_radius" in msg and "out_count" in msg, (kw, msg)
    rc, msg = _rc(k=0)                                      # neither result asked for
    assert rc == ERR_ARG and "nothing" in msg
    for name in ("Na", "Nb"):
        rc, msg = _rc(**{name: (1 << 20) + 1})
        assert rc == ERR_UNSUPPORTED and "%s=%d" % (name, (1 << 20) + 1) in msg
    rc, msg = _rc(k=9)
    assert rc == ERR_UNSUPPORTED and "k=9" in msg
    for D in (8, 24, 1000, 16400, 32768):
        rc, msg = _rc(D=D)
        assert rc == ERR_UNSUPPORTED and "D=%d" % D in msg, (D, msg)
    for kw in (dict(), dict(col_radius=A, out_count=A), dict(k=0, col_radius=A, out_count=A)):
        need = _L().lib().mmvae_knn_cross_scratch_bytes(300, 100, 64, kw.get("k", 3), int("out_count" in kw))
        for have in (0, need - 1):
            rc, msg = _rc(scratch_bytes=have, **kw)
            assert rc == ERR_WORKSPACE and "scratch_bytes=%d" % have in msg and str(need) in msg, (have, msg)


def test_scratch_bytes_is_zero_for_refused_shapes_and_positive_otherwise(pkg):
    L = _L()
    fn = L.lib().mmvae_knn_cross_scratch_bytes
    up16 = lambda v: (v + 15) // 16 * 16
    for (Na, Nb, D, k, c) in ((1, 1, 16, 1, 0), (5, 37, 16, 8, 1), (64, 20000, 4096, 3, 1), (259, 517, 784, 0, 1), (200, 5000, 64, 3, 0),
                              (20000, 20000, 4096, 3, 1), (40000, 40000, 4096, 3, 1), (1 << 20, 1 << 20, 16384, 8, 1)):
        got, ranges = fn(Na, Nb, D, k, c), L.knn_cross_ranges(Na, Nb)
        assert 1 <= ranges <= L.KNN_CROSS_MAX_RANGES
        assert got == up16(4 * Na) + up16(4 * Nb) + 2 * ranges * Na * k * 8 + (up16(2 * ranges * Na * 4) if c else 0) > 0, (Na, Nb, D, k, c)
    # the column split fills the chip at few rows and stays small at many
    assert L.knn_cross_ranges(64, 20000) == 128 and L.knn_cross_ranges(20000, 20000) == 14 and L.knn_cross_ranges(40000, 40000) == 7
    for bad in ((0, 100, 64, 3, 0), (100, 0, 64, 3, 0), (100, 100, 24, 3, 0), (100, 100, 32768, 3, 0), (100, 100, 64, 9, 0),
                (100, 100, 64, -1, 1), (100, 3, 64, 5, 0), ((1 << 20) + 1, 100, 64, 3, 0), (100, (1 << 20) + 1, 64, 3, 0), (100, 100, 64, 0, 0)):
        assert fn(*bad) == 0, bad


# ================================================================ Python surface
def test_python_surface_refuses_before_any_launch(pkg):
    a, b = torch.zeros((4, 8, 8), dtype=torch.uint8), torch.zeros((30, 8, 8), dtype=torch.uint8)
    r = torch.zeros(30, dtype=torch.int32)
    calls = (("cross_neighbours", lambda x, y, **kw: pkg.cross_neighbours(x, y, **kw)),
             ("ball_counts", lambda x, y, **kw: pkg.ball_counts(x, y, kw.pop("radius", r), **kw)),
             ("sample_quality", lambda x, y, **kw: pkg.sample_quality(x, y, **kw)))
    for name, fn in calls:
        with pytest.raises(ValueError, match="GPU"):
            fn(a, b)                                        # host tensors (everything else about them is fine)
        with pytest.raises(ValueError, match="GPU"):
            fn(a.view(4, 64), b.view(30, 1, 8, 8))
        with pytest.raises(ValueError, match="uint8"):
            fn(a.float(), b)
        with pytest.raises(ValueError, match="uint8"):
            fn(a, b.to(torch.int64))
        with pytest.raises(ValueError, match="uint8"):
            fn(a.numpy(), b)
        with pytest.raises(ValueError, match="do not match"):
            fn(torch.zeros((4, 4, 12), dtype=torch.uint8), b)
        with pytest.raises(ValueError, match="must have shape"):
            fn(torch.zeros((4, 2, 8, 8), dtype=torch.uint8), b)
        with pytest.raises(ValueError, match="D=24"):
            fn(torch.zeros((4, 4, 6), dtype=torch.uint8), torch.zeros((30, 4, 6), dtype=torch.uint8))
        with pytest.raises(ValueError, match="D=20480"):
            fn(torch.zeros((9, 128, 160), dtype=torch.uint8), torch.zeros((9, 128, 160), dtype=torch.uint8))
        if name != "ball_counts":
            with pytest.raises(ValueError, match="k=0"):
                fn(a, b, k=0)
            with pytest.raises(ValueError, match="k=9"):
                fn(a, b, k=9)
    with pytest.raises(ValueError, match="k=5"):
        pkg.cross_neighbours(a, b[:4], k=5)
    with pytest.raises(ValueError, match="self excluded"):
        pkg.cross_neighbours(a, a, k=4, exclude_self=True)                 # 4 rows: 3 columns are left
    with pytest.raises(ValueError, match="GPU"):
        pkg.cross_neighbours(a, a, k=3, exclude_self=True)
    with pytest.raises(ValueError, match="Na=0"):
        pkg.cross_neighbours(a[:0], b)
    with pytest.raises(ValueError, match="negative"):
        pkg.ball_counts(a, b, torch.tensor([5] * 29 + [-1], dtype=torch.int64))
    with pytest.raises(ValueError, match="int32 or int64"):
        pkg.ball_counts(a, b, r.float())
    with pytest.raises(ValueError, match="radius of shape"):
        pkg.ball_counts(a, b, r[:29])
    with pytest.raises(ValueError, match="k=3 neighbours inside fake"):
        pkg.sample_quality(b, a[:3], k=3)                   # k neighbours inside a set need k + 1 rows
    with pytest.raises(ValueError, match="lut"):
        pkg.sample_quality(a, b, lut=torch.zeros(255, dtype=torch.uint8))
    with pytest.raises(ValueError, match="lut"):
        pkg.sample_quality(a, b, lut=torch.zeros(256, dtype=torch.int64))


def test_tensors_on_different_devices_are_refused(pkg):
    """One side on the host and one on another device; a meta tensor stands in for a device this machine need not have."""
    a, b = torch.zeros((4, 64), dtype=torch.uint8), torch.zeros((30, 64), dtype=torch.uint8, device="meta")
    with pytest.raises(ValueError, match="a on cpu, b on meta"):
        pkg.cross_neighbours(a, b)
    with pytest.raises(ValueError, match="a on meta, b on cpu"):
        pkg.sample_quality(b, a, k=1)
    with pytest.raises(ValueError, match="radius on meta"):
        pkg.ball_counts(a, a, torch.zeros(4, dtype=torch.int32, device="meta"))


def test_new_names_are_exported(pkg):
    samples = importlib.import_module("moving-mnist-vae_amd.samples")
    main = importlib.import_module("moving-mnist-vae_amd.main")
    for name in ("cross_neighbours", "ball_counts", "sample_quality", "sample_quality_to_host", "sample_frames"):
        assert getattr(pkg, name) is getattr(samples, name) and getattr(main, name) is getattr(samples, name), name
    assert list(inspect.signature(pkg.cross_neighbours).parameters) == ["a", "b", "k", "exclude_self"]
    assert list(inspect.signature(pkg.ball_counts).parameters) == ["a", "b", "radius", "exclude_self"]
    assert list(inspect.signature(pkg.sample_quality).parameters) == ["real", "fake", "k", "lut"]
    assert inspect.signature(pkg.sample_quality).parameters["k"].default == 3
    assert list(inspect.signature(pkg.sample_frames).parameters) == ["model", "n", "data_mean", "data_std", "centres", "generator", "z", "batch"]
    p = inspect.signature(pkg.evaluate).parameters
    assert p["sample_quality"].default == 0 and list(p)[-1] == "sample_quality"
    for phrase in ("real", "pooled index", "equal sizes", "pixel space"):
        assert phrase in pkg.sample_quality.__doc__, phrase
    assert "sample_pixels" in pkg.sample_frames.__doc__
