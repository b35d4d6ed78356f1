"""No GPU: the host side of the per-tensor histograms -- the numpy restatement of the binning rule that tests/test_tensor_hist_gpu.py
compares the kernels with (checked here against a hand-worked example and against torch.histc where "divide first" and "multiply
first" coincide), the C argument contract of mmvae_tensor_hist (every refusal happens before anything is enqueued, so the made-up
device addresses are never used), the segment table and chunk list of a small VAE and a small PixelVAE, and the export surface."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_WORKSPACE = -1, -3
BINS = 64


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _mon():
    return importlib.import_module("moving-mnist-vae_amd.monitor")


# ================================================================ the reference
def hist_ref(x):
    """The rule of include/mmvae.h for one tensor, in numpy f32: dict(counts int64 (64,), lo, hi np.float32, n_finite, n_nonfinite,
    n_zero ints, sum, sumsq f64, abs_sum f64).  Every f32 operation is a single correctly rounded numpy operation on float32 arrays."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    f = x[np.isfinite(x)]
    out = {"n_finite": int(f.size), "n_nonfinite": int(x.size - f.size), "n_zero": int((f == 0).sum()),
           "sum": float(f.astype(np.float64).sum()), "sumsq": float((f.astype(np.float64) ** 2).sum()),
           "abs_sum": float(np.abs(f.astype(np.float64)).sum())}
    if f.size == 0:
        out.update(counts=np.zeros(BINS, dtype=np.int64), lo=np.float32(0), hi=np.float32(0))
        return out
    lo, hi = np.float32(f.min()), np.float32(f.max())
    if lo == hi:
        lo, hi = np.float32(lo - np.float32(1)), np.float32(hi + np.float32(1))
    with np.errstate(all="ignore"):
        q = ((f - lo) * np.float32(64)) / np.float32(hi - lo)
    assert q.dtype == np.float32
    b = np.minimum(q.astype(np.int64), BINS - 1)
    out.update(counts=np.bincount(b, minlength=BINS).astype(np.int64), lo=lo, hi=hi)
    return out


def test_reference_matches_a_hand_worked_example():
    # lo = -1, hi = 3, width 4: bin = int((x + 1) * 16), the maximum folded into bin 63
    x = [-1.0, -0.97, -0.9375, 0.0, -0.0, 1.0, 2.999, 3.0, 3.0, float("nan"), float("inf"), float("-inf")]
    r = hist_ref(x)
    want = np.zeros(BINS, dtype=np.int64)
    for b in (0, 0, 1, 16, 16, 32, 63, 63, 63):
        want[b] += 1
    assert np.array_equal(r["counts"], want)
    assert (r["lo"], r["hi"], r["n_finite"], r["n_nonfinite"], r["n_zero"]) == (-1.0, 3.0, 9, 3, 2)
    assert r["sum"] == pytest.approx(-1 - 0.97 - 0.9375 + 1 + 2.999 + 6, abs=1e-6)
    # a constant: the range is widened by one on either side, the value lands in the middle bin
    r = hist_ref([0.5] * 7)
    assert (r["lo"], r["hi"]) == (-0.5, 1.5) and r["counts"][32] == 7 and r["counts"].sum() == 7
    # nothing finite: no range, no counts
    r = hist_ref([float("nan"), float("inf")])
    assert (r["lo"], r["hi"], r["n_finite"], r["n_nonfinite"]) == (0.0, 0.0, 0, 2) and r["counts"].sum() == 0
    r = hist_ref([])
    assert (r["lo"], r["hi"], r["n_finite"], r["n_nonfinite"]) == (0.0, 0.0, 0, 0) and r["counts"].sum() == 0


def test_reference_agrees_with_torch_histc_where_both_orders_coincide():
    """lo = 0, hi = 64, integer data: (x - 0) * 64 / 64 and (x - 0) / 64 * 64 are both exact, so ATen's CPU histc (divide first) is a
    yardstick here."""
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 65, (5000,), generator=g).float()
    x[0], x[1] = 0.0, 64.0
    r = hist_ref(x.numpy())
    assert (r["lo"], r["hi"]) == (0.0, 64.0)
    assert np.array_equal(r["counts"], torch.histc(x, bins=64, min=0, max=64).long().numpy())
    assert r["counts"][63] == int(((x == 63) | (x == 64)).sum())


# ================================================================ C ABI
def test_header_declares_and_binding_binds_the_entry_points(pkg):
    L = _L()
    txt = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    assert re.search(r"MMVAE_API\s+int\s+mmvae_tensor_hist\s*\(", txt)
    assert re.search(r"MMVAE_API\s+int64_t\s+mmvae_tensor_hist_chunks\s*\(", txt)
    assert re.search(r"MMVAE_API\s+size_t\s+mmvae_tensor_hist_scratch_bytes\s*\(", txt)
    for name, nargs in (("mmvae_tensor_hist", 15), ("mmvae_tensor_hist_chunks", 5), ("mmvae_tensor_hist_scratch_bytes", 2)):
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1] and len(L.PROTOTYPES[name][1]) == nargs
        decl = re.search(r"MMVAE_API[^;(]*\b%s\s*\(([^;]*?)\)\s*;" % name, txt).group(1)
        assert len(decl.split(",")) == nargs, name
    assert L.lib().mmvae_abi_version() == 3 and "#define MMVAE_ABI_VERSION 3" in txt and L.ABI_VERSION == 3
    assert "#define MMVAE_TENSOR_HIST_BINS 64" in txt and "#define MMVAE_TENSOR_HIST_STATS 8" in txt
    assert (_mon().BINS, _mon().STATS) == (64, 8)
    assert "tensor_hist.hip" in open(os.path.join(ROOT, "moving-mnist-vae_amd", "csrc", "Makefile")).read()


A = 0x1000                                                  # a made-up, aligned device address: never dereferenced
SEG = [[3, 10], [20, 0], [21, 100]]


def _rc(seg=SEG, chunks="auto", flat=A, flat_numel=1000, seg_host="auto", seg_dev=A, chunks_host="auto", chunks_dev=A, counts=A, lo=A, hi=A,
        stats=A, scratch=A, scratch_bytes=None, T=None, n_chunks=None):
    lib = _L().lib()
    seg = np.array(seg, dtype=np.int64).reshape(-1, 2)
    if isinstance(chunks, str):
        chunks = _mon().chunk_list(seg, 64) if (seg >= 0).all() else np.zeros((0, 3), dtype=np.int64)
    chunks = np.ascontiguousarray(np.array(chunks, dtype=np.int64).reshape(-1, 3))
    T = seg.shape[0] if T is None else T
    n = chunks.shape[0] if n_chunks is None else n_chunks
    if scratch_bytes is None:
        scratch_bytes = lib.mmvae_tensor_hist_scratch_bytes(max(T, 1), max(n, 0)) or 64
    sh = seg.ctypes.data if isinstance(seg_host, str) else seg_host
    ch = (chunks.ctypes.data if chunks.shape[0] else None) if isinstance(chunks_host, str) else chunks_host
    rc = lib.mmvae_tensor_hist(flat, flat_numel, sh, seg_dev, T, ch, chunks_dev, n, counts, lo, hi, stats, scratch, scratch_bytes, None)
    return rc, (lib.mmvae_last_error() or b"").decode()


def test_tensor_hist_refuses_bad_arguments_before_any_launch(pkg):
    for null in ("flat", "seg_host", "seg_dev", "chunks_host", "chunks_dev", "counts", "lo", "hi", "stats", "scratch"):
        rc, msg = _rc(**{null: None})
        assert rc == ERR_ARG and "NULL" in msg, (null, rc, msg)
    for T in (0, -1):
        rc, msg = _rc(T=T)
        assert rc == ERR_ARG and "T=%d" % T in msg
    rc, msg = _rc(n_chunks=-1)
    assert rc == ERR_ARG and "n_chunks=-1" in msg
    rc, msg = _rc(seg=[[3, 10], [-1, 4]])
    assert rc == ERR_ARG and "offset=-1" in msg
    rc, msg = _rc(seg=[[3, -10], [5, 4]])
    assert rc == ERR_ARG and "numel=-10" in msg
    rc, msg = _rc(flat_numel=120)                           # the last segment ends at 121
    assert rc == ERR_ARG and "flat_numel=120" in msg and "segment 2" in msg
    assert _rc(seg=[[2 ** 62, 2 ** 62]], chunks=[], flat_numel=2 ** 62)[0] == ERR_ARG       # (no overflow in offset + numel)
    for bad, word in (([0, 0, 11], "leaves segment 0"), ([0, 10, 1], "leaves segment 0"), ([0, -1, 2], "leaves segment 0"),
                      ([0, 2, -1], "leaves segment 0"), ([1, 0, 1], "leaves segment 1"), ([2, 64, 37], "leaves segment 2"),
                      ([3, 0, 1], "segment 3"), ([-1, 0, 1], "segment -1"), ([0, 2 ** 62, 2 ** 62], "leaves segment 0")):
        rc, msg = _rc(chunks=[[0, 0, 10], bad])
        assert rc == ERR_ARG and word in msg and "chunk 1" in msg, (bad, rc, msg)
    need = _L().lib().mmvae_tensor_hist_scratch_bytes(3, 3)
    assert need >= 3 * 7 * 8
    for have in (0, need - 1):
        rc, msg = _rc(scratch_bytes=have)
        assert rc == ERR_WORKSPACE and "scratch_bytes=%d" % have in msg and str(need) in msg, (have, msg)
    rc, msg = _rc(scratch=A + 4)
    assert rc == ERR_ARG and "aligned" in msg


def test_chunk_helper_tiles_every_segment_once(pkg):
    lib, mon = _L().lib(), _mon()
    seg = np.array([[1, 0], [1, 1], [7, 63], [99, 64], [200, 65], [400, 3 * 64 + 17], [1000, 0]], dtype=np.int64)
    ch = mon.chunk_list(seg, 64)
    assert ch.dtype == np.int64 and ch.shape == (0 + 1 + 1 + 1 + 2 + 4 + 0, 3)
    assert ch.tolist() == [[1, 0, 1], [2, 0, 63], [3, 0, 64], [4, 0, 64], [4, 64, 1], [5, 0, 64], [5, 64, 64], [5, 128, 64], [5, 192, 17]]
    assert lib.mmvae_tensor_hist_chunks(seg.ctypes.data, 7, 64, None, 0) == 9
    small = np.full((2, 3), -7, dtype=np.int64)
    assert lib.mmvae_tensor_hist_chunks(seg.ctypes.data, 7, 64, small.ctypes.data, 2) == 9 and (small == -7).all()     # too small: only counted
    assert lib.mmvae_tensor_hist_chunks(None, 7, 64, None, 0) == ERR_ARG
    assert lib.mmvae_tensor_hist_chunks(seg.ctypes.data, 0, 64, None, 0) == ERR_ARG
    assert lib.mmvae_tensor_hist_chunks(seg.ctypes.data, 7, 0, None, 0) == ERR_ARG
    neg = np.array([[0, -1]], dtype=np.int64)
    assert lib.mmvae_tensor_hist_chunks(neg.ctypes.data, 1, 64, None, 0) == ERR_ARG
    assert lib.mmvae_tensor_hist_scratch_bytes(0, 5) == 0 and lib.mmvae_tensor_hist_scratch_bytes(3, -1) == 0
    assert lib.mmvae_tensor_hist_scratch_bytes(3, 0) > 0


# ================================================================ Python surface
def _models():
    M = importlib.import_module("moving-mnist-vae_amd.model")
    return {"vae": M.VAE(1, 32, 1, 2, 8, False, False, 4, "ReLu", 1, 1, 0, True, 0.1, 16),
            "pixelvae": M.VAE(1, 16, 2, 2, 32, True, False, 3, "ReLu", 1, 1, 0, True, 0.0, 32)}


@pytest.mark.parametrize("kind", ["vae", "pixelvae"])
def test_tables_cover_every_parameter_exactly_once_in_order(pkg, kind):
    mon = _mon()
    m = _models()[kind]
    names, seg = mon.segment_table(m)
    named = list(m.named_parameters())
    assert names == [n for n, _ in named] and seg.shape == (len(named), 2) and seg.dtype == np.int64
    if kind == "pixelvae":
        assert names[0].startswith("pixelcnn.") and m._poff > 0
        first_net = next(i for i, n in enumerate(names) if not n.startswith("pixelcnn."))
        assert seg[first_net, 0] == m._poff and all(n.startswith("pixelcnn.") for n in names[:first_net])
    covered = np.zeros(m._n_params, dtype=np.int64)
    base = m._flat.data_ptr()
    for (name, p), (off, n) in zip(named, seg.tolist()):
        assert n == p.numel() and p.data_ptr() == base + 4 * off, name
        covered[off:off + n] += 1
    assert (covered == 1).all()                              # the parameters tile the flat buffer
    ch = mon.chunk_list(seg)
    assert mon.CHUNK == 4096 and (ch[:, 2] <= mon.CHUNK).all() and (ch[:, 2] > 0).all()
    assert (np.diff(ch[:, 0]) >= 0).all()
    hit = np.zeros(m._n_params, dtype=np.int64)
    for t, start, length in ch.tolist():
        assert 0 <= start and start + length <= seg[t, 1], "a chunk crosses its segment"
        hit[seg[t, 0] + start:seg[t, 0] + start + length] += 1
    assert (hit == 1).all()
    assert ch.shape[0] == sum(-(-n // mon.CHUNK) for n in seg[:, 1].tolist())
    assert seg[:, 1].max() > mon.CHUNK                       # (the largest tensor really is spread over several chunks)


def test_as_dict_edges_and_keys(pkg):
    """as_dict on a stand-in whose host copy is fixed: the edges are linspace(lo, hi, 65), the keys carry the prefix."""
    mon = _mon()
    h = mon.TensorHistograms.__new__(mon.TensorHistograms)
    h.names, h.what = ["a.weight", "b.bias"], "gradients"
    stats = np.zeros((2, 8))
    stats[0, :7] = [10, 1, 2, 5.0, 9.0, 0.5, 0.9486832980505138]
    host = {"counts": np.arange(128, dtype=np.int32).reshape(2, 64), "lo": np.array([-1.5, 0.0], dtype=np.float32),
            "hi": np.array([2.25, 0.0], dtype=np.float32), "stats": stats}
    h.to_host = lambda: host
    d = h.as_dict()
    assert sorted(d) == ["gradients/a.weight", "gradients/b.bias", "gradients/stats"]
    counts, edges = d["gradients/a.weight"]
    assert counts == list(range(64)) and all(isinstance(c, int) for c in counts)
    assert edges.shape == (65,) and np.array_equal(edges, np.linspace(-1.5, 2.25, 65)) and edges[0] == -1.5 and edges[-1] == 2.25
    assert np.array_equal(d["gradients/b.bias"][1], np.zeros(65)) and d["gradients/b.bias"][0] == list(range(64, 128))
    s = d["gradients/stats"]["a.weight"]
    assert (s["lo"], s["hi"], s["n_finite"], s["n_nonfinite"], s["n_zero"], s["sum"], s["sumsq"], s["mean"]) == (-1.5, 2.25, 10, 1, 2, 5, 9, 0.5)
    assert sorted(h.as_dict(prefix="g/")) == ["g/a.weight", "g/b.bias", "g/stats"]


def test_surface_is_exported_and_refuses_without_a_gpu_model(pkg):
    mon, main = _mon(), importlib.import_module("moving-mnist-vae_amd.main")
    for name in ("TensorHistograms", "tensor_histograms", "make_histogram_callback"):
        assert getattr(pkg, name) is getattr(mon, name) and getattr(main, name) is getattr(mon, name), name
    assert list(inspect.signature(pkg.TensorHistograms).parameters) == ["model", "what", "optimizer"]
    assert list(inspect.signature(pkg.tensor_histograms).parameters) == ["model", "what", "optimizer"]
    sig = inspect.signature(pkg.make_histogram_callback).parameters
    assert list(sig) == ["every", "what", "sink", "directory"] and sig["every"].default == 100 and sig["what"].default == ("gradients",)
    m = _models()["vae"]
    with pytest.raises(ValueError, match="what="):
        pkg.TensorHistograms(m, "activations")
    with pytest.raises(ValueError, match="optimizer"):
        pkg.TensorHistograms(m, "exp_avg")
    with pytest.raises(pkg.MmvaeError, match="GPU"):
        pkg.TensorHistograms(m)                              # a host model: no CPU fallback
    with pytest.raises(ValueError):
        pkg.make_histogram_callback(what=("gradients", "nope"), sink=print)
    with pytest.raises(ValueError):
        pkg.make_histogram_callback(every=0, sink=print)
    with pytest.raises(ValueError, match="sink"):
        pkg.make_histogram_callback()
    cb = pkg.make_histogram_callback(every=7, what="parameters", sink=print)
    assert cb.what == ("parameters",) and cb(model=m, optimizer=None, epoch=0, index=3) is None        # not a 7th step: nothing is touched
    src = inspect.getsource(mon)
    assert "import wandb" not in src and "import matplotlib" not in src


def test_train_reads_the_stats_callback_once(pkg):
    src = inspect.getsource(pkg.train)
    assert src.count('getattr(args, "stats_callback", None)') == 1
    assert src.index("loss.backward()") < src.index("stats_callback(model=model, optimizer=optimizer, epoch=epoch, index=index)") \
        < src.index("optimizer.step()")
