"""GPU: mmvae_tensor_hist and the Python surface on top of it (TensorHistograms, tensor_histograms, make_histogram_callback, the
``stats_callback`` hook of train()).

Counts, lo, hi, n_finite, n_nonfinite and n_zero must EQUAL the numpy f32 restatement of tests/test_tensor_hist_cpu.py (hist_ref: min / max
of the finite subset as np.float32, widened when equal, then min(int(((f - lo) * 64) / (hi - lo)), 63), each step one correctly rounded
f32 operation).  The f64 sum and sum of squares must lie within n 2^-52 sum|x| (resp. n 2^-52 sum x^2) of numpy's f64 sums: every term
is exact in f64 (an f32, or the product of two), and a sum of n terms in ANY order is off by at most (n - 1) 2^-53 sum|terms| (1 + o(1))
on either side -- the bound is derived, not measured.  mean and rms are one f64 division (and one square root) of the device's own sums:
4 2^-52 relative.  Magnitudes stay below 1e30, so the restatement never overflows."""
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_tensor_hist_cpu import hist_ref  # noqa: E402

gpu = pytest.mark.gpu
BINS, STATS, CHUNK = 64, 8, 4096
EPS = 2.0 ** -52
NAN, INF = float("nan"), float("inf")


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _M():
    return importlib.import_module("moving-mnist-vae_amd.model")


def _mon():
    return importlib.import_module("moving-mnist-vae_amd.monitor")


def _run(flat, seg, chunk=CHUNK, chunks=None, out=None):
    """One mmvae_tensor_hist call through the C ABI on a device copy of ``flat`` (numpy f32), every output buffer pre-filled with
    garbage.  Returns dict(counts, lo, hi, stats) as numpy arrays, and the device buffers."""
    L = _L()
    dev = torch.device("cuda")
    seg = np.ascontiguousarray(np.array(seg, dtype=np.int64).reshape(-1, 2))
    ch = np.ascontiguousarray(_mon().chunk_list(seg, chunk) if chunks is None else np.array(chunks, dtype=np.int64).reshape(-1, 3))
    T, n = seg.shape[0], ch.shape[0]
    d_flat = flat if torch.is_tensor(flat) else torch.from_numpy(np.asarray(flat, dtype=np.float32)).to(dev)
    d_seg, d_ch = torch.from_numpy(seg).to(dev), (torch.from_numpy(ch).to(dev) if n else None)
    if out is None:
        out = {"counts": torch.full((T, BINS), 0x5a5a5a5a, dtype=torch.int32, device=dev),
               "lo": torch.full((T,), 7.5e29, dtype=torch.float32, device=dev), "hi": torch.full((T,), NAN, dtype=torch.float32, device=dev),
               "stats": torch.full((T, STATS), NAN, dtype=torch.float64, device=dev)}
    nbytes = L.lib().mmvae_tensor_hist_scratch_bytes(T, n)
    scratch = torch.full((nbytes // 8,), NAN, dtype=torch.float64, device=dev)
    L.call("mmvae_tensor_hist", dev, L.ptr(d_flat), d_flat.numel(), seg.ctypes.data, L.ptr(d_seg), T, ch.ctypes.data if n else None, L.ptr(d_ch),
           n, L.ptr(out["counts"]), L.ptr(out["lo"]), L.ptr(out["hi"]), L.ptr(out["stats"]), L.ptr(scratch), nbytes)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, out


def _check_segment(x, res, t, tag=""):
    """Row t of a result against hist_ref of the numpy f32 array x."""
    r = hist_ref(x)
    tag = "%s segment %d (n=%d)" % (tag, t, np.asarray(x).size)
    st = res["stats"][t]
    assert (st[0], st[1], st[2]) == (r["n_finite"], r["n_nonfinite"], r["n_zero"]), tag
    assert res["lo"][t] == r["lo"] and res["hi"][t] == r["hi"], (tag, res["lo"][t], r["lo"], res["hi"][t], r["hi"])
    assert np.array_equal(res["counts"][t].astype(np.int64), r["counts"]), (tag, np.nonzero(res["counts"][t] != r["counts"])[0])
    assert int(res["counts"][t].sum()) == r["n_finite"], tag
    n = r["n_finite"]
    assert abs(st[3] - r["sum"]) <= n * EPS * r["abs_sum"], (tag, st[3], r["sum"])
    assert abs(st[4] - r["sumsq"]) <= n * EPS * r["sumsq"], (tag, st[4], r["sumsq"])
    if n:
        assert abs(st[5] - st[3] / n) <= 4 * EPS * abs(st[3] / n) and abs(st[6] - np.sqrt(st[4] / n)) <= 4 * EPS * np.sqrt(st[4] / n), tag
    else:
        assert st[5] == 0 and st[6] == 0, tag
    assert st[7] == 0, tag


def _pack(parts, rng):
    """Lay the arrays of ``parts`` into one flat buffer at odd offsets (no segment starts 16-byte aligned), the gaps filled with NaN and
    1e30 sentinels that must not show in any result.  Returns (flat f32, segments)."""
    pieces, seg, at = [], [], 0
    for p in parts:
        gap = 1 + 2 * int(rng.integers(0, 4))
        if (at + gap) % 2 == 0:                                            # the next offset must be odd
            gap += 1
        fill = np.where(np.arange(gap) % 2 == 0, np.float32(NAN), np.float32(1e30)).astype(np.float32)
        pieces.append(fill)
        at += gap
        assert at % 2 == 1
        seg.append([at, len(p)])
        pieces.append(np.asarray(p, dtype=np.float32))
        at += len(p)
    pieces.append(np.array([NAN, 1e30, NAN], dtype=np.float32))
    return np.concatenate(pieces), seg


@gpu
@pytest.mark.parametrize("chunk", [4096, 100])
def test_every_length_around_the_chunk_at_odd_offsets(pkg, chunk):
    rng = np.random.default_rng(chunk)
    lengths = [0, 1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 17]
    parts = [(rng.standard_normal(n) * 0.01).astype(np.float32) for n in lengths]
    flat, seg = _pack(parts, rng)
    res, _ = _run(flat, seg, chunk)
    for t, p in enumerate(parts):
        _check_segment(p, res, t, "chunk=%d" % chunk)
    # no sentinel (NaN, 1e30) reached a result: the data is below 0.1, a one-element range is widened by 1
    assert np.isfinite(res["stats"]).all() and np.abs(res["hi"]).max() < 1.1 and np.abs(res["lo"]).max() < 1.1


@gpu
def test_one_segment_and_hundreds_of_tiny_ones(pkg):
    rng = np.random.default_rng(1)
    x = rng.standard_normal(10001).astype(np.float32)
    res, _ = _run(np.concatenate([[NAN], x, [1e30]]).astype(np.float32), [[1, 10001]])
    _check_segment(x, res, 0, "T=1")
    parts = [rng.standard_normal(1 + (i % 2)).astype(np.float32) for i in range(230)]
    parts[7], parts[8] = np.array([0.25, 0.25], dtype=np.float32), np.array([NAN], dtype=np.float32)
    flat, seg = _pack(parts, rng)
    res, _ = _run(flat, seg)
    for t, p in enumerate(parts):
        _check_segment(p, res, t, "T=230")


@gpu
def test_special_values(pkg):
    rng = np.random.default_rng(2)
    normal = rng.standard_normal(5000).astype(np.float32)
    top = rng.uniform(-3, 2, 4000).astype(np.float32)
    top[::5] = 2.0                                                       # the maximum 800 times: all in bin 63
    edges = rng.integers(0, 65, 6000).astype(np.float32)
    edges[:2] = [0.0, 64.0]
    mixed = rng.standard_normal(3000).astype(np.float32)
    mixed[::7], mixed[1::11], mixed[2::13], mixed[3::17] = -0.0, NAN, INF, -INF
    mixed[5::19], mixed[6::23] = 1e-41, -3e-45                           # denormals
    denorm = (rng.integers(-8000, 8000, 2000) * np.float32(1.4e-45)).astype(np.float32)      # nothing but denormals and zeros
    parts = {"constant": np.full(777, 0.5, dtype=np.float32), "constant_zero": np.zeros(130, dtype=np.float32),
             "constant_negzero": np.full(9, -0.0, dtype=np.float32), "one_value": np.array([-3.25], dtype=np.float32),
             "max_many_times": top, "bin_edges": edges, "mixed": mixed, "denormals": denorm,
             "all_nonfinite": np.array([NAN, INF, -INF] * 50, dtype=np.float32), "scaled_1e-30": normal * np.float32(1e-30),
             "scaled_1e20": normal * np.float32(1e20), "two_values": np.array([1.0, 2.0] * 33, dtype=np.float32)}
    flat, seg = _pack(list(parts.values()), rng)
    res, _ = _run(flat, seg, 1001)                                        # an odd chunk: chunk starts at every alignment (heads of 0..3)
    for t, (name, p) in enumerate(parts.items()):
        _check_segment(p, res, t, name)
    names = list(parts)
    t = names.index("constant")
    assert (res["lo"][t], res["hi"][t]) == (-0.5, 1.5) and res["counts"][t][32] == 777
    t = names.index("max_many_times")
    assert res["hi"][t] == 2.0 and res["counts"][t][63] >= 800
    t = names.index("bin_edges")
    assert (res["lo"][t], res["hi"][t]) == (0.0, 64.0)
    assert res["counts"][t][63] == int(((edges == 63) | (edges == 64)).sum()) and res["counts"][t][10] == int((edges == 10).sum())
    t = names.index("all_nonfinite")
    assert (res["lo"][t], res["hi"][t]) == (0.0, 0.0) and res["counts"][t].sum() == 0 and res["stats"][t][1] == 150
    t = names.index("mixed")
    assert res["stats"][t][1] == int((~np.isfinite(mixed)).sum()) and res["stats"][t][2] == int((mixed == 0).sum()) > 0
    t = names.index("denormals")
    assert 0 < res["hi"][t] < 1.2e-38 and res["counts"][t].sum() == 2000


@gpu
def test_two_calls_give_the_same_bits_and_garbage_is_overwritten(pkg):
    rng = np.random.default_rng(3)
    parts = [rng.standard_normal(n).astype(np.float32) * np.float32(s) for n, s in ((50000, 1.0), (3, 1e-3), (0, 1.0), (4097, 30.0))]
    flat, seg = _pack(parts, rng)
    a, _ = _run(flat, seg)
    b, dev_out = _run(flat, seg)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    c, _ = _run(flat, seg, out=dev_out)                                   # onto the previous results, not onto garbage
    for k in a:
        assert a[k].tobytes() == c[k].tobytes(), k
    for t, p in enumerate(parts):
        _check_segment(p, a, t)
    # a chunk list in another order, with an empty chunk: the integers cannot change (the f64 sums may, within their bound)
    ch = _mon().chunk_list(np.array(seg, dtype=np.int64), CHUNK)
    shuffled = np.concatenate([ch[::-1], [[2, 0, 0]]])
    d, _ = _run(flat, seg, chunks=shuffled)
    assert np.array_equal(d["counts"], a["counts"]) and np.array_equal(d["lo"], a["lo"]) and np.array_equal(d["hi"], a["hi"])
    assert np.array_equal(d["stats"][:, :3], a["stats"][:, :3])
    for t, p in enumerate(parts):
        _check_segment(p, d, t, "shuffled")


# ================================================================ end to end
CTORS = {"vae": (1, 32, 1, 2, 8, False, False, 4, "ReLu", 1, 1, 0, True, 0.1, 16),
         "pixelvae": (1, 16, 2, 2, 32, True, False, 3, "ReLu", 1, 1, 0, True, 0.0, 32)}


def _one_backward(oracle, kind, dt, **opt_kw):
    M = _M()
    dev = torch.device("cuda")
    torch.manual_seed(3)
    m = M.VAE(*CTORS[kind], compute_dtype=dt).to(dev).train()
    opt = M.FusedAdam(list(m.parameters()), **opt_kw)
    S = m.input_image_size
    labels = oracle.synthetic_labels(4, S, seed=9).view(4, S * S)
    categorical = kind == "pixelvae"
    args = types.SimpleNamespace(data_ratio_of_labels=torch.ones(2) if categorical else None, dataset="MovingMNIST", quiet=True)

    def backward():
        image, target = m.prepare_batch(labels, dev, oracle.DATA_MEAN, oracle.DATA_STD, categorical)
        out = m(image)
        loss = m.loss(target, *out, dev, args)[0]
        opt.zero_grad()
        loss.backward()
    return m, opt, backward


def _check_all(h, tensors, tag):
    """Every row of a TensorHistograms against hist_ref of the matching tensor."""
    torch.cuda.synchronize()
    res = h.to_host()
    assert len(h.names) == len(tensors) == res["counts"].shape[0]
    for t, x in enumerate(tensors):
        _check_segment(x.detach().float().cpu().numpy().reshape(-1), res, t, "%s %s" % (tag, h.names[t]))
    for k in ("n_finite", "n_nonfinite", "n_zero", "mean", "rms"):
        assert torch.equal(getattr(h, k).cpu(), torch.from_numpy(res["stats"][:, _mon().STAT_NAMES.index(k)].copy())), k
    assert h.counts.shape == (len(tensors), BINS) and h.counts.dtype == torch.int32 and h.counts.is_cuda and h.lo.dtype == torch.float32


@gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["vae", "pixelvae"])
def test_model_gradients_parameters_and_moments(pkg, oracle, kind, dt):
    m, opt, backward = _one_backward(oracle, kind, dt)
    with pytest.raises(pkg.MmvaeError, match="no backward"):
        pkg.tensor_histograms(m, "gradients", opt)                       # before any backward
    backward()
    named = list(m.named_parameters())
    h = pkg.tensor_histograms(m, "gradients", opt)
    assert h.names == [n for n, _ in named]
    assert all(p.grad is not None for _, p in named)
    _check_all(h, [p.grad for _, p in named], "gradients")
    assert float(h.n_nonfinite.sum()) == 0 and float(h.rms.max()) > 0
    d = h.as_dict(prefix="gradients/")
    assert sorted(d) == sorted(["gradients/" + n for n in h.names] + ["gradients/stats"])
    host = h.to_host()
    for t, n in enumerate(h.names):
        counts, edges = d["gradients/" + n]
        assert counts == host["counts"][t].tolist() and np.array_equal(edges, np.linspace(float(host["lo"][t]), float(host["hi"][t]), 65))
        assert d["gradients/stats"][n]["n_finite"] == named[t][1].numel()
    _check_all(pkg.tensor_histograms(m, "parameters"), [p for _, p in named], "parameters")
    opt.step()
    _check_all(pkg.tensor_histograms(m, "exp_avg", opt), [opt.state[p]["exp_avg"] for _, p in named], "exp_avg")
    hv = pkg.tensor_histograms(m, "exp_avg_sq", opt)
    _check_all(hv, [opt.state[p]["exp_avg_sq"] for _, p in named], "exp_avg_sq")
    assert float(hv.mean.min()) >= 0.0 and float(hv.lo.min()) >= -1.0   # squares; -1 is the widened range of an all-zero moment
    # a NaN in one gradient element shows in that tensor's row, and only there
    backward()
    t = len(named) // 2
    named[t][1].grad.view(-1)[0] = NAN
    h.update()
    torch.cuda.synchronize()
    nn = h.n_nonfinite.cpu()
    assert nn[t] == 1 and nn.sum() == 1
    _check_all(h, [p.grad for _, p in named], "gradients with a NaN")


@gpu
def test_train_calls_the_stats_callback_and_is_not_perturbed(pkg, oracle, tmp_path):
    M = _M()
    dev = torch.device("cuda")
    batches = [oracle.synthetic_labels(4, 16, seed=s).view(4, 256) for s in (5, 6)]
    runs = []
    for with_cb in (False, True):
        torch.manual_seed(11)
        m = M.VAE(*CTORS["vae"], compute_dtype="f32").to(dev).train()
        opt = M.FusedAdam(list(m.parameters()))
        g = torch.Generator().manual_seed(4)
        m.injected_eps = torch.randn(4, 8, 1, 1, generator=g).to(dev)
        m.injected_true_samples = torch.randn(4, 8, generator=g).to(dev)
        args = types.SimpleNamespace(data_ratio_of_labels=None, dataset="MovingMNIST", quiet=True)
        got = []
        if with_cb:
            args.stats_callback = pkg.make_histogram_callback(every=1, sink=got.append, directory=str(tmp_path / "hist"))
        out = pkg.train(m, batches, opt, dev, args, epoch=3, data_mean=oracle.DATA_MEAN, data_std=oracle.DATA_STD)
        runs.append(([list(map(float, l)) for l in out], m._flat.detach().clone(), got, [n for n, _ in m.named_parameters()]))
    (plain, p_flat, _, _), (hooked, h_flat, got, names) = runs
    assert plain == hooked and all(np.isfinite(plain[0])) and len(plain[0]) == 2
    assert torch.equal(p_flat, h_flat)
    assert len(got) == 2
    for d in got:
        assert sorted(d) == sorted(["gradients/" + n for n in names] + ["gradients/stats"])
        for n in names:
            counts, edges = d["gradients/" + n]
            assert len(counts) == 64 and edges.shape == (65,) and sum(counts) == d["gradients/stats"][n]["n_finite"] > 0
    assert got[0]["gradients/" + names[0]][0] != got[1]["gradients/" + names[0]][0] or \
        got[0]["gradients/stats"][names[0]]["sum"] != got[1]["gradients/stats"][names[0]]["sum"]       # two different steps
    assert sorted(os.listdir(tmp_path / "hist")) == ["hist-3-0.npz", "hist-3-1.npz"]
    z = np.load(tmp_path / "hist" / "hist-3-1.npz")
    assert z["gradients_counts"].tolist() == [got[1]["gradients/" + n][0] for n in names] and z["gradients_names"].tolist() == names


@gpu
def test_update_replays_inside_a_captured_graph(pkg, oracle):
    m, opt, backward = _one_backward(oracle, "vae", "f32")
    backward()
    h = pkg.TensorHistograms(m, "gradients", opt)
    G = opt._flat_grads(m)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h.update()                                                       # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):                      # one stream, a linear chain of three launches
            h.update()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(8)
    G.copy_((torch.randn(G.numel(), generator=g) * 3.0).to(G.device))
    G[5] = INF
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    replayed = h._blob.clone()
    eager = pkg.TensorHistograms(m, "gradients", opt)
    eager.update()
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager._blob)
    _check_all(h, [p.grad for _, p in m.named_parameters()], "replayed")
    assert float(h.n_nonfinite.sum()) == 1
