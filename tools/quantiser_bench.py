"""Developer tool (GPU box): throughput of the byte-histogram kernel behind fit_quantiser, and the wall time of the fit.

Buffers of the training set's size (10 000 clips x 20 x 64 x 64 uint8 = 819 MB, several times the Infinity Cache) with
  skewed : Moving-MNIST-like -- rows of 64 pixels, half of them empty, the rest one stroke of 4..16 non-zero pixels (half of those
           saturated at 255): about 92 % zeros, in runs
  uniform: uniform random bytes
  zeros  : all zeros
Per buffer, mmvae_u8_histogram (the library call, caller-owned counts) and torch.bincount on the same device tensor alternate over
ROUNDS timed rounds after one warm-up round; each round is a HIP-event window over enough calls to last tens of milliseconds; the
counts of the two are compared exactly.  GB/s = bytes of the buffer / time per call (every byte is read once).
Then fit_quantiser end to end (histogram launch + 2 KB copy + exact 1-D k-means + label statistics), host clock, the call ends in
a device -> host copy; and, where scikit-learn imports, the reference's own recipe (utils.py:284-287): KMeans on the pixels of 3000
random clips on the CPU (--no-sklearn skips it, --sklearn-clips N shrinks it).
Prints one JSON line."""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--clips", type=int, default=10000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--no-sklearn", action="store_true")
ap.add_argument("--sklearn-clips", type=int, default=3000)
a = ap.parse_args()
pkg = importlib.import_module("moving-mnist-vae_amd")
L = importlib.import_module("moving-mnist-vae_amd._lib"); lib = L.lib()
assert torch.cuda.is_available(), "quantiser_bench needs a GPU"
dev = torch.device("cuda:0")
N, CLIP = a.clips, 20 * 64 * 64
gen = torch.Generator(device=dev).manual_seed(0)


def skewed(n_clips):
    out = torch.zeros((n_clips, 20, 64, 64), dtype=torch.uint8, device=dev)
    x = torch.arange(64, device=dev)[None, :]
    for lo in range(0, n_clips, 500):                                   # in pieces: the temporaries stay small
        rows = out[lo:lo + 500].view(-1, 64)
        r = rows.shape[0]
        length = torch.randint(4, 17, (r, 1), device=dev, generator=gen)
        start = (torch.rand((r, 1), device=dev, generator=gen) * (64 - length)).long()
        mask = (torch.rand((r, 1), device=dev, generator=gen) < 0.5) & (x >= start) & (x < start + length)
        value = torch.randint(1, 256, (r, 64), device=dev, generator=gen, dtype=torch.uint8)
        value[torch.rand((r, 64), device=dev, generator=gen) < 0.5] = 255
        rows.copy_(torch.where(mask, value, torch.zeros_like(value)))
    return out


buffers = {"skewed": skewed(N), "uniform": torch.randint(0, 256, (N, 20, 64, 64), device=dev, generator=gen, dtype=torch.uint8),
           "zeros": torch.zeros((N, 20, 64, 64), dtype=torch.uint8, device=dev)}
st = torch.cuda.current_stream().cuda_stream
counts = torch.zeros(256, dtype=torch.int64, device=dev)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps                                   # ms per call


res = {"clips": N, "bytes": N * CLIP, "rounds": a.rounds, "buffers": {}}
for name, buf in buffers.items():
    flat = buf.view(-1)
    nbytes = flat.numel()
    try:
        torch.bincount(flat[:1024], minlength=256)
        binc_in, binc_note = flat, "uint8"
    except RuntimeError:                                                # a torch build whose bincount takes no uint8
        binc_in, binc_note = flat.to(torch.int64), "int64 (converted outside the timed window)"
    calls = {"u8_histogram": lambda: L.check(lib.mmvae_u8_histogram(L.ptr(buf), CLIP, None, N, L.ptr(counts), st), "u8_histogram"),
             "torch_bincount": lambda: torch.bincount(binc_in, minlength=256)}
    counts.zero_(); calls["u8_histogram"](); ours = counts.clone()
    assert torch.equal(ours, calls["torch_bincount"]()), name
    reps = {k: max(3, min(200, int(50.0 / max(window(fn, 2), 1e-3)))) for k, fn in calls.items()}     # about 50 ms per window
    ms = {k: [] for k in calls}
    for r in range(a.rounds + 1):                                       # round 0 warms up and is dropped
        for k, fn in calls.items():
            t = window(fn, reps[k])
            if r:
                ms[k].append(t)
    res["buffers"][name] = {"zeros_fraction": float((flat == 0).float().mean()), "calls_per_window": reps, "bincount_input": binc_note,
                            "ms_median": {k: statistics.median(v) for k, v in ms.items()}, "ms_min": {k: min(v) for k, v in ms.items()},
                            "GBps_median": {k: nbytes / statistics.median(v) / 1e6 for k, v in ms.items()}}
    del binc_in

# the fit end to end, on the skewed buffer
fit_ms = {}
for label, kw in (("q2_all_clips", dict(n_clusters=2)), ("q4_all_clips", dict(n_clusters=4)), ("q256_all_clips", dict(n_clusters=256)),
                  ("q2_3000_clips", dict(n_clusters=2, clips=min(3000, N)))):
    ts = []
    for r in range(6):                                                  # the first call is dropped
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fit = pkg.fit_quantiser(buffers["uniform" if kw["n_clusters"] == 256 else "skewed"], **kw)
        ts.append((time.perf_counter() - t0) * 1e3)
    fit_ms[label] = {"ms_median": statistics.median(ts[1:]), "ms_min": min(ts[1:]), "inertia": fit.inertia}
res["fit_quantiser"] = fit_ms
fit2 = pkg.fit_quantiser(buffers["skewed"], 2)
res["fit_q2"] = {"centres": fit2.centres.tolist(), "data_mean": fit2.data_mean, "data_std": fit2.data_std, "ratios": fit2.ratios.tolist()}

try:
    if a.no_sklearn:
        raise ImportError("skipped (--no-sklearn)")
    from sklearn.cluster import KMeans
    k = min(a.sklearn_clips, N)
    idx = np.random.default_rng(0).choice(N, k, replace=False)
    sub = buffers["skewed"][torch.from_numpy(idx).to(dev)].cpu().numpy()
    t0 = time.perf_counter()
    X = sub.reshape(-1, 1) / 255                                        # utils.py:285
    km = KMeans(n_clusters=2).fit(X)                                    # utils.py:287 (n_jobs is gone from scikit-learn)
    t1 = time.perf_counter()
    res["sklearn"] = {"clips": k, "points": int(X.shape[0]), "seconds": t1 - t0, "iterations": int(km.n_iter_), "inertia": float(km.inertia_),
                      "centres_sorted": sorted(km.cluster_centers_.ravel().tolist()),
                      "our_inertia_same_clips": pkg.fit_quantiser(buffers["skewed"][torch.from_numpy(idx).to(dev)], 2).inertia}
except ImportError as e:
    res["sklearn"] = {"skipped": str(e)}
print(json.dumps(res), flush=True)
