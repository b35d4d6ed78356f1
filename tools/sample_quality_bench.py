"""Developer tool (GPU box): time of the set-to-set sweep (mmvae_knn_cross) and of ``sample_quality`` at the size of the Moving MNIST test
split, 20 000 frames of D = 4096 bytes a side, k = 3, against what a user could write before.
  knn_cross        : mmvae_knn_cross itself on preallocated buffers (k = 3, no counts)
  loop             : the same result from mmvae_nearest_frames, 64 rows of ``a`` a call (313 calls, each re-reading ``b``), preallocated
  aten             : chunks of 2048 rows -- ``|a|^2 + |b|^2 - 2 a b^T`` in f32, ``topk`` -- with its peak extra memory; f32, so not exact
  sample_quality   : the Python call, four sweeps and the scores
  loop_knn_parts   : the k-NN parts of those four sweeps from the loop (R x R and F x F with k + 1 neighbours, both directions of R x F
                     with 1); the ball counts have no expression through mmvae_nearest_frames, so this is a lower bound of a loop version
  aten_quality     : the scores from chunked f32 distance rows (topk, comparisons against the radii); not exact
The data are random bytes with a few rows of ``a`` planted in ``b``.  Before timing, the new call and the loop are checked to give equal
bits, and the ATen chain to find the planted rows and agree on every distance within 2e-5 of 2 D 255^2.  The candidates alternate; each
timed sample is a window of back-to-back calls between two HIP events, 3 warm-up windows, then 15 timed ones; medians are reported, with
``2 Na Nb D / time`` in POP/s for the new call.  The new call must beat the loop by more than the spread: its slowest window against the
loop's fastest (asserted).  ``--only-new N`` runs the new call N times and nothing else (for a counter run).  Prints one JSON line."""
import importlib, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

pkg = importlib.import_module("moving-mnist-vae_amd")
L = importlib.import_module("moving-mnist-vae_amd._lib")
assert torch.cuda.is_available(), "sample_quality_bench needs a GPU"
dev = torch.device("cuda:0")
N, D, K, ROWS, CHUNK, WARM, TIMED = 20000, 4096, 3, 64, 2048, 3, 15
st = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(0)
a = torch.randint(0, 256, (N, D), dtype=torch.uint8, device=dev, generator=g)
b = torch.randint(0, 256, (N, D), dtype=torch.uint8, device=dev, generator=g)
PLANTED = {0: 17, 5000: 19999, 19999: 3}
for i, j in PLANTED.items():
    b[j] = a[i]


class Cross:
    """mmvae_knn_cross on buffers allocated once."""

    def __init__(self, x, y, k):
        self.x, self.y, self.k = x, y, k
        self.nbytes = L.lib().mmvae_knn_cross_scratch_bytes(x.shape[0], y.shape[0], D, k, 0)
        self.scratch = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.dist = torch.empty((x.shape[0], k), dtype=torch.int32, device=dev)
        self.index = torch.empty((x.shape[0], k), dtype=torch.int64, device=dev)

    def __call__(self):
        L.check(L.lib().mmvae_knn_cross(L.ptr(self.x), self.x.shape[0], L.ptr(self.y), self.y.shape[0], D, self.k, 0, L.ptr(self.dist),
                                        L.ptr(self.index), None, None, L.ptr(self.scratch), self.nbytes, st), "mmvae_knn_cross")
        return self.dist, self.index


class Loop:
    """The same (dist, index) from mmvae_nearest_frames, ROWS rows a call."""

    def __init__(self, x, y, k):
        self.x, self.y, self.k = x, y, k
        self.nbytes = L.lib().mmvae_nearest_frames_scratch_bytes(ROWS, y.shape[0], D, k)
        self.scratch = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.dist = torch.empty((x.shape[0], k), dtype=torch.int32, device=dev)
        self.index = torch.empty((x.shape[0], k), dtype=torch.int64, device=dev)

    def __call__(self):
        fn, n = L.lib().mmvae_nearest_frames, self.x.shape[0]
        for lo in range(0, n, ROWS):
            m = min(ROWS, n - lo)
            L.check(fn(self.x.data_ptr() + lo * D, m, L.ptr(self.y), self.y.shape[0], D, None, self.k, self.dist.data_ptr() + lo * self.k * 4,
                       self.index.data_ptr() + lo * self.k * 8, L.ptr(self.scratch), self.nbytes, st), "mmvae_nearest_frames")
        return self.dist, self.index


def aten_rows(x, y, yn, lo):
    xf = x[lo:lo + CHUNK].float()
    return (xf * xf).sum(1)[:, None] + yn[None, :] - 2.0 * (xf @ y.T)


def aten(x, y, k):
    yf = y.float()
    yn = (yf * yf).sum(1)
    out = [torch.topk(aten_rows(x, yf, yn, lo), k, dim=1, largest=False) for lo in range(0, x.shape[0], CHUNK)]
    return torch.cat([v for v, _ in out]), torch.cat([i for _, i in out])


def aten_quality(real, fake, k):
    rf, ff = real.float(), fake.float()
    rn, fn = (rf * rf).sum(1), (ff * ff).sum(1)
    inf = float("inf")

    def sweep(x, y, yn, k, radius, own):
        best, count = [], []
        for lo in range(0, x.shape[0], CHUNK):
            d = aten_rows(x, y, yn, lo)
            if own:
                d[torch.arange(d.shape[0], device=dev), torch.arange(lo, lo + d.shape[0], device=dev)] = inf
            best.append(torch.topk(d, k, dim=1, largest=False)[0])
            if radius is not None:
                count.append((d <= radius[None, :]).sum(1))
        return torch.cat(best), (torch.cat(count) if radius is not None else None)

    d_rr, d_ff = sweep(real, rf, rn, k, None, True)[0], sweep(fake, ff, fn, k, None, True)[0]
    d_fr, in_real = sweep(fake, rf, rn, 1, d_rr[:, k - 1], False)
    d_rf, in_fake = sweep(real, ff, fn, 1, d_ff[:, k - 1], False)
    nr, nf = real.shape[0], fake.shape[0]
    right = (d_rr[:, 0] <= d_rf[:, 0]).sum() + (d_ff[:, 0] < d_fr[:, 0]).sum()
    return {"precision": (in_real > 0).double().mean(), "recall": (in_fake > 0).double().mean(), "density": in_real.double().sum() / (k * nf),
            "coverage": (d_rf[:, 0] <= d_rr[:, k - 1]).double().mean(), "accuracy": right.double() / (nr + nf)}


def time_all(calls, per_window):
    us = {k: [] for k in calls}
    for r in range(WARM + TIMED):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per_window[k]):
                out = fn()
            e1.record()
            torch.cuda.synchronize()
            del out
            if r >= WARM:
                us[k].append(e0.elapsed_time(e1) * 1e3 / per_window[k])
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in us.items()}


new = Cross(a, b, K)
if len(sys.argv) > 2 and sys.argv[1] == "--only-new":
    for _ in range(int(sys.argv[2])):
        new()
    torch.cuda.synchronize()
    sys.exit(0)

loop = Loop(a, b, K)
nd, ni = (t.clone() for t in new())
ld, li = loop()
assert torch.equal(nd, ld) and torch.equal(ni, li)
for i, j in PLANTED.items():
    assert nd[i, 0] == 0 and ni[i, 0] == j
torch.cuda.synchronize()
res = {"Na": N, "Nb": N, "D": D, "k": K, "windows": TIMED, "knn_cross_scratch_MB": new.nbytes / 1e6}
base = torch.cuda.memory_allocated()
torch.cuda.reset_peak_memory_stats()
ad, ai = aten(a, b, K)
torch.cuda.synchronize()
res["aten_peak_extra_MB"] = (torch.cuda.max_memory_allocated() - base) / 1e6
assert all(int(ai[i, 0]) == j for i, j in PLANTED.items())
assert ((ad - nd.float()).abs() <= 2e-5 * 2 * D * 255 ** 2).all()
res["aten_index_mismatches"] = int((ai != ni).sum())
del ad, ai

# sample_quality: blobs instead of noise would be the workload; the time of the sweeps does not depend on the bytes
scores = pkg.sample_quality(a, b, k=K)
host = pkg.sample_quality_to_host(scores)
approx = {k: float(v) for k, v in aten_quality(a, b, K).items()}
res["scores"], res["aten_scores"] = host, approx
parts = [Loop(a, a, K + 1), Loop(b, b, K + 1), Loop(b, a, 1), Loop(a, b, 1)]
calls = {"knn_cross": new, "loop": loop, "aten": lambda: aten(a, b, K), "sample_quality": lambda: pkg.sample_quality(a, b, k=K),
         "loop_knn_parts": lambda: [p() for p in parts], "aten_quality": lambda: aten_quality(a, b, K)}
per = {"knn_cross": 3, "loop": 1, "aten": 1, "sample_quality": 1, "loop_knn_parts": 1, "aten_quality": 1}
t = res["us_per_call"] = time_all(calls, per)
res["POP_per_s"] = 2.0 * N * N * D / (t["knn_cross"]["median"] * 1e-6) / 1e15
res["loop_over_new"] = t["loop"]["median"] / t["knn_cross"]["median"]
res["aten_over_new"] = t["aten"]["median"] / t["knn_cross"]["median"]
res["loop_parts_over_sample_quality"] = t["loop_knn_parts"]["median"] / t["sample_quality"]["median"]
res["aten_quality_over_sample_quality"] = t["aten_quality"]["median"] / t["sample_quality"]["median"]
print(json.dumps(res), flush=True)
assert t["knn_cross"]["max"] < t["loop"]["min"], "the new call does not beat the loop by more than the spread of the windows"
