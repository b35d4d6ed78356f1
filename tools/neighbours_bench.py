"""Developer tool (GPU box): time of the nearest-frames search over a Moving-MNIST-sized resident set (F = 200 000 frames of D = 4096
bytes, 819 MB -- the size tools/quantiser_bench.py uses) against the ATen chain a user would write by hand.
  c_plain / c_lut : mmvae_nearest_frames itself on preallocated buffers (k = 5), for M = 6 and M = 64 queries, without and with a
                    256-byte lut (a random permutation, so the lookup cannot be folded away; the queries are in the table's space)
  nearest_frames  : the Python call (argument checks, the scratch and output allocations) at M = 6 without a lut
  aten            : chunks of 16 384 frames -- ``frames[c].float()``, ``|q|^2 + |f|^2 - 2 q f^T`` in f32, ``topk`` per chunk, a final ``topk``
                    over the chunks' winners -- with its peak extra memory (torch.cuda.max_memory_allocated above the resident data)
The data are random bytes with copies of the first three queries planted at known frames.  Before timing every candidate is checked
against the others: the library calls and the Python call give equal bits; the ATen chain is f32 (its sums pass 2^24, so it is not
exact) and must find the planted frames first and agree on every distance within 2e-5 of 2 D 255^2.  The candidates alternate; each timed
sample is a window of back-to-back calls between two HIP events, 3 warm-up windows, then 15 timed ones; medians are reported, and
``F * D / time`` in TB/s for the library calls.  Prints one JSON line."""
import importlib, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

pkg = importlib.import_module("moving-mnist-vae_amd")
L = importlib.import_module("moving-mnist-vae_amd._lib")
assert torch.cuda.is_available(), "neighbours_bench needs a GPU"
dev = torch.device("cuda:0")
F, D, K, CHUNK, WARM, TIMED = 200000, 4096, 5, 16384, 3, 15
st = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(0)
frames = torch.randint(0, 256, (F, 64, 64), dtype=torch.uint8, device=dev, generator=g)
flat = frames.view(F, D)
lut = torch.randperm(256, device=dev, generator=g).to(torch.uint8)
PLANTED = (0, F // 3, F - 1)


def queries_for(M, table):
    q = torch.randint(0, 256, (M, D), dtype=torch.uint8, device=dev, generator=g)
    for m, f in enumerate(PLANTED):
        q[m] = flat[f] if table is None else table[flat[f].long()]
    return q


class CCall:
    """mmvae_nearest_frames on buffers allocated once."""

    def __init__(self, q, table):
        self.q, self.table, self.M = q, table, q.shape[0]
        self.nbytes = L.lib().mmvae_nearest_frames_scratch_bytes(self.M, F, D, K)
        self.scratch = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.dist = torch.empty((self.M, K), dtype=torch.int32, device=dev)
        self.index = torch.empty((self.M, K), dtype=torch.int64, device=dev)

    def __call__(self):
        L.check(L.lib().mmvae_nearest_frames(L.ptr(self.q), self.M, L.ptr(flat), F, D, L.ptr(self.table), K, L.ptr(self.dist), L.ptr(self.index),
                                             L.ptr(self.scratch), self.nbytes, st), "mmvae_nearest_frames")
        return self.dist, self.index


def aten(q, table):
    qf = q.float()
    qn = (qf * qf).sum(1)
    ds, ix = [], []
    for lo in range(0, F, CHUNK):
        c = flat[lo:lo + CHUNK]
        fc = (c if table is None else table[c.long()]).float()
        d = qn[:, None] + (fc * fc).sum(1)[None, :] - 2.0 * (qf @ fc.T)
        v, i = torch.topk(d, K, dim=1, largest=False)
        ds.append(v)
        ix.append(i + lo)
    ds, ix = torch.cat(ds, 1), torch.cat(ix, 1)
    v, j = torch.topk(ds, K, dim=1, largest=False)
    return v, torch.gather(ix, 1, j)


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


res = {"F": F, "D": D, "k": K, "bytes": F * D, "windows": TIMED, "us_per_call": {}, "TB_per_s": {}, "aten_peak_extra_MB": {}}
calls, per = {}, {}
for M in (6, 64):
    for name, table in (("plain", None), ("lut", lut)):
        q = queries_for(M, table)
        c = CCall(q, table)
        dist, index = (t.clone() for t in c())
        pd, pi = pkg.nearest_frames(q, frames, k=K, lut=table)
        assert torch.equal(dist, pd) and torch.equal(index, pi), (M, name)
        assert index[:3, 0].tolist() == list(PLANTED) and dist[:3, 0].tolist() == [0, 0, 0], (M, name)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ad, ai = aten(q, table)
        torch.cuda.synchronize()
        res["aten_peak_extra_MB"][f"M={M} {name}"] = (torch.cuda.max_memory_allocated() - base) / 1e6
        assert ai[:3, 0].tolist() == list(PLANTED), (M, name)
        assert ((ad - dist.float()).abs() <= 2e-5 * 2 * D * 255 ** 2).all(), (M, name)        # f32 sums of magnitude up to 2 D 255^2
        calls[f"c_{name} M={M}"], per[f"c_{name} M={M}"] = c, 5
        if name == "plain":
            calls[f"aten M={M}"], per[f"aten M={M}"] = (lambda q=q: aten(q, None)), 1
        elif M == 6:
            calls["aten_lut M=6"], per["aten_lut M=6"] = (lambda q=q: aten(q, lut)), 1
        if M == 6 and name == "plain":
            calls["nearest_frames M=6"], per["nearest_frames M=6"] = (lambda q=q: pkg.nearest_frames(q, frames, k=K)), 5
res["us_per_call"] = time_all(calls, per)
for k, v in res["us_per_call"].items():
    if k.startswith(("c_", "nearest_frames")):
        res["TB_per_s"][k] = F * D / (v["median"] * 1e-6) / 1e12
print(json.dumps(res), flush=True)
