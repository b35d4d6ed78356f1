"""Developer tool (GPU box): time of the fused resize + quantise launch behind MovingMNISTClips(image_size=S) against its two yardsticks.

Input: 5120 planes of 64 x 64 uint8 (one step's 256 clips x 20 frames), Moving-MNIST-like (mostly black, bright strokes), resized
64 -> 32 and quantised with q = 2, labels and image written.
  fused        : mmvae_resize_quantise_normalise on the 5120 contiguous planes
  quantise     : mmvae_quantise_normalise (quantise_frames) on the same planes at the native size: the same bytes read, four times
                 the outputs written
  fused_gather : the loader's launch -- 256 clips picked by clip_index out of --clips resident clips (several times the Infinity
                 Cache at the default), against index_select + quantise_frames (the native loader's step)
fused and quantise are the library calls on preallocated outputs; the two gather rows are the Python calls the loader makes.
Each call: 3 warm-up launches, then 20 timed ones, one HIP-event pair per launch; the candidates alternate launch by launch.
GB/s = algorithmic bytes (planes read once, outputs written once) / median time.
  pil_host     : the reference's host path for the same planes -- Image.fromarray(a).resize((32, 32), BILINEAR) per plane plus a numpy
                 label lookup -- on this machine's CPU, one thread, if PIL imports (--host-only runs nothing else and needs no GPU;
                 --host-planes N shrinks it, the time is scaled to 5120).
Prints one JSON line."""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--clips", type=int, default=4000)
ap.add_argument("--host-only", action="store_true")
ap.add_argument("--host-planes", type=int, default=5120)
a = ap.parse_args()
PLANES, S, WARM, TIMED = 5120, 32, 3, 20
CENTRES = [0.004, 0.82]
res = {"planes": PLANES, "in": 64, "out": S, "q": 2}


def strokes_np(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 256, size=(n, 64, 64), dtype=np.uint8)
    x[rng.random(x.shape) < 0.5] = 255
    yy = np.arange(64)[None, :, None]
    top = rng.integers(0, 36, size=(n, 1, 1))
    xx = np.arange(64)[None, None, :]
    left = rng.integers(0, 36, size=(n, 1, 1))
    x[~((yy >= top) & (yy < top + 28) & (xx >= left) & (xx < left + 28) & (rng.random(x.shape) < 0.4))] = 0
    return x


try:
    import PIL
    from PIL import Image
    n = min(a.host_planes, PLANES)
    planes = strokes_np(n, 1)
    lut = (np.abs(np.arange(256, dtype=np.float32)[:, None] / np.float32(255) - np.asarray(CENTRES, dtype=np.float32)[None, :])).argmin(axis=1)
    out = np.empty((n, S, S), dtype=np.int64)
    t0 = time.perf_counter()
    for i in range(n):
        out[i] = lut[np.asarray(Image.fromarray(planes[i], "L").resize((S, S), Image.BILINEAR))]
    dt = time.perf_counter() - t0
    res["pil_host"] = {"pil": PIL.__version__, "planes_timed": n, "ms_for_5120_planes": dt * 1e3 * PLANES / n, "threads": 1}
except ImportError as e:
    res["pil_host"] = {"skipped": str(e)}
if a.host_only:
    print(json.dumps(res), flush=True)
    sys.exit(0)

import torch

pkg = importlib.import_module("moving-mnist-vae_amd")
M = importlib.import_module("moving-mnist-vae_amd.data")
assert torch.cuda.is_available(), "resize_bench needs a GPU"
dev = torch.device("cuda:0")
planes = torch.from_numpy(strokes_np(PLANES, 1)).to(dev)
resident = planes.view(256, 20, 64, 64).repeat((a.clips + 255) // 256, 1, 1, 1)[:a.clips].contiguous()
resident += torch.arange(a.clips, device=dev, dtype=torch.uint8).view(-1, 1, 1, 1) * (resident > 0)      # (clips differ)
gen = torch.Generator().manual_seed(0)
picks = [torch.randperm(a.clips, generator=gen)[:256].to(dev) for _ in range(WARM + TIMED)]
c = torch.tensor(CENTRES, dtype=torch.float32, device=dev)
step = {"i": 0}


L = importlib.import_module("moving-mnist-vae_amd._lib")
st = torch.cuda.current_stream().cuda_stream
hb, hc, hk = M._resample_tables(64, S, dev)
lab32, img32 = torch.empty((PLANES, S, S), dtype=torch.int64, device=dev), torch.empty((PLANES, S, S), dtype=torch.float32, device=dev)
lab64, img64 = torch.empty((PLANES, 64, 64), dtype=torch.int64, device=dev), torch.empty((PLANES, 64, 64), dtype=torch.float32, device=dev)


def fused():                                                            # the library call itself, on the caller's outputs
    L.check(L.lib().mmvae_resize_quantise_normalise(L.ptr(planes), 4096, None, 1, PLANES, 64, 64, S, S, L.ptr(hb), L.ptr(hc), hk, L.ptr(hb),
                                                    L.ptr(hc), hk, L.ptr(c), 2, 0.08, 0.27, L.ptr(lab32), L.ptr(img32), None, st), "fused")


def quantise():
    L.check(L.lib().mmvae_quantise_normalise(L.ptr(planes), planes.numel(), L.ptr(c), 2, 0.08, 0.27, L.ptr(lab64), L.ptr(img64), st), "quantise")


def fused_gather():
    return M._resize_launch(resident, (S, S), c, 0.0, 1.0, picks[step["i"]], (True, False, False))[0]


def select_quantise():
    return pkg.quantise_frames(resident.index_select(0, picks[step["i"]]), c, 0.0, 1.0)[0]


calls = {"fused": fused, "quantise": quantise, "fused_gather": fused_gather, "index_select_quantise": select_quantise}
ms = {k: [] for k in calls}
for r in range(WARM + TIMED):
    step["i"] = r
    for k, fn in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        del out
        if r >= WARM:
            ms[k].append(e0.elapsed_time(e1))
# what was timed is what the tests check: the fused labels are the labels of the resized bytes
fused()
lab, img = lab32, img32
want = pkg.quantise_frames(pkg.resize_frames(planes, S), c, 0.08, 0.27)
assert torch.equal(lab, want[0]) and torch.equal(img, want[1])
in_bytes, px = PLANES * 64 * 64, PLANES * S * S
algo = {"fused": in_bytes + px * 12, "quantise": in_bytes * 13, "fused_gather": in_bytes + px * 8, "index_select_quantise": in_bytes * 15}
res["note"] = "fused / quantise: the C call on preallocated outputs; the two gather rows hold the Python call (allocation, index_select)"
res["gpu"] = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "algorithmic_bytes": algo[k],
                  "GBps_median": algo[k] / statistics.median(v) / 1e6} for k, v in ms.items()}
res["resident_clips"] = a.clips
print(json.dumps(res), flush=True)
