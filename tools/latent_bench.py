"""Developer tool (GPU box): times of the latent diagnostics against the ATen chains a user would write by hand.
  scatter_c     : mmvae_scatter_panel itself (side 256, radius 4 pixels) on preallocated buffers, for n = 5120 (a batch) and n = 204800
                  (a held-out set), points read in place from an (n, 32) encoding (stride 32) and from a dense (n, 2) tensor
  scatter_panel : the Python call at stride 32 (argument checks, the limits and the xform on the device, allocation of the panel)
  scatter_aten  : the same counts in ATen -- sub-pixel positions, the pixel indices of a 10 x 10 box of disc offsets per point, the
                  coverage test, ``bincount`` over the covered indices and the tone table (the boolean gather synchronises)
  stats_c       : mmvae_latent_stats at (5120, 64) with logvar and encoding
  stats_aten    : the equivalent f64 ATen reductions (convert, exp, six sums, stack)
The candidates alternate; each timed sample is a window of back-to-back calls between two HIP events, 3 warm-up windows, then 15 timed
ones; the medians are reported.  Every candidate is first checked against the ATen result (bytes equal; sums within 1e-12).  Prints one
JSON line."""
import importlib, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

pkg = importlib.import_module("moving-mnist-vae_amd")
L = importlib.import_module("moving-mnist-vae_amd._lib")
assert torch.cuda.is_available(), "latent_bench needs a GPU"
dev = torch.device("cuda:0")
SIDE, R16, Z, WARM, TIMED = 256, 64, 32, 3, 15
st = torch.cuda.current_stream().cuda_stream
tone = pkg.scatter_tone().to(dev)
panel = torch.empty((SIDE, SIDE), dtype=torch.uint8, device=dev)
box = torch.arange(2 * R16 // 16 + 2, device=dev)


def xform_of(pts):
    lim = pts[:, :2].abs().amax(dim=0) + 4.0
    return torch.cat([lim, float(8 * SIDE) / lim]).contiguous()


def scatter_c(pts, xform):
    L.check(L.lib().mmvae_scatter_panel(L.ptr(pts), pts.shape[0], pts.shape[1], 0, 1, L.ptr(xform), SIDE, R16, L.ptr(tone), L.ptr(panel),
                                        SIDE, st), "mmvae_scatter_panel")
    return panel


def scatter_aten(pts, xform):
    qx = torch.floor((pts[:, 0] + xform[0]) * xform[2]).long()
    qy = torch.floor((xform[1] - pts[:, 1]) * xform[3]).long()
    j = torch.div(qx - R16 - 8 + 15, 16, rounding_mode="floor")[:, None, None] + box[None, None, :]
    i = torch.div(qy - R16 - 8 + 15, 16, rounding_mode="floor")[:, None, None] + box[None, :, None]
    dx, dy = 16 * j + 8 - qx[:, None, None], 16 * i + 8 - qy[:, None, None]
    cover = (dx * dx + dy * dy <= R16 * R16) & (i >= 0) & (i < SIDE) & (j >= 0) & (j < SIDE)
    counts = torch.bincount((i * SIDE + j)[cover], minlength=SIDE * SIDE)
    return tone[counts.clamp(max=255)].view(SIDE, SIDE)


def stats_aten(mu, lv, enc):
    m, l, c = mu.double(), lv.double(), enc.double()
    e = l.exp()
    return torch.stack([m.sum(0), (m * m).sum(0), (0.5 * (e + m * m - l - 1.0)).sum(0), e.sum(0), c.sum(0), (c * c).sum(0)])


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


res = {"side": SIDE, "radius16": R16, "windows": TIMED, "us_per_call": {}}
g = torch.Generator().manual_seed(0)
for n in (5120, 204800):
    enc = torch.randn((n, Z), generator=g).to(dev)
    dense = enc[:, :2].contiguous()
    xform = xform_of(enc)
    want = scatter_aten(enc, xform)
    assert torch.equal(scatter_c(enc, xform), want) and torch.equal(scatter_c(dense, xform), want) and torch.equal(pkg.scatter_panel(enc), want)
    calls = {"scatter_c_stride32": lambda: scatter_c(enc, xform), "scatter_c_stride2": lambda: scatter_c(dense, xform),
             "scatter_panel": lambda: pkg.scatter_panel(enc), "scatter_aten": lambda: scatter_aten(enc, xform)}
    few = 100 if n == 5120 else 10
    res["us_per_call"][f"n={n}"] = time_all(calls, {"scatter_c_stride32": few, "scatter_c_stride2": few, "scatter_panel": few,
                                                     "scatter_aten": max(few // 5, 2)})
N, D = 5120, 64
mu, lv = torch.randn((N, D), generator=g).to(dev), (torch.randn((N, D), generator=g) * 0.5).to(dev)
enc = mu + torch.randn((N, D), generator=g).to(dev) * (0.5 * lv).exp()
acc = torch.empty((6, D), dtype=torch.float64, device=dev)


def stats_c():
    L.check(L.lib().mmvae_latent_stats(L.ptr(mu), L.ptr(lv), L.ptr(enc), N, D, 0, L.ptr(acc), st), "mmvae_latent_stats")
    return acc


want = stats_aten(mu, lv, enc)
assert ((stats_c() - want).abs() <= 1e-12 * want.abs().clamp_min(1.0) * N).all()
res["us_per_call"][f"stats {N}x{D}"] = time_all({"stats_c": stats_c, "stats_aten": lambda: stats_aten(mu, lv, enc)},
                                                {"stats_c": 100, "stats_aten": 100})
print(json.dumps(res), flush=True)
