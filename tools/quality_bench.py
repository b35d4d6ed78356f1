"""Developer tool (GPU box): times of the per-frame quality measures against the ATen chain a user would write by hand, at
n = 5120 pairs of 64 x 64 frames -- the input as an f32 'image' column against the argmax of (n, 2, 64, 64) f32 logits, what
``reconstruction_quality`` compares for a categorical model.
  quality_c       : mmvae_frame_quality itself on a preallocated (2, n) f64 buffer
  quality_c_bytes : the same launch with both sides given as uint8 bytes (no decode, 1/6 of the input traffic): what the SSIM
                    arithmetic alone costs
  frame_quality   : the Python call (argument checks, descriptors, allocation, mse and psnr by f64 tensor operations)
  quality_aten    : the ATen chain -- argmax, lut indexing, the f32 byte rule, the five maps (a, b, a^2, b^2, a b) in f64, one depthwise
                    ``conv2d`` of them with the 11 x 11 window, the SSIM map, its mean, the squared error
The candidates alternate; each timed sample is a window of back-to-back calls between two HIP events, 3 warm-up windows, then 15 timed
ones; the medians are reported.  The ATen chain is first checked against the kernel (sse equal, ssim within 1e-9).  Prints one JSON
line."""
import ctypes, importlib, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

pkg = importlib.import_module("moving-mnist-vae_amd")
L = importlib.import_module("moving-mnist-vae_amd._lib")
assert torch.cuda.is_available(), "quality_bench needs a GPU"
dev = torch.device("cuda:0")
N, S, Q, WARM, TIMED = 5120, 64, 2, 3, 15
st = torch.cuda.current_stream().cuda_stream
g = torch.Generator().manual_seed(0)
lo, hi = -0.2345, 4.2660                                             # label 0 and label 1 at mean 0.0521, std 0.2222
lut = pkg.gray_lut(Q).to(dev)
image = torch.empty((N, S, S), device=dev)
logits = torch.empty((N, Q, S, S), device=dev)
for i in range(0, N, 512):                                           # sparse frames, noisy logits that mostly agree with them
    lab = (torch.rand((512, S, S), generator=g) < 0.06)
    image[i:i + 512] = torch.where(lab, hi, lo).to(dev)
    noise = torch.randn((512, Q, S, S), generator=g)
    noise[:, 1] += torch.where(lab, 2.0, -2.0)
    logits[i:i + 512] = noise.to(dev)
out = torch.empty((2, N), dtype=torch.float64, device=dev)
col_a = L.PanelCol(L.PANEL_IMAGE_F32, L.ptr(image), 0, None, None, lo, hi)
col_b = L.PanelCol(L.PANEL_LOGITS_ARGMAX, L.ptr(logits), Q, None, L.ptr(lut), 0.0, 1.0)
kw = torch.exp(-(torch.arange(11, dtype=torch.float64, device=dev) - 5) ** 2 / (2 * 1.5 ** 2))
kw = kw / kw.sum()
window = (kw[:, None] * kw[None, :]).expand(5, 1, 11, 11).contiguous()
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def quality_c(a=col_a, b=col_b):
    L.check(L.lib().mmvae_frame_quality(ctypes.addressof(a), ctypes.addressof(b), N, S, L.ptr(out), st), "mmvae_frame_quality")
    return out


def frame_quality():
    return pkg.frame_quality(pkg.column("image", image, lo=lo, hi=hi), pkg.column("argmax", logits, lut))


def bytes_aten():
    a = torch.floor((image - lo) / (hi - lo) * 255.0 + 0.5).clamp(0, 255)
    return a, lut[logits.argmax(dim=1)]


def quality_aten():
    a, b = bytes_aten()
    a, b = a.double(), b.double()
    d = a - b
    sse = (d * d).flatten(1).sum(1)
    E = torch.nn.functional.conv2d(torch.stack([a, b, a * a, b * b, a * b], dim=1), window, groups=5)
    ma, mb = E[:, 0], E[:, 1]
    va, vb, cab = E[:, 2] - ma * ma, E[:, 3] - mb * mb, E[:, 4] - ma * mb
    ssim = ((2 * ma * mb + C1) * (2 * cab + C2)) / ((ma * ma + mb * mb + C1) * (va + vb + C2))
    return sse, ssim.flatten(1).mean(1)


def time_all(calls, per_window):
    us = {k: [] for k in calls}
    for r in range(WARM + TIMED):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per_window[k]):
                res = fn()
            e1.record()
            torch.cuda.synchronize()
            del res
            if r >= WARM:
                us[k].append(e0.elapsed_time(e1) * 1e3 / per_window[k])
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in us.items()}


e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
quality_aten()                                                       # (the first call also picks the convolution's algorithm)
e0.record()
sse_want, ssim_want = quality_aten()
e1.record()
torch.cuda.synchronize()
aten_ms = e0.elapsed_time(e1)
got = quality_c().clone()
py = frame_quality()
assert torch.equal(got[0], sse_want) and torch.equal(py["sse"], sse_want) and torch.equal(py["ssim"], got[1])
worst = (got[1] - ssim_want).abs().max().item()
assert worst <= 1e-9, worst
a_bytes, b_bytes = (t.to(torch.uint8).contiguous() for t in bytes_aten())
del sse_want, ssim_want
col_ab = L.PanelCol(L.FRAME_BYTES_U8, L.ptr(a_bytes), 0, None, None, 0.0, 0.0)
col_bb = L.PanelCol(L.FRAME_BYTES_U8, L.ptr(b_bytes), 0, None, None, 0.0, 0.0)
assert torch.equal(quality_c(col_ab, col_bb), got)
calls = {"quality_c": quality_c, "quality_c_bytes": lambda: quality_c(col_ab, col_bb), "frame_quality": frame_quality,
         "quality_aten": quality_aten}
res = {"n": N, "S": S, "Q": Q, "windows": TIMED, "worst_ssim_difference_to_aten": worst,
       "input_bytes": {"quality_c": image.numel() * 4 + logits.numel() * 4, "quality_c_bytes": 2 * N * S * S},
       "us_per_call": time_all(calls, {"quality_c": 20, "quality_c_bytes": 20, "frame_quality": 20,
                                       "quality_aten": 3 if aten_ms < 200.0 else 1})}
print(json.dumps(res), flush=True)
