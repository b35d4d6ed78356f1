"""Developer tool (GPU box): time of one `recon` contact sheet -- 8 argmax columns, n = 6 planes, S = 64, Q = 2: a (384, 512) uint8
sheet from eight (6, 2, 64, 64) f32 logits tensors -- through render_sheet (one mmvae_panel_sheet launch) against the equivalent ATen
chain a user would write by hand: per column ``lut[logits.argmax(dim=1)]``, the strips concatenated with ``torch.cat`` and ``.to(uint8)``.
  sheet_c      : the library call itself on a preallocated sheet and prebuilt descriptors
  render_sheet : the Python call (argument checks, descriptor array, allocation of the sheet)
  aten         : the chain above (17 ATen kernels)
Both Python rows include their host work: at this size every candidate is bound by launches, not by bytes (the sheet is 196 KB).
The candidates alternate; each timed sample is a window of 200 back-to-back calls between two HIP events (one call is a few
microseconds, far below an event pair's resolution), 3 warm-up windows, then 15 timed ones.  Prints one JSON line."""
import ctypes, importlib, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

pkg = importlib.import_module("moving-mnist-vae_amd")
L = importlib.import_module("moving-mnist-vae_amd._lib")
assert torch.cuda.is_available(), "panels_bench needs a GPU"
dev = torch.device("cuda:0")
NCOLS, N, S, Q, WARM, TIMED, CALLS = 8, 6, 64, 2, 3, 15, 200
g = torch.Generator().manual_seed(0)
logits = [torch.randn((N, Q, S, S), generator=g).to(dev) for _ in range(NCOLS)]
lut = pkg.gray_lut(Q).to(dev)
lut_f = lut.float()
cols = [pkg.column("argmax", x, lut) for x in logits]
arr = (L.PanelCol * NCOLS)(*[L.PanelCol(L.PANEL_LOGITS_ARGMAX, L.ptr(x), Q, None, L.ptr(lut), 0.0, 1.0) for x in logits])
sheet = torch.empty((N * S, NCOLS * S), dtype=torch.uint8, device=dev)
st = torch.cuda.current_stream().cuda_stream


def sheet_c():
    L.check(L.lib().mmvae_panel_sheet(ctypes.addressof(arr), NCOLS, N, S, L.ptr(sheet), st), "mmvae_panel_sheet")
    return sheet


def render_sheet():
    return pkg.render_sheet(cols, N)


def aten():
    return torch.cat([lut_f[x.argmax(dim=1)].reshape(N * S, S) for x in logits], dim=1).to(torch.uint8)


calls = {"sheet_c": sheet_c, "render_sheet": render_sheet, "aten": aten}
want = aten()
for k, fn in calls.items():
    assert torch.equal(fn(), want), k                       # (random logits: no ties)
us = {k: [] for k in calls}
for r in range(WARM + TIMED):
    for k, fn in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        del out
        if r >= WARM:
            us[k].append(e0.elapsed_time(e1) * 1e3 / CALLS)
res = {"sheet": [N * S, NCOLS * S], "columns": NCOLS, "n": N, "S": S, "Q": Q, "calls_per_window": CALLS, "windows": TIMED,
       "us_per_call": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in us.items()}}
print(json.dumps(res), flush=True)
