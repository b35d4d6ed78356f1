"""Developer tool (GPU box): what the guard of mmvae_adam_step_guarded costs per step at the benchmark model's parameter count --
200 guarded steps against 200 mmvae_adam_step_dev steps, HIP events, warm caches, the two alternating over several rounds; next to
them the norm kernel alone (also at 1024 and 8 n elements: its fixed cost and its streaming rate) and a device-to-device copy of the
gradient buffer (the machine's copy bandwidth at this size, for scale).
Prints one JSON line."""
import importlib, json, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
L = importlib.import_module("moving-mnist-vae_amd._lib"); lib = L.lib()
M = importlib.import_module("moving-mnist-vae_amd.model")
n = int(sys.argv[1]) if len(sys.argv) > 1 else M.VAE(1, 32, 1, 2, 128, False, False, 4, "ReLu", 1, 1, 0, True, 0.1, 64)._n_params
STEPS, ROUNDS = 200, 5
g = torch.randn(n, device="cuda") * 1e-3
p, m, v, g2 = torch.randn(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.empty(n, device="cuda")
state = torch.zeros(4, dtype=torch.float64, device="cuda"); part = torch.zeros(L.SUM_PARTIALS, dtype=torch.float64, device="cuda")
acc = torch.zeros(1, dtype=torch.float64, device="cuda"); step = torch.zeros(1, dtype=torch.float64, device="cuda")
st = torch.cuda.current_stream().cuda_stream
hp = (1e-3, 0.9, 0.999, 1e-8, 0.0)
calls = {
    "guarded": lambda: L.check(lib.mmvae_adam_step_guarded(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, *hp, L.ptr(state), L.ptr(part), 1.0, 1.0, st), "guarded"),
    "plain": lambda: L.check(lib.mmvae_adam_step_dev(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, *hp, L.ptr(step), 1.0, st), "dev"),
    "norm": lambda: L.check(lib.mmvae_grad_norm_sq(L.ptr(g), n, 1.0, L.ptr(acc), L.ptr(part), st), "norm"),
    "copy": lambda: g2.copy_(g),
}
us = {k: [] for k in calls}
for r in range(ROUNDS + 1):                    # round 0 warms every call up and is dropped
    for k, fn in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS): fn()
        e1.record(); torch.cuda.synchronize()
        if r: us[k].append(e0.elapsed_time(e1) * 1000 / STEPS)
med = {k: statistics.median(x) for k, x in us.items()}
# the norm alone over sizes: time = fixed (launch + the ordered reduction's tail) + 4 n bytes / bandwidth
sweep = {}
for k in (1024, n, 8 * n):
    gk = torch.randn(k, device="cuda")
    ts = []
    for r in range(ROUNDS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS): L.check(lib.mmvae_grad_norm_sq(L.ptr(gk), k, 1.0, L.ptr(acc), L.ptr(part), st), "norm")
        e1.record(); torch.cuda.synchronize()
        if r: ts.append(e0.elapsed_time(e1) * 1000 / STEPS)
    sweep[k] = statistics.median(ts)
print(json.dumps(dict(n=n, steps=STEPS, rounds=ROUNDS, us_per_call_median=med, us_per_call_all=us, guard_us=med["guarded"] - med["plain"],
                      guard_share_of_6ms_step=(med["guarded"] - med["plain"]) / 6000.0, copy_GBps=8.0 * n / med["copy"] / 1e3,
                      norm_read_GBps=4.0 * n / med["norm"] / 1e3, norm_us_by_n=sweep, skipped=state[2].item())), flush=True)
