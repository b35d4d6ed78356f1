"""Developer tool (GPU box): what the gradient of the aggregate-posterior sweep costs (mmvae_posterior_mixture_bwd), at
training batches: N = M = 5120 and 10240 samples and posteriors, z = 32 and z = 64, both upstream gradients (the total correlation's
pattern, g_joint = 1 / N and g_dims = -1 / N).
  forward_c     : mmvae_posterior_mixture itself, both outputs, on preallocated buffers -- the yardstick, code of the parent commit
  backward_c    : mmvae_posterior_mixture_bwd itself on preallocated buffers
  op            : posterior_mixture(differentiable=True) and torch.autograd.grad through it (checks, allocations, one forward + one backward)
  aten          : the ATen autograd chain a user would write -- the bank in chunks of CHUNK rows, the broadcast (CHUNK, N, z) f32 terms,
                  ``logsumexp`` per chunk, the chunk results combined by one more ``logsumexp`` in f64, ``.backward()``.  Autograd keeps
                  every chunk's broadcast intermediates, about 5 * N * M * z * 4 bytes; a shape whose estimate exceeds ATEN_BUDGET is not
                  run (it is reported as not fitting the budget), the others report their measured peak extra memory.
Each path is first checked against the other (|difference| <= 1e-3 of the largest gradient: the chain's terms and sums are f32).  The
candidates alternate; each timed sample is a window of back-to-back calls between two HIP events, 3 warm-up windows, then 15 timed ones;
medians are reported.  backward_over_forward is the ratio of the two library calls; by operation count it is
(ntiles * (3 z + 12 * 16) + ntiles * (3 z + 14 * 16)) / (3 z + 10 z) with ntiles = ceil(z / 16): the joint exponent is recomputed by
every 16-dimension tile of both sweeps.

Whole step (--step): a 5120-frame config-2 train step (bench.py's model, batch and loop) with ``args.latent_penalty =
make_latent_penalty(beta=6)`` and without the attribute, alternating, STEP_ROUNDS rounds of STEP_STEPS steps each after a warm-up.
Prints one JSON line."""
import importlib, json, math, os, statistics, sys, time, types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

pkg = importlib.import_module("moving-mnist-vae_amd")
L = importlib.import_module("moving-mnist-vae_amd._lib")
assert torch.cuda.is_available(), "mixture_grad_bench needs a GPU"
dev = torch.device("cuda:0")
CHUNK, WARM, TIMED = 64, 3, 15
ATEN_BUDGET = 48 << 30
STEP_ROUNDS, STEP_STEPS = 3, 20
LOG_2PI = math.log(2.0 * math.pi)
st = torch.cuda.current_stream().cuda_stream


def inputs(N, d):
    g = torch.Generator().manual_seed(d)
    mu, lv = torch.randn((N, d), generator=g), torch.rand((N, d), generator=g) * 4.0 - 4.0
    z = mu + torch.exp(0.5 * lv) * torch.randn((N, d), generator=g)
    return z.to(dev), mu.to(dev), lv.to(dev)


class LibraryCalls:
    """Both C entry points on buffers allocated once."""

    def __init__(self, z, mu, lv, gj, gd):
        self.z, self.mu, self.lv, self.gj, self.gd = z, mu, lv, gj, gd
        (self.N, self.d), lib = z.shape, L.lib()
        self.fbytes = lib.mmvae_posterior_mixture_scratch_bytes(self.N, self.N, self.d)
        self.bbytes = lib.mmvae_posterior_mixture_bwd_scratch_bytes(self.N, self.N, self.d)
        self.fscratch = torch.empty(self.fbytes, dtype=torch.uint8, device=dev)
        self.bscratch = torch.empty(self.bbytes, dtype=torch.uint8, device=dev)
        self.out = torch.empty(self.N, dtype=torch.float64, device=dev)
        self.dims = torch.empty((self.N, self.d), dtype=torch.float64, device=dev)
        self.grads = tuple(torch.empty_like(t) for t in (z, mu, lv))

    def forward(self):
        L.check(L.lib().mmvae_posterior_mixture(L.ptr(self.z), self.N, L.ptr(self.mu), L.ptr(self.lv), self.N, self.d, L.ptr(self.out),
                                                L.ptr(self.dims), L.ptr(self.fscratch), self.fbytes, st), "mmvae_posterior_mixture")

    def backward(self):
        g = self.grads
        L.check(L.lib().mmvae_posterior_mixture_bwd(L.ptr(self.z), self.N, L.ptr(self.mu), L.ptr(self.lv), self.N, self.d, L.ptr(self.out),
                                                    L.ptr(self.dims), L.ptr(self.gj), L.ptr(self.gd), L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]),
                                                    L.ptr(self.bscratch), self.bbytes, st), "mmvae_posterior_mixture_bwd")
        return g


def op_grads(z, mu, lv, gj, gd):
    leaves = [t.detach().requires_grad_(True) for t in (z, mu, lv)]
    log_qz, dims = pkg.posterior_mixture(*leaves, differentiable=True)
    return torch.autograd.grad((gj * log_qz).sum() + (gd * dims).sum(), leaves)


def aten_grads(z, mu, lv, gj, gd):
    z, mu, lv = (t.detach().requires_grad_(True) for t in (z, mu, lv))
    M = mu.shape[0]
    w, c = -0.5 * torch.exp(-lv), -0.5 * (lv + LOG_2PI)
    joint, dims = [], []
    for j0 in range(0, M, CHUNK):
        t = (z[None] - mu[j0:j0 + CHUNK, None]) ** 2 * w[j0:j0 + CHUNK, None] + c[j0:j0 + CHUNK, None]      # (CHUNK, N, z) f32
        joint.append(torch.logsumexp(t.sum(2), 0))
        dims.append(torch.logsumexp(t, 0))
    log_m = math.log(M)
    log_qz = torch.logsumexp(torch.stack(joint).double(), 0) - log_m
    log_qz_dims = torch.logsumexp(torch.stack(dims).double(), 0) - log_m
    return torch.autograd.grad((gj * log_qz).sum() + (gd * log_qz_dims).sum(), (z, mu, lv))


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


def kernel_cases():
    cases = {}
    for N in (5120, 10240):
        for d in (32, 64):
            z, mu, lv = inputs(N, d)
            gj = torch.full((N,), 1.0 / N, dtype=torch.float64, device=dev)
            gd = torch.full((N, d), -1.0 / N, dtype=torch.float64, device=dev)
            lib_calls = LibraryCalls(z, mu, lv, gj, gd)
            lib_calls.forward()
            got = tuple(t.clone() for t in lib_calls.backward())
            op = op_grads(z, mu, lv, gj, gd)
            assert all(torch.equal(a, b) for a, b in zip(got, op))
            calls = {"forward_c": lib_calls.forward, "backward_c": lib_calls.backward, "op": lambda: op_grads(z, mu, lv, gj, gd)}
            window = {"forward_c": 5, "backward_c": 5, "op": 5}
            rec = {"scratch_bytes": lib_calls.bbytes, "aten_estimate_bytes": 5 * N * N * d * 4}
            if rec["aten_estimate_bytes"] <= ATEN_BUDGET:
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                want = aten_grads(z, mu, lv, gj, gd)
                torch.cuda.synchronize()
                rec["aten_peak_extra_bytes"] = torch.cuda.max_memory_allocated() - base
                rec["worst_difference_to_aten_over_largest_gradient"] = [((g - w).abs().max() / w.abs().max()).item() for g, w in zip(got, want)]
                assert max(rec["worst_difference_to_aten_over_largest_gradient"]) <= 1e-3, rec
                del want
                calls["aten"], window["aten"] = (lambda: aten_grads(z, mu, lv, gj, gd)), 1
            else:
                rec["aten"] = f"not run: its autograd intermediates (about {rec['aten_estimate_bytes'] / 2 ** 30:.0f} GiB) exceed the {ATEN_BUDGET >> 30} GiB budget"
            del op, got
            t = time_all(calls, window)
            rec["us_per_call"] = t
            rec["backward_over_forward"] = t["backward_c"]["median"] / t["forward_c"]["median"]
            nt = (d + 15) // 16
            rec["backward_over_forward_by_operation_count"] = (nt * (3 * d + 12 * 16) + nt * (3 * d + 14 * 16)) / (13.0 * d)
            rec["pair_terms_per_s_backward"] = float(N) * N * d / (t["backward_c"]["median"] * 1e-6)
            if "aten" in t:
                rec["speedup_over_aten"] = t["aten"]["median"] / (t["forward_c"]["median"] + t["backward_c"]["median"])
            cases[f"N{N}_z{d}"] = rec
            del lib_calls, calls
            torch.cuda.empty_cache()
    return cases


def whole_step():
    """bench.py's headline loop (config 2: 256 clips = 5120 frames, z = 128, bf16) with and without the hook, alternating."""
    bench = importlib.import_module("bench")
    M = importlib.import_module("moving-mnist-vae_amd.model")
    torch.manual_seed(0)
    model = M.VAE(1, 32, 1, 2, 128, False, False, 4, "ReLu", 1, 1, 0, True, 0.1, 64, compute_dtype="bf16").to(dev).train()
    opt = M.FusedAdam(list(model.parameters()))
    batch = bench.synthetic_clips(256, 1234, dev)
    hook = pkg.make_latent_penalty(beta=6)
    plain = types.SimpleNamespace(data_ratio_of_labels=None, dataset="MovingMNIST", quiet=True)
    hooked = types.SimpleNamespace(data_ratio_of_labels=None, dataset="MovingMNIST", quiet=True, latent_penalty=hook)

    def run(args, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pkg.train(model, [batch] * k, opt, dev, args, data_mean=bench.DATA_MEAN, data_std=bench.DATA_STD)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k

    run(plain, 5)
    run(hooked, 5)
    ms = {"without": [], "with_beta6": []}
    for _ in range(STEP_ROUNDS):
        ms["without"].append(run(plain, STEP_STEPS))
        ms["with_beta6"].append(run(hooked, STEP_STEPS))
    rows = hook.to_host()
    out = {k: {"median_ms_per_step": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}
    out["frames"], out["z"], out["rounds"], out["steps_per_round"] = 5120, 128, STEP_ROUNDS, STEP_STEPS
    out["added_ms_per_step"] = out["with_beta6"]["median_ms_per_step"] - out["without"]["median_ms_per_step"]
    out["last_penalty_mi_tc_dwkl"] = [float(v) for v in rows[-1]]
    return out


res = {"aten_chunk": CHUNK, "windows": TIMED}
if "--step" in sys.argv[1:]:
    res["whole_step"] = whole_step()
else:
    res["cases"] = kernel_cases()
print(json.dumps(res), flush=True)
