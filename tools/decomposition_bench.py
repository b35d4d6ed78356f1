"""Developer tool (GPU box): times of the aggregate-posterior sweep (mmvae_posterior_mixture) against the ATen chain a user would write
by hand, at the size of the Moving-MNIST test split: N = M = 20 000 samples and posteriors, z = 32 and z = 64, with and without the
per-dimension output.
  mixture_c     : mmvae_posterior_mixture itself on preallocated outputs and scratch
  mixture       : the Python call (argument checks, the cached scratch, the output allocations)
  aten          : the ATen chain -- the bank in chunks of CHUNK rows, the broadcast (CHUNK, N, z) f32 terms, ``logsumexp`` over the
                  chunk (of the terms for the per-dimension output, of their sum over z for the joint), the chunk results stacked and
                  combined by one more ``logsumexp`` in f64.  Its peak extra memory (torch.cuda.max_memory_allocated over the call) is
                  reported.
Each path is first checked against the other (|difference| <= 1e-4 (1 + |value|): the chain's terms and sums are f32).  The candidates
alternate; each timed sample is a window of back-to-back calls between two HIP events, 3 warm-up windows, then 15 timed ones; the
medians are reported.

pair_terms_per_s = N * M * z / time.  Ceilings for this chip, 256 CUs x 4 SIMDs at 2.4 GHz:
  exponentials  v_exp_f32 is a quarter-rate instruction: 16 lanes per clock and SIMD, so 256 * 4 * 16 * 2.4e9 = 3.93e13 per second.
                The per-dimension output needs one exponential per pair-term, so that is its ceiling in pair-terms per second.
  plain VALU    32 lanes per clock and SIMD: 7.86e13 lane-operations per second.  The joint alone needs a subtract, a multiply and an
                FMA per pair-term and one exponential per PAIR: its ceiling is 7.86e13 / 3 = 2.62e13 pair-terms per second.
Prints one JSON line."""
import importlib, json, math, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

pkg = importlib.import_module("moving-mnist-vae_amd")
L = importlib.import_module("moving-mnist-vae_amd._lib")
assert torch.cuda.is_available(), "decomposition_bench needs a GPU"
dev = torch.device("cuda:0")
N = M = 20000
CHUNK, WARM, TIMED = 64, 3, 15
EXP_CEILING, VALU_CEILING = 256 * 4 * 16 * 2.4e9, 256 * 4 * 32 * 2.4e9
LOG_2PI = math.log(2.0 * math.pi)
st = torch.cuda.current_stream().cuda_stream


def inputs(d):
    g = torch.Generator().manual_seed(d)
    mu, lv = torch.randn((M, d), generator=g), torch.rand((M, d), generator=g) * 4.0 - 4.0
    z = mu + torch.exp(0.5 * lv) * torch.randn((N, d), generator=g)
    return z.to(dev), mu.to(dev), lv.to(dev)


class MixtureC:
    """mmvae_posterior_mixture on buffers allocated once."""

    def __init__(self, z, mu, lv, per_dim):
        self.z, self.mu, self.lv, d = z, mu, lv, z.shape[1]
        self.nbytes = L.lib().mmvae_posterior_mixture_scratch_bytes(N, M, d)
        self.scratch = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.out = torch.empty(N, dtype=torch.float64, device=dev)
        self.dims = torch.empty((N, d), dtype=torch.float64, device=dev) if per_dim else None

    def __call__(self):
        L.check(L.lib().mmvae_posterior_mixture(L.ptr(self.z), N, L.ptr(self.mu), L.ptr(self.lv), M, self.z.shape[1], L.ptr(self.out),
                                                L.ptr(self.dims), L.ptr(self.scratch), self.nbytes, st), "mmvae_posterior_mixture")
        return self.out, self.dims


def aten(z, mu, lv, per_dim):
    w, c = -0.5 * torch.exp(-lv), -0.5 * (lv + LOG_2PI)
    joint, dims = [], []
    for j0 in range(0, M, CHUNK):
        t = (z[None] - mu[j0:j0 + CHUNK, None]) ** 2 * w[j0:j0 + CHUNK, None] + c[j0:j0 + CHUNK, None]      # (CHUNK, N, z) f32
        joint.append(torch.logsumexp(t.sum(2), 0))
        if per_dim:
            dims.append(torch.logsumexp(t, 0))
    log_m = math.log(M)
    return (torch.logsumexp(torch.stack(joint).double(), 0) - log_m,
            torch.logsumexp(torch.stack(dims).double(), 0) - log_m if per_dim else None)


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


res = {"N": N, "M": M, "aten_chunk": CHUNK, "windows": TIMED, "exp_ceiling_per_s": EXP_CEILING, "valu_ceiling_per_s": VALU_CEILING, "cases": {}}
for d in (32, 64):
    z, mu, lv = inputs(d)
    for per_dim in (False, True):
        c_call = MixtureC(z, mu, lv, per_dim)
        got = tuple(None if t is None else t.clone() for t in c_call())
        py = pkg.posterior_mixture(z, mu, lv, per_dim=per_dim)
        assert torch.equal(py[0], got[0]) and (not per_dim or torch.equal(py[1], got[1]))
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        want = aten(z, mu, lv, per_dim)
        torch.cuda.synchronize()
        aten_peak = torch.cuda.max_memory_allocated() - base
        worst = []
        for g, w in zip(got, want):
            if g is not None:
                worst.append(((g - w).abs() / (1.0 + w.abs())).max().item())
                assert worst[-1] <= 1e-4, worst
        del want, py, got
        calls = {"mixture_c": c_call, "mixture": lambda: pkg.posterior_mixture(z, mu, lv, per_dim=per_dim), "aten": lambda: aten(z, mu, lv, per_dim)}
        t = time_all(calls, {"mixture_c": 5, "mixture": 5, "aten": 1})
        terms = float(N) * M * d
        rate = terms / (t["mixture_c"]["median"] * 1e-6)
        res["cases"][f"z{d}_{'dims' if per_dim else 'joint'}"] = {
            "us_per_call": t, "worst_relative_difference_to_aten": worst, "aten_peak_extra_bytes": aten_peak,
            "scratch_bytes": c_call.nbytes, "pair_terms_per_s": rate,
            "fraction_of_ceiling": rate / (EXP_CEILING if per_dim else VALU_CEILING / 3.0),
            "speedup_over_aten": t["aten"]["median"] / t["mixture_c"]["median"]}
        del c_call, calls
print(json.dumps(res), flush=True)
