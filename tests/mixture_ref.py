"""The f64 reference of mmvae_posterior_mixture and of elbo_decomposition, the error scale of the gate, and the inputs of the cases
that tests/test_decomposition_cpu.py (conditions on the inputs, identities) and tests/test_decomposition_gpu.py (parity) share.

Reference: the header's formulas in torch f64 from the f32 inputs, with torch.logsumexp.  Error scale, with
a = (z - mu)^2 exp(-logvar) in f64:
    e_ijd = 0.5 * (a_ijd * (4 + |logvar_jd|) + |logvar_jd| + log 2 pi)
    B_i   = sum_j softmax_j(s_i.)  * sum_d e_ijd + |log_qz[i]|          + 1
    B_id  = sum_j softmax_j(t_i.d) * e_ijd       + |log_qz_dims[i][d]|  + 1
Gate: |device - reference| <= K * 2^-24 * B for every element of both outputs (K: tests/test_decomposition_gpu.py)."""
import functools
import math

import torch

U = 2.0 ** -24
LOG_2PI = math.log(2.0 * math.pi)
MIN_CHUNK = 64                # MIXTURE_MIN_CHUNK of _lib.py: with a single block of samples the bank is cut into chunks of 64 rows

# name -> (N, M, d, spread of the bank means, lo, hi of the bank log-variances, seed)
CASES = {
    "one": (1, 1, 1, 1.0, -2.0, 1.0, 1),
    "ragged_67x130": (67, 130, 5, 2.0, -6.0, 0.0, 2),
    "ragged_130x67": (130, 67, 33, 1.0, -12.0, 4.0, 3),
    "64x1000x64": (64, 1000, 64, 1.0, -4.0, 0.0, 4),
    "257x257x2": (257, 257, 2, 3.0, -8.0, 2.0, 5),
    "three_tiles_d130": (40, 300, 130, 1.0, -3.0, 1.0, 6),
    "widest_d512": (9, 70, 512, 0.5, -2.0, 0.0, 7),
    "chunk_edges": (3, 3 * MIN_CHUNK + 7, 64, 1.0, -5.0, 1.0, 8),          # three whole chunks of the bank and a remainder of 7 rows
    "one_chunk": (300, 40, 20, 1.0, -4.0, 1.0, 9),                          # fewer rows than a chunk: the sweep writes the outputs itself
    "extreme": (8, 24, 6, None, None, None, 10),
}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(z (N, d), mu (M, d), logvar (M, d), index (N,)) as f32 / int64 CPU tensors; sample i is drawn from posterior index[i]."""
    N, M, d, spread, lo, hi, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    if name == "extreme":
        # in-domain extremes: rows 0..7 ordinary, 8..15 logvar = +30, 16..19 logvar = -30 at mu ~ +9990, 20..23 at mu ~ -9990;
        # samples 0..5 sit 1e4 away from rows 16..23, sample 6 on row 16 and sample 7 near row 20 sit 1e4 away from everything else
        mu = torch.randn((M, d), generator=g)
        lv = torch.rand((M, d), generator=g) * 2.0 - 2.0
        lv[8:16] = 30.0
        lv[16:20] = -30.0
        mu[16:20] = 9990.0 + torch.arange(4.0)[:, None] * 0.5
        mu[20:24] = -9990.0 - torch.arange(4.0)[:, None]
        index = torch.tensor([0, 1, 2, 3, 4, 5, 16, 20])
    else:
        mu = spread * torch.randn((M, d), generator=g)
        lv = lo + (hi - lo) * torch.rand((M, d), generator=g)
        index = torch.arange(N) % M
    z = mu[index] + torch.exp(0.5 * lv[index]) * torch.randn((N, d), generator=g)
    return z.float().contiguous(), mu.float().contiguous(), lv.float().contiguous(), index


def mixture_ref(z, mu, lv):
    """dict of f64 CPU tensors: log_qz (N,), log_qz_dims (N, d), their error scales B (N,), B_dims (N, d), and top_weight (N,), the
    largest softmax weight of a bank row in the joint."""
    z, mu, lv = z.double(), mu.double(), lv.double()
    M = mu.shape[0]
    a = (z[:, None, :] - mu[None]) ** 2 * torch.exp(-lv)[None]                    # (N, M, d)
    t = -0.5 * (a + lv[None] + LOG_2PI)
    e = 0.5 * (a * (4.0 + lv.abs()[None]) + lv.abs()[None] + LOG_2PI)
    s = t.sum(2)
    log_qz = torch.logsumexp(s, 1) - math.log(M)
    dims = torch.logsumexp(t, 1) - math.log(M)
    w, wd = torch.softmax(s, 1), torch.softmax(t, 1)
    return {"log_qz": log_qz, "log_qz_dims": dims, "B": (w * e.sum(2)).sum(1) + log_qz.abs() + 1.0,
            "B_dims": (wd * e).sum(1) + dims.abs() + 1.0, "top_weight": w.max(1).values}


@functools.lru_cache(maxsize=None)
def case_ref(name):
    z, mu, lv, _ = case_inputs(name)
    return mixture_ref(z, mu, lv)


def own_density(z, mu, lv):
    """log N(z_i; mu_i, exp(lv_i)) summed over d, f64 from the f32 inputs, rows matched."""
    z, mu, lv = z.double(), mu.double(), lv.double()
    return (-0.5 * ((z - mu) ** 2 * torch.exp(-lv) + lv + LOG_2PI)).sum(1)


def decomposition_ref(mu, lv, z, index=None, log_qz=None, dims=None):
    """elbo_decomposition in f64 on the CPU.  log_qz / dims: the mixture outputs to use (default: the f64 reference's)."""
    if log_qz is None:
        r = mixture_ref(z, mu, lv)
        log_qz, dims = r["log_qz"], r["log_qz_dims"]
    M = mu.shape[0]
    index = torch.arange(z.shape[0]) if index is None else index
    z64, m64, l64 = z.double(), mu.double()[index], lv.double()[index]
    own = own_density(z, mu[index], lv[index])
    pz_dims = -0.5 * (z64 * z64 + LOG_2PI)
    pz, indep = pz_dims.sum(1), dims.sum(1)
    tc, dwkl = (log_qz - indep).mean(), (indep - pz).mean()
    return {"mi": (own - log_qz).mean(), "tc": tc, "dwkl": dwkl, "marginal_kl": tc + dwkl, "kl_sampled": (own - pz).mean(),
            "kl_analytic": (0.5 * (torch.exp(l64) + m64 * m64 - l64 - 1.0)).sum(1).mean(), "dwkl_per_dim": (dims - pz_dims).mean(0),
            "log_m": torch.tensor(math.log(M), dtype=torch.float64), "n": z.shape[0], "m": M}
