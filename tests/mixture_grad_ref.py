"""The f64 reference of mmvae_posterior_mixture_bwd (the gradient of mmvae_posterior_mixture), the error scale of its gate, a plain f32
restatement that fixes the gate's constant, and the upstream-gradient patterns that tests/test_mixture_grad_cpu.py and
tests/test_mixture_grad_gpu.py share.  The cases and their inputs are those of tests/mixture_ref.py.

Reference, with t_ijd / s_ij of mixture_ref.py, r = softmax_j s, rd = softmax_j t (per dimension), upstream g_joint [N], g_dims [N][d]:
    a_ijd = g_joint[i] r_ij + g_dims[i][d] rd_ijd,        u_ijd = (z_id - mu_jd) exp(-logvar_jd)
    d_z[i][d] = -sum_j a u,    d_mu[j][d] = sum_i a u,    d_logvar[j][d] = sum_i a 0.5 ((z_id - mu_jd) u - 1)
Error scale, with U = 2^-24, e_ijd, B_i, B_id of mixture_ref.py, E_ij = sum_d e_ijd + B_i, E_ijd = e_ijd + B_id,
am(E) = 4 + expm1(min(U E, 80)) / U (a relative error U E of an exponent multiplies the weight by e^(U E): 4 + E while U E is small) and
F = 2^-100 (the f32 underflow of a weight):
    W_ijd = |g_joint[i]| (r_ij + F) am(E_ij) + |g_dims[i][d]| (rd_ijd + F) am(E_ijd)
    B(d_z[i][d]) = sum_j W |u|,   B(d_mu[j][d]) = sum_i W |u|,   B(d_logvar[j][d]) = sum_i W 0.5 (|z_id - mu_jd| |u| + 1)
Gate: |device - reference| <= K * U * B for every element of the three outputs.  K is NOT fitted to the kernel: it is twice the largest
ratio that `restatement_f32` (the same formulas in torch f32 with softmax, no chunking) reaches against the f64 reference over CASES x
PATTERNS, rounded up to a power of two -- the factor of two allows for another summation order.  test_mixture_grad_cpu.py re-derives the
ratio on every run and asserts it stays within K / 2.

The penalty's gradient (latent_penalty) adds the elementwise parts that autograd forms in f64 and rounds to the f32 inputs' dtype: the own
density (coefficient alpha - 1) and the prior (gamma - 1).  Their scale per element is O(1) terms, `elementwise_scale` below."""
import functools
import math

import torch

from mixture_ref import CASES, LOG_2PI, case_inputs

U = 2.0 ** -24
F = 2.0 ** -100
K = 2.0                       # 2 x 0.880 (chunk_edges, 'tc' pattern, d_mu: the largest of the 120 ratios), up to a power of two
PATTERNS = ("tc", "random", "joint", "dims")


def upstream(name, pattern):
    """(g_joint (N,) or None, g_dims (N, d) or None) as f64 CPU tensors: 'tc' is what the total correlation's mean sends down."""
    N, _, d = CASES[name][:3]
    g = torch.Generator().manual_seed(99)
    gj, gd = torch.randn(N, generator=g, dtype=torch.float64), torch.randn((N, d), generator=g, dtype=torch.float64)
    if pattern == "tc":
        return torch.full((N,), 1.0 / N, dtype=torch.float64), torch.full((N, d), -1.0 / N, dtype=torch.float64)
    if pattern == "random":
        return gj, gd
    if pattern == "joint":
        return gj, None
    assert pattern == "dims"
    return None, gd


def am(E):
    return 4.0 + torch.expm1(torch.clamp(U * E, max=80.0)) / U


def grad_ref(z, mu, lv, g_joint, g_dims):
    """dict of f64 CPU tensors: d_z (N, d), d_mu, d_lv (M, d), their error scales B_z, B_mu, B_lv, and ue_max: the largest U * E over
    the pairs that carry weight (r >= 2^-60, resp. rd >= 2^-60) -- the gate is 4 + E there while this stays small."""
    z, mu, lv = z.double(), mu.double(), lv.double()
    (N, d), M = z.shape, mu.shape[0]
    gj = torch.zeros(N, dtype=torch.float64) if g_joint is None else g_joint.double()
    gd = torch.zeros((N, d), dtype=torch.float64) if g_dims is None else g_dims.double()
    dl = z[:, None, :] - mu[None]                                                  # (N, M, d)
    iv = torch.exp(-lv)[None]
    sq = dl * dl * iv
    t = -0.5 * (sq + lv[None] + LOG_2PI)
    s = t.sum(2)
    r, rd = torch.softmax(s, 1), torch.softmax(t, 1)
    u = dl * iv
    a = gj[:, None, None] * r[:, :, None] + gd[:, None, :] * rd
    half = 0.5 * (dl * u - 1.0)
    out = {"d_z": -(a * u).sum(1), "d_mu": (a * u).sum(0), "d_lv": (a * half).sum(0)}
    e = 0.5 * (sq * (4.0 + lv.abs()[None]) + lv.abs()[None] + LOG_2PI)
    log_qz, dims = torch.logsumexp(s, 1) - math.log(M), torch.logsumexp(t, 1) - math.log(M)
    B_i = (r * e.sum(2)).sum(1) + log_qz.abs() + 1.0
    B_id = (rd * e).sum(1) + dims.abs() + 1.0
    E_j, E_d = e.sum(2) + B_i[:, None], e + B_id[:, None, :]
    W = gj.abs()[:, None, None] * ((r + F) * am(E_j))[:, :, None] + gd.abs()[:, None, :] * (rd + F) * am(E_d)
    out.update(B_z=(W * u.abs()).sum(1), B_mu=(W * u.abs()).sum(0), B_lv=(W * 0.5 * (dl.abs() * u.abs() + 1.0)).sum(0))
    heavy_j, heavy_d = r >= 2.0 ** -60, rd >= 2.0 ** -60
    out["ue_max"] = U * max(E_j[heavy_j].max().item(), E_d[heavy_d].max().item())
    return out


@functools.lru_cache(maxsize=None)
def case_grad_ref(name, pattern):
    z, mu, lv, _ = case_inputs(name)
    return grad_ref(z, mu, lv, *upstream(name, pattern))


def restatement_f32(z, mu, lv, g_joint, g_dims):
    """The same formulas in plain torch f32 (softmax, whole-array sums): what f32 arithmetic reaches without any care."""
    z, mu, lv = z.float(), mu.float(), lv.float()
    (N, d) = z.shape
    gj = torch.zeros(N) if g_joint is None else g_joint.float()
    gd = torch.zeros((N, d)) if g_dims is None else g_dims.float()
    dl = z[:, None, :] - mu[None]
    iv = torch.exp(-lv)[None]
    t = -0.5 * (dl * dl * iv + lv[None] + float(LOG_2PI))
    r, rd = torch.softmax(t.sum(2), 1), torch.softmax(t, 1)
    u = dl * iv
    a = gj[:, None, None] * r[:, :, None] + gd[:, None, :] * rd
    return {"d_z": -(a * u).sum(1), "d_mu": (a * u).sum(0), "d_lv": (a * (0.5 * (dl * u - 1.0))).sum(0)}


def ratios(got, ref):
    """{'d_z', 'd_mu', 'd_lv'} -> the largest |got - reference| / (U * B) of that output; `got` may hold device or f32 tensors."""
    return {k: ((got[k].detach().cpu().double() - ref[k]).abs() / (U * ref["B_" + k[2:]])).max().item() for k in ("d_z", "d_mu", "d_lv")}


def autograd_ref(z, mu, lv, g_joint, g_dims):
    """torch f64 autograd of mixture_ref.py's formulas: (d_z, d_mu, d_lv)."""
    z, mu, lv = (t.double().clone().requires_grad_(True) for t in (z, mu, lv))
    M = mu.shape[0]
    t = -0.5 * ((z[:, None, :] - mu[None]) ** 2 * torch.exp(-lv)[None] + lv[None] + LOG_2PI)
    log_qz, dims = torch.logsumexp(t.sum(2), 1) - math.log(M), torch.logsumexp(t, 1) - math.log(M)
    form = 0.0
    if g_joint is not None:
        form = form + (g_joint * log_qz).sum()
    if g_dims is not None:
        form = form + (g_dims * dims).sum()
    return torch.autograd.grad(form, (z, mu, lv))


def penalty_ref(mu, lv, z, alpha=1.0, beta=1.0, gamma=1.0, dataset_size=None):
    """latent_penalty in f64 on the CPU (sample i from posterior i): (penalty, terms, (d_mu, d_lv, d_z)) by torch autograd."""
    z, mu, lv = (t.double().clone().requires_grad_(True) for t in (z, mu, lv))
    (N, d) = z.shape
    t = -0.5 * ((z[:, None, :] - mu[None]) ** 2 * torch.exp(-lv)[None] + lv[None] + LOG_2PI)
    log_qz, dims = torch.logsumexp(t.sum(2), 1) - math.log(N), torch.logsumexp(t, 1) - math.log(N)
    own = (-0.5 * ((z - mu) ** 2 * torch.exp(-lv) + lv + LOG_2PI)).sum(1)
    pz, indep = (-0.5 * (z * z + LOG_2PI)).sum(1), dims.sum(1)
    terms = {"mi": (own - log_qz).mean(), "tc": (log_qz - indep).mean(), "dwkl": (indep - pz).mean()}
    if dataset_size is not None:
        log_d = math.log(dataset_size)
        terms = {"mi": terms["mi"] + log_d, "tc": terms["tc"] + (d - 1) * log_d, "dwkl": terms["dwkl"] - d * log_d}
    penalty = (alpha - 1.0) * terms["mi"] + (beta - 1.0) * terms["tc"] + (gamma - 1.0) * terms["dwkl"]
    grads = torch.autograd.grad(penalty, (mu, lv, z))
    return penalty.detach(), {k: v.detach() for k, v in terms.items()}, grads


def penalty_upstream(N, d, alpha=1.0, beta=1.0, gamma=1.0):
    """The upstream gradients that the penalty's composition sends into the mixture: log_qz enters mi with -1 / N and tc with 1 / N;
    each log_qz_dims enters tc with -1 / N and dwkl with 1 / N."""
    gj = ((beta - 1.0) - (alpha - 1.0)) / N
    gd = ((gamma - 1.0) - (beta - 1.0)) / N
    return torch.full((N,), gj, dtype=torch.float64), torch.full((N, d), gd, dtype=torch.float64)


def elementwise_scale(mu, lv, z, alpha=1.0, gamma=1.0):
    """The scale of the penalty gradient's elementwise parts (own density, prior), per element, in units of U: O(1) terms each, formed in
    f64 by autograd and rounded to f32 on the way into the f32 inputs.  (B_mu, B_lv, B_z)."""
    z, mu, lv = z.double(), mu.double(), lv.double()
    N = z.shape[0]
    dl = z - mu
    u = dl * torch.exp(-lv)
    ca, cg = abs(alpha - 1.0) / N, abs(gamma - 1.0) / N
    return ca * u.abs(), ca * 0.5 * (dl.abs() * u.abs() + 1.0), ca * u.abs() + cg * z.abs()
