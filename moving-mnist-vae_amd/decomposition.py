"""ELBO surgery on the device: what the KL term of a trained model is made of.

``E_x KL(q(z|x) || p(z)) = I_q(x; z) + KL(q(z) || p(z))`` (Hoffman & Johnson 2016), and the second term splits further into total
correlation and dimension-wise KL (Chen et al. 2018).  Two runs of the ``normal_vae_<kl>_kl_<mmd>_mmd`` sweep can print the same
average KL and differ completely in this split: a collapsed code against an informative code with a matched marginal.  The estimator
needs ``log q(z_i) = logsumexp_j log q(z_i | x_j) - log M`` over the whole held-out set -- every (sample, posterior) pair in every
dimension.  ``posterior_mixture`` is that sweep (``mmvae_posterior_mixture``: terms in f32, sums of exponentials in f64, f64 outputs,
fixed order); ``elbo_decomposition`` turns its outputs into the split by f64 tensor operations, no host read;
``evaluate(..., decomposition=True)`` runs it over a data loader.

Training against the split (Chen et al. 2018, beta-TCVAE): ``posterior_mixture(..., differentiable=True)`` carries a gradient
(``mmvae_posterior_mixture_bwd``: two pair sweeps, f64 sums, fixed order), ``latent_penalty`` is the minibatch estimate of
``(alpha - 1) MI + (beta - 1) TC + (gamma - 1) DWKL`` built on it, and ``make_latent_penalty`` returns the callable that ``train`` adds
to the loss when ``args.latent_penalty`` holds it.
"""
import math

import torch

from . import _lib as L

_LOG_2PI = math.log(2.0 * math.pi)
_SCRATCH = {}                          # (device, bytes) -> uint8 device tensor, kept for the life of the process


def _rows(t, what, name):
    """Shape check of one (rows, z) or (rows, z, 1, 1) argument, nothing launched: returns (rows, z)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if not (t.dim() == 2 or (t.dim() == 4 and tuple(t.shape[2:]) == (1, 1))) or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: {name} must have shape (rows, z) or (rows, z, 1, 1) with rows, z >= 1, got {tuple(t.shape)}")
    return int(t.shape[0]), int(t.shape[1])


def _checked(z, mu, logvar, what, max_n=None):
    """Every check of ``posterior_mixture`` before anything is launched; returns the three as contiguous f32 (rows, z) tensors.
    ``max_n``: the row limit (default: the forward's; the differentiable form passes the backward's)."""
    max_n = L.MIXTURE_MAX_N if max_n is None else max_n
    (N, d), (M, dm), (Ml, dl) = _rows(z, what, "z"), _rows(mu, what, "mu"), _rows(logvar, what, "logvar")
    if (M, dm) != (Ml, dl):
        raise ValueError(f"{what}: mu {tuple(mu.shape)} and logvar {tuple(logvar.shape)} differ in shape")
    if d != dm:
        raise ValueError(f"{what}: samples of width {d} against a bank of width {dm}")
    if d > L.MIXTURE_MAX_D:
        raise ValueError(f"{what}: z={d} unsupported (1..{L.MIXTURE_MAX_D})")
    if N > max_n or M > max_n:
        raise ValueError(f"{what}: {N} samples against {M} posteriors unsupported (at most {max_n} of either)")
    if not (z.is_cuda and z.device == mu.device == logvar.device):
        raise ValueError(f"{what} expects z, mu and logvar on one GPU (they are on {z.device}, {mu.device}, {logvar.device})")
    return tuple(t.detach().reshape(t.shape[0], d).float().contiguous() for t in (z, mu, logvar))


def _scratch(device, nbytes):
    key = (device, nbytes)
    buf = _SCRATCH.get(key)
    if buf is None:
        buf = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return buf


def _mixture(z, mu, logvar, per_dim):
    (N, d), M, dev = z.shape, mu.shape[0], z.device
    nbytes = L.lib().mmvae_posterior_mixture_scratch_bytes(N, M, d)
    scratch = _scratch(dev, nbytes)
    log_qz = torch.empty(N, dtype=torch.float64, device=dev)
    dims = torch.empty((N, d), dtype=torch.float64, device=dev) if per_dim else None
    L.call("mmvae_posterior_mixture", dev, L.ptr(z), N, L.ptr(mu), L.ptr(logvar), M, d, L.ptr(log_qz), L.ptr(dims), L.ptr(scratch), nbytes)
    return log_qz, dims


class _MixtureFn(torch.autograd.Function):
    """posterior_mixture with a gradient: the forward is the library call on detached f32 copies, the backward ONE call of
    mmvae_posterior_mixture_bwd; gradients go back in each input's own shape and dtype."""

    @staticmethod
    def forward(ctx, z, mu, logvar, per_dim):
        z32, mu32, lv32 = (t.detach().reshape(t.shape[0], t.shape[1]).float().contiguous() for t in (z, mu, logvar))
        log_qz, dims = _mixture(z32, mu32, lv32, per_dim)
        ctx.like = tuple((t.shape, t.dtype) for t in (z, mu, logvar))
        ctx.set_materialize_grads(False)                      # an output that nothing consumed arrives as None, and goes on as NULL
        ctx.save_for_backward(z32, mu32, lv32, log_qz, dims)
        if not per_dim:
            return log_qz
        return log_qz, dims

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_joint, g_dims=None):
        z, mu, lv, log_qz, dims = ctx.saved_tensors
        if g_joint is None and g_dims is None:
            return None, None, None, None
        (N, d), M, dev = z.shape, mu.shape[0], z.device
        g_joint = None if g_joint is None else g_joint.double().contiguous()
        g_dims = None if g_dims is None else g_dims.double().contiguous()
        nbytes = L.lib().mmvae_posterior_mixture_bwd_scratch_bytes(N, M, d)
        scratch = _scratch(dev, nbytes)
        d_z, d_mu, d_lv = torch.empty_like(z), torch.empty_like(mu), torch.empty_like(lv)
        L.call("mmvae_posterior_mixture_bwd", dev, L.ptr(z), N, L.ptr(mu), L.ptr(lv), M, d, L.ptr(log_qz), L.ptr(dims if g_dims is not None else None),
               L.ptr(g_joint), L.ptr(g_dims), L.ptr(d_z), L.ptr(d_mu), L.ptr(d_lv), L.ptr(scratch), nbytes)
        grads = tuple(g.reshape(shape).to(dtype) if need else None
                      for g, (shape, dtype), need in zip((d_z, d_mu, d_lv), ctx.like, ctx.needs_input_grad[:3]))
        return grads + (None,)


def posterior_mixture(z, mu, logvar, per_dim=True, differentiable=False):
    """The aggregate posterior at every sample, on the device (mmvae_posterior_mixture).  ``z``: N samples, ``mu`` / ``logvar``: the
    bank of M diagonal Gaussian posteriors, each (rows, z) or (rows, z, 1, 1) as ``model(image)`` returns them (made f32 and contiguous
    if they are not).  Returns ``(log_qz, log_qz_dims)``, float64 device tensors of shape (N,) and (N, z):
    ``log_qz[i] = logsumexp_j log q(z_i | x_j) - log M`` and ``log_qz_dims[i][d]`` the same for the d-th marginal alone
    (``per_dim=False`` skips that work and returns None for it; ``log_qz`` has the same bits either way).  The Gaussian terms are formed
    in f32 and the maximum is subtracted before any exponential; sums of exponentials are f64; fixed order, no atomics: the same bits
    every run.  No host read, no synchronisation, capturable in a graph.  The scratch buffer is cached per device and size and shared by
    the calls on that device, which must therefore be issued on one stream.  z <= 512, N, M <= 2^20; values are specified for
    ``|z|, |mu| <= 1e4`` and ``|logvar| <= 30``.  Everything is checked before anything is launched (ValueError).

    ``differentiable=True``: the same values, carrying a ``grad_fn`` -- gradients with respect to ``z``, ``mu`` and ``logvar`` come from
    ONE call of ``mmvae_posterior_mixture_bwd`` (terms in f32, every sum longer than 8 terms in f64, fixed order, no atomics; include/mmvae.h
    states the formulas) and arrive in each input's own shape and dtype.  An output that nothing consumed costs nothing there
    (``per_dim=False`` never sweeps the marginals).  The backward takes at most 16384 samples and 16384 posteriors -- training batches --
    and that limit is checked here, in the forward, so that no graph is built that cannot be differentiated.  No double backward."""
    if not differentiable:
        z, mu, logvar = _checked(z, mu, logvar, "posterior_mixture")
        return _mixture(z, mu, logvar, bool(per_dim))
    _checked(z, mu, logvar, "posterior_mixture(differentiable=True)", L.MIXTURE_BWD_MAX_N)
    if not per_dim:
        return _MixtureFn.apply(z, mu, logvar, False), None
    return _MixtureFn.apply(z, mu, logvar, True)


def _decompose(mu, logvar, encoding, index, what):
    """elbo_decomposition and the per-sample log q(z) it came from: (dict, log_qz)."""
    if index is not None:
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1:
            raise ValueError(f"{what}: index must be a 1-D int64 tensor")
        if isinstance(encoding, torch.Tensor) and index.numel() != encoding.shape[0]:
            raise ValueError(f"{what}: {index.numel()} indices for {encoding.shape[0]} samples")
    z, mu, logvar = _checked(encoding, mu, logvar, what)
    (N, d), M, dev = z.shape, mu.shape[0], z.device
    if index is None and N != M:
        raise ValueError(f"{what}: {N} samples against {M} posteriors need an index (sample i is drawn from posterior index[i])")
    log_qz, dims = _mixture(z, mu, logvar, True)
    z64, mu64, lv64 = z.double(), mu.double(), logvar.double()
    if index is not None:
        index = index.to(dev)
        mu64, lv64 = mu64.index_select(0, index), lv64.index_select(0, index)
    dz = z64 - mu64
    own = (-0.5 * (dz * dz * torch.exp(-lv64) + lv64 + _LOG_2PI)).sum(1)          # log q(z_i | x_index[i])
    pz_dims = -0.5 * (z64 * z64 + _LOG_2PI)                                       # log p(z_id)
    pz = pz_dims.sum(1)
    indep = dims.sum(1)
    tc, dwkl = (log_qz - indep).mean(), (indep - pz).mean()
    out = {"mi": (own - log_qz).mean(), "tc": tc, "dwkl": dwkl, "marginal_kl": tc + dwkl, "kl_sampled": (own - pz).mean(),
           "kl_analytic": (0.5 * (torch.exp(lv64) + mu64 * mu64 - lv64 - 1.0)).sum(1).mean(),
           "dwkl_per_dim": (dims - pz_dims).mean(0),
           "log_m": torch.full((), math.log(M), dtype=torch.float64, device=dev), "n": N, "m": M}
    return out, log_qz


def elbo_decomposition(mu, logvar, encoding, index=None):
    """The split of the averaged KL term, estimated on a held-out set: ``mu`` / ``logvar`` are the posteriors of M images (the bank),
    ``encoding[i]`` is ONE sample of posterior ``index[i]``.  ``index=None`` means ``arange`` and needs N == M (every image's own
    sample, what ``evaluate`` keeps); an int64 ``index`` of N entries in [0, M) scores a subset of samples against the full bank (its
    values are not checked: that would be a host read).  One ``posterior_mixture`` call, then f64 tensor operations, no host read.  With
    ``own_i = log q(z_i | x_index[i])`` and ``pz_i = log p(z_i)`` (both formed in f64 from the f32 inputs) and
    ``indep_i = sum_d log_qz_dims[i][d]``, returns 0-dim float64 device tensors

      ``mi``            mean_i (own_i - log_qz[i])           I_q(x; z), the index-code mutual information
      ``tc``            mean_i (log_qz[i] - indep_i)         total correlation of q(z)
      ``dwkl``          mean_i (indep_i - pz_i)              dimension-wise KL, sum_d KL(q(z_d) || p(z_d))
      ``marginal_kl``   tc + dwkl                            KL(q(z) || p(z))
      ``kl_sampled``    mean_i (own_i - pz_i)                the same samples' estimate of the averaged KL: mi + marginal_kl up to f64 rounding
      ``kl_analytic``   the mean closed-form KL of the sampled posteriors (what ``kl_sampled`` estimates)
      ``log_m``         log M

    plus ``dwkl_per_dim`` (float64, (z,): each dimension's share of ``dwkl``), the counts ``n``, ``m`` (ints) and ``log_qz`` (float64,
    (N,): the per-sample densities the means were taken over).

    Known limits of the estimator.  ``mi <= log M`` by construction: the sample's own posterior is one of the M in the bank, so
    ``log_qz[i] >= own_i - log M``; a value near ``log_m`` means SATURATED (every sample is attributable to its own image among these
    M), not measured -- the true mutual information may be far larger, and only a larger held-out set can tell.  All figures are
    Monte-Carlo estimates from one sample per image; ``kl_sampled - kl_analytic`` shows the size of that noise.  ``log_qz`` averages
    over the M held-out posteriors only, which biases ``marginal_kl`` upwards for small M."""
    out, log_qz = _decompose(mu, logvar, encoding, index, "elbo_decomposition")
    out["log_qz"] = log_qz
    return out


_SCALARS = ("mi", "tc", "dwkl", "marginal_kl", "kl_sampled", "kl_analytic", "log_m")


def decomposition_to_host(dec):
    """The dict of ``elbo_decomposition`` as Python floats and a numpy array, in ONE device-to-host copy."""
    flat = torch.cat([torch.stack([dec[k] for k in _SCALARS]), dec["dwkl_per_dim"]]).cpu().numpy()
    out = {k: float(flat[i]) for i, k in enumerate(_SCALARS)}
    out.update(dwkl_per_dim=flat[len(_SCALARS):].copy(), n=dec["n"], m=dec["m"])
    return out


# ---------------------------------------------------------------------------------------------- training against the split
def _coefficient(v, name, what):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{what}: {name} must be a finite number, got {v!r}")
    return float(v)


def _penalty_args(alpha, beta, gamma, dataset_size, what):
    coef = tuple(_coefficient(v, n, what) for v, n in ((alpha, "alpha"), (beta, "beta"), (gamma, "gamma")))
    if dataset_size is not None and (isinstance(dataset_size, bool) or not isinstance(dataset_size, int) or dataset_size < 1):
        raise ValueError(f"{what}: dataset_size must be None or a positive int, got {dataset_size!r}")
    return coef


def latent_penalty(mu, logvar, encoding, alpha=1.0, beta=1.0, gamma=1.0, dataset_size=None):
    """The beta-TCVAE penalty of Chen et al. 2018 on one minibatch, differentiable: ``mu`` / ``logvar`` / ``encoding`` are what
    ``model(image)`` returns, N posteriors and ONE sample of each (sample i drawn from posterior i, so N == M), each (N, z) or
    (N, z, 1, 1).  Returns ``(penalty, terms)``: ``terms = {'mi', 'tc', 'dwkl'}``, 0-dim float64 device tensors by exactly the formulas of
    ``elbo_decomposition`` with the minibatch as the bank, and

      ``penalty = (alpha - 1) * mi + (beta - 1) * tc + (gamma - 1) * dwkl``

    -- the amount that turns a loss holding ``1 * KL`` per image into ``alpha MI + beta TC + gamma DWKL``, up to the estimator's own
    noise (the loss's KL is analytic, ``mi + tc + dwkl`` is its one-sample estimate).  The own density and the prior are f64 tensor
    operations that autograd differentiates itself; only the mixture goes through ``posterior_mixture(differentiable=True)``.  A
    coefficient equal to 1 contributes no gradient work: its term is reported detached, ``alpha`` alone never sweeps the marginals (``tc``
    and ``dwkl`` are then NaN, not computed), and ``alpha = beta = gamma = 1`` returns an exact zero (and NaN terms) without a library call.

    ``dataset_size=None`` is the plain minibatch estimate: on the same tensors ``terms['tc']`` has the bits of
    ``elbo_decomposition(...)['tc']``.  An integer ``dataset_size`` D applies the constants of minibatch weighted sampling
    (``log q(z) ~ logsumexp_j - log(N D)``): ``mi + log D``, ``tc + (z - 1) log D``, ``dwkl - z log D``; they change values only, never
    gradients.

    Known limits, as for ``elbo_decomposition``: ``mi <= log M`` by construction (with ``dataset_size``: ``log M + log D``), so a value
    near it means saturated, not measured; every figure is a Monte-Carlo estimate from one sample per image, over the N posteriors of
    this batch only.  N <= 16384, z <= 512.  Everything is checked before anything is launched (ValueError)."""
    what = "latent_penalty"
    a, b, c = _penalty_args(alpha, beta, gamma, dataset_size, what)
    (N, d), (M, _) = _rows(encoding, what, "encoding"), _rows(mu, what, "mu")
    if N != M:
        raise ValueError(f"{what}: {N} samples against {M} posteriors (sample i must be drawn from posterior i)")
    _checked(encoding, mu, logvar, what, L.MIXTURE_BWD_MAX_N)
    dev = encoding.device
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    if a == 1.0 and b == 1.0 and c == 1.0:
        return torch.zeros((), dtype=torch.float64, device=dev), {"mi": nan, "tc": nan, "dwkl": nan}
    per_dim = b != 1.0 or c != 1.0
    log_qz, dims = posterior_mixture(encoding, mu, logvar, per_dim=per_dim, differentiable=True)
    z64, mu64, lv64 = (t.reshape(N, d).double() for t in (encoding, mu, logvar))
    if a == 1.0:
        z_mi, mu64, lv64, q_mi = z64.detach(), mu64.detach(), lv64.detach(), log_qz.detach()
    else:
        z_mi, q_mi = z64, log_qz
    dz = z_mi - mu64
    own = (-0.5 * (dz * dz * torch.exp(-lv64) + lv64 + _LOG_2PI)).sum(1)              # log q(z_i | x_i)
    terms = {"mi": (own - q_mi).mean(), "tc": nan, "dwkl": nan}
    if per_dim:
        indep = dims.sum(1)
        z_kl, i_kl = (z64.detach(), indep.detach()) if c == 1.0 else (z64, indep)
        pz = (-0.5 * (z_kl * z_kl + _LOG_2PI)).sum(1)                                 # log p(z_i)
        terms["tc"] = ((log_qz - indep) if b != 1.0 else (log_qz.detach() - indep.detach())).mean()
        terms["dwkl"] = (i_kl - pz).mean()
    if dataset_size is not None:
        log_d = math.log(dataset_size)
        terms = {"mi": terms["mi"] + log_d, "tc": terms["tc"] + (d - 1) * log_d, "dwkl": terms["dwkl"] - d * log_d}
    penalty = None
    for coef, key in ((a, "mi"), (b, "tc"), (c, "dwkl")):
        if coef != 1.0:
            part = (coef - 1.0) * terms[key]
            penalty = part if penalty is None else penalty + part
    return penalty, terms


class LatentPenalty:
    """What ``make_latent_penalty`` returns: ``self(mu, logvar, encoding)`` is ``latent_penalty``'s penalty with this object's
    coefficients, plain attributes (``alpha``, ``beta``, ``gamma``, ``dataset_size``) that a schedule may set per epoch.  Each call's
    ``(penalty, mi, tc, dwkl)`` stays on the device; ``to_host()`` hands all of them over as a float64 numpy array of shape (calls, 4) in
    ONE device-to-host copy and resets (an empty (0, 4) array when nothing was recorded)."""

    def __init__(self, alpha=1.0, beta=1.0, gamma=1.0, dataset_size=None):
        _penalty_args(alpha, beta, gamma, dataset_size, "make_latent_penalty")
        self.alpha, self.beta, self.gamma, self.dataset_size = alpha, beta, gamma, dataset_size
        self._rows = []

    def __call__(self, mu, logvar, encoding):
        penalty, terms = latent_penalty(mu, logvar, encoding, self.alpha, self.beta, self.gamma, self.dataset_size)
        self._rows.append(torch.stack([penalty.detach(), terms["mi"].detach(), terms["tc"].detach(), terms["dwkl"].detach()]))
        return penalty

    def to_host(self):
        rows, self._rows = self._rows, []
        if not rows:
            import numpy
            return numpy.zeros((0, 4))
        return torch.stack(rows).cpu().numpy()


def make_latent_penalty(alpha=1.0, beta=1.0, gamma=1.0, dataset_size=None):
    """A callable for ``args.latent_penalty``: ``train`` adds its value to the loss of every step, which turns the loss's ``1 * KL`` into
    ``alpha MI + beta TC + gamma DWKL`` (``latent_penalty``; ``make_latent_penalty(beta=6)`` is beta-TCVAE with beta = 6).  Set
    ``model.kl`` to 1 for that reading.  Under a data-parallel ``GradSync`` the bank is the rank's own batch: nothing is gathered, every
    rank penalises the total correlation of its own N posteriors.  See ``LatentPenalty`` for the per-step record (``to_host()``)."""
    return LatentPenalty(alpha, beta, gamma, dataset_size)
