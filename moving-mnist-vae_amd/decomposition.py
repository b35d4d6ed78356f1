"""ELBO surgery on the device: what the KL term of a trained model is made of.

``E_x KL(q(z|x) || p(z)) = I_q(x; z) + KL(q(z) || p(z))`` (Hoffman & Johnson 2016), and the second term splits further into total
correlation and dimension-wise KL (Chen et al. 2018).  Two runs of the ``normal_vae_<kl>_kl_<mmd>_mmd`` sweep can print the same
average KL and differ completely in this split: a collapsed code against an informative code with a matched marginal.  The estimator
needs ``log q(z_i) = logsumexp_j log q(z_i | x_j) - log M`` over the whole held-out set -- every (sample, posterior) pair in every
dimension.  ``posterior_mixture`` is that sweep (``mmvae_posterior_mixture``: terms in f32, sums of exponentials in f64, f64 outputs,
fixed order); ``elbo_decomposition`` turns its outputs into the split by f64 tensor operations, no host read;
``evaluate(..., decomposition=True)`` runs it over a data loader.
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


def _checked(z, mu, logvar, what):
    """Every check of ``posterior_mixture`` before anything is launched; returns the three as contiguous f32 (rows, z) tensors."""
    (N, d), (M, dm), (Ml, dl) = _rows(z, what, "z"), _rows(mu, what, "mu"), _rows(logvar, what, "logvar")
    if (M, dm) != (Ml, dl):
        raise ValueError(f"{what}: mu {tuple(mu.shape)} and logvar {tuple(logvar.shape)} differ in shape")
    if d != dm:
        raise ValueError(f"{what}: samples of width {d} against a bank of width {dm}")
    if d > L.MIXTURE_MAX_D:
        raise ValueError(f"{what}: z={d} unsupported (1..{L.MIXTURE_MAX_D})")
    if N > L.MIXTURE_MAX_N or M > L.MIXTURE_MAX_N:
        raise ValueError(f"{what}: {N} samples against {M} posteriors unsupported (at most {L.MIXTURE_MAX_N} of either)")
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


def posterior_mixture(z, mu, logvar, per_dim=True):
    """The aggregate posterior at every sample, on the device (mmvae_posterior_mixture).  ``z``: N samples, ``mu`` / ``logvar``: the
    bank of M diagonal Gaussian posteriors, each (rows, z) or (rows, z, 1, 1) as ``model(image)`` returns them (made f32 and contiguous
    if they are not).  Returns ``(log_qz, log_qz_dims)``, float64 device tensors of shape (N,) and (N, z):
    ``log_qz[i] = logsumexp_j log q(z_i | x_j) - log M`` and ``log_qz_dims[i][d]`` the same for the d-th marginal alone
    (``per_dim=False`` skips that work and returns None for it; ``log_qz`` has the same bits either way).  The Gaussian terms are formed
    in f32 and the maximum is subtracted before any exponential; sums of exponentials are f64; fixed order, no atomics: the same bits
    every run.  No host read, no synchronisation, capturable in a graph.  The scratch buffer is cached per device and size and shared by
    the calls on that device, which must therefore be issued on one stream.  z <= 512, N, M <= 2^20; values are specified for
    ``|z|, |mu| <= 1e4`` and ``|logvar| <= 30``.  Everything is checked before anything is launched (ValueError)."""
    z, mu, logvar = _checked(z, mu, logvar, "posterior_mixture")
    return _mixture(z, mu, logvar, bool(per_dim))


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
