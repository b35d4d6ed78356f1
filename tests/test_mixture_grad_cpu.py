"""No GPU: the host side of the mixture gradient -- the f64 reference of tests/mixture_grad_ref.py against torch autograd and closed
forms, the derivation of the gate's constant K and the condition that keeps the gate from being vacuous, the C ABI declarations /
bindings of mmvae_posterior_mixture_bwd, and every argument error that the C entry point, posterior_mixture(differentiable=True) and
latent_penalty refuse before anything is launched."""
import importlib
import inspect
import math
import os
import re

import pytest
import torch

from mixture_grad_ref import (F, K, PATTERNS, U, autograd_ref, case_grad_ref, grad_ref, penalty_ref, penalty_upstream, ratios,
                              restatement_f32, upstream)
from mixture_ref import CASES, case_inputs, decomposition_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -4


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


# ================================================================ the reference
@pytest.mark.parametrize("name", ["ragged_67x130", "one_chunk", "257x257x2"])
def test_reference_against_torch_autograd(name):
    z, mu, lv, _ = case_inputs(name)
    for pattern in ("random", "joint", "dims"):
        gj, gd = upstream(name, pattern)
        ref = case_grad_ref(name, pattern)
        for got, key in zip(autograd_ref(z, mu, lv, gj, gd), ("d_z", "d_mu", "d_lv")):
            assert (got - ref[key]).abs().max() <= 1e-13 * ref[key].abs().max(), (pattern, key)


def test_single_posterior_closed_form():
    """M = 1: r = rd = 1, so a_id = g_joint[i] + g_dims[i][d]."""
    g = torch.Generator().manual_seed(4)
    z, mu, lv = torch.randn((9, 6), generator=g), torch.randn((1, 6), generator=g), torch.randn((1, 6), generator=g)
    gj, gd = torch.randn(9, generator=g, dtype=torch.float64), torch.randn((9, 6), generator=g, dtype=torch.float64)
    ref = grad_ref(z, mu, lv, gj, gd)
    a = gj[:, None] + gd
    dl = z.double() - mu.double()
    u = dl * torch.exp(-lv.double())
    for key, want in (("d_z", -a * u), ("d_mu", (a * u).sum(0, keepdim=True)), ("d_lv", (a * 0.5 * (dl * u - 1)).sum(0, keepdim=True))):
        assert (ref[key] - want).abs().max() <= 1e-13 * want.abs().max(), key


@pytest.mark.parametrize("M", [7, 300])
def test_identical_bank_divides_the_single_posterior_gradients_over_the_rows(M):
    g = torch.Generator().manual_seed(M)
    N, d = 11, 5
    m, lv = torch.randn((1, d), generator=g), torch.rand((1, d), generator=g) * 4 - 3
    z = m + torch.exp(0.5 * lv) * torch.randn((N, d), generator=g)
    gj, gd = torch.randn(N, generator=g, dtype=torch.float64), torch.randn((N, d), generator=g, dtype=torch.float64)
    one = grad_ref(z, m, lv, gj, gd)
    many = grad_ref(z, m.expand(M, d).contiguous(), lv.expand(M, d).contiguous(), gj, gd)
    assert (many["d_z"] - one["d_z"]).abs().max() <= 1e-12 * one["d_z"].abs().max()
    for key in ("d_mu", "d_lv"):
        assert (many[key] - one[key] / M).abs().max() <= 1e-12 * one[key].abs().max() / M, key


# ================================================================ the gate
def test_gate_constant_follows_from_the_f32_restatement_and_the_gate_is_not_vacuous():
    """K = 2 x (largest ratio of the plain f32 restatement over the 10 cases x 4 upstream patterns), rounded up to a power of two: the
    restatement must stay within K / 2, and K / 4 must not already hold it (else the power of two below would be the rule's answer).
    Non-vacuity: on every pair that carries weight U * E stays below 2^-10, so am(E) is within 0.1 % of 4 + E wherever a summand counts."""
    worst, where, ue = 0.0, None, 0.0
    for name in CASES:
        z, mu, lv, _ = case_inputs(name)
        for pattern in PATTERNS:
            ref = case_grad_ref(name, pattern)
            for key in ("d_z", "d_mu", "d_lv", "B_z", "B_mu", "B_lv"):
                assert torch.isfinite(ref[key]).all(), (name, pattern, key)
            r = ratios(restatement_f32(z, mu, lv, *upstream(name, pattern)), ref)
            top = max(r, key=r.get)
            if r[top] > worst:
                worst, where = r[top], (name, pattern, top)
            ue = max(ue, ref["ue_max"])
    print(f"f32 restatement: largest error / (2^-24 B) = {worst:.3f} at {where}; largest U * E on a pair that carries weight = {ue:.3e}")
    assert K / 4 < worst <= K / 2
    assert K == 2.0 ** math.ceil(math.log2(2.0 * worst))
    assert ue < 2.0 ** -10
    assert F == 2.0 ** -100 and U == 2.0 ** -24


def test_extreme_case_is_finite_in_the_reference():
    for pattern in PATTERNS:
        ref = case_grad_ref("extreme", pattern)
        assert all(torch.isfinite(ref[k]).all() for k in ("d_z", "d_mu", "d_lv"))


# ================================================================ C ABI
def test_header_declares_and_binding_binds_the_entry_points(pkg):
    L = _L()
    txt = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    assert re.search(r"MMVAE_API\s+size_t\s+mmvae_posterior_mixture_bwd_scratch_bytes\s*\(", txt)
    assert re.search(r"MMVAE_API\s+int\s+mmvae_posterior_mixture_bwd\s*\(", txt)
    for name, nargs in (("mmvae_posterior_mixture_bwd_scratch_bytes", 3), ("mmvae_posterior_mixture_bwd", 16)):
        assert len(L.PROTOTYPES[name][1]) == nargs
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1]
    assert L.lib().mmvae_abi_version() == 3 and "#define MMVAE_ABI_VERSION 3" in txt
    assert L.MIXTURE_BWD_MAX_N == 16384
    assert "posterior_mixture_bwd.hip" in open(os.path.join(ROOT, "moving-mnist-vae_amd", "csrc", "Makefile")).read()
    contract = txt[txt.index("The gradient of both outputs"):txt.index("mmvae_posterior_mixture_bwd_scratch_bytes(int")]
    for word in ("no atomics", "f64", "Capturable", "written", "16384", "unspecified"):
        assert word in contract, word


A = 0x1000                                                                      # a made-up device address, never dereferenced


def _rc(N=5, M=7, d=8, scratch_bytes=None, **ptrs):
    lib = _L().lib()
    p = dict(z=A, mu=A, logvar=A, log_qz=A, log_qz_dims=A, g_joint=A, g_dims=A, d_z=A, d_mu=A, d_logvar=A, scratch=A)
    p.update(ptrs)
    if scratch_bytes is None:
        scratch_bytes = lib.mmvae_posterior_mixture_bwd_scratch_bytes(N, M, d) or (1 << 20)
    rc = lib.mmvae_posterior_mixture_bwd(p["z"], N, p["mu"], p["logvar"], M, d, p["log_qz"], p["log_qz_dims"], p["g_joint"], p["g_dims"],
                                         p["d_z"], p["d_mu"], p["d_logvar"], p["scratch"], scratch_bytes, None)
    return rc, (lib.mmvae_last_error() or b"").decode()


def test_backward_refuses_bad_arguments_before_any_launch(pkg):
    big = _L().MIXTURE_BWD_MAX_N + 1
    for kw in ({"d": 513}, {"N": big}, {"M": big}):
        rc, msg = _rc(**kw)
        assert rc == ERR_UNSUPPORTED and "%s=%d" % next(iter(kw.items())) in msg, kw
    for kw in ({"d": 0}, {"d": -8}, {"N": 0}, {"N": -1}, {"M": 0}, {"M": -3}):
        rc, msg = _rc(**kw)
        assert rc == ERR_ARG and "%s=%d" % next(iter(kw.items())) in msg, kw
    for null in ("z", "mu", "logvar", "log_qz", "d_z", "d_mu", "d_logvar", "scratch"):
        rc, msg = _rc(**{null: None})
        assert rc == ERR_ARG and null in msg, null
    rc, msg = _rc(g_joint=None, g_dims=None)
    assert rc == ERR_ARG and "both NULL" in msg
    rc, msg = _rc(log_qz_dims=None)                                              # g_dims without log_qz_dims
    assert rc == ERR_ARG and "log_qz_dims" in msg
    assert _rc(scratch=A + 8)[0] == ERR_ARG                                      # 16-byte alignment
    need = _L().lib().mmvae_posterior_mixture_bwd_scratch_bytes(5, 7, 8)
    rc, msg = _rc(scratch_bytes=need - 1)
    assert rc == ERR_ARG and "scratch_bytes" in msg
    assert _rc(scratch_bytes=0)[0] == ERR_ARG


def test_scratch_bytes_is_a_function_of_the_shape(pkg):
    fn = _L().lib().mmvae_posterior_mixture_bwd_scratch_bytes
    assert fn(5, 7, 8) == fn(5, 7, 8) > 0 and fn(5, 7, 8) % 16 == 0
    for bad in ((0, 7, 8), (5, 0, 8), (5, 7, 0), (5, 7, 513), (16385, 7, 8), (5, 16385, 8), (-1, -1, -1)):
        assert fn(*bad) == 0, bad
    assert fn(16384, 16384, 512) > (1 << 29)                                     # the top of the range: sizes are 64-bit
    assert fn(64, 1000, 64) >= fn(64, 500, 64) and fn(64, 1000, 64) >= fn(64, 1000, 32)
    assert fn(5120, 5120, 64) < (1 << 28)                                        # a training batch: well under 256 MiB


# ================================================================ Python surface
def test_differentiable_mixture_refuses_before_any_launch(pkg):
    z, mu, lv = torch.zeros(4, 8), torch.zeros(6, 8), torch.zeros(6, 8)
    kw = dict(differentiable=True)
    with pytest.raises(ValueError, match="GPU"):
        pkg.posterior_mixture(z, mu, lv, **kw)
    with pytest.raises(ValueError, match="width"):
        pkg.posterior_mixture(torch.zeros(4, 9), mu, lv, **kw)
    with pytest.raises(ValueError, match="differ in shape"):
        pkg.posterior_mixture(z, mu, torch.zeros(5, 8), **kw)
    with pytest.raises(ValueError, match="unsupported"):
        pkg.posterior_mixture(torch.zeros(2, 513), torch.zeros(3, 513), torch.zeros(3, 513), **kw)
    with pytest.raises(ValueError, match="shape"):
        pkg.posterior_mixture(torch.zeros(4, 8, 2, 1), mu, lv, **kw)
    with pytest.raises(ValueError, match="tensor"):
        pkg.posterior_mixture(None, mu, lv, **kw)
    # the backward's limit, in the forward: a shape the plain call takes (<= 2^20) is refused here
    wide = torch.zeros(16385, 1)
    with pytest.raises(ValueError, match="at most 16384"):
        pkg.posterior_mixture(wide, mu[:, :1], lv[:, :1], **kw)
    with pytest.raises(ValueError, match="at most 16384"):
        pkg.posterior_mixture(z[:, :1], wide, wide, **kw)
    with pytest.raises(ValueError, match="GPU"):                                 # ... and the plain call gets as far as the device check
        pkg.posterior_mixture(wide, mu[:, :1], lv[:, :1])


def test_latent_penalty_refuses_before_any_launch(pkg):
    mu, lv, enc = torch.zeros(6, 8), torch.zeros(6, 8), torch.zeros(6, 8)
    with pytest.raises(ValueError, match="GPU"):
        pkg.latent_penalty(mu, lv, enc, beta=6)
    with pytest.raises(ValueError, match="posterior i"):
        pkg.latent_penalty(mu, lv, torch.zeros(4, 8), beta=6)
    with pytest.raises(ValueError, match="width"):
        pkg.latent_penalty(mu, lv, torch.zeros(6, 4), beta=6)
    with pytest.raises(ValueError, match="tensor"):
        pkg.latent_penalty(mu, None, enc, beta=6)
    with pytest.raises(ValueError, match="at most 16384"):
        pkg.latent_penalty(torch.zeros(16385, 1), torch.zeros(16385, 1), torch.zeros(16385, 1), beta=6)
    for bad in (dict(alpha=float("nan")), dict(beta=float("inf")), dict(gamma="2"), dict(beta=None), dict(alpha=True)):
        with pytest.raises(ValueError, match="finite number"):
            pkg.latent_penalty(mu, lv, enc, **bad)
        with pytest.raises(ValueError, match="finite number"):
            pkg.make_latent_penalty(**bad)
    for bad in (0, -5, 2.5, True):
        with pytest.raises(ValueError, match="dataset_size"):
            pkg.latent_penalty(mu, lv, enc, beta=6, dataset_size=bad)
        with pytest.raises(ValueError, match="dataset_size"):
            pkg.make_latent_penalty(beta=6, dataset_size=bad)


def test_unit_coefficients_are_an_exact_zero_without_a_library_call(pkg, monkeypatch):
    L = _L()
    calls = []
    monkeypatch.setattr(L, "call", lambda *a, **k: calls.append(a))
    monkeypatch.setattr(L, "lib", lambda: calls.append("lib"))
    dec = importlib.import_module("moving-mnist-vae_amd.decomposition")
    seen = []
    monkeypatch.setattr(dec, "_checked", lambda *a, **k: seen.append(a))         # (the device check: these tensors live on the CPU)
    mu = torch.zeros(6, 8, requires_grad=True)
    penalty, terms = pkg.latent_penalty(mu, torch.zeros(6, 8), torch.zeros(6, 8), 1, 1.0, 1)
    assert seen and not calls
    assert penalty.dtype == torch.float64 and penalty.dim() == 0 and penalty.item() == 0.0 and not penalty.requires_grad
    assert sorted(terms) == ["dwkl", "mi", "tc"] and all(t.dtype == torch.float64 and t.dim() == 0 and math.isnan(t.item()) for t in terms.values())
    hook = pkg.make_latent_penalty()
    assert hook(mu, torch.zeros(6, 8), torch.zeros(6, 8)).item() == 0.0 and not calls
    rows = hook.to_host()
    assert rows.shape == (1, 4) and rows[0][0] == 0.0 and hook.to_host().shape == (0, 4)


def test_dataset_size_constants_and_the_implied_upstream_gradients():
    """The reference composition: minibatch weighted sampling shifts mi by log D, tc by (z - 1) log D, dwkl by -z log D and no gradient;
    beta alone sends (beta - 1) / N into log_qz and -(beta - 1) / N into every log_qz_dims."""
    z, mu, lv, _ = case_inputs("257x257x2")
    N, d = z.shape
    coef = dict(alpha=2.0, beta=6.0, gamma=0.5)
    p0, t0, g0 = penalty_ref(mu, lv, z, **coef)
    p1, t1, g1 = penalty_ref(mu, lv, z, **coef, dataset_size=60000)
    log_d = math.log(60000)
    for k, shift in (("mi", log_d), ("tc", (d - 1) * log_d), ("dwkl", -d * log_d)):
        assert abs((t1[k] - t0[k]).item() - shift) <= 1e-12 * abs(shift)
    assert abs((p1 - p0).item() - (1.0 * log_d + 5.0 * (d - 1) * log_d + 0.5 * d * log_d)) <= 1e-12 * abs(p1.item())
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))
    want = decomposition_ref(mu, lv, z)
    for k in ("mi", "tc", "dwkl"):
        assert abs((t0[k] - want[k]).item()) <= 1e-12 * max(abs(want[k].item()), 1.0)
    gj, gd = penalty_upstream(N, d, beta=6.0)
    assert gj[0].item() == 5.0 / N and gd[0, 0].item() == -5.0 / N
    _, _, (r_mu, r_lv, r_z) = penalty_ref(mu, lv, z, beta=6.0)
    ref = grad_ref(z, mu, lv, gj, gd)
    for got, key in ((r_z, "d_z"), (r_mu, "d_mu"), (r_lv, "d_lv")):
        assert (got - ref[key]).abs().max() <= 1e-12 * ref[key].abs().max(), key


def test_new_names_are_exported_and_documented(pkg):
    dec = importlib.import_module("moving-mnist-vae_amd.decomposition")
    main = importlib.import_module("moving-mnist-vae_amd.main")
    for name in ("latent_penalty", "make_latent_penalty"):
        assert getattr(pkg, name) is getattr(dec, name) is getattr(main, name)
    assert inspect.signature(pkg.posterior_mixture).parameters["differentiable"].default is False
    sig = inspect.signature(pkg.latent_penalty).parameters
    assert [sig[k].default for k in ("alpha", "beta", "gamma", "dataset_size")] == [1.0, 1.0, 1.0, None]
    hook = pkg.make_latent_penalty(beta=6, dataset_size=60000)
    assert (hook.alpha, hook.beta, hook.gamma, hook.dataset_size) == (1.0, 6, 1.0, 60000) and callable(hook)
    doc = pkg.latent_penalty.__doc__
    assert "log M" in doc and "saturated" in doc.lower() and "one sample per image" in doc
    assert "rank's own batch" in pkg.make_latent_penalty.__doc__
    assert "latent_penalty" in inspect.getsource(main.train)
