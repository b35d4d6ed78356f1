"""No GPU: the host side of the ELBO decomposition -- the f64 reference of tests/mixture_ref.py against closed forms, the identities of
the split and the conditions on the inputs of every case tests/test_decomposition_gpu.py runs, the C ABI declarations / bindings of
mmvae_posterior_mixture, and the argument errors that the C entry points and the Python surface refuse before anything is launched."""
import importlib
import inspect
import math
import os
import re

import pytest
import torch

from mixture_ref import CASES, LOG_2PI, MIN_CHUNK, case_inputs, case_ref, decomposition_ref, mixture_ref, own_density

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -4


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


# ================================================================ the reference against closed forms
@pytest.mark.parametrize("M", [1, 7, 300])
def test_identical_bank_is_that_gaussian(M):
    """A bank of M copies of N(m, s^2): q(z) is that Gaussian whatever M, so log_qz / log_qz_dims are its log-density and there is
    neither mutual information nor total correlation."""
    g = torch.Generator().manual_seed(M)
    N, d = 11, 5
    m, lv = torch.randn(d, generator=g), torch.rand(d, generator=g) * 4 - 3
    mu, logvar = m.expand(M, d).contiguous(), lv.expand(M, d).contiguous()
    z = m + torch.exp(0.5 * lv) * torch.randn((N, d), generator=g)
    r = mixture_ref(z, mu, logvar)
    want = -0.5 * ((z.double() - m.double()) ** 2 * torch.exp(-lv.double()) + lv.double() + LOG_2PI)
    assert (r["log_qz_dims"] - want).abs().max() <= 1e-12 * want.abs().max()
    assert (r["log_qz"] - want.sum(1)).abs().max() <= 1e-12 * want.sum(1).abs().max()
    dec = decomposition_ref(mu, logvar, z, index=torch.arange(N) % M)
    scale = want.sum(1).abs().max().item()
    assert abs(dec["mi"].item()) <= 1e-12 * scale and abs(dec["tc"].item()) <= 1e-12 * scale


def test_single_posterior_gives_the_own_density():
    g = torch.Generator().manual_seed(4)
    z, mu, lv = torch.randn((9, 6), generator=g), torch.randn((1, 6), generator=g), torch.randn((1, 6), generator=g)
    r = mixture_ref(z, mu, lv)
    own = own_density(z, mu.expand(9, 6), lv.expand(9, 6))
    assert (r["log_qz"] - own).abs().max() <= 1e-12 * own.abs().max()
    assert (r["log_qz_dims"].sum(1) - own).abs().max() <= 1e-12 * own.abs().max()


# ================================================================ the cases of the GPU test
@pytest.mark.parametrize("name", list(CASES))
def test_case_inputs_meet_their_conditions(name):
    N, M, d = CASES[name][:3]
    z, mu, lv, index = case_inputs(name)
    assert tuple(z.shape) == (N, d) and tuple(mu.shape) == tuple(lv.shape) == (M, d) and tuple(index.shape) == (N,)
    assert all(t.dtype == torch.float32 for t in (z, mu, lv))
    assert z.abs().max() <= 1e4 and mu.abs().max() <= 1e4 and lv.abs().max() <= 30                 # the documented domain
    if name != "extreme":
        assert lv.min() >= -12 and lv.max() <= 4
    r = case_ref(name)
    for k in ("log_qz", "log_qz_dims", "B", "B_dims"):
        assert torch.isfinite(r[k]).all(), k
    assert (r["B"] >= 1).all() and (r["B_dims"] >= 1).all()
    assert (r["top_weight"] > 1e-3).all()                  # every sample has at least one bank row that counts


def test_case_table_reaches_the_edges():
    L = _L()
    assert MIN_CHUNK == L.MIXTURE_MIN_CHUNK
    N, M, d = CASES["chunk_edges"][:3]
    assert N <= 64 and M > 2 * MIN_CHUNK and M % MIN_CHUNK != 0                                      # > two chunks and a remainder
    assert CASES["one_chunk"][1] <= MIN_CHUNK
    assert CASES["widest_d512"][2] == L.MIXTURE_MAX_D and CASES["three_tiles_d130"][2] > 4 * 32
    z, mu, lv, index = case_inputs("extreme")
    assert (lv == 30).any() and (lv == -30).any()
    far = (z[:, None, :] - mu[None]).abs().amax(2)
    assert (far.max(1).values >= 9.9e3).all()                                                       # every sample is ~1e4 from some row


@pytest.mark.parametrize("name", list(CASES))
def test_split_identities(name):
    z, mu, lv, index = case_inputs(name)
    r = case_ref(name)
    dec = decomposition_ref(mu, lv, z, index, r["log_qz"], r["log_qz_dims"])
    total = dec["mi"] + dec["tc"] + dec["dwkl"]
    # every mean is a sum of N f64 terms of the magnitudes below: 1e-12 of them
    mag = own_density(z, mu[index], lv[index]).abs().mean() + r["log_qz"].abs().mean() + r["log_qz_dims"].abs().sum(1).mean()
    assert abs((total - dec["kl_sampled"]).item()) <= 1e-12 * mag.item()
    assert abs((dec["marginal_kl"] - dec["tc"] - dec["dwkl"]).item()) <= 1e-12 * mag.item()
    assert dec["mi"].item() <= math.log(mu.shape[0]) + 1e-12 * mag.item()
    assert abs(dec["dwkl_per_dim"].sum().item() - dec["dwkl"].item()) <= 1e-12 * mag.item()
    assert dec["n"] == z.shape[0] and dec["m"] == mu.shape[0]


# ================================================================ C ABI
def test_header_declares_and_binding_binds_the_entry_points(pkg):
    L = _L()
    txt = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    assert re.search(r"MMVAE_API\s+size_t\s+mmvae_posterior_mixture_scratch_bytes\s*\(", txt)
    assert re.search(r"MMVAE_API\s+int\s+mmvae_posterior_mixture\s*\(", txt)
    for name, nargs in (("mmvae_posterior_mixture_scratch_bytes", 3), ("mmvae_posterior_mixture", 11)):
        assert len(L.PROTOTYPES[name][1]) == nargs
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1]
    assert L.lib().mmvae_abi_version() == 3 and "#define MMVAE_ABI_VERSION 3" in txt
    assert "posterior_mixture.hip" in open(os.path.join(ROOT, "moving-mnist-vae_amd", "csrc", "Makefile")).read()
    assert "unspecified" in txt[txt.index("aggregate-posterior densities"):txt.index("mmvae_posterior_mixture_scratch_bytes(int")]


A = 0x1000                                                                      # a made-up device address, never dereferenced


def _rc(N=5, M=7, d=8, z=A, mu=A, logvar=A, log_qz=A, dims=A, scratch=A, scratch_bytes=None):
    lib = _L().lib()
    if scratch_bytes is None:
        scratch_bytes = lib.mmvae_posterior_mixture_scratch_bytes(N, M, d) or (1 << 20)
    rc = lib.mmvae_posterior_mixture(z, N, mu, logvar, M, d, log_qz, dims, scratch, scratch_bytes, None)
    return rc, (lib.mmvae_last_error() or b"").decode()


def test_posterior_mixture_refuses_bad_arguments_before_any_launch(pkg):
    big = _L().MIXTURE_MAX_N + 1
    for kw in ({"d": 513}, {"N": big}, {"M": big}):
        rc, msg = _rc(**kw)
        assert rc == ERR_UNSUPPORTED and "%s=%d" % next(iter(kw.items())) in msg, kw
    for kw in ({"d": 0}, {"d": -8}, {"N": 0}, {"N": -1}, {"M": 0}, {"M": -3}):
        rc, msg = _rc(**kw)
        assert rc == ERR_ARG and "%s=%d" % next(iter(kw.items())) in msg, kw
    for null in ("z", "mu", "logvar", "log_qz", "scratch"):
        rc, msg = _rc(**{null: None})
        assert rc == ERR_ARG and null in msg, null
    assert _rc(scratch=A + 8)[0] == ERR_ARG                                      # 16-byte alignment
    need = _L().lib().mmvae_posterior_mixture_scratch_bytes(5, 7, 8)
    rc, msg = _rc(scratch_bytes=need - 1)
    assert rc == ERR_ARG and "scratch_bytes" in msg
    assert _rc(scratch_bytes=0)[0] == ERR_ARG


def test_scratch_bytes_is_a_function_of_the_shape(pkg):
    fn = _L().lib().mmvae_posterior_mixture_scratch_bytes
    assert fn(5, 7, 8) == fn(5, 7, 8) > 0 and fn(5, 7, 8) % 16 == 0
    for bad in ((0, 7, 8), (5, 0, 8), (5, 7, 0), (5, 7, 513), ((1 << 20) + 1, 7, 8), (5, (1 << 20) + 1, 8), (-1, -1, -1)):
        assert fn(*bad) == 0, bad
    # the re-laid bank alone: 12 bytes per entry, M up to a multiple of 8, d up to a multiple of its tile
    assert fn(5, 7, 8) >= 8 * 16 * 12 and fn(1, 1000, 64) >= 1000 * 64 * 12
    assert fn(1 << 20, 1 << 20, 512) > (1 << 32)                                 # no 32-bit overflow at the top of the range
    assert fn(64, 1000, 64) >= fn(64, 500, 64) and fn(64, 1000, 64) >= fn(64, 1000, 32)


# ================================================================ Python surface
def test_python_surface_refuses_before_any_launch(pkg):
    z, mu, lv = torch.zeros(4, 8), torch.zeros(6, 8), torch.zeros(6, 8)
    with pytest.raises(ValueError, match="GPU"):
        pkg.posterior_mixture(z, mu, lv)
    with pytest.raises(ValueError, match="width"):
        pkg.posterior_mixture(torch.zeros(4, 9), mu, lv)
    with pytest.raises(ValueError, match="differ in shape"):
        pkg.posterior_mixture(z, mu, torch.zeros(5, 8))
    with pytest.raises(ValueError, match="differ in shape"):
        pkg.posterior_mixture(z, mu, torch.zeros(6, 9))
    with pytest.raises(ValueError, match="unsupported"):
        pkg.posterior_mixture(torch.zeros(2, 513), torch.zeros(3, 513), torch.zeros(3, 513))
    with pytest.raises(ValueError, match="shape"):
        pkg.posterior_mixture(torch.zeros(4, 8, 2, 1), mu, lv)
    with pytest.raises(ValueError, match="shape"):
        pkg.posterior_mixture(torch.zeros(32), mu, lv)
    with pytest.raises(ValueError, match="tensor"):
        pkg.posterior_mixture(None, mu, lv)
    # elbo_decomposition(mu, logvar, encoding, index): the same checks, and the index's own
    with pytest.raises(ValueError, match="GPU"):
        pkg.elbo_decomposition(mu, lv, torch.zeros(6, 8))
    with pytest.raises(ValueError, match="int64"):
        pkg.elbo_decomposition(mu, lv, z, index=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="indices"):
        pkg.elbo_decomposition(mu, lv, z, index=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="width"):
        pkg.elbo_decomposition(mu, lv, torch.zeros(6, 4))


def test_new_names_are_exported_and_documented(pkg):
    dec = importlib.import_module("moving-mnist-vae_amd.decomposition")
    for name in ("posterior_mixture", "elbo_decomposition"):
        assert getattr(pkg, name) is getattr(dec, name)
    assert inspect.signature(pkg.posterior_mixture).parameters["per_dim"].default is True
    assert inspect.signature(pkg.elbo_decomposition).parameters["index"].default is None
    assert inspect.signature(pkg.evaluate).parameters["decomposition"].default is False
    for doc in (pkg.elbo_decomposition.__doc__, pkg.evaluate.__doc__):
        assert "log M" in doc or "log_m" in doc
        assert "saturated" in doc.lower() and "one sample per image" in doc
