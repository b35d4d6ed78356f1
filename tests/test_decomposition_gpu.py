"""GPU: mmvae_posterior_mixture and the Python surface on top of it (posterior_mixture, elbo_decomposition,
evaluate(..., decomposition=True)) against the f64 reference of tests/mixture_ref.py.

Gate: |device - reference| <= K * 2^-24 * B for every element of both outputs, B the error scale of mixture_ref.py (the softmax-weighted
f32 rounding of the terms that count, plus the magnitude of the result, plus 1).  K is twice the largest ratio observed over the case
table on an MI355X, rounded up to a power of two (DESIGN.md 4.21 records the ratios); a plain f32 restatement of the formulas on the CPU
reaches 0.6 (joint) and 1.5 (per dimension) on inputs of this kind, so a ratio above about 8 would not be f32 rounding."""
import importlib
import math
import types

import pytest
import torch

from mixture_ref import CASES, U, case_inputs, case_ref, decomposition_ref, mixture_ref, own_density

gpu = pytest.mark.gpu
K_JOINT, K_DIMS = 1.0, 2.0             # largest ratios observed over the case table: 0.324 (joint), 0.712 (per dimension)
ERR_ARG = -1
SOME = ["ragged_130x67", "three_tiles_d130", "chunk_edges", "one_chunk"]       # two tiles / five tiles / chunks with a remainder / one chunk


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _dev(name):
    return tuple(t.cuda() for t in case_inputs(name))


def _ratios(got, got_dims, ref):
    rj = ((got.cpu() - ref["log_qz"]).abs() / (U * ref["B"])).max().item()
    rd = ((got_dims.cpu() - ref["log_qz_dims"]).abs() / (U * ref["B_dims"])).max().item()
    return rj, rd


def _raw(z, mu, lv, per_dim=True, fill=float("nan"), poison=None, short=0):
    """The C entry point on buffers of this test's own: outputs prefilled with `fill`, the scratch with the byte `poison` (None: as
    allocated), `short` bytes fewer than needed announced.  Returns (rc, log_qz, log_qz_dims or None)."""
    L = _L()
    (N, d), M = z.shape, mu.shape[0]
    nbytes = L.lib().mmvae_posterior_mixture_scratch_bytes(N, M, d)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    if poison is not None:
        scratch.fill_(poison)
    out = torch.full((N,), fill, dtype=torch.float64, device="cuda")
    dims = torch.full((N, d), fill, dtype=torch.float64, device="cuda") if per_dim else None
    rc = L.lib().mmvae_posterior_mixture(L.ptr(z), N, L.ptr(mu), L.ptr(lv), M, d, L.ptr(out), L.ptr(dims), L.ptr(scratch), nbytes - short,
                                         L.cur_stream())
    torch.cuda.synchronize()
    return rc, out, dims


def _same_bits(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


# ================================================================ the kernel
@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_f64_reference(pkg, name):
    z, mu, lv, _ = _dev(name)
    got, dims = pkg.posterior_mixture(z, mu, lv)
    assert got.dtype == dims.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (z.shape[0],) and tuple(dims.shape) == tuple(z.shape)
    assert torch.isfinite(got).all() and torch.isfinite(dims).all()
    rj, rd = _ratios(got, dims, case_ref(name))
    print(f"posterior_mixture[{name} {CASES[name][:3]}]: error / (2^-24 B): joint {rj:.3f}, per-dimension {rd:.3f}")
    assert rj <= K_JOINT and rd <= K_DIMS


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_without_the_per_dimension_output_log_qz_has_the_same_bits(pkg, name):
    z, mu, lv, _ = _dev(name)
    full, _ = pkg.posterior_mixture(z, mu, lv)
    alone, none = pkg.posterior_mixture(z, mu, lv, per_dim=False)
    assert none is None and _same_bits(full, alone)


@gpu
@pytest.mark.parametrize("name", SOME)
def test_written_not_accumulated_deterministic_and_blind_to_the_scratch(pkg, name):
    z, mu, lv, _ = _dev(name)
    want, want_dims = pkg.posterior_mixture(z, mu, lv)
    again, again_dims = pkg.posterior_mixture(z, mu, lv)
    assert _same_bits(want, again) and _same_bits(want_dims, again_dims)                    # two calls, the same bits
    for fill, poison in ((float("nan"), None), (1e300, 0xFF), (float("nan"), 0x00)):       # 0xFF bytes: NaN in f32 and in f64
        rc, out, dims = _raw(z, mu, lv, fill=fill, poison=poison)
        assert rc == 0
        assert _same_bits(out, want) and _same_bits(dims, want_dims), (fill, poison)        # every element written, none added to
    rc, out, none = _raw(z, mu, lv, per_dim=False, poison=0xFF)
    assert rc == 0 and _same_bits(out, want)


@gpu
def test_short_scratch_is_refused_and_nothing_runs(pkg):
    z, mu, lv, _ = _dev("ragged_130x67")
    rc, out, dims = _raw(z, mu, lv, fill=5.0, short=1)
    assert rc == ERR_ARG and "scratch_bytes" in _L().lib().mmvae_last_error().decode()
    assert (out == 5.0).all() and (dims == 5.0).all()


@gpu
@pytest.mark.parametrize("name", ["ragged_130x67", "chunk_edges"])
def test_layouts(pkg, name):
    z, mu, lv, _ = _dev(name)
    want, want_dims = pkg.posterior_mixture(z, mu, lv)
    four = pkg.posterior_mixture(z[:, :, None, None], mu[:, :, None, None], lv[:, :, None, None])
    assert _same_bits(four[0], want) and _same_bits(four[1], want_dims)
    strided = [t.t().contiguous().t() for t in (z, mu, lv)]                                 # column-major storage
    assert not any(t.is_contiguous() for t in strided if t.shape[0] > 1 and t.shape[1] > 1)
    got = pkg.posterior_mixture(*strided)
    assert _same_bits(got[0], want) and _same_bits(got[1], want_dims)
    wide = [torch.cat([t, t], 1)[:, :t.shape[1]] for t in (z, mu, lv)]                      # a slice of wider rows
    got = pkg.posterior_mixture(*wide)
    assert _same_bits(got[0], want) and _same_bits(got[1], want_dims)
    got = pkg.posterior_mixture(z.double(), mu.double(), lv.double())                       # made f32
    assert _same_bits(got[0], want) and _same_bits(got[1], want_dims)


@gpu
def test_single_posterior_is_the_own_density(pkg):
    g = torch.Generator().manual_seed(12)
    N, d = 70, 40
    mu, lv = torch.randn((1, d), generator=g), torch.rand((1, d), generator=g) * 6 - 5
    z = (mu + torch.exp(0.5 * lv) * torch.randn((N, d), generator=g)).float()
    got, dims = pkg.posterior_mixture(z.cuda(), mu.cuda(), lv.cuda())
    ref = mixture_ref(z, mu, lv)
    own = own_density(z, mu.expand(N, d), lv.expand(N, d))
    assert ((got.cpu() - own).abs() <= K_JOINT * U * ref["B"]).all()
    assert ((dims.cpu().sum(1) - own).abs() <= K_DIMS * U * ref["B_dims"].sum(1)).all()


@gpu
@pytest.mark.parametrize("name", SOME)
def test_doubled_bank_changes_nothing(pkg, name):
    """q(z) of the bank concatenated with itself is the same mixture: 2 M rows, log(2 M) subtracted."""
    z, mu, lv, _ = _dev(name)
    ref = case_ref(name)
    one, one_dims = pkg.posterior_mixture(z, mu, lv)
    two, two_dims = pkg.posterior_mixture(z, torch.cat([mu, mu]), torch.cat([lv, lv]))
    assert ((one - two).abs().cpu() <= 2 * K_JOINT * U * ref["B"]).all()
    assert ((one_dims - two_dims).abs().cpu() <= 2 * K_DIMS * U * ref["B_dims"]).all()


@gpu
def test_replays_in_a_graph(pkg):
    """One posterior_mixture call captured on a single stream and replayed on new contents equals the eager call, to the bit."""
    z, mu, lv, _ = (t.clone() for t in _dev("three_tiles_d130"))
    call = lambda: pkg.posterior_mixture(z, mu, lv)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                                              # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(3)
    for _ in range(2):
        z.copy_(torch.randn(z.shape, generator=g))
        mu.copy_(torch.randn(mu.shape, generator=g))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager = call()
        assert torch.equal(captured[0], eager[0]) and torch.equal(captured[1], eager[1])
    rj, rd = _ratios(captured[0], captured[1], mixture_ref(z.cpu(), mu.cpu(), lv.cpu()))
    assert rj <= K_JOINT and rd <= K_DIMS


# ================================================================ elbo_decomposition
def _dec_bounds(ref):
    """The gate carried through the means: what each key may differ by from the f64 reference."""
    bj, bd = K_JOINT * U * ref["B"], K_DIMS * U * ref["B_dims"]
    return {"mi": bj.mean(), "tc": (bj + bd.sum(1)).mean(), "dwkl": bd.sum(1).mean(), "marginal_kl": bj.mean() + 2 * bd.sum(1).mean(),
            "dwkl_per_dim": bd.mean(0)}


def _check_decomposition(tag, got, want, ref):
    bounds = _dec_bounds(ref)
    scale = 1e-12 * (ref["B"].mean() + ref["B_dims"].sum(1).mean()).item()                  # f64 roundings of the means
    for k in ("mi", "tc", "dwkl", "marginal_kl"):
        g, w = float(got[k]), float(want[k])
        print(f"{tag}: {k} {g!r} (reference {w!r}, bound {float(bounds[k]):.3e})")
        assert abs(g - w) <= float(bounds[k]) + scale, k
    per = torch.as_tensor(got["dwkl_per_dim"]).cpu()
    assert per.dtype == torch.float64 and ((per - want["dwkl_per_dim"]).abs() <= bounds["dwkl_per_dim"] + scale).all()
    for k in ("kl_sampled", "kl_analytic", "log_m"):                                        # f64 tensor operations on the f32 inputs
        assert abs(float(got[k]) - float(want[k])) <= 1e-12 * max(abs(float(want[k])), 1.0), k
    assert got["n"] == want["n"] and got["m"] == want["m"]


@gpu
@pytest.mark.parametrize("name", ["64x1000x64", "257x257x2", "extreme"])
def test_elbo_decomposition_values(pkg, name):
    z, mu, lv, index = _dev(name)
    cz, cmu, clv, cindex = case_inputs(name)
    ref = case_ref(name)
    got = pkg.elbo_decomposition(mu, lv, z, index=index)
    for k in ("mi", "tc", "dwkl", "marginal_kl", "kl_sampled", "kl_analytic", "log_m"):
        assert got[k].dtype == torch.float64 and got[k].dim() == 0 and got[k].is_cuda, k
    assert got["dwkl_per_dim"].is_cuda and tuple(got["dwkl_per_dim"].shape) == (z.shape[1],)
    assert isinstance(got["n"], int) and isinstance(got["m"], int)
    assert _same_bits(got["log_qz"], pkg.posterior_mixture(z, mu, lv, per_dim=False)[0])
    _check_decomposition(f"elbo_decomposition[{name}]", got, decomposition_ref(cmu, clv, cz, cindex, ref["log_qz"], ref["log_qz_dims"]), ref)
    assert float(got["mi"]) <= math.log(mu.shape[0]) + float(_dec_bounds(ref)["mi"])
    # kl_analytic against the per-image kernel's mean: its f32 terms carry 0.5 * 8u of |l| + e^l + m^2 + 1 (tests/test_eval_ops_gpu.py)
    L = _L()
    m_i, l_i = mu[index].contiguous(), lv[index].contiguous()
    rows = torch.empty(z.shape[0], dtype=torch.float64, device="cuda")
    assert L.lib().mmvae_kl_per_image(L.ptr(m_i), L.ptr(l_i), z.shape[0], z.shape[1], L.ptr(rows), L.cur_stream()) == 0
    mag = (l_i.double().abs() + torch.exp(l_i.double()) + m_i.double() ** 2 + 1.0).sum(1).mean().item()
    assert abs(float(got["kl_analytic"]) - rows.mean().item()) <= 0.5 * 8 * U * mag


@gpu
def test_elbo_decomposition_index_path(pkg):
    z, mu, lv, _ = _dev("257x257x2")
    ref = case_ref("257x257x2")
    full = pkg.elbo_decomposition(mu, lv, z)                                                # index = arange
    same = pkg.elbo_decomposition(mu, lv, z, index=torch.arange(257, device="cuda"))
    for k in ("mi", "tc", "dwkl", "kl_sampled", "kl_analytic"):
        assert _same_bits(full[k], same[k]), k
    pick = torch.tensor([5, 0, 256, 77, 78, 200, 13])
    sub = pkg.elbo_decomposition(mu, lv, z[pick.cuda()], index=pick.cuda())
    assert sub["n"] == 7 and sub["m"] == 257
    # the same pairs in another launch shape (another cut of the bank): the matching rows of the full call, within twice the gate
    assert ((sub["log_qz"] - full["log_qz"][pick.cuda()]).abs().cpu() <= 2 * K_JOINT * U * ref["B"][pick]).all()
    cz, cmu, clv, _ = case_inputs("257x257x2")
    want = decomposition_ref(cmu, clv, cz[pick], pick)
    sref = mixture_ref(cz[pick], cmu, clv)
    _check_decomposition("elbo_decomposition[index]", sub, want, sref)
    with pytest.raises(ValueError, match="index"):
        pkg.elbo_decomposition(mu, lv, z[:9])                                               # N != M needs an index
    with pytest.raises(ValueError):
        pkg.elbo_decomposition(mu.cpu(), lv, z)


# ================================================================ evaluate(decomposition=True)
@gpu
def test_evaluate_decomposition(pkg, oracle):
    Q = importlib.import_module("test_frame_quality_gpu")
    E = importlib.import_module("test_evaluate_gpu")
    m = Q._model(oracle, "gauss16")
    S, z, dev = m.input_image_size, m.z_dimensions, torch.device("cuda")
    loader = [oracle.synthetic_labels(n, S, seed=40 + i, p=p).view(n, -1) for i, (n, p) in enumerate(((4, 0.05), (4, 0.2), (3, 0.35)))]
    args = types.SimpleNamespace(data_ratio_of_labels=None)
    g = lambda: torch.Generator(device="cuda").manual_seed(7)
    seen = []
    hook = m.register_forward_hook(lambda mod, inp, out: seen.append(tuple(t.detach().float().reshape(t.shape[0], -1).cpu() for t in out[:3])))
    try:
        res = pkg.evaluate(m, loader, dev, args, Q.MEAN, Q.STD, generator=g(), return_per_image=True, decomposition=True)
    finally:
        hook.remove()
    plain = pkg.evaluate(m, loader, dev, args, Q.MEAN, Q.STD, generator=g(), return_per_image=True)
    assert len(seen) == 3 and "decomposition" not in plain and sorted(plain["per_image"]) == ["iw_bound", "kl", "nll"]
    assert sorted(res) == sorted(list(plain) + ["decomposition"]) and sorted(res["per_image"]) == ["iw_bound", "kl", "log_qz", "nll"]
    for k, v in plain.items():
        if k != "per_image":
            assert res[k] == v, k                                                           # floats: equal means bit-equal
    for k, v in plain["per_image"].items():
        assert (res["per_image"][k] is None and v is None) or torch.equal(res["per_image"][k], v), k
    mu, lv, enc = (torch.cat([s[i] for s in seen]) for i in range(3))
    assert tuple(mu.shape) == (11, z)
    ref = mixture_ref(enc, mu, lv)
    dec = res["decomposition"]
    assert sorted(dec) == sorted(["mi", "tc", "dwkl", "marginal_kl", "kl_sampled", "kl_analytic", "log_m", "dwkl_per_dim", "n", "m"])
    assert all(isinstance(dec[k], float) for k in ("mi", "tc", "dwkl", "marginal_kl", "kl_sampled", "kl_analytic", "log_m"))
    assert type(dec["dwkl_per_dim"]).__module__ == "numpy" and dec["dwkl_per_dim"].shape == (z,) and dec["n"] == dec["m"] == res["n_images"] == 11
    _check_decomposition("evaluate(decomposition=True)", dec, decomposition_ref(mu, lv, enc, None, ref["log_qz"], ref["log_qz_dims"]), ref)
    assert ((res["per_image"]["log_qz"].cpu() - ref["log_qz"]).abs() <= K_JOINT * U * ref["B"]).all()
    # a PixelCNN on its own has no latent
    pargs = types.SimpleNamespace(model="pixelcnn_3", input_channels=1, input_image_size=8, intermediate_channels=16, z_dimension=32,
                                  sigma_decoder=0.0, require_rsample=True, nll=1.0, quantization=4, compute_dtype="f32")
    torch.manual_seed(3)
    p, _ = pkg.select_model(pargs)
    p = p.to("cuda").eval()
    assert p.only_pixelcnn
    pres = pkg.evaluate(p, E._two_batches(oracle, p), dev, args, E.MEAN, E.STD, decomposition=True, return_per_image=True)
    assert pres["decomposition"] is None and pres["per_image"]["log_qz"] is None and pres["kl"] is None
    # without a sampled code there is no q(z|x) density
    ctor = list(Q.MODELS["gauss16"][0])
    ctor[12] = False
    torch.manual_seed(3)
    plain_ae = importlib.import_module("moving-mnist-vae_amd.model").VAE(*ctor, compute_dtype="bf16").to("cuda").eval()
    with pytest.raises(ValueError, match="require_rsample"):
        pkg.evaluate(plain_ae, loader, dev, args, Q.MEAN, Q.STD, decomposition=True)
