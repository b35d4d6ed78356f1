"""GPU: held-out evaluation through the Python surface -- VAE.per_image_terms, VAE.iw_bound and evaluate() -- on eval-mode models of
every family: Gaussian VAE (28 x 28: the cropped, non-contiguous reconstruction; f32 and bf16; 64 x 64), categorical VAE (Q = 2),
PixelVAE (teacher-forced) and a PixelCNN on its own.

The per-image terms are compared with the float64 formulas of tests/test_eval_ops_gpu.py applied on the CPU to the MODEL'S OWN mu,
logvar and reconstruction: that isolates the new kernels from the network's precision, so the tolerances are that file's derived
bounds (units of u = 2^-24 times the term magnitudes), asserted for every image.  Their sums are also checked against N times the
scalars of the untouched VAE.loss within the sum of both bounds (the per-image one and the batch sum's, the same formula) plus the one
f32 rounding of the scalar VAE.loss returns.

Worst error / bound ratios measured on the MI355X: per_image_terms nll 0.15, kl 0.06, their sums against VAE.loss 0.04; iw_bound 0.11
(K = 1: 0.14); evaluate's per-image nll 0.15 (weighted 0.01, PixelCNN 0.05)."""
import importlib
import math
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_eval_ops_gpu import (U, U64, _report, ce_bound_pixels, iw_bound_cols, logratio_bound_rows, nll_bound_rows, ref_ce,  # noqa: E402
                               ref_gauss_nll, ref_iw, ref_kl, ref_logratio)

gpu = pytest.mark.gpu
MEAN, STD = 0.0521, 0.2222

# name -> (VAE's positional constructor arguments, compute dtype, N)
#         in mid dec_out pix_out z  pixelcnn only layers                     sigma S
CASES = {
    "gauss28_f32": ((1, 32, 1, 2, 32, False, False, 4, "ReLu", 1, 1, 0, True, 0.1, 28), "f32", 3),
    "gauss28_bf16": ((1, 32, 1, 2, 32, False, False, 4, "ReLu", 1, 1, 0, True, 0.1, 28), "bf16", 3),
    "gauss64": ((1, 32, 1, 2, 8, False, False, 4, "ReLu", 1, 1, 0, True, 0.1, 64), "bf16", 2),
    "cat_q2": ((1, 32, 2, 2, 32, False, False, 4, "ReLu", 1, 1, 0, True, 0.1, 32), "bf16", 3),
    "pixelvae": ((1, 16, 1, 2, 8, True, False, 2, "ReLu", 1, 1, 0, True, 0.0, 16), "bf16", 3),
    "pixelcnn": ((1, 16, 1, 4, 32, True, True, 2, "ReLu", 1, 1, 0, True, 0.0, 8), "f32", 3),
}


def _M():
    return importlib.import_module("moving-mnist-vae_amd.model")


def _model(oracle, name, **over):
    ctor, dt, N = CASES[name]
    M = _M()
    torch.manual_seed(3)
    ctor = list(ctor)
    if "require_rsample" in over:
        ctor[12] = over["require_rsample"]
    m = M.VAE(*ctor, compute_dtype=dt)
    if not m.only_pixelcnn and m.pixelcnn is None:
        # well-conditioned weights and non-trivial BatchNorm running statistics (the default ones are 0 / 1)
        m.load_state_dict(oracle.filled_state(oracle.state_spec(ctor[0], ctor[4], ctor[2], ctor[14], ctor[12]), seed=5))
    return m.to("cuda").eval(), N


def _labels(oracle, m, N, seed=21, p=0.0521):
    Q = m.pixelcnn_out_channels if m.only_pixelcnn else 2
    lab = oracle.synthetic_labels(N, m.input_image_size, seed=seed, p=p)
    if Q > 2:
        lab = lab * torch.randint(1, Q, lab.shape, generator=torch.Generator().manual_seed(seed))
    return lab.view(N, -1)


def _categorical(m):
    return m.pixelcnn is not None or m.decoder_out_channels > m.in_channels


def _ref_nll(m, rec, target, weight=None):
    """f64 per-image NLL of the reconstruction the model produced, and its bound (tests/test_eval_ops_gpu.py)."""
    N = rec.shape[0]
    rec = rec.detach().float().cpu()
    if _categorical(m):
        r = ref_ce(rec.reshape(N, rec.shape[1], -1), target.cpu().reshape(N, -1), None if weight is None else weight.cpu().float())
        return r["loss"].sum(1), ce_bound_pixels(r).sum(1)
    r2, t2 = rec.reshape(N, -1), target.detach().float().cpu().reshape(N, -1)
    return ref_gauss_nll(r2, t2, m.sigma_decoder).sum(1), nll_bound_rows(r2, t2, m.sigma_decoder)


def _forward(m, labels, eps=None):
    image, target = m.prepare_batch(labels, torch.device("cuda"), MEAN, STD, _categorical(m))
    m.injected_eps = eps
    try:
        mu, lv, enc, rec = m(image, sample=image)
    finally:
        m.injected_eps = None
    return image, target, mu, lv, enc, rec


# ---------------------------------------------------------------- no GPU: there is no CPU fallback
def test_cpu_model_raises(pkg):
    M = _M()
    L = importlib.import_module("moving-mnist-vae_amd._lib")
    assert pkg.evaluate is importlib.import_module("moving-mnist-vae_amd.main").evaluate
    m = M.VAE(1, 32, 1, 2, 32, False, False, 4, "ReLu", 1, 1, 0, True, 0.1, 28).eval()
    x = torch.zeros(2, 1, 28, 28)
    with pytest.raises(L.MmvaeError):
        m.per_image_terms(x, torch.zeros(2, 32, 1, 1), torch.zeros(2, 32, 1, 1), x)
    with pytest.raises(L.MmvaeError):
        m.iw_bound(x, x, 2)
    with pytest.raises(ValueError):
        m.iw_bound(x, x, 0)


# ---------------------------------------------------------------- per_image_terms
@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_per_image_terms(pkg, oracle, name):
    """nll and kl of every image against the f64 formulas on the model's own outputs (bounds: nll_bound_rows / ce_bound_pixels, 0.5 *
    8u * magnitude for the KL), f64 device tensors with no gradient; and their sums against N x the scalars of VAE.loss (coefficients
    1, mmd 0): twice the bound (both are sums of the same f32 terms) plus u of the f32 scalar."""
    m, N = _model(oracle, name)
    labels = _labels(oracle, m, N)
    with torch.no_grad():
        z = m.z_dimensions
        eps = torch.randn(N, z, 1, 1, generator=torch.Generator().manual_seed(9)).cuda()
        image, target, mu, lv, enc, rec = _forward(m, labels, eps)
        if m.adjust != 0 and m.pixelcnn is None:
            assert not rec.is_contiguous()
        nll, kl = m.per_image_terms(target, mu, lv, rec)
        args = types.SimpleNamespace(data_ratio_of_labels=None)
        _, nll_s, kl_s, _ = m.loss(target, mu, lv, enc, rec, torch.device("cuda"), args)
    assert nll.dtype == torch.float64 and nll.shape == (N,) and nll.is_cuda and not nll.requires_grad
    ref, bound = _ref_nll(m, rec, target)
    _report(f"terms_nll[{name}]", (nll.cpu() - ref).abs(), bound)
    tot = torch.tensor([abs(nll.sum().item() - N * float(nll_s))])
    _report(f"terms_nll_vs_loss[{name}]", tot, 2 * bound.sum().reshape(1) + U * abs(N * float(nll_s)))
    if m.only_pixelcnn:
        assert kl is None and mu is None
        return
    assert kl.dtype == torch.float64 and kl.shape == (N,) and kl.is_cuda
    t, mag = ref_kl(mu.cpu().view(N, z), lv.cpu().view(N, z))
    kb = 0.5 * 8 * U * mag.sum(1)
    _report(f"terms_kl[{name}]", (kl.cpu() - t.sum(1)).abs(), kb)
    _report(f"terms_kl_vs_loss[{name}]", torch.tensor([abs(kl.sum().item() - N * float(kl_s))]), 2 * kb.sum().reshape(1) + U * abs(N * float(kl_s)))


@gpu
def test_per_image_terms_without_logvar(pkg, oracle):
    m, N = _model(oracle, "gauss28_f32", require_rsample=False)
    with torch.no_grad():
        image, target, mu, lv, enc, rec = _forward(m, _labels(oracle, m, N))
        nll, kl = m.per_image_terms(target, mu, lv, rec)
    assert lv is None and kl is None
    ref, bound = _ref_nll(m, rec, target)
    _report("terms_nll[no_logvar]", (nll.cpu() - ref).abs(), bound)
    with pytest.raises(ValueError):
        m.iw_bound(image, target, 2)


# ---------------------------------------------------------------- iw_bound
@gpu
@pytest.mark.parametrize("name", ["gauss28_f32", "cat_q2", "pixelvae"])
def test_iw_bound_matches_recomputed_rows(pkg, oracle, name):
    """K = 3 with injected noise.  Each pass is redone through the public surface -- encoder.rsample on the injected eps (the code
    mu + exp(lv/2) eps), get_reconstruction (teacher-forced for the PixelVAE) -- its rows recomputed in f64 on the CPU (NLL of that
    reconstruction; the log ratio from mu, logvar, eps), and reduced with torch.logsumexp.  The bound: the log-mean-exp moves by at
    most the largest change of a row entry (its gradient is a softmax), so max_k (nll bound + log-ratio bound) per image, plus
    iw_bound_cols.  K = 1 is logratio - nll of that pass, to the last bit of the device rows."""
    L = importlib.import_module("moving-mnist-vae_amd._lib")
    m, N = _model(oracle, name)
    K, z = 3, m.z_dimensions
    labels = _labels(oracle, m, N)
    eps = torch.randn(K, N, z, generator=torch.Generator().manual_seed(13)).cuda()
    with torch.no_grad():
        image, target, mu, lv, _, _ = _forward(m, labels, eps[0].view(N, z, 1, 1))
        got = m.iw_bound(image, target, K, eps=eps)
        assert got.dtype == torch.float64 and got.shape == (N,) and got.is_cuda
        nll_rows, lr_rows, nb, lb = [], [], [], []
        for k in range(K):
            m.injected_eps = eps[k].view(N, z, 1, 1)
            enc = m.encoder.rsample(mu, lv)
            m.injected_eps = None
            rec = m.get_reconstruction(enc, sample=image)
            r, b = _ref_nll(m, rec, target)
            nll_rows.append(r); nb.append(b)
            t, _, _ = ref_logratio(mu.cpu().view(N, z), lv.cpu().view(N, z), eps[k].cpu())
            lr_rows.append(t.sum(1)); lb.append(logratio_bound_rows(mu.cpu().view(N, z), lv.cpu().view(N, z), eps[k].cpu()))
            if k == 0:
                nll0 = m.per_image_terms(target, None, None, rec)[0]
                lr0 = torch.empty(N, dtype=torch.float64, device="cuda")
                assert L.lib().mmvae_latent_logratio(mu.data_ptr(), lv.data_ptr(), eps[0].data_ptr(), N, z, lr0.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream) == 0
        got1 = m.iw_bound(image, target, 1, eps=eps[:1])
    nll_rows, lr_rows = torch.stack(nll_rows), torch.stack(lr_rows)
    bound = (torch.stack(nb) + torch.stack(lb)).max(0).values + iw_bound_cols(nll_rows, lr_rows)
    _report(f"iw[{name}]", (got.cpu() - ref_iw(nll_rows, lr_rows)).abs(), bound)
    assert torch.equal(got1, lr0 - nll0)
    _report(f"iw_k1[{name}]", (got1.cpu() - (lr_rows[0] - nll_rows[0])).abs(), nb[0] + lb[0] + U64 * (lr_rows[0] - nll_rows[0]).abs())


@gpu
def test_iw_bound_refuses(pkg, oracle):
    L = importlib.import_module("moving-mnist-vae_amd._lib")
    m, N = _model(oracle, "gauss28_f32")
    with torch.no_grad():
        image, target, *_ = _forward(m, _labels(oracle, m, N))
    m.train()
    with pytest.raises(L.MmvaeError):
        m.iw_bound(image, target, 2)
    m.eval()
    with pytest.raises(ValueError):
        m.iw_bound(image, target, 0)
    with pytest.raises(ValueError):
        m.iw_bound(image, target, 2, eps=torch.zeros(2, N, 4))
    p, Np = _model(oracle, "pixelcnn")
    with torch.no_grad():
        pimage, ptarget, *_ = _forward(p, _labels(oracle, p, Np))
    with pytest.raises(ValueError):
        p.iw_bound(pimage, ptarget, 2)


# ---------------------------------------------------------------- evaluate
def _two_batches(oracle, m):
    """3 + 2 images, the second batch far denser than the first: the mean over images is not the mean of the batch means."""
    a = _labels(oracle, m, 3, seed=31, p=0.03)
    b = _labels(oracle, m, 2, seed=32, p=0.35)
    return [a, b]


def _replay(m, loader, seed, K, weight=None):
    """What evaluate() computes, image by image, redone with the same generator: the f64 reference NLL of every image's
    reconstruction with its bound, and the device KL / iw_bound of the same draws."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ref, bound, kls, iws = [], [], [], []
    m.eval()
    with torch.no_grad():
        for labels in loader:
            N, z = labels.shape[0], m.z_dimensions
            eps = torch.randn((N, z, 1, 1), device="cuda", dtype=torch.float32, generator=gen)
            image, target, mu, lv, _, rec = _forward(m, labels, eps)
            r, b = _ref_nll(m, rec, target, weight)
            ref.append(r); bound.append(b)
            t, _ = ref_kl(mu.cpu().view(N, z), lv.cpu().view(N, z))
            kls.append(t.sum(1))
            if K:
                e = torch.randn((K, N, z), device="cuda", dtype=torch.float32, generator=gen)
                iws.append(m.iw_bound(image, target, K, eps=e, weight=weight).cpu())
    return torch.cat(ref), torch.cat(bound), torch.cat(kls), (torch.cat(iws) if K else None)


@gpu
@pytest.mark.parametrize("name", ["gauss28_f32", "cat_q2"])
def test_evaluate_means_over_images(pkg, oracle, name):
    """A 3 + 2 loader: every mean is the mean over the 5 per-image values (and differs from the mean of the two batch means), the
    per-image values are those of an image-by-image replay with the same generator, the train flag comes back, and no parameter or
    BatchNorm buffer moves."""
    m, _ = _model(oracle, name)
    loader = _two_batches(oracle, m)
    dev = torch.device("cuda")
    args = types.SimpleNamespace(data_ratio_of_labels=torch.tensor([0.6, 3.0]))
    K = 2
    m.train()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    res = pkg.evaluate(m, loader, dev, args, MEAN, STD, iw_samples=K, generator=torch.Generator(device="cuda").manual_seed(7),
                       return_per_image=True)
    assert m.training is True
    after = m.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    m.eval()
    plain = pkg.evaluate(m, loader, dev, args, MEAN, STD, generator=torch.Generator(device="cuda").manual_seed(7))
    assert m.training is False
    assert plain["iw_bound"] is None and "per_image" not in plain and plain["n_images"] == 5

    pi = res["per_image"]
    assert res["n_images"] == 5
    for key in ("nll", "kl", "iw_bound"):
        v = pi[key]
        assert v.dtype == torch.float64 and v.shape == (5,) and v.is_cuda
        mean = v.sum().item() / 5
        assert abs(res[key] - mean) <= 4 * U64 * v.abs().sum().item() / 5, key
        batchwise = 0.5 * (v[:3].mean().item() + v[3:].mean().item())
        assert abs(res[key] - batchwise) > 1e-6 * abs(mean), key      # the data makes the two differ
    assert res["elbo"] == -(res["nll"] + res["kl"])
    assert plain["kl"] == res["kl"]                                    # (the analytic KL does not depend on the draws)
    dims = m.in_channels * m.input_image_size ** 2
    if name == "cat_q2":
        assert res["bits_per_dim"] == res["nll"] / (dims * math.log(2.0))
    else:
        assert res["bits_per_dim"] is None

    ref, bound, kl_ref, iw_dev = _replay(m, loader, 7, K)
    _report(f"evaluate_nll[{name}]", (pi["nll"].cpu() - ref).abs(), bound)
    assert torch.equal(pi["iw_bound"].cpu(), iw_dev)


@gpu
def test_evaluate_weighted(pkg, oracle):
    """weighted=True passes args.data_ratio_of_labels to the cross-entropy: the per-image NLL follows the f64 reference with those
    weights on the same reconstructions (and is not the unweighted one); a Gaussian model ignores the flag."""
    m, _ = _model(oracle, "cat_q2")
    loader = _two_batches(oracle, m)
    dev = torch.device("cuda")
    w = torch.tensor([0.6, 3.0])
    args = types.SimpleNamespace(data_ratio_of_labels=w)
    g = lambda: torch.Generator(device="cuda").manual_seed(11)
    res_w = pkg.evaluate(m, loader, dev, args, MEAN, STD, weighted=True, generator=g(), return_per_image=True)
    res_u = pkg.evaluate(m, loader, dev, args, MEAN, STD, generator=g(), return_per_image=True)
    ref_w, bound_w, _, _ = _replay(m, loader, 11, 0, weight=w)
    ref_u, bound_u, _, _ = _replay(m, loader, 11, 0)
    _report("evaluate_weighted", (res_w["per_image"]["nll"].cpu() - ref_w).abs(), bound_w)
    _report("evaluate_unweighted", (res_u["per_image"]["nll"].cpu() - ref_u).abs(), bound_u)
    assert ((ref_w - ref_u).abs() > 100 * (bound_w + bound_u)).all()
    assert torch.equal(res_w["per_image"]["kl"], res_u["per_image"]["kl"])
    assert res_w["bits_per_dim"] == res_w["nll"] / (32 * 32 * math.log(2.0))


@gpu
def test_evaluate_pixelcnn_only(pkg, oracle):
    """No latent: nll and bits_per_dim only; iw_samples is refused (iw_bound's ValueError), the mode restored on the way out."""
    m, _ = _model(oracle, "pixelcnn")
    loader = _two_batches(oracle, m)
    dev = torch.device("cuda")
    args = types.SimpleNamespace(data_ratio_of_labels=None)
    res = pkg.evaluate(m, loader, dev, args, MEAN, STD, return_per_image=True)
    assert res["kl"] is None and res["elbo"] is None and res["iw_bound"] is None and res["per_image"]["kl"] is None
    refs, bounds = [], []
    with torch.no_grad():
        for labels in loader:
            image, target, _, _, _, rec = _forward(m, labels)
            r, b = _ref_nll(m, rec, target)
            refs.append(r); bounds.append(b)
    ref, bound = torch.cat(refs), torch.cat(bounds)
    _report("evaluate_pixelcnn", (res["per_image"]["nll"].cpu() - ref).abs(), bound)
    assert abs(res["nll"] - ref.mean().item()) <= bound.mean().item() + 4 * U64 * ref.abs().mean().item()
    assert res["bits_per_dim"] == res["nll"] / (8 * 8 * math.log(2.0))
    m.train()
    with pytest.raises(ValueError):
        pkg.evaluate(m, loader, dev, args, MEAN, STD, iw_samples=2)
    assert m.training is True
