"""GPU: op-level parity of csrc/eval_loss.hip through the C ABI -- the per-image Gaussian NLL, weighted cross-entropy, analytic KL,
log importance ratio log p(z) - log q(z|x), and the log-mean-exp of the importance-weighted bound -- against float64 torch
evaluations restated here: Normal.log_prob, F.cross_entropy(reduction='none', weight=...), the KL formula, torch.logsumexp.

Every tolerance is an error bound derived next to its test, as in tests/test_latent_loss_ops_gpu.py: units of u = 2^-24 (the relative
rounding error of one f32 operation) times the magnitudes of the terms before any cancellation, device expf / logf taken as <= 2 ulp
(4u), summed over the image's elements; the f64 accumulation adds nothing measurable.  The f64-only iw_bound is bounded in units of
2^-53 in the same way, for the kernel and for torch's own f64 evaluation.  Every test asserts |device - reference| <= bound for
EVERY image and prints the worst ratio.

Worst error / bound ratios measured on the MI355X (each test's own figure is in its docstring): Gaussian NLL 0.10, cross-entropy
0.15, KL 0.09, log ratio 0.19, iw_bound below 0.0001.

The pure-CPU reference helpers are checked against the torch functions in tests that run without a GPU."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U = 2.0 ** -24                      # unit roundoff of f32
U64 = 2.0 ** -53                    # unit roundoff of f64
ERR_ARG = -1
gpu = pytest.mark.gpu


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _rows(name, n, *args):
    """Call a per-image entry point twice on fresh NaN-filled outputs (tensor arguments stay alive across the calls); the two results
    must be the same bits.  Returns the f64 [n] result on the host."""
    L = _L()
    fn = getattr(L.lib(), name)
    outs = []
    for _ in range(2):
        out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        rc = fn(*[_p(a) if (isinstance(a, torch.Tensor) or a is None) else a for a in args], _p(out), _st())
        assert rc == 0, (name, rc, L.lib().mmvae_last_error())
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]), name
    return outs[0].cpu()


def _report(name, err, bound):
    """Assert err <= bound for every image; print the worst ratio (recorded in the docstrings)."""
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    print(f"RATIO {name} {ratio.max().item():.4f}")
    assert (err <= bound).all(), (name, ratio.max().item(), err.max().item())


# ================================================================ float64 references (pure CPU)
def ref_gauss_nll(r, t, sigma):
    """-Normal(r, sigma).log_prob(t) per element in f64 (sigma: the f32 value the kernel receives)."""
    s = float(np.float32(sigma))
    r, t = r.double(), t.double()
    return (t - r) ** 2 / (2 * s * s) + math.log(s) + math.log(math.sqrt(2 * math.pi))


def nll_bound_rows(r, t, sigma):
    """Per image [N, per]: tests/test_latent_loss_ops_gpu.py's _nll_bound applied to one row.  The quadratic part -- t - r rounded (2u
    relative on its square), the square, up to three roundings of non-negative partial sums, 1/(2 sigma^2) (2 roundings): 8u of the
    row's f64 quadratic sum; the constant log(sigma) + log(sqrt(2 pi)) -- logf 4u max(|log sigma|, 1), the addition and the f32
    constant u each of (|log sigma| + 1): per element."""
    s = float(np.float32(sigma))
    q = ((t.double() - r.double()) ** 2).sum(1) / (2 * s * s)
    return 8 * U * q + r.shape[1] * (4 * U * max(abs(math.log(s)), 1.0) + 2 * U * (abs(math.log(s)) + 1.0))


def ref_ce(x, tg, w):
    """F.cross_entropy(x, tg, weight=w, reduction='none') in f64 with the per-pixel quantities the bound uses.
    x [N, Q, HW] f32, tg [N, HW] int64, w [Q] or None."""
    xd = x.double()
    mx = xd.max(dim=1, keepdim=True).values
    z = xd - mx                                                   # exact in f64
    lse = z.exp().sum(dim=1, keepdim=True).log()
    logp = z - lse
    wt = torch.ones(x.shape[0], x.shape[2], dtype=torch.float64) if w is None else w.double()[tg]
    loss = -wt * logp.gather(1, tg[:, None]).squeeze(1)
    return dict(loss=loss, z=z, p=logp.exp(), lse=lse.squeeze(1), wt=wt, ztg=z.gather(1, tg[:, None]).squeeze(1))


def ce_bound_pixels(r):
    """Per pixel (tests/test_latent_loss_ops_gpu.py's _ce_fwd_bound), z_q = x_q - max, p = softmax, s = sum e^z: s's relative error <=
    u sum_q p_q |z_q| (the z's, one f32 rounding each) + 4u (expf) + (Q - 1)u (summation); log s adds 4u max(|log s|, 1); log s - z_tg
    re-rounds z_tg (u|z_tg|) and the result (u|loss|); w[t] * (...) one more u|loss|.  Summed over an image's pixels by the caller."""
    Q = r["p"].shape[1]
    spz = (r["p"] * r["z"].abs()).sum(1)
    return r["wt"] * (spz + 4 + (Q - 1) + 4 * r["lse"].abs().clamp_min(1.0) + r["ztg"].abs()) * U + 2 * U * r["loss"].abs()


def ref_kl(mu, lv):
    """-0.5 (lv - exp(lv) - mu^2 + 1) per element in f64, and the magnitude |lv| + e^lv + mu^2 + 1 of its terms before cancellation."""
    mu, lv = mu.double(), lv.double()
    return -0.5 * (lv - lv.exp() - mu * mu + 1), lv.abs() + lv.exp() + mu * mu + 1


def ref_logratio(mu, lv, eps):
    """log p(z) - log q(z|x) per element in f64 with z = mu + exp(lv/2) eps formed in f64: -0.5 (z^2 - eps^2 - lv); plus z and
    e = exp(lv/2) eps for the bound."""
    mu, lv, eps = mu.double(), lv.double(), eps.double()
    e = (0.5 * lv).exp() * eps
    z = mu + e
    return -0.5 * (z * z - eps * eps - lv), z, e


def logratio_bound_rows(mu, lv, eps):
    """The kernel forms z in f32 as the reparameterisation kernel does: expf 4u and the product u of |eps e^(lv/2)|, the sum u of |z|
    (test_rsample_fwd_bwd's 6u|eps e| + 2u|z| = dz); everything after that is f64.  |z_dev^2 - z^2| <= 2|z| dz + dz^2, halved by the
    -0.5; the f64 part: F64_TERMS * 2^-53 of the term magnitudes z^2 + eps^2 + |lv|."""
    _, z, e = ref_logratio(mu, lv, eps)
    dz = 6 * U * e.abs() + 2 * U * z.abs()
    mag = z * z + eps.double() ** 2 + lv.double().abs()
    return (0.5 * (2 * z.abs() * dz + dz * dz) + F64_TERMS * U64 * mag).sum(1)


# f64 roundings of (z^2 - eps^2) - lv summed over an image, in units of 2^-53 times sum(z^2 + eps^2 + |lv|): the kernel's four operations
# per element and the <= 10 additions an element passes through (two per thread at d = 512, six shuffle steps, the wave sums), and the
# four operations of a torch f64 evaluation whose rows are summed exactly (_fsum_rows): 4 + 10 + 4, rounded up.
F64_TERMS = 20


def _fsum_rows(t):
    """Correctly rounded row sums of an f64 [N, d] tensor."""
    return torch.tensor([math.fsum(row) for row in t.tolist()], dtype=torch.float64)


def ref_iw(nll, lr):
    """torch.logsumexp over the K samples of lr - nll, minus log K; f64 [K, N] -> [N]."""
    return torch.logsumexp(lr - nll, dim=0) - math.log(nll.shape[0])


def iw_bound_cols(nll, lr):
    """f64 throughout; w = lr - nll and w - max are correctly rounded IEEE operations, the same in the kernel and in torch.  From
    there, per evaluation and per column, in units of 2^-53: exp <= 2 ulp (4) and the K-term sum (K - 1), relative to s = sum
    exp(w - max) in [1, K], so absolute in log s; log itself 4 max(|log s|, 1); max + log s one rounding of its value; log K
    4 log K; the last subtraction one rounding of the result.  The kernel and torch's own f64 evaluation each stay within that:
    twice the sum."""
    K = nll.shape[0]
    w = lr - nll
    mx = w.max(dim=0).values
    logs = (w - mx).exp().sum(0).log()
    out = mx + logs - math.log(K)
    one = 4 + (K - 1) + 4 * logs.abs().clamp_min(1.0) + (mx + logs).abs() + 4 * math.log(K) + out.abs()
    return 2 * U64 * one


# ================================================================ reference self-checks (no GPU)
def test_ref_gauss_nll_is_normal_log_prob():
    g = torch.Generator().manual_seed(1)
    r, t = torch.randn(3, 50, generator=g), torch.randn(3, 50, generator=g)
    for sigma in (0.1, 1.0):
        s = float(np.float32(sigma))
        want = -torch.distributions.Normal(r.double(), s).log_prob(t.double())
        assert torch.allclose(ref_gauss_nll(r, t, sigma), want, rtol=1e-13, atol=1e-13)
    assert (nll_bound_rows(r, t, 0.1) > 0).all() and nll_bound_rows(r, t, 0.1).shape == (3,)


def test_ref_ce_is_cross_entropy():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 5, 7, generator=g) * 4
    tg = torch.randint(0, 5, (2, 7), generator=g)
    w = torch.rand(5, generator=g) + 0.5
    w[1] = 0.0
    for ww in (None, w):
        want = torch.nn.functional.cross_entropy(x.double(), tg, weight=None if ww is None else ww.double(), reduction="none")
        r = ref_ce(x, tg, ww)
        assert torch.allclose(r["loss"], want, rtol=1e-13, atol=1e-14)
        assert (ce_bound_pixels(r) >= 0).all()


def test_ref_kl_is_normal_kl():
    g = torch.Generator().manual_seed(3)
    mu, lv = torch.randn(4, 16, generator=g), torch.rand(4, 16, generator=g) * 12 - 8
    q = torch.distributions.Normal(mu.double(), (0.5 * lv.double()).exp())
    want = torch.distributions.kl_divergence(q, torch.distributions.Normal(0.0, 1.0))
    t, mag = ref_kl(mu, lv)
    assert torch.allclose(t, want, rtol=1e-12, atol=1e-13)
    assert (mag >= 1).all()


def test_ref_logratio_is_log_p_minus_log_q():
    g = torch.Generator().manual_seed(4)
    mu, lv, eps = torch.randn(4, 16, generator=g), torch.rand(4, 16, generator=g) * 12 - 8, torch.randn(4, 16, generator=g)
    t, z, _ = ref_logratio(mu, lv, eps)
    q = torch.distributions.Normal(mu.double(), (0.5 * lv.double()).exp())
    want = torch.distributions.Normal(0.0, 1.0).log_prob(z) - q.log_prob(z)
    # log q's (z - mu)^2 / (2 var) cancels down from 1 / var = e^8: relative to that magnitude
    assert ((t - want).abs() <= 1e-12 * (1 + z * z + (-lv.double()).exp())).all()
    t0, z0, _ = ref_logratio(mu, lv, torch.zeros_like(eps))
    assert torch.equal(z0, mu.double()) and torch.allclose(t0, -0.5 * (mu.double() ** 2 - lv.double()), rtol=1e-15, atol=0)
    assert (logratio_bound_rows(mu, lv, eps) > 0).all()


def test_ref_iw_is_log_mean_exp():
    g = torch.Generator().manual_seed(5)
    nll = 1e5 + 50 * torch.randn(6, 3, generator=g, dtype=torch.float64)
    lr = -100 + 30 * torch.randn(6, 3, generator=g, dtype=torch.float64)
    w = lr - nll
    sh = w - w.max(0).values
    want = w.max(0).values + sh.exp().mean(0).log()
    assert torch.allclose(ref_iw(nll, lr), want, rtol=1e-15, atol=1e-10)
    assert torch.equal(ref_iw(nll[:1], lr[:1]), w[0])
    assert (iw_bound_cols(nll, lr) > 0).all()


# ================================================================ GPU tests
# ---------------------------------------------------------------- Gaussian NLL per image
def _nll_inputs(N, per, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, 5, (N, per), generator=g).float() - 1.0          # normalised labels in [-1, 3]
    r = t + torch.randn(N, per, generator=g) * 0.3
    return r, t


@gpu
@pytest.mark.parametrize("sigma", [0.1, 1.0])
@pytest.mark.parametrize("N,per", [(1, 81), (3, 784), (2, 4096), (5, 3 * 81), (300, 257)])
def test_gauss_nll_per_image(N, per, sigma):
    """Odd rows (81, 243, 257: every row starts at another offset from a 16-byte boundary), rows shorter and longer than one pass of
    the block, more images than fit one wave of blocks.  Bound: nll_bound_rows.  Measured max ratio 0.10."""
    r, t = _nll_inputs(N, per, N * 1009 + per)
    got = _rows("mmvae_gauss_nll_per_image", N, r.cuda(), t.cuda(), N, per, sigma)
    ref = ref_gauss_nll(r, t, sigma).sum(1)
    _report(f"gauss_nll[{N}x{per},{sigma}]", (got - ref).abs(), nll_bound_rows(r, t, sigma))


@gpu
@pytest.mark.parametrize("off_r,off_t", [(1, 1), (1, 2), (3, 0), (2, 2)])
def test_gauss_nll_per_image_unaligned_base(off_r, off_t):
    """Two rows of 81 whose base pointers sit 4, 8 or 12 bytes past a 16-byte boundary inside larger buffers, recon and target at the
    same and at different offsets (the kernel may use 16-byte loads only in the first case, and only behind the row's head).  The
    buffers' other elements are NaN: a read outside the rows poisons the sum.  Measured max ratio 0.10."""
    N, per, sigma = 2, 81, 0.1
    r, t = _nll_inputs(N, per, 77 + off_r * 4 + off_t)
    br = torch.full((N * per + 8,), float("nan"))
    bt = torch.full((N * per + 8,), float("nan"))
    br[off_r:off_r + N * per] = r.reshape(-1)
    bt[off_t:off_t + N * per] = t.reshape(-1)
    brd, btd = br.cuda(), bt.cuda()
    rv, tv = brd[off_r:off_r + N * per], btd[off_t:off_t + N * per]
    assert rv.data_ptr() % 16 == 4 * off_r % 16 and tv.data_ptr() % 16 == 4 * off_t % 16
    got = _rows("mmvae_gauss_nll_per_image", N, rv, tv, N, per, sigma)
    ref = ref_gauss_nll(r, t, sigma).sum(1)
    _report(f"gauss_nll_unaligned[{off_r},{off_t}]", (got - ref).abs(), nll_bound_rows(r, t, sigma))


# ---------------------------------------------------------------- cross-entropy per image
def _ce_case(name, x, tg, w):
    N, Q, HW = x.shape
    got = _rows("mmvae_ce_per_image", N, x.cuda(), tg.cuda(), None if w is None else w.cuda(), N, Q, HW)
    r = ref_ce(x, tg, w)
    _report(name, (got - r["loss"].sum(1)).abs(), ce_bound_pixels(r).sum(1))
    return got, r


@gpu
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("HW", [4, 81, 784, 4096])
@pytest.mark.parametrize("Q", [1, 2, 3, 4, 16])
def test_ce_per_image(Q, HW, weighted):
    """N = 1 and 3, logits ~ 4 N(0, 1), uniform targets; Q = 1 (every loss exactly 0) up to the PixelCNN's limit of 16; HW below, at no
    multiple of, and above the block's 256 threads.  Bound: ce_bound_pixels summed over the image.  Measured max ratio 0.15."""
    for N in (1, 3):
        g = torch.Generator().manual_seed(Q * 10007 + HW * 3 + N)
        x = torch.randn(N, Q, HW, generator=g) * 4
        tg = torch.randint(0, Q, (N, HW), generator=g)
        w = (torch.rand(Q, generator=g) + 0.5) if weighted else None
        got, _ = _ce_case(f"ce[{N},{Q},{HW},{'w' if weighted else '-'}]", x, tg, w)
        if Q == 1:
            assert torch.equal(got, torch.zeros(N, dtype=torch.float64))


@gpu
def test_ce_per_image_wide_logits():
    """Logits over +-80: exp(x) itself overflows f32 at 88.7 and the distances to the maximum reach 160 (their exponentials underflow
    to 0): only the max-subtracted form stays within the bound.  Measured ratio 0.008."""
    g = torch.Generator().manual_seed(11)
    x = torch.rand(3, 4, 784, generator=g) * 160 - 80
    x[:, 0, 0], x[:, 1, 0] = 80.0, -80.0
    tg = torch.randint(0, 4, (3, 784), generator=g)
    got, r = _ce_case("ce_wide", x, tg, None)
    assert torch.isfinite(got).all() and r["loss"].max() > 80


@gpu
def test_ce_per_image_zero_weight_and_single_class():
    """A class of weight 0 contributes exactly nothing (an image of that class alone: 0.0); every target the same class (the weight
    gather and the target plane read at one index throughout).  Measured max ratio 0.03 (both)."""
    g = torch.Generator().manual_seed(12)
    x = torch.randn(3, 3, 81, generator=g) * 4
    tg = torch.randint(0, 3, (3, 81), generator=g)
    tg[1] = 2
    w = torch.tensor([0.7, 1.9, 0.0])
    got, _ = _ce_case("ce_zero_weight", x, tg, w)
    assert got[1].item() == 0.0 and got[0].item() > 0
    tg1 = torch.full((3, 81), 1, dtype=torch.int64)
    _ce_case("ce_single_class", x, tg1, None)
    _ce_case("ce_single_class_w", x, tg1, w)


# ---------------------------------------------------------------- KL and log ratio per image
def _latent_inputs(N, d, seed):
    g = torch.Generator().manual_seed(seed)
    mu, eps = torch.randn(N, d, generator=g), torch.randn(N, d, generator=g)
    lv = torch.rand(N, d, generator=g) * 12 - 8                             # logvar over [-8, 4]
    lv.view(-1)[0], lv.view(-1)[-1] = -8.0, 4.0
    return mu, lv, eps


@gpu
@pytest.mark.parametrize("N", [1, 3, 130])
@pytest.mark.parametrize("d", [8, 32, 512])
def test_kl_per_image(d, N):
    """The kernel's f32 term ((l - e^l) - m^2) + 1 against the f64 formula: expf 4u e^l, m^2 u m^2, then one rounding of each of the
    three partial results, all bounded by the term magnitude |l| + e^l + m^2 + 1: per element 0.5 * 8u * magnitude (the bound of
    test_kl_fwd_matches_reference), summed over the image.  Measured max ratio 0.09."""
    mu, lv, _ = _latent_inputs(N, d, N * 131 + d)
    got = _rows("mmvae_kl_per_image", N, mu.cuda(), lv.cuda(), N, d)
    t, mag = ref_kl(mu, lv)
    _report(f"kl[{N},{d}]", (got - t.sum(1)).abs(), 0.5 * 8 * U * mag.sum(1))


@gpu
@pytest.mark.parametrize("N", [1, 3, 130])
@pytest.mark.parametrize("d", [8, 32, 512])
def test_latent_logratio(d, N):
    """Bound: logratio_bound_rows.  Also against the f32 code mmvae_rsample_fwd itself produces from the same inputs: with that z the
    rest is f64 arithmetic on both sides, so the two agree to the f64 part of the bound alone -- the kernel's z IS the decoder's
    input.  With eps = 0: z = mu exactly and the ratio is -0.5 sum(mu^2 - lv), again to f64 rounding.  Measured max ratio 0.19
    (f64 reference), 0.04 (device z), 0.04 (eps = 0)."""
    L = _L()
    mu, lv, eps = _latent_inputs(N, d, N * 137 + d)
    mud, lvd, epsd = mu.cuda(), lv.cuda(), eps.cuda()
    got = _rows("mmvae_latent_logratio", N, mud, lvd, epsd, N, d)
    t, z, _ = ref_logratio(mu, lv, eps)
    _report(f"logratio[{N},{d}]", (got - t.sum(1)).abs(), logratio_bound_rows(mu, lv, eps))
    zd = torch.empty_like(mud)
    assert L.lib().mmvae_rsample_fwd(_p(mud), _p(lvd), _p(epsd), _p(zd), N * d, _st()) == 0
    torch.cuda.synchronize()
    z32 = zd.cpu().double()
    mag = z32 * z32 + eps.double() ** 2 + lv.double().abs()
    tz = -0.5 * (z32 * z32 - eps.double() ** 2 - lv.double())
    _report(f"logratio_device_z[{N},{d}]", (got - _fsum_rows(tz)).abs(), (F64_TERMS * U64 * mag).sum(1))
    zero = torch.zeros_like(eps)
    got0 = _rows("mmvae_latent_logratio", N, mud, lvd, zero.cuda(), N, d)
    ref0 = -0.5 * (mu.double() ** 2 - lv.double())
    _report(f"logratio_eps0[{N},{d}]", (got0 - _fsum_rows(ref0)).abs(), (F64_TERMS * U64 * (mu.double() ** 2 + lv.double().abs())).sum(1))


# ---------------------------------------------------------------- importance-weighted bound
def _iw_inputs(K, N, seed, lead_col=None):
    g = torch.Generator().manual_seed(seed)
    nll = 1e5 + 50 * torch.randn(K, N, generator=g, dtype=torch.float64)
    lr = -100 + 30 * torch.randn(K, N, generator=g, dtype=torch.float64)
    if lead_col is not None:                      # one sample more than 800 nats ahead of every other in this column
        w = lr - nll
        k = K // 2
        nll[k, lead_col] = -(w[:, lead_col].max().item() + 900.0) + lr[k, lead_col].item()
    return nll, lr


@gpu
@pytest.mark.parametrize("N", [1, 7])
@pytest.mark.parametrize("K", [1, 5, 64])
def test_iw_bound(K, N):
    """Rows around 1e5 nats (an image's NLL), spread over ~60 nats; for K > 1 the last column holds one sample > 800 nats ahead of
    the rest (exp of the others underflows to 0: the result is that sample - log K, and exp of any unshifted value is 0 or inf).
    K = 1 must return logratio - nll to the last bit.  Bound: iw_bound_cols.  Measured max ratio below 0.0001."""
    nll, lr = _iw_inputs(K, N, K * 17 + N, lead_col=(N - 1) if K > 1 else None)
    got = _rows("mmvae_iw_bound", N, nll.cuda(), lr.cuda(), K, N)
    ref = ref_iw(nll, lr)
    assert torch.isfinite(got).all()
    _report(f"iw[{K},{N}]", (got - ref).abs(), iw_bound_cols(nll, lr))
    if K == 1:
        assert torch.equal(got, (lr - nll)[0])
    else:
        w = lr - nll
        lead = w[:, N - 1].max()
        assert (lead - w[:, N - 1].sort().values[-2]) > 800
        assert abs(got[N - 1].item() - (lead.item() - math.log(K))) <= 4 * U64 * abs(lead.item())


# ---------------------------------------------------------------- argument errors
@gpu
def test_bad_arguments_enqueue_nothing():
    """MMVAE_ERR_ARG for null pointers and non-positive N, per, Q, HW, d, K or sigma -- ordinary invalid arguments only, every device
    pointer valid for the sizes named -- and the output buffer keeps its sentinel."""
    lib = _L().lib()
    st = _st()
    f = torch.zeros(64, device="cuda")
    tg = torch.zeros(64, dtype=torch.int64, device="cuda")
    dd = torch.zeros(64, dtype=torch.float64, device="cuda")
    out = torch.full((8,), 5.0, dtype=torch.float64, device="cuda")
    F, T, D, O = _p(f), _p(tg), _p(dd), _p(out)
    bad = [
        lib.mmvae_gauss_nll_per_image(None, F, 2, 8, 0.1, O, st), lib.mmvae_gauss_nll_per_image(F, None, 2, 8, 0.1, O, st),
        lib.mmvae_gauss_nll_per_image(F, F, 2, 8, 0.1, None, st), lib.mmvae_gauss_nll_per_image(F, F, 0, 8, 0.1, O, st),
        lib.mmvae_gauss_nll_per_image(F, F, -1, 8, 0.1, O, st), lib.mmvae_gauss_nll_per_image(F, F, 2, 0, 0.1, O, st),
        lib.mmvae_gauss_nll_per_image(F, F, 2, 8, 0.0, O, st), lib.mmvae_gauss_nll_per_image(F, F, 2, 8, -0.1, O, st),
        lib.mmvae_gauss_nll_per_image(F, F, 2, 8, float("nan"), O, st),
        lib.mmvae_ce_per_image(None, T, None, 2, 2, 4, O, st), lib.mmvae_ce_per_image(F, None, None, 2, 2, 4, O, st),
        lib.mmvae_ce_per_image(F, T, None, 2, 2, 4, None, st), lib.mmvae_ce_per_image(F, T, None, 0, 2, 4, O, st),
        lib.mmvae_ce_per_image(F, T, None, 2, 0, 4, O, st), lib.mmvae_ce_per_image(F, T, None, 2, 2, 0, O, st),
        lib.mmvae_ce_per_image(F, T, F, 2, -2, 4, O, st),
        lib.mmvae_kl_per_image(None, F, 2, 8, O, st), lib.mmvae_kl_per_image(F, None, 2, 8, O, st), lib.mmvae_kl_per_image(F, F, 2, 8, None, st),
        lib.mmvae_kl_per_image(F, F, 0, 8, O, st), lib.mmvae_kl_per_image(F, F, 2, 0, O, st), lib.mmvae_kl_per_image(F, F, 2, -8, O, st),
        lib.mmvae_latent_logratio(None, F, F, 2, 8, O, st), lib.mmvae_latent_logratio(F, None, F, 2, 8, O, st),
        lib.mmvae_latent_logratio(F, F, None, 2, 8, O, st), lib.mmvae_latent_logratio(F, F, F, 2, 8, None, st),
        lib.mmvae_latent_logratio(F, F, F, 0, 8, O, st), lib.mmvae_latent_logratio(F, F, F, 2, 0, O, st),
        lib.mmvae_iw_bound(None, D, 3, 2, O, st), lib.mmvae_iw_bound(D, None, 3, 2, O, st), lib.mmvae_iw_bound(D, D, 3, 2, None, st),
        lib.mmvae_iw_bound(D, D, 0, 2, O, st), lib.mmvae_iw_bound(D, D, 3, 0, O, st), lib.mmvae_iw_bound(D, D, -3, 2, O, st),
    ]
    torch.cuda.synchronize()
    assert bad == [ERR_ARG] * len(bad), bad
    assert torch.equal(out.cpu(), torch.full((8,), 5.0, dtype=torch.float64))
    # and the same buffers with valid arguments run
    assert lib.mmvae_kl_per_image(F, F, 2, 8, O, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:2].cpu(), torch.zeros(2, dtype=torch.float64)) and out[2].item() == 5.0
