"""GPU: mmvae_posterior_mixture_bwd and what stands on it -- posterior_mixture(differentiable=True), latent_penalty, and the
args.latent_penalty hook of train -- against the f64 reference of tests/mixture_grad_ref.py.

Gate: |device - reference| <= K * 2^-24 * B for every element of d_z, d_mu and d_logvar; B and the rule that fixes K (= 2, from a plain
f32 restatement on the CPU, not from the kernel) are in mixture_grad_ref.py.  The device's own ratios are printed before they are
asserted; DESIGN.md 4.22 records them."""
import importlib
import math
import types

import pytest
import torch

from mixture_grad_ref import (K, PATTERNS, U, case_grad_ref, elementwise_scale, grad_ref, penalty_ref, penalty_upstream, ratios, upstream)
from mixture_ref import CASES, case_inputs, case_ref, decomposition_ref, mixture_ref

gpu = pytest.mark.gpu
K_JOINT, K_DIMS = 1.0, 2.0             # the forward's gate (tests/test_decomposition_gpu.py)
ERR_ARG = -1
SOME = ["ragged_130x67", "three_tiles_d130", "chunk_edges", "one_chunk"]


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _dev(name):
    return tuple(t.cuda() for t in case_inputs(name)[:3])


def _cuda(t):
    return None if t is None else t.cuda()


def _raw(z, mu, lv, log_qz, dims, gj, gd, fill=float("nan"), poison=None, short=0):
    """The C entry point on buffers of this test's own: outputs prefilled with `fill`, the scratch with the byte `poison` (None: as
    allocated), `short` bytes fewer than needed announced.  Returns (rc, {'d_z', 'd_mu', 'd_lv'})."""
    L = _L()
    (N, d), M = z.shape, mu.shape[0]
    nbytes = L.lib().mmvae_posterior_mixture_bwd_scratch_bytes(N, M, d)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    if poison is not None:
        scratch.fill_(poison)
    out = {"d_z": torch.full((N, d), fill, device="cuda"), "d_mu": torch.full((M, d), fill, device="cuda"),
           "d_lv": torch.full((M, d), fill, device="cuda")}
    rc = L.lib().mmvae_posterior_mixture_bwd(L.ptr(z), N, L.ptr(mu), L.ptr(lv), M, d, L.ptr(log_qz), L.ptr(dims), L.ptr(gj), L.ptr(gd),
                                             L.ptr(out["d_z"]), L.ptr(out["d_mu"]), L.ptr(out["d_lv"]), L.ptr(scratch), nbytes - short,
                                             L.cur_stream())
    torch.cuda.synchronize()
    return rc, out


def _same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("d_z", "d_mu", "d_lv"))


def _check(tag, got, ref):
    r = ratios(got, ref)
    print(f"{tag}: error / (2^-24 B): d_z {r['d_z']:.3f}, d_mu {r['d_mu']:.3f}, d_logvar {r['d_lv']:.3f}")
    for k in ("d_z", "d_mu", "d_lv"):
        assert torch.isfinite(got[k]).all(), k
        assert r[k] <= K, (k, r[k])


# ================================================================ the C entry point
@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_f64_reference(pkg, name, pattern):
    """'joint' passes NULL for g_dims AND log_qz_dims, 'dims' passes NULL for g_joint: the reference has that gradient zero."""
    z, mu, lv = _dev(name)
    log_qz, dims = pkg.posterior_mixture(z, mu, lv)
    gj, gd = (_cuda(t) for t in upstream(name, pattern))
    rc, got = _raw(z, mu, lv, log_qz, dims if gd is not None else None, gj, gd)
    assert rc == 0
    _check(f"posterior_mixture_bwd[{name} {CASES[name][:3]} {pattern}]", got, case_grad_ref(name, pattern))


@gpu
@pytest.mark.parametrize("name", SOME)
def test_written_not_accumulated_deterministic_and_blind_to_the_scratch(pkg, name):
    z, mu, lv = _dev(name)
    log_qz, dims = pkg.posterior_mixture(z, mu, lv)
    gj, gd = (_cuda(t) for t in upstream(name, "random"))
    rc, want = _raw(z, mu, lv, log_qz, dims, gj, gd, fill=0.0, poison=0x00)
    assert rc == 0
    rc, again = _raw(z, mu, lv, log_qz, dims, gj, gd, fill=0.0, poison=0x00)
    assert rc == 0 and _same_bits(want, again)                                              # two calls, the same bits
    for fill, poison in ((float("nan"), 0xFF), (1e30, None)):                              # 0xFF bytes: NaN in f32 and in f64
        rc, got = _raw(z, mu, lv, log_qz, dims, gj, gd, fill=fill, poison=poison)
        assert rc == 0 and _same_bits(got, want), (fill, poison)                            # every element written, none added to
    # log_qz_dims given but no gradient for it: the same bits as NULL
    rc, a = _raw(z, mu, lv, log_qz, dims, gj, None, poison=0xFF)
    rc2, b = _raw(z, mu, lv, log_qz, None, gj, None)
    assert rc == 0 and rc2 == 0 and _same_bits(a, b)


@gpu
def test_short_scratch_is_refused_and_nothing_runs(pkg):
    z, mu, lv = _dev("ragged_130x67")
    log_qz, dims = pkg.posterior_mixture(z, mu, lv)
    gj, gd = (_cuda(t) for t in upstream("ragged_130x67", "random"))
    rc, out = _raw(z, mu, lv, log_qz, dims, gj, gd, fill=5.0, short=1)
    assert rc == ERR_ARG and "scratch_bytes" in _L().lib().mmvae_last_error().decode()
    assert all((out[k] == 5.0).all() for k in out)


@gpu
def test_replays_in_a_graph(pkg):
    """One capture of the library call on a single stream: its replay on new contents equals the eager call, to the bit."""
    name = "three_tiles_d130"
    z, mu, lv = (t.clone() for t in _dev(name))
    gj, gd = (_cuda(t) for t in upstream(name, "random"))
    L = _L()
    (N, d), M = z.shape, mu.shape[0]
    nbytes = L.lib().mmvae_posterior_mixture_bwd_scratch_bytes(N, M, d)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    log_qz, dims = pkg.posterior_mixture(z, mu, lv)
    outs = [{"d_z": torch.empty_like(z), "d_mu": torch.empty_like(mu), "d_lv": torch.empty_like(lv)} for _ in range(2)]

    def call(o):
        assert L.lib().mmvae_posterior_mixture_bwd(L.ptr(z), N, L.ptr(mu), L.ptr(lv), M, d, L.ptr(log_qz), L.ptr(dims), L.ptr(gj), L.ptr(gd),
                                                   L.ptr(o["d_z"]), L.ptr(o["d_mu"]), L.ptr(o["d_lv"]), L.ptr(scratch), nbytes,
                                                   L.cur_stream()) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(outs[0])                                                                       # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call(outs[0])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(3)
    z.copy_(z + 0.25 * torch.randn(z.shape, generator=g).cuda())
    fresh = pkg.posterior_mixture(z, mu, lv)
    log_qz.copy_(fresh[0])
    dims.copy_(fresh[1])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    call(outs[1])
    torch.cuda.synchronize()
    assert _same_bits(outs[0], outs[1])
    _check("posterior_mixture_bwd[replayed]", outs[0], grad_ref(z.cpu(), mu.cpu(), lv.cpu(), gj.cpu(), gd.cpu()))


# ================================================================ posterior_mixture(differentiable=True)
def _op_grads(pkg, z, mu, lv, cj, cd, per_dim=True):
    """d (cj . log_qz + cd . log_qz_dims) / d (z, mu, logvar) through the Python op; leaves of the inputs' own shape and dtype."""
    leaves = [t.clone().requires_grad_(True) for t in (z, mu, lv)]
    log_qz, dims = pkg.posterior_mixture(*leaves, per_dim=per_dim, differentiable=True)
    form = (cj * log_qz).sum() if cj is not None else 0.0
    if cd is not None:
        form = form + (cd * dims).sum()
    gz, gm, gl = torch.autograd.grad(form, leaves)
    for g, t in zip((gz, gm, gl), (z, mu, lv)):
        assert g.shape == t.shape and g.dtype == t.dtype
    return {"d_z": gz, "d_mu": gm, "d_lv": gl}, log_qz, dims


@gpu
@pytest.mark.parametrize("name", ["ragged_130x67", "one_chunk"])
def test_python_op_gradients(pkg, name):
    z, mu, lv = _dev(name)
    cj, cd = (_cuda(t) for t in upstream(name, "random"))                                   # a random f64 linear form of both outputs
    got, log_qz, dims = _op_grads(pkg, z, mu, lv, cj, cd)
    assert log_qz.grad_fn is not None and dims.grad_fn is not None and log_qz.dtype == dims.dtype == torch.float64
    _check(f"posterior_mixture(differentiable=True)[{name}]", got, case_grad_ref(name, "random"))
    plain, plain_dims = pkg.posterior_mixture(z.clone().requires_grad_(True), mu, lv)       # the default: detached, today's bits
    assert plain.grad_fn is None and plain_dims.grad_fn is None and not plain.requires_grad
    assert torch.equal(plain, log_qz.detach()) and torch.equal(plain_dims, dims.detach())
    # an output that nothing consumed goes down as NULL; per_dim=False never has one
    only_j, _, _ = _op_grads(pkg, z, mu, lv, cj, None)
    no_dims, lq, none = _op_grads(pkg, z, mu, lv, cj, None, per_dim=False)
    assert none is None and torch.equal(lq.detach(), plain) and _same_bits(only_j, no_dims)
    _check(f"posterior_mixture(differentiable=True)[{name}, joint only]", only_j, case_grad_ref(name, "joint"))
    only_d, _, _ = _op_grads(pkg, z, mu, lv, None, cd)
    _check(f"posterior_mixture(differentiable=True)[{name}, per-dimension only]", only_d, case_grad_ref(name, "dims"))


@gpu
@pytest.mark.parametrize("name", ["ragged_130x67", "chunk_edges"])
def test_layouts(pkg, name):
    z, mu, lv = _dev(name)
    cj, cd = (_cuda(t) for t in upstream(name, "random"))
    want, _, _ = _op_grads(pkg, z, mu, lv, cj, cd)
    four = [t[:, :, None, None] for t in (z, mu, lv)]
    got, _, _ = _op_grads(pkg, *four, cj, cd)
    assert all(got[k].dim() == 4 for k in got)
    assert _same_bits({k: v.reshape(v.shape[0], -1) for k, v in got.items()}, want)
    strided = [t.t().contiguous().t() for t in (z, mu, lv)]                                 # column-major storage
    assert not any(t.is_contiguous() for t in strided if t.shape[0] > 1 and t.shape[1] > 1)
    got, _, _ = _op_grads(pkg, *strided, cj, cd)
    assert _same_bits({k: v.contiguous() for k, v in got.items()}, want)
    got, _, _ = _op_grads(pkg, z.double(), mu.double(), lv.double(), cj, cd)                # made f32; gradients come back f64
    assert _same_bits({k: v.float() for k, v in got.items()}, want)


# ================================================================ latent_penalty
def _draw_96():
    g = torch.Generator().manual_seed(21)
    mu, lv = torch.randn((96, 64), generator=g), -4.0 + 4.0 * torch.rand((96, 64), generator=g)
    z = mu + torch.exp(0.5 * lv) * torch.randn((96, 64), generator=g)
    return z.float().contiguous(), mu.float().contiguous(), lv.float().contiguous()


def _penalty_inputs(which):
    return case_inputs("257x257x2")[:3] if which == "257x257x2" else _draw_96()


@gpu
@pytest.mark.parametrize("which", ["257x257x2", "draw_96x96x64"])
def test_latent_penalty_values_and_gradients(pkg, which):
    cz, cmu, clv = _penalty_inputs(which)
    N, d = cz.shape
    leaves = [t.cuda().requires_grad_(True) for t in (cmu, clv, cz)]
    penalty, terms = pkg.latent_penalty(*leaves, beta=6)
    assert penalty.dtype == torch.float64 and penalty.dim() == 0 and penalty.is_cuda
    dec = pkg.elbo_decomposition(leaves[0].detach(), leaves[1].detach(), leaves[2].detach())
    assert torch.equal(terms["tc"].detach().view(torch.int64), dec["tc"].view(torch.int64))           # bit-equal
    for k in ("mi", "dwkl"):
        assert torch.equal(terms[k].view(torch.int64), dec[k].view(torch.int64)) and not terms[k].requires_grad
    ref = mixture_ref(cz, cmu, clv)
    want = decomposition_ref(cmu, clv, cz)
    bound_tc = (K_JOINT * U * ref["B"] + K_DIMS * U * ref["B_dims"].sum(1)).mean().item()            # the forward's gate through the mean
    print(f"latent_penalty[{which}]: penalty {penalty.item()!r} (reference {5 * want['tc'].item()!r}, bound {5 * bound_tc:.3e})")
    assert abs(penalty.item() - 5.0 * want["tc"].item()) <= 5.0 * bound_tc + 1e-12 * abs(want["tc"].item())
    got = dict(zip(("d_mu", "d_lv", "d_z"), torch.autograd.grad(penalty, leaves)))
    assert all(g.dtype == torch.float32 for g in got.values())
    _, _, (r_mu, r_lv, r_z) = penalty_ref(cmu, clv, cz, beta=6)
    gj, gd = penalty_upstream(N, d, beta=6)                                                 # 5 / N and -5 / N
    assert gj[0].item() == 5.0 / N and gd[0, 0].item() == -5.0 / N
    scale = grad_ref(cz, cmu, clv, gj, gd)
    e_mu, e_lv, e_z = elementwise_scale(cmu, clv, cz)                                       # zeros: beta alone has no elementwise part
    ref_g = {"d_z": r_z, "d_mu": r_mu, "d_lv": r_lv, "B_z": scale["B_z"] + e_z, "B_mu": scale["B_mu"] + e_mu, "B_lv": scale["B_lv"] + e_lv}
    assert (scale["d_z"] - r_z).abs().max() <= 1e-12 * r_z.abs().max()                      # the composition does imply these upstreams
    _check(f"latent_penalty[{which}] gradients", got, ref_g)


@gpu
def test_latent_penalty_all_three_coefficients(pkg):
    """alpha, beta and gamma at once, with a dataset size: the own density and the prior join in (elementwise_scale), values shift by the
    minibatch-weighted-sampling constants, gradients do not."""
    cz, cmu, clv = _draw_96()
    N, d = cz.shape
    coef = dict(alpha=2.0, beta=6.0, gamma=0.5)
    leaves = [t.cuda().requires_grad_(True) for t in (cmu, clv, cz)]
    penalty, terms = pkg.latent_penalty(*leaves, **coef, dataset_size=60000)
    plain, plain_terms = pkg.latent_penalty(*leaves, **coef)
    log_d = math.log(60000)
    for k, shift in (("mi", log_d), ("tc", (d - 1) * log_d), ("dwkl", -d * log_d)):
        assert abs(terms[k].item() - plain_terms[k].item() - shift) <= 1e-12 * abs(shift)
    got = dict(zip(("d_mu", "d_lv", "d_z"), torch.autograd.grad(penalty, leaves)))
    same = dict(zip(("d_mu", "d_lv", "d_z"), torch.autograd.grad(plain, leaves)))
    assert _same_bits(got, same)
    want_p, want_t, (r_mu, r_lv, r_z) = penalty_ref(cmu, clv, cz, **coef, dataset_size=60000)
    ref = mixture_ref(cz, cmu, clv)
    bj, bd = (K_JOINT * U * ref["B"]).mean().item(), (K_DIMS * U * ref["B_dims"].sum(1)).mean().item()
    bound = 1.0 * bj + 5.0 * (bj + bd) + 0.5 * bd
    assert abs(penalty.item() - want_p.item()) <= bound + 1e-12 * (abs(want_t["mi"].item()) + abs(want_t["tc"].item()) + abs(want_t["dwkl"].item()))
    scale = grad_ref(cz, cmu, clv, *penalty_upstream(N, d, **coef))
    e_mu, e_lv, e_z = elementwise_scale(cmu, clv, cz, alpha=2.0, gamma=0.5)
    ref_g = {"d_z": r_z, "d_mu": r_mu, "d_lv": r_lv, "B_z": scale["B_z"] + e_z, "B_mu": scale["B_mu"] + e_mu, "B_lv": scale["B_lv"] + e_lv}
    _check("latent_penalty[alpha, beta, gamma] gradients", got, ref_g)


# ================================================================ train with args.latent_penalty
N_E2E = 24


def _train_step(pkg, oracle, hook="absent"):
    """One train step of the 16 x 16 Gaussian model of tests/test_decomposition_gpu.py on 24 frames with fixed noise.  Returns the four
    lists, {parameter name: gradient} (before the optimiser step), (value, gradient) of mu, logvar and encoding, and eps."""
    Q = importlib.import_module("test_frame_quality_gpu")
    M = importlib.import_module("moving-mnist-vae_amd.model")
    m = Q._model(oracle, "gauss16").train()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(8)
    m.injected_eps = torch.randn(N_E2E, m.z_dimensions, 1, 1, generator=g).to(dev)
    m.injected_true_samples = torch.randn(N_E2E, m.z_dimensions, generator=g).to(dev)
    opt = M.FusedAdam(list(m.parameters()))
    grads, seen = [], []
    args = types.SimpleNamespace(data_ratio_of_labels=None, dataset="MovingMNIST", quiet=True,
                                 stats_callback=lambda model, **kw: grads.append([p.grad.detach().clone() for p in model.parameters()]))
    if hook != "absent":
        args.latent_penalty = hook
    def keep(mod, inp, out):
        for t in out[:3]:
            t.retain_grad()
        seen.append(out[:3])
    handle = m.register_forward_hook(keep)
    try:
        lists = pkg.train(m, [oracle.synthetic_labels(N_E2E, 16, seed=31, p=0.2).view(N_E2E, -1)], opt, dev, args, data_mean=Q.MEAN, data_std=Q.STD)
    finally:
        handle.remove()
    torch.cuda.synchronize()
    assert len(grads) == 1 and len(seen) == 1
    latent = [(t.detach().reshape(N_E2E, -1).float().cpu(), t.grad.detach().reshape(N_E2E, -1).float().cpu()) for t in seen[0]]
    named = dict(zip((n for n, _ in m.named_parameters()), grads[0]))
    return [list(map(float, l)) for l in lists], named, latent, m.injected_eps.reshape(N_E2E, -1).cpu()


@gpu
def test_train_with_the_latent_penalty(pkg, oracle):
    plain_lists, plain_grads, plain_latent, eps = _train_step(pkg, oracle)
    hook = pkg.make_latent_penalty(beta=6)
    lists, grads, latent, _ = _train_step(pkg, oracle, hook)
    rows = hook.to_host()
    assert rows.shape == (1, 4) and all(math.isfinite(v) for v in rows[0]) and hook.to_host().shape == (0, 4)
    assert lists == plain_lists                                                             # the four lists stay the reference's
    for (v, _), (pv, _) in zip(latent, plain_latent):
        assert torch.equal(v, pv)                                                           # the same forward pass
    (mu, g_mu), (lv, g_lv), (enc, g_enc) = latent
    (_, p_mu), (_, p_lv), (_, p_enc) = plain_latent
    want_p, want_t, (r_mu, r_lv, r_z) = penalty_ref(mu, lv, enc, beta=6)
    assert abs(rows[0][0] - want_p.item()) <= 1e-5 * max(abs(want_p.item()), 1.0) and abs(rows[0][2] - want_t["tc"].item()) <= 1e-5 * max(abs(want_t["tc"].item()), 1.0)
    scale = grad_ref(enc, mu, lv, *penalty_upstream(N_E2E, mu.shape[1], beta=6))
    # the retained gradient of mu / logvar is the TOTAL one: the penalty reaches them directly and through encoding = mu + exp(logvar / 2) eps
    # (mmvae_rsample_bwd: d_mu += d_enc, d_logvar += d_enc * 0.5 * eps * exp(logvar / 2)).  Beyond the gate, every f32 addition of autograd
    # and that kernel's two products round the magnitudes they handle: 8 U of their sum.
    half = 0.5 * eps.double() * torch.exp(0.5 * lv.double())
    total = {"d_z": r_z, "d_mu": r_mu + r_z, "d_lv": r_lv + r_z * half}
    bound = {"d_z": K * U * scale["B_z"], "d_mu": K * U * (scale["B_mu"] + scale["B_z"]), "d_lv": K * U * (scale["B_lv"] + scale["B_z"] * half.abs())}
    mags = {"d_z": r_z.abs(), "d_mu": r_mu.abs() + r_z.abs(), "d_lv": r_lv.abs() + (r_z * half).abs()}
    for k, got, base in (("d_z", g_enc, p_enc), ("d_mu", g_mu, p_mu), ("d_lv", g_lv, p_lv)):
        err = (got.double() - base.double() - total[k]).abs()
        allowed = bound[k] + 8 * U * (base.double().abs() + mags[k])
        print(f"train(latent_penalty)[{k}]: worst error / allowed {(err / allowed).max().item():.3f}; penalty share of the gradient "
              f"{(total[k].abs().max() / got.abs().max()).item():.3f}")
        assert (err <= allowed).all(), k
    enc_names = [n for n in grads if n.startswith("encoder.")]
    assert enc_names and sorted(grads) == sorted(plain_grads)
    assert any(not torch.equal(grads[n], plain_grads[n]) for n in enc_names)               # the penalty reaches the encoder's weights


@gpu
def test_train_without_the_hook_is_unchanged(pkg, oracle):
    """No attribute, the attribute set to None, and alpha = beta = gamma = 1: the same parameter gradients and lists, to the bit."""
    base_lists, base_grads, base_latent, _ = _train_step(pkg, oracle)
    for hook in ("absent", None, pkg.make_latent_penalty()):
        lists, grads, latent, _ = _train_step(pkg, oracle, hook)
        assert lists == base_lists
        assert all(torch.equal(grads[n], base_grads[n]) for n in base_grads)
        assert all(torch.equal(a[1], b[1]) for a, b in zip(latent, base_latent))
