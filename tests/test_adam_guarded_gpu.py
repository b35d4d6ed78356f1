"""The guarded Adam step: global-norm clipping and skipping of non-finite steps on the device (mmvae_grad_norm_sq,
mmvae_adam_step_guarded, FusedAdam(max_grad_norm=..., skip_nonfinite=...)).

CPU: the per-step-scale f64 emulation the GPU tests judge against is itself checked against tests/test_latent_loss_ops_gpu.py's
adam_emulate and against torch.optim.Adam fed clip_grad_norm_-clipped gradients.  GPU, ops level: the norm's summation bound,
determinism, misalignment, non-finite inputs; five guarded steps inside the propagated f32 bound; guard off == mmvae_adam_step_dev to
the bit; skipped steps leave everything alone; graph replay == eager.  GPU, model level: FusedAdam's keywords and properties on the
smallest VAE.

Norm bound: n non-negative f64 terms, each the rounded square of an exact product, summed in any order: at most n - 1 additions
and one rounding per term, |dev - ref| <= (n + 2) * 2^-53 * ref (the reference's own f64 sum included with room to spare: torch sums
pairwise).  The square root halves a relative error and adds its own rounding, so the same bound holds for the norm."""
import functools
import importlib
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_latent_loss_ops_gpu import ADAM, ERR_ARG, U, _L, _p, _st, adam_emulate, gpu  # noqa: E402

U64 = 2.0 ** -53
SIZES = [1, 257, 524289]       # one element; odd, two blocks of the update; one past the 2048 x 256 grid-stride cap (129 norm blocks)


def f32(x):
    return float(np.float32(x))


# ================================================================ the emulation (pure CPU)
def adam_emulate_scaled(p, grads, lr, b1, b2, eps, wd, scales, f32_hyper=True):
    """adam_emulate with one f64 gradient scale PER STEP (grad_scale x clip factor); scales[k] is None for a skipped step, which
    leaves p, m, v, the step count t (hence the bias corrections) and the error bounds alone.

    The kernel does not see the f64 scale s but s^ = f32(s), and forms g_dev = fl32(g * s^).  Against the exact g0 = g * s:
        |g_dev - g0| <= |g| |s - s^| + U |g s^|,        |s - s^| <= U |s|,
    i.e. the U |g0| of adam_emulate (the product's rounding) plus at most one more U |g0| for the rounding of the scalar, taken here
    at its actual value |g| |s - s^|: zero when s is an f32 number, so that with a constant f32 scale every output, bounds included,
    is exactly adam_emulate's.  Everything after the gradient is adam_emulate's sequence, restated.

    f32_hyper=False keeps beta1, beta2 and the bias corrections in f64 (torch.optim.Adam's own arithmetic on f64 tensors) instead of
    rounding them through f32 as the kernels receive them."""
    p = p.double().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    Ep, Em, Ev = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    r = f32 if f32_hyper else float
    b1f, b2f = r(b1), r(b2)
    t = 0
    for g, s in zip(grads, scales):
        if s is None:
            continue
        t += 1
        sh = f32(s)
        g0 = g.double() * s
        gg = g0 + wd * p if wd != 0 else g0
        Eg = U * (g.double() * sh).abs() + g.double().abs() * abs(s - sh) + (wd * Ep + 2 * U * abs(wd) * p.abs() + U * gg.abs() if wd != 0 else 0.0)
        mn = m + (gg - m) * (1 - b1f)
        Em = b1f * Em + (1 - b1f) * Eg + U * (2 * (gg - m).abs() * (1 - b1f) + (gg - m).abs() + mn.abs()) + U * (1 - b1f) * (gg - m).abs()
        vn = v * b2f + (1 - b2f) * gg * gg
        Ev = b2f * Ev + (1 - b2f) * 2 * gg.abs() * Eg + U * (v * b2f + 4 * (1 - b2f) * gg * gg + vn + (1 - b2f) * gg * gg)
        bc1 = r(1 - b1f ** t)
        bc2 = r(math.sqrt(1 - b2f ** t))
        sq = vn.sqrt()
        denom = sq / bc2 + eps
        Ed = torch.where(vn > 0, Ev / (2 * sq.clamp_min(1e-300)), Ev.sqrt()) / bc2 + U * (3 * sq / bc2 + denom)
        step = lr / bc1
        upd = step * mn / denom
        Ep = Ep + step * (Em / denom + mn.abs() * Ed / denom ** 2) + U * (3 * upd.abs() + (p - upd).abs())
        p, m, v = p - upd, mn, vn
    return (p, m, v), (Ep, Em, Ev), t


def clip_factor(max_norm, total):
    """torch.nn.utils.clip_grad_norm_: min(1, max_norm / (total + 1e-6)); max_norm <= 0: off."""
    return min(1.0, max_norm / (total + 1e-6)) if max_norm > 0 else 1.0


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """p0 and five gradients of magnitudes 1e-7 .. 1: the generator of test_latent_loss_ops_gpu._adam_run.  Shared; never written."""
    g = torch.Generator().manual_seed(n + 11)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * torch.exp(torch.rand(n, generator=g) * math.log(1e7)) * 1e-7 for _ in range(5)]
    return p0, grads


def _ref_norm_sq(g, gs):
    return ((g.double() * gs) ** 2).sum().item()


def test_emulation_with_a_constant_scale_is_adam_emulate():
    p0, grads = _inputs(257)
    a = ADAM
    args = (f32(a["lr"]), a["b1"], a["b2"], f32(a["eps"]), f32(a["wd"]))
    (p, m, v), (Ep, Em, Ev), t = adam_emulate_scaled(p0, grads, *args, [a["gs"]] * 5)
    (rp, rm, rv), (rEp, rEm, rEv) = adam_emulate(p0, grads, *args, a["gs"])
    assert t == 5
    for x, y in ((p, rp), (m, rm), (v, rv), (Ep, rEp), (Em, rEm), (Ev, rEv)):
        assert torch.equal(x, y)
    # a scale that is no f32 number widens the gradient term, by at most U |g0| (here: visibly, and never narrows it)
    (_, _, _), (Ep2, Em2, Ev2), _ = adam_emulate_scaled(p0, grads, *args, [0.1] * 5)
    (_, _, _), (rEp2, rEm2, rEv2) = adam_emulate(p0, grads, *args, 0.1)
    assert (Em2 >= rEm2).all() and (Em2 > rEm2).any() and (Em2 <= 2 * rEm2).all()


def test_emulation_matches_torch_adam_on_clipped_gradients():
    """torch.optim.Adam(foreach=False) on f64 tensors, gradients clipped by clip_grad_norm_ itself, one step left out (what a skip
    does); the emulation with the clip factors as per-step scales and f64 hyper-parameters agrees to 1e-12."""
    g = torch.Generator().manual_seed(6)
    p0 = torch.randn(300, generator=g, dtype=torch.float64)
    grads = [torch.randn(300, generator=g, dtype=torch.float64) * 10.0 ** (k - 3) for k in range(6)]
    max_norm = grads[2].norm().item() * 1.5            # steps 0-2 unclipped, 3-5 clipped
    kw = dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-3, weight_decay=0.1)
    prm = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([prm], foreach=False, **kw)
    scales = []
    for k, gr in enumerate(grads):
        if k == 4:
            scales.append(None)
            continue
        prm.grad = gr.clone()
        total = torch.nn.utils.clip_grad_norm_([prm], max_norm).item()
        scales.append(clip_factor(max_norm, total))
        opt.step()
    assert [s == 1.0 for s in scales if s is not None] == [True, True, True, False, False]
    (p, m, v), _, t = adam_emulate_scaled(p0, grads, 3e-3, 0.8, 0.95, 1e-3, 0.1, scales, f32_hyper=False)
    st = opt.state[prm]
    assert t == 5 and int(st["step"]) == 5
    for got, ref in ((p, prm.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
        assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12 * ref.abs().max().item()), (got - ref).abs().max().item()


# ================================================================ GPU, ops level
def _norm_sq(gd, n, gs, part=True):
    """mmvae_grad_norm_sq on the device tensor gd (first n elements) -> (f64 sum, ticket word afterwards)."""
    L = _L()
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    sc = torch.zeros(L.SUM_PARTIALS, dtype=torch.float64, device="cuda")
    rc = L.lib().mmvae_grad_norm_sq(_p(gd), n, gs, _p(acc), _p(sc) if part else None, _st())
    assert rc == 0, (rc, L.lib().mmvae_last_error())
    torch.cuda.synchronize()
    return acc.item(), sc[:1].view(torch.int64).item()


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_sq(n):
    """sum (0.25 g)^2 against the f64 torch sum within (n + 2) 2^-53 (module docstring); twice the same bits; ticket back at zero;
    g one float off a 16-byte boundary and n no multiple of 4 (heads and tails of 1-3 elements); the one-block form; an inf at n - 1
    gives +inf, a NaN at 0 gives NaN."""
    gs = ADAM["gs"]
    g = _inputs(n)[1][0]
    ref = _ref_norm_sq(g, gs)
    gd = g.cuda()
    a, ticket = _norm_sq(gd, n, gs)
    b, _ = _norm_sq(gd, n, gs)
    print(f"\nn={n}: |dev - ref| / ((n + 2) 2^-53 ref) = {abs(a - ref) / ((n + 2) * U64 * ref):.3f}")
    assert abs(a - ref) <= (n + 2) * U64 * ref
    assert a == b and ticket == 0
    one, _ = _norm_sq(gd, n, gs, part=False)
    assert abs(one - ref) <= (n + 2) * U64 * ref
    # misaligned views of one padded buffer: offsets 1, 2, 3 floats past a 16-byte boundary, lengths that leave tails of 0 .. 3
    pad = torch.zeros(n + 8, device="cuda")
    assert pad.data_ptr() % 16 == 0
    for off in (1, 2, 3):
        for cut in (0, 1, 2, 3):
            k = n - cut
            if k < 1:
                continue
            pad.zero_()
            view = pad[off:off + k]
            view.copy_(gd[:k])
            got, ticket = _norm_sq(view, k, gs)
            r = _ref_norm_sq(g[:k], gs)
            assert abs(got - r) <= (k + 2) * U64 * r, (off, cut)
            assert ticket == 0
    bad = gd.clone()
    bad[n - 1] = float("inf")
    assert _norm_sq(bad, n, gs)[0] == float("inf")
    bad = gd.clone()
    bad[0] = float("nan")
    assert math.isnan(_norm_sq(bad, n, gs)[0])


class _Guarded:
    """p, m, v, state and scratch of a sequence of mmvae_adam_step_guarded calls (ADAM's hyper-parameters)."""

    def __init__(self, p0, max_norm):
        L = _L()
        n = p0.numel()
        self.n, self.max_norm, self.lib = n, max_norm, L.lib()
        self.p, self.m, self.v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        self.state = torch.zeros(4, dtype=torch.float64, device="cuda")
        self.part = torch.zeros(L.SUM_PARTIALS, dtype=torch.float64, device="cuda")

    def step(self, gd):
        a = ADAM
        rc = self.lib.mmvae_adam_step_guarded(_p(self.p), _p(gd), _p(self.m), _p(self.v), self.n, a["lr"], a["b1"], a["b2"], a["eps"], a["wd"],
                                              _p(self.state), _p(self.part), a["gs"], self.max_norm, _st())
        assert rc == 0, (rc, self.lib.mmvae_last_error())

    def pmv(self):
        return self.p.cpu(), self.m.cpu(), self.v.cpu()


def _emulate(p0, grads, scales):
    a = ADAM
    return adam_emulate_scaled(p0, grads, f32(a["lr"]), a["b1"], a["b2"], f32(a["eps"]), f32(a["wd"]), scales)


def _within(got, ref, E):
    return ((got.double() - ref).abs() <= E + 1e-30).all(), ((got.double() - ref).abs() / (E + 1e-30)).max().item()


@gpu
@pytest.mark.parametrize("which", ["off", "half", "double"])
@pytest.mark.parametrize("n", SIZES)
def test_guarded_five_steps(n, which):
    """Five guarded steps (ADAM's hyper-parameters, grad_scale 0.25) with max_norm off, at half the median per-step norm (every step
    clips) and at twice it (none does): the device's norm within the summation bound every step, then p, exp_avg, exp_avg_sq within
    the propagated bound of adam_emulate_scaled run with the scale computed on the host from the device's own norm.

    n = 1: five norms of one element each spread over five decades, and no multiple of their median clips all or none of them;
    there max_norm is half the smallest / twice the largest norm instead, which does.
    Measured max ratio to the bound at n = 524289: 0.81 (p), 0.30 (exp_avg), 0.50 (exp_avg_sq); the norm: 0.007 of its bound at most."""
    gs = ADAM["gs"]
    p0, grads = _inputs(n)
    norms = [math.sqrt(_ref_norm_sq(g, gs)) for g in grads]
    med = sorted(norms)[2]
    lo = 0.5 * med if 0.5 * med < min(norms) else 0.5 * min(norms)
    hi = 2.0 * med if 2.0 * med > max(norms) + 1e-6 else 2.0 * max(norms)
    max_norm = f32({"off": 0.0, "half": lo, "double": hi}[which])
    if which == "half":
        assert all(clip_factor(max_norm, t * (1 + (n + 2) * U64)) < 1.0 and clip_factor(max_norm, t * (1 - (n + 2) * U64)) < 1.0 for t in norms)
    if which == "double":
        assert all(max_norm / (t * (1 + (n + 2) * U64) + 1e-6) > 1.0 for t in norms)
    run = _Guarded(p0, max_norm)
    scales = []
    for g, ref in zip(grads, norms):
        run.step(g.cuda())
        total = run.state[1].item()
        assert abs(total - ref) <= (n + 2) * U64 * ref, (total, ref)
        scales.append(gs * clip_factor(max_norm, total))
    assert run.state.cpu().tolist()[0] == 5.0 and run.state[2].item() == 0.0 and run.state[3].item() == 0.0
    assert run.part[:1].view(torch.int64).item() == 0
    assert all((s < gs) if which == "half" else (s == gs) for s in scales)
    (rp, rm, rv), (Ep, Em, Ev), t = _emulate(p0, grads, scales)
    assert t == 5
    ratios = []
    for got, ref, E in zip(run.pmv(), (rp, rm, rv), (Ep, Em, Ev)):
        ok, ratio = _within(got, ref, E)
        ratios.append(ratio)
        assert ok, ratio
    print(f"\nn={n} {which}: max |dev - emulation| / bound = {ratios[0]:.2f} (p) {ratios[1]:.2f} (exp_avg) {ratios[2]:.2f} (exp_avg_sq)")


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_guard_off_is_bitwise_the_plain_step(n):
    """max_norm = 0 and finite gradients: the folded scalar is grad_scale itself, so five steps give the bits of mmvae_adam_step_dev."""
    a = ADAM
    p0, grads = _inputs(n)
    run = _Guarded(p0, 0.0)
    lib = run.lib
    p, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    step = torch.zeros(1, dtype=torch.float64, device="cuda")
    for g in grads:
        gd = g.cuda()
        run.step(gd)
        assert lib.mmvae_adam_step_dev(_p(p), _p(gd), _p(m), _p(v), n, a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], _p(step), a["gs"], _st()) == 0
    torch.cuda.synchronize()
    assert step.item() == 5.0 and run.state[0].item() == 5.0
    assert torch.equal(run.p, p) and torch.equal(run.m, m) and torch.equal(run.v, v)


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_step_is_skipped(n):
    """Five calls, the second with an inf at n - 1, the fourth with a NaN at n // 2: those two leave p, m, v bitwise alone and count
    as skipped; the result is the three finite steps with t = 1, 2, 3 (the bias corrections did not advance on the skips)."""
    gs = ADAM["gs"]
    p0, grads = _inputs(n)
    run = _Guarded(p0, 0.0)
    scales = []
    for k, g in enumerate(grads):
        gd = g.cuda()
        if k == 1:
            gd[n - 1] = float("inf")
        if k == 3:
            gd[n // 2] = float("nan")
        before = [x.clone() for x in (run.p, run.m, run.v)]
        run.step(gd)
        if k in (1, 3):
            assert all(torch.equal(x, y) for x, y in zip(before, (run.p, run.m, run.v)))
            total = run.state[1].item()
            assert total == float("inf") if k == 1 else math.isnan(total)
            scales.append(None)
        else:
            scales.append(gs)
    assert run.state.cpu().tolist()[0] == 3.0 and run.state[2].item() == 2.0 and run.state[3].item() == 0.0
    (rp, rm, rv), (Ep, Em, Ev), t = _emulate(p0, grads, scales)
    assert t == 3
    for got, ref, E in zip(run.pmv(), (rp, rm, rv), (Ep, Em, Ev)):
        ok, ratio = _within(got, ref, E)
        assert ok, ratio


@gpu
def test_guarded_step_replays_in_a_graph():
    """One mmvae_adam_step_guarded call (three launches, one stream, one branch) captured with torch.cuda.graph and replayed four
    times on new gradients, the third holding an inf: p, m, v and the state equal the same four calls run eagerly, to the bit."""
    n = 524289
    p0, grads = _inputs(n)
    max_norm = f32(0.9 * math.sqrt(_ref_norm_sq(grads[0], ADAM["gs"])))          # clips: the factor is recomputed on every replay
    feeds = [g.clone() for g in grads[:4]]
    feeds[2][n - 1] = float("inf")
    eager = _Guarded(p0, max_norm)
    for g in feeds:
        eager.step(g.cuda())
    torch.cuda.synchronize()
    cap = _Guarded(p0, max_norm)
    static = torch.zeros(n, device="cuda")
    side = torch.cuda.Stream()                      # warm-up off the capture, then back to the initial state
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.step(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    cap.p.copy_(p0); cap.m.zero_(); cap.v.zero_(); cap.state.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.step(static)
    for g in feeds:
        static.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert cap.state.cpu().tolist() == eager.state.cpu().tolist() and cap.state[0].item() == 3.0 and cap.state[2].item() == 1.0
    assert torch.equal(cap.p, eager.p) and torch.equal(cap.m, eager.m) and torch.equal(cap.v, eager.v)


@gpu
def test_guarded_argument_checks():
    L = _L()
    lib = L.lib()
    x = torch.ones(8, device="cuda")
    p, m, v = torch.ones(8, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    part = torch.zeros(L.SUM_PARTIALS, dtype=torch.float64, device="cuda")
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    st = _st()
    # n == 0: a no-op, with or without state
    assert lib.mmvae_adam_step_guarded(_p(p), _p(x), _p(m), _p(v), 0, *hp, _p(state), _p(part), 1.0, 1.0, st) == 0
    assert lib.mmvae_adam_step_guarded(_p(p), _p(x), _p(m), _p(v), 0, *hp, None, None, 1.0, 1.0, st) == 0
    assert lib.mmvae_grad_norm_sq(_p(x), 0, 1.0, _p(state), _p(part), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), torch.ones(8)) and state.cpu().tolist() == [0.0] * 4 and m.abs().sum().item() == 0.0
    assert lib.mmvae_adam_step_guarded(_p(p), _p(x), _p(m), _p(v), 8, *hp, None, _p(part), 1.0, 1.0, st) == ERR_ARG
    assert lib.mmvae_adam_step_guarded(_p(p), _p(x), _p(m), _p(v), 8, *hp, _p(state), None, 1.0, 1.0, st) == ERR_ARG
    assert lib.mmvae_grad_norm_sq(_p(x), 8, 1.0, None, _p(part), st) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), torch.ones(8))


# ================================================================ GPU, model level
def _M():
    return importlib.import_module("moving-mnist-vae_amd.model")


class _Tiny:
    """The smallest legal VAE (1 channel, z = 8, 16 x 16 images, 4 of them, f32) with injected noise, and one backward on demand."""

    def __init__(self, oracle, **opt_kw):
        M = _M()
        self.dev = torch.device("cuda")
        torch.manual_seed(3)
        self.m = M.VAE(1, 32, 1, 2, 8, False, False, 4, "ReLu", 1, 1, 0, True, 0.1, 16, compute_dtype="f32").to(self.dev).train()
        g = torch.Generator().manual_seed(4)
        self.m.injected_eps = torch.randn(4, 8, 1, 1, generator=g).to(self.dev)
        self.m.injected_true_samples = torch.randn(4, 8, generator=g).to(self.dev)
        self.image = oracle.normalise(oracle.synthetic_labels(4, 16, seed=9), 16).to(self.dev)
        self.args = types.SimpleNamespace(data_ratio_of_labels=None)
        self.opt = M.FusedAdam(list(self.m.parameters()), **opt_kw)

    def backward(self):
        mu, lv, enc, rec = self.m(self.image)
        loss = self.m.loss(self.image, mu, lv, enc, rec, self.dev, self.args)[0]
        self.opt.zero_grad()
        loss.backward()

    def grads(self):
        return torch.cat([p.grad.reshape(-1) for p in self.m.parameters()]).clone()

    def pmv(self):
        return self.m._flat.detach().clone(), self.opt._m.clone(), self.opt._v.clone()


@gpu
def test_fused_adam_guard_that_never_bites_is_the_capturable_step(oracle):
    a, b = _Tiny(oracle, max_grad_norm=1e30), _Tiny(oracle, capturable=True)
    for _ in range(3):
        a.backward(); a.opt.step()
        b.backward(); b.opt.step()
    assert all(torch.equal(x, y) for x, y in zip(a.pmv(), b.pmv()))
    for (ka, pa), (kb, pb) in zip(a.m.named_parameters(), b.m.named_parameters()):
        assert ka == kb and torch.equal(pa, pb), ka
    sa, sb = a.opt.state_dict()["state"], b.opt.state_dict()["state"]
    assert all(torch.equal(sa[i][k], sb[i][k]) for i in sa for k in ("step", "exp_avg", "exp_avg_sq"))
    assert a.opt.skipped_steps == 0 and float(sa[0]["step"]) == 3.0


@gpu
def test_fused_adam_grad_norm_skip_and_resume(oracle):
    """grad_norm after a step is the f64 norm of the concatenated .grads (the summation bound); step() leaves .grad alone; a NaN in one
    .grad element skips the step (parameters, moments, step count unchanged, skipped_steps == 1) and the next finite step proceeds;
    load_flat_state() into a fresh guarded optimiser restores the count on the device."""
    t = _Tiny(oracle, skip_nonfinite=True)
    t.backward()
    G = t.grads()
    t.opt.step()
    n = G.numel()
    ref = G.double().norm().item()
    gn = t.opt.grad_norm
    assert gn.dim() == 0 and gn.dtype == torch.float64 and gn.is_cuda
    assert abs(gn.item() - ref) <= (n + 2) * U64 * ref
    assert torch.equal(t.grads(), G)
    assert t.opt.skipped_steps == 0
    # a poisoned step
    t.backward()
    list(t.m.parameters())[3].grad.view(-1)[0] = float("nan")
    before = t.pmv()
    t.opt.step()
    assert all(torch.equal(x, y) for x, y in zip(before, t.pmv()))
    assert t.opt.skipped_steps == 1 and math.isnan(t.opt.grad_norm.item())
    assert float(t.opt.state_dict()["state"][0]["step"]) == 1.0
    # the next finite one
    t.backward()
    t.opt.step()
    after = t.pmv()
    assert not torch.equal(before[0], after[0]) and torch.isfinite(after[0]).all() and torch.isfinite(after[1]).all()
    sd = t.opt.state_dict()
    assert float(sd["state"][0]["step"]) == 2.0 and t.opt.skipped_steps == 1
    # resume
    r = _Tiny(oracle, skip_nonfinite=True)
    r.opt.load_flat_state(sd)
    assert r.opt._guard[0].item() == 2.0 and r.opt._guard[2].item() == 0.0
    assert torch.equal(r.opt._m, t.opt._m) and torch.equal(r.opt._v, t.opt._v)
    r.m.load_state_dict(t.m.state_dict())
    r.backward(); r.opt.step()
    t.backward(); t.opt.step()
    assert all(torch.equal(x, y) for x, y in zip(r.pmv(), t.pmv()))
    assert float(r.opt.state_dict()["state"][0]["step"]) == 3.0


@gpu
def test_fused_adam_clip_shows_in_exp_avg(oracle):
    """max_grad_norm at half the measured norm, first step from zero moments: exp_avg = (1 - beta1) * s * g with
    s = f32(max_norm / (norm + 1e-6)), to 4 f32 ulps (the kernel: fl(g s), then m = 0 + (g' - 0) * fl(1 - beta1): two roundings and
    the f32 value of 1 - beta1, against the f64 product); .grad is not rewritten."""
    probe = _Tiny(oracle, skip_nonfinite=True)
    probe.backward()
    norm = probe.grads().double().norm().item()
    t = _Tiny(oracle, max_grad_norm=0.5 * norm)
    t.backward()
    G = t.grads()
    t.opt.step()
    assert torch.equal(t.grads(), G)
    total = t.opt.grad_norm.item()
    s = f32(clip_factor(f32(0.5 * norm), total))
    assert 0.49 < s < 0.51
    want = (1.0 - 0.9) * s * G.double()
    got = t.opt._m.double()
    ulp = 2.0 ** -23 * want.abs()
    assert ((got - want).abs() <= 4 * ulp + 2.0 ** -147).all(), ((got - want).abs() / (ulp + 2.0 ** -149)).max().item()
    assert t.opt.skipped_steps == 0 and float(t.opt.state_dict()["state"][0]["step"]) == 1.0
