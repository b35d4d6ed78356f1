"""Device-side autoregressive sampler of the PixelCNN / PixelVAE models (VAE.sample_pixels -> mmvae_pixelcnn_sample; reference main.py:186-202).

One flipped label changes every later pixel, so two samplers are never compared free-running.  Every parity test is TEACHER-FORCED: the
device sampler runs once with return_probs=True; for pixel k the prefix state (pixels < k from the sampler's final sample, the rest from
the initial sample) is rebuilt and the comparison model evaluated on it.  The comparison models are the CPU oracle
(oracle.vae_oracle.pixelcnn_forward, pinned to the reference by the committed goldens) and the product's own generic forward
(run_pixelcnn).

Bounds (none of them measured on the code under test):
  logits   f32: 2e-3 * max|logit|, the project's f32 bound for PixelCNN logits (TOL["f32"]["recon"] of tests/test_pixelcnn.py);
           bf16 against the product's forward: that plus one bf16 rounding, 2^-8 * max|logit| (the generic path stores its logits in bf16,
           the head keeps f32).
  probs    the probability of any set of classes is 1/2-Lipschitz in the logits' max norm (its gradient has L1 norm 2 P (1 - P) <= 1/2),
           so |d prob|, |d cdf| <= logit bound / 2.
  labels   must equal draw_labels(comparison probs, u) wherever every |u - cdf_k| > delta, delta = the logit bound (twice the cdf bound);
           draws closer to a boundary are left out, and against the oracle at most 5 % of all draws may be left out.
"""
import importlib
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32_LOGIT = 2e-3                   # x max|logit|
BF16_LOGIT = 2e-3 + 2.0 ** -8      # x max|logit|
MAX_LEFT_OUT = 0.05
LAYERS, MID = 3, 16

# (S, Q, N, seed of the uniforms).  The seeds are chosen so that the ORACLE, run as a free sampler on the CPU with the same draw rule, leaves
# out well under 5 % of its draws (test_oracle_free_sampler_leaves_out_few_draws; with Q - 1 boundaries and delta = 2e-3 * max|logit| ~ 6e-3
# the expected share is 2 (Q - 1) delta, i.e. about 1 % for Q = 2 and 4 % for Q = 4).  Observed there: (8, 2, seed 1) 1.56 %,
# (8, 4, seed 4) 1.04 %, (12, 2, seed 2) 0.00 %, (12, 4, seed 5) 2.31 %  [seed 1 gives 5.09 % for (12, 4): not used.  The issue
# quotes 1.4 % for that recipe; with its stated delta = 2e-3 * max|logit| = 6.6e-3 and three boundaries the expected share is 4 %, so that
# figure must come from a narrower margin than the one it specifies -- the specified one is what is used here].
ONLY_CASES = [(8, 2, 3, 1), (8, 4, 3, 4), (12, 2, 3, 2), (12, 4, 3, 5)]
# PixelVAE VAE(1, 16, 2, 2, 32, True, False, 3, ..., input_image_size=32), N = 2, seed 1: observed 1.07 % (z_image from the oracle's eval-mode decoder)
VAE_SEED, VAE_N, VAE_S, VAE_Z = 1, 2, 32, 32


def _model_module():
    return importlib.import_module("moving-mnist-vae_amd.model")


def _uniforms(N, S, seed):
    torch.manual_seed(seed)
    return torch.rand(N, S * S)


def _pixels(S, which=None):
    return list(range(S * S)) if which is None else list(which)


def _prefix_states(initial, final, pixels):
    """[len(pixels) * N, C, S, S]: for each pixel k the sample with pixels < k (row-major) taken from `final`, the rest from `initial`."""
    N, C, S, _ = initial.shape
    out = []
    for k in pixels:
        st = initial.clone().view(N, C, S * S)
        st[:, :, :k] = final.view(N, C, S * S)[:, :, :k]
        out.append(st.view(N, C, S, S))
    return torch.cat(out, 0)


def _forced_logits(forward, cond, initial, final, pixels, chunk=32):
    """Teacher-forced logits [len(pixels), N, Q] of `forward` (an (M, C, S, S) -> (M, Q, S, S) map; InstanceNorm is per image, so prefix
    states of several pixels share a batch) at each pixel of `pixels`, on that pixel's prefix state."""
    N, _, S, _ = initial.shape
    rows = []
    for c0 in range(0, len(pixels), chunk):
        pk = pixels[c0:c0 + chunk]
        x = _prefix_states(initial, final, pk)
        if cond is not None:
            x = torch.cat([cond.repeat(len(pk), 1, 1, 1), x], dim=1)
        lg = forward(x)
        for t, k in enumerate(pk):
            rows.append(lg[t * N:(t + 1) * N, :, k // S, k % S])
    return torch.stack(rows, 0)


def _compare(pkg, logits_ref, probs, labels, u, pixels, logit_rel, what):
    """probs [N, S*S, Q], labels [N, S*S] of the device sampler against teacher-forced comparison logits [P, N, Q].  Returns the share of
    draws left out of the label comparison."""
    logits_ref = logits_ref.double()
    bound = logit_rel * float(logits_ref.abs().max())
    p_ref = torch.softmax(logits_ref, dim=-1)                                 # [P, N, Q]
    p_dev = probs[:, pixels, :].permute(1, 0, 2).double()
    l_dev = labels[:, pixels].t()
    uu = u[:, pixels].t().double()
    perr = float((p_dev - p_ref).abs().max())
    print(f"{what}: max|logit| {float(logits_ref.abs().max()):.3f}, max|d prob| {perr:.3e} (bound {bound / 2:.3e})")
    assert perr <= bound / 2, (what, perr, bound / 2)
    cdf = torch.cumsum(p_ref, dim=-1)[..., :-1]
    clear = ((uu.unsqueeze(-1) - cdf).abs() > bound).all(dim=-1)
    want = pkg.draw_labels(p_ref, uu)
    left_out = 1.0 - float(clear.double().mean())
    wrong = int((l_dev[clear] != want[clear]).sum())
    print(f"{what}: {left_out:.2%} of {clear.numel()} draws within {bound:.2e} of a cdf boundary, {wrong} wrong labels")
    assert wrong == 0, (what, wrong)
    return left_out


def _only_state(O, Q, S):
    spec = O.pixelcnn_spec(1, MID, Q, LAYERS, "pixelcnn.")
    return spec, O.filled_state(spec, seed=0)


def _vae_state(O):
    spec = O.pixelcnn_spec(2 + 1, MID, 2, LAYERS) + O.state_spec(1, VAE_Z, 2, VAE_S, True)
    return spec, O.filled_state(spec, seed=0)


def _vae_encoding():
    torch.manual_seed(7)
    return torch.randn(VAE_N, VAE_Z, 1, 1)


def _free_sampler_left_out(O, pkg, sd, cond, N, S, Q, u, sub_mean):
    """The oracle as a free sampler on the CPU (zero initial sample, the product's draw rule): share of draws within delta of a boundary."""
    sample = torch.zeros(N, 1, S, S)
    logits = torch.empty(S * S, N, Q)
    for k in range(S * S):
        x = sample if cond is None else torch.cat([cond, sample], dim=1)
        lg = O.pixelcnn_forward(sd, x, LAYERS)[:, :, k // S, k % S]
        logits[k] = lg
        lab = pkg.draw_labels(torch.softmax(lg, dim=1), u[:, k])
        sample[:, :, k // S, k % S] = ((lab.float() - sub_mean) / O.DATA_STD).unsqueeze(1)
    delta = F32_LOGIT * float(logits.abs().max())
    cdf = torch.cumsum(torch.softmax(logits.double(), dim=-1), dim=-1)[..., :-1]
    close = ((u.t().double().unsqueeze(-1) - cdf).abs() <= delta).any(dim=-1)
    return float(close.double().mean()), float(logits.abs().max())


# ------------------------------------------------------------------------------------------------------------------------ CPU

def test_library_and_header_expose_the_sampler():
    L = importlib.import_module("moving-mnist-vae_amd._lib")
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for name in ("mmvae_pixelcnn_sample_workspace_bytes", "mmvae_pixelcnn_sample"):
        assert name in L.PROTOTYPES
        assert getattr(lib, name) is not None
        assert re.search(r"MMVAE_API\s+[\w\s\*]+\b" + name + r"\s*\(", header), name
    assert lib.mmvae_abi_version() == 3


@pytest.mark.parametrize("Q", [2, 4, 16])
def test_draw_labels_is_searchsorted_of_the_cdf(pkg, Q):
    rng = np.random.default_rng(Q)
    probs = rng.random((257, Q)).astype(np.float32) + 1e-3
    probs /= probs.sum(1, keepdims=True)
    u = rng.random(257).astype(np.float32)
    u[0], u[1], u[2] = 0.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 0.0
    probs[2] = 0.0
    probs[2, Q - 1] = 1.0                                    # leading zero-probability classes are never drawn, u = 0 included
    got = pkg.draw_labels(torch.from_numpy(probs), torch.from_numpy(u))
    assert got.dtype == torch.int64 and tuple(got.shape) == (257,)
    cdf = np.cumsum(probs, axis=1, dtype=np.float32)
    want = np.array([np.searchsorted(cdf[r, :-1], u[r], side="right") for r in range(257)])
    assert np.array_equal(got.numpy(), want)
    assert got.min() >= 0 and got.max() <= Q - 1 and int(got[2]) == Q - 1
    # batched leading axes
    got2 = pkg.draw_labels(torch.from_numpy(probs).view(1, 257, Q).expand(3, 257, Q), torch.from_numpy(u).expand(3, 257))
    assert torch.equal(got2, got.expand(3, 257))


class _StubModel:
    """What generate / generate_only_pixelcnn need of a model, on the CPU: zero logits."""

    def __init__(self, S, Q):
        self.input_image_size, self.Q, self.calls, self.sampled = S, Q, 0, []

    def run_pixelcnn(self, x):
        self.calls += 1
        return torch.zeros(x.shape[0], self.Q, x.shape[2], x.shape[3])

    def sample_pixels(self, sample, z_image=None, **kw):
        self.sampled.append((z_image, kw))
        return "out", sample


def test_generate_default_path_is_the_reference_loop(pkg, monkeypatch):
    S, Q, N = 3, 4, 2
    calls = []
    real = torch.multinomial

    def counting(probs, n, *a, **k):
        calls.append(tuple(probs.shape))
        return real(probs, n, *a, **k)

    monkeypatch.setattr(torch, "multinomial", counting)
    for only in (False, True):
        m = _StubModel(S, Q)
        del calls[:]
        sample = torch.zeros(N, 1, S, S)
        torch.manual_seed(3)
        if only:
            out, smp = pkg.generate_only_pixelcnn(sample, m, 0.05, 0.2, uniforms=None)
        else:
            out, smp = pkg.generate(torch.zeros(N, 2, S, S), sample, m, 0.05, 0.2, uniforms=None)
        assert calls == [(N, Q)] * (S * S) and m.calls == S * S and not m.sampled
        assert smp is sample and tuple(out.shape) == (N, Q, S, S)
        # the global RNG is consumed exactly as by the plain loop
        torch.manual_seed(3)
        want = torch.stack([real(torch.full((N, Q), 1.0 / Q), 1) for _ in range(S * S)], 0).view(S, S, N).permute(2, 0, 1).float()
        assert torch.equal(smp[:, 0], (want - (0.0 if only else 0.05)) / 0.2)
    # with uniforms both delegate to sample_pixels
    m, u = _StubModel(S, Q), torch.rand(N, S * S)
    z = torch.zeros(N, 2, S, S)
    assert pkg.generate(z, sample, m, 0.05, 0.2, uniforms=u) == ("out", sample)
    assert pkg.generate_only_pixelcnn(sample, m, 0.05, 0.2, uniforms=True) == ("out", sample)
    assert m.calls == 0 and m.sampled[0][0] is z and m.sampled[0][1] == dict(data_mean=0.05, data_std=0.2, uniforms=u)
    assert m.sampled[1][0] is None and m.sampled[1][1] == dict(data_mean=0.05, data_std=0.2, uniforms=None)


@pytest.mark.parametrize("S,Q,N,seed", ONLY_CASES)
def test_oracle_free_sampler_leaves_out_few_draws(pkg, oracle, S, Q, N, seed):
    """The 5 % cap of the GPU parity test is a condition on the seeds: the oracle alone must meet it."""
    _, sd = _only_state(oracle, Q, S)
    share, mx = _free_sampler_left_out(oracle, pkg, sd, None, N, S, Q, _uniforms(N, S, seed), 0.0)
    print(f"S {S} Q {Q}: max|logit| {mx:.2f}, {share:.2%} left out")
    assert share <= MAX_LEFT_OUT


def test_oracle_free_sampler_leaves_out_few_draws_pixelvae(pkg, oracle):
    _, sd = _vae_state(oracle)
    z_image = oracle.get_reconstruction(sd, _vae_encoding(), VAE_S, training=False)
    share, mx = _free_sampler_left_out(oracle, pkg, sd, z_image, VAE_N, VAE_S, 2, _uniforms(VAE_N, VAE_S, VAE_SEED), oracle.DATA_MEAN)
    print(f"PixelVAE: max|logit| {mx:.2f}, {share:.2%} left out")
    assert share <= MAX_LEFT_OUT


# ------------------------------------------------------------------------------------------------------------------------ GPU

def _only_model(O, Q, S, dt, layers=LAYERS, mid=MID, state=True):
    M = _model_module()
    m = M.VAE(1, mid, 1, Q, 32, True, True, layers, "ReLu", 1, 1, 0, True, 0.0, S, compute_dtype=dt)
    sd = None
    if state:
        sd = O.filled_state(O.pixelcnn_spec(1, mid, Q, layers, "pixelcnn."), seed=0)
        m.load_state_dict(sd)
    return m.to("cuda").eval(), sd


def _vae_model(O, dt, S=VAE_S, layers=LAYERS, mid=MID, state=True):
    M = _model_module()
    m = M.VAE(1, mid, 2, 2, VAE_Z, True, False, layers, "ReLu", 1, 1, 0, True, 0.0, S, compute_dtype=dt)
    sd = None
    if state:
        _, sd = _vae_state(O)
        m.load_state_dict(sd)
    return m.to("cuda").eval(), sd


def _check_written_values(sample, labels, sub_mean, data_std, initial):
    # the correctly rounded f32 quotient, as the input pipeline's kernels and the oracle's normalise() give it: computed on the CPU (torch on the
    # GPU multiplies by the reciprocal of a scalar divisor, which is up to one unit in the last place off)
    N, C, S, _ = sample.shape
    want = (labels.cpu().view(N, 1, S, S).float() - sub_mean) / data_std
    assert torch.equal(sample.cpu(), want.expand(N, C, S, S))
    assert sample.data_ptr() == initial.data_ptr()                    # in place


@pytest.mark.gpu
@pytest.mark.parametrize("S,Q,N,seed", ONLY_CASES)
def test_sampler_matches_oracle_pixelcnn_only(pkg, oracle, S, Q, N, seed):
    O = oracle
    m, sd = _only_model(O, Q, S, "f32")
    u = _uniforms(N, S, seed)
    initial = torch.zeros(N, 1, S, S)
    smp = initial.clone().cuda()
    out, got, probs, labels = m.sample_pixels(smp, None, data_mean=O.DATA_MEAN, data_std=O.DATA_STD, uniforms=u.cuda(), return_probs=True)
    assert got is smp
    _check_written_values(got, labels, 0.0, O.DATA_STD, smp)          # PixelCNN-only: the mean is not subtracted (main.py:191)
    final, probs, labels = got.cpu(), probs.cpu(), labels.cpu()
    fwd = lambda x: O.pixelcnn_forward(sd, x, LAYERS)
    ref = _forced_logits(fwd, None, initial, final, _pixels(S))
    left = _compare(pkg, ref, probs, labels, u, _pixels(S), F32_LOGIT, f"only S{S} Q{Q} vs oracle")
    assert left <= MAX_LEFT_OUT, left
    # the returned logits: the full forward on the state before the last pixel was written
    last = _prefix_states(initial, final, [S * S - 1])
    full = fwd(last)
    err = float((out.cpu() - full).abs().max())
    assert err <= F32_LOGIT * float(full.abs().max()), err


@pytest.mark.gpu
def test_sampler_matches_oracle_pixelvae(pkg, oracle):
    O = oracle
    m, sd = _vae_model(O, "f32")
    N, S = VAE_N, VAE_S
    with torch.no_grad():
        z_image = m.get_z_image(_vae_encoding().cuda())
    u = _uniforms(N, S, VAE_SEED)
    initial = torch.zeros(N, 1, S, S)
    smp = initial.clone().cuda()
    out, got, probs, labels = m.sample_pixels(smp, z_image, data_mean=O.DATA_MEAN, data_std=O.DATA_STD, uniforms=u.cuda(), return_probs=True)
    _check_written_values(got, labels, O.DATA_MEAN, O.DATA_STD, smp)
    final, probs, labels, zc = got.cpu(), probs.cpu(), labels.cpu(), z_image.cpu().float()
    fwd = lambda x: O.pixelcnn_forward(sd, x, LAYERS)
    ref = _forced_logits(fwd, zc, initial, final, _pixels(S))
    left = _compare(pkg, ref, probs, labels, u, _pixels(S), F32_LOGIT, "PixelVAE vs oracle")
    assert left <= MAX_LEFT_OUT, left
    full = fwd(torch.cat([zc, _prefix_states(initial, final, [S * S - 1])], dim=1))
    err = float((out.cpu() - full).abs().max())
    assert err <= F32_LOGIT * float(full.abs().max()), err


def _border_pixels(S):
    """64 pixels of an S x S map (S >= 16): corners, points along the four borders and a diagonal."""
    e = S - 1
    px = {(0, 0), (0, e), (e, 0), (e, e)}
    step = max(1, S // 8)
    for t in range(1, S, step):
        px |= {(0, t), (e, t), (t, 0), (t, e), (t, t), (t, e - t)}
    px |= {(1, 1), (2, 2), (2, 3), (3, 2), (3, 3), (3, 4), (4, 4), (3, e), (3, e - 3), (e - 1, e - 1), (e - 3, 2), (2, e - 3), (e - 2, e - 3)}
    out = sorted(i * S + j for i, j in px)
    assert len(out) == 64, len(out)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", ["only_S12_Q4", "vae_S32", "vae_S64_L4_M32"])
def test_sampler_matches_generic_forward(pkg, oracle, case, dt):
    """Staging, pixel order, tap geometry at the borders and the head arithmetic against the tested generic path (run_pixelcnn)."""
    O = oracle
    torch.manual_seed(0)
    if case == "only_S12_Q4":
        N, S = 3, 12
        (m, _), z_image, sub_mean, pixels = _only_model(O, 4, S, dt), None, 0.0, _pixels(S)
    elif case == "vae_S32":
        N, S = 2, 32
        m, _ = _vae_model(O, dt)
        pixels, sub_mean = _pixels(S), O.DATA_MEAN
    else:
        N, S = 2, 64
        m, _ = _vae_model(O, dt, S=64, layers=4, mid=32, state=False)          # the constructor's (seeded) initialisation
        pixels, sub_mean = _border_pixels(S), O.DATA_MEAN
    if case != "only_S12_Q4":
        with torch.no_grad():
            z_image = m.get_z_image(torch.randn(N, VAE_Z, 1, 1, device="cuda")).float()
    u = _uniforms(N, S, 1)
    initial = (O.synthetic_labels(N, S, seed=9).float().view(N, 1, S, S) - sub_mean) / O.DATA_STD      # a non-trivial initial sample
    smp = initial.clone().cuda()
    out, got, probs, labels = m.sample_pixels(smp, z_image, data_mean=O.DATA_MEAN, data_std=O.DATA_STD, uniforms=u.cuda(), return_probs=True)
    _check_written_values(got, labels, sub_mean, O.DATA_STD, smp)
    final = got.cpu()

    def fwd(x):
        with torch.no_grad():
            return m.run_pixelcnn(x.cuda()).cpu()

    ref = _forced_logits(fwd, None if z_image is None else z_image.cpu(), initial, final, pixels, chunk=1)       # the sampler's own batch size: the same launches
    rel = F32_LOGIT if dt == "f32" else BF16_LOGIT
    _compare(pkg, ref, probs.cpu(), labels.cpu(), u, pixels, rel, f"{case} {dt} vs run_pixelcnn")
    # the labels follow the recorded probabilities by the published rule (cumulative sums of Q f32 values: (Q - 1) roundings of 2^-24 each)
    Q = probs.shape[-1]
    cdf = torch.cumsum(probs.cpu().double(), dim=-1)[..., :-1]
    clear = ((u.double().unsqueeze(-1) - cdf).abs() > Q * 2.0 ** -23).all(dim=-1)
    assert float(clear.double().mean()) > 0.99
    assert torch.equal(labels.cpu()[clear], pkg.draw_labels(probs.cpu().double(), u.double())[clear])
    last = _prefix_states(initial, final, [S * S - 1])
    full = fwd(last if z_image is None else torch.cat([z_image.cpu(), last], dim=1))
    assert float((out.cpu() - full).abs().max()) <= rel * float(full.abs().max())


@pytest.mark.gpu
def test_sampler_distribution(pkg, oracle):
    """All weights zero, last bias b: every pixel's distribution is softmax(b); the label histogram over N * S * S = 10 240 draws is within 4
    binomial standard deviations of it per class."""
    Q, S, N = 4, 32, 10
    m, _ = _only_model(oracle, Q, S, "f32", state=False)
    b = torch.tensor([0.3, -1.1, 1.2, 0.0])
    with torch.no_grad():
        for p in m.parameters():
            p.zero_()
        m.state_dict()[f"pixelcnn.layers.{LAYERS - 1}.bias"].copy_(b)
    u = _uniforms(N, S, 11)
    smp = torch.zeros(N, 1, S, S, device="cuda")
    _, _, probs, labels = m.sample_pixels(smp, data_mean=0.0, data_std=1.0, uniforms=u.cuda(), return_probs=True)
    p = torch.softmax(b.double(), 0)
    # f32 rounding: exp, the sum of four terms and the division, a few units of 2^-24 relative on values <= 1
    assert float((probs.cpu().double() - p).abs().max()) <= 1e-6
    n = N * S * S
    assert n >= 10000
    hist = torch.bincount(labels.cpu().flatten(), minlength=Q).double()
    sd = torch.sqrt(n * p * (1 - p))
    print("histogram", hist.tolist(), "expected", (n * p).tolist(), "sd", sd.tolist())
    assert bool(((hist - n * p).abs() <= 4 * sd).all()), (hist, n * p, sd)
    assert torch.equal(smp.cpu().view(N, -1), labels.cpu().float())


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_sampler_is_deterministic_and_keeps_masked_parameters(pkg, oracle, dt):
    O = oracle
    m, sd = _vae_model(O, dt)
    N, S = VAE_N, VAE_S
    with torch.no_grad():
        z_image = m.get_z_image(_vae_encoding().cuda())
    u = _uniforms(N, S, 2).cuda()
    runs = [m.sample_pixels(torch.zeros(N, 1, S, S, device="cuda"), z_image, data_mean=O.DATA_MEAN, data_std=O.DATA_STD, uniforms=u, return_probs=True)
            for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    for i in range(LAYERS):
        w = m.state_dict()[f"pixelcnn.layers.{i}.weight"].cpu()
        assert torch.equal(w, sd[f"pixelcnn.layers.{i}.weight"] * sd[f"pixelcnn.layers.{i}.mask"])
        assert torch.equal(m.state_dict()[f"pixelcnn.layers.{i}.bias"].cpu(), sd[f"pixelcnn.layers.{i}.bias"])
    # generate(..., uniforms=u) is sample_pixels; two returned values without return_probs
    g_out, g_smp = pkg.generate(z_image, torch.zeros(N, 1, S, S, device="cuda"), m, O.DATA_MEAN, O.DATA_STD, uniforms=u)
    assert torch.equal(g_out, runs[0][0]) and torch.equal(g_smp, runs[0][1])
    # uniforms=True / None: drawn with torch.rand, reproducible through the generator
    gen = torch.Generator(device="cuda")
    outs = []
    for _ in range(2):
        gen.manual_seed(5)
        outs.append(m.sample_pixels(torch.zeros(N, 1, S, S, device="cuda"), z_image, data_mean=O.DATA_MEAN, data_std=O.DATA_STD, generator=gen)[1])
    assert torch.equal(outs[0], outs[1])
    # a non-contiguous / non-f32 sample is still updated in place
    wide = torch.zeros(N, 1, S, 2 * S, device="cuda", dtype=torch.float64)
    view = wide[:, :, :, ::2]
    m.sample_pixels(view, z_image, data_mean=O.DATA_MEAN, data_std=O.DATA_STD, uniforms=u)
    assert torch.equal(view.float(), runs[0][1]) and float(wide[:, :, :, 1::2].abs().max()) == 0.0


@pytest.mark.gpu
def test_generate_only_pixelcnn_delegates(pkg, oracle):
    O = oracle
    m, _ = _only_model(O, 2, 8, "f32")
    u = _uniforms(3, 8, 1).cuda()
    a = m.sample_pixels(torch.zeros(3, 1, 8, 8, device="cuda"), data_mean=O.DATA_MEAN, data_std=O.DATA_STD, uniforms=u)
    b = pkg.generate_only_pixelcnn(torch.zeros(3, 1, 8, 8, device="cuda"), m, O.DATA_MEAN, O.DATA_STD, uniforms=u)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # and the default path still is the reference's loop over run_pixelcnn (same distribution: values are labels / std)
    torch.manual_seed(0)
    out, smp = pkg.generate_only_pixelcnn(torch.zeros(3, 1, 8, 8, device="cuda"), m, O.DATA_MEAN, O.DATA_STD)
    assert tuple(out.shape) == (3, 2, 8, 8) and set((smp * O.DATA_STD).round().flatten().tolist()) <= {0.0, 1.0}


def _train_step(m, opt, labels, O, args):
    dev = torch.device("cuda")
    image, target = m.prepare_batch(labels, dev, O.DATA_MEAN, O.DATA_STD, True)
    out = m(image)
    loss = m.loss(target, *out, dev, args)[0]
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss.detach())


@pytest.mark.gpu
def test_sampler_and_training_do_not_disturb_each_other(pkg, oracle):
    O = oracle
    M = _model_module()
    dev = torch.device("cuda")
    args = types.SimpleNamespace(data_ratio_of_labels=torch.ones(2), dataset="MovingMNIST", quiet=True)
    labels = O.synthetic_labels(4, VAE_S, seed=5).view(4, VAE_S * VAE_S)
    u = _uniforms(4, VAE_S, 3).cuda()
    results = []
    for with_sampler in (False, True):
        m, _ = _vae_model(O, "bf16")
        m.train()
        torch.manual_seed(21)
        m.injected_eps = torch.randn(4, VAE_Z, 1, 1, device=dev)
        opt = M.FusedAdam(list(m.parameters()))
        if with_sampler:
            z_image = torch.full((4, 2, VAE_S, VAE_S), 0.25, device=dev)
            m.sample_pixels(torch.zeros(4, 1, VAE_S, VAE_S, device=dev), z_image, data_mean=O.DATA_MEAN, data_std=O.DATA_STD, uniforms=u)
        loss = _train_step(m, opt, labels, O, args)
        results.append((loss, {k: v.detach().clone() for k, v in m.state_dict().items()}))
    assert results[0][0] == results[1][0]
    for k, v in results[0][1].items():
        assert torch.equal(v, results[1][1][k]), k
    # a backward through a forward taken BEFORE a sampling call: the workspace is gone
    m, _ = _vae_model(O, "bf16")
    m.train()
    image, target = m.prepare_batch(labels, dev, O.DATA_MEAN, O.DATA_STD, True)
    out = m(image)
    loss = m.loss(target, *out, dev, args)[0]
    with torch.no_grad():
        z_image = out[3].new_zeros(4, 2, VAE_S, VAE_S)
    m.sample_pixels(torch.zeros(4, 1, VAE_S, VAE_S, device=dev), z_image, data_mean=O.DATA_MEAN, data_std=O.DATA_STD, uniforms=u)
    with pytest.raises(M.MmvaeError, match="overwritten by a later forward"):
        loss.backward()


@pytest.mark.gpu
def test_sampler_argument_errors(pkg, oracle):
    O = oracle
    M = _model_module()
    m, _ = _vae_model(O, "f32")
    N, S = 2, VAE_S
    u = _uniforms(N, S, 1).cuda()
    z = torch.zeros(N, 2, S, S, device="cuda")
    smp = torch.zeros(N, 1, S, S, device="cuda")
    before = smp.clone()
    with pytest.raises(M.MmvaeError, match=r"2 conditioning \+ 2 sample channels, the net takes 3"):
        m.sample_pixels(torch.zeros(N, 2, S, S, device="cuda"), z, data_mean=0.0, data_std=1.0, uniforms=u)
    with pytest.raises(M.MmvaeError, match="data_std must not be zero"):
        m.sample_pixels(smp, z, data_mean=0.0, data_std=0.0, uniforms=u)
    assert torch.equal(smp, before)                                      # nothing was enqueued
    with pytest.raises(ValueError):
        m.sample_pixels(smp, None, data_mean=0.0, data_std=1.0, uniforms=u)              # a PixelVAE needs z_image
    with pytest.raises(ValueError):
        m.sample_pixels(smp, z, data_mean=0.0, data_std=1.0, uniforms=u[:, :-1])
    mo, _ = _only_model(O, 2, 8, "f32")
    with pytest.raises(ValueError):
        mo.sample_pixels(torch.zeros(1, 1, 8, 8, device="cuda"), torch.zeros(1, 1, 8, 8, device="cuda"), data_mean=0.0, data_std=1.0)
    # the C entry itself: workspace too small, null uniforms
    L = importlib.import_module("moving-mnist-vae_amd._lib")
    lib = L.lib()
    need = lib.mmvae_pixelcnn_sample_workspace_bytes(mo._hp, 1, 8)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    s8, u8 = torch.zeros(1, 1, 8, 8, device="cuda"), torch.rand(1, 64, device="cuda")
    args = lambda uni, nbytes: (mo._hp, 1, 8, None, 0, s8.data_ptr(), 1, uni, 0.0, 1.0, mo._flat.data_ptr(), ws.data_ptr(), nbytes, None, None, None, None)
    assert lib.mmvae_pixelcnn_sample(*args(u8.data_ptr(), need - 1)) == -3 and b"workspace too small" in lib.mmvae_last_error()
    assert lib.mmvae_pixelcnn_sample(*args(None, need)) == -1
    assert lib.mmvae_pixelcnn_sample(*args(u8.data_ptr(), need)) == 0
    torch.cuda.synchronize()
