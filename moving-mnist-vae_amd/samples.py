"""Sample-quality scores on the device: do the frames a model draws look like held-out frames, and do they cover them?

Every score here is a function of exact nearest-neighbour relations between a set of real frames and a set of samples, in pixel space
(on 64 x 64 one-channel frames no pretrained network is needed): the leave-one-out 1-NN two-sample accuracy (Lopez-Paz & Oquab 2017),
precision and recall by k-NN balls (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020).  The relations come from
``mmvae_knn_cross``: a tiled int8 GEMM on the matrix unit with a selection epilogue, exact integer squared distances, no N x N matrix
and no floating point.  ``cross_neighbours`` and ``ball_counts`` are that call; ``sample_quality`` is four sweeps and a few f64 tensor
operations; ``sample_frames`` draws the samples as the very bytes the ``normal_sampling`` sheet of ``plot_vae`` shows.
"""
import torch

from . import _lib as L
from .neighbours import _cross_args, _cross_launch, _lut256, _rows_u8, ball_counts, cross_neighbours  # noqa: F401
from .panels import _decoder_column, _draw, _fit_planes, _plot_mode, _plot_setup, render_sheet

SAMPLE_QUALITY_KEYS = ("precision", "recall", "density", "coverage", "accuracy", "accuracy_real", "accuracy_fake")


def _ratio(num, den):
    """num / den in f64 on the device, the correctly rounded quotient of two exact integers (a tensor divided by a Python number is
    multiplied by a rounded reciprocal there)."""
    return num.to(torch.float64) / torch.full((), float(den), dtype=torch.float64, device=num.device)


def sample_quality(real, fake, k=3, lut=None):
    """How close a set of samples ``fake`` is to a set of real frames ``real``, and how much of it they cover: a dict of 0-dim f64 device
    tensors (``sample_quality_to_host`` reads them in one copy).  Write R, F for the sets, d for the squared byte distance and
    ``NND_k(x in S)`` for the distance from x to its k-th nearest neighbour in its own set S, x itself excluded.  All comparisons exact.

      ``precision`` = mean over f of [ exists r : d(f, r) <= NND_k(r) ]      samples that fall into the real manifold's k-NN balls
      ``recall``    = mean over r of [ exists f : d(r, f) <= NND_k(f) ]      the same with the roles swapped
      ``density``   = (1 / (k |F|)) sum over f of #{ r : d(f, r) <= NND_k(r) }
      ``coverage``  = mean over r of [ min_f d(r, f) <= NND_k(r) ]
      ``accuracy``, ``accuracy_real``, ``accuracy_fake``: the leave-one-out 1-NN classifier on the pooled set cat(real, fake) -- a point is
        classified by its nearest OTHER point; ties are resolved by the kernel's order (d, pooled index) with ``real`` first, so at equal
        distance a real neighbour wins over a fake one.  Near 0.5 the sets are indistinguishable, near 1 separable, below 0.5 the samples
        sit on top of the data (``fake`` an exact copy of ``real``: 0).

    Four sweeps (R x R and F x F leave-one-out for the radii, R x F in both directions with the ball counts); the pooled 1-NN follows from
    them without a concatenated copy.  ``real`` / ``fake`` as the sides of ``cross_neighbours``, each with more than ``k`` rows.  ``lut``
    (256 uint8) maps ``real`` into the samples' space by one gather before the sweeps -- ``gray_lut(Q, centres)[fit.lut]`` turns raw
    bytes into the dequantised greys a model trained on k-means labels draws (the case ``nearest_frames`` documents).
    Two limits.  The estimates depend on |R|, |F| and k: compare them only at equal sizes.  This is pixel space: a one-pixel shift of a
    digit counts as distance."""
    what = "sample_quality"
    k = int(k)
    if k < 1:
        raise ValueError(f"{what}: k={k} unsupported (1..{L.KNN_CROSS_MAX_K})")
    if lut is not None:
        lut = _lut256(lut, what)
    R, F = _rows_u8(real, "real", what)[0], _rows_u8(fake, "fake", what)[0]
    for t, name in ((R, "real"), (F, "fake")):
        if t.shape[0] < k + 1:
            raise ValueError(f"{what}: k={k} neighbours inside {name} need more than k rows, got {t.shape[0]}")
    R, F, _ = _cross_args(R, F, k, False, None, what)
    if lut is not None:
        R = lut.to(R.device)[R.long()]
    nr, nf = R.shape[0], F.shape[0]
    d_rr = _cross_launch(R, R, k, True, None)[0]
    d_ff = _cross_launch(F, F, k, True, None)[0]
    nnd_r, nnd_f = d_rr[:, k - 1].contiguous(), d_ff[:, k - 1].contiguous()
    d_fr, _, in_real = _cross_launch(F, R, 1, False, nnd_r)              # per sample: nearest real frame, real balls it lies in
    d_rf, _, in_fake = _cross_launch(R, F, 1, False, nnd_f)
    right_real = (d_rr[:, 0] <= d_rf[:, 0]).sum()                       # a tie goes to the lower pooled index: the real neighbour
    right_fake = (d_ff[:, 0] < d_fr[:, 0]).sum()
    return {"precision": _ratio((in_real > 0).sum(), nf), "recall": _ratio((in_fake > 0).sum(), nr),
            "density": _ratio(in_real.sum(dtype=torch.int64), k * nf), "coverage": _ratio((d_rf[:, 0] <= nnd_r).sum(), nr),
            "accuracy": _ratio(right_real + right_fake, nr + nf), "accuracy_real": _ratio(right_real, nr),
            "accuracy_fake": _ratio(right_fake, nf)}


def sample_quality_to_host(scores):
    """The dict of ``sample_quality`` as Python floats, in ONE device-to-host copy."""
    flat = torch.stack([scores[key] for key in SAMPLE_QUALITY_KEYS]).tolist()
    return dict(zip(SAMPLE_QUALITY_KEYS, flat))


def sample_frames(model, n, data_mean, data_std, centres=None, generator=None, z=None, batch=512):
    """``n`` samples of a plain VAE (either decoder) as grey bytes, uint8 (n, S, S) on the model's device: ``get_reconstruction(z)`` of
    ``z ~ N(0, I)`` (drawn through ``generator``, or the given ``z`` (n, z_dimensions[, 1, 1])), rendered by the very column the
    ``normal_sampling`` sheet of ``plot_vae`` draws -- ``_plot_setup`` and ``_decoder_column`` through one-column ``render_sheet`` calls
    of ``batch`` rows -- so ``sample_quality`` measures the picture one would see.  Eval mode under ``no_grad``; the model's mode is
    restored and nothing in it changes.  PixelCNN / PixelVAE models draw pixel by pixel: use ``model.sample_pixels``, whose drawn labels
    through ``gray_lut(Q, centres)`` are the bytes."""
    n, batch = int(n), int(batch)
    if n < 1 or batch < 1:
        raise ValueError(f"sample_frames: n={n} and batch={batch} must be positive")
    if getattr(model, "pixelcnn", None) is not None or getattr(model, "only_pixelcnn", False):
        raise ValueError("sample_frames serves a plain VAE; a PixelCNN / PixelVAE draws with model.sample_pixels")
    if model.in_channels != 1:
        raise ValueError(f"sample_frames: in_channels={model.in_channels}, a grey frame has one channel")
    device = next(model.parameters()).device
    zd, S = int(model.z_dimensions), int(model.input_image_size)
    if z is not None:
        if not isinstance(z, torch.Tensor) or z.numel() != n * zd or z.shape[0] != n:
            raise ValueError(f"sample_frames: z of shape {tuple(getattr(z, 'shape', ()))} for n={n} codes of {zd} dimensions")
        z = z.detach().to(device=device, dtype=torch.float32).reshape(n, zd, 1, 1)
    out = torch.empty((n, S, S), dtype=torch.uint8, device=device)
    with _plot_mode(model):
        lo, hi, lut = _plot_setup(model, data_mean, data_std, centres, None, None)
        for start in range(0, n, batch):
            rows = min(batch, n - start)
            code = _draw(torch.randn, (rows, zd, 1, 1), device, generator) if z is None else z[start:start + rows]
            planes = _fit_planes(model.get_reconstruction(code), S)
            out[start:start + rows] = render_sheet([_decoder_column(model, planes, lut, lo, hi)], rows).view(rows, S, S)
    return out
