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
from .data import MovingMNISTClips
from .panels import _decoder_column, _draw, _fit_planes, _plot_mode, _plot_setup, render_sheet

SAMPLE_QUALITY_KEYS = ("precision", "recall", "density", "coverage", "accuracy", "accuracy_real", "accuracy_fake")


def _rows_u8(t, name, what):
    """One side of a sweep, checked on its own: the uint8 tensor as (N, D) rows (not yet made dense)."""
    if isinstance(t, MovingMNISTClips):
        t = t.clips.reshape(-1, t.clips.shape[-2] * t.clips.shape[-1])
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise ValueError(f"{what}: {name} must be a uint8 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() not in (2, 3):
        raise ValueError(f"{what}: {name} must have shape [N, H, W], [N, 1, H, W] or [N, H*W], got {tuple(t.shape)}")
    return t.detach().reshape(t.shape[0], t.shape[1] if t.dim() == 2 else t.shape[1] * t.shape[2])


def _cross_args(a, b, k, exclude_self, radius, what):
    """Every check of a sweep (nothing is launched here): returns (a (Na, D), b (Nb, D), radius int32 (Nb,) or None), the planes dense
    and 16-byte aligned."""
    a, b = _rows_u8(a, "a", what), _rows_u8(b, "b", what)
    (Na, D), (Nb, Db) = a.shape, b.shape
    if D != Db:
        raise ValueError(f"{what}: rows of {D} bytes in a do not match rows of {Db} bytes in b")
    if not 0 <= k <= L.KNN_CROSS_MAX_K:
        raise ValueError(f"{what}: k={k} unsupported (1..{L.KNN_CROSS_MAX_K})")
    for n, name in ((Na, "Na"), (Nb, "Nb")):
        if not 1 <= n <= L.KNN_CROSS_MAX_N:
            raise ValueError(f"{what}: {name}={n} rows unsupported (1..{L.KNN_CROSS_MAX_N})")
    if D % 16 or not 16 <= D <= L.KNN_CROSS_MAX_D:
        raise ValueError(f"{what}: D={D} bytes per row unsupported (a multiple of 16 in 16..{L.KNN_CROSS_MAX_D})")
    avail = Nb - 1 if exclude_self else Nb
    if k > avail:
        raise ValueError(f"{what}: k={k} exceeds the {avail} columns available (Nb={Nb}{', self excluded' if exclude_self else ''})")
    if radius is not None:
        if not isinstance(radius, torch.Tensor) or radius.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: radius must be an int32 or int64 tensor, got {getattr(radius, 'dtype', type(radius).__name__)}")
        if radius.dim() != 1 or radius.shape[0] != Nb:
            raise ValueError(f"{what}: radius of shape {tuple(radius.shape)} for Nb={Nb} columns")
    if a.device != b.device or (radius is not None and radius.device != b.device):
        raise ValueError(f"{what}: a on {a.device}, b on {b.device}" + ("" if radius is None else f", radius on {radius.device}"))
    if radius is not None and bool((radius.detach() < 0).any()):            # the one device -> host read of ball_counts
        raise ValueError(f"{what}: a radius is negative (squared distances are not)")
    if not a.is_cuda:
        raise ValueError(f"{what} expects its tensors on the GPU")
    a, b = (t.contiguous() for t in (a, b))
    a, b = (t if t.data_ptr() % 16 == 0 else t.clone() for t in (a, b))
    return a, b, radius


def _radius_i32(radius):
    """Checked squared-distance radii as the int32 the kernel compares against.  No distance exceeds D * 255^2 < 2^31, so larger radii
    are clamped to the int32 maximum without changing any comparison."""
    return radius.detach().clamp(max=2 ** 31 - 1).to(torch.int32).contiguous()


def _cross_launch(a, b, k, exclude_self, radius):
    """mmvae_knn_cross on checked arguments: (dist, index) or (None, None), and the counts or None."""
    (Na, D), Nb, dev = a.shape, b.shape[0], a.device
    nbytes = L.lib().mmvae_knn_cross_scratch_bytes(Na, Nb, D, k, int(radius is not None))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dist = torch.empty((Na, k), dtype=torch.int32, device=dev) if k else None
    index = torch.empty((Na, k), dtype=torch.int64, device=dev) if k else None
    count = torch.empty((Na,), dtype=torch.int32, device=dev) if radius is not None else None
    L.call("mmvae_knn_cross", dev, L.ptr(a), Na, L.ptr(b), Nb, D, k, int(bool(exclude_self)), L.ptr(dist), L.ptr(index), L.ptr(radius),
           L.ptr(count), L.ptr(scratch), nbytes)
    return dist, index, count


def cross_neighbours(a, b, k=1, exclude_self=False):
    """The ``k`` nearest rows of ``b`` for every row of ``a``, exactly (mmvae_knn_cross): a tiled int8 GEMM over all Na x Nb pairs, no
    Na x Nb matrix anywhere.  ``a``, ``b``: uint8 device tensors [N, H, W], [N, 1, H, W] or [N, H*W], or a ``MovingMNISTClips`` (its
    ``.clips``, flattened to frames).  The distance is the sum of squared byte differences in exact integers.  Returns ``(dist, index)``:
    int32 and int64 (Na, k) device tensors, nearest first, equal distances to the lower index of ``b``.  ``exclude_self=True`` leaves the
    pairs (i, i) out -- leave-one-out when ``a`` and ``b`` are the same set; a duplicate of row i at another index stays, at distance 0.
    Na, Nb <= 2^20, 1 <= k <= 8, H*W a multiple of 16 up to 16384, k <= Nb (Nb - 1 with ``exclude_self``).  Everything is checked before
    anything is launched (ValueError); no host read inside the call; the same bits every run."""
    k = int(k)
    if k < 1:
        raise ValueError(f"cross_neighbours: k={k} unsupported (1..{L.KNN_CROSS_MAX_K})")
    a, b, _ = _cross_args(a, b, k, exclude_self, None, "cross_neighbours")
    dist, index, _ = _cross_launch(a, b, k, exclude_self, None)
    return dist, index


def ball_counts(a, b, radius, exclude_self=False):
    """For every row i of ``a``, in how many balls of ``b`` it lies: ``#{ j : d(i, j) <= radius[j] }`` as an int32 (Na,) device tensor
    (mmvae_knn_cross without a selection).  ``radius``: int32 or int64 device tensor (Nb,) of SQUARED distances, each >= 0 (checked:
    one device -> host read); the comparison is inclusive and exact.  ``a``, ``b``, ``exclude_self`` and the limits as in
    ``cross_neighbours``."""
    a, b, radius = _cross_args(a, b, 0, exclude_self, radius, "ball_counts")
    return _cross_launch(a, b, 0, exclude_self, _radius_i32(radius))[2]


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
        lut = torch.as_tensor(lut)
        if lut.dtype != torch.uint8 or lut.numel() != 256:
            raise ValueError(f"{what}: lut is 256 uint8 values")
    R, F = _rows_u8(real, "real", what), _rows_u8(fake, "fake", what)
    for t, name in ((R, "real"), (F, "fake")):
        if t.shape[0] < k + 1:
            raise ValueError(f"{what}: k={k} neighbours inside {name} need more than k rows, got {t.shape[0]}")
    R, F, _ = _cross_args(R, F, k, False, None, what)
    if lut is not None:
        R = lut.detach().reshape(-1).to(R.device)[R.long()]
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
