"""Per-frame MSE, PSNR and SSIM on the device: how close a reconstructed or sampled frame is to the true one, as a number.

The likelihoods ``evaluate`` reports cannot be compared across model families (a Gaussian VAE's NLL is a density, a categorical
model's a code length); the per-frame measures everyone reports on Moving MNIST can.  Both sides of a comparison are column specs of
the contact sheet (``column(...)`` of ``panels.py``), and the kernel reduces them to grey bytes by the sheet's own rule: the metric is
of exactly the picture ``render_sheet`` would show, so the two can never disagree.  One launch per comparison
(``mmvae_frame_quality``: squared error exact, SSIM in f64); ``mse`` and ``psnr`` follow by f64 tensor operations, no host read.
"""
import ctypes

import torch

from . import _lib as L
from .panels import (_COLUMN_KEYS, _COLUMN_KINDS, _class_column, _decoder_column, _fit_planes, _image_column, _plane_side, _plot_setup,
                     column)

_QUALITY_KINDS = _COLUMN_KINDS + ("bytes",)
_PEAK_SQ = 65025.0                     # 255^2


def _mse_psnr(sse, pixels):
    """mse = sse / pixels and psnr = 10 log10(255^2 / mse) in f64 on the device.  The divisor is a device tensor: a tensor divided by a
    Python number is multiplied by its rounded reciprocal there, which is not the correctly rounded quotient."""
    mse = sse / torch.full((), float(pixels), dtype=torch.float64, device=sse.device)
    return mse, 10.0 * torch.log10(_PEAK_SQ / mse)


def _side(spec, name):
    """One side of frame_quality, checked on its own: (descriptor, n, S, device).  The descriptor is render_sheet's (see panels.py)."""
    if not isinstance(spec, dict):
        spec = dict(zip(_COLUMN_KEYS, spec))
    kind, t = spec.get("kind"), spec.get("tensor")
    what = f"frame_quality: side {name} ({kind})"
    if kind not in _QUALITY_KINDS:
        raise ValueError(f"frame_quality: side {name} has kind {kind!r}, expected one of {_QUALITY_KINDS}")
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: the source must be a tensor")
    if t.dim() < 2 or t.shape[0] < 1:
        raise ValueError(f"{what}: expected at least one plane, got shape {tuple(t.shape)}")
    if not t.is_cuda:
        raise ValueError(f"{what}: the source must be on the GPU")
    n, t = int(t.shape[0]), t.detach()
    if kind == "bytes":
        if t.dtype != torch.uint8:
            raise ValueError(f"{what}: expected uint8, got {t.dtype}")
        if t.dim() == 4:
            if t.shape[1] != 1:
                raise ValueError(f"{what}: bytes have one channel, got shape {tuple(t.shape)} (reshape to (n * C, S, S))")
            t = t[:, 0]
        descs, S = [(L.FRAME_BYTES_U8, t.contiguous(), 0, None, None, 0.0, 1.0)], _plane_side(t, 1, what)
    elif kind == "image":
        descs, S = _image_column(spec, t, what)
    else:
        descs, S = _class_column(spec, t, what, n)
    if len(descs) != 1:
        raise ValueError(f"{what}: shape {tuple(t.shape)} is {len(descs)} columns, a side is one: reshape to (n * C, S, S)")
    return descs[0], n, S, t.device


def frame_quality(a, b):
    """Squared error, MSE, PSNR and SSIM of ``n`` pairs of frames on the device, ONE launch (mmvae_frame_quality).  ``a`` and ``b``:
    column specs as ``column(...)`` builds them for ``render_sheet`` ('labels', 'argmax', 'sample', 'image'), or kind ``'bytes'``: a
    uint8 device tensor taken as it is (generated clips, ``resize_frames`` output, dequantised samples).  Each side is reduced to grey
    bytes by the sheet's rule and must resolve to exactly one column of the same ``n`` planes of one side 11 <= S <= 64, both on one
    device; a (n, C, S, S) image is the caller's to reshape to (n * C, S, S).  Returns a dict of float64 device tensors of shape (n,):
    ``sse`` (sum of squared byte differences, exact) and ``ssim`` (Wang et al. 2004: 11 x 11 Gaussian window of sigma 1.5, population
    covariance, data range 255, the mean over the positions whose window lies inside the frame -- skimage's ``structural_similarity``
    with ``gaussian_weights=True, use_sample_covariance=False``; all of it in f64) from the launch, ``mse = sse / S^2`` and
    ``psnr = 10 log10(65025 / mse)`` (``+inf`` where the frames are equal) by f64 tensor operations.  No host read, no atomics: the
    same bits every run, capturable in a graph.  Everything is checked before anything is launched; a violation raises ValueError."""
    (da, na, Sa, dev_a), (db, nb, Sb, dev_b) = _side(a, "a"), _side(b, "b")
    if na != nb:
        raise ValueError(f"frame_quality: {na} planes against {nb}")
    if Sa != Sb:
        raise ValueError(f"frame_quality: planes of side {Sa} against planes of side {Sb}")
    if dev_a != dev_b:
        raise ValueError(f"frame_quality: side a on {dev_a}, side b on {dev_b}")
    if not L.FRAME_MIN_S <= Sa <= L.FRAME_MAX_S:
        raise ValueError(f"frame_quality: side {Sa} unsupported ({L.FRAME_MIN_S}..{L.FRAME_MAX_S}: the window is 11 x 11)")
    cols = [L.PanelCol(code, L.ptr(t), Q, L.ptr(u), L.ptr(lut), lo, hi) for code, t, Q, u, lut, lo, hi in (da, db)]
    out = torch.empty((2, na), dtype=torch.float64, device=dev_a)
    L.call("mmvae_frame_quality", dev_a, ctypes.addressof(cols[0]), ctypes.addressof(cols[1]), na, Sa, L.ptr(out))
    sse, ssim = out[0], out[1]
    mse, psnr = _mse_psnr(sse, Sa * Sa)
    return {"sse": sse, "ssim": ssim, "mse": mse, "psnr": psnr}


def reconstruction_quality(model, image, reconstruction, data_mean, data_std, centres=None):
    """``frame_quality`` of the two columns the ``recon`` sheet of ``plot_vae`` / ``plot_pixelcnn`` / ``plot_pixelvae`` shows, for every
    image of the batch: the input as an f32 column over [label 0, label Q - 1] (``(k - data_mean) / data_std``) against what the model
    emitted -- the per-pixel argmax through ``gray_lut(Q, centres)`` for a categorical decoder and for PixelCNN outputs, the f32 mean
    for a Gaussian decoder.  ``image``: the normalised (N, C, S, S) batch; ``reconstruction``: what ``model(image)`` returned (an odd
    ``input_image_size`` leaves one row and column too many: the leading S x S are compared, as the sheet shows them).  Returns the
    dict of ``frame_quality`` with tensors of shape (N,).  ``in_channels > 1``: a Gaussian model's channels are compared as planes
    and averaged back per image (``sse`` summed, ``mse`` / ``ssim`` averaged, ``psnr`` of that mse); a categorical one raises
    ValueError (its logits carry classes, not channels).  Runs no part of the model and changes nothing in it."""
    lo, hi, lut = _plot_setup(model, data_mean, data_std, centres, None, None)
    img = image.detach().float()
    if img.dim() != 4 or img.shape[-1] != img.shape[-2]:
        raise ValueError(f"reconstruction_quality: expected an (N, C, S, S) image, got {tuple(img.shape)}")
    N, C, S = int(img.shape[0]), int(img.shape[1]), int(img.shape[-1])
    rec = _fit_planes(reconstruction.detach(), S)
    categorical = model.pixelcnn is not None or model.decoder_out_channels > model.in_channels
    if categorical:
        if C != 1:
            raise ValueError("reconstruction_quality: a categorical model with in_channels > 1 has no grey picture to compare")
        theirs = column("argmax", rec, lut)
    else:
        theirs = _decoder_column(model, rec.reshape(N * C, S, S), lut, lo, hi)
    q = frame_quality(column("image", img.reshape(N * C, S, S), lo=lo, hi=hi), theirs)
    if C == 1:
        return q
    sse, ssim = q["sse"].view(N, C).sum(1), q["ssim"].view(N, C).mean(1)
    mse, psnr = _mse_psnr(sse, C * S * S)
    return {"sse": sse, "ssim": ssim, "mse": mse, "psnr": psnr}
