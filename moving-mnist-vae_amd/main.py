"""Train-step driver with the reference's ``main.train`` signature.

Mirrors the loop body of the reference ``main.py:362-429`` (normalise ->
forward -> loss -> bookkeeping -> zero_grad / backward / step) so that a user
of the reference can swap ``from main import train`` for this one.  Around the
loop: held-out evaluation (``evaluate``, ``latent_stats``; the per-frame MSE /
PSNR / SSIM behind ``evaluate(quality=True)`` live in ``quality.py``, the ELBO split
behind ``evaluate(decomposition=True)`` in ``decomposition.py``), the model-name
grammar (``select_model``), the reference's samplers (``generate*``) and its
checkpoint format.  The plotting branch (``main.py:401-424``) hangs off
``args.plot_callback``: ``make_plot_callback`` in ``panels.py`` returns one, and
the picture panels (``plot_vae`` / ``plot_pixelcnn`` / ``plot_pixelvae``) and the
scatter plot (``scatter_plot``) live there too.  The per-parameter histograms of
``wandb.hook_torch`` (``main.py:456``) hang off ``args.stats_callback``, called
between ``backward`` and ``step``: ``make_histogram_callback`` in ``monitor.py``
returns one.  A further loss term on the latent code hangs off
``args.latent_penalty`` (``make_latent_penalty`` in ``decomposition.py``: the
beta-TCVAE objective of Chen et al. 2018).  The device-side input pipeline
(``quantise_frames``, ``fit_quantiser``, ``MovingMNISTClips``, ...) lives in
``data.py``.  The reference's ``main.py`` carries those names, so this module
re-exports them.

Nothing here does arithmetic on the hot path when the model is the HIP
``VAE`` of this package: batch preparation, forward, loss, backward and the
optimiser step all land in the C-ABI library (see ``model.py``).  The generic
torch fallback below exists so the same loop can drive the CPU oracle / the
reference model in parity tests; it is never used for the HIP model.
"""
from __future__ import annotations

import time
from typing import List, Tuple

import numpy as np
import torch

from .data import (KMEANS_FILE_NOTE, GeneratedClips, MovingMNISTClips, QuantiserFit, choose_transformer, clips_from_npz_array,  # noqa: F401
                   fit_quantiser, generate_batch, generate_clips, load_idx_images, load_kmeans_file, pixel_histogram,
                   quantise_frames, resize_frames, resize_quantise_frames, save_kmeans_file, save_moving_mnist_files, velocity_table)
from .decomposition import (LatentPenalty, _decompose, decomposition_to_host, elbo_decomposition, latent_penalty, make_latent_penalty,  # noqa: F401
                            posterior_mixture)
from .model import VAE
from .monitor import TensorHistograms, make_histogram_callback, tensor_histograms  # noqa: F401
from .neighbours import nearest_frames  # noqa: F401
from .panels import (_plot_setup, column, gray_lut, latent_slide, make_plot_callback, neighbour_sheet, plot_neighbours, plot_pixelcnn, plot_pixelvae,  # noqa: F401
                     plot_vae, render_sheet, sample_from_reconstruction, scatter_panel, scatter_plot, scatter_tone, write_png_gray)
from .quality import frame_quality, reconstruction_quality  # noqa: F401
from . import samples as _samples
from .samples import ball_counts, cross_neighbours, sample_frames, sample_quality, sample_quality_to_host  # noqa: F401


def prepare_batch(model, batch, device, args, data_mean, data_std):
    """main.py:374-388: returns (image, target).  Categorical (main.py:381) by the HIP model's rule, whatever model this is."""
    if getattr(args, "dataset", "MovingMNIST") == "MNIST":
        batch = batch[0]
    size = model.input_image_size
    hook = getattr(model, "prepare_batch", None)
    if hook is not None:
        # HIP model: one fused kernel, labels -> normalised frames (+ targets)
        return hook(batch, device, data_mean, data_std, VAE.is_categorical(model))
    frames = batch.to(device)
    image = (frames.float().view(-1, 1, size, size) - data_mean) / data_std
    target = frames.view(-1, size, size).to(device).long() if VAE.is_categorical(model) else image
    return image, target


def train(model, data_loader, optimizer, device, args, epoch=0, data_mean=0, data_std=1, plot_every=200,
          directory="output/") -> Tuple[List[float], List[float], List[float], List[float]]:
    """One epoch.  Returns per-step lists (loss, nll, kl, mmd) like main.py:429."""
    losses, nlls, kls, mmds = [], [], [], []
    t0 = time.time()
    model.train(True)
    plot_callback = getattr(args, "plot_callback", None)
    stats_callback = getattr(args, "stats_callback", None)
    penalty_fn = getattr(args, "latent_penalty", None)                     # make_latent_penalty(...): beta-TCVAE and its kin
    # HIP model: the step scalars stay on the device (model._last_group) and are read back once, after the loop or
    # when the plot callback needs them -- the host never waits for the GPU in the middle of a step.
    pending = []                      # (position in the lists, scalar group)

    def materialise():
        sync = getattr(model, "_sync", None)
        if sync is not None and pending:       # data parallel: the logged values are means over ranks (one message)
            sync.reduce_step_scalars([g for _, g in pending])
        for pos, grp in pending:
            losses[pos], nlls[pos], kls[pos], mmds[pos] = grp.get(0), grp.get(1), grp.get(2), grp.get(3)
        pending.clear()

    for index, batch in enumerate(data_loader):
        model.train(True)                                                    # main.py:372
        image, target = prepare_batch(model, batch, device, args, data_mean, data_std)
        mu, logvar, encoding, reconstruction = model(image)                  # main.py:389
        if hasattr(model, "_last_group"):      # HIP model: scalars stay on the device until the end of the loop
            loss, nll_v, kl_v, mmd_v = model.loss(target, mu, logvar, encoding, reconstruction, device, args, deferred=True)
        else:
            loss, nll_v, kl_v, mmd_v = model.loss(target, mu, logvar, encoding, reconstruction, device, args)
        grp = getattr(model, "_last_group", None)
        if grp is not None and getattr(nll_v, "_g", None) is grp:
            pending.append((len(losses), grp))
            losses.append(None); nlls.append(None); kls.append(None); mmds.append(None)
        else:
            losses.append(loss.item())                                       # main.py:393
            nlls.append(nll_v)
            kls.append(kl_v)
            mmds.append(mmd_v)
        if penalty_fn is not None:
            # (alpha - 1) MI + (beta - 1) TC + (gamma - 1) DWKL of this batch, through plain autograd.  Under deferred=True the VALUE of
            # `loss` is not defined yet at this point (its kernels run behind the decoder's backward pass): only the gradient of the sum is
            # used, and the four returned lists stay the reference's -- the penalty's own figures are penalty_fn.to_host()'s.
            loss = loss + penalty_fn(mu, logvar, encoding).to(loss.dtype)
        optimizer.zero_grad()                                                # main.py:397-399
        loss.backward()
        if stats_callback is not None:                                       # main.py:456 (wandb.hook_torch): the gradients, before the step
            stats_callback(model=model, optimizer=optimizer, epoch=epoch, index=index)
        optimizer.step()
        if plot_callback is not None and index % plot_every == 0:            # main.py:401
            materialise()
            plot_callback(model=model, image=image, reconstruction=reconstruction, encoding=encoding,
                          epoch=epoch, index=index, directory=directory,
                          running={"nll": np.mean(nlls), "kl": np.mean(kls), "mmd": np.mean(mmds)})
    materialise()
    elapsed = time.time() - t0
    if not getattr(args, "quiet", False) and losses:
        print("Epoch={:d}; Loss={:0.5f} NLL={:.3f}; KL={:.3f}; MMD={:.3f}; time_tr={:.1f}s;".format(
            epoch, np.mean(losses), np.mean(nlls), np.mean(kls), np.mean(mmds), elapsed))
    return losses, nlls, kls, mmds


_SAMPLE_QUALITY_K = 3                              # the k of evaluate(sample_quality=n): Naeem et al.'s and sample_quality's default


def evaluate(model, data_loader, device, args, data_mean=0, data_std=1, iw_samples=0, weighted=False, generator=None,
             return_per_image=False, latent_stats=False, quality=False, centres=None, decomposition=False, sample_quality=0) -> dict:
    """Held-out evaluation of the HIP model (the reference builds a test loader, main.py:497, and never reads it): one eval-mode pass
    over ``data_loader`` under ``torch.no_grad()``; the model's train / eval mode is restored afterwards and no parameter or buffer
    changes.  Batches are prepared as in ``train``.  Per-image terms come from ``model.per_image_terms`` (and ``model.iw_bound``
    with ``iw_samples`` = K > 0), are summed on the device in f64 and read back once, at the end.

    Returns means PER IMAGE in nats (a ragged last batch weighs what its images weigh): ``n_images``, ``nll`` (-log p(x|z), one
    sample of q(z|x) per image; unweighted unless ``weighted`` passes ``args.data_ratio_of_labels``), ``kl`` (0 without a logvar),
    ``elbo`` = -(nll + kl), ``iw_bound`` (None when ``iw_samples`` == 0) and ``bits_per_dim`` = nll / (C S S ln 2) for categorical
    models (None for Gaussian ones: a density, not a code length).  A PixelCNN on its own has no latent: ``kl``, ``elbo`` and
    ``iw_bound`` are None.  ``generator`` (a device generator) draws every noise tensor; None uses the global one.
    ``return_per_image=True`` adds ``per_image``: {'nll', 'kl', 'iw_bound'} as concatenated f64 device tensors (or None).
    ``latent_stats=True`` adds ``latent``: per-dimension diagnostics of the latent code (f64 numpy arrays of length z) from one
    ``latent_stats`` accumulator carried over the loader and read once at the end -- ``kl_per_dim`` (mean per image of each dimension's
    KL; which dimensions have collapsed to the prior), ``mu_mean`` / ``mu_var`` (mean and population variance of the posterior means),
    ``active_units`` (dimensions with ``mu_var > 0.01``, Burda et al. 2016), ``mean_posterior_var`` (mean of exp(logvar)), ``z_mean`` /
    ``z_var`` (of the sampled codes: the aggregate posterior's moments).  Without a logvar ``kl_per_dim`` and ``mean_posterior_var`` are
    None; a PixelCNN on its own has ``latent`` None.  Under this flag ``kl`` (and ``elbo``) are taken from the same accumulator, whose
    terms are formed in f64: ``sum(kl_per_dim) == kl`` up to f64 summation order, and ``kl`` moves by the f32 rounding of the
    per-image kernel's terms (a few 1e-8 relative) against the value without the flag.
    ``quality=True`` adds ``quality``: {'mse', 'psnr', 'ssim'} of the reconstruction against the input as 8-bit pictures
    (``reconstruction_quality`` on every batch, ``centres`` the k-means centres of its grey table): ``mse`` and ``ssim`` are means per
    image, ``psnr = 10 log10(65025 / mean mse)``.  The sums join the f64 device sums above and come back in the same single copy;
    ``per_image`` gains 'mse' and 'ssim'.  Needs 11 <= input_image_size <= 64.  Without the flag nothing changes, keys or bits.
    ``decomposition=True`` adds ``decomposition``: the split of the averaged KL term over this data set (``elbo_decomposition``, which
    see for the keys: ``mi``, ``tc``, ``dwkl``, ``marginal_kl``, ``kl_sampled``, ``kl_analytic``, ``log_m`` as floats, ``dwkl_per_dim``
    as a numpy array, the counts ``n`` = ``m`` = ``n_images``).  Every batch's ``mu``, ``logvar`` and ``encoding`` are kept on the device
    as f32 (3 * 4 * n_images * z bytes), one ``elbo_decomposition`` call follows the loop and its result comes back in one more
    device-to-host copy; ``per_image`` gains 'log_qz'.  Known limits: ``mi <= log_m`` by construction (each sample's own posterior is in
    the bank), so a value near ``log_m`` means saturated, not measured; all figures are Monte-Carlo estimates from one sample per image.
    A PixelCNN on its own has ``decomposition`` None; a model built with ``require_rsample=False`` has no q(z|x) density and raises
    ValueError, as ``iw_bound`` does.  Without the flag nothing changes, keys or bits.
    ``sample_quality=n`` (n > 0, a plain one-channel VAE) adds ``samples``: {'precision', 'recall', 'density', 'coverage', 'accuracy',
    'accuracy_real', 'accuracy_fake', 'n_real', 'n_fake', 'k'} of ``n`` decodings of z ~ N(0, I) (``sample_frames``, drawn through
    ``generator`` AFTER the pass over the loader, so no other entry depends on the argument) against every frame of the loader, both as
    the grey bytes of the sheets (the input column of ``recon``, the ``normal_sampling`` column; ``centres`` as for ``quality``), by
    ``sample_quality`` with k = 3, which see for the definitions and the two limits.  The frames are kept on the device as uint8
    (n_images * S * S bytes); the seven scores join the single device-to-host copy.  Without the argument nothing changes, launch for
    launch."""
    if not hasattr(model, "per_image_terms"):
        raise TypeError("evaluate() drives the HIP VAE of this package (it needs model.per_image_terms)")
    n_samples = int(sample_quality or 0)
    if n_samples < 0:
        raise ValueError(f"evaluate(sample_quality={n_samples}): the number of samples cannot be negative")
    if n_samples and (model.only_pixelcnn or model.pixelcnn is not None or model.in_channels != 1):
        raise ValueError("evaluate(sample_quality=n) needs a plain one-channel VAE (PixelCNN / PixelVAE draw with model.sample_pixels)")
    latent = not model.only_pixelcnn
    want_dec = bool(decomposition) and latent
    if want_dec and not model.require_rsample:
        raise ValueError("evaluate(decomposition=True) needs q(z|x): the model was built with require_rsample=False")
    categorical = VAE.is_categorical(model)
    weight = getattr(args, "data_ratio_of_labels", None) if (weighted and categorical) else None
    was_training = bool(model.training)
    sums = None                                    # f64 device: nll, kl, iw (, mse, ssim with `quality`)
    want_latent, acc = bool(latent_stats) and latent, None      # acc: f64 device [6][z], see latent_stats()
    kept = {"nll": [], "kl": [], "iw_bound": []}
    if quality:
        kept.update(mse=[], ssim=[])
    bank = ([], [], [])                            # mu, logvar, encoding of every batch (f32, on the device), with `decomposition`
    n_images = 0
    real_bytes = []                                # the loader's frames as the recon sheet's input column, with `sample_quality`
    if n_samples:
        lo, hi, _ = _plot_setup(model, data_mean, data_std, centres, None, None)
    model.eval()
    try:
        with torch.no_grad():
            for batch in data_loader:
                image, target = prepare_batch(model, batch, device, args, data_mean, data_std)
                N = image.shape[0]
                injected = False
                if latent and model.require_rsample and model.injected_eps is None:
                    # the draw VAE._rsample would make itself, through `generator`
                    model.injected_eps = torch.randn((N, model.z_dimensions, 1, 1), device=image.device, dtype=torch.float32, generator=generator)
                    injected = True
                try:
                    mu, logvar, encoding, reconstruction = model(image, sample=image)   # PixelVAE: teacher-forced on the image itself
                finally:
                    if injected:
                        model.injected_eps = None
                nll, kl = model.per_image_terms(target, mu, logvar, reconstruction, weight=weight)
                if want_latent:
                    acc, have_lv = _latent_stats_into(model, mu, logvar, encoding, acc), logvar is not None
                if want_dec:
                    for rows, t in zip(bank, (mu, logvar, encoding)):
                        rows.append(t.detach().reshape(N, -1).float().clone())
                iw = model.iw_bound(image, target, iw_samples, generator=generator, weight=weight) if iw_samples else None
                if sums is None:
                    sums = torch.zeros(5 if quality else 3, dtype=torch.float64, device=nll.device)
                sums[0] += nll.sum()
                if kl is not None:
                    sums[1] += kl.sum()
                if iw is not None:
                    sums[2] += iw.sum()
                if quality:
                    q = reconstruction_quality(model, image, reconstruction, data_mean, data_std, centres)
                    sums[3] += q["mse"].sum()
                    sums[4] += q["ssim"].sum()
                if n_samples:
                    S = image.shape[-1]
                    real_bytes.append(render_sheet([column("image", image.detach().float().reshape(N, S, S), lo=lo, hi=hi)], N).view(N, S, S))
                n_images += N
                if return_per_image:
                    kept["nll"].append(nll)
                    if kl is not None:
                        kept["kl"].append(kl)
                    if iw is not None:
                        kept["iw_bound"].append(iw)
                    if quality:
                        kept["mse"].append(q["mse"])
                        kept["ssim"].append(q["ssim"])
    finally:
        model.train(was_training)
    if n_images == 0:
        raise ValueError("evaluate(): the data loader yielded no batch")
    n_sums = sums.numel()
    if n_samples:
        fake = _samples.sample_frames(model, n_samples, data_mean, data_std, centres, generator)
        scores = _samples.sample_quality(torch.cat(real_bytes), fake, k=_SAMPLE_QUALITY_K)
        sums = torch.cat([sums, torch.stack([scores[key] for key in _samples.SAMPLE_QUALITY_KEYS])])
    host = sums.tolist()                                                                # the one device -> host copy
    s_nll, s_kl, s_iw, *s_quality = (v / n_images for v in host[:n_sums])
    latent_out = None
    if want_latent:
        a = acc.cpu().numpy()                                                           # ... and the accumulator's
        mu_mean, z_mean = a[0] / n_images, a[4] / n_images
        mu_var = np.maximum(a[1] / n_images - mu_mean * mu_mean, 0.0)
        latent_out = {"kl_per_dim": a[2] / n_images if have_lv else None, "mu_mean": mu_mean, "mu_var": mu_var,
                      "active_units": int((mu_var > 0.01).sum()), "mean_posterior_var": a[3] / n_images if have_lv else None,
                      "z_mean": z_mean, "z_var": np.maximum(a[5] / n_images - z_mean * z_mean, 0.0)}
        if have_lv:
            s_kl = float(a[2].sum()) / n_images
    dims = model.in_channels * model.input_image_size ** 2
    out = {"n_images": n_images, "nll": s_nll, "kl": s_kl if latent else None, "elbo": -(s_nll + s_kl) if latent else None,
           "iw_bound": s_iw if iw_samples else None, "bits_per_dim": s_nll / (dims * float(np.log(2.0))) if categorical else None}
    if quality:
        s_mse, s_ssim = s_quality
        out["quality"] = {"mse": s_mse, "psnr": float("inf") if s_mse == 0.0 else 10.0 * float(np.log10(65025.0 / s_mse)), "ssim": s_ssim}
    if n_samples:
        out["samples"] = dict(zip(_samples.SAMPLE_QUALITY_KEYS, host[n_sums:]), n_real=n_images, n_fake=n_samples, k=_SAMPLE_QUALITY_K)
    if return_per_image:
        out["per_image"] = {k: (torch.cat(v) if v else None) for k, v in kept.items()}
    if latent_stats:
        out["latent"] = latent_out
    if decomposition:
        out["decomposition"] = None
        if want_dec:
            dec, log_qz = _decompose(*(torch.cat(rows) for rows in bank), None, "evaluate(decomposition=True)")
            out["decomposition"] = decomposition_to_host(dec)
            if return_per_image:
                out["per_image"]["log_qz"] = log_qz
        elif return_per_image:
            out["per_image"]["log_qz"] = None
    return out


def _latent_stats_into(model, mu, logvar, encoding, acc):
    from . import _lib as L
    d = int(model.z_dimensions)
    if mu is None:
        raise ValueError("latent_stats needs the posterior means (a PixelCNN on its own has no latent)")
    dev = mu.device
    N = int(mu.shape[0])

    def rows(t, what):
        if t is None:
            return None
        t = t.detach().float().contiguous()
        if t.device != dev or t.numel() != N * d:
            raise ValueError(f"latent_stats: {what} {tuple(t.shape)} on {t.device} does not hold {N} x {d} values on {dev}")
        return t

    m, lv, enc = rows(mu, "mu"), rows(logvar, "logvar"), rows(encoding, "encoding")
    accumulate = acc is not None
    if acc is None:
        acc = torch.empty((L.LATENT_STATS_ROWS, d), dtype=torch.float64, device=dev)
    elif (not isinstance(acc, torch.Tensor) or acc.dtype != torch.float64 or tuple(acc.shape) != (L.LATENT_STATS_ROWS, d)
          or acc.device != dev or not acc.is_contiguous()):
        raise ValueError(f"latent_stats: acc must be a contiguous float64 ({L.LATENT_STATS_ROWS}, {d}) tensor on {dev}")
    L.call("mmvae_latent_stats", dev, L.ptr(m), L.ptr(lv), L.ptr(enc), N, d, int(accumulate), L.ptr(acc))
    return acc


def latent_stats(model, mu, logvar, encoding, acc=None):
    """Per-dimension f64 sums over the images of a batch, on the device in one launch (mmvae_latent_stats), no host read: a (6, z)
    float64 device tensor with rows sum ``mu``, sum ``mu^2``, sum ``0.5 (exp(logvar) + mu^2 - logvar - 1)`` (each dimension's KL), sum
    ``exp(logvar)``, sum ``encoding``, sum ``encoding^2``, every term formed in double from the f32 inputs.  ``mu`` / ``logvar`` /
    ``encoding``: what ``model(image)`` returns, (N, z, 1, 1) or (N, z); ``logvar`` / ``encoding`` may be None (their rows are zero).
    ``acc=None`` returns a fresh accumulator; passing the one an earlier call returned ADDS this batch to it, so one tensor is carried
    over a data loader and divided by the image count at the end (``evaluate(..., latent_stats=True)`` does that).  Fixed order, no
    atomics: the same bits every run."""
    return _latent_stats_into(model, mu, logvar, encoding, acc)


# ---------------------------------------------------------------------------------------------------------------------
# Drop-in contract around the loop: model-name grammar, the reference's samplers, checkpoint format
# ---------------------------------------------------------------------------------------------------------------------
def _is_number(text) -> bool:
    try:
        float(text)
        return True
    except ValueError:
        return False


def select_model(args):
    """Model factory with the reference's name grammar and keyword mapping (main.py:41-147):
    ``pixelcnn_<layers>`` | ``<normal|categorical>_<vae|pixelvae>_<kl>_kl_<mmd>_mmd``.  Returns ``(model, model_params)`` with the reference's
    dict keys."""
    parts = args.model.split("_")
    if len(parts) == 2:                                                         # main.py:57-66
        if parts[0] != "pixelcnn":
            raise AssertionError("It has to be only pixelcnn_2/4/7")
        if not _is_number(parts[1]):
            raise AssertionError("The number of layers has to be an int")
        only_pixelcnn = use_pixelcnn = True
        args.num_pixelcnn_layers = int(float(parts[1]))
        mp = {"model_name": "PixelCNN", "is_decoder_out_normal": False, "only_pixelcnn": True, "use_pixelcnn": True, "coeff_kl": 0., "coeff_mmd": 0.}
    else:                                                                       # main.py:69-87
        only_pixelcnn = False
        if not (len(parts) == 6 and "vae" in parts[1]):
            raise AssertionError("model name should be of the format normal_pixelvae_1_kl_10_mmd")
        if parts[1] not in ("pixelvae", "vae"):
            raise AssertionError("model should be vae or pixelvae")
        if not (_is_number(parts[2]) and _is_number(parts[4])):
            raise AssertionError("coefficients should be numeric")
        use_pixelcnn = parts[1] == "pixelvae"
        is_normal = parts[0] == "normal"
        mp = {"is_decoder_out_normal": is_normal, "only_pixelcnn": False, "use_pixelcnn": use_pixelcnn,
              "coeff_kl": float(parts[2]), "coeff_mmd": float(parts[4])}
        if use_pixelcnn:
            mp["model_name"] = "PixelVAE"
            if not is_normal and not (args.decoder_out_channels > args.input_channels):
                raise AssertionError("decoder_out_channels should be > input_channels when categorical_pixelvae else simply use normal_pixelvae")
        else:
            mp["model_name"] = "VAE"
    # main.py:91-93: normal_vae_* needs sigma_decoder != 0, normal_pixelvae_* needs sigma_decoder == 0
    if mp["is_decoder_out_normal"] and not (use_pixelcnn == (args.sigma_decoder == 0)):
        raise AssertionError("sigma_decoder should be 0 when using vae and non-zero when using pixelvae/pixelcnn")
    if use_pixelcnn:                                                            # main.py:95-100
        if not getattr(args, "num_pixelcnn_layers", 4) >= 2:
            raise AssertionError("num of pixelcnn layers should be greater than 2 when using pixelvae/pixelcnn")
        if getattr(args, "pixelcnn_activation", "ReLu") not in ("ReLu", "ELU"):
            raise AssertionError("Choose either Relu or ELU")
    mp.update({"input_channels": args.input_channels, "input_image_size": args.input_image_size,
               "intermediate_channels": args.intermediate_channels, "z_dimension": args.z_dimension,
               "sigma_decoder": args.sigma_decoder, "require_rsample": args.require_rsample,
               "num_pixelcnn_layers": getattr(args, "num_pixelcnn_layers", 4),
               "pixelcnn_activation": getattr(args, "pixelcnn_activation", "ReLu"), "coeff_nll": args.nll})
    if use_pixelcnn:                                                            # main.py:114-124
        mp["pixelcnn_out_channels"] = int(args.quantization)
        if not only_pixelcnn:
            mp["decoder_out_channels"] = args.input_channels if mp["is_decoder_out_normal"] else args.decoder_out_channels
        else:
            mp["decoder_out_channels"] = 0
    else:                                                                       # main.py:126-134
        mp["pixelcnn_out_channels"] = 0
        mp["decoder_out_channels"] = mp["input_channels"] if mp["is_decoder_out_normal"] else int(args.quantization)
    model = VAE(in_channels=mp["input_channels"], intermediate_channels=mp["intermediate_channels"],
                decoder_out_channels=mp["decoder_out_channels"], pixelcnn_out_channels=mp["pixelcnn_out_channels"],
                z_dimension=mp["z_dimension"], pixelcnn=mp["use_pixelcnn"], only_pixelcnn=mp["only_pixelcnn"],
                pixelcnn_layers=mp["num_pixelcnn_layers"], pixelcnn_activation=mp["pixelcnn_activation"],
                nll=mp["coeff_nll"], kl=mp["coeff_kl"], mmd=mp["coeff_mmd"], require_rsample=mp["require_rsample"],
                sigma_decoder=mp["sigma_decoder"], input_image_size=mp["input_image_size"],
                compute_dtype=getattr(args, "compute_dtype", None), blocks_per_stage=int(getattr(args, "blocks_per_stage", 1)))
    # build-defined extensions ride along in the parameter dict (and from there into the checkpoint)
    mp["compute_dtype"], mp["blocks_per_stage"] = model.compute_dtype, model.blocks_per_stage
    return model, mp


@torch.no_grad()
def generate_only_pixelcnn(sample, model, data_mean, data_std, uniforms=None):
    """main.py:186-192: autoregressive sampling of a PixelCNN-only model, pixel by pixel (S * S forward passes; `sample` is updated in place).
    Default: the reference's loop, drawing with torch.multinomial from the global RNG.  uniforms: an (N, S*S) tensor of uniforms in [0, 1), or
    True to draw them with torch.rand -- the whole loop then runs on the device in one call, model.sample_pixels (same distribution, another
    random stream)."""
    if uniforms is not None:
        return model.sample_pixels(sample, None, data_mean=data_mean, data_std=data_std, uniforms=None if uniforms is True else uniforms)
    import torch.nn.functional as F
    out = None
    for i in range(model.input_image_size):
        for j in range(model.input_image_size):
            out = model.run_pixelcnn(sample)
            probs = F.softmax(out[:, :, i, j], dim=1)
            sample[:, :, i, j] = torch.multinomial(probs, 1).float() / data_std                      # (sic: the reference does not subtract the mean here)
    return out, sample


@torch.no_grad()
def generate(z_image, sample, model, data_mean, data_std, uniforms=None):
    """main.py:195-202: autoregressive sampling of a PixelVAE's PixelCNN conditioned on the decoder image.  uniforms: as in
    generate_only_pixelcnn (None: the reference's loop; a tensor or True: model.sample_pixels on the device)."""
    if uniforms is not None:
        return model.sample_pixels(sample, z_image, data_mean=data_mean, data_std=data_std, uniforms=None if uniforms is True else uniforms)
    import torch.nn.functional as F
    output_ = None
    for i in range(model.input_image_size):
        for j in range(model.input_image_size):
            concat = torch.cat([z_image, sample], dim=1)
            output_ = model.run_pixelcnn(concat)
            probs = F.softmax(output_[:, :, i, j], dim=1)
            sample[:, :, i, j] = (torch.multinomial(probs, 1).float() - data_mean) / data_std
    return output_, sample


def save_checkpoint(model, optimizer, epoch, directory):
    """Same file and dict layout as main.py:522-526 (``latest-model.model`` = {'epoch','state_dict','optimizer'}), so
    checkpoints move between the reference and this package in both directions."""
    import os
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, "latest-model.model")
    ck = {"epoch": epoch, "state_dict": model.state_dict(), "optimizer": optimizer.state_dict()}
    # the reference network keeps the reference's three keys; a build-defined variant (deeper net, fp8 compute mode) adds what a loader
    # needs to rebuild it
    blocks, cdt = int(getattr(model, "blocks_per_stage", 1)), getattr(model, "compute_dtype", None)
    if blocks != 1 or cdt == "fp8":
        ck["mmvae"] = {"compute_dtype": cdt, "blocks_per_stage": blocks}
    torch.save(ck, path)
    return path


def checkpoint_variant(path, map_location=None):
    """The build-defined constructor keywords a checkpoint was saved with: {'compute_dtype', 'blocks_per_stage'} (reference
    checkpoints, which lack the entry: the reference network, default compute mode)."""
    ck = torch.load(path, map_location=map_location, weights_only=False)
    v = dict(ck.get("mmvae") or {})
    return {"compute_dtype": v.get("compute_dtype"), "blocks_per_stage": int(v.get("blocks_per_stage", 1))}


def load_checkpoint(path, model, optimizer=None, map_location=None):
    """The resume path the reference lacks: restores parameters / BN buffers (and Adam moments for FusedAdam or
    torch.optim.Adam); returns the stored epoch."""
    ck = torch.load(path, map_location=map_location, weights_only=False)
    want = int((ck.get("mmvae") or {}).get("blocks_per_stage", 1))
    have = int(getattr(model, "blocks_per_stage", 1))
    if want != have:
        raise ValueError(f"checkpoint was saved from a net with blocks_per_stage={want}, the model has {have} "
                         "(build it with checkpoint_variant(path)['blocks_per_stage'])")
    model.load_state_dict(ck["state_dict"])
    if optimizer is not None and "optimizer" in ck:
        loader = getattr(optimizer, "load_flat_state", None)
        if loader is not None:
            loader(ck["optimizer"])
        else:
            optimizer.load_state_dict(ck["optimizer"])
    return ck.get("epoch", 0)
