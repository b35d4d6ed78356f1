"""Train-step driver with the reference's ``main.train`` signature.

Mirrors the loop body of the reference ``main.py:362-429`` (normalise ->
forward -> loss -> bookkeeping -> zero_grad / backward / step) so that a user
of the reference can swap ``from main import train`` for this one.  The
plotting branch (``main.py:401-424``) hangs off ``args.plot_callback``:
``make_plot_callback`` returns one that renders the reference's picture panels
(``plot_vae`` / ``plot_pixelcnn`` / ``plot_pixelvae``, ``main.py:205-359``) as
8-bit greyscale contact sheets on the device (``render_sheet``, one kernel
launch per sheet) and writes them as PNG files (``write_png_gray``, standard
library only).  The reference's scatter plot of q(z|x) against p(z)
(``scatter_plot``, ``main.py:166-183``) is rendered on the device as well, as a
density panel (``scatter_panel``; opt-in from the plot functions with
``scatter=True``).  matplotlib figures and wandb stay with the caller: the
callback keeps what they need in ``.last``.

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


def _is_categorical(model) -> bool:
    # main.py:381 -- cross entropy when a PixelCNN exists or the decoder emits
    # more channels than the input has.
    return model.pixelcnn is not None or model.decoder_out_channels > model.in_channels


def prepare_batch(model, batch, device, args, data_mean, data_std):
    """main.py:374-388: returns (image, target)."""
    if getattr(args, "dataset", "MovingMNIST") == "MNIST":
        batch = batch[0]
    size = model.input_image_size
    hook = getattr(model, "prepare_batch", None)
    if hook is not None:
        # HIP model: one fused kernel, labels -> normalised frames (+ targets)
        return hook(batch, device, data_mean, data_std, _is_categorical(model))
    frames = batch.to(device)
    image = (frames.float().view(-1, 1, size, size) - data_mean) / data_std
    if _is_categorical(model):
        target = frames.view(-1, size, size).to(device).long()
    else:
        target = image
    return image, target


def train(model, data_loader, optimizer, device, args, epoch=0, data_mean=0, data_std=1, plot_every=200,
          directory="output/") -> Tuple[List[float], List[float], List[float], List[float]]:
    """One epoch.  Returns per-step lists (loss, nll, kl, mmd) like main.py:429."""
    losses: List[float] = []
    nlls: List[float] = []
    kls: List[float] = []
    mmds: List[float] = []
    t0 = time.time()
    model.train(True)
    plot_callback = getattr(args, "plot_callback", None)
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
        optimizer.zero_grad()                                                # main.py:397-399
        loss.backward()
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


def evaluate(model, data_loader, device, args, data_mean=0, data_std=1, iw_samples=0, weighted=False, generator=None,
             return_per_image=False, latent_stats=False) -> dict:
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
    per-image kernel's terms (a few 1e-8 relative) against the value without the flag."""
    if not hasattr(model, "per_image_terms"):
        raise TypeError("evaluate() drives the HIP VAE of this package (it needs model.per_image_terms)")
    latent = not model.only_pixelcnn
    categorical = _is_categorical(model)
    weight = getattr(args, "data_ratio_of_labels", None) if (weighted and categorical) else None
    was_training = bool(model.training)
    sums = None                                    # f64 device: nll, kl, iw
    want_latent, acc = bool(latent_stats) and latent, None      # acc: f64 device [6][z], see latent_stats()
    kept = {"nll": [], "kl": [], "iw_bound": []}
    n_images = 0
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
                iw = model.iw_bound(image, target, iw_samples, generator=generator, weight=weight) if iw_samples else None
                if sums is None:
                    sums = torch.zeros(3, dtype=torch.float64, device=nll.device)
                sums[0] += nll.sum()
                if kl is not None:
                    sums[1] += kl.sum()
                if iw is not None:
                    sums[2] += iw.sum()
                n_images += N
                if return_per_image:
                    kept["nll"].append(nll)
                    if kl is not None:
                        kept["kl"].append(kl)
                    if iw is not None:
                        kept["iw_bound"].append(iw)
    finally:
        model.train(was_training)
    if n_images == 0:
        raise ValueError("evaluate(): the data loader yielded no batch")
    s_nll, s_kl, s_iw = (v / n_images for v in sums.tolist())                           # the one device -> host copy
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
    if return_per_image:
        out["per_image"] = {k: (torch.cat(v) if v else None) for k, v in kept.items()}
    if latent_stats:
        out["latent"] = latent_out
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
    with torch.cuda.device(dev):
        L.check(L.lib().mmvae_latent_stats(L.ptr(m), L.ptr(lv), L.ptr(enc), N, d, int(accumulate), L.ptr(acc),
                                           torch.cuda.current_stream().cuda_stream), "mmvae_latent_stats")
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
# Drop-in contract around the loop: model-name grammar, checkpoint format, device-side input quantisation
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
    from .model import VAE
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


def quantise_frames(frames_u8, centres, data_mean, data_std):
    """Device-side input pipeline: uint8 frames -> k-means labels (int64) and normalised f32 image, one
    kernel (replaces ToTensor + kmeans.predict on the host, main.py:21-38, and the normalisation of main.py:383-387)."""
    from ._lib import check, lib, ptr
    f = frames_u8.contiguous()
    if f.dtype != torch.uint8 or not f.is_cuda:
        raise ValueError("quantise_frames expects a uint8 tensor on the GPU")
    c = torch.as_tensor(centres, dtype=torch.float32, device=f.device).contiguous()
    labels = torch.empty(f.shape, dtype=torch.int64, device=f.device)
    image = torch.empty(f.shape, dtype=torch.float32, device=f.device)
    check(lib().mmvae_quantise_normalise(ptr(f), f.numel(), ptr(c), c.numel(), float(data_mean), float(data_std), ptr(labels),
                                         ptr(image), torch.cuda.current_stream().cuda_stream), "mmvae_quantise_normalise")
    return labels, image


_RESAMPLE_TABLES = {}                  # (in_size, out_size, device) -> (bounds int32 [out, 2], coeffs int32 [out, ksize], ksize), on the device


def _resample_tables(in_size, out_size, device):
    """Device copy of mmvae_resample_coeffs(in_size, out_size), built once per (in, out, device): later calls copy nothing."""
    from ._lib import check, lib
    import ctypes
    key = (int(in_size), int(out_size), str(device))
    hit = _RESAMPLE_TABLES.get(key)
    if hit is None:
        ksize = ctypes.c_int(0)
        check(lib().mmvae_resample_coeffs(key[0], key[1], ctypes.byref(ksize), None, None), "mmvae_resample_coeffs")
        bounds = np.zeros((key[1], 2), dtype=np.int32)
        coeffs = np.zeros((key[1], ksize.value), dtype=np.int32)
        check(lib().mmvae_resample_coeffs(key[0], key[1], ctypes.byref(ksize), bounds.ctypes.data, coeffs.ctypes.data), "mmvae_resample_coeffs")
        hit = (torch.from_numpy(bounds).to(device), torch.from_numpy(coeffs).to(device), int(ksize.value))
        _RESAMPLE_TABLES[key] = hit
    return hit


def _size_pair(size):
    if isinstance(size, (tuple, list)):
        if len(size) != 2:
            raise ValueError("size is an int or an (h, w) pair")
        return int(size[0]), int(size[1])
    return int(size), int(size)


def _checked_clip_index(clip_index, n, device, what):
    idx = torch.as_tensor(clip_index, dtype=torch.int64, device=device).reshape(-1).contiguous()
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise IndexError(f"{what}: clip_index outside [0, {n})")
    return idx


def _resize_launch(frames_u8, size, centres, data_mean, data_std, idx, want):
    """One mmvae_resize_quantise_normalise launch.  frames_u8: uint8 device tensor [..., H, W]; idx: None, or trusted int64 device
    indices into the leading axis of an (N, C, H, W) tensor (whole clips are gathered).  want: which of (labels, image, resized) to
    produce.  Returns the three tensors (None where not wanted), shaped [..., S_h, S_w] (leading axis len(idx) under a gather)."""
    from ._lib import check, lib, ptr
    f = frames_u8
    if f.dim() < 2:
        raise ValueError("expected frames of shape [..., H, W]")
    H, W = int(f.shape[-2]), int(f.shape[-1])
    out_h, out_w = size
    if idx is not None:
        if f.dim() < 3:
            raise ValueError("clip_index needs a leading clip axis: frames of shape (N, ..., H, W)")
        f = f.contiguous()
        per_clip = f[0].numel() // (H * W) if f.shape[0] else 1
        lead, stride, n_frames = (idx.numel(),) + tuple(f.shape[1:-2]), H * W, idx.numel() * per_clip
    elif f.dim() == 3 and f.stride(2) == 1 and f.stride(1) == W and f.stride(0) >= H * W:
        per_clip, lead, stride, n_frames = 1, (f.shape[0],), int(f.stride(0)), int(f.shape[0])          # planes of a larger buffer, in place
    else:
        f = f.contiguous()
        per_clip, lead, stride, n_frames = 1, tuple(f.shape[:-2]), H * W, f.numel() // (H * W) if H * W else 0
    hb, hc, hk = _resample_tables(W, out_w, f.device)
    vb, vc, vk = _resample_tables(H, out_h, f.device)
    shape = tuple(lead) + (out_h, out_w)
    labels = torch.empty(shape, dtype=torch.int64, device=f.device) if want[0] else None
    image = torch.empty(shape, dtype=torch.float32, device=f.device) if want[1] else None
    resized = torch.empty(shape, dtype=torch.uint8, device=f.device) if want[2] else None
    if n_frames == 0:                            # nothing to launch (and empty tensors have no address to hand over)
        return labels, image, resized
    c = None
    if want[0] or want[1]:
        c = torch.as_tensor(centres, dtype=torch.float32, device=f.device).reshape(-1).contiguous()
    with torch.cuda.device(f.device):
        check(lib().mmvae_resize_quantise_normalise(ptr(f), stride, ptr(idx), per_clip, n_frames, H, W, out_h, out_w, ptr(hb), ptr(hc), hk,
                                                    ptr(vb), ptr(vc), vk, ptr(c), 0 if c is None else c.numel(), float(data_mean),
                                                    float(data_std), ptr(labels), ptr(image), ptr(resized),
                                                    torch.cuda.current_stream().cuda_stream), "mmvae_resize_quantise_normalise")
    return labels, image, resized


def _resize_args(frames_u8, size, clip_index, what):
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or not frames_u8.is_cuda:
        raise ValueError(f"{what} expects a uint8 tensor on the GPU")
    if frames_u8.dim() < 2:
        raise ValueError(f"{what} expects frames of shape [..., H, W]")
    size = _size_pair(size)
    idx = None
    if clip_index is not None:
        if frames_u8.dim() < 3:
            raise ValueError(f"{what}: clip_index needs a leading clip axis")
        idx = _checked_clip_index(clip_index, frames_u8.shape[0], frames_u8.device, what)
    native = size == (int(frames_u8.shape[-2]), int(frames_u8.shape[-1]))
    return size, idx, native


def resize_frames(frames_u8, size, clip_index=None):
    """``transforms.Resize`` of the reference's input transform (main.py:33-36) on the device: every (H, W) plane of the uint8 device
    tensor ``frames_u8`` [..., H, W] is resized as a PIL mode-``L`` image, independently -- what the reference does to an MNIST image
    (its resize branch cannot take a 20-channel Moving-MNIST item: ToPILImage stops at 4 channels).  The bytes are PIL's
    ``Image.resize(..., Image.BILINEAR)`` exactly: antialiased triangle filter, 22-bit fixed-point taps, the horizontal pass first,
    uint8 rounding behind each pass.  ``size``: an int S (S x S; the reference only ever resizes square images) or an ``(h, w)``
    pair; sides up to 128.  ``clip_index`` (int64 indices into the leading axis, checked against it first: one device -> host read)
    resizes only those clips, in that order, without materialising the gather.  Returns uint8 [..., S_h, S_w]; at the native size
    the input comes back (gathered if asked) and nothing is launched."""
    size, idx, native = _resize_args(frames_u8, size, clip_index, "resize_frames")
    if native:
        return frames_u8 if idx is None else frames_u8.index_select(0, idx)
    return _resize_launch(frames_u8, size, None, 0.0, 1.0, idx, (False, False, True))[2]


def resize_quantise_frames(frames_u8, size, centres, data_mean, data_std, clip_index=None):
    """``resize_frames`` fused with ``quantise_frames``: one launch from resident uint8 planes to ``(labels int64, image f32)`` at
    ``size`` (the second branch of the reference's choose_transformer plus the normalisation of main.py:383-387).  Equal, bit for
    bit, to ``quantise_frames(resize_frames(frames_u8, size), centres, data_mean, data_std)``.  At the native size this IS
    ``quantise_frames``."""
    size, idx, native = _resize_args(frames_u8, size, clip_index, "resize_quantise_frames")
    if native:
        return quantise_frames(frames_u8 if idx is None else frames_u8.index_select(0, idx), centres, data_mean, data_std)
    labels, image, _ = _resize_launch(frames_u8, size, centres, data_mean, data_std, idx, (True, True, False))
    return labels, image


def choose_transformer(centres, args):
    """The reference's dispatch rule (choose_transformer, main.py:27-38) over device uint8 batches: MNIST at 28 and MovingMNIST at 64
    only quantise, every other ``args.input_image_size`` resizes to it first.  Returns a callable: uint8 device batch (B, ..., H, W)
    -> int64 k-means labels of shape (B, -1), what the reference's loader yields per item."""
    dataset, size = getattr(args, "dataset", "MovingMNIST"), int(args.input_image_size)
    c = torch.as_tensor(centres, dtype=torch.float32).reshape(-1)
    if (dataset == "MNIST" and size == 28) or (dataset == "MovingMNIST" and size == 64):
        def transform(batch_u8):
            labels, _ = quantise_frames(batch_u8, c, 0.0, 1.0)
            return labels.view(labels.shape[0], -1)
    else:
        def transform(batch_u8):
            _resize_args(batch_u8, size, None, "choose_transformer")
            labels = _resize_launch(batch_u8, (size, size), c, 0.0, 1.0, None, (True, False, False))[0]
            return labels.view(labels.shape[0], -1)
    return transform


def pixel_histogram(frames_u8, clip_index=None):
    """Byte histogram of uint8 frames on the device: a (256,) int64 device tensor, ``counts[b]`` = occurrences of byte ``b``
    (exact; integer atomics, so the same bits every run).  ``frames_u8``: a contiguous uint8 device tensor of any alignment whose
    leading axis is the clip axis.  ``clip_index`` (int64 indices into that axis; repeats count again) histograms only those
    clips, without materialising a gather -- the reference's "3000 random clips" (utils.py:284); the indices are checked against
    the clip axis first (one device -> host read), since the kernel trusts them."""
    from ._lib import check, lib, ptr
    f = frames_u8.contiguous()
    if f.dtype != torch.uint8 or not f.is_cuda:
        raise ValueError("pixel_histogram expects a uint8 tensor on the GPU")
    if f.dim() < 1:
        raise ValueError("pixel_histogram expects a leading clip axis")
    counts = torch.zeros(256, dtype=torch.int64, device=f.device)
    n = f.shape[0]
    clip_bytes = f.numel() // n if n else 0
    idx = None
    if clip_index is not None:
        idx = torch.as_tensor(clip_index, dtype=torch.int64, device=f.device).reshape(-1).contiguous()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise IndexError(f"pixel_histogram: clip_index outside [0, {n})")
        n = idx.numel()
    with torch.cuda.device(f.device):
        check(lib().mmvae_u8_histogram(ptr(f), clip_bytes, ptr(idx), n, ptr(counts), torch.cuda.current_stream().cuda_stream),
              "mmvae_u8_histogram")
    return counts


class QuantiserFit:
    """What ``fit_quantiser`` returns.  ``centres``: (q,) f64, ASCENDING, on the ToTensor scale [0, 1] -- label k is the k-th darkest
    cluster (scikit-learn's label order is arbitrary, and ``data_mean`` / ``data_std``, statistics of the labels, follow the order:
    use a quantiser with its own statistics).  ``data_mean`` / ``data_std``: mean and population std of the labels, unrounded.
    ``ratios``: (q,) class frequencies.  ``counts``: (256,) int64 histogram the fit was made on.  ``inertia``: the k-means
    objective on the ToTensor scale.  ``lut``: (256,) uint8, the label ``quantise_frames`` gives each byte with these centres."""

    def __init__(self, centres, data_mean, data_std, ratios, counts, inertia, lut):
        self.centres, self.data_mean, self.data_std, self.ratios = centres, data_mean, data_std, ratios
        self.counts, self.inertia, self.lut = counts, inertia, lut

    def weights(self, device=None):
        """``args.data_ratio_of_labels`` under ``--weighted_entropy`` (main.py:481): ``1 - ratios`` as a float tensor."""
        return torch.tensor(1.0 - self.ratios, dtype=torch.float32, device=device)


def _fit_counts(counts, n_clusters):
    """Host half of fit_quantiser: (256,) counts -> QuantiserFit through the library's exact 1-D k-means and label statistics."""
    from ._lib import check, lib
    q = int(n_clusters)
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    if counts.shape != (256,):
        raise ValueError("expected 256 counts")
    centres = np.zeros(max(q, 1), dtype=np.float64)
    inertia = np.zeros(1, dtype=np.float64)
    check(lib().mmvae_kmeans1d_fit(counts.ctypes.data, q, centres.ctypes.data, inertia.ctypes.data), "mmvae_kmeans1d_fit")
    c32 = centres.astype(np.float32)                      # what quantise_frames hands the kernel
    lut = np.zeros(256, dtype=np.uint8)
    ratios = np.zeros(q, dtype=np.float64)
    stats = np.zeros(2, dtype=np.float64)
    check(lib().mmvae_quantiser_stats(counts.ctypes.data, c32.ctypes.data, q, lut.ctypes.data, ratios.ctypes.data, stats.ctypes.data,
                                      stats.ctypes.data + 8), "mmvae_quantiser_stats")
    return QuantiserFit(centres, float(stats[0]), float(stats[1]), ratios, counts.astype(np.int64), float(inertia[0]), lut)


def fit_quantiser(source, n_clusters, clips=None, generator=None):
    """Fit the k-means pixel quantiser on the device (the fit of utils.save_kmeans_file, utils.py:279-309): one histogram launch
    over the resident uint8 data, one 2 KB device -> host copy, then the exact 1-D k-means and the label statistics on those 256
    numbers.  ``source``: a uint8 device tensor (leading axis = clips) or a ``MovingMNISTClips``.  ``clips=None`` uses every clip
    -- no sampling noise in ``data_mean`` / ``data_std``; an int draws that many DISTINCT clips with ``generator`` (the reference
    uses 3000).  Deterministic given the clips; never worse than Lloyd's iterations.  Returns a ``QuantiserFit``."""
    frames = source.clips if isinstance(source, MovingMNISTClips) else source
    idx = None
    if clips is not None:
        n, k = frames.shape[0], int(clips)
        if not 0 < k <= n:
            raise ValueError(f"fit_quantiser: clips={k} of {n} available")
        gdev = generator.device if generator is not None else "cpu"
        idx = torch.randperm(n, generator=generator, device=gdev)[:k]
    counts = pixel_histogram(frames, idx).cpu().numpy()                 # the one device -> host copy
    return _fit_counts(counts, n_clusters)


KMEANS_FILE_NOTE = ("k-means pixel quantiser: data only (numpy arrays), not a pickle. centres ascending on the [0, 1] scale; "
                    "data_mean / data_std / ratios rounded to 4 digits; counts = the byte histogram fitted on.")


def save_kmeans_file(n_clusters, dataset="MovingMNIST", folder="data", source=None, device="cuda"):
    """The reference's entry point (utils.py:279-309) on the device.  ``source`` None loads ``folder``/movingmnisttrain.npz; else
    an (N, C, W, H) uint8 array in the file's layout, a uint8 device tensor or a ``MovingMNISTClips``.  Fits on every clip, rounds
    ``data_mean`` / ``data_std`` / ``ratios`` to 4 digits as utils.py:303-305 does, and writes ``folder``/kmeans_{dataset}_{q}.npz
    (arrays only: centres, data_mean, data_std, ratios, counts and a note -- NOT the reference's joblib pickle of an sklearn
    object; read it with ``load_kmeans_file``).  Returns ``(centres, data_mean, data_std, ratios)`` like utils.py:309, centres
    of shape (q, 1) as ``kmeans.cluster_centers_``."""
    import os
    if source is None:
        path = os.path.join(folder, "movingmnisttrain.npz")
        if not os.path.isfile(path):
            raise FileNotFoundError(path)
        source = np.load(path)["arr_0"]
    if isinstance(source, np.ndarray):
        source = clips_from_npz_array(source).to(device)
    fit = fit_quantiser(source, n_clusters)
    data_mean, data_std, ratios = round(fit.data_mean, 4), round(fit.data_std, 4), fit.ratios.round(4)
    os.makedirs(folder, exist_ok=True)
    np.savez(os.path.join(folder, "kmeans_{:}_{:}.npz".format(dataset, int(n_clusters))), centres=fit.centres,
             data_mean=np.float64(data_mean), data_std=np.float64(data_std), ratios=ratios, counts=fit.counts, note=np.str_(KMEANS_FILE_NOTE))
    return fit.centres.reshape(-1, 1), data_mean, data_std, ratios


def load_kmeans_file(path):
    """Reads a file ``save_kmeans_file`` wrote (never unpickles): {'centres' (q,) f64, 'data_mean', 'data_std' floats, 'ratios' (q,),
    'counts' (256,) int64}."""
    with np.load(path, allow_pickle=False) as d:
        return {"centres": d["centres"].astype(np.float64), "data_mean": float(d["data_mean"]), "data_std": float(d["data_std"]),
                "ratios": d["ratios"].astype(np.float64), "counts": d["counts"].astype(np.int64)}


def clips_from_npz_array(arr) -> torch.Tensor:
    """File layout of movingmnist{train,test}.npz ['arr_0'] is (N, C, W, H) uint8.  The reference dataset transposes it to
    (N, H, W, C) (movingmnistdataset.py:15) and ToTensor turns every sample into (C, H, W) (main.py:29-31): net effect, the
    last two axes swap.  Returns the (N, C, H, W) uint8 tensor of clips the rest of the input pipeline works on (host memory)."""
    a = np.asarray(arr)
    if a.ndim != 4 or a.dtype != np.uint8:
        raise ValueError("expected a uint8 array of shape (N, C, W, H)")
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 1, 3, 2)))


class MovingMNISTClips:
    """Device-side replacement for ``DataLoader(MovingMNISTDataset(...), transform=ToTensor + kmeans.predict)``
    (movingmnistdataset.py:8-27, main.py:21-38, :491-500): the whole uint8 dataset sits in HBM (10 000 clips x 20 x 64 x 64 =
    819 MB), a batch is an index gather + ONE quantise kernel, and the iterator yields what the reference's loader yields --
    int64 k-means labels of shape (B, C*H*W) -- so ``train()`` consumes it unchanged.  No host work per step.

    source: a folder holding movingmnisttrain.npz / movingmnisttest.npz, or an (N, C, W, H) uint8 array in the file's layout.
    centres: the q k-means centres on the ToTensor scale [0, 1] (kmeans_dict['kmeans'].cluster_centers_.ravel()), or None: call
    ``fit_quantiser`` before iterating.
    image_size: None or the clips' own H: as above.  Another S: the reference's resize branch (``--input_image_size`` S, its default
    being 32) -- the gather, ``resize_frames`` and the quantiser are ONE launch and the iterator yields labels of shape (B, C*S*S).
    ``fit_quantiser`` still fits on the native bytes, as the reference's save_kmeans_file does; for label statistics at S fit on
    ``resize_frames(loader.clips, S)`` instead (``fit_quantiser(resize_frames(loader.clips, S), q)``)."""

    def __init__(self, source, centres, batch_size, device, train=True, shuffle=True, seed=None, drop_last=False, image_size=None):
        import os
        if isinstance(source, (str, os.PathLike)):
            path = os.path.join(source, "movingmnisttrain.npz" if train else "movingmnisttest.npz")
            if not os.path.isfile(path):
                raise FileNotFoundError(path)
            source = np.load(path)["arr_0"]
        self.device = torch.device(device)
        self.clips = clips_from_npz_array(source).to(self.device)
        self.train_data = self.clips                  # len(dataset.train_data) is read by main.py:506
        self.centres = None if centres is None else torch.as_tensor(centres, dtype=torch.float32).reshape(-1)
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), bool(shuffle), bool(drop_last)
        self.image_size = None if image_size is None else _size_pair(image_size)
        if self.image_size is not None and self.image_size[0] != self.image_size[1]:
            raise ValueError("image_size is one int S (the model's input_image_size)")
        self._gen = torch.Generator(device="cpu")
        if seed is not None:
            self._gen.manual_seed(int(seed))

    def __len__(self):
        n = self.clips.shape[0]
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def fit_quantiser(self, n_clusters, clips=None, generator=None):
        """Fits the quantiser on the resident clips (module-level ``fit_quantiser``), installs its centres and returns the
        ``QuantiserFit`` (``data_mean`` / ``data_std`` for ``train``, ``weights()`` for ``args.data_ratio_of_labels``)."""
        fit = fit_quantiser(self, n_clusters, clips=clips, generator=generator)
        self.centres = torch.as_tensor(fit.centres, dtype=torch.float32).reshape(-1)
        return fit

    def __iter__(self):
        if self.centres is None:
            raise RuntimeError("MovingMNISTClips has no k-means centres: pass `centres` or call .fit_quantiser(n_clusters) first")
        n = self.clips.shape[0]
        order = torch.randperm(n, generator=self._gen) if self.shuffle else torch.arange(n)
        order = order.to(self.device)
        resize = self.image_size is not None and self.image_size != tuple(self.clips.shape[-2:])
        for i in range(len(self)):
            idx = order[i * self.batch_size:(i + 1) * self.batch_size]
            if resize:                           # gather + resize + quantise in one launch (idx comes from `order`: in range)
                labels = _resize_launch(self.clips, self.image_size, self.centres, 0.0, 1.0, idx.contiguous(), (True, False, False))[0]
            else:
                frames = self.clips.index_select(0, idx)
                labels, _ = quantise_frames(frames, self.centres, 0.0, 1.0)
            yield labels.view(labels.shape[0], -1)


# ---------------------------------------------------------------------------------------------------------------------
# Picture panels: the reference's plot branch (main.py:205-359, :401-424) and the legacy utils.test pieces (utils.py:77-83, :219-264)
# ---------------------------------------------------------------------------------------------------------------------
_COLUMN_KEYS = ("kind", "tensor", "lut", "uniforms", "lo", "hi")
_COLUMN_KINDS = ("labels", "argmax", "sample", "image")


def column(kind, tensor, lut=None, uniforms=None, lo=None, hi=None):
    """One column spec of ``render_sheet``.  ``kind``: 'labels' (uint8 or int64 class labels, ``lut`` required), 'argmax' / 'sample' (f32
    logits (n, Q, S, S); ``lut`` defaults to ``gray_lut(Q)``; 'sample' needs ``uniforms`` (n, S*S)), 'image' (f32, needs ``lo`` < ``hi``)."""
    return {"kind": kind, "tensor": tensor, "lut": lut, "uniforms": uniforms, "lo": lo, "hi": hi}


def gray_lut(Q, centres=None):
    """The grey byte of each of ``Q`` classes, a uint8 (Q,) tensor.  With ``centres`` (the k-means centres of pixel / 255, one per class):
    ``floor(255 * centre + 0.5)`` clamped to [0, 255] -- the dequantised pixel.  Without: the classes spread evenly over [0, 255],
    ``(510 k + (Q - 1)) // (2 (Q - 1))`` in integer arithmetic (round-half-up of 255 k / (Q - 1)); Q = 1 gives 0."""
    Q = int(Q)
    if Q < 1:
        raise ValueError("gray_lut: Q must be positive")
    if centres is not None:
        c = np.asarray(centres.detach().cpu() if isinstance(centres, torch.Tensor) else centres, dtype=np.float64).reshape(-1)
        if c.size != Q:
            raise ValueError(f"gray_lut: {c.size} centres for Q = {Q}")
        return torch.from_numpy(np.clip(np.floor(255.0 * c + 0.5), 0, 255).astype(np.uint8))
    if Q == 1:
        return torch.zeros(1, dtype=torch.uint8)
    return torch.tensor([(510 * k + (Q - 1)) // (2 * (Q - 1)) for k in range(Q)], dtype=torch.uint8)


def _plane_side(t, lead, what):
    """Side S of the square planes behind the ``lead`` leading axes of ``t``: (..., S, S) or flat (..., S*S)."""
    rest = tuple(t.shape[lead:])
    if len(rest) == 2 and rest[0] == rest[1]:
        return int(rest[0])
    if len(rest) == 1:
        S = int(round(float(rest[0]) ** 0.5))
        if S * S == rest[0]:
            return S
    raise ValueError(f"{what}: expected square planes, got shape {tuple(t.shape)}")


def render_sheet(columns, rows):
    """8-bit greyscale contact sheet on the device, ONE launch (mmvae_panel_sheet): uint8 (rows * S, ncols * S); column c fills
    ``[:, c*S:(c+1)*S]`` with its ``rows`` planes stacked vertically -- the reference's ``x[:6].view(-1, S)`` strips side by side.
    ``columns``: specs as ``column(...)`` builds them (dicts, or tuples in that argument order).  Every source must be a device tensor
    holding exactly ``rows`` planes of one side S <= 64, all on one device: labels (rows, S, S) / (rows, 1, S, S) / (rows, S*S), logits
    (rows, Q, S, S) / (rows, Q, S*S) with Q <= 16, images (rows, S, S) / (rows, S*S), or (rows, C, S, S) which becomes one column per
    channel (the reference's ``view(-1, S)`` runs the channels down the strip; here the sheet stays rectangular).  At most 8 columns.
    Everything is checked before anything is launched; a violation raises ValueError."""
    import ctypes
    from . import _lib as L
    rows = int(rows)
    if rows < 1:
        raise ValueError("render_sheet: rows must be positive")
    if not columns:
        raise ValueError("render_sheet: no columns")
    descs, keep, S, device = [], [], None, None

    def side(s):
        nonlocal S
        if S is None:
            S = s
        if s != S:
            raise ValueError(f"render_sheet: planes of side {s} next to planes of side {S}")

    for i, spec in enumerate(columns):
        if not isinstance(spec, dict):
            spec = dict(zip(_COLUMN_KEYS, spec))
        kind, t = spec.get("kind"), spec.get("tensor")
        what = f"render_sheet: column {i} ({kind})"
        if kind not in _COLUMN_KINDS:
            raise ValueError(f"render_sheet: column {i} has kind {kind!r}, expected one of {_COLUMN_KINDS}")
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: the source must be a tensor")
        if t.dim() < 2 or t.shape[0] != rows:
            raise ValueError(f"{what}: expected exactly {rows} planes, got shape {tuple(t.shape)}")
        if not t.is_cuda:
            raise ValueError(f"{what}: the source must be on the GPU")
        if device is None:
            device = t.device
        if t.device != device:
            raise ValueError(f"{what}: source on {t.device}, the first column on {device}")
        t = t.detach()
        if kind == "image":
            lo, hi = spec.get("lo"), spec.get("hi")
            if lo is None or hi is None or not float(hi) > float(lo):
                raise ValueError(f"{what}: needs lo < hi, got lo={lo}, hi={hi}")
            if t.dtype != torch.float32:
                raise ValueError(f"{what}: expected float32, got {t.dtype}")
            planes = [t[:, c] for c in range(t.shape[1])] if t.dim() == 4 else [t]
            for p in planes:
                side(_plane_side(p, 1, what))
                p = p.contiguous()
                keep.append(p)
                descs.append((L.PANEL_IMAGE_F32, p, 0, None, None, float(lo), float(hi)))
            continue
        lut = spec.get("lut")
        if kind == "labels":
            if t.dtype not in (torch.uint8, torch.int64):
                raise ValueError(f"{what}: expected uint8 or int64 labels, got {t.dtype}")
            if lut is None:
                raise ValueError(f"{what}: labels need a lut (gray_lut(Q))")
            if t.dim() == 4:
                if t.shape[1] != 1:
                    raise ValueError(f"{what}: labels have one channel, got shape {tuple(t.shape)}")
                t = t[:, 0]
            side(_plane_side(t, 1, what))
            code, Q = (L.PANEL_LABELS_U8 if t.dtype == torch.uint8 else L.PANEL_LABELS_I64), None
        else:
            if t.dtype != torch.float32 or t.dim() not in (3, 4):
                raise ValueError(f"{what}: expected float32 logits (rows, Q, S, S), got {t.dtype} {tuple(t.shape)}")
            side(_plane_side(t, 2, what))
            code, Q = (L.PANEL_LOGITS_ARGMAX if kind == "argmax" else L.PANEL_LOGITS_SAMPLE), int(t.shape[1])
            if lut is None:
                lut = gray_lut(Q) if 1 <= Q <= L.PANEL_MAX_Q else None
        if lut is not None:
            lut = torch.as_tensor(lut)
            if lut.dtype != torch.uint8:
                raise ValueError(f"{what}: the lut must be uint8")
            lut = lut.reshape(-1)
            Q = int(lut.numel()) if Q is None else Q
            if lut.numel() != Q:
                raise ValueError(f"{what}: lut of {lut.numel()} entries for Q = {Q}")
        if not 1 <= Q <= L.PANEL_MAX_Q:
            raise ValueError(f"{what}: Q = {Q} classes, supported 1..{L.PANEL_MAX_Q}")
        u = None
        if kind == "sample":
            u = spec.get("uniforms")
            if not isinstance(u, torch.Tensor) or u.device != device or u.numel() != rows * S * S:
                raise ValueError(f"{what}: needs uniforms (rows, S*S) on {device}")
            u = u.detach().contiguous().float()
        t, lut = t.contiguous(), lut.to(device).contiguous()
        keep += [t, lut, u]
        descs.append((code, t, Q, u, lut, 0.0, 1.0))
    if not 1 <= S <= L.PANEL_MAX_S:
        raise ValueError(f"render_sheet: side {S} unsupported (1..{L.PANEL_MAX_S})")
    if len(descs) > L.PANEL_MAX_COLS:
        raise ValueError(f"render_sheet: {len(descs)} columns, at most {L.PANEL_MAX_COLS} fit one sheet")
    arr = (L.PanelCol * len(descs))(*[L.PanelCol(code, L.ptr(t), Q, L.ptr(u), L.ptr(lut), lo, hi) for code, t, Q, u, lut, lo, hi in descs])
    out = torch.empty((rows * S, len(descs) * S), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        L.check(L.lib().mmvae_panel_sheet(ctypes.addressof(arr), len(descs), rows, S, L.ptr(out), torch.cuda.current_stream().cuda_stream),
                "mmvae_panel_sheet")
    return out


def write_png_gray(path, sheet):
    """Writes a uint8 (H, W) sheet (device or host tensor, or array) as an 8-bit greyscale PNG with the standard library only (zlib,
    struct): one device -> host copy of the bytes, no filtering (filter type 0 on every row).  Returns ``path``."""
    import struct
    import zlib
    a = sheet.detach().cpu().numpy() if isinstance(sheet, torch.Tensor) else np.asarray(sheet)       # the one device -> host copy
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png_gray expects a non-empty uint8 (H, W) sheet")
    h, w = a.shape
    raw = np.zeros((h, w + 1), dtype=np.uint8)           # a filter byte (0: none) in front of every row
    raw[:, 1:] = a

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0))
           + chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)
    return path


_SCATTER_TONES = {}                    # device -> scatter_tone() there (the default table is copied once per device)


def scatter_tone(alpha=0.1):
    """The grey of a pixel under k overlapping markers, a uint8 (256,) host tensor: ``tone[k] = round(255 (1 - alpha)^k)`` -- black
    ink of opacity ``alpha`` (the reference's ``alpha=0.1``, main.py:172-173) composited k times over white; counts saturate at 255."""
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("scatter_tone: alpha must lie in [0, 1]")
    k = np.arange(256, dtype=np.float64)
    return torch.from_numpy(np.floor(255.0 * (1.0 - alpha) ** k + 0.5).astype(np.uint8))


def _scatter_points(points, what):
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise ValueError(f"{what} expects a float32 tensor on the GPU")
    if points.dtype != torch.float32:
        raise ValueError(f"{what}: expected float32 points, got {points.dtype}")
    if points.dim() == 4 and points.shape[2] == 1 and points.shape[3] == 1:
        points = points.reshape(points.shape[0], points.shape[1])
    if points.dim() != 2 or points.shape[1] < 1:
        raise ValueError(f"{what}: expected points of shape (N, z) or (N, z, 1, 1), got {tuple(points.shape)}")
    return points.detach().contiguous()


def _scatter_xform(pts, dims, lims, side):
    """The four device floats of mmvae_scatter_panel, {xlim, ylim, 8 side / xlim, 8 side / ylim}, without a host read.  lims None:
    ``max|.| + 4`` per axis (main.py:170-171; 4 for no points)."""
    if lims is None:
        if pts.shape[0] == 0:
            lim = torch.full((2,), 4.0, dtype=torch.float32, device=pts.device)
        else:
            lim = pts[:, list(dims)].abs().amax(dim=0) + 4.0
    else:
        lim = torch.as_tensor(lims, dtype=torch.float32).to(pts.device).reshape(-1)
        if lim.numel() != 2:
            raise ValueError("scatter_panel: lims is (xlim, ylim)")
    return torch.cat([lim, float(8 * side) / lim]).contiguous()


def _scatter_launch(pts, dims, xform, side, radius16, tone, out):
    from . import _lib as L
    with torch.cuda.device(pts.device):
        L.check(L.lib().mmvae_scatter_panel(L.ptr(pts) if pts.shape[0] else None, pts.shape[0], pts.shape[1], dims[0], dims[1], L.ptr(xform),
                                            side, radius16, L.ptr(tone), L.ptr(out), out.stride(0), torch.cuda.current_stream().cuda_stream),
                "mmvae_scatter_panel")
    return out


def _scatter_args(points, dims, side, radius, tone, out, what):
    from . import _lib as L
    pts = _scatter_points(points, what)
    dims = tuple(int(v) for v in dims)
    if len(dims) != 2 or not all(0 <= v < pts.shape[1] for v in dims):
        raise ValueError(f"{what}: dims {dims} outside the {pts.shape[1]} columns of the points")
    side = int(side)
    if side % 16 or not 16 <= side <= L.SCATTER_MAX_SIDE:
        raise ValueError(f"{what}: side {side} unsupported (a multiple of 16 in 16..{L.SCATTER_MAX_SIDE})")
    radius16 = int(round(float(radius) * 16.0))
    if not L.SCATTER_MIN_RADIUS16 <= radius16 <= L.SCATTER_MAX_RADIUS16:
        raise ValueError(f"{what}: radius {radius} unsupported ({L.SCATTER_MIN_RADIUS16 / 16}..{L.SCATTER_MAX_RADIUS16 / 16} pixels)")
    if tone is None:
        tone = _SCATTER_TONES.get(pts.device)
        if tone is None:
            tone = _SCATTER_TONES[pts.device] = scatter_tone().to(pts.device)
    else:
        tone = torch.as_tensor(tone)
        if tone.dtype != torch.uint8 or tone.numel() != 256:
            raise ValueError(f"{what}: tone is 256 uint8 values (scatter_tone())")
        tone = tone.reshape(-1).to(pts.device).contiguous()
    if out is None:
        out = torch.empty((side, side), dtype=torch.uint8, device=pts.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (side, side) or out.device != pts.device
          or out.stride(1) != 1 or out.stride(0) < side):
        raise ValueError(f"{what}: out must be a uint8 ({side}, {side}) tensor on {pts.device} with contiguous rows (a slice of a sheet will do)")
    return pts, dims, side, radius16, tone, out


def scatter_panel(points, *, dims=(0, 1), lims=None, side=256, radius=4.0, tone=None, out=None):
    """Density panel of 2-D points on the device, ONE launch (mmvae_scatter_panel): a uint8 (side, side) device tensor.  ``points``:
    float32 (N, z) or (N, z, 1, 1) on the GPU, read in place; ``dims`` picks the two plotted columns (the reference plots latent
    dimensions 0 and 1).  The panel spans [-xlim, xlim] x [-ylim, ylim], y pointing up; ``lims=None`` takes ``max|.| + 4`` per axis
    as main.py:170-171 does, computed on the device without a host read; otherwise ``(xlim, ylim)`` as floats or a tensor.  Every point
    is a disc of ``radius`` pixels (0.75 .. 8, in sixteenths) placed on a grid of 16 sub-positions per pixel; a pixel whose centre lies
    under k discs gets ``tone[k]`` (``scatter_tone()`` by default: k markers of alpha 0.1 over white).  Points with a non-finite
    coordinate or outside the limits by more than their radius are skipped.  ``out``: a uint8 (side, side) view with contiguous rows
    to render into (half of a sheet).  Integer counts: the same bytes every run and for every order of the points.  This is a density
    image under that rule, not a pixel copy of a matplotlib figure: no antialiased marker edges, axes, titles or tick labels."""
    pts, dims, side, radius16, tone, out = _scatter_args(points, dims, side, radius, tone, out, "scatter_panel")
    return _scatter_launch(pts, dims, _scatter_xform(pts, dims, lims, side), side, radius16, tone, out)


def scatter_plot(encoding, directory, epoch, plot_count, *, generator=None, prior=None, side=256, radius=4.0, save=True,
                 return_tensors=False):
    """main.py:166-183 on the device: one uint8 (side, 2 * side) sheet, ``p(z)`` on the left and ``q(z|x)`` on the right, written as
    ``<directory>/scatter-<epoch>-<plot_count>.png`` with ``save``.  ``encoding``: (N, z) or (N, z, 1, 1) float32 on the GPU; its
    dimensions 0 and 1 are plotted.  The prior points are ``torch.randn(N, 2)`` drawn through ``generator`` (``prior``: (N, 2) points
    to use instead).  Both halves share the limits of ``q(z|x)``, ``max|.| + 4`` per axis (the reference's axes are sharex / sharey and
    its limits come from the encoding).  Two ``scatter_panel`` launches into the halves of one sheet, no host read before the PNG.
    ``return_tensors=True`` returns ``(sheet, {'prior', 'xform'})``: the prior points and the four device floats {xlim, ylim, sx, sy}
    both panels were rendered with.  A density image, not a copy of the matplotlib figure (see ``scatter_panel``)."""
    sheet_side = int(side)
    pts, dims, side, radius16, tone, _ = _scatter_args(encoding, (0, 1), sheet_side, radius, None, None, "scatter_plot")
    if pts.shape[1] < 2:
        raise ValueError("scatter_plot needs at least two latent dimensions")
    if prior is None:
        prior = _draw(torch.randn, (pts.shape[0], 2), pts.device, generator)
    prior = _scatter_points(prior.to(pts.device), "scatter_plot")
    if prior.shape[1] != 2:
        raise ValueError(f"scatter_plot: prior must be (N, 2), got {tuple(prior.shape)}")
    xform = _scatter_xform(pts, dims, None, side)
    sheet = torch.empty((side, 2 * side), dtype=torch.uint8, device=pts.device)
    _scatter_launch(prior, (0, 1), xform, side, radius16, tone, sheet[:, :side])
    _scatter_launch(pts, dims, xform, side, radius16, tone, sheet[:, side:])
    if save:
        import os
        os.makedirs(directory, exist_ok=True)
        write_png_gray(os.path.join(directory, "scatter-{}-{}.png".format(epoch, plot_count)), sheet)
    return (sheet, {"prior": prior, "xform": xform}) if return_tensors else sheet


def _add_scatter(sheets, tensors, encoding, generator):
    """``scatter=True`` of the plot functions: the last sheet, from the last draw taken from ``generator``."""
    sheets["scatter"], t = scatter_plot(encoding.detach().float(), None, 0, 0, generator=generator, save=False, return_tensors=True)
    tensors["scatter_prior"], tensors["scatter_xform"] = t["prior"], t["xform"]


def sample_from_reconstruction(reconstruction, uniforms=None, generator=None):
    """The reference's legacy ``utils.sample_from_recostruction`` (utils.py:77-83): one draw per pixel from the softmax of a logits tensor
    (N, Q, H, W), on the device (``decode_labels`` in sample mode).  Returns the int64 labels (N, H, W) -- the reference goes on to
    normalise them with MNIST's constants; ``(labels - mean) / std`` does that for any data."""
    from .model import decode_labels
    return decode_labels(reconstruction, mode="sample", uniforms=uniforms, generator=generator)


def _draw(fn, shape, device, generator):
    """torch.randn / torch.rand through ``generator`` wherever it lives (a host generator draws on the host, then one copy)."""
    device = torch.device(device)
    if generator is not None and generator.device.type != device.type:
        return fn(shape, generator=generator, device=generator.device, dtype=torch.float32).to(device)
    return fn(shape, generator=generator, device=device, dtype=torch.float32)


class _plot_mode:
    """eval mode + no_grad for the length of a plot; the model's previous mode comes back (the reference leaves it in eval mode, which
    only works because its loop calls model.train() at the top of every step)."""

    def __init__(self, model):
        self.model, self.grad = model, torch.no_grad()

    def __enter__(self):
        self.was_training = bool(self.model.training)
        self.model.eval()
        self.grad.__enter__()

    def __exit__(self, *exc):
        self.grad.__exit__(*exc)
        self.model.train(self.was_training)
        return False


def _n_classes(model):
    if model.pixelcnn is not None:
        return int(model.pixelcnn_out_channels)
    if model.decoder_out_channels > model.in_channels:
        return int(model.decoder_out_channels)
    return None


def _plot_setup(model, data_mean, data_std, centres, lo, hi):
    """(lo, hi, lut): the f32 range [label 0, label Q - 1] on the normalised scale and the grey of each class.  Q: the model's class
    count; a Gaussian model has none, there len(centres), else 2 (the reference's default --quantization)."""
    Q = _n_classes(model)
    n_c = None if centres is None else int(np.asarray(centres.detach().cpu() if isinstance(centres, torch.Tensor) else centres).size)
    levels = Q or n_c or 2
    lut = None if Q is None else gray_lut(Q, centres if n_c == Q else None)
    if lo is None:
        lo = (0.0 - float(data_mean)) / float(data_std)
    if hi is None:
        hi = (max(levels - 1, 1) - float(data_mean)) / float(data_std)
    return float(lo), float(hi), lut


def _fit_planes(t, S):
    """The leading S x S of every plane.  The decoder's crop (model.py:307-310, :328-329) takes (32 - S) // 2 off both ends, which leaves
    an odd S one row and one column too many; next to an S x S input a sheet can only show S of them."""
    return t[..., :S, :S] if t.shape[-1] > S or t.shape[-2] > S else t


def _finish_plot(sheets, tensors, directory, epoch, plot_count, save, return_tensors):
    if save:
        import os
        os.makedirs(directory, exist_ok=True)
        for name, sheet in sheets.items():
            write_png_gray(os.path.join(directory, "{}-{}-{}.png".format(name, epoch, plot_count)), sheet)
    return (sheets, tensors) if return_tensors else sheets


def plot_vae(model, device, image, reconstruction, encoding, directory, epoch, plot_count, *, data_mean=0.0, data_std=1.0, centres=None,
             rows=6, generator=None, save=True, return_tensors=False, lo=None, hi=None, scatter=False):
    """main.py:205-245 on the device.  Sheets (uint8 device tensors, written as ``<directory>/<name>-<epoch>-<plot_count>.png`` with
    ``save``): ``recon`` = Input | Reconstruction, ``normal_sampling`` = ``get_reconstruction(z)`` of ``z ~ N(0, I)`` drawn through
    ``generator``.  A categorical decoder (``decoder_out_channels > in_channels``) is rendered as the per-pixel argmax through
    ``gray_lut(Q, centres)``, a Gaussian one as f32.  f32 columns map [lo, hi] to [0, 255]; the defaults are the normalised values of
    label 0 and label Q - 1, ``(k - data_mean) / data_std`` (the reference's plot_vae takes no statistics and lets imshow autoscale:
    pass the ones ``train`` was given).  Runs in eval mode under ``torch.no_grad()`` and restores the model's mode; no parameter or
    buffer changes.  ``rows``: images per column (the reference's 6; fewer if the batch is smaller).  At an odd ``input_image_size`` the
    decoder's crop leaves one row and column too many (model.py:307-310); the sheet shows the leading S x S.  ``scatter=True`` appends the
    reference's scatter plot of the WHOLE ``encoding`` (main.py:244) as a last sheet, ``scatter`` (``scatter_plot``); its prior draw is the
    last one taken from ``generator``, so the other sheets do not depend on the flag.  ``return_tensors=True`` returns
    ``(sheets, tensors)`` with every tensor the columns were rendered from."""
    with _plot_mode(model):
        lo, hi, lut = _plot_setup(model, data_mean, data_std, centres, lo, hi)
        img = image[:rows].detach().float()
        n, S = img.shape[0], img.shape[-1]
        rec = _fit_planes(reconstruction[:rows].detach(), S)
        random_encoding = _draw(torch.randn, tuple(encoding[:rows].shape), device, generator)
        output_random_encoding = _fit_planes(model.get_reconstruction(random_encoding), S)
        if model.decoder_out_channels > model.in_channels:
            def col(t):
                return column("argmax", t, lut)
        else:
            def col(t):
                return column("image", t.float(), lo=lo, hi=hi)
        sheets = {"recon": render_sheet([column("image", img, lo=lo, hi=hi), col(rec)], n),
                  "normal_sampling": render_sheet([col(output_random_encoding)], n)}
        tensors = {"image": img, "reconstruction": rec, "random_encoding": random_encoding,
                   "output_random_encoding": output_random_encoding, "lut": lut, "lo": lo, "hi": hi}
        if scatter:
            _add_scatter(sheets, tensors, encoding, generator)
    return _finish_plot(sheets, tensors, directory, epoch, plot_count, save, return_tensors)


def plot_pixelcnn(model, device, image, reconstruction, directory, epoch, plot_count, data_mean, data_std, *, centres=None, rows=6,
                  generator=None, save=True, return_tensors=False, lo=None, hi=None):
    """main.py:248-281 on the device.  ``recon`` = Input | argmax of ``reconstruction``; ``sample`` = argmax of the sampler's last logits
    | the drawn labels, the sampler (``model.sample_pixels``, uniforms through ``generator``) starting from ``-data_mean / data_std`` as
    main.py:264 does.  The sample column is rendered from the drawn LABELS, not from the normalised f32 values the sampler writes: no
    class can land on a rounding boundary.  Otherwise as ``plot_vae``."""
    with _plot_mode(model):
        lo, hi, lut = _plot_setup(model, data_mean, data_std, centres, lo, hi)
        img, rec = image[:rows].detach().float(), reconstruction[:rows].detach()
        n, S = img.shape[0], model.input_image_size
        sample = torch.zeros(tuple(img.shape), device=img.device) - data_mean / data_std
        uniforms = _draw(torch.rand, (n, S * S), img.device, generator)
        sample_logits, sample, _, sample_labels = model.sample_pixels(sample, None, data_mean=data_mean, data_std=data_std, uniforms=uniforms,
                                                                      return_probs=True)
        sheets = {"recon": render_sheet([column("image", img, lo=lo, hi=hi), column("argmax", rec, lut)], n),
                  "sample": render_sheet([column("argmax", sample_logits, lut), column("labels", sample_labels, lut)], n)}
        tensors = {"image": img, "reconstruction": rec, "sample_logits": sample_logits, "sample": sample, "sample_labels": sample_labels,
                   "uniforms": uniforms, "lut": lut, "lo": lo, "hi": hi}
    return _finish_plot(sheets, tensors, directory, epoch, plot_count, save, return_tensors)


def plot_pixelvae(model, device, image, reconstruction, encoding, directory, epoch, plot_count, data_mean, data_std, *, centres=None,
                  rows=6, generator=None, save=True, return_tensors=False, lo=None, hi=None, scatter=False):
    """main.py:283-359 on the device.  ``recon_z_`` = Input | z_image (one column per decoder channel) | argmax of the teacher-forced
    ``reconstruction`` | argmax of the free-running sampler's last logits | its drawn labels; ``normal-recon`` = the same five from
    ``z ~ N(0, I)``, the teacher-forced column being ``run_pixelcnn(cat([random_z_image, image[:rows]]))`` (main.py:343).  At most 4
    decoder channels fit the 8 columns of a sheet.  One deliberate deviation: each free-running pass starts from a fresh zero
    ``sample`` (the reference hands the second pass the first one's filled sample, whose stale pixels its InstanceNorm then sees).
    Sample columns are rendered from the drawn labels.  ``scatter=True`` appends the ``scatter`` sheet of the whole ``encoding``
    (main.py:358), its prior draw being the last one taken from ``generator``.  Otherwise as ``plot_vae``."""
    with _plot_mode(model):
        lo, hi, lut = _plot_setup(model, data_mean, data_std, centres, lo, hi)
        img, rec, enc = image[:rows].detach().float(), reconstruction[:rows].detach(), encoding[:rows].detach()
        n, S = img.shape[0], model.input_image_size

        def free_running(z_img):
            u = _draw(torch.rand, (n, S * S), img.device, generator)
            logits, _, _, labels = model.sample_pixels(torch.zeros(tuple(img.shape), device=img.device), z_img, data_mean=data_mean,
                                                       data_std=data_std, uniforms=u, return_probs=True)
            return logits, labels, u

        z_image = model.get_z_image(enc).contiguous()
        free_logits, free_labels, uniforms = free_running(z_image)
        random_encoding = _draw(torch.randn, tuple(enc.shape), device, generator)
        random_z_image = model.get_z_image(random_encoding).contiguous()
        random_free_logits, random_free_labels, random_uniforms = free_running(random_z_image)
        random_tf_logits = model.run_pixelcnn(torch.cat([random_z_image, img], dim=1))

        def sheet(z_img, tf, free, labels):
            return render_sheet([column("image", img, lo=lo, hi=hi), column("image", z_img, lo=lo, hi=hi), column("argmax", tf, lut),
                                 column("argmax", free, lut), column("labels", labels, lut)], n)

        sheets = {"recon_z_": sheet(z_image, rec, free_logits, free_labels),
                  "normal-recon": sheet(random_z_image, random_tf_logits, random_free_logits, random_free_labels)}
        tensors = {"image": img, "reconstruction": rec, "z_image": z_image, "free_logits": free_logits, "free_labels": free_labels,
                   "uniforms": uniforms, "random_encoding": random_encoding, "random_z_image": random_z_image,
                   "random_tf_logits": random_tf_logits, "random_free_logits": random_free_logits,
                   "random_free_labels": random_free_labels, "random_uniforms": random_uniforms, "lut": lut, "lo": lo, "hi": hi}
        if scatter:
            _add_scatter(sheets, tensors, encoding, generator)
    return _finish_plot(sheets, tensors, directory, epoch, plot_count, save, return_tensors)


def latent_slide(model, z_first, z_end, steps=6, *, data_mean=0.0, data_std=1.0, centres=None, generator=None, uniforms=None, lo=None,
                 hi=None):
    """The slide between two latent codes of the reference's utils.test (utils.py:235-264): encodings
    ``sqrt(1 - a) * z_first + sqrt(a) * z_end`` with ``a = k / (steps - 1)``, k = 0 .. steps - 1 (``steps=1``: ``z_first`` alone), one per
    row.  A VAE gives one sheet column, ``get_z_image`` of the encodings rendered as in ``plot_vae`` (argmax for a categorical decoder);
    a PixelVAE gives z_image (one column per channel) | argmax of the free-running sampler's last logits | its drawn labels, the sampler
    starting from zeros with ``uniforms`` (steps, S*S), drawn through ``generator`` when None.  Eval mode, no_grad, mode restored.
    Returns the uint8 device sheet (steps * S, ncols * S)."""
    steps = int(steps)
    if steps < 1:
        raise ValueError("latent_slide: steps must be positive")
    if model.only_pixelcnn:
        raise ValueError("latent_slide needs a latent: the model is a PixelCNN on its own")
    with _plot_mode(model):
        lo, hi, lut = _plot_setup(model, data_mean, data_std, centres, lo, hi)
        zf, ze = (z.detach().float().reshape(1, model.z_dimensions, 1, 1) for z in (z_first, z_end))
        a = (torch.arange(steps, dtype=torch.float32, device=zf.device) / max(steps - 1, 1)).view(-1, 1, 1, 1)
        encodings = (1.0 - a) ** 0.5 * zf + a ** 0.5 * ze
        z_images = _fit_planes(model.get_z_image(encodings), model.input_image_size).contiguous()
        if model.pixelcnn is None:
            if model.decoder_out_channels > model.in_channels:
                return render_sheet([column("argmax", z_images, lut)], steps)
            return render_sheet([column("image", z_images, lo=lo, hi=hi)], steps)
        S = model.input_image_size
        if uniforms is None:
            uniforms = _draw(torch.rand, (steps, S * S), z_images.device, generator)
        sample = torch.zeros((steps, model.in_channels, S, S), device=z_images.device)
        logits, _, _, labels = model.sample_pixels(sample, z_images, data_mean=data_mean, data_std=data_std, uniforms=uniforms,
                                                   return_probs=True)
        return render_sheet([column("image", z_images, lo=lo, hi=hi), column("argmax", logits, lut), column("labels", labels, lut)], steps)


class _PlotCallback:
    """What ``make_plot_callback`` returns."""

    def __init__(self, data_mean, data_std, centres, rows, generator, save, scatter=False):
        self.data_mean, self.data_std, self.centres, self.rows, self.generator, self.save = data_mean, data_std, centres, rows, generator, save
        self.scatter = bool(scatter)
        self.plot_count, self.last, self._epoch = 0, None, None

    def __call__(self, *, model, image, reconstruction, encoding, epoch, index, directory, running):
        if epoch != self._epoch:                               # main.py:370: the count restarts with every epoch
            self._epoch, self.plot_count = epoch, 0
        kw = dict(centres=self.centres, rows=self.rows, generator=self.generator, save=self.save)
        device = image.device
        if model.pixelcnn is None:                             # main.py:405-416
            sheets = plot_vae(model, device, image, reconstruction, encoding, directory, epoch, self.plot_count, data_mean=self.data_mean,
                              data_std=self.data_std, scatter=self.scatter, **kw)
        elif model.only_pixelcnn:
            sheets = plot_pixelcnn(model, device, image, reconstruction, directory, epoch, self.plot_count, self.data_mean, self.data_std, **kw)
        else:
            sheets = plot_pixelvae(model, device, image, reconstruction, encoding, directory, epoch, self.plot_count, self.data_mean,
                                   self.data_std, scatter=self.scatter, **kw)
        self.last = {"sheets": sheets, "encoding": encoding, "running": running, "epoch": epoch, "index": index, "plot_count": self.plot_count}
        self.plot_count += 1
        return sheets


def make_plot_callback(data_mean, data_std, centres=None, rows=6, generator=None, save=True, scatter=False):
    """The plot branch of the reference's loop (main.py:401-424) as a callable for ``args.plot_callback``: ``train`` calls it every
    ``plot_every`` steps with the keywords ``model, image, reconstruction, encoding, epoch, index, directory, running``; it renders the
    sheets of ``plot_vae`` / ``plot_pixelcnn`` / ``plot_pixelvae`` (chosen as main.py:405-416 chooses), writes them under ``directory``
    with ``save``, numbers them with its own ``plot_count`` (restarting with every epoch, as the reference's does) and keeps the last
    products in ``.last`` ({'sheets', 'encoding', 'running', 'epoch', 'index', 'plot_count'}: what a logger needs).  ``scatter=True``
    adds the reference's scatter plot of the encoding (main.py:244, :358; the one item both branches log as 'Scatter Plot') as a last
    sheet, ``scatter``, for models with a latent.  Pass a ``generator`` of its own to keep the plots' random draws out of the
    training's random stream."""
    return _PlotCallback(data_mean, data_std, centres, rows, generator, save, scatter)
