"""Device-side input pipeline: what the reference does on the host between the dataset files and the train step.

uint8 frames resident on the device -> k-means labels and the normalised image (``quantise_frames``), with the reference's PIL
``Resize`` in front where it resizes (``resize_frames``, ``resize_quantise_frames``, ``choose_transformer``); the fit of the k-means
quantiser itself (``pixel_histogram``, ``fit_quantiser``, ``save_kmeans_file`` / ``load_kmeans_file``); the loader that feeds
``main.train`` from HBM (``MovingMNISTClips``); and the data itself: Moving MNIST clips generated on the device from a glyph bank
(``generate_clips``, ``generate_batch``, the endless loader ``GeneratedClips``), MNIST's IDX file (``load_idx_images``) and the two
dataset files the reference reads (``save_moving_mnist_files``).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from ._lib import call, check, lib, ptr


def _u8_on_gpu(t, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda:
        raise ValueError(f"{what} expects a uint8 tensor on the GPU")
    return t


def quantise_frames(frames_u8, centres, data_mean, data_std):
    """Device-side input pipeline: uint8 frames -> k-means labels (int64) and normalised f32 image, one
    kernel (replaces ToTensor + kmeans.predict on the host, main.py:21-38, and the normalisation of main.py:383-387)."""
    f = _u8_on_gpu(frames_u8.contiguous(), "quantise_frames")
    c = torch.as_tensor(centres, dtype=torch.float32, device=f.device).contiguous()
    labels = torch.empty(f.shape, dtype=torch.int64, device=f.device)
    image = torch.empty(f.shape, dtype=torch.float32, device=f.device)
    call("mmvae_quantise_normalise", f.device, ptr(f), f.numel(), ptr(c), c.numel(), float(data_mean), float(data_std), ptr(labels), ptr(image))
    return labels, image


_RESAMPLE_TABLES = {}                  # (in_size, out_size, device) -> (bounds int32 [out, 2], coeffs int32 [out, ksize], ksize), on the device


def _resample_tables(in_size, out_size, device):
    """Device copy of mmvae_resample_coeffs(in_size, out_size), built once per (in, out, device): later calls copy nothing."""
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
    """One mmvae_resize_quantise_normalise launch.  frames_u8: uint8 device tensor [..., H, W] (``_resize_args`` has seen it, or it is
    the loader's own clips); idx: None, or trusted int64 device indices into the leading axis of an (N, C, H, W) tensor (whole clips are
    gathered).  want: which of (labels, image, resized) to produce.  Returns the three tensors (None where not wanted), shaped
    [..., S_h, S_w] (leading axis len(idx) under a gather)."""
    f = frames_u8
    H, W = int(f.shape[-2]), int(f.shape[-1])
    out_h, out_w = size
    if idx is not None:
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
    call("mmvae_resize_quantise_normalise", f.device, ptr(f), stride, ptr(idx), per_clip, n_frames, H, W, out_h, out_w, ptr(hb), ptr(hc), hk,
         ptr(vb), ptr(vc), vk, ptr(c), 0 if c is None else c.numel(), float(data_mean), float(data_std), ptr(labels), ptr(image), ptr(resized))
    return labels, image, resized


def _resize_args(frames_u8, size, clip_index, what):
    if _u8_on_gpu(frames_u8, what).dim() < 2:
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
    f = _u8_on_gpu(frames_u8.contiguous(), "pixel_histogram")
    if f.dim() < 1:
        raise ValueError("pixel_histogram expects a leading clip axis")
    counts = torch.zeros(256, dtype=torch.int64, device=f.device)
    n = f.shape[0]
    clip_bytes = f.numel() // n if n else 0
    idx = None
    if clip_index is not None:
        idx = _checked_clip_index(clip_index, n, f.device, "pixel_histogram")
        n = idx.numel()
    call("mmvae_u8_histogram", f.device, ptr(f), clip_bytes, ptr(idx), n, ptr(counts))
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


def _load_npz_clips(folder, train=True):
    """``folder``/movingmnist{train,test}.npz ['arr_0']: the (N, C, W, H) uint8 array of the dataset file."""
    path = os.path.join(folder, "movingmnisttrain.npz" if train else "movingmnisttest.npz")
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    return np.load(path)["arr_0"]


def save_kmeans_file(n_clusters, dataset="MovingMNIST", folder="data", source=None, device="cuda"):
    """The reference's entry point (utils.py:279-309) on the device.  ``source`` None loads ``folder``/movingmnisttrain.npz; else
    an (N, C, W, H) uint8 array in the file's layout, a uint8 device tensor or a ``MovingMNISTClips``.  Fits on every clip, rounds
    ``data_mean`` / ``data_std`` / ``ratios`` to 4 digits as utils.py:303-305 does, and writes ``folder``/kmeans_{dataset}_{q}.npz
    (arrays only: centres, data_mean, data_std, ratios, counts and a note -- NOT the reference's joblib pickle of an sklearn
    object; read it with ``load_kmeans_file``).  Returns ``(centres, data_mean, data_std, ratios)`` like utils.py:309, centres
    of shape (q, 1) as ``kmeans.cluster_centers_``."""
    if source is None:
        source = _load_npz_clips(folder)
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
        if isinstance(source, (str, os.PathLike)):
            source = _load_npz_clips(source, train)
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


# ---- Moving MNIST generator (mmvae_generate_clips; the rule is stated in include/mmvae.h)

_VELOCITY_TABLES = {}                  # (speed, device) -> int32 [4096, 2] on the device


def velocity_table(speed):
    """The generator's direction table for ``speed`` (the fraction of the free range a digit travels per frame): int32 (4096, 2) on
    the host, ``[a] = (rint(speed * 65536 * cos(2 pi a / 4096)), rint(speed * 65536 * sin(2 pi a / 4096)))`` in f64."""
    speed = float(speed)
    if not 0.0 < speed <= 1.0:
        raise ValueError(f"velocity_table: speed={speed} unsupported (0 < speed <= 1)")
    from . import _lib as L
    angle = 2.0 * np.pi * np.arange(L.CLIPGEN_DIRECTIONS, dtype=np.float64) / 4096.0
    return np.stack([np.rint(speed * 65536.0 * np.cos(angle)), np.rint(speed * 65536.0 * np.sin(angle))], axis=1).astype(np.int32)


def _velocity_on(device, speed):
    key = (float(speed), str(device))
    hit = _VELOCITY_TABLES.get(key)
    if hit is None:
        hit = _VELOCITY_TABLES[key] = torch.from_numpy(velocity_table(speed)).to(device)
    return hit


def _clipgen_args(bank, n_clips, seed, first_clip, frames, canvas, digits, speed, what):
    """Every check of the generator's Python calls (nothing is launched, the library is not loaded): returns
    (n_clips, seed, first_clip, T, S, K, speed, D, G).  ``bank`` is anything with a dtype and a shape."""
    from . import _lib as L
    n_clips, seed, first_clip, T, S, K, speed = int(n_clips), int(seed), int(first_clip), int(frames), int(canvas), int(digits), float(speed)
    if getattr(bank, "dtype", None) not in (torch.uint8, np.dtype(np.uint8)) or len(bank.shape) != 3 or bank.shape[1] != bank.shape[2]:
        raise ValueError(f"{what}: bank must be a uint8 array of shape [D, G, G], got {getattr(bank, 'dtype', type(bank).__name__)} "
                         f"{tuple(getattr(bank, 'shape', ()))}")
    D, G = int(bank.shape[0]), int(bank.shape[1])
    if S % 16 or not 16 <= S <= 64:
        raise ValueError(f"{what}: canvas={S} unsupported (a multiple of 16 in 16..64)")
    if not 1 <= G <= L.CLIPGEN_MAX_G:
        raise ValueError(f"{what}: bank glyph side G={G} unsupported (1..{L.CLIPGEN_MAX_G})")
    if S - G < 1:
        raise ValueError(f"{what}: canvas={S} leaves a {G} x {G} glyph no room to move (canvas - G >= 1)")
    if not 1 <= T <= L.CLIPGEN_MAX_T:
        raise ValueError(f"{what}: frames={T} unsupported (1..{L.CLIPGEN_MAX_T})")
    if not 1 <= K <= L.CLIPGEN_MAX_K:
        raise ValueError(f"{what}: digits={K} unsupported (1..{L.CLIPGEN_MAX_K})")
    if not 1 <= D <= L.CLIPGEN_MAX_D:
        raise ValueError(f"{what}: bank of D={D} glyphs unsupported (1..2^24)")
    if not 0.0 < speed <= 1.0:
        raise ValueError(f"{what}: speed={speed} unsupported (0 < speed <= 1)")
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"{what}: seed={seed} unsupported (0..2^64 - 1)")
    if n_clips < 0:
        raise ValueError(f"{what}: n_clips={n_clips} is negative")
    if first_clip < 0 or first_clip + n_clips > 2 ** 63 - 1:
        raise ValueError(f"{what}: first_clip={first_clip} with n_clips={n_clips} unsupported (clip indices in 0..2^63 - 1)")
    return n_clips, seed, first_clip, T, S, K, speed, D, G


def generate_batch(bank, n_clips, seed, first_clip, centres, data_mean, data_std, want=(True, True, False), frames=20, canvas=64, digits=2,
                   speed=0.1):
    """Moving MNIST clips ``first_clip .. first_clip + n_clips - 1`` of ``seed`` straight into the quantiser's outputs, one launch
    (mmvae_generate_clips; the integer rule is in include/mmvae.h): ``digits`` glyphs of ``bank`` (uint8 device tensor [D, G, G]) bounce
    inside a ``canvas`` x ``canvas`` frame for ``frames`` frames, overlaps composited with max.  A clip depends on (seed, its index,
    the bank, the parameters) only.  ``want``: which of (labels int64, image f32, bytes uint8) to produce; returns the three tensors
    (None where not wanted), each (N, T, S, S) on the bank's device.  labels / image equal
    ``quantise_frames(generate_clips(...), centres, data_mean, data_std)`` bit for bit; ``centres`` is read for them only."""
    n, seed, first, T, S, K, speed, D, G = _clipgen_args(bank, n_clips, seed, first_clip, frames, canvas, digits, speed, "generate_batch")
    want = tuple(bool(w) for w in want)
    if len(want) != 3 or not any(want):
        raise ValueError("generate_batch: want is three flags (labels, image, bytes), at least one of them set")
    bank = _u8_on_gpu(bank, "generate_batch").contiguous()
    shape, dev = (n, T, S, S), bank.device
    labels = torch.empty(shape, dtype=torch.int64, device=dev) if want[0] else None
    image = torch.empty(shape, dtype=torch.float32, device=dev) if want[1] else None
    out = torch.empty(shape, dtype=torch.uint8, device=dev) if want[2] else None
    if n == 0:                                   # nothing to launch (and empty tensors have no address to hand over)
        return labels, image, out
    c = None
    if want[0] or want[1]:
        c = torch.as_tensor(centres, dtype=torch.float32, device=dev).reshape(-1).contiguous()
    call("mmvae_generate_clips", dev, ptr(bank), D, G, ptr(_velocity_on(dev, speed)), seed, first, n, T, S, K, ptr(c),
         0 if c is None else c.numel(), float(data_mean), float(data_std), ptr(labels), ptr(image), ptr(out))
    return labels, image, out


def generate_clips(bank, n_clips, seed, first_clip=0, frames=20, canvas=64, digits=2, speed=0.1):
    """The bytes of ``generate_batch``: uint8 (N, T, S, S) on the bank's device -- what ``MovingMNISTClips.clips`` holds, so
    ``fit_quantiser``, ``resize_frames``, ``nearest_frames`` and the panels take it as is."""
    return generate_batch(bank, n_clips, seed, first_clip, None, 0.0, 1.0, (False, False, True), frames, canvas, digits, speed)[2]


class GeneratedClips:
    """``MovingMNISTClips`` without a dataset file: every batch is generated on the device by ``generate_batch`` (one launch from the
    glyph bank to the int64 labels), and no clip is ever seen twice.  Same iterator contract: yields int64 k-means labels of shape
    (B, T*S*S), has ``__len__``, a ``train_data`` whose ``len`` is ``clips_per_epoch``, and ``fit_quantiser`` -- so ``train()`` consumes
    it unchanged.

    bank: uint8 [D, G, G] glyphs (``load_idx_images`` of MNIST's train-images file; a host array or tensor is copied to ``device``).
    Batch ``i`` of the ``e``-th iteration over the loader covers the clip indices from ``first_clip + e * clips_per_epoch + i * B``
    (the last batch of an epoch may be ragged).  ``image_size`` other than the canvas generates the bytes and resizes them through
    ``resize_quantise_frames``' launch (two launches); ``fit_quantiser`` still fits on the native bytes, like ``MovingMNISTClips``."""

    def __init__(self, bank, centres, batch_size, clips_per_epoch, device, seed=0, first_clip=0, image_size=None, frames=20, digits=2,
                 speed=0.1, canvas=64):
        self.batch_size, self.clips_per_epoch = int(batch_size), int(clips_per_epoch)
        if self.batch_size < 1:
            raise ValueError(f"GeneratedClips: batch_size={self.batch_size} unsupported (>= 1)")
        if self.clips_per_epoch < 1:
            raise ValueError(f"GeneratedClips: clips_per_epoch={self.clips_per_epoch} unsupported (>= 1)")
        _, self.seed, self.first_clip, self.frames, self.canvas, self.digits, self.speed, _, _ = _clipgen_args(
            bank, self.clips_per_epoch, seed, first_clip, frames, canvas, digits, speed, "GeneratedClips")
        self.image_size = None if image_size is None else _size_pair(image_size)
        if self.image_size is not None and self.image_size[0] != self.image_size[1]:
            raise ValueError("image_size is one int S (the model's input_image_size)")
        self.device = torch.device(device)
        self.bank = torch.as_tensor(bank).to(self.device).contiguous()
        self.train_data = range(self.clips_per_epoch)             # len(dataset.train_data) is read by main.py:506
        self.centres = None if centres is None else torch.as_tensor(centres, dtype=torch.float32).reshape(-1)
        self._epoch = 0

    def __len__(self):
        return (self.clips_per_epoch + self.batch_size - 1) // self.batch_size

    def _generate(self, first, n, centres, want):
        return generate_batch(self.bank, n, self.seed, first, centres, 0.0, 1.0, want, self.frames, self.canvas, self.digits, self.speed)

    def fit_quantiser(self, n_clusters, clips=4096):
        """Fits the quantiser on the ``clips`` clips from ``first_clip`` on (generated 1024 at a time into one histogram), installs its
        centres and returns the ``QuantiserFit``."""
        clips = int(clips)
        if clips < 1:
            raise ValueError(f"fit_quantiser: clips={clips} unsupported (>= 1)")
        counts = torch.zeros(256, dtype=torch.int64, device=self.device)
        for lo in range(0, clips, 1024):
            counts += pixel_histogram(self._generate(self.first_clip + lo, min(1024, clips - lo), None, (False, False, True))[2])
        fit = _fit_counts(counts.cpu().numpy(), n_clusters)                  # the one device -> host copy
        self.centres = torch.as_tensor(fit.centres, dtype=torch.float32).reshape(-1)
        return fit

    def __iter__(self):
        if self.centres is None:
            raise RuntimeError("GeneratedClips has no k-means centres: pass `centres` or call .fit_quantiser(n_clusters) first")
        epoch, self._epoch = self._epoch, self._epoch + 1
        return self._batches(self.first_clip + epoch * self.clips_per_epoch)

    def _batches(self, first):
        resize = self.image_size is not None and self.image_size != (self.canvas, self.canvas)
        for lo in range(0, self.clips_per_epoch, self.batch_size):
            n = min(self.batch_size, self.clips_per_epoch - lo)
            if resize:
                frames = self._generate(first + lo, n, None, (False, False, True))[2]
                labels = _resize_launch(frames, self.image_size, self.centres, 0.0, 1.0, None, (True, False, False))[0]
            else:
                labels = self._generate(first + lo, n, self.centres, (True, False, False))[0]
            yield labels.view(labels.shape[0], -1)


def load_idx_images(path):
    """The IDX3 ubyte file of MNIST's images (what torchvision leaves under ``raw/``: train-images-idx3-ubyte, plain or ``.gz``) as a
    uint8 array (D, rows, cols).  Checks the magic number (0x00000803: unsigned bytes, three dimensions) and that the file holds exactly
    the bytes its header announces.  Standard library and numpy only; downloads nothing."""
    import gzip
    path = os.fspath(path)
    with open(path, "rb") as fh:
        raw = fh.read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    if len(raw) < 16:
        raise ValueError(f"{path}: {len(raw)} bytes, shorter than an IDX3 header")
    magic, n, rows, cols = (int(v) for v in np.frombuffer(raw, dtype=">u4", count=4))
    if magic != 0x00000803:
        raise ValueError(f"{path}: magic number 0x{magic:08x}, an IDX3 ubyte file starts with 0x00000803")
    if len(raw) != 16 + n * rows * cols:
        raise ValueError(f"{path}: header announces {n} x {rows} x {cols} bytes, the file holds {len(raw) - 16}")
    return np.frombuffer(raw, dtype=np.uint8, offset=16).reshape(n, rows, cols).copy()


def save_moving_mnist_files(folder, bank, n_train=10000, n_test=1000, seed=0, frames=20, canvas=64, digits=2, speed=0.1, device="cuda"):
    """Writes ``folder``/movingmnisttrain.npz and movingmnisttest.npz, the two files the reference reads (movingmnistdataset.py:11-14):
    ``arr_0`` uint8 in the file layout (N, C, W, H), i.e. the generated (N, T, S, S) clips with the last two axes swapped, so that
    ``clips_from_npz_array`` / ``MovingMNISTClips(folder, ...)`` give the generated clips back exactly.  Train clips are the indices
    [0, n_train) of ``seed``, test clips [n_train, n_train + n_test): the files can be made again from (bank, seed).  ``bank``: uint8
    [D, G, G] on the host or the device.  Returns the two paths."""
    n_train, n_test = int(n_train), int(n_test)
    if n_test < 0:
        raise ValueError(f"save_moving_mnist_files: n_test={n_test} is negative")
    _clipgen_args(bank, n_train, seed, 0, frames, canvas, digits, speed, "save_moving_mnist_files")
    _clipgen_args(bank, n_test, seed, n_train, frames, canvas, digits, speed, "save_moving_mnist_files")
    dev_bank = torch.as_tensor(bank)
    if not dev_bank.is_cuda:
        dev_bank = dev_bank.to(device)
    os.makedirs(folder, exist_ok=True)
    paths = []
    for name, first, n in (("movingmnisttrain.npz", 0, n_train), ("movingmnisttest.npz", n_train, n_test)):
        arr = np.empty((n, int(frames), int(canvas), int(canvas)), dtype=np.uint8)
        for lo in range(0, n, 1024):                                 # 1024 clips = 84 MB on the device at the canonical shape
            m = min(1024, n - lo)
            clips = generate_clips(dev_bank, m, seed, first + lo, frames, canvas, digits, speed)
            arr[lo:lo + m] = clips.transpose(2, 3).cpu().numpy()
        paths.append(os.path.join(folder, name))
        np.savez(paths[-1], arr)
    return tuple(paths)
