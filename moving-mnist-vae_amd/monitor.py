"""Per-parameter histograms on the device: what ``wandb.hook_torch(model)`` logs in the reference (main.py:456).

The hook builds, for every parameter, a 64-bin histogram of its gradient from the tensor's ``min()``, ``max()`` and ``histc(bins=64)``.
The HIP model keeps all parameters in one flat f32 buffer and all gradients (and both Adam moments) in buffers of the same layout, so
``TensorHistograms`` takes every tensor's histogram, range and exact statistics in one call of ``mmvae_tensor_hist`` (three launches,
no host read): ``update()`` can run inside the train step, between ``backward`` and ``step``, without making the host wait, and inside
a captured graph.  ``make_histogram_callback`` returns what ``train`` calls through ``args.stats_callback``.

Deliberately different from the hook: NaN and inf are counted (``n_nonfinite``) and kept out of the range and the bins, where ``histc``
raises or the hook drops the tensor; the statistics (zeros, mean, rms) are exact over the whole tensor, not read off the bins; a
data-parallel model (``GradSync``) is refused, because its gradient buffer is being all-reduced on another stream at that moment.
Neither wandb nor matplotlib is imported: ``as_dict`` returns the ``np_histogram`` pairs ``wandb.Histogram`` takes.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib as L
from ._lib import MmvaeError

BINS, STATS = 64, 8                   # MMVAE_TENSOR_HIST_BINS, MMVAE_TENSOR_HIST_STATS
CHUNK = 4096                          # elements per chunk (a block of 256 threads: four 16-byte loads per thread)
WHAT = ("gradients", "parameters", "exp_avg", "exp_avg_sq")
STAT_NAMES = ("n_finite", "n_nonfinite", "n_zero", "sum", "sumsq", "mean", "rms")


def segment_table(model):
    """(names, segments): the model's parameters in ``named_parameters()`` order (a PixelCNN's first) and an int64 (T, 2) array of
    (offset, numel) into the flat buffer, in elements.  Host only."""
    tab = model._ptable
    if not tab:
        raise MmvaeError("the model has no parameters")
    seg = np.array([[off, n] for (_, _, off, n, _) in tab], dtype=np.int64).reshape(-1, 2)
    return [e.name for e in tab], seg


def chunk_list(segments, chunk=CHUNK):
    """The int64 (n, 3) chunk list (segment, start, length) of a segment table: the segments in order, each cut into pieces of at most
    ``chunk`` elements.  Host only (mmvae_tensor_hist_chunks)."""
    seg = np.ascontiguousarray(segments, dtype=np.int64).reshape(-1, 2)
    fn = L.lib().mmvae_tensor_hist_chunks
    n = fn(seg.ctypes.data, seg.shape[0], int(chunk), None, 0)
    if n < 0:
        L.check(int(n), "mmvae_tensor_hist_chunks")
    out = np.zeros((max(n, 1), 3), dtype=np.int64)
    got = fn(seg.ctypes.data, seg.shape[0], int(chunk), out.ctypes.data, out.shape[0])
    assert got == n
    return out[:n]


class TensorHistograms:
    """64-bin histograms, ranges and statistics of every parameter tensor of a HIP ``VAE``: of its gradients, its parameters, or
    ``FusedAdam``'s first / second moments (``what``; the last two need ``optimizer``).

    The tables and every output buffer are built once, here.  ``update()`` enqueues the library call on the current stream and returns
    nothing: no allocation, no host read.  Results stay on the device -- ``counts`` (T, 64) int32, ``lo`` / ``hi`` (T,) f32 (the range
    the bins span: min / max of the finite values, widened by 1 on either side when they are equal, 0 / 0 without a finite value),
    ``n_finite`` / ``n_nonfinite`` / ``n_zero`` / ``sum`` / ``sumsq`` / ``mean`` / ``rms`` (T,) f64 -- until ``as_dict()`` copies them to
    the host in one transfer.  ``names`` lists the tensors, in ``model.named_parameters()`` order."""

    def __init__(self, model, what="gradients", optimizer=None):
        if what not in WHAT:
            raise ValueError(f"what={what!r}: one of {WHAT}")
        if what in ("exp_avg", "exp_avg_sq") and optimizer is None:
            raise ValueError(f"what={what!r} reads FusedAdam's moments: pass optimizer=")
        if not hasattr(model, "_ptable") or not hasattr(model, "_flat"):
            raise MmvaeError("TensorHistograms needs the HIP VAE of this package")
        model._ensure_flat()
        dev = model._flat.device
        if dev.type != "cuda":
            raise MmvaeError("TensorHistograms needs the model on the GPU: there is no CPU fallback")
        self._model, self._opt, self.what = model, optimizer, what
        self.names, self._seg = segment_table(model)
        self._chunks = chunk_list(self._seg)
        T, n = self._seg.shape[0], self._chunks.shape[0]
        self._seg_dev = torch.from_numpy(self._seg).to(dev)
        self._chunks_dev = torch.from_numpy(np.ascontiguousarray(self._chunks)).to(dev) if n else None
        # one blob, so that as_dict() is one copy: stats f64 (T, 8) | counts int32 (T, 64) | lo f32 (T) | hi f32 (T)
        a, b, c = T * STATS * 8, T * STATS * 8 + T * BINS * 4, T * STATS * 8 + T * BINS * 4 + T * 4
        self._blob = torch.zeros(c + T * 4, dtype=torch.uint8, device=dev)
        self._cuts = (a, b, c)
        self.stats = self._blob[:a].view(torch.float64).view(T, STATS)
        self.counts = self._blob[a:b].view(torch.int32).view(T, BINS)
        self.lo, self.hi = self._blob[b:c].view(torch.float32), self._blob[c:].view(torch.float32)
        for k, name in enumerate(STAT_NAMES):
            setattr(self, name, self.stats[:, k])
        self._scratch_bytes = int(L.lib().mmvae_tensor_hist_scratch_bytes(T, n))
        self._scratch = torch.zeros(self._scratch_bytes // 8, dtype=torch.float64, device=dev)

    def _source(self):
        model = self._model
        model._ensure_flat()
        if model._flat.device != self._blob.device:
            raise MmvaeError("the model moved to another device after TensorHistograms was built")
        if self.what == "parameters":
            return model._flat
        if self.what == "gradients":
            if getattr(model, "_sync", None) is not None:
                raise MmvaeError("TensorHistograms(what='gradients') under data-parallel GradSync is not supported: the gradient buffer "
                                 "is being all-reduced on another stream between backward and step")
            from .model import FusedAdam
            G = FusedAdam._flat_grads(model)
            if G is None:
                raise MmvaeError("TensorHistograms(what='gradients'): no backward has run, the parameters have no gradients")
            return G
        m, v = self._opt._moments(model)
        return m if self.what == "exp_avg" else v

    def update(self):
        """Histogram the buffer as it is now, on the current stream.  (Gradients that autograd did not leave in the model's flat buffer
        -- ``.grad`` tensors assigned by hand -- are gathered into it first, as ``FusedAdam.step`` does: copies, not capturable.)"""
        src = self._source()
        n = self._chunks.shape[0]
        L.call("mmvae_tensor_hist", src.device, L.ptr(src), src.numel(), self._seg.ctypes.data, L.ptr(self._seg_dev), self._seg.shape[0],
               self._chunks.ctypes.data if n else None, L.ptr(self._chunks_dev), n, L.ptr(self.counts), L.ptr(self.lo), L.ptr(self.hi),
               L.ptr(self.stats), L.ptr(self._scratch), self._scratch_bytes)

    def to_host(self):
        """One device-to-host copy: {'counts' (T, 64) int32, 'lo', 'hi' (T,) f32, 'stats' (T, 8) f64} as numpy arrays."""
        raw = self._blob.cpu().numpy()
        a, b, c = self._cuts
        T = len(self.names)
        return {"stats": raw[:a].view(np.float64).reshape(T, STATS), "counts": raw[a:b].view(np.int32).reshape(T, BINS),
                "lo": raw[b:c].view(np.float32), "hi": raw[c:].view(np.float32)}

    def as_dict(self, prefix=None):
        """{prefix + name: (counts list, edges)} with ``edges = numpy.linspace(lo, hi, 65)`` -- the ``np_histogram`` pair of
        ``wandb.Histogram``, under the key names ``hook_torch`` uses -- plus ``prefix + 'stats'``: {name: {lo, hi, n_finite, n_nonfinite,
        n_zero, sum, sumsq, mean, rms}}.  ``prefix`` defaults to ``what + '/'``.  One device-to-host copy."""
        return self._pairs(self.to_host(), self.what + "/" if prefix is None else prefix)

    def _pairs(self, h, prefix):
        out, stats = {}, {}
        for t, name in enumerate(self.names):
            out[prefix + name] = (h["counts"][t].tolist(), np.linspace(float(h["lo"][t]), float(h["hi"][t]), BINS + 1))
            row = {"lo": float(h["lo"][t]), "hi": float(h["hi"][t])}
            row.update({k: float(h["stats"][t, i]) for i, k in enumerate(STAT_NAMES)})
            stats[name] = row
        out[prefix + "stats"] = stats
        return out


def tensor_histograms(model, what="gradients", optimizer=None):
    """One shot: ``TensorHistograms(model, what, optimizer)`` after one ``update()``."""
    h = TensorHistograms(model, what, optimizer)
    h.update()
    return h


class _HistogramCallback:
    """What ``make_histogram_callback`` returns."""

    def __init__(self, every, what, sink, directory):
        self.every, self.what, self.sink, self.directory = every, what, sink, directory
        self._hists = None

    def __call__(self, model, optimizer=None, epoch=0, index=0, **_):
        if index % self.every:
            return None
        if self._hists is None or self._hists[0]._model is not model:
            self._hists = [TensorHistograms(model, w, optimizer) for w in self.what]
        for h in self._hists:                      # enqueue everything first, then read
            h.update()
        out, flat = {}, {}
        for h in self._hists:
            host = h.to_host()
            out.update(h._pairs(host, h.what + "/"))
            flat[h.what + "_names"] = np.array(h.names)
            for k, v in host.items():
                flat[h.what + "_" + k] = v
        if self.sink is not None:
            self.sink(out)
        if self.directory is not None:
            os.makedirs(self.directory, exist_ok=True)
            np.savez(os.path.join(self.directory, f"hist-{epoch}-{index}.npz"), **flat)
        return out


def make_histogram_callback(every=100, what=("gradients",), sink=None, directory=None):
    """A callable for ``args.stats_callback``: ``train`` calls it between ``loss.backward()`` and ``optimizer.step()`` with ``model=,
    optimizer=, epoch=, index=``.  Every ``every``-th step it updates one ``TensorHistograms`` per entry of ``what`` and hands the merged
    ``as_dict()`` (keys ``gradients/<name>``, ...) to ``sink`` (``wandb.log``-like: any callable taking the dict) and / or writes
    ``<directory>/hist-<epoch>-<index>.npz`` (arrays ``<what>_counts``, ``<what>_lo``, ``<what>_hi``, ``<what>_stats``, ``<what>_names``)."""
    what = (what,) if isinstance(what, str) else tuple(what)
    if not what or any(w not in WHAT for w in what):
        raise ValueError(f"what={what!r}: entries of {WHAT}")
    if int(every) < 1:
        raise ValueError("every must be a positive number of steps")
    if sink is None and directory is None:
        raise ValueError("make_histogram_callback needs a sink or a directory")
    return _HistogramCallback(int(every), what, sink, directory)
