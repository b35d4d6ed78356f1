"""Exact nearest neighbours in pixel space: ``nearest_frames`` (mmvae_nearest_frames, up to 64 queries against every resident frame) and
``cross_neighbours`` / ``ball_counts`` (mmvae_knn_cross, set against set).  Both measure the sum of squared byte differences in exact
integers and give equal distances to the lower index (csrc/knn_select.hpp defines the key).  The argument checks, the dense and aligned
rows and the launch are written once here; ``panels.neighbour_sheet`` and ``samples.sample_quality`` use them too."""
import torch

from . import _lib as L
from .data import MovingMNISTClips


def _rows_u8(t, name, what, n="N", planes=False):
    """One operand, checked on its own: the uint8 tensor as (N, D) rows (not yet made dense) and the shape of one row as it came.
    With ``planes``, and for a ``MovingMNISTClips`` (its ``.clips``), [..., H, W] with every leading axis flattened."""
    if isinstance(t, MovingMNISTClips):
        t, planes = t.clips, True
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise ValueError(f"{what}: {name} must be a uint8 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if planes:
        if t.dim() < 2:
            raise ValueError(f"{what}: {name} must have shape [..., H, W], got {tuple(t.shape)}")
        H, W = int(t.shape[-2]), int(t.shape[-1])
        return t.detach().reshape(t.numel() // (H * W) if H * W else 0, H * W), (H, W)
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() not in (2, 3):
        raise ValueError(f"{what}: {name} must have shape [{n}, H, W], [{n}, 1, H, W] or [{n}, H*W], got {tuple(t.shape)}")
    return t.detach().reshape(t.shape[0], t.shape[1] if t.dim() == 2 else t.shape[1] * t.shape[2]), tuple(t.shape[1:])


def _check_limits(what, k, kmin, counts, D, row):
    """The limits of both entry points (k and D are the same for both): k, each (n, its words, most) of ``counts``, D bytes per ``row``."""
    if not kmin <= k <= L.NEAREST_MAX_K:
        raise ValueError(f"{what}: k={k} unsupported (1..{L.NEAREST_MAX_K})")
    for n, words, most in counts:
        if not 1 <= n <= most:
            raise ValueError(f"{what}: {words} unsupported (1..{most})")
    if D % 16 or not 16 <= D <= L.NEAREST_MAX_D:
        raise ValueError(f"{what}: D={D} bytes per {row} unsupported (a multiple of 16 in 16..{L.NEAREST_MAX_D})")


def _lut256(lut, what):
    lut = torch.as_tensor(lut)
    if lut.dtype != torch.uint8 or lut.numel() != 256:
        raise ValueError(f"{what}: lut is 256 uint8 values")
    return lut.detach().reshape(-1)


def _dense16(*rows):
    """Checked rows as the kernels read them: dense and 16-byte aligned (a copy only where they are not)."""
    return tuple(t if t.data_ptr() % 16 == 0 else t.clone() for t in (t.contiguous() for t in rows))


def _launch(entry, x, y, k, head, radius=None):
    """``mmvae_<entry>`` on checked arguments, with scratch of the size the library names and fresh outputs: (dist, index), both None at
    k = 0, and the ball counts where ``radius`` is given.  ``head``: what the entry point takes between D and out_dist."""
    (Nx, D), Ny, dev, cross = x.shape, y.shape[0], x.device, entry == "knn_cross"
    nbytes = getattr(L.lib(), f"mmvae_{entry}_scratch_bytes")(Nx, Ny, D, k, *((int(radius is not None),) if cross else ()))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dist = torch.empty((Nx, k), dtype=torch.int32, device=dev) if k else None
    index = torch.empty((Nx, k), dtype=torch.int64, device=dev) if k else None
    count = torch.empty((Nx,), dtype=torch.int32, device=dev) if radius is not None else None
    L.call(f"mmvae_{entry}", dev, L.ptr(x), Nx, L.ptr(y), Ny, D, *head, L.ptr(dist), L.ptr(index),
           *((L.ptr(radius), L.ptr(count)) if cross else ()), L.ptr(scratch), nbytes)
    return dist, index, count


def _nearest_args(queries, frames, k, lut, what):
    """Every check of ``nearest_frames`` (nothing is launched here): returns (queries (M, D), frames (F, D), k, device lut or None,
    (H, W)), the rows dense and 16-byte aligned."""
    q, plane = _rows_u8(queries, "queries", what, n="M")
    f, (H, W) = _rows_u8(frames, "frames", what, planes=True)
    (M, Dq), (F, D) = q.shape, f.shape
    if (plane != (H, W)) if len(plane) == 2 else (Dq != D):
        raise ValueError(f"{what}: query planes {plane} do not match the frames' {H} x {W}")
    k = int(k)
    _check_limits(what, k, 1, ((M, f"M={M} queries", L.NEAREST_MAX_M),), D, "plane")
    if not k <= F <= 2 ** 31 - 1:
        raise ValueError(f"{what}: F={F} frames for k={k} (k..2^31 - 1)")
    if lut is not None:
        lut = _lut256(lut, what)
    if not f.is_cuda or not q.is_cuda:
        raise ValueError(f"{what} expects queries and frames on the GPU")
    if q.device != f.device:
        raise ValueError(f"{what}: queries on {q.device}, frames on {f.device}")
    q, f = _dense16(q, f)
    if lut is not None:
        lut = lut.to(f.device).contiguous()
    return q, f, k, lut, (H, W)


def _nearest_launch(q, f, k, lut):
    return _launch("nearest_frames", q, f, k, (L.ptr(lut), k))[:2]


def nearest_frames(queries, frames, k=5, lut=None):
    """The ``k`` nearest training frames of every query, exactly, in one pass over the resident uint8 data (mmvae_nearest_frames): did
    the model learn to draw, or did it memorise?  ``frames``: a uint8 device tensor [..., H, W] whose leading axes are flattened to F
    frames, or a ``MovingMNISTClips`` (its ``.clips``).  ``queries``: uint8 on the same device, [M, H, W], [M, 1, H, W] or [M, H*W].
    The distance is the sum of squared byte differences, ``sum (q - t(x))^2`` in exact integers, with ``t = lut[.]`` applied to the
    FRAMES only (``lut``: None or 256 uint8 values on any device -- ``fit.lut`` of a ``QuantiserFit`` compares class labels,
    ``gray_lut(Q, centres)[fit.lut]`` dequantised greys; the queries are already in that space).  Returns ``(dist, index)``: int32 and
    int64 (M, k) device tensors, nearest first, equal distances to the lower index; ``index`` addresses ``frames.reshape(-1, H*W)``
    (for clips ``divmod(index, 20)`` is (clip, frame)).  M <= 64, k <= 8, H*W a multiple of 16 up to 16384, k <= F.  Everything is
    checked before anything is launched (ValueError); no host read inside the call; the same bits every run."""
    q, f, k, lut, _ = _nearest_args(queries, frames, k, lut, "nearest_frames")
    return _nearest_launch(q, f, k, lut)


def _cross_args(a, b, k, exclude_self, radius, what):
    """Every check of a sweep (nothing is launched here): returns (a (Na, D), b (Nb, D), radius), the rows dense and 16-byte aligned."""
    a, b = _rows_u8(a, "a", what)[0], _rows_u8(b, "b", what)[0]
    (Na, D), (Nb, Db) = a.shape, b.shape
    if D != Db:
        raise ValueError(f"{what}: rows of {D} bytes in a do not match rows of {Db} bytes in b")
    _check_limits(what, k, 0, ((Na, f"Na={Na} rows", L.KNN_CROSS_MAX_N), (Nb, f"Nb={Nb} rows", L.KNN_CROSS_MAX_N)), D, "row")
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
    return _dense16(a, b) + (radius,)


def _cross_launch(a, b, k, exclude_self, radius):
    """mmvae_knn_cross on checked arguments: (dist, index) or (None, None), and the counts or None."""
    return _launch("knn_cross", a, b, k, (k, int(bool(exclude_self))), radius)


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
    return _cross_launch(a, b, k, exclude_self, None)[:2]


def ball_counts(a, b, radius, exclude_self=False):
    """For every row i of ``a``, in how many balls of ``b`` it lies: ``#{ j : d(i, j) <= radius[j] }`` as an int32 (Na,) device tensor
    (mmvae_knn_cross without a selection).  ``radius``: int32 or int64 device tensor (Nb,) of SQUARED distances, each >= 0 (checked:
    one device -> host read); the comparison is inclusive and exact.  ``a``, ``b``, ``exclude_self`` and the limits as in
    ``cross_neighbours``."""
    a, b, radius = _cross_args(a, b, 0, exclude_self, radius, "ball_counts")
    # no distance exceeds D * 255^2 < 2^31: larger radii are clamped to the int32 maximum without changing any comparison
    return _cross_launch(a, b, 0, exclude_self, radius.detach().clamp(max=2 ** 31 - 1).to(torch.int32).contiguous())[2]
