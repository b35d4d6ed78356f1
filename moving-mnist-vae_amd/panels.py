"""Picture panels: the reference's plot branch (main.py:205-359, :401-424) and the legacy utils.test pieces (utils.py:77-83, :219-264).

``make_plot_callback`` returns what ``main.train`` calls through ``args.plot_callback``: it renders the reference's picture panels
(``plot_vae`` / ``plot_pixelcnn`` / ``plot_pixelvae``) as 8-bit greyscale contact sheets on the device (``render_sheet``, one kernel
launch per sheet) and writes them as PNG files (``write_png_gray``, standard library only).  The reference's scatter plot of q(z|x)
against p(z) (``scatter_plot``, main.py:166-183) is a density panel (``scatter_panel``; opt-in from the plot functions with
``scatter=True``).  matplotlib figures and wandb stay with the caller: the callback keeps what they need in ``.last``.
"""
import contextlib
import os

import numpy as np
import torch

from . import _lib as L
from .neighbours import _nearest_args, _nearest_launch

_COLUMN_KEYS = ("kind", "tensor", "lut", "uniforms", "lo", "hi")
_COLUMN_KINDS = ("labels", "argmax", "sample", "image")


def column(kind, tensor, lut=None, uniforms=None, lo=None, hi=None):
    """One column spec of ``render_sheet``.  ``kind``: 'labels' (uint8 or int64 class labels, ``lut`` required), 'argmax' / 'sample' (f32
    logits (n, Q, S, S); ``lut`` defaults to ``gray_lut(Q)``; 'sample' needs ``uniforms`` (n, S*S)), 'image' (f32, needs ``lo`` < ``hi``)."""
    return {"kind": kind, "tensor": tensor, "lut": lut, "uniforms": uniforms, "lo": lo, "hi": hi}


def _centres_array(centres, dtype=None):
    """k-means centres, given as a tensor (any device), an array or a sequence, as a host array."""
    return np.asarray(centres.detach().cpu() if isinstance(centres, torch.Tensor) else centres, dtype=dtype)


def gray_lut(Q, centres=None):
    """The grey byte of each of ``Q`` classes, a uint8 (Q,) tensor.  With ``centres`` (the k-means centres of pixel / 255, one per class):
    ``floor(255 * centre + 0.5)`` clamped to [0, 255] -- the dequantised pixel.  Without: the classes spread evenly over [0, 255],
    ``(510 k + (Q - 1)) // (2 (Q - 1))`` in integer arithmetic (round-half-up of 255 k / (Q - 1)); Q = 1 gives 0."""
    Q = int(Q)
    if Q < 1:
        raise ValueError("gray_lut: Q must be positive")
    if centres is not None:
        c = _centres_array(centres, np.float64).reshape(-1)
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


# One column of render_sheet, checked on its own: (descriptors, side).  A descriptor is (MMVAE_PANEL_* code, source, Q, uniforms, lut,
# lo, hi) and holds the very tensors whose addresses go to the kernel, so keeping the descriptors keeps those alive.
def _image_column(spec, t, what):
    lo, hi = spec.get("lo"), spec.get("hi")
    if lo is None or hi is None or not float(hi) > float(lo):
        raise ValueError(f"{what}: needs lo < hi, got lo={lo}, hi={hi}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: expected float32, got {t.dtype}")
    planes = [t[:, c] for c in range(t.shape[1])] if t.dim() == 4 else [t]           # (rows, C, S, S): one column per channel
    sides = [_plane_side(p, 1, what) for p in planes]
    return [(L.PANEL_IMAGE_F32, p.contiguous(), 0, None, None, float(lo), float(hi)) for p in planes], (sides[0] if sides else None)


def _class_column(spec, t, what, rows):
    kind, lut = spec["kind"], spec.get("lut")
    if kind == "labels":
        if t.dtype not in (torch.uint8, torch.int64):
            raise ValueError(f"{what}: expected uint8 or int64 labels, got {t.dtype}")
        if lut is None:
            raise ValueError(f"{what}: labels need a lut (gray_lut(Q))")
        if t.dim() == 4:
            if t.shape[1] != 1:
                raise ValueError(f"{what}: labels have one channel, got shape {tuple(t.shape)}")
            t = t[:, 0]
        S = _plane_side(t, 1, what)
        code, Q = (L.PANEL_LABELS_U8 if t.dtype == torch.uint8 else L.PANEL_LABELS_I64), None
    else:
        if t.dtype != torch.float32 or t.dim() not in (3, 4):
            raise ValueError(f"{what}: expected float32 logits (rows, Q, S, S), got {t.dtype} {tuple(t.shape)}")
        S = _plane_side(t, 2, what)
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
        if not isinstance(u, torch.Tensor) or u.device != t.device or u.numel() != rows * S * S:
            raise ValueError(f"{what}: needs uniforms (rows, S*S) on {t.device}")
        u = u.detach().contiguous().float()
    return [(code, t.contiguous(), Q, u, lut.to(t.device).contiguous(), 0.0, 1.0)], S


def render_sheet(columns, rows):
    """8-bit greyscale contact sheet on the device, ONE launch (mmvae_panel_sheet): uint8 (rows * S, ncols * S); column c fills
    ``[:, c*S:(c+1)*S]`` with its ``rows`` planes stacked vertically -- the reference's ``x[:6].view(-1, S)`` strips side by side.
    ``columns``: specs as ``column(...)`` builds them (dicts, or tuples in that argument order).  Every source must be a device tensor
    holding exactly ``rows`` planes of one side S <= 64, all on one device: labels (rows, S, S) / (rows, 1, S, S) / (rows, S*S), logits
    (rows, Q, S, S) / (rows, Q, S*S) with Q <= 16, images (rows, S, S) / (rows, S*S), or (rows, C, S, S) which becomes one column per
    channel (the reference's ``view(-1, S)`` runs the channels down the strip; here the sheet stays rectangular).  At most 8 columns.
    Everything is checked before anything is launched; a violation raises ValueError."""
    import ctypes
    rows = int(rows)
    if rows < 1:
        raise ValueError("render_sheet: rows must be positive")
    if not columns:
        raise ValueError("render_sheet: no columns")
    descs, S, device = [], None, None
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
        cols, s = _image_column(spec, t.detach(), what) if kind == "image" else _class_column(spec, t.detach(), what, rows)
        if S is None:
            S = s
        if s is not None and s != S:
            raise ValueError(f"render_sheet: planes of side {s} next to planes of side {S}")
        descs += cols
    if not 1 <= S <= L.PANEL_MAX_S:
        raise ValueError(f"render_sheet: side {S} unsupported (1..{L.PANEL_MAX_S})")
    if len(descs) > L.PANEL_MAX_COLS:
        raise ValueError(f"render_sheet: {len(descs)} columns, at most {L.PANEL_MAX_COLS} fit one sheet")
    arr = (L.PanelCol * len(descs))(*[L.PanelCol(code, L.ptr(t), Q, L.ptr(u), L.ptr(lut), lo, hi) for code, t, Q, u, lut, lo, hi in descs])
    out = torch.empty((rows * S, len(descs) * S), dtype=torch.uint8, device=device)
    L.call("mmvae_panel_sheet", device, ctypes.addressof(arr), len(descs), rows, S, L.ptr(out))
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


def _save_sheets(sheets, directory, epoch, plot_count):
    """Every sheet as ``<directory>/<name>-<epoch>-<plot_count>.png``."""
    os.makedirs(directory, exist_ok=True)
    for name, sheet in sheets.items():
        write_png_gray(os.path.join(directory, "{}-{}-{}.png".format(name, epoch, plot_count)), sheet)


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
    L.call("mmvae_scatter_panel", pts.device, L.ptr(pts) if pts.shape[0] else None, pts.shape[0], pts.shape[1], dims[0], dims[1], L.ptr(xform),
           side, radius16, L.ptr(tone), L.ptr(out), out.stride(0))
    return out


def _scatter_args(points, dims, side, radius, tone, out, what):
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
        _save_sheets({"scatter": sheet}, directory, epoch, plot_count)
    return (sheet, {"prior": prior, "xform": xform}) if return_tensors else sheet


def _add_scatter(sheets, tensors, encoding, generator):
    """``scatter=True`` of the plot functions: the last sheet, from the last draw taken from ``generator``."""
    sheets["scatter"], t = scatter_plot(encoding.detach().float(), None, 0, 0, generator=generator, save=False, return_tensors=True)
    tensors["scatter_prior"], tensors["scatter_xform"] = t["prior"], t["xform"]


def neighbour_sheet(queries, frames, k=5, lut=None, display_lut=None):
    """Each query next to its ``k`` nearest training frames: one ``nearest_frames`` call, one gather of the M * k neighbour planes
    (with ``lut`` applied, so the sheet shows the values that were compared) and one ``render_sheet`` launch.  Returns
    ``(sheet, dist, index)``: the uint8 (M * S, (k + 1) * S) device sheet -- column 0 the queries, columns 1..k the neighbours, nearest
    first -- and what ``nearest_frames`` returned.  ``display_lut``: a uint8 table of at most 16 greys for compared values that are class
    labels (``gray_lut(Q, centres)``); every column then goes through the 'labels' kind.  Without it the compared bytes are shown as
    greys ('image' columns with lo = 0, hi = 255: the byte itself).  Square planes of side <= 64, ``k <= 7`` (a sheet has 8 columns);
    otherwise as ``nearest_frames``.  Everything is checked before anything is launched; a violation raises ValueError."""
    if not 1 <= int(k) <= L.PANEL_MAX_COLS - 1:
        raise ValueError(f"neighbour_sheet: k={int(k)} unsupported (1..{L.PANEL_MAX_COLS - 1}: a sheet has {L.PANEL_MAX_COLS} columns)")
    if display_lut is not None:
        display_lut = torch.as_tensor(display_lut)
        if display_lut.dtype != torch.uint8 or not 1 <= display_lut.numel() <= L.PANEL_MAX_Q:
            raise ValueError(f"neighbour_sheet: display_lut is 1..{L.PANEL_MAX_Q} uint8 greys")
    q, f, k, lut, (H, W) = _nearest_args(queries, frames, k, lut, "neighbour_sheet")
    if H != W or H > L.PANEL_MAX_S:
        raise ValueError(f"neighbour_sheet: planes of {H} x {W}, a sheet shows square planes of side 1..{L.PANEL_MAX_S}")
    dist, index = _nearest_launch(q, f, k, lut)
    planes = f.index_select(0, index.reshape(-1))
    if lut is not None:
        planes = lut[planes.long()]
    planes = planes.view(q.shape[0], k, -1)
    sources = [q] + [planes[:, j] for j in range(k)]
    if display_lut is not None:
        cols = [column("labels", t, display_lut) for t in sources]
    else:
        cols = [column("image", t.float(), lo=0.0, hi=255.0) for t in sources]
    return render_sheet(cols, q.shape[0]), dist, index


def plot_neighbours(queries, frames, directory, epoch, plot_count, **kw):
    """``neighbour_sheet(queries, frames, **kw)`` written as ``<directory>/neighbours-<epoch>-<plot_count>.png``; returns
    ``(sheet, dist, index)``."""
    sheet, dist, index = neighbour_sheet(queries, frames, **kw)
    _save_sheets({"neighbours": sheet}, directory, epoch, plot_count)
    return sheet, dist, index


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


@contextlib.contextmanager
def _plot_mode(model):
    """eval mode + no_grad for the length of a plot; the model's previous mode comes back (the reference leaves it in eval mode, which
    only works because its loop calls model.train() at the top of every step)."""
    was_training = bool(model.training)
    model.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        model.train(was_training)


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
    n_c = None if centres is None else int(_centres_array(centres).size)
    levels = Q or n_c or 2
    lut = None if Q is None else gray_lut(Q, centres if n_c == Q else None)
    if lo is None:
        lo = (0.0 - float(data_mean)) / float(data_std)
    if hi is None:
        hi = (max(levels - 1, 1) - float(data_mean)) / float(data_std)
    return float(lo), float(hi), lut


def _decoder_column(model, t, lut, lo, hi):
    """What the decoder emitted, as a column: the per-pixel argmax for a categorical decoder, the f32 values otherwise."""
    if model.decoder_out_channels > model.in_channels:
        return column("argmax", t, lut)
    return column("image", t.float(), lo=lo, hi=hi)


def _free_running(model, sample, z_image, data_mean, data_std, generator, uniforms=None):
    """The free-running sampler (``model.sample_pixels``) from ``sample``, conditioned on ``z_image`` (None: a PixelCNN on its own);
    ``uniforms`` None draws them (N, S*S) through ``generator``.  Returns (last logits, filled sample, drawn labels, uniforms)."""
    if uniforms is None:
        uniforms = _draw(torch.rand, (sample.shape[0], model.input_image_size ** 2), sample.device, generator)
    logits, sample, _, labels = model.sample_pixels(sample, z_image, data_mean=data_mean, data_std=data_std, uniforms=uniforms,
                                                    return_probs=True)
    return logits, sample, labels, uniforms


def _fit_planes(t, S):
    """The leading S x S of every plane.  The decoder's crop (model.py:307-310, :328-329) takes (32 - S) // 2 off both ends, which leaves
    an odd S one row and one column too many; next to an S x S input a sheet can only show S of them."""
    return t[..., :S, :S] if t.shape[-1] > S or t.shape[-2] > S else t


def _finish_plot(sheets, tensors, directory, epoch, plot_count, save, return_tensors):
    if save:
        _save_sheets(sheets, directory, epoch, plot_count)
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
        sheets = {"recon": render_sheet([column("image", img, lo=lo, hi=hi), _decoder_column(model, rec, lut, lo, hi)], n),
                  "normal_sampling": render_sheet([_decoder_column(model, output_random_encoding, lut, lo, hi)], n)}
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
        n = img.shape[0]
        start = torch.zeros(tuple(img.shape), device=img.device) - data_mean / data_std
        sample_logits, sample, sample_labels, uniforms = _free_running(model, start, None, data_mean, data_std, generator)
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
        n = img.shape[0]

        def free_running(z_img):
            return _free_running(model, torch.zeros(tuple(img.shape), device=img.device), z_img, data_mean, data_std, generator)

        z_image = model.get_z_image(enc).contiguous()
        free_logits, _, free_labels, uniforms = free_running(z_image)
        random_encoding = _draw(torch.randn, tuple(enc.shape), device, generator)
        random_z_image = model.get_z_image(random_encoding).contiguous()
        random_free_logits, _, random_free_labels, random_uniforms = free_running(random_z_image)
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
        S = model.input_image_size
        z_images = _fit_planes(model.get_z_image(encodings), S).contiguous()
        if model.pixelcnn is None:
            return render_sheet([_decoder_column(model, z_images, lut, lo, hi)], steps)
        start = torch.zeros((steps, model.in_channels, S, S), device=z_images.device)
        logits, _, labels, _ = _free_running(model, start, z_images, data_mean, data_std, generator, uniforms)
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
