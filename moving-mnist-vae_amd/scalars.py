"""What a step hands to the host: the four logged scalars as float-like views of one device tensor, and class labels of logits."""
import torch

from ._lib import call, ptr


def draw_labels(probs, u):
    """The sampler's draw rule, the one definition of it: ``label = #{k in [0, Q-2] : cdf_k <= u}`` with ``cdf`` the cumulative sums of
    ``probs`` (..., Q) along the last axis in channel order and ``u`` (...) uniform in [0, 1) -- inverse-CDF sampling of the categorical
    distribution ``probs``.  Pure torch, any device; returns int64 labels of ``u``'s shape."""
    cdf = torch.cumsum(probs, dim=-1)[..., :-1]
    return (cdf <= u.unsqueeze(-1)).sum(dim=-1)


@torch.no_grad()
def decode_labels(logits, mode="argmax", uniforms=None, generator=None):
    """Class labels of a logits tensor (N, Q, H, W) -- what ``forward``, ``get_reconstruction`` and ``run_pixelcnn`` return for a
    categorical model -- as int64 (N, H, W), one kernel (mmvae_logits_to_labels), 1 <= Q <= 16.  ``mode="argmax"``: the lowest index
    among equal maxima (``logits.argmax(dim=1)`` away from ties; a NaN never wins).  ``mode="sample"``: one draw per pixel from the
    f32 softmax by ``draw_labels``'s rule with ``u = uniforms[n, h * W + w]``; ``uniforms=None`` draws them with
    ``torch.rand((N, H * W), generator=generator)`` (the reference's utils.sample_from_recostruction, utils.py:77-83, with another
    random stream than torch.multinomial)."""
    if mode not in ("argmax", "sample"):
        raise ValueError("mode is 'argmax' or 'sample'")
    if not isinstance(logits, torch.Tensor) or logits.dim() != 4 or not logits.is_cuda:
        raise ValueError("decode_labels expects logits of shape (N, Q, H, W) on the GPU")
    x = logits.detach().contiguous().float()
    N, Q, H, W = x.shape
    u = None
    if mode == "sample":
        if uniforms is None:
            uniforms = torch.rand((N, H * W), device=x.device, generator=generator)
        u = uniforms.to(x.device).contiguous().float()
        if u.numel() != N * H * W:
            raise ValueError(f"uniforms must hold N * H * W = {N * H * W} values, got {tuple(uniforms.shape)}")
    labels = torch.empty((N, H, W), dtype=torch.int64, device=x.device)
    if labels.numel() == 0:
        return labels
    call("mmvae_logits_to_labels", x.device, ptr(x), N, Q, H * W, 1 if mode == "sample" else 0, ptr(u), ptr(labels))
    return labels


class _StepScalars:
    """The four scalars of one step (loss, nll/N, kl/N, mmd/N) as a device tensor, copied to the host on first use.  `join` (optional):
    orders the stream that produced them (the net's side stream, _LossFn) before the current one -- called before any read."""
    __slots__ = ("dev", "vals", "join")

    def __init__(self, dev_tensor, join=None):
        self.dev, self.vals, self.join = dev_tensor, None, join

    def ready(self):
        """The device tensor, ordered before the current stream."""
        if self.join is not None:
            self.join()
            self.join = None
        return self.dev

    def get(self, i):
        if self.vals is None:
            self.vals = self.ready().tolist()    # the only device->host copy (and synchronisation) of the step
        return self.vals[i]


class DeferredScalar:
    """Float-like view of one step scalar.  ``VAE.loss`` returns these instead of Python floats so that the host does
    not have to wait for the forward pass before it enqueues the backward pass (the reference synchronises three
    times per step with ``.item()``); any arithmetic, comparison, formatting or ``float()`` reads the value."""
    __slots__ = ("_g", "_i")

    def __init__(self, group, index):
        self._g, self._i = group, index

    def __float__(self):
        return self._g.get(self._i)

    item = __float__

    def __repr__(self):
        return repr(float(self))

    def __format__(self, spec):
        return format(float(self), spec)

    def __bool__(self):
        return bool(float(self))

    def __hash__(self):
        return hash(float(self))

    def __array__(self, dtype=None, copy=None):
        import numpy as _np
        return _np.asarray(float(self), dtype=dtype)


def _forward_float(name):
    def op(self, *other):
        f = getattr(float, name)
        return f(float(self), *[float(o) if isinstance(o, DeferredScalar) else o for o in other])
    op.__name__ = name
    return op


for _n in ("__add__", "__radd__", "__sub__", "__rsub__", "__mul__", "__rmul__", "__truediv__", "__rtruediv__", "__pow__", "__rpow__",
           "__neg__", "__pos__", "__abs__", "__lt__", "__le__", "__gt__", "__ge__", "__eq__", "__ne__", "__round__", "__int__",
           "__floordiv__", "__rfloordiv__", "__mod__", "__rmod__"):
    setattr(DeferredScalar, _n, _forward_float(_n))
