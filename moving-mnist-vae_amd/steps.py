"""The autograd shell of one train step: five ``autograd.Function``s over the C ABI, and the hand-off object (``_StepState``)
through which one phase of a step leaves a value for a later phase."""
from typing import NamedTuple

import torch

from ._lib import SUM_PARTIALS, check, cur_stream, lib, ptr

# ------------------------------------------------------------------------------------------ the step's hand-off
# prepare_batch -> _EncoderFn.forward: the image (a weakref, its _version then) whose storage-type copy sits in the workspace at ws_ptr
_Staged = NamedTuple("_Staged", [("image_ref", object), ("version", int), ("ws_ptr", int), ("N", int)])
# _DecoderFn.forward -> _LossFn.forward: the last train-mode reconstruction and that forward's stamp
_Recon = NamedTuple("_Recon", [("data_ptr", int), ("stamp", int)])
# _LossFn.backward -> _DecoderFn.backward: the Gaussian loss gradient coef / sigma^2 * gscale * (recon - target), to be evaluated inside the
# output BatchNorm's backward of the decoder forward `stamp`; `token` travels through autograd in place of d_recon
_Tail = NamedTuple("_Tail", [("token", torch.Tensor), ("target", torch.Tensor), ("sigma", float), ("coef", float), ("gscale", torch.Tensor),
                             ("stamp", int)])


class _PendingLoss:
    """The loss-scalar launch of one VAE.loss call: created there, filled in by _LossFn.forward (the closure and the tensor it writes),
    launched once -- by _LossFn.forward itself in the in-stream form; with `side`, by the decoder's backward on the net's side stream, or
    else by the first read of the scalars or the next loss on the caller's.  The model keeps its last one, and with it the operands,
    until the next loss.  The closure holds DETACHED tensors only and never the model: a tensor with a grad_fn would keep the step's
    autograd graph, whose nodes hold the model, in a reference cycle with it (45 GB workspaces waiting for the cycle collector)."""
    __slots__ = ("side", "closure", "out", "launched")

    def __init__(self, side):
        self.side, self.closure, self.out, self.launched = side, None, None, False

    def launch_on(self, st):
        if not self.launched:
            self.launched = True
            self.closure(st)


class _StepState:
    """Every value that one phase of a step leaves on the model for a later phase ("The step's hand-off object")."""
    __slots__ = ("staged", "recon", "tail", "nan_token", "loss")

    def __init__(self):
        self.loss = None                           # _PendingLoss of the last loss
        self.reset()

    def reset(self):
        """Forget what refers to device storage the model has just replaced (_reflatten).  The last loss stays: its closure owns its
        operands, and scalars not yet launched are still owed to their reader."""
        self.staged = self.recon = self.tail = None        # _Staged, _Recon, _Tail
        self.nan_token = None                              # cached (1,) NaN tensor behind _Tail.token

    @property
    def loss_pending(self):
        return self.loss is not None and not self.loss.launched

    def flush_loss(self, st, only=None):
        """Launch the last loss's scalar kernels on stream `st` unless they are already launched (`only`: if they write this tensor)."""
        if self.loss is not None and (only is None or self.loss.out is only):
            self.loss.launch_on(st)

    def take_staged(self, x, ws, N):
        """True if prepare_batch staged this very tensor (same object, untouched since) into this workspace; consumes the entry."""
        s, self.staged = self.staged, None
        return s is not None and s.image_ref() is x and s.version == x._version and s.ws_ptr == ws.data_ptr() and s.N == N

    def tail_token(self, like):
        """A 0-strided NaN of `like`'s shape: any consumer other than _DecoderFn.backward fails loudly instead of silently."""
        if self.nan_token is None or self.nan_token.device != like.device:
            self.nan_token = torch.full((1,), float("nan"), device=like.device, dtype=torch.float32)
        return self.nan_token.expand(like.shape)


# ------------------------------------------------------------------------------------------ autograd glue
class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, *params):
        N = x.shape[0]
        z = model.z_dimensions
        mu = torch.empty((N, z, 1, 1), device=x.device, dtype=torch.float32)
        logvar = torch.empty_like(mu) if model.require_rsample else None
        training = bool(model.training)
        ws = model._workspace(N, training)
        # staged input: no conversion pass over x
        fn = lib().mmvae_encoder_fwd_staged if model._step.take_staged(x, ws, N) else lib().mmvae_encoder_fwd
        check(fn(model._h, N, ptr(x), model._net_ptr(model._flat), ptr(model._bnf), ptr(model._bni), ptr(ws), ws.numel(),
                 ptr(mu), ptr(logvar), int(training), cur_stream()), "mmvae_encoder_fwd")
        ctx.model, ctx.N, ctx.training = model, N, training
        ctx.token = model._stamp("enc", training)
        return mu if logvar is None else (mu, logvar)

    @staticmethod
    def backward(ctx, d_mu, d_logvar=None):
        model = ctx.model
        model._check_stamp("enc", ctx.token, ctx.training)
        z, N = model.z_dimensions, ctx.N
        dev = model._flat.device
        d_mu = torch.zeros((N, z), device=dev) if d_mu is None else d_mu.contiguous().float()
        if model.require_rsample:
            d_logvar = torch.zeros((N, z), device=dev) if d_logvar is None else d_logvar.contiguous().float()
        G = model._grad_target()
        G[model._poff:model._dec_off].zero_()
        ws = model._workspace(N, True)
        check(lib().mmvae_encoder_bwd(model._h, N, ptr(d_mu), ptr(d_logvar), model._net_ptr(model._flat), model._net_ptr(G), ptr(ws), ws.numel(),
                                      cur_stream()), "mmvae_encoder_bwd")
        if model._sync is not None:
            model._sync.bucket_ready(G, 0, model._dec_off)      # (a PixelCNN's gradients sit in front and are complete by now: it ran first)
        return (None, None) + model._grad_views(G, model._enc_rows)


class _DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, encoding, *params):
        N = encoding.shape[0]
        training = bool(model.training)
        recon = torch.empty((N, model.decoder_out_channels, model._dec_side, model._dec_side), device=encoding.device, dtype=torch.float32)
        ws = model._workspace(N, training)
        check(lib().mmvae_decoder_fwd(model._h, N, ptr(encoding), model._net_ptr(model._flat), ptr(model._bnf), ptr(model._bni), ptr(ws), ws.numel(),
                                      ptr(recon), int(training), cur_stream()), "mmvae_decoder_fwd")
        ctx.model, ctx.N, ctx.training = model, N, training
        ctx.token = model._stamp("dec", training)
        ctx.need_denc = bool(ctx.needs_input_grad[1])
        model._step.recon = _Recon(recon.data_ptr(), ctx.token) if training else None
        return recon

    @staticmethod
    def backward(ctx, d_recon):
        model = ctx.model
        model._check_stamp("dec", ctx.token, ctx.training)
        N = ctx.N
        step = model._step
        # Gaussian loss tail (see _LossFn.backward): the incoming "gradient" is the loss function's token -- the real one is evaluated
        # inside the output BatchNorm's backward from the saved conv output and the target, and never stored
        tail, step.tail = step.tail, None
        fused_tail = (tail is not None and tail.stamp == ctx.token and d_recon.stride(0) == 0 and d_recon.data_ptr() == tail.token.data_ptr())
        if not fused_tail:
            d_recon = d_recon.contiguous().float()
        d_enc = torch.empty((N, model.z_dimensions, 1, 1), device=d_recon.device, dtype=torch.float32) if ctx.need_denc else None
        G = model._grad_target()
        G[model._dec_off:].zero_()
        ws = model._workspace(N, True)
        h, st = model._h, cur_stream()

        def join_at_end_of_backward():
            torch.autograd.Variable._execution_engine.queue_callback(lambda: check(lib().mmvae_net_join(h, st), "mmvae_net_join"))
        # The decoder's weight gradients stay in flight on the net's side stream while the encoder backward is enqueued;
        # mmvae_encoder_bwd orders them before this stream again, and so does the end-of-backward callback below when the graph
        # holds no encoder (a decoder driven from a leaf encoding).  With a GradSync attached the decoder bucket is all-reduced
        # from a communication stream that waits for this stream AND the side stream (GradSync.bucket_ready), so the caller's
        # stream is not held up there either.
        defer = model.defer_join
        check(lib().mmvae_net_defer_join(h, int(defer)), "mmvae_net_defer_join")
        if fused_tail:
            check(lib().mmvae_decoder_bwd_gauss(h, N, ptr(tail.target), tail.sigma, tail.coef, ptr(tail.gscale), model._net_ptr(model._flat),
                                                model._net_ptr(G), ptr(ws), ws.numel(), ptr(d_enc), st), "mmvae_decoder_bwd_gauss")
        else:
            check(lib().mmvae_decoder_bwd(h, N, ptr(d_recon), model._net_ptr(model._flat), model._net_ptr(G), ptr(ws), ws.numel(), ptr(d_enc), st),
                  "mmvae_decoder_bwd")
        if defer:
            join_at_end_of_backward()
        if model._sync is not None:
            model._sync.bucket_ready(G, model._dec_off, model._n_params, side_of=model if defer else None)
        if step.loss_pending:
            # the step's loss scalars (_LossFn.forward): behind the decoder's weight gradients on the side stream -- every fork of this pass
            # ordered that stream behind the forward pass already, so no new wait is needed, and the stream idles here until the encoder's
            # weight gradients arrive
            side = lib().mmvae_net_side_stream(h)
            step.loss.launch_on(side if side else st)
            if side and not defer:
                join_at_end_of_backward()
        return (None, d_enc) + model._grad_views(G, model._dec_rows)


class _PixelFn(torch.autograd.Function):
    """PixelCNN.forward (model.py:248-255) through mmvae_pixelcnn_fwd / _bwd."""

    @staticmethod
    def forward(ctx, model, x, *params):
        N, S = x.shape[0], x.shape[2]
        x = x.contiguous().float()
        with torch.no_grad():
            model._flat[:model._poff].mul_(model._pix_mask)          # model.py:222: weight.data *= mask in every forward
        out = torch.empty((N, model.pixelcnn_out_channels, S, S), device=x.device, dtype=torch.float32)
        ws = model._pixel_workspace(N, S)
        check(lib().mmvae_pixelcnn_fwd(model._hp, N, S, ptr(x), ptr(model._flat), ptr(ws), ws.numel(), ptr(out), cur_stream()), "mmvae_pixelcnn_fwd")
        ctx.model, ctx.N, ctx.S = model, N, S
        ctx.token = model._stamp("pix", True)
        ctx.need_dx = bool(ctx.needs_input_grad[1])
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, d_out):
        model, N, S = ctx.model, ctx.N, ctx.S
        model._check_stamp("pix", ctx.token, True, "the saved activations of this PixelCNN forward were overwritten by a later forward")
        (x,) = ctx.saved_tensors
        d_out = d_out.contiguous().float()
        G = model._grad_target()
        G[:model._poff].zero_()
        d_x = torch.empty_like(x) if ctx.need_dx else None
        ws = model._pixel_workspace(N, S)
        check(lib().mmvae_pixelcnn_bwd(model._hp, N, S, ptr(x), ptr(d_out), ptr(model._flat), ptr(G), ptr(ws), ws.numel(), ptr(d_x), cur_stream()),
              "mmvae_pixelcnn_bwd")
        return (None, d_x) + model._grad_views(G, model._pix_rows)


class _RsampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, logvar, eps):
        mu, logvar, eps = mu.contiguous(), logvar.contiguous(), eps.contiguous()
        enc = torch.empty_like(mu)
        check(lib().mmvae_rsample_fwd(ptr(mu), ptr(logvar), ptr(eps), ptr(enc), mu.numel(), cur_stream()), "mmvae_rsample_fwd")
        ctx.save_for_backward(logvar, eps)
        return enc

    @staticmethod
    def backward(ctx, d_enc):
        logvar, eps = ctx.saved_tensors
        d_enc = d_enc.contiguous()
        d_mu, d_lv = torch.empty_like(d_enc), torch.empty_like(d_enc)
        check(lib().mmvae_rsample_bwd(ptr(d_enc), ptr(logvar), ptr(eps), ptr(d_mu), ptr(d_lv), d_enc.numel(), cur_stream()), "mmvae_rsample_bwd")
        return d_mu, d_lv, None


class _LossFn(torch.autograd.Function):
    """VAE.loss arithmetic (model.py:385-405): KL + MMD + Gaussian-NLL | weighted CE, all reductions on device."""

    @staticmethod
    def forward(ctx, model, rec, target, mu, logvar, encoding, recon, true_samples, weight):
        L = lib()
        N, dev, step = target.shape[0], recon.device, model._step
        # px, kl, mmd, (pad), then the sums' ordered-reduction scratch (mmvae.h MMVAE_SUM_PARTIALS): the sums run one after another on
        # one stream, and each leaves the scratch's ticket at zero for the next
        acc = torch.zeros(4 + SUM_PARTIALS, dtype=torch.float64, device=dev)
        out = torch.empty(4, dtype=torch.float32, device=dev)      # loss, px/N, kl/N, mmd/N
        # `rec.side` (VAE.loss(deferred=True) inside a train step): the loss scalars are logged values -- no gradient kernel
        # reads them -- so their kernels (KL, MMD, NLL / CE sums, the combine) leave the critical stream: they are enqueued on the net's side
        # stream by the decoder's backward pass, behind its weight gradients, where that stream idles while the caller's runs the latency-bound
        # kernels around the latent code (_DecoderFn.backward); the backward pass's own join (mmvae_encoder_bwd / the end-of-backward
        # mmvae_net_join) orders them before the caller's stream again.  Never launched by then: see _PendingLoss.
        step.flush_loss(cur_stream())
        base, part = acc.data_ptr(), acc.data_ptr() + 32
        recon = recon.contiguous()
        categorical = model.is_categorical()
        if mu is not None and logvar is not None:
            mu, logvar = mu.contiguous(), logvar.contiguous()
        scratch = None
        if encoding is not None:
            encoding = encoding.contiguous()
            scratch = torch.empty(2 * N, dtype=torch.float32, device=dev)
        target = target.contiguous()
        nll_c, kl_c, mmd_c, sigma = float(model.nll), float(model.kl), float(model.mmd), float(model.sigma_decoder)
        # the closure keeps every operand alive until the record is dropped -- as detached views (_PendingLoss)
        det = lambda t: None if t is None else t.detach()
        k_mu, k_lv, k_enc, k_rec, k_tgt, k_ts, k_w = det(mu), det(logvar), det(encoding), det(recon), det(target), det(true_samples), det(weight)

        def launch(st):
            if k_mu is not None and k_lv is not None:
                check(L.mmvae_kl_fwd_ex(ptr(k_mu), ptr(k_lv), k_mu.numel(), base + 8, part, st), "mmvae_kl_fwd_ex")
            if k_enc is not None:
                check(L.mmvae_mmd_fwd_ex(ptr(k_ts), ptr(k_enc), N, k_enc.shape[1], ptr(scratch), base + 16, part, st), "mmvae_mmd_fwd_ex")
            if categorical:
                Q, HW = k_rec.shape[1], k_rec.shape[2] * k_rec.shape[3]
                check(L.mmvae_ce_fwd_ex(ptr(k_rec), ptr(k_tgt), ptr(k_w), N, Q, HW, base, part, st), "mmvae_ce_fwd_ex")
            else:
                check(L.mmvae_gauss_nll_fwd_ex(ptr(k_rec), ptr(k_tgt), k_rec.numel(), sigma, base, part, st), "mmvae_gauss_nll_fwd_ex")
            check(L.mmvae_loss_finish(base, ptr(out), nll_c, kl_c, mmd_c, float(N), st), "mmvae_loss_finish")
            _ = acc                     # (referenced: the accumulator lives as long as the closure)

        rec.closure, rec.out = launch, out
        step.loss = rec
        if not rec.side:
            rec.launch_on(cur_stream())
        ctx.model, ctx.N, ctx.categorical = model, N, categorical
        # the reconstruction is the decoder's own output tensor (no crop, no copy): its gradient can be folded into the decoder's backward
        lr = step.recon
        ctx.direct_tail = (lr.stamp if (lr is not None and lr.data_ptr == recon.data_ptr() and not categorical and model.fuse_loss_tail and
                                        target.dtype == torch.float32 and target.shape == recon.shape) else None)
        ctx.save_for_backward(target, mu, logvar, encoding, recon, true_samples, weight)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        L = lib()
        model, N = ctx.model, ctx.N
        target, mu, logvar, encoding, recon, ts, weight = ctx.saved_tensors
        st = cur_stream()
        g = g.contiguous().float()
        sigma, coef = float(model.sigma_decoder), float(model.nll) / N
        if ctx.direct_tail is not None and model._stamps.get(("dec", True)) == ctx.direct_tail:
            # No d_recon tensor: hand the decoder's backward what it needs to evaluate coef / sigma^2 * g * (recon - target) itself, and a
            # token in place of the gradient
            d_recon = model._step.tail_token(recon)
            model._step.tail = _Tail(d_recon, target, sigma, coef, g, ctx.direct_tail)
        else:
            d_recon = torch.empty_like(recon)
            if ctx.categorical:
                Q, HW = recon.shape[1], recon.shape[2] * recon.shape[3]
                check(L.mmvae_ce_bwd(ptr(recon), ptr(target), ptr(weight), N, Q, HW, coef, ptr(g), ptr(d_recon), st), "mmvae_ce_bwd")
            else:
                check(L.mmvae_gauss_nll_bwd(ptr(recon), ptr(target), recon.numel(), sigma, coef, ptr(g), ptr(d_recon), st), "mmvae_gauss_nll_bwd")
        d_mu = d_lv = d_enc = None
        if mu is not None and logvar is not None:
            d_mu, d_lv = torch.empty_like(mu), torch.empty_like(logvar)
            check(L.mmvae_kl_bwd(ptr(mu), ptr(logvar), float(model.kl) / N, ptr(g), ptr(d_mu), ptr(d_lv), mu.numel(), st), "mmvae_kl_bwd")
        if encoding is not None and float(model.mmd) != 0.0:
            d_enc = torch.zeros_like(encoding)
            check(L.mmvae_mmd_bwd(ptr(ts), ptr(encoding), N, encoding.shape[1], float(model.mmd) / N, ptr(g), ptr(d_enc), st), "mmvae_mmd_bwd")
        return None, None, None, d_mu, d_lv, d_enc, d_recon, None, None
