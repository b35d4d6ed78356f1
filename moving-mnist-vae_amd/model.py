"""Drop-in ``VAE`` for the reference ``model.VAE`` (model.py:258-439), MI355X-native.

Same constructor keywords, attributes, ``forward`` / ``loss`` / helper signatures, ``state_dict`` keys and
parameter registration order as the reference; every arithmetic op of the hot path runs in hand-written HIP
kernels behind the C ABI of ``include/mmvae.h``.  PyTorch is used for device memory, the ``nn.Module`` /
autograd shell and ``torch.distributed`` only.  There is NO CPU fallback: without the built library, or
without a GPU, the model raises.

Layout: all parameters live in ONE flat f32 device buffer (``nn.Parameter``s are views into it, in the
reference's registration order), likewise gradients, Adam moments and BN running statistics -- so the
optimiser step is one kernel and the data-parallel all-reduce is two bucket-sized collectives.

This module holds the model and re-exports its neighbours: ``steps`` (the autograd functions and the step's hand-off object),
``scalars`` (step scalars, label helpers), ``optim`` (FusedAdam), ``parallel`` (Communicator, GradSync).
"""
import ctypes
import math
import os
import weakref
from typing import NamedTuple

import torch
from torch import nn

from ._lib import SUM_PARTIALS, MmvaeError, call, check, cur_stream, lib, ptr  # noqa: F401
from .optim import FusedAdam  # noqa: F401
from .parallel import Communicator, GradSync  # noqa: F401
from .scalars import DeferredScalar, _StepScalars, decode_labels, draw_labels  # noqa: F401
from .steps import _DecoderFn, _EncoderFn, _LossFn, _PendingLoss, _PixelFn, _RsampleFn, _Staged, _StepState  # noqa: F401

_DTYPES = {"f32": 0, "fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1, "fp8": 2}
_WS_KEYS = (True, False, "pix")     # VAE._ws: the net's train-mode and eval-mode workspaces, the PixelCNN's one


# a row of VAE._ptable: a parameter and its place in the flat buffer (elements)
_ParamRow = NamedTuple("_ParamRow", [("name", str), ("param", nn.Parameter), ("offset", int), ("numel", int), ("shape", tuple)])
# a row of VAE._btable: a BatchNorm buffer (kind 1: f32 statistics in _bnf, 2: the int64 batch counter in _bni) and its place there
_BufferRow = NamedTuple("_BufferRow", [("node", nn.Module), ("leaf", str), ("kind", int), ("offset", int), ("numel", int), ("shape", tuple)])


class _Scope(nn.Module):
    """Name-space node of the module tree (mirrors the reference's nesting so state_dict keys match)."""

    def __init__(self, owner=None, role=None):
        super().__init__()
        self._owner_ref = weakref.ref(owner) if owner is not None else None
        self._role = role

    def forward(self, *a, **k):  # encoder(x) / decoder(z), like VAE_Encoder / VAE_Decoder (model.py:114,181)
        owner = self._owner_ref() if self._owner_ref else None
        if owner is None or self._role is None:
            raise MmvaeError("this sub-module is a parameter name-space; call the VAE instead")
        return owner._encode(*a, **k) if self._role == "encoder" else owner._decode_full(*a, **k)

    def rsample(self, mu, logvar):   # VAE_Encoder.rsample, model.py:148-150
        owner = self._owner_ref() if self._owner_ref else None
        if owner is None or self._role != "encoder":
            raise AttributeError("rsample")
        return owner._rsample(mu, logvar)


# ------------------------------------------------------------------------------------------ the model
class VAE(nn.Module):
    def __init__(self, in_channels, intermediate_channels, decoder_out_channels=1, pixelcnn_out_channels=2, z_dimension=32,
                 pixelcnn=True, only_pixelcnn=True, pixelcnn_layers=4, pixelcnn_activation="ReLu", nll=1, kl=1, mmd=0,
                 require_rsample=True, sigma_decoder=0.1, input_image_size=64, compute_dtype=None, blocks_per_stage=1):
        """Same arguments as the reference (model.py:259-262) plus ``compute_dtype`` ("bf16" default, or "f32";
        also settable through the MMVAE_DTYPE environment variable): storage type of activations / MFMA inputs, and
        ``blocks_per_stage`` (default 1 = the reference network): residual blocks per encoder / decoder stage of the deeper
        build-defined variant (BASELINE configs[3]; include/mmvae.h: mmvae_net_create_ex)."""
        super().__init__()
        if (pixelcnn or only_pixelcnn) and pixelcnn_activation != "ReLu":
            # (the reference accepts "ELU" at the command line but its PixelCNN only knows "ReLu" / "Elu": model.py:243-246 vs main.py:100)
            raise NotImplementedError("PixelCNN is built with the ReLu activation only")
        self.in_channels = in_channels
        self.z_dimensions = z_dimension
        self.decoder_out_channels = decoder_out_channels
        self.pixelcnn_out_channels = pixelcnn_out_channels
        self.num_pixelcnn_layers = pixelcnn_layers
        self.require_rsample = require_rsample
        self.nll, self.kl, self.mmd = nll, kl, mmd
        self.sigma_decoder = sigma_decoder
        self.input_image_size = input_image_size
        self.only_pixelcnn = only_pixelcnn
        self.adjust = (64 - input_image_size) // 2 if input_image_size > 32 else (32 - input_image_size) // 2   # model.py:307-310
        dt = compute_dtype or os.environ.get("MMVAE_DTYPE", "bf16")
        if dt not in _DTYPES:
            raise ValueError(f"compute_dtype must be one of {sorted(_DTYPES)}")
        self.compute_dtype = {0: "f32", 1: "bf16", 2: "fp8"}[_DTYPES[dt]]

        L = lib()
        d = self.__dict__
        self.blocks_per_stage = int(blocks_per_stage)
        d["_ptable"], d["_btable"] = [], []
        # ---- PixelCNN first: the reference registers it before the encoder / decoder (model.py:283-300), so its parameters lead the
        # parameter list and the state_dict
        d["_hp"], d["_poff"] = None, 0
        pix_in = in_channels if only_pixelcnn else decoder_out_channels + in_channels                          # model.py:288,312
        if only_pixelcnn or pixelcnn:
            hp = ctypes.c_void_p()
            check(L.mmvae_pixelcnn_create(ctypes.byref(hp), pix_in, intermediate_channels, pixelcnn_out_channels, pixelcnn_layers,
                                          1 if _DTYPES[dt] != 0 else 0), "mmvae_pixelcnn_create")
            d["_hp"], d["_poff"] = hp, int(L.mmvae_pixelcnn_num_params(hp))
        # ---- encoder / decoder
        d["_h"] = None
        n_params, n_bnf, dec_off = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        n_bni, dec_side = ctypes.c_int32(0), ctypes.c_int32(0)
        if not only_pixelcnn:
            h = ctypes.c_void_p()
            check(L.mmvae_net_create_ex(ctypes.byref(h), in_channels, z_dimension, decoder_out_channels, input_image_size,
                                        int(bool(require_rsample)), _DTYPES[dt], self.blocks_per_stage), "mmvae_net_create_ex")
            d["_h"] = h
            check(L.mmvae_net_sizes(h, ctypes.byref(n_params), ctypes.byref(n_bnf), ctypes.byref(n_bni), ctypes.byref(dec_off),
                                    ctypes.byref(dec_side)), "mmvae_net_sizes")
        d["_n_params"], d["_n_bnf"], d["_n_bni"] = self._poff + n_params.value, n_bnf.value, n_bni.value
        d["_dec_off"], d["_dec_side"] = self._poff + dec_off.value, dec_side.value          # absolute: first decoder parameter of the flat buffer
        d["_flat"] = torch.zeros(self._n_params, dtype=torch.float32)
        d["_bnf"] = torch.zeros(self._n_bnf, dtype=torch.float32)
        d["_bni"] = torch.zeros(self._n_bni, dtype=torch.int64)
        d["_G"] = [None, None]
        d["_ws"] = dict.fromkeys(_WS_KEYS)
        d["_stamps"] = {}
        d["_sync"] = None
        d["_step"] = _StepState()          # what one phase of a step leaves for a later one (steps.py)
        d["_last_group"] = None            # the _StepScalars of the last loss() (main.train reads it)
        # Gaussian NLL: fold the loss gradient into the decoder's backward (no d_recon tensor).  Set False when the reconstruction
        # tensor feeds anything besides VAE.loss in the autograd graph.
        d["fuse_loss_tail"] = os.environ.get("MMVAE_FUSE_LOSS_TAIL", "1") != "0"
        # keep the decoder's weight gradients in flight on the side stream past its backward (_DecoderFn.backward); developer A/B switch
        d["defer_join"] = os.environ.get("MMVAE_DEFER_JOIN", "1") != "0"
        d["injected_eps"] = None           # parity tests: noise for rsample / loss instead of torch.randn
        d["injected_true_samples"] = None
        if self._hp is not None:
            d["_pix_mask"] = self._build_pixel_tree(pix_in, intermediate_channels, pixelcnn_out_channels, pixelcnn_layers)
        else:
            self.pixelcnn = None
        if self._h is not None:
            self._build_tree(L)
        # the table's three regions, in flat-buffer (= registration) order: the one source of the per-region parameter lists and gradient views
        d["_pix_rows"] = [r for r in self._ptable if r.offset < self._poff]
        d["_enc_rows"] = [r for r in self._ptable if self._poff <= r.offset < self._dec_off]
        d["_dec_rows"] = [r for r in self._ptable if r.offset >= self._dec_off]
        d["_pix_params"], d["_enc_params"], d["_dec_params"] = ([r.param for r in rows] for rows in (self._pix_rows, self._enc_rows, self._dec_rows))
        d["_grad_key"] = (self._enc_rows or self._pix_rows)[0].param          # see _grad_target
        self._reset_parameters()

    # ---- construction helpers
    def _build_tree(self, L):
        name_buf = ctypes.create_string_buffer(128)
        ndim, kind = ctypes.c_int32(), ctypes.c_int32()
        shape = (ctypes.c_int32 * 4)()
        off = ctypes.c_int64()
        for i in range(L.mmvae_net_num_entries(self._h)):
            check(L.mmvae_net_entry(self._h, i, name_buf, 128, ctypes.byref(ndim), shape, ctypes.byref(kind), ctypes.byref(off)), "mmvae_net_entry")
            name = name_buf.value.decode()
            shp = tuple(shape[k] for k in range(ndim.value))
            numel = math.prod(shp)
            parts = name.split(".")
            node = self
            for depth, comp in enumerate(parts[:-1]):
                if comp not in node._modules:
                    role = comp if (depth == 0 and comp in ("encoder", "decoder")) else None
                    node.add_module(comp, _Scope(self, role))
                node = node._modules[comp]
            if kind.value == 0:
                o = self._poff + off.value
                p = nn.Parameter(self._flat[o:o + numel].view(shp))
                p._mmvae_owner = weakref.ref(self)
                node.register_parameter(parts[-1], p)
                self._ptable.append(_ParamRow(name, p, o, numel, shp))
            else:                                              # (kind 2, a batch counter, is a 0-dim entry: one element, shape ())
                buf = self._bnf if kind.value == 1 else self._bni
                node.register_buffer(parts[-1], buf[off.value:off.value + numel].view(shp))
                self._btable.append(_BufferRow(node, parts[-1], kind.value, off.value, numel, shp))

    def _build_pixel_tree(self, pix_in, mid, pix_out, layers):
        """pixelcnn.layers.<i>.{weight, bias, mask}: the reference's names and order (model.py:234-241; `mask` is a registered buffer, :216)."""
        top = _Scope(self, None)
        self.add_module("pixelcnn", top)
        lay = _Scope(self, None)
        top.add_module("layers", lay)
        off = 0
        masks = []
        for i in range(layers):
            cin = pix_in if i == 0 else mid
            cout = pix_out if i == layers - 1 else mid
            node = _Scope(self, None)
            lay.add_module(str(i), node)
            for leaf, shp in (("weight", (cout, cin, 7, 7)), ("bias", (cout,))):
                n = math.prod(shp)
                p = nn.Parameter(self._flat[off:off + n].view(shp))
                p._mmvae_owner = weakref.ref(self)
                node.register_parameter(leaf, p)
                self._ptable.append(_ParamRow(f"pixelcnn.layers.{i}.{leaf}", p, off, n, shp))
                off += n
            m = torch.ones(cout, cin, 7, 7)
            m[:, :, 3, 3 + (0 if i == 0 else 1):] = 0                  # type 'A' first, 'B' afterwards (model.py:216-220, :234-239)
            m[:, :, 4:] = 0
            node.register_buffer("mask", m)
            masks += [m.reshape(-1), torch.ones(cout)]
        assert off == self._poff
        return torch.cat(masks)                     # multiplies the PixelCNN's flat parameter region (biases: ones)

    @torch.no_grad()
    def _reset_parameters(self):
        """PyTorch default initialisation in the reference's module-construction order, so that
        ``torch.manual_seed(s); VAE(...)`` yields the same parameters as the reference under the same seed:
        convs kaiming_uniform(a=sqrt(5)), conv bias U(+-1/sqrt(fan_in)), BN gamma=1 beta=0, running stats (0,1).
        Order: a block's shortcut conv is created before its main-path convs (model.py:132-141, :196-207)."""
        byname = {r.name: r.param for r in self._ptable}

        def conv(name):
            nn.init.kaiming_uniform_(byname[name], a=math.sqrt(5))

        def conv_and_bias(pre):             # nn.Conv2d.reset_parameters of a conv with a bias: weight, then bias
            conv(pre + "weight")
            w = byname[pre + "weight"]
            bound = 1.0 / math.sqrt(w.shape[1] * w.shape[2] * w.shape[3])
            nn.init.uniform_(byname[pre + "bias"], -bound, bound)

        # PixelCNN first (constructed first, model.py:283-300), layer by layer
        for i in range(len(self._pix_rows) // 2):
            conv_and_bias(f"pixelcnn.layers.{i}.")
        if self._h is None:
            return
        conv("encoder.conv1.weight")
        for i in range(1, 5):
            j = 0
            while f"encoder.layer{i}.{j}.conv1.weight" in byname:
                pre = f"encoder.layer{i}.{j}."
                if pre + "downsample.0.weight" in byname:
                    conv(pre + "downsample.0.weight")
                conv(pre + "conv1.weight"); conv(pre + "conv2.weight")
                j += 1
        conv("encoder.conv_mu.weight")
        if self.require_rsample:
            conv("encoder.conv_logvar.weight")
        conv("decoder.conv1.weight")
        i = 1
        while f"decoder.uplayer{i}.0.conv1.weight" in byname:
            # reference construction order of a stage: the upsample shortcut, then the blocks in order (model.py:196-209)
            j = 0
            while f"decoder.uplayer{i}.{j}.conv1.weight" in byname:
                j += 1
            conv(f"decoder.uplayer{i}.{j - 1}.upsample.0.weight")
            for b in range(j):
                pre = f"decoder.uplayer{i}.{b}."
                conv(pre + "conv1.weight"); conv(pre + "conv2.weight")
            i += 1
        conv_and_bias("decoder.conv2.")
        for r in self._ptable:
            if len(r.shape) == 1 and r.name != "decoder.conv2.bias" and not r.name.startswith("pixelcnn."):
                r.param.fill_(1.0 if r.name.endswith(".weight") else 0.0)
        for r in self._btable:
            b = r.node._buffers[r.leaf]
            if r.leaf == "running_var":
                b.fill_(1.0)
            else:
                b.zero_()

    # ---- flat storage management
    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        self._reflatten()
        return self

    @torch.no_grad()
    def _reflatten(self):
        dev = self._ptable[0].param.device
        flat = torch.empty(self._n_params, dtype=torch.float32, device=dev)
        for (_, p, off, n, shp) in self._ptable:
            flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = flat[off:off + n].view(shp)
            p.grad = None
        bnf = torch.empty(self._n_bnf, dtype=torch.float32, device=dev)
        bni = torch.empty(self._n_bni, dtype=torch.int64, device=dev)
        for r in self._btable:
            dst = (bnf if r.kind == 1 else bni)[r.offset:r.offset + r.numel]
            dst.copy_(r.node._buffers[r.leaf].reshape(-1))
            r.node._buffers[r.leaf] = dst.view(r.shape)
        d = self.__dict__
        d["_flat"], d["_bnf"], d["_bni"] = flat, bnf, bni
        d["_G"] = [None, None]
        d["_ws"] = dict.fromkeys(_WS_KEYS)
        self._step.reset()
        if self._hp is not None:
            d["_pix_mask"] = self._pix_mask.to(dev)

    def _ensure_flat(self):
        first, last = self._ptable[0], self._ptable[-1]
        base, es = self._flat.data_ptr(), 4
        if first.param.data_ptr() != base + first.offset * es or last.param.data_ptr() != base + last.offset * es:
            self._reflatten()
        if not self._flat.is_cuda:
            raise MmvaeError("the HIP VAE only runs on a GPU: call model.to('cuda') first (there is no CPU fallback; "
                             "the CPU restatement under oracle/ is test infrastructure)")

    def _net_ptr(self, flat_like):
        """Device address of the encoder / decoder's region of a flat parameter-shaped buffer (behind the PixelCNN's, if any)."""
        return flat_like.data_ptr() + 4 * self._poff

    def _pixel_workspace(self, N, S):
        """The PixelCNN's one workspace, shared by forward / backward and the sampler (sized for whichever asks for more)."""
        return self._grown("pix", max(lib().mmvae_pixelcnn_workspace_bytes(self._hp, int(N), int(S)),
                                      lib().mmvae_pixelcnn_sample_workspace_bytes(self._hp, int(N), int(S))))

    def _workspace(self, N, training):
        """The net's workspace of this mode (train and eval keep one each: an eval pass leaves the saved activations of a train step alone)."""
        return self._grown(training, lib().mmvae_net_workspace_bytes(self._h, int(N)))

    def _grown(self, key, need):
        """Workspace `key` (_WS_KEYS), reallocated only when it is too small or on another device than the parameters."""
        ws = self._ws[key]
        if ws is None or ws.numel() < need or ws.device != self._flat.device:
            ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=self._flat.device)
        return ws

    def _ws_view(self, dev_ptr, n):
        """f32 view of n floats at a device address inside one of this model's workspaces (SyncBN all-reduce operands)."""
        for ws in self._ws.values():
            if ws is not None and ws.data_ptr() <= dev_ptr < ws.data_ptr() + ws.numel():
                off = dev_ptr - ws.data_ptr()
                return ws[off:off + 4 * n].view(torch.float32)
        raise MmvaeError("sync_bn: operand outside the model's workspace")

    def _stamp(self, which, training):
        tok = self._stamps[which, training] = self._stamps.get((which, training), 0) + 1
        return tok

    def _check_stamp(self, which, tok, training, overwritten="the saved activations of this forward were overwritten by a later forward; "
                                                             "call backward before running the model again in train mode"):
        if not training:
            raise MmvaeError("backward through an eval-mode forward is not supported (BatchNorm batch statistics are needed)")
        if self._stamps.get((which, training)) != tok:
            raise MmvaeError(overwritten)

    def _grad_target(self):
        """Flat gradient buffer to write into: buffer 0 normally; buffer 1 when .grad tensors already exist
        (so that autograd's accumulation into them stays correct).  The choice is keyed on the parameter whose .grad autograd
        writes LAST in a backward pass -- the encoder's first parameter (the PixelCNN's when there is no encoder): its .grad does not change
        between the backward nodes of one pass (PixelCNN -> decoder -> encoder), so all of them pick the same buffer."""
        g, G0 = self._grad_key.grad, self._G[0]
        idx = int(g is not None and G0 is not None and G0.data_ptr() <= g.data_ptr() < G0.data_ptr() + 4 * self._n_params)
        if self._G[idx] is None or self._G[idx].device != self._flat.device:
            self._G[idx] = torch.zeros(self._n_params, dtype=torch.float32, device=self._flat.device)
        return self._G[idx]

    @staticmethod
    def _grad_views(G, rows):
        """The gradients of one region's parameters (_pix_rows, _enc_rows or _dec_rows) as views of the flat gradient buffer G."""
        chunks = G[rows[0].offset:rows[-1].offset + rows[-1].numel].split([r.numel for r in rows])
        return tuple(c.view(r.shape) for c, r in zip(chunks, rows))

    # ---- the reference surface
    def _encode(self, x):
        self._ensure_flat()
        x = x.contiguous().float()
        S = self.input_image_size
        if x.dim() != 4 or x.shape[1] != self.in_channels or x.shape[2] != S or x.shape[3] != S:
            raise ValueError(f"expected input (N,{self.in_channels},{S},{S}), got {tuple(x.shape)}")
        out = _EncoderFn.apply(self, x, *self._enc_params)
        return out if self.require_rsample else (out, None)

    def _rsample(self, mu, logvar):
        eps = self.injected_eps
        if eps is None:
            eps = torch.randn(mu.shape, device=mu.device, dtype=mu.dtype)
        return _RsampleFn.apply(mu, logvar, eps.to(mu.device).view(mu.shape))

    def _decode_full(self, encoding):
        self._ensure_flat()
        enc = encoding.contiguous().float().view(-1, self.z_dimensions, 1, 1)
        return _DecoderFn.apply(self, enc, *self._dec_params)

    def _decode(self, encoding):
        out = self._decode_full(encoding)
        if self.adjust != 0:                                   # model.py:328-329
            out = out[:, :, self.adjust:-self.adjust, self.adjust:-self.adjust]
        return out

    def run_pixelcnn(self, concat):                            # model.py:350-351
        if self._hp is None:
            raise MmvaeError("this model has no PixelCNN")
        self._ensure_flat()
        x = concat.contiguous().float()
        if x.dim() != 4 or x.shape[2] != x.shape[3]:
            raise ValueError(f"expected a square (N, C, S, S) input, got {tuple(x.shape)}")
        return _PixelFn.apply(self, x, *self._pix_params)

    @torch.no_grad()
    def sample_pixels(self, sample, z_image=None, *, data_mean, data_std, uniforms=None, generator=None, return_probs=False):
        """The autoregressive sampler of main.py:186-202 as ONE call (mmvae_pixelcnn_sample): all S x S pixels are enqueued on the current
        stream, no host work per pixel.  ``sample`` (N, C, S, S) is updated in place, pixel by pixel in row-major order, with
        ``(label - sub_mean) / data_std`` in every channel, the label drawn from the softmax of the PixelCNN's logits at that pixel.
        A PixelCNN-only model takes ``z_image=None`` and uses ``sub_mean = 0`` (the reference's ``generate_only_pixelcnn`` does not subtract
        the mean); a PixelVAE needs ``z_image`` (what ``get_z_image`` returns) and uses ``sub_mean = data_mean`` (``generate``).

        The written value is the correctly rounded f32 quotient, as in ``prepare_batch``'s images (torch on the GPU multiplies by the
        reciprocal of the scalar instead: the reference loop's values can differ from these in the last bit).

        Randomness: ``label = draw_labels(probs, u)`` with ``u = uniforms[n, i * S + j]``; ``uniforms=None`` draws them with
        ``torch.rand((N, S * S), generator=generator)``.  That is the distribution of ``torch.multinomial(probs, 1)`` but another random
        stream: the same seed gives other images than the reference's loop.

        Returns ``(out_logits, sample)`` like the reference's functions -- the logits are those of the last full forward, i.e. on the
        sample as it was before the last pixel was written -- plus ``(probs (N, S*S, Q) f32, labels (N, S*S) int64)`` of every draw with
        ``return_probs=True``.  Works in train and eval mode (InstanceNorm has no running statistics).  Like a forward it masks the stored
        weights, and it reuses the PixelCNN's workspace: a backward through an earlier forward raises afterwards."""
        if self._hp is None:
            raise MmvaeError("this model has no PixelCNN")
        self._ensure_flat()
        if sample.dim() != 4 or sample.shape[2] != sample.shape[3]:
            raise ValueError(f"expected a square (N, C, S, S) sample, got {tuple(sample.shape)}")
        N, Cs, S = sample.shape[0], sample.shape[1], sample.shape[2]
        dev = self._flat.device
        if sample.device != dev:
            raise ValueError(f"sample is on {sample.device}, the model on {dev}")
        if self.only_pixelcnn:
            if z_image is not None:
                raise ValueError("a PixelCNN-only model takes no z_image")
            cond, Cc, sub_mean = None, 0, 0.0                                  # main.py:191 (sic)
        else:
            if z_image is None:
                raise ValueError("a PixelVAE samples conditioned on z_image (model.get_z_image(encoding))")
            cond = z_image.to(dev).contiguous().float()
            if cond.dim() != 4 or cond.shape[0] != N or tuple(cond.shape[2:]) != (S, S):
                raise ValueError(f"z_image {tuple(z_image.shape)} does not match sample {tuple(sample.shape)}")
            Cc, sub_mean = cond.shape[1], float(data_mean)                     # main.py:201
        work = sample if (sample.dtype == torch.float32 and sample.is_contiguous()) else sample.contiguous().float()
        if uniforms is None:
            uniforms = torch.rand((N, S * S), device=dev, generator=generator)
        u = uniforms.to(dev).contiguous().float()
        if u.numel() != N * S * S:
            raise ValueError(f"uniforms must hold N * S * S = {N * S * S} values, got {tuple(uniforms.shape)}")
        Q = self.pixelcnn_out_channels
        out = torch.empty((N, Q, S, S), device=dev, dtype=torch.float32)
        probs = torch.empty((N, S * S, Q), device=dev, dtype=torch.float32) if return_probs else None
        labels = torch.empty((N, S * S), device=dev, dtype=torch.int64) if return_probs else None
        self._flat[:self._poff].mul_(self._pix_mask)                           # model.py:222: weight.data *= mask in every forward
        ws = self._pixel_workspace(N, S)
        self._stamp("pix", True)                                               # the workspace of an earlier forward is gone
        check(lib().mmvae_pixelcnn_sample(self._hp, N, S, ptr(cond), Cc, ptr(work), Cs, ptr(u), sub_mean, float(data_std), ptr(self._flat),
                                          ptr(ws), ws.numel(), ptr(out), ptr(probs), ptr(labels), cur_stream()), "mmvae_pixelcnn_sample")
        if work is not sample:
            sample.copy_(work)
        return (out, sample, probs, labels) if return_probs else (out, sample)

    def is_categorical(self):
        """p(x|z) is categorical (cross entropy), not Gaussian: with a PixelCNN, or a decoder that emits more channels than the input has
        (model.py:398, main.py:381).  Reads attributes only: ``VAE.is_categorical(m)`` also answers for a reference or oracle model."""
        return self.pixelcnn is not None or self.decoder_out_channels > self.in_channels

    def forward(self, x, sample=None):
        """model.py:316-342: returns (mu, logvar, encoding, reconstruction).  With a PixelCNN the reconstruction is its output on
        concat([decoder_output, x]) in train mode / concat([decoder_output, sample]) in eval mode (:331-336); only_pixelcnn: on x itself."""
        if self.only_pixelcnn:
            return None, None, None, self.run_pixelcnn(x)                                   # :339-340
        mu, logvar = self._encode(x)
        encoding = self._rsample(mu, logvar) if self.require_rsample else mu
        decoder_output = self._decode(encoding)
        if self._hp is None:
            return mu, logvar, encoding, decoder_output
        other = x if self.training else sample
        if other is None:
            raise ValueError("a PixelVAE in eval mode needs `sample` (model.py:334-335)")
        return mu, logvar, encoding, self.run_pixelcnn(torch.cat([decoder_output, other.to(decoder_output.dtype)], dim=1))

    def get_z_image(self, encoding):                           # model.py:344-348
        return self._decode(encoding)

    def get_reconstruction(self, encoding, sample=None):       # model.py:353-362
        decoder_output = self._decode(encoding)
        if self._hp is None:
            return decoder_output
        return self.run_pixelcnn(torch.cat([decoder_output, sample.to(decoder_output.dtype)], dim=1))

    def decode_labels(self, logits, mode="argmax", uniforms=None, generator=None):
        """``decode_labels`` of this module: class labels int64 (N, H, W) of a logits tensor (N, Q, H, W), by argmax or one draw per pixel."""
        return decode_labels(logits, mode=mode, uniforms=uniforms, generator=generator)

    def kl_divergence(self, encoding_mu, encoding_logvar):     # model.py:364-365
        acc = torch.zeros(1 + SUM_PARTIALS, dtype=torch.float64, device=encoding_mu.device)       # the sum, then its scratch
        mu, lv = encoding_mu.contiguous().float(), encoding_logvar.contiguous().float()
        check(lib().mmvae_kl_fwd_ex(ptr(mu), ptr(lv), mu.numel(), ptr(acc), ptr(acc) + 8, cur_stream()), "mmvae_kl_fwd_ex")
        return acc[0].float()

    def compute_kernel(self, x, y):                            # model.py:367-376
        """(x_size, y_size) matrix exp(-mean_d((x_i - y_j)^2) / d) -- the helper itself; ``loss`` never materialises it."""
        x, y = x.contiguous().float(), y.contiguous().float()
        if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1]:
            raise ValueError("compute_kernel expects (n, d) and (m, d)")
        out = torch.empty((x.shape[0], y.shape[0]), dtype=torch.float32, device=x.device)
        check(lib().mmvae_rbf_kernel(ptr(x), ptr(y), x.shape[0], y.shape[0], x.shape[1], ptr(out), cur_stream()), "mmvae_rbf_kernel")
        return out

    def compute_mmd(self, x, y):                               # model.py:378-383
        acc = torch.zeros(1 + SUM_PARTIALS, dtype=torch.float64, device=x.device)                # the sum, then its scratch
        x, y = x.contiguous().float(), y.contiguous().float()
        check(lib().mmvae_mmd_fwd_ex(ptr(x), ptr(y), x.shape[0], x.shape[1], None, ptr(acc), ptr(acc) + 8, cur_stream()), "mmvae_mmd_fwd_ex")
        return acc[0].float()

    def loss(self, target, encoding_mu, encoding_logvar, encoding, reconstruction, device, args, deferred=False):
        """model.py:385-406: returns (loss tensor with grad, nll/N, kl/N, mmd/N as Python floats) -- ONE device->host
        copy of the four scalars instead of the reference's three ``.item()`` calls.  ``deferred=True`` (used by this
        package's ``train``) returns float-like ``DeferredScalar``s instead, read back when first used, so that the host
        does not wait for the forward pass before it enqueues the backward pass."""
        N = target.shape[0]
        dev = reconstruction.device
        categorical = self.is_categorical()
        ts = enc2 = weight = None
        if encoding is not None:
            enc2 = encoding.view(-1, encoding.shape[1])
            ts = self.injected_true_samples
            if ts is None:
                ts = torch.randn(N, encoding.shape[1], device=dev)          # model.py:395
            ts = ts.to(dev).contiguous().float()
        if categorical:
            weight = getattr(args, "data_ratio_of_labels", None)
            if weight is not None:
                weight = weight.to(dev).contiguous().float()
            target = target.long()
        # the side-stream form needs the backward pass that follows to join it (and to keep the operands alive): train steps only
        rec = _PendingLoss(side=bool(deferred and self.training and torch.is_grad_enabled() and reconstruction.requires_grad and self._h is not None))
        loss_t = _LossFn.apply(self, rec, target, encoding_mu, encoding_logvar, enc2, reconstruction, ts, weight)
        join = None
        if rec.side:
            wr, mine = weakref.ref(self), rec.out    # (weak: the group hangs off the model; and not `rec`: train() keeps the groups, not the operands)

            def join():
                net = wr()
                if net is not None and net._h is not None:     # (a destroyed net has synchronised its side stream)
                    net._step.flush_loss(cur_stream(), only=mine)        # never launched (no decoder backward ran): here, on this stream
                    check(lib().mmvae_net_join(net._h, cur_stream()), "mmvae_net_join")
        grp = _StepScalars(rec.out, join)
        self._last_group = grp
        if deferred:
            return loss_t, DeferredScalar(grp, 1), DeferredScalar(grp, 2), DeferredScalar(grp, 3)
        return loss_t, grp.get(1), grp.get(2), grp.get(3)

    # ---- held-out evaluation: per-image terms (csrc/eval_loss.hip).  The reference has no counterpart: it builds a test loader (main.py:497)
    # and never reads it.
    def _nll_rows(self, target, reconstruction, weight, out):
        """Raw per-image negative log-likelihood of `reconstruction` into `out` (f64, N contiguous values on the device): categorical under
        the condition of `loss` (model.py:398), Gaussian with sigma_decoder otherwise; not scaled by self.nll."""
        dev = self._flat.device
        N = reconstruction.shape[0]
        if reconstruction.device != dev or reconstruction.dim() != 4:
            raise ValueError(f"expected an (N, C, H, W) reconstruction on {dev}, got {tuple(reconstruction.shape)} on {reconstruction.device}")
        recon = reconstruction.detach().float().contiguous()          # (the crop of a 28 x 28 model is a strided view)
        if self.is_categorical():
            Q, HW = recon.shape[1], recon.shape[2] * recon.shape[3]
            tgt = target.detach().to(dev).long().contiguous()
            if tgt.numel() != N * HW:
                raise ValueError(f"target {tuple(target.shape)} does not hold one label per pixel of {tuple(recon.shape)}")
            w = None
            if weight is not None:
                w = weight.detach().to(dev).float().contiguous()
                if w.numel() != Q:
                    raise ValueError(f"weight must hold {Q} values, got {tuple(weight.shape)}")
            check(lib().mmvae_ce_per_image(ptr(recon), ptr(tgt), ptr(w), N, Q, HW, ptr(out), cur_stream()), "mmvae_ce_per_image")
        else:
            tgt = target.detach().to(dev).float().contiguous()
            if tgt.numel() != recon.numel():
                raise ValueError(f"target {tuple(target.shape)} does not match the reconstruction {tuple(recon.shape)}")
            check(lib().mmvae_gauss_nll_per_image(ptr(recon), ptr(tgt), N, recon.numel() // N, float(self.sigma_decoder), ptr(out), cur_stream()),
                  "mmvae_gauss_nll_per_image")

    def per_image_terms(self, target, encoding_mu, encoding_logvar, reconstruction, weight=None):
        """The two terms of the ELBO per image, as f64 device tensors (no host read): ``(nll [N], kl [N] or None)``.  ``nll`` is the raw
        negative log-likelihood -log p(x|z) of the reconstruction -- the summand of ``loss`` before the ``self.nll`` coefficient and the
        division by N, cross-entropy or Gaussian under the same condition (``weight``: per-class weights of the cross-entropy; None, the
        default, gives a true likelihood) -- and ``kl`` the analytic KL(q(z|x) || N(0, I)), None without a logvar."""
        self._ensure_flat()
        N = reconstruction.shape[0]
        dev = self._flat.device
        nll = torch.empty(N, dtype=torch.float64, device=dev)
        self._nll_rows(target, reconstruction, weight, nll)
        if encoding_logvar is None or encoding_mu is None:
            return nll, None
        mu, lv = encoding_mu.detach().float().contiguous(), encoding_logvar.detach().float().contiguous()
        if mu.shape[0] != N or lv.shape != mu.shape or mu.device != dev:
            raise ValueError(f"mu {tuple(mu.shape)} / logvar {tuple(lv.shape)} do not match {N} images on {dev}")
        kl = torch.empty(N, dtype=torch.float64, device=dev)
        check(lib().mmvae_kl_per_image(ptr(mu), ptr(lv), N, mu.numel() // N, ptr(kl), cur_stream()), "mmvae_kl_per_image")
        return nll, kl

    @torch.no_grad()
    def iw_bound(self, x, target, K, eps=None, generator=None, weight=None):
        """Importance-weighted bound (Burda et al. 2016) on log p(x) per image, f64 [N] on the device, from K samples of q(z|x):
        ``log (1/K) sum_k p(x|z_k) p(z_k) / q(z_k|x)``.  K = 1 is a one-sample ELBO estimate; the bound tightens with K.

        One encoder forward, then K passes of reparameterisation, decoder and (PixelVAE) the PixelCNN teacher-forced on ``x`` as in
        ``forward(x, sample=x)``; each pass writes row k of two f64 [K, N] buffers (mmvae_gauss_nll_per_image / mmvae_ce_per_image,
        mmvae_latent_logratio) and mmvae_iw_bound reduces them.  ``eps`` [K, N, z] is the noise; None draws it with
        ``torch.randn(..., generator=generator)``.  Eval mode only: batch statistics would make the images of a batch interact."""
        if self.only_pixelcnn:
            raise ValueError("a PixelCNN on its own has no latent code: no importance-weighted bound")
        if not self.require_rsample:
            raise ValueError("iw_bound needs q(z|x): the model was built with require_rsample=False")
        K = int(K)
        if K < 1:
            raise ValueError(f"K must be >= 1, got {K}")
        if self.training:
            raise MmvaeError("iw_bound runs in eval mode only (train-mode BatchNorm couples the images of a batch): call model.eval() first")
        mu, logvar = self._encode(x)
        N, z = mu.shape[0], self.z_dimensions
        dev = mu.device
        if eps is None:
            eps = torch.randn((K, N, z), device=dev, dtype=torch.float32, generator=generator)
        eps = eps.to(dev).float().contiguous()
        if eps.numel() != K * N * z:
            raise ValueError(f"eps must be (K, N, z) = ({K}, {N}, {z}), got {tuple(eps.shape)}")
        eps = eps.view(K, N, z)
        rows = torch.empty((2, K, N), dtype=torch.float64, device=dev)          # [0]: nll, [1]: log p(z) - log q(z|x)
        for k in range(K):
            encoding = _RsampleFn.apply(mu, logvar, eps[k].view(mu.shape))
            recon = self._decode(encoding)
            if self._hp is not None:
                recon = self.run_pixelcnn(torch.cat([recon, x.to(recon.dtype)], dim=1))
            self._nll_rows(target, recon, weight, rows[0, k])
            check(lib().mmvae_latent_logratio(ptr(mu), ptr(logvar), ptr(eps[k]), N, z, ptr(rows[1, k]), cur_stream()), "mmvae_latent_logratio")
        out = torch.empty(N, dtype=torch.float64, device=dev)
        check(lib().mmvae_iw_bound(ptr(rows[0]), ptr(rows[1]), K, N, ptr(out), cur_stream()), "mmvae_iw_bound")
        return out

    # ---- train-loop hook (main.py:374-388): labels -> normalised frames, one kernel
    def prepare_batch(self, batch, device, data_mean, data_std, categorical):
        S = self.input_image_size
        labels = batch.to(device)
        if labels.dtype not in (torch.int64, torch.uint8):
            labels = labels.long()
        labels = labels.contiguous()
        N = labels.numel() // (S * S * self.in_channels)
        image = torch.empty((N, self.in_channels, S, S), device=labels.device, dtype=torch.float32)
        self._ensure_flat()
        if self._h is None:
            # a PixelCNN on its own (main.py:50-58 "pixelcnn_N"): no encoder workspace to stage into, the f32 image only
            labels = labels.long()
            check(lib().mmvae_normalise_labels(ptr(labels), image.numel(), float(data_mean), float(data_std), ptr(image), cur_stream()),
                  "mmvae_normalise_labels")
            self._step.staged = None
        else:
            # one pass: the f32 image (network input, Gaussian target) and its storage-type copy straight into the workspace the forward
            # pass is about to use (train() calls the model right after; _EncoderFn checks that it really is this tensor object, unmodified)
            ws = self._workspace(N, bool(self.training))
            check(lib().mmvae_net_stage_labels(self._h, N, ptr(labels), labels.element_size(), float(data_mean), float(data_std), ptr(image), ptr(ws),
                                               ws.numel(), cur_stream()), "mmvae_net_stage_labels")
            self._step.staged = _Staged(weakref.ref(image), image._version, ws.data_ptr(), N)
        return image, (labels.view(-1, S, S).long() if categorical else image)

    def __repr__(self):
        """The reference's description text (model.py:408-439)."""
        size = str(self.input_image_size) + "x" + str(self.input_image_size) + "x"
        string = ""
        pixelcnn_input = size
        if self.only_pixelcnn:
            pixelcnn_used = "by itself"
            pixelcnn_input += str(self.in_channels)
        else:
            pixelcnn_used = "in the decoder"
            pixelcnn_input += str(self.in_channels + self.decoder_out_channels)
            rsample_text = " Where Z is rsampled from a Normal Distribution." if self.require_rsample else ""
            string += ("We are using an encoder which takes input of " + size + str(self.in_channels) + " and encodes into " +
                       str(self.z_dimensions) + " dimensional latent space." + rsample_text +
                       " \nIt is then pushed into a decoder which outputs an image of dimension " + size +
                       str(self.decoder_out_channels) + ".\n")
        if self.pixelcnn is None:
            if self.decoder_out_channels == self.in_channels:
                string += "We assume p(x/z) follows a normal distribution with mean x_recon and sigma " + str(self.sigma_decoder) + ".\n"
            else:
                string += "We assume p(x/z) follows a categorical distribution. \n"
        else:
            string += ("We are using PixelCNN " + pixelcnn_used + " which takes an input of " + pixelcnn_input + " dimension goes through " +
                       str(self.num_pixelcnn_layers) + " layers and outputs a " + size + str(self.pixelcnn_out_channels) + " dimensions image")
        return string

    def extra_repr(self):
        return f"MI355X/HIP backend, compute_dtype={self.compute_dtype}"

    def __del__(self):
        try:
            h = self.__dict__.get("_h")
            if h:
                lib().mmvae_net_destroy(h)
            hp = self.__dict__.get("_hp")
            if hp:
                lib().mmvae_pixelcnn_destroy(hp)
        except Exception:
            pass
