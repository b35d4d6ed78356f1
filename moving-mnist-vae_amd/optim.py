"""torch.optim.Adam over the model's flat parameter buffer: one HIP kernel per step."""
import math
import weakref

import torch

from ._lib import SUM_PARTIALS, MmvaeError, check, cur_stream, lib, ptr


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (defaults of main.py:468) as ONE HIP kernel over the model's flat parameter buffer.
    Drop-in: ``FusedAdam(list(model.parameters()))``; ``state_dict()`` has the torch.optim.Adam layout."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False, max_grad_norm=None,
                 skip_nonfinite=False):
        """capturable=True keeps the step count on the device (mmvae_adam_step_dev), so that a train step captured in a HIP graph
        (torch.cuda.graph) replays with advancing bias corrections; the eager default computes them on the host.

        max_grad_norm (a positive float) clips the global gradient norm as torch.nn.utils.clip_grad_norm_ does, and skip_nonfinite=True
        leaves parameters, moments and the step count alone on a step whose gradients hold an inf or a NaN (what GradScaler does);
        either one selects mmvae_adam_step_guarded, which does both on the stream: no host read, capturable, and a clipped step
        skips a non-finite gradient too (its norm is not finite, so there is no factor to clip by).  The step count then lives on the
        device as with capturable=True.  The one deliberate difference from clip_grad_norm_: ``.grad`` is NOT rewritten -- the clip
        factor exists only inside the kernel, folded with the data-parallel 1/world scale; read the norm from ``grad_norm``."""
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be a positive number or None")
        params = list(params)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        owner = getattr(params[0], "_mmvae_owner", None)
        model = owner() if owner is not None else None
        if model is None or [id(p) for p in params] != [id(e.param) for e in model._ptable]:
            raise MmvaeError("FusedAdam needs exactly list(model.parameters()) of one HIP VAE, in order")
        self._model = weakref.ref(model)
        self._t = 0
        self._m = self._v = None
        self._capturable = bool(capturable)
        self._step_dev = None
        self._guarded = max_grad_norm is not None or bool(skip_nonfinite)
        self._max_norm = float(max_grad_norm) if max_grad_norm is not None else 0.0      # <= 0: skip only (mmvae.h)
        self._guard = None

    def _moments(self, model):
        flat = model._flat
        if self._m is None or self._m.device != flat.device:
            old_m, old_v = self._m, self._v
            self._m, self._v = torch.zeros_like(flat), torch.zeros_like(flat)
            if old_m is not None:
                self._m.copy_(old_m); self._v.copy_(old_v)
            for (_, p, off, n, shp) in model._ptable:
                self.state[p] = {"step": torch.tensor(float(self._t)), "exp_avg": self._m[off:off + n].view(shp),
                                 "exp_avg_sq": self._v[off:off + n].view(shp)}
        if self._capturable and (self._step_dev is None or self._step_dev.device != flat.device):
            # the device-side step counter is created HERE, outside step(): the first step() may run inside torch.cuda.graph, and
            # an allocation + fill captured there would reset the counter on every replay
            self._step_dev = torch.full((1,), float(self._t), dtype=torch.float64, device=flat.device)
        if self._guarded and (self._guard is None or self._guard.device != flat.device):
            # mmvae_adam_step_guarded's state {step count, norm, skipped steps, norm^2 accumulator}, then its sum's scratch; created
            # here for the same reason.  The step count is a view of it, so resume and state_dict() treat it as they treat _step_dev.
            old = self._guard
            self._guard = torch.zeros(4 + SUM_PARTIALS, dtype=torch.float64, device=flat.device)
            if old is not None:
                self._guard[:3].copy_(old[:3])
            else:
                self._guard[0] = float(self._t)
            self._step_dev = self._guard[0:1]
        return self._m, self._v

    def prepare_capture(self):
        """Allocate the moments and the device-side step counter (and the guard's state) now (call once before capturing a step in a
        HIP graph)."""
        model = self._model()
        model._ensure_flat()
        self._moments(model)
        return self

    def _set_host_step(self):
        for st_ in self.state.values():
            st_["step"] = torch.tensor(float(self._t))

    def _sync_step_from_device(self):
        """capturable: the authoritative step count lives on the device (graph replays advance it without the host seeing
        a step() call); read it back -- one small D2H copy -- whenever the host needs it (state_dict, resume)."""
        if (self._capturable or self._guarded) and self._step_dev is not None:
            self._t = int(round(float(self._step_dev.item())))
            self._set_host_step()

    def state_dict(self):
        self._sync_step_from_device()
        return super().state_dict()

    def _guard_state(self):
        if not self._guarded:
            raise MmvaeError("grad_norm / skipped_steps need FusedAdam(max_grad_norm=...) or FusedAdam(skip_nonfinite=True)")
        if self._guard is None:
            self.prepare_capture()
        return self._guard

    @property
    def grad_norm(self):
        """Total gradient norm of the last step() (after the data-parallel scale, before clipping; inf / NaN after a skipped step):
        a 0-dim f64 device tensor viewing the guard's state, read without a synchronisation."""
        return self._guard_state()[1]

    @property
    def skipped_steps(self):
        """Number of steps skipped so far for a non-finite gradient (one small D2H copy)."""
        return int(round(float(self._guard_state()[2].item())))

    @staticmethod
    def _flat_grads(model):
        first, last = model._ptable[0], model._ptable[-1]
        if first.param.grad is None:
            return None
        for G in model._G:
            if G is not None and first.param.grad.data_ptr() == G.data_ptr() and last.param.grad is not None and \
                    last.param.grad.data_ptr() == G.data_ptr() + last.offset * 4:
                return G
        G = model._grad_target()                     # slow path: gradients live elsewhere -> gather
        for (_, p, off, n, _) in model._ptable:
            if p.grad is None:
                G[off:off + n].zero_()
            else:
                G[off:off + n].copy_(p.grad.reshape(-1))
        return G

    @torch.no_grad()
    def load_flat_state(self, state_dict):
        """Resume from a torch.optim.Adam-layout state_dict (this class's own or the reference's ``optimizer`` entry)."""
        model = self._model()
        model._ensure_flat()
        m, v = self._moments(model)
        st = state_dict.get("state", {})
        for i, (_, p, off, n, shp) in enumerate(model._ptable):
            e = st.get(i)
            if e is None:
                continue
            m[off:off + n].copy_(e["exp_avg"].reshape(-1).to(m.device))
            v[off:off + n].copy_(e["exp_avg_sq"].reshape(-1).to(v.device))
            self._t = int(float(e["step"]))
        self._set_host_step()
        if self._step_dev is not None:            # capturable: the device counter follows the restored count (in place: a captured
            self._step_dev.fill_(float(self._t))  # graph keeps pointing at this tensor)
        if state_dict.get("param_groups"):
            g = state_dict["param_groups"][0]
            for k in ("lr", "betas", "eps", "weight_decay"):
                if k in g:
                    self.param_groups[0][k] = g[k]

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        model = self._model()
        model._ensure_flat()
        G = self._flat_grads(model)
        if G is None:
            return loss
        scale = model._sync.finish(G) if model._sync is not None else 1.0
        g =self.param_groups[0]
        m, v = self._moments(model)
        self._t += 1
        b1, b2 = g["betas"]
        # what the three kernels share: buffers, size and Adam's hyper-parameters
        common = (ptr(model._flat), ptr(G), ptr(m), ptr(v), model._n_params, float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                  float(g["weight_decay"]))
        # the device-side step count (guarded, capturable): state[p]["step"] is refreshed from it in state_dict() -- under graph replay
        # the host does not see the steps, and a skipped step does not advance it
        if self._guarded:
            check(lib().mmvae_adam_step_guarded(*common, ptr(self._guard), self._guard.data_ptr() + 32, scale, self._max_norm, cur_stream()),
                  "mmvae_adam_step_guarded")
        elif self._capturable:
            check(lib().mmvae_adam_step_dev(*common, ptr(self._step_dev), scale, cur_stream()), "mmvae_adam_step_dev")
        else:
            bc1, bc2s = 1.0 - b1 ** self._t, math.sqrt(1.0 - b2 ** self._t)
            check(lib().mmvae_adam_step(*common, bc1, bc2s, scale, cur_stream()), "mmvae_adam_step")
            self._set_host_step()
        return loss
