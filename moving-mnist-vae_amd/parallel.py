"""Data-parallel training: the library's own RCCL communicator and the two-bucket gradient exchange."""
import ctypes
import importlib
import os

import torch

from ._lib import MmvaeError, check, cur_stream, ptr


def lib():      # under the name callers know it by: these classes are used as model.GradSync, and a stand-in library is put at model.lib
    return importlib.import_module(__package__ + ".model").lib()


class Communicator:
    """RCCL communicator behind the C ABI (``mmvae_comm_*``, include/mmvae.h): in-place f32 sum all-reduce enqueued on a HIP
    stream by the library itself.  ``Communicator.from_torch_distributed()`` builds one next to an initialised
    torch.distributed job (the 128-byte RCCL id travels through the job's own object broadcast)."""

    def __init__(self, world, rank, unique_id: bytes):
        self._h = ctypes.c_void_p()
        self.world, self.rank = int(world), int(rank)
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        check(lib().mmvae_comm_init(ctypes.byref(self._h), self.world, self.rank, ctypes.cast(buf, ctypes.c_void_p)), "mmvae_comm_init")

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        check(lib().mmvae_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p)), "mmvae_comm_unique_id")
        return buf.raw

    @classmethod
    def from_torch_distributed(cls, group=None):
        import torch.distributed as dist
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        box = [cls.unique_id() if rank == 0 else None]
        if world > 1:
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        return cls(world, rank, box[0])

    def all_reduce_(self, t: torch.Tensor, stream=None):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise MmvaeError("Communicator.all_reduce_ expects a contiguous f32 GPU tensor")
        st = cur_stream() if stream is None else stream
        check(lib().mmvae_comm_allreduce(self._h, ptr(t), t.numel(), st), "mmvae_comm_allreduce")
        return t

    def destroy(self):
        h, self._h = self._h, None
        if h:
            check(lib().mmvae_comm_destroy(h), "mmvae_comm_destroy")

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class GradSync:
    """Data-parallel gradient exchange: one process per GPU, sum-all-reduce over RCCL/xGMI of the flat gradient in two
    buckets -- decoder gradients are complete first and are reduced while the encoder backward still runs -- and 1/world
    scaling folded into Adam.  ``comm="torch"`` (default) issues the buckets through torch.distributed (backend "nccl" = RCCL;
    "gloo" in the CPU tests); ``comm="rccl"`` (or a ``Communicator``) issues them through this library's own RCCL communicator
    (``mmvae_comm_allreduce``) from a communication stream, with no Python in the SyncBN path.
    BatchNorm statistics stay per-rank (like DistributedDataParallel's default) unless sync_bn=True: then every train-mode
    BatchNorm normalises with the statistics of the GLOBAL batch (the reference's semantics at the global batch size):
    the library sums its per-channel partial sums over the ranks -- one small all-reduce per BatchNorm and direction,
    stream-ordered (in-stream RCCL call with a Communicator, host callback into torch.distributed otherwise), equal shards per
    rank assumed."""

    def __init__(self, model, group=None, broadcast=True, sync_bn=False, comm=None):
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.world = dist.get_world_size(group)
        self.handles, self.reduced = [], []                    # async torch.distributed handles, (lo, hi) of the buckets announced
        self._comm_stream, self._comm_pending = None, False
        model._sync = self
        self._cb = None
        comm = comm if comm is not None else os.environ.get("MMVAE_COMM", "torch")
        if isinstance(comm, str):
            if comm not in ("torch", "rccl"):
                raise ValueError("comm must be 'torch', 'rccl' or a Communicator")
            comm = Communicator.from_torch_distributed(group) if comm == "rccl" else None
        self.comm = comm
        self._bn_comms = ()
        if sync_bn and self.comm is not None:
            # the SyncBN rows get communicators of their own, one per stream they are issued from (caller's stream, library side
            # stream): RCCL orders the collectives of ONE communicator, so sharing the bucket communicator would queue the encoder's
            # rows behind the decoder's gradient bucket and lean on RCCL serialising concurrent streams (mmvae.h)
            self._bn_comms = (Communicator.from_torch_distributed(group), Communicator.from_torch_distributed(group))
            check(lib().mmvae_net_set_sync_bn_comm2(model._h, self._bn_comms[0]._h, self._bn_comms[1]._h), "mmvae_net_set_sync_bn_comm2")
        elif sync_bn:
            model._ensure_flat()

            def _allreduce(buf, n, stream, user):
                try:
                    t = model._ws_view(buf, n)
                    st = torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream(t.device)
                    with torch.cuda.stream(st):
                        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
                    return 0
                except Exception:  # noqa: BLE001 -- must not unwind through the C frames
                    import traceback
                    traceback.print_exc()
                    return -1

            self._cb = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p)(_allreduce)
            check(lib().mmvae_net_set_sync_bn(model._h, ctypes.cast(self._cb, ctypes.c_void_p), None, self.world), "mmvae_net_set_sync_bn")
        if broadcast and self.world > 1:
            model._ensure_flat() if model._flat.is_cuda else None
            dist.broadcast(model._flat, 0, group=group)
            dist.broadcast(model._bnf, 0, group=group)

    def _all_reduce(self, t, async_op):
        """One sum all-reduce on the CURRENT stream context; async_op: through torch.distributed, leave the handle for finish()."""
        if self.comm is not None:
            self.comm.all_reduce_(t)
        else:
            h = self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group, async_op=async_op)
            if async_op:
                self.handles.append(h)

    def bucket_ready(self, G, lo, hi, side_of=None):
        """Start the all-reduce of G[lo:hi].  side_of: the model whose library side stream still carries part of this bucket
        (deferred join): the collective is then issued from a communication stream that waits for the caller's stream and for
        that side stream, and the caller's stream goes on with the encoder backward."""
        if self.world == 1:
            return
        if side_of is None and self.comm is None:
            self._all_reduce(G[lo:hi], True)
        else:
            if self._comm_stream is None:
                self._comm_stream = torch.cuda.Stream(device=G.device)
            cs = self._comm_stream
            cs.wait_stream(torch.cuda.current_stream(G.device))
            with torch.cuda.stream(cs):
                if side_of is not None:
                    check(lib().mmvae_net_join(side_of._h, cs.cuda_stream), "mmvae_net_join")
                self._all_reduce(G[lo:hi], True)
            self._comm_pending = True
        self.reduced.append((lo, hi))

    def reduce_step_scalars(self, groups):
        """Logged scalars of data-parallel training: ONE all-reduce of the stacked (steps, 4) device tensor, mean over
        ranks.  `groups` are the _StepScalars of the steps not yet read back."""
        if self.world == 1 or not groups:
            return
        stacked = torch.stack([g.ready() for g in groups]).contiguous()
        self._all_reduce(stacked, False)
        for g, v in zip(groups, (stacked / self.world).tolist()):
            g.vals = v

    def finish(self, G):
        """Wait for the in-flight buckets; returns the factor Adam applies to the summed gradient."""
        for h in self.handles:
            h.wait()
        if self._comm_pending:                                   # buckets issued from the communication stream
            torch.cuda.current_stream(G.device).wait_stream(self._comm_stream)
            self._comm_pending = False
        covered = sorted(self.reduced)
        self.handles, self.reduced = [], []
        if self.world > 1:
            pos = 0
            for lo, hi in covered:
                if lo > pos:
                    self._all_reduce(G[pos:lo], False)
                pos = max(pos, hi)
            if pos < G.numel():
                self._all_reduce(G[pos:], False)
        return 1.0 / self.world
