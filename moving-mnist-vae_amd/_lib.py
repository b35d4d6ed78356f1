"""ctypes binding of libmmvae_hip.so (the C ABI declared in include/mmvae.h).

There is no CPU fallback: if the library is missing the product path raises, loudly.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MMVAE_LIB_PATH: developer A/B runs of two builds on one box; the product always loads the in-tree library)
LIB_PATH = os.environ.get("MMVAE_LIB_PATH") or os.path.join(_HERE, "libmmvae_hip.so")
_lib = None
ABI_VERSION = 3            # MMVAE_ABI_VERSION of include/mmvae.h
SUM_PARTIALS = 1025        # MMVAE_SUM_PARTIALS: f64 scratch of each loss sum (mmvae_kl_fwd_ex, ...)
BN_SCRATCH_BYTES = 16 << 20     # MMVAE_BN_SCRATCH_BYTES: mmvae_batchnorm_fwd / _bwd, mmvae_stem_bwd
STEM_SCRATCH_BYTES = 12800      # MMVAE_STEM_SCRATCH_BYTES: packed weights of mmvae_stem_fwd

P = c_void_p

# name -> (restype, argtypes); mirrors include/mmvae.h one to one (checked by tests/test_capi_cpu.py)
PROTOTYPES = {
    "mmvae_abi_version": (c_int, []),
    "mmvae_last_error": (c_char_p, []),
    "mmvae_net_create": (c_int, [POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, c_int]),
    "mmvae_net_create_ex": (c_int, [POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "mmvae_net_destroy": (None, [P]),
    "mmvae_net_sizes": (c_int, [P, POINTER(c_int64), POINTER(c_int64), POINTER(c_int32), POINTER(c_int64), POINTER(c_int32)]),
    "mmvae_net_num_entries": (c_int, [P]),
    "mmvae_net_entry": (c_int, [P, c_int, c_char_p, c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int64)]),
    "mmvae_net_workspace_bytes": (c_size_t, [P, c_int]),
    "mmvae_encoder_fwd": (c_int, [P, c_int, P, P, P, P, P, c_size_t, P, P, c_int, P]),
    "mmvae_net_stage_labels": (c_int, [P, c_int, P, c_int, c_float, c_float, P, P, c_size_t, P]),
    "mmvae_encoder_fwd_staged": (c_int, [P, c_int, P, P, P, P, P, c_size_t, P, P, c_int, P]),
    "mmvae_encoder_bwd": (c_int, [P, c_int, P, P, P, P, P, c_size_t, P]),
    "mmvae_decoder_fwd": (c_int, [P, c_int, P, P, P, P, P, c_size_t, P, c_int, P]),
    "mmvae_decoder_bwd": (c_int, [P, c_int, P, P, P, P, c_size_t, P, P]),
    "mmvae_decoder_bwd_gauss": (c_int, [P, c_int, P, c_float, c_float, P, P, P, P, c_size_t, P, P]),
    "mmvae_net_defer_join": (c_int, [P, c_int]),
    "mmvae_net_join": (c_int, [P, P]),
    "mmvae_net_fork": (P, [P, P]),
    "mmvae_net_side_stream": (P, [P]),
    "mmvae_net_set_join_grad": (c_int, [P, c_int]),
    "mmvae_net_describe_routes": (c_int, [P, c_int, c_char_p, c_int]),
    "mmvae_net_set_sync_bn": (c_int, [P, P, P, c_int]),
    "mmvae_rsample_fwd": (c_int, [P, P, P, P, c_int64, P]),
    "mmvae_rsample_bwd": (c_int, [P, P, P, P, P, c_int64, P]),
    "mmvae_kl_fwd": (c_int, [P, P, c_int64, P, P]),
    "mmvae_kl_fwd_ex": (c_int, [P, P, c_int64, P, P, P]),
    "mmvae_kl_bwd": (c_int, [P, P, c_float, P, P, P, c_int64, P]),
    "mmvae_gauss_nll_fwd": (c_int, [P, P, c_int64, c_float, P, P]),
    "mmvae_gauss_nll_fwd_ex": (c_int, [P, P, c_int64, c_float, P, P, P]),
    "mmvae_gauss_nll_bwd": (c_int, [P, P, c_int64, c_float, c_float, P, P, P]),
    "mmvae_ce_fwd": (c_int, [P, P, P, c_int, c_int, c_int, P, P]),
    "mmvae_ce_fwd_ex": (c_int, [P, P, P, c_int, c_int, c_int, P, P, P]),
    "mmvae_ce_bwd": (c_int, [P, P, P, c_int, c_int, c_int, c_float, P, P, P]),
    "mmvae_mmd_fwd": (c_int, [P, P, c_int, c_int, P, P, P]),
    "mmvae_mmd_fwd_ex": (c_int, [P, P, c_int, c_int, P, P, P, P]),
    "mmvae_mmd_bwd": (c_int, [P, P, c_int, c_int, c_float, P, P, P]),
    "mmvae_loss_finish": (c_int, [P, P, c_float, c_float, c_float, c_float, P]),
    "mmvae_gauss_nll_per_image": (c_int, [P, P, c_int, c_int64, c_float, P, P]),
    "mmvae_ce_per_image": (c_int, [P, P, P, c_int, c_int, c_int, P, P]),
    "mmvae_kl_per_image": (c_int, [P, P, c_int, c_int, P, P]),
    "mmvae_latent_logratio": (c_int, [P, P, P, c_int, c_int, P, P]),
    "mmvae_iw_bound": (c_int, [P, P, c_int, c_int, P, P]),
    "mmvae_normalise_labels": (c_int, [P, c_int64, c_float, c_float, P, P]),
    "mmvae_quantise_normalise": (c_int, [P, c_int64, P, c_int, c_float, c_float, P, P, P]),
    "mmvae_u8_histogram": (c_int, [P, c_int64, P, c_int64, P, P]),
    "mmvae_kmeans1d_fit": (c_int, [P, c_int, P, P]),
    "mmvae_quantiser_stats": (c_int, [P, P, c_int, P, P, P, P]),
    "mmvae_resample_coeffs": (c_int, [c_int, c_int, POINTER(c_int), P, P]),
    "mmvae_resize_quantise_normalise": (c_int, [P, c_int64, P, c_int, c_int64, c_int, c_int, c_int, c_int, P, P, c_int, P, P, c_int, P, c_int,
                                                c_float, c_float, P, P, P, P]),
    "mmvae_generate_clips": (c_int, [P, c_int64, c_int, P, c_uint64, c_int64, c_int64, c_int, c_int, c_int, P, c_int, c_float, c_float, P, P, P, P]),
    "mmvae_logits_to_labels": (c_int, [P, c_int, c_int, c_int, c_int, P, P, P]),
    "mmvae_panel_sheet": (c_int, [P, c_int, c_int, c_int, P, P]),
    "mmvae_frame_quality": (c_int, [P, P, c_int, c_int, P, P]),
    "mmvae_scatter_panel": (c_int, [P, c_int64, c_int, c_int, c_int, P, c_int, c_int, P, P, c_int64, P]),
    "mmvae_latent_stats": (c_int, [P, P, P, c_int, c_int, c_int, P, P]),
    "mmvae_posterior_mixture_scratch_bytes": (c_size_t, [c_int, c_int, c_int]),
    "mmvae_posterior_mixture": (c_int, [P, c_int, P, P, c_int, c_int, P, P, P, c_size_t, P]),
    "mmvae_posterior_mixture_bwd_scratch_bytes": (c_size_t, [c_int, c_int, c_int]),
    "mmvae_posterior_mixture_bwd": (c_int, [P, c_int, P, P, c_int, c_int, P, P, P, P, P, P, P, P, c_size_t, P]),
    "mmvae_nearest_frames_scratch_bytes": (c_size_t, [c_int, c_int64, c_int, c_int]),
    "mmvae_nearest_frames": (c_int, [P, c_int, P, c_int64, c_int, P, c_int, P, P, P, c_size_t, P]),
    "mmvae_knn_cross_scratch_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int, c_int]),
    "mmvae_knn_cross": (c_int, [P, c_int64, P, c_int64, c_int, c_int, c_int, P, P, P, P, P, c_size_t, P]),
    "mmvae_tensor_hist_chunks": (c_int64, [P, c_int, c_int64, P, c_int64]),
    "mmvae_tensor_hist_scratch_bytes": (c_size_t, [c_int, c_int64]),
    "mmvae_tensor_hist": (c_int, [P, c_int64, P, P, c_int, P, P, c_int64, P, P, P, P, P, c_size_t, P]),
    "mmvae_adam_step": (c_int, [P, P, P, P, c_int64, c_float, c_float, c_float, c_float, c_float, c_float, c_float, c_float, P]),
    "mmvae_adam_step_dev": (c_int, [P, P, P, P, c_int64, c_float, c_float, c_float, c_float, c_float, P, c_float, P]),
    "mmvae_grad_norm_sq": (c_int, [P, c_int64, c_float, P, P, P]),
    "mmvae_adam_step_guarded": (c_int, [P, P, P, P, c_int64, c_float, c_float, c_float, c_float, c_float, P, P, c_float, c_float, P]),
    "mmvae_conv2d_fwd": (c_int, [c_int, c_int, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P, P]),
    "mmvae_conv2d_dgrad": (c_int, [c_int, c_int, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    "mmvae_conv2d_dgrad_ex": (c_int, [c_int, c_int, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P]),
    "mmvae_conv2d_wgrad": (c_int, [c_int, c_int, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P]),
    "mmvae_conv2d_wgrad_pair": (c_int, [c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P]),
    "mmvae_conv2d_fwd_pair": (c_int, [c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P, P, P]),
    "mmvae_conv2d_dgrad_bn_sums": (c_int, [c_int, P, P, P, P, P, P, P, c_int, c_int, P, P]),
    "mmvae_stem_bwd_dg": (c_int, [c_int, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, c_int, c_int, P, P]),
    "mmvae_rbf_kernel": (c_int, [P, P, c_int, c_int, c_int, P, P]),
    "mmvae_comm_unique_id": (c_int, [P]),
    "mmvae_comm_init": (c_int, [POINTER(c_void_p), c_int, c_int, P]),
    "mmvae_comm_allreduce": (c_int, [P, P, c_int64, P]),
    "mmvae_comm_destroy": (c_int, [P]),
    "mmvae_net_set_sync_bn_comm": (c_int, [P, P]),
    "mmvae_net_set_sync_bn_comm2": (c_int, [P, P, P]),
    "mmvae_convT_bwd_fused": (c_int, [c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P, P, P, P, P]),
    "mmvae_batchnorm_fwd": (c_int, [c_int, P, c_int64, c_int, P, P, P, P, P, c_float, c_float, c_int, P, P, P, P, P]),
    "mmvae_batchnorm_bwd": (c_int, [c_int, P, P, P, c_int64, c_int, P, P, P, P, P, P, P, P]),
    "mmvae_stem_fwd": (c_int, [c_int, P, P, P, c_int, c_int, P, P, P]),
    "mmvae_stem_bwd": (c_int, [c_int, P, P, P, P, P, P, P, P, P, P, P, P, c_int, c_int, P, P]),
    "mmvae_tail_join_fwd": (c_int, [c_int, P, P, P, P, P, P, P, P, P, P, c_int, c_int, c_int, P]),
    "mmvae_tail_join_fwd_stream": (c_int, [c_int, P, P, P, P, P, P, P, P, P, P, c_int, c_int, c_int, P]),
    "mmvae_tail_join_bwd_reduce": (c_int, [c_int, P, P, c_int, P, P, P, P, P, P, P, P, c_int, c_int, c_int, P]),
    "mmvae_tail_join_bwd_apply": (c_int, [c_int, P, P, c_int, P, P, P, P, P, P, P, P, P, P, P, P, P, P, c_int, c_int, c_int, P]),
    "mmvae_upblock_bwd_fused": (c_int, [P] * 27 + [c_int, P, P]),
    "mmvae_join_conv1x1_fwd": (c_int, [P, P, P, P, P, P, P, c_int, P, P, P, c_int64, P, P]),
    "mmvae_conv1x1_bwd_fused": (c_int, [P] * 13 + [c_int64, P, P]),
    "mmvae_upblock_tail_fwd": (c_int, [P] * 16 + [c_int, P, P]),
    "mmvae_upblock_tail_fwd_store": (c_int, [P] * 18 + [c_int, P, P]),
    "mmvae_convT4_stats": (c_int, [c_int, P, P, P, P, P, c_int, c_int, P, P]),
    "mmvae_pixelcnn_create": (c_int, [POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int]),
    "mmvae_pixelcnn_destroy": (None, [P]),
    "mmvae_pixelcnn_num_params": (c_int64, [P]),
    "mmvae_pixelcnn_workspace_bytes": (c_size_t, [P, c_int, c_int]),
    "mmvae_pixelcnn_fwd": (c_int, [P, c_int, c_int, P, P, P, c_size_t, P, P]),
    "mmvae_pixelcnn_bwd": (c_int, [P, c_int, c_int, P, P, P, P, P, c_size_t, P, P]),
    "mmvae_pixelcnn_sample_workspace_bytes": (c_size_t, [P, c_int, c_int]),
    "mmvae_pixelcnn_sample": (c_int, [P, c_int, c_int, P, c_int, P, c_int, P, c_float, c_float, P, P, c_size_t, P, P, P, P]),
    "mmvae_convert": (c_int, [c_int, c_int, P, P, c_int64, P]),
}


class MmvaeError(RuntimeError):
    pass


PICK_ARGMAX, PICK_SAMPLE = 0, 1                                  # MMVAE_PICK_*
PANEL_LABELS_U8, PANEL_LABELS_I64, PANEL_LOGITS_ARGMAX, PANEL_LOGITS_SAMPLE, PANEL_IMAGE_F32 = range(5)      # MMVAE_PANEL_*
PANEL_MAX_COLS, PANEL_MAX_Q, PANEL_MAX_S = 8, 16, 64
FRAME_BYTES_U8, FRAME_MIN_S, FRAME_MAX_S = 5, 11, 64             # MMVAE_FRAME_BYTES_U8; the sides mmvae_frame_quality accepts
SCATTER_MAX_SIDE, SCATTER_MIN_RADIUS16, SCATTER_MAX_RADIUS16 = 512, 12, 128      # mmvae_scatter_panel's accepted ranges
LATENT_STATS_ROWS, LATENT_STATS_MAX_D = 6, 512                                   # mmvae_latent_stats: rows of acc, widest latent
MIXTURE_MAX_D, MIXTURE_MAX_N, MIXTURE_MIN_CHUNK = 512, 1 << 20, 64           # mmvae_posterior_mixture: widest latent, most samples / bank rows, fewest rows of a bank chunk
MIXTURE_BWD_MAX_N = 16384                                                        # mmvae_posterior_mixture_bwd: most samples / bank rows
NEAREST_MAX_M, NEAREST_MAX_K, NEAREST_MAX_D = 64, 8, 16384                       # mmvae_nearest_frames: queries, neighbours, bytes per plane
KNN_CROSS_MAX_N, KNN_CROSS_MAX_K, KNN_CROSS_MAX_D = 1 << 20, 8, 16384                # mmvae_knn_cross: rows a side, neighbours, bytes per row
KNN_CROSS_TILE, KNN_CROSS_TARGET_BLOCKS, KNN_CROSS_MAX_RANGES = 128, 2048, 128       # its block tile and column split (knn_cross.hip: make_plan)
CLIPGEN_MAX_G, CLIPGEN_MAX_T, CLIPGEN_MAX_K, CLIPGEN_MAX_D, CLIPGEN_DIRECTIONS = 32, 32, 4, 1 << 24, 4096       # MMVAE_CLIPGEN_*


class PanelCol(ctypes.Structure):
    """mmvae_panel_col of include/mmvae.h: one column of mmvae_panel_sheet (the pointers are device pointers)."""
    _fields_ = [("kind", c_int32), ("src", c_void_p), ("Q", c_int32), ("uniforms", c_void_p), ("lut", c_void_p), ("lo", c_float),
                ("hi", c_float)]


def lib():
    """Load (once) and return the shared library.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MmvaeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C moving-mnist-vae_amd/csrc`). "
            "There is no CPU fallback for the product path.")
    l = ctypes.CDLL(LIB_PATH)
    # include/mmvae.h: "bindings check mmvae_abi_version() at load time" -- a stale or foreign build would be called with shifted
    # arguments.  Checked before the table is bound: a stale build may lack a symbol, and it should get this message, not an AttributeError.
    l.mmvae_abi_version.restype, l.mmvae_abi_version.argtypes = c_int, []
    got = l.mmvae_abi_version()
    if got != ABI_VERSION:
        raise MmvaeError(f"{LIB_PATH} has C ABI version {got}, this binding expects {ABI_VERSION}: rebuild the library "
                         "(make -C moving-mnist-vae_amd/csrc)")
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(l, name, None)
        if fn is None:            # (a build of the same ABI version from before an export was added)
            raise MmvaeError(f"{LIB_PATH} lacks {name}: rebuild the library (make -C moving-mnist-vae_amd/csrc)")
        fn.restype = res
        fn.argtypes = args
    _lib = l
    return l


def knn_cross_ranges(Na: int, Nb: int) -> int:
    """Contiguous column ranges mmvae_knn_cross cuts ``b`` into at this shape (make_plan of knn_cross.hip); every row of ``a`` gets two
    partial results per range, merged by key."""
    tiles = lambda n: (n + KNN_CROSS_TILE - 1) // KNN_CROSS_TILE
    want = (KNN_CROSS_TARGET_BLOCKS + tiles(Na) - 1) // tiles(Na)
    return min(want, KNN_CROSS_MAX_RANGES, tiles(Nb))


def build_hash() -> str:
    """Short hash of the kernel sources the library was built from (csrc/ + the public header); keys the committed PMC
    tables under profiles/ to the build they were measured on."""
    import hashlib
    h = hashlib.sha1()
    csrc = os.path.join(_HERE, "csrc")
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".inc", ".cpp", ".hpp")))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "mmvae.h"))
    for f in files:
        with open(f, "rb") as fh:
            h.update(os.path.basename(f).encode() + b"\0" + fh.read())
    return h.hexdigest()[:12]


def check(rc: int, what: str) -> int:
    if rc < 0:
        msg = lib().mmvae_last_error()
        raise MmvaeError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
    return rc


def cur_stream():
    """The current HIP stream's handle, as the C ABI takes it."""
    return torch.cuda.current_stream().cuda_stream


def call(name: str, device, *args) -> int:
    """One launch off the train step: ``lib().<name>(*args, stream)`` on ``device``'s current stream, return code checked."""
    with torch.cuda.device(device):
        return check(getattr(lib(), name)(*args, cur_stream()), name)


def ptr(t):
    """Device/host pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()
