"""MI355X-native conv-VAE train path (drop-in for moving-mnist-vae's model.VAE / main.train).

The directory name carries a hyphen (it mirrors the upstream repository name), so import it
with ``importlib.import_module("moving-mnist-vae_amd")``.  Importing the package does not need
a GPU; constructing / running the model does, and fails loudly when the HIP library is absent.
"""
from .main import (MovingMNISTClips, QuantiserFit, checkpoint_variant, choose_transformer, clips_from_npz_array, evaluate, fit_quantiser, generate,  # noqa: F401
                   generate_only_pixelcnn, load_checkpoint, load_kmeans_file, pixel_histogram, quantise_frames, resize_frames,
                   resize_quantise_frames, save_checkpoint, save_kmeans_file, select_model, train)


def __getattr__(name):
    if name in ("VAE", "FusedAdam", "GradSync", "Communicator", "MmvaeError", "draw_labels"):
        from . import model as _m
        return getattr(_m, name)
    raise AttributeError(name)
