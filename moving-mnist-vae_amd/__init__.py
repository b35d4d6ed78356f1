"""MI355X-native conv-VAE train path (drop-in for moving-mnist-vae's model.VAE / main.train).

The directory name carries a hyphen (it mirrors the upstream repository name), so import it
with ``importlib.import_module("moving-mnist-vae_amd")``.  Importing the package does not need
a GPU; constructing / running the model does, and fails loudly when the HIP library is absent.
"""
from .main import (MovingMNISTClips, QuantiserFit, checkpoint_variant, choose_transformer, clips_from_npz_array, column, evaluate, fit_quantiser,  # noqa: F401
                   generate, generate_only_pixelcnn, gray_lut, latent_slide, latent_stats, load_checkpoint, load_kmeans_file,
                   make_plot_callback, pixel_histogram, plot_pixelcnn, plot_pixelvae, plot_vae, quantise_frames, render_sheet,
                   resize_frames, resize_quantise_frames, sample_from_reconstruction, save_checkpoint, save_kmeans_file, scatter_panel,
                   scatter_plot, scatter_tone, select_model, train, write_png_gray)


def __getattr__(name):
    if name in ("VAE", "FusedAdam", "GradSync", "Communicator", "MmvaeError", "draw_labels", "decode_labels"):
        from . import model as _m
        return getattr(_m, name)
    raise AttributeError(name)
