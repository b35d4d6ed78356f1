"""MI355X-native conv-VAE train path (drop-in for moving-mnist-vae's model.VAE / main.train).

The directory name carries a hyphen (it mirrors the upstream repository name), so import it
with ``importlib.import_module("moving-mnist-vae_amd")``.  Importing the package does not need
a GPU; constructing / running the model does, and fails loudly when the HIP library is absent.
"""
from .data import (GeneratedClips, MovingMNISTClips, QuantiserFit, choose_transformer, clips_from_npz_array, fit_quantiser,  # noqa: F401
                   generate_batch, generate_clips, load_idx_images, load_kmeans_file, pixel_histogram, quantise_frames,
                   resize_frames, resize_quantise_frames, save_kmeans_file, save_moving_mnist_files, velocity_table)
from .decomposition import elbo_decomposition, latent_penalty, make_latent_penalty, posterior_mixture  # noqa: F401
from .main import (checkpoint_variant, evaluate, generate, generate_only_pixelcnn, latent_stats, load_checkpoint, save_checkpoint,  # noqa: F401
                   select_model, train)
from .monitor import TensorHistograms, make_histogram_callback, tensor_histograms  # noqa: F401
from .neighbours import nearest_frames  # noqa: F401
from .panels import (column, gray_lut, latent_slide, make_plot_callback, neighbour_sheet, plot_neighbours, plot_pixelcnn, plot_pixelvae,  # noqa: F401
                     plot_vae, render_sheet, sample_from_reconstruction, scatter_panel, scatter_plot, scatter_tone, write_png_gray)
from .quality import frame_quality, reconstruction_quality  # noqa: F401
from .samples import ball_counts, cross_neighbours, sample_frames, sample_quality, sample_quality_to_host  # noqa: F401


def __getattr__(name):
    if name in ("VAE", "FusedAdam", "GradSync", "Communicator", "MmvaeError", "draw_labels", "decode_labels"):
        from . import model as _m
        return getattr(_m, name)
    raise AttributeError(name)
