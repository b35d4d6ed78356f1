"""GPU: the fused resize + quantise kernel (mmvae_resize_quantise_normalise) and its Python surface -- resize_frames,
resize_quantise_frames, MovingMNISTClips(image_size=...), choose_transformer -- against the integer restatement of PIL's resize in
tests/resize_ref.py (and PIL's own bytes in tests/golden/pil_resize.npz).  Every comparison is exact: the bytes are integer sums,
the labels a table lookup, the image one f32 division by a constant."""
import importlib
import types

import numpy as np
import pytest
import torch

import resize_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

GRID_CAP = 2048                        # blocks of one launch (resize.hip): more planes than this make a block take several
GRID_TIE_CENTRES = [0.0, 2 / 255.0, 4 / 255.0]


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


@pytest.fixture(scope="module")
def clips_np():
    """(6, 20, 64, 64) uint8 in the npz file's (N, C, W, H) layout: mostly black with bright strokes, like the dataset."""
    rng = np.random.default_rng(42)
    a = rng.integers(0, 256, size=(6, 20, 64, 64), dtype=np.uint8)
    a[rng.random(a.shape) < 0.7] = 0
    return a


@pytest.fixture(scope="module")
def clips_ref32(clips_np):
    """The resized bytes of those clips at 32, in the (N, C, H, W) orientation the loader works on; computed once, read-only."""
    out = R.resize(np.ascontiguousarray(clips_np.transpose(0, 1, 3, 2)), 32)
    out.setflags(write=False)
    return out


def _centres(name):
    return GRID_TIE_CENTRES if name == "tie" else load_golden(name)["centres"]


def _random(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _image_of(pkg, resized_np, centres, mean, std):
    """The image quantise_frames makes of these bytes: the kernel the fused call has to equal bit for bit."""
    return pkg.quantise_frames(torch.from_numpy(np.ascontiguousarray(resized_np)).cuda(), centres, mean, std)[1]


def _raw(L, pkg, frames, stride, index, per_clip, n, in_hw, out_hw, centres, labels, image, resized, mean=0.0, std=1.0):
    """The C entry point itself, on the caller's outputs."""
    M = importlib.import_module("moving-mnist-vae_amd.data")
    hb, hc, hk = M._resample_tables(in_hw[1], out_hw[1], "cuda:0")
    vb, vc, vk = M._resample_tables(in_hw[0], out_hw[0], "cuda:0")
    rc = L.lib().mmvae_resize_quantise_normalise(L.ptr(frames), stride, L.ptr(index), per_clip, n, in_hw[0], in_hw[1], out_hw[0], out_hw[1],
                                                 L.ptr(hb), L.ptr(hc), hk, L.ptr(vb), L.ptr(vc), vk, L.ptr(centres),
                                                 0 if centres is None else centres.numel(), mean, std, L.ptr(labels), L.ptr(image),
                                                 L.ptr(resized), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


# ---------------------------------------------------------------------------------------------------------------------- the bytes
def test_fixture_cases_equal_pil(pkg):
    g = load_golden("pil_resize")
    for i, (ih, iw, oh, ow) in enumerate(g["cases"].tolist()):
        got = pkg.resize_frames(torch.from_numpy(g[f"x{i}"]).cuda(), (oh, ow))
        if (ih, iw) == (oh, ow):
            assert np.array_equal(got.cpu().numpy(), g[f"x{i}"])
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (3, oh, ow)
        assert np.array_equal(got.cpu().numpy(), g[f"y{i}"]), (ih, iw, oh, ow)


@pytest.mark.parametrize("n", [1, 3])
def test_frame_counts(pkg, n):
    x = _random((n, 64, 64), n)
    assert np.array_equal(pkg.resize_frames(torch.from_numpy(x).cuda(), 32).cpu().numpy(), R.resize(x, 32))


def test_more_planes_than_twice_the_grid(pkg):
    n = 2 * GRID_CAP + 5                                                # a block takes planes b, b + grid, b + 2 grid
    x = _random((n, 16, 10), 7)                                         # 160-byte planes: the 16-byte loads and stores
    x[:, 0, 0] = np.arange(n) % 251                                     # no two neighbouring planes alike
    want = R.resize(x, (6, 6))
    got = pkg.resize_frames(torch.from_numpy(x).cuda(), (6, 6))
    assert np.array_equal(got.cpu().numpy(), want)
    labels, image = pkg.resize_quantise_frames(torch.from_numpy(x).cuda(), (6, 6), _centres("kmeans_q4"), 0.3, 0.7)
    assert np.array_equal(labels.cpu().numpy(), R.label_table(_centres("kmeans_q4"))[want])
    assert torch.equal(image, _image_of(pkg, want, _centres("kmeans_q4"), 0.3, 0.7))


@pytest.mark.parametrize("in_hw,out_hw", [((40, 64), (20, 32)), ((64, 64), (9, 9)), ((64, 64), (63, 63)), ((28, 28), (32, 32)),
                                          ((128, 128), (1, 1)), ((1, 1), (128, 128)), ((128, 128), (127, 127)), ((13, 7), (5, 11))])
def test_sizes(pkg, in_hw, out_hw):
    x = _random((2,) + in_hw, in_hw[0] * 131 + out_hw[1])
    got = pkg.resize_frames(torch.from_numpy(x).cuda(), out_hw)
    assert tuple(got.shape) == (2,) + out_hw
    assert np.array_equal(got.cpu().numpy(), R.resize(x, out_hw))


@pytest.mark.parametrize("size", [32, 9, 63, 33])
def test_saturation_and_rounding(pkg, size):
    yy, xx = np.mgrid[0:64, 0:64]
    planes = np.stack([np.zeros((64, 64)), np.full((64, 64), 255), ((yy + xx) % 2) * 255, (yy * 64 + xx) // 16, xx * 4, 255 - yy * 4]).astype(np.uint8)
    got = pkg.resize_frames(torch.from_numpy(planes).cuda(), size).cpu().numpy()
    assert np.array_equal(got, R.resize(planes, size))
    assert not got[0].any() and (got[1] == 255).all()


# ------------------------------------------------------------------------------------------------------------------- scalar paths
@pytest.mark.parametrize("offset", [1, 3])
def test_views_into_a_larger_buffer(pkg, offset):
    n = 3
    a = _random(n * 4096 + 32, offset)
    view = torch.from_numpy(a).cuda()[offset:offset + n * 4096].view(n, 64, 64)
    assert view.data_ptr() % 16 == offset
    want = R.resize(a[offset:offset + n * 4096].reshape(n, 64, 64), 32)
    assert np.array_equal(pkg.resize_frames(view, 32).cpu().numpy(), want)
    labels, _ = pkg.resize_quantise_frames(view, 32, _centres("kmeans_q2"), 0.0, 1.0)
    assert np.array_equal(labels.cpu().numpy(), R.label_table(_centres("kmeans_q2"))[want])


@pytest.mark.parametrize("stride", [4096 + 16, 4096 + 5])                # 16-byte loads with a gap / byte loads
def test_frame_stride_larger_than_the_plane(pkg, stride):
    n = 4
    a = _random((n, stride), stride)
    view = torch.from_numpy(a).cuda()[:, :4096].view(n, 64, 64)
    assert view.stride(0) == stride and not view.is_contiguous()
    assert np.array_equal(pkg.resize_frames(view, 28).cpu().numpy(), R.resize(a[:, :4096].reshape(n, 64, 64), 28))


def test_unaligned_outputs_and_odd_plane_sizes(pkg, L):
    x = _random((3, 64, 64), 5)
    want = R.resize(x, (7, 9))                                          # 63 pixels a plane: the one-pixel-per-lane stores
    c = torch.tensor(_centres("kmeans_q4"), dtype=torch.float32, device="cuda")
    labels, image = pkg.resize_quantise_frames(torch.from_numpy(x).cuda(), (7, 9), c, 0.5, 2.0)
    lut = R.label_table(_centres("kmeans_q4"))
    assert np.array_equal(labels.cpu().numpy(), lut[want])
    assert torch.equal(image, _image_of(pkg, want, c, 0.5, 2.0))
    # 32 x 32 planes into outputs that start one element into their buffers
    want = R.resize(x, 32)
    lab = torch.full((3 * 1024 + 1,), -5, dtype=torch.int64, device="cuda")
    img = torch.full((3 * 1024 + 1,), -5.0, dtype=torch.float32, device="cuda")
    res = torch.full((3 * 1024 + 1,), 77, dtype=torch.uint8, device="cuda")
    assert _raw(L, pkg, torch.from_numpy(x).cuda(), 4096, None, 1, 3, (64, 64), (32, 32), c, lab[1:], img[1:], res[1:], 0.5, 2.0) == 0
    assert lab[0].item() == -5 and img[0].item() == -5.0 and res[0].item() == 77
    assert np.array_equal(res[1:].cpu().numpy().reshape(3, 32, 32), want)
    assert np.array_equal(lab[1:].cpu().numpy().reshape(3, 32, 32), lut[want])
    assert torch.equal(img[1:].view(3, 32, 32), _image_of(pkg, want, c, 0.5, 2.0))


# ------------------------------------------------------------------------------------------------------------------------- gather
def test_clip_index_gathers_whole_clips(pkg):
    n = 5
    x = _random((n, 3, 28, 28), 9)
    dev = torch.from_numpy(x).cuda()
    lut = R.label_table(_centres("kmeans_q2"))
    for index in ([3, 3, 0, 4, 3], list(range(n - 1, -1, -1)), [2]):
        want = R.resize(x[index], 14)
        got = pkg.resize_frames(dev, 14, clip_index=index)
        assert tuple(got.shape) == (len(index), 3, 14, 14)
        assert np.array_equal(got.cpu().numpy(), want), index
        labels, _ = pkg.resize_quantise_frames(dev, 14, _centres("kmeans_q2"), 0.0, 1.0, clip_index=torch.tensor(index))
        assert np.array_equal(labels.cpu().numpy(), lut[want]), index
    assert np.array_equal(pkg.resize_frames(dev, 28, clip_index=[1, 1]).cpu().numpy(), x[[1, 1]])       # native size: a plain gather
    for bad in ([-1], [n], [0, 1, n + 4]):
        with pytest.raises(IndexError):
            pkg.resize_frames(dev, 14, clip_index=bad)
        with pytest.raises(IndexError):
            pkg.resize_quantise_frames(dev, 14, _centres("kmeans_q2"), 0.0, 1.0, clip_index=bad)


def test_argument_checks(pkg):
    with pytest.raises(ValueError):
        pkg.resize_frames(torch.zeros(2, 8, 8, dtype=torch.uint8), 4)                          # host tensor
    with pytest.raises(ValueError):
        pkg.resize_frames(torch.zeros(2, 8, 8, dtype=torch.float32, device="cuda"), 4)
    with pytest.raises(ValueError):
        pkg.resize_quantise_frames(torch.zeros(2, 8, 8, dtype=torch.int64, device="cuda"), 4, [0.0, 1.0], 0.0, 1.0)
    with pytest.raises(ValueError):
        pkg.resize_quantise_frames(torch.zeros(2, 8, 8, dtype=torch.uint8), 4, [0.0, 1.0], 0.0, 1.0)
    L = importlib.import_module("moving-mnist-vae_amd._lib")
    with pytest.raises(L.MmvaeError):
        pkg.resize_frames(torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda"), 129)
    with pytest.raises(L.MmvaeError):
        pkg.resize_frames(torch.zeros(1, 8, 129, dtype=torch.uint8, device="cuda"), 8)


# ---------------------------------------------------------------------------------------------------------------------- quantiser
@pytest.mark.parametrize("name", ["kmeans_q2", "kmeans_q4", "tie"])
def test_fused_call_equals_resize_then_quantise(pkg, name):
    centres = _centres(name)
    frames = load_golden("kmeans_q2")["frames"]                         # (5, 64, 64); the last one holds all 256 values
    x = torch.from_numpy(np.concatenate([frames, _random((2, 64, 64), 3)])).cuda()
    mean, std = 0.0784, 0.2689
    for size in (32, 56):
        labels, image = pkg.resize_quantise_frames(x, size, centres, mean, std)
        resized = pkg.resize_frames(x, size)
        want_labels, want_image = pkg.quantise_frames(resized, centres, mean, std)
        assert labels.dtype == torch.int64 and image.dtype == torch.float32 and labels.shape == image.shape == resized.shape
        assert torch.equal(labels, want_labels) and torch.equal(image, want_image)
        assert np.array_equal(labels.cpu().numpy(), R.label_table(centres)[R.resize(x.cpu().numpy(), size)])
        assert len(centres) < 3 or len(torch.unique(labels)) == len(centres)


def test_each_output_alone_and_none_at_all(pkg, L):
    x = _random((3, 64, 64), 21)
    dev = torch.from_numpy(x).cuda()
    want = R.resize(x, 32)
    c = torch.tensor(_centres("kmeans_q2"), dtype=torch.float32, device="cuda")
    lut = R.label_table(_centres("kmeans_q2"))
    lab = torch.empty((3, 32, 32), dtype=torch.int64, device="cuda")
    img = torch.empty((3, 32, 32), dtype=torch.float32, device="cuda")
    res = torch.empty((3, 32, 32), dtype=torch.uint8, device="cuda")
    assert _raw(L, pkg, dev, 4096, None, 1, 3, (64, 64), (32, 32), c, lab, None, None) == 0
    assert np.array_equal(lab.cpu().numpy(), lut[want])
    assert _raw(L, pkg, dev, 4096, None, 1, 3, (64, 64), (32, 32), c, None, img, None, 0.25, 0.5) == 0
    assert torch.equal(img, _image_of(pkg, want, c, 0.25, 0.5))
    assert _raw(L, pkg, dev, 4096, None, 1, 3, (64, 64), (32, 32), None, None, None, res) == 0
    assert np.array_equal(res.cpu().numpy(), want)
    assert _raw(L, pkg, dev, 4096, None, 1, 3, (64, 64), (32, 32), c, None, None, None) == -1
    assert b"NULL" in L.lib().mmvae_last_error()
    assert _raw(L, pkg, dev, 4096, None, 1, 3, (64, 64), (32, 32), None, lab, None, None) == -1                # labels need centres


def test_no_frames_write_nothing(pkg, L):
    dev = torch.from_numpy(_random((2, 64, 64), 1)).cuda()
    c = torch.tensor(_centres("kmeans_q2"), dtype=torch.float32, device="cuda")
    lab = torch.full((2, 32, 32), -9, dtype=torch.int64, device="cuda")
    img = torch.full((2, 32, 32), -9.0, dtype=torch.float32, device="cuda")
    res = torch.full((2, 32, 32), 99, dtype=torch.uint8, device="cuda")
    assert _raw(L, pkg, dev, 4096, None, 1, 0, (64, 64), (32, 32), c, lab, img, res) == 0
    assert _raw(L, pkg, dev, 4096, torch.zeros(0, dtype=torch.int64, device="cuda"), 20, 0, (64, 64), (32, 32), c, lab, img, res) == 0
    assert (lab == -9).all() and (img == -9.0).all() and (res == 99).all()
    assert tuple(pkg.resize_frames(torch.zeros((0, 64, 64), dtype=torch.uint8, device="cuda"), 32).shape) == (0, 32, 32)


def test_native_size_is_the_quantise_path(pkg):
    x = torch.from_numpy(_random((3, 64, 64), 8)).cuda()
    centres = _centres("kmeans_q4")
    labels, image = pkg.resize_quantise_frames(x, 64, centres, 0.1, 0.9)
    want_labels, want_image = pkg.quantise_frames(x, centres, 0.1, 0.9)
    assert torch.equal(labels, want_labels) and torch.equal(image, want_image)
    assert pkg.resize_frames(x, (64, 64)) is x


def test_two_calls_give_the_same_bits(pkg):
    x = torch.from_numpy(_random((40, 64, 64), 12)).cuda()
    a = pkg.resize_quantise_frames(x, 32, _centres("kmeans_q4"), 0.2, 0.8)
    b = pkg.resize_quantise_frames(x, 32, _centres("kmeans_q4"), 0.2, 0.8)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(pkg.resize_frames(x, 32), pkg.resize_frames(x, 32))


def test_tables_are_built_once(pkg):
    M = importlib.import_module("moving-mnist-vae_amd.data")
    x = torch.zeros((1, 24, 24), dtype=torch.uint8, device="cuda")
    pkg.resize_frames(x, 11)
    first = M._resample_tables(24, 11, x.device)
    pkg.resize_frames(x, 11)
    assert M._resample_tables(24, 11, x.device)[0] is first[0] and first[0].is_cuda and first[2] == 7


# ------------------------------------------------------------------------------------------------------------------------- loader
def test_loader_resizes_to_32(pkg, clips_np, clips_ref32):
    centres = _centres("kmeans_q2")
    loader = pkg.MovingMNISTClips(clips_np, centres, 2, "cuda", shuffle=False, image_size=32)
    batches = [b for b in loader]
    assert len(batches) == len(loader) == 3
    lut = R.label_table(centres)
    for i, b in enumerate(batches):
        assert b.dtype == torch.int64 and tuple(b.shape) == (2, 20 * 32 * 32)
        assert np.array_equal(b.cpu().numpy(), lut[clips_ref32[2 * i:2 * i + 2]].reshape(2, -1)), i
    # shuffled: the same clips, in the generator's order
    shuffled = pkg.MovingMNISTClips(clips_np, centres, 4, "cuda", shuffle=True, seed=3, image_size=32)
    order = torch.randperm(6, generator=torch.Generator().manual_seed(3)).numpy()
    got = np.concatenate([b.cpu().numpy() for b in shuffled])
    assert np.array_equal(got, lut[clips_ref32[order]].reshape(6, -1))


@pytest.mark.parametrize("image_size", [None, 64])
def test_loader_at_the_native_size_is_unchanged(pkg, clips_np, image_size):
    centres = _centres("kmeans_q4")
    loader = pkg.MovingMNISTClips(clips_np, centres, 4, "cuda", shuffle=False, image_size=image_size)
    frames = pkg.clips_from_npz_array(clips_np).cuda()
    got = [b for b in loader]
    assert [tuple(b.shape) for b in got] == [(4, 20 * 64 * 64), (2, 20 * 64 * 64)]
    want, _ = pkg.quantise_frames(frames, centres, 0.0, 1.0)
    assert torch.equal(torch.cat(got), want.view(6, -1))


def test_fit_on_resized_frames(pkg, clips_np, clips_ref32):
    loader = pkg.MovingMNISTClips(clips_np, None, 2, "cuda", shuffle=False, image_size=32)
    native = loader.fit_quantiser(2)                                    # on the native bytes, as save_kmeans_file does
    assert np.array_equal(native.counts, np.bincount(clips_np.ravel(), minlength=256))
    at32 = pkg.fit_quantiser(pkg.resize_frames(loader.clips, 32), 2)
    assert np.array_equal(at32.counts, np.bincount(clips_ref32.ravel(), minlength=256))


def test_train_and_evaluate_consume_the_resized_loader(pkg, clips_np):
    M = importlib.import_module("moving-mnist-vae_amd.model")
    loader = pkg.MovingMNISTClips(clips_np, _centres("kmeans_q2"), 2, "cuda", shuffle=False, image_size=32)
    torch.manual_seed(0)
    model = M.VAE(in_channels=1, intermediate_channels=32, decoder_out_channels=2, pixelcnn_out_channels=2, z_dimension=32, pixelcnn=False,
                  only_pixelcnn=False, pixelcnn_layers=4, pixelcnn_activation="ReLu", nll=1, kl=1, mmd=0, require_rsample=True,
                  sigma_decoder=0.1, input_image_size=32).to("cuda")
    opt = M.FusedAdam(list(model.parameters()))
    args = types.SimpleNamespace(data_ratio_of_labels=None, quiet=True, dataset="MovingMNIST")
    losses, nlls, kls, mmds = pkg.train(model, loader, opt, torch.device("cuda"), args, data_mean=0.08, data_std=0.27)
    assert len(losses) == 3 and np.isfinite(losses).all() and np.isfinite(nlls).all() and np.isfinite(kls).all()
    out = pkg.evaluate(model, loader, torch.device("cuda"), args, data_mean=0.08, data_std=0.27)
    assert out["n_images"] == 6 * 20 and np.isfinite(out["nll"]) and np.isfinite(out["kl"])


# -------------------------------------------------------------------------------------------------------------- choose_transformer
def test_choose_transformer_follows_the_reference_rule(pkg):
    centres = _centres("kmeans_q2")
    lut = R.label_table(centres)
    moving = _random((2, 20, 64, 64), 31)
    mnist = _random((3, 1, 28, 28), 32)
    for dataset, size, x in (("MovingMNIST", 64, moving), ("MNIST", 28, mnist)):
        t = pkg.choose_transformer(centres, types.SimpleNamespace(dataset=dataset, input_image_size=size))
        got = t(torch.from_numpy(x).cuda())
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), lut[x].reshape(len(x), -1))
    for dataset, size, x in (("MovingMNIST", 32, moving), ("MNIST", 14, mnist), ("MNIST", 64, mnist), ("MovingMNIST", 28, moving)):
        t = pkg.choose_transformer(centres, types.SimpleNamespace(dataset=dataset, input_image_size=size))
        got = t(torch.from_numpy(x).cuda())
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), lut[R.resize(x, size)].reshape(len(x), -1))
    with pytest.raises(ValueError):
        pkg.choose_transformer(centres, types.SimpleNamespace(dataset="MNIST", input_image_size=14))(torch.from_numpy(mnist))
