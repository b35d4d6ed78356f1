"""GPU: the byte-histogram kernel (mmvae_u8_histogram) against np.bincount, exactly, at the smallest shapes where it can go wrong
(scalar head / 16-byte body / scalar tail, unaligned bases, clip starts that rotate through every alignment, more than one work
item and block, inputs that put every byte on one LDS word), and the fit built on it end to end: fit_quantiser, the host label
table against the quantise kernel, MovingMNISTClips.fit_quantiser, save_kmeans_file / load_kmeans_file."""
import importlib

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

CLIP = 20 * 64 * 64                   # one Moving-MNIST clip: 81920 bytes, more than one work item
GRID_TIE_CENTRES = [0.0, 2 / 255.0, 4 / 255.0]


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


@pytest.fixture(scope="module")
def golden_frames():
    return load_golden("kmeans_q2")["frames"]                           # (5, 64, 64) uint8; the last one is a ramp of all 256 values


def _bincount(a):
    return np.bincount(np.asarray(a, dtype=np.uint8).ravel(), minlength=256).astype(np.int64)


def _random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


def _raw(L, frames, clip_bytes, index, n_clips, counts):
    """The C entry point itself, on the caller's counts."""
    rc = L.lib().mmvae_u8_histogram(L.ptr(frames), clip_bytes, L.ptr(index), n_clips, L.ptr(counts), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------------------------ contiguous
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4099])
def test_contiguous_sizes(pkg, n):
    a = _random_bytes(n, n)
    got = pkg.pixel_histogram(torch.from_numpy(a).cuda())
    assert got.dtype == torch.int64 and got.shape == (256,) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), _bincount(a))


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("n", [17, 4099, 3 * CLIP + 5])
def test_base_pointer_inside_a_larger_buffer(pkg, offset, n):
    a = _random_bytes(n + 40, 7 * n + offset)
    view = torch.from_numpy(a).cuda()[offset:offset + n]
    assert view.data_ptr() % 16 == offset
    assert np.array_equal(pkg.pixel_histogram(view).cpu().numpy(), _bincount(a[offset:offset + n]))


def test_zero_clips_leave_the_counts_alone_and_calls_accumulate(pkg, L):
    a, b = _random_bytes(4099, 1), _random_bytes(333, 2)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    start = torch.arange(256, dtype=torch.int64, device="cuda") * 3 + 1
    counts = start.clone()
    assert _raw(L, da, 4099, None, 0, counts) == 0
    assert _raw(L, da, 17, torch.zeros(0, dtype=torch.int64, device="cuda"), 0, counts) == 0
    assert torch.equal(counts, start)
    assert _raw(L, da, 1, None, 4099, counts) == 0
    assert _raw(L, db, 333, None, 1, counts) == 0
    assert np.array_equal(counts.cpu().numpy(), start.cpu().numpy() + _bincount(a) + _bincount(b))
    assert pkg.pixel_histogram(torch.zeros((0, 20, 8, 8), dtype=torch.uint8, device="cuda")).sum().item() == 0


# ------------------------------------------------------------------------------------------------------- worst-case contention
def test_constant_and_two_valued_clips(pkg):
    zeros = np.zeros((1, 20, 64, 64), dtype=np.uint8)
    full = np.full((1, 20, 64, 64), 255, dtype=np.uint8)
    two = np.full(CLIP, 7, dtype=np.uint8)
    two[5::16] = 200                                                    # 15 : 1
    for a in (zeros, full, two.reshape(1, 20, 64, 64)):
        got = pkg.pixel_histogram(torch.from_numpy(a).cuda()).cpu().numpy()
        assert np.array_equal(got, _bincount(a))
    assert _bincount(two)[7] == 15 * _bincount(two)[200]


def test_every_value_present(pkg, golden_frames):
    ramp = golden_frames[4]
    assert len(np.unique(ramp)) == 256
    assert np.array_equal(pkg.pixel_histogram(torch.from_numpy(ramp).cuda()).cpu().numpy(), _bincount(ramp))
    assert np.array_equal(pkg.pixel_histogram(torch.from_numpy(golden_frames).cuda()).cpu().numpy(), _bincount(golden_frames))


# --------------------------------------------------------------------------------------------------------------------- indexed
@pytest.mark.parametrize("offset", [0, 1])
def test_indexed_clips_of_1620_bytes(pkg, offset):
    n = 11
    a = _random_bytes(n * 1620 + 16, 99)                                # 1620 = 4 mod 16: clip starts rotate through alignments
    clips_np = a[offset:offset + n * 1620].reshape(n, 20, 9, 9)
    clips = torch.from_numpy(a).cuda()[offset:offset + n * 1620].view(n, 20, 9, 9)
    for index in ([3, 3, 7, 0, 3], list(range(n - 1, -1, -1)), [5], [0, n - 1]):
        got = pkg.pixel_histogram(clips, torch.tensor(index)).cpu().numpy()
        assert np.array_equal(got, _bincount(clips_np[index])), index
    assert pkg.pixel_histogram(clips, []).sum().item() == 0


def test_indexed_clips_of_more_than_one_work_item(pkg):
    a = _random_bytes(3 * CLIP + 16, 5)
    clips_np = a[3:3 + 3 * CLIP].reshape(3, 20, 64, 64)
    clips = torch.from_numpy(a).cuda()[3:3 + 3 * CLIP].view(3, 20, 64, 64)
    index = [2, 0, 2]
    assert np.array_equal(pkg.pixel_histogram(clips, index).cpu().numpy(), _bincount(clips_np[index]))


def test_argument_checks(pkg):
    with pytest.raises(ValueError):
        pkg.pixel_histogram(torch.zeros(4, 4, dtype=torch.uint8))                             # host tensor
    with pytest.raises(ValueError):
        pkg.pixel_histogram(torch.zeros(4, 4, dtype=torch.int32, device="cuda"))
    clips = torch.zeros(4, 16, dtype=torch.uint8, device="cuda")
    for bad in ([4], [-1], [0, 1, 9]):
        with pytest.raises(IndexError):
            pkg.pixel_histogram(clips, bad)
    with pytest.raises(ValueError):
        pkg.fit_quantiser(clips, 2, clips=5)


# ------------------------------------------------------------------------------------------------- host and device rules agree
def test_host_label_table_is_what_quantise_frames_returns(pkg, L, golden_frames):
    dev = torch.from_numpy(golden_frames).cuda()
    fits = {q: pkg.fit_quantiser(dev, q) for q in (2, 4)}
    for q, fit in fits.items():
        labels, _ = pkg.quantise_frames(dev, fit.centres, 0.0, 1.0)
        assert np.array_equal(labels.cpu().numpy(), fit.lut[golden_frames].astype(np.int64)), q
        assert np.array_equal(fit.counts, _bincount(golden_frames))
    counts = np.ascontiguousarray(_bincount(golden_frames), dtype=np.uint64)
    for centres in (load_golden("kmeans_q2")["centres"], load_golden("kmeans_q4")["centres"], GRID_TIE_CENTRES):
        c32 = np.ascontiguousarray(centres, dtype=np.float32)
        lut = np.zeros(256, dtype=np.uint8)
        assert L.lib().mmvae_quantiser_stats(counts.ctypes.data, c32.ctypes.data, c32.size, lut.ctypes.data, None, None, None) == 0
        labels, _ = pkg.quantise_frames(dev, centres, 0.0, 1.0)
        assert np.array_equal(labels.cpu().numpy(), lut[golden_frames].astype(np.int64)), centres
        ramp = torch.arange(256, dtype=torch.uint8, device="cuda")
        assert np.array_equal(pkg.quantise_frames(ramp, centres, 0.0, 1.0)[0].cpu().numpy(), lut.astype(np.int64))


def test_sampled_clips_are_distinct_and_follow_the_generator(pkg):
    clips_np = _random_bytes(9 * 1620, 3).reshape(9, 20, 9, 9)
    clips = torch.from_numpy(clips_np).cuda()
    fit = pkg.fit_quantiser(clips, 3, clips=4, generator=torch.Generator().manual_seed(11))
    index = torch.randperm(9, generator=torch.Generator().manual_seed(11))[:4].numpy()
    assert len(set(index.tolist())) == 4
    assert np.array_equal(fit.counts, _bincount(clips_np[index]))
    again = pkg.fit_quantiser(clips, 3, clips=4, generator=torch.Generator().manual_seed(11))
    assert np.array_equal(again.centres, fit.centres) and again.inertia == fit.inertia


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_loader_fits_its_own_quantiser_and_the_file_round_trips(pkg, golden_frames, tmp_path):
    arr = np.stack([np.roll(golden_frames, i, axis=0) for i in range(6)])           # (N, C, W, H) = (6, 5, 64, 64), the file's layout
    loader = pkg.MovingMNISTClips(arr, None, 4, "cuda", shuffle=False)
    with pytest.raises(RuntimeError):
        next(iter(loader))
    fit = loader.fit_quantiser(2)
    assert fit.centres.dtype == np.float64 and fit.centres[0] < fit.centres[1]
    assert np.array_equal(fit.counts, _bincount(arr))
    batches = [b.cpu().numpy() for b in loader]
    assert [b.shape for b in batches] == [(4, 5 * 64 * 64), (2, 5 * 64 * 64)]
    labels = np.concatenate(batches)
    x = arr.transpose(0, 1, 3, 2).reshape(6, -1).astype(np.float32) / np.float32(255.0)
    want = np.argmin((x[..., None] - fit.centres.astype(np.float32)) ** 2, axis=-1)
    assert np.array_equal(labels, want)
    # both sides are f64 sums of small integers
    mean, std = labels.mean(dtype=np.float64), labels.std(dtype=np.float64)
    ratios = np.bincount(labels.ravel(), minlength=2) / labels.size
    print("label mean", mean, fit.data_mean, "std", std, fit.data_std, "ratios", ratios, fit.ratios)
    assert abs(mean - fit.data_mean) <= 1e-12 * abs(mean) and abs(std - fit.data_std) <= 1e-12 * std
    np.testing.assert_allclose(fit.ratios, ratios, rtol=1e-12)
    w = fit.weights(device="cuda")
    assert w.is_cuda and w.dtype == torch.float32 and np.allclose(w.cpu().numpy(), 1.0 - ratios)

    centres, data_mean, data_std, r = pkg.save_kmeans_file(2, dataset="Tiled", folder=str(tmp_path), source=arr)
    assert centres.shape == (2, 1) and np.array_equal(centres.ravel(), fit.centres)
    assert data_mean == round(fit.data_mean, 4) and data_std == round(fit.data_std, 4) and np.array_equal(r, fit.ratios.round(4))
    path = tmp_path / "kmeans_Tiled_2.npz"
    assert path.is_file()
    with np.load(path, allow_pickle=False) as raw:                                   # data only
        assert {"centres", "data_mean", "data_std", "ratios", "counts"} <= set(raw.files)
    d = pkg.load_kmeans_file(str(path))
    assert np.array_equal(d["centres"], fit.centres) and np.array_equal(d["counts"], fit.counts) and np.array_equal(d["ratios"], r)
    assert d["data_mean"] == data_mean and d["data_std"] == data_std
