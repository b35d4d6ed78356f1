"""CPU: the host half of the Moving MNIST generator -- the IDX reader, the velocity table, the declaration / prototype pair of
mmvae_generate_clips, the argument checks (which run before the library is touched), and the self-consistency of the numpy
restatement of the rule (tests/clipgen_ref.py) the GPU tests compare the kernel with."""
import gzip
import importlib
import os
import re
import struct

import numpy as np
import pytest
import torch

import clipgen_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    return importlib.import_module("moving-mnist-vae_amd.data")


def _idx_bytes(images, magic=0x00000803):
    return struct.pack(">IIII", magic, *images.shape) + images.tobytes()


def test_load_idx_images_plain_and_gz(pkg, tmp_path):
    images = np.random.default_rng(0).integers(0, 256, size=(5, 4, 3), dtype=np.uint8)
    plain, packed = tmp_path / "t-images-idx3-ubyte", tmp_path / "t-images-idx3-ubyte.gz"
    plain.write_bytes(_idx_bytes(images))
    with gzip.open(packed, "wb") as fh:
        fh.write(_idx_bytes(images))
    for path in (plain, str(packed)):
        got = pkg.load_idx_images(path)
        assert got.dtype == np.uint8 and got.shape == (5, 4, 3) and np.array_equal(got, images)


def test_load_idx_images_refuses_wrong_magic_and_truncation(pkg, tmp_path):
    images = np.zeros((2, 3, 3), dtype=np.uint8)
    bad = tmp_path / "labels"
    bad.write_bytes(_idx_bytes(images, magic=0x00000801))
    with pytest.raises(ValueError, match="magic"):
        pkg.load_idx_images(bad)
    cut = tmp_path / "cut"
    cut.write_bytes(_idx_bytes(images)[:-1])
    with pytest.raises(ValueError, match="holds 17"):
        pkg.load_idx_images(cut)
    long = tmp_path / "long"
    long.write_bytes(_idx_bytes(images) + b"\0")
    with pytest.raises(ValueError, match="holds 19"):
        pkg.load_idx_images(long)
    stub = tmp_path / "stub"
    stub.write_bytes(b"\0\0\x08\x03")
    with pytest.raises(ValueError, match="header"):
        pkg.load_idx_images(stub)


@pytest.mark.parametrize("speed", [0.1, 1.0, 0.037])
def test_velocity_table_is_the_formula(pkg, speed):
    got = pkg.velocity_table(speed)
    assert got.dtype == np.int32 and got.shape == (4096, 2)
    for a in (0, 1, 511, 1024, 1700, 2048, 3072, 4095):
        assert got[a, 0] == int(np.rint(speed * 65536 * np.cos(2 * np.pi * a / 4096)))
        assert got[a, 1] == int(np.rint(speed * 65536 * np.sin(2 * np.pi * a / 4096)))
    assert np.array_equal(got, R.velocity_table(speed))
    assert np.abs(got).max() <= 65536
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="speed"):
            pkg.velocity_table(bad)


def test_header_declares_and_binding_prototypes_generate_clips():
    L = importlib.import_module("moving-mnist-vae_amd._lib")
    txt = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    m = re.search(r"MMVAE_API int mmvae_generate_clips\(([^;]*)\);", txt)
    assert m, "include/mmvae.h does not declare mmvae_generate_clips"
    assert "mmvae_generate_clips" in L.PROTOTYPES
    res, args = L.PROTOTYPES["mmvae_generate_clips"]
    assert len(args) == len(m.group(1).split(",")) == 18
    for macro, value in (("MAX_G", L.CLIPGEN_MAX_G), ("MAX_T", L.CLIPGEN_MAX_T), ("MAX_K", L.CLIPGEN_MAX_K),
                         ("DIRECTIONS", L.CLIPGEN_DIRECTIONS)):
        assert re.search(rf"#define MMVAE_CLIPGEN_{macro} {value}\b", txt), macro
    assert "#define MMVAE_CLIPGEN_MAX_D (1 << 24)" in txt and L.CLIPGEN_MAX_D == 1 << 24
    assert "#define MMVAE_ABI_VERSION 3" in txt                   # additions only


def test_argument_checks_raise_before_the_library_is_touched(pkg, M, monkeypatch):
    def untouchable(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(M, "lib", untouchable)
    monkeypatch.setattr(M, "call", untouchable)
    bank = torch.zeros(3, 5, 5, dtype=torch.uint8)              # on the host: the device check comes last and is a ValueError too
    cases = [
        (dict(canvas=24), "canvas"), (dict(canvas=80), "canvas"), (dict(canvas=0), "canvas"),
        (dict(frames=0), "frames"), (dict(frames=33), "frames"),
        (dict(digits=0), "digits"), (dict(digits=5), "digits"),
        (dict(speed=0.0), "speed"), (dict(speed=1.01), "speed"),
        (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"),
        (dict(first_clip=-1), "first_clip"), (dict(first_clip=2 ** 63 - 2), "first_clip"),
        (dict(n_clips=-1), "n_clips"),
    ]
    for kw, name in cases:
        args = dict(n_clips=2, seed=1, canvas=16, frames=4)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            pkg.generate_clips(bank, **args)
        if "n_clips" not in kw:
            args.pop("n_clips")
            with pytest.raises(ValueError, match=name):
                pkg.GeneratedClips(bank, [0.0, 1.0], 2, 4, "cpu", **args)
    for bad_bank, name in ((torch.zeros(3, 5, 5), "bank"), (torch.zeros(3, 5, 4, dtype=torch.uint8), "bank"),
                           (np.zeros((5, 5), dtype=np.uint8), "bank"), (torch.zeros(0, 5, 5, dtype=torch.uint8), "D=0"),
                           (torch.zeros(2, 33, 33, dtype=torch.uint8), "G=33"), (torch.zeros(2, 16, 16, dtype=torch.uint8), "room")):
        with pytest.raises(ValueError, match=name):
            pkg.generate_clips(bad_bank, 2, 0, canvas=64 if bad_bank.shape[-1] == 33 else 16)
    with pytest.raises(ValueError, match="batch_size"):
        pkg.GeneratedClips(bank, None, 0, 4, "cpu", canvas=16)
    with pytest.raises(ValueError, match="clips_per_epoch"):
        pkg.GeneratedClips(bank, None, 2, 0, "cpu", canvas=16)
    with pytest.raises(ValueError, match="want"):
        pkg.generate_batch(bank, 2, 0, 0, [0.0, 1.0], 0.0, 1.0, want=(False, False, False), canvas=16)
    with pytest.raises(ValueError, match="GPU"):                 # everything else in order: only now the device matters
        pkg.generate_clips(bank, 2, 0, canvas=16)
    with pytest.raises(ValueError, match="n_test"):
        pkg.save_moving_mnist_files("unused", bank, 2, -1, canvas=16)
    with pytest.raises(ValueError, match="canvas"):
        pkg.save_moving_mnist_files("unused", bank, 2, 1, canvas=20)


def test_generated_clips_loader_contract_on_the_host(pkg):
    bank = np.zeros((3, 5, 5), dtype=np.uint8)
    loader = pkg.GeneratedClips(bank, None, 4, 10, "cpu", canvas=16, frames=3)
    assert len(loader) == 3 and len(loader.train_data) == 10 and loader.centres is None
    with pytest.raises(RuntimeError, match="fit_quantiser"):
        iter(loader)


def _ramp_bank(D, G):
    return ((np.arange(D * G * G, dtype=np.int64) * 37 + 11) % 255 + 1).astype(np.uint8).reshape(D, G, G)


def test_reference_is_a_function_of_the_clip_index():
    bank = _ramp_bank(9, 5)
    whole = R.generate(bank, 3, seed=77, first_clip=0, frames=6, canvas=16, digits=3)
    assert np.array_equal(R.generate(bank, 2, seed=77, first_clip=1, frames=6, canvas=16, digits=3), whole[1:3])
    assert not np.array_equal(whole[0], whole[1])
    assert not np.array_equal(whole, R.generate(bank, 3, seed=78, first_clip=0, frames=6, canvas=16, digits=3))
    high = 2 ** 33 + 5
    assert np.array_equal(R.generate(bank, 1, seed=77, first_clip=high + 1, frames=6, canvas=16, digits=3),
                          R.generate(bank, 2, seed=77, first_clip=high, frames=6, canvas=16, digits=3)[1:])


@pytest.mark.parametrize("S,G,T,K,speed", [(64, 28, 20, 2, 0.1), (32, 31, 3, 2, 0.1), (16, 1, 32, 4, 0.1), (16, 5, 8, 4, 1.0)])
def test_reference_positions_stay_inside(S, G, T, K, speed):
    info = {}
    out = R.generate(_ramp_bank(4, G), 40, seed=5, frames=T, canvas=S, digits=K, speed=speed, info=info)
    assert out.shape == (40, T, S, S)
    pos = np.array(info["positions"])
    assert pos.shape == (40 * K * T, 5)
    assert pos[:, 3].min() >= 0 and pos[:, 4].min() >= 0 and pos[:, 3].max() <= S - G and pos[:, 4].max() <= S - G
    assert info["bounces"] > 0


def test_reference_glyph_frequencies():
    """D = 7, seed 123, 7000 clips, K = 3: every glyph's count within 4 binomial standard deviations of n / 7 (measured: 1.62)."""
    D, n = 7, 7000 * 3
    counts = np.zeros(D, dtype=np.int64)
    for c in range(7000):
        for k in range(3):
            counts[R.draws(123, c, k, D)[0]] += 1
    assert counts.sum() == n
    sd = np.sqrt(n * (1 / D) * (1 - 1 / D))
    worst = np.abs(counts - n / D).max() / sd
    print("worst glyph frequency deviation: %.2f binomial standard deviations" % worst)
    assert worst <= 4.0
