"""GPU: mmvae_nearest_frames and the Python surface on top of it (nearest_frames, neighbour_sheet, plot_neighbours) against the CPU
reference of tests/test_neighbours_cpu.py (float64 expansion, exact below 2^53, then a stable sort).  Every comparison is exact
(torch.equal): distances and indices, ties included.  The random cases carry an asymmetric operand on both sides of the matrix product,
so a wrong row / column assignment of the int8 MFMA's A or B lanes cannot pass them."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_neighbours_cpu import nearest_ref  # noqa: E402
from test_panels_cpu import _decode_png_gray  # noqa: E402

gpu = pytest.mark.gpu


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _rand(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _dev(f):
    """Host planes to the device; flat (F, D) rows go as F planes of 1 x D (``frames`` is [..., H, W])."""
    return f.cuda().unsqueeze(1) if f.dim() == 2 else f.cuda()


def _planted(M, F, D, seed):
    """Random bytes with exact copies of queries at frame 0 (query 0), F - 1 (query 1), two interior indices far apart (query 2, at both)
    and a second copy of query 0 in the middle."""
    q, f = _rand((M, D), seed), _rand((F, D), seed + 1)
    f[0], f[F - 1], f[F // 3], f[2 * F // 3 + 5], f[F // 2] = q[0], q[1], q[2], q[2], q[0]
    return q, f


def _blobs(M, F, S, seed):
    """Moving-MNIST-like planes: zeros with one 14 x 14 patch of bright bytes per plane (about 95 % zeros); the queries are frames with
    a handful of pixels changed, and fresh planes."""
    g = torch.Generator().manual_seed(seed)
    patches = torch.randint(128, 256, (64, 14, 14), dtype=torch.uint8, generator=g)
    which, pos = torch.randint(0, 64, (F + M,), generator=g).tolist(), torch.randint(0, S - 14, (F + M, 2), generator=g).tolist()
    planes = torch.zeros((F + M, S, S), dtype=torch.uint8)
    for i in range(F + M):
        planes[i, pos[i][0]:pos[i][0] + 14, pos[i][1]:pos[i][1] + 14] = patches[which[i]]
    f, q = planes[:F].reshape(F, S * S), planes[F:].reshape(M, S * S).clone()
    src = torch.randint(0, F, (M // 2,), generator=g)
    q[:M // 2] = f[src]
    q[:M // 2, ::97] ^= 0x40
    return q, f.contiguous()


_CASES = {}


def _case(name):
    """(queries, frames) on the host, built once per session; the reference is cached beside them by the callers."""
    if name not in _CASES:
        if name == "tail784":
            _CASES[name] = (_rand((6, 784), 10), _rand((17, 784), 11))
        elif name == "big4096":
            _CASES[name] = _planted(16, 30000, 4096, 20)
    return _CASES[name]


_REFS = {}


def _ref(name, q, f, k, lut=None, tag=""):
    key = (name, k, tag)
    if key not in _REFS:
        _REFS[key] = nearest_ref(q, f, k, lut)
    return _REFS[key]


def _check(pkg, q, f, k, lut=None, ref=None):
    want_d, want_i = ref if ref is not None else nearest_ref(q, f, k, lut)
    dist, index = pkg.nearest_frames(q.cuda(), _dev(f), k=k, lut=lut)
    assert dist.dtype == torch.int32 and index.dtype == torch.int64 and dist.is_cuda and index.is_cuda
    assert tuple(dist.shape) == tuple(index.shape) == (q.shape[0], k)
    dist, index = dist.cpu(), index.cpu()
    assert torch.equal(dist, want_d), (dist, want_d)
    assert torch.equal(index, want_i), (index, want_i)
    return dist, index


# ------------------------------------------------------------------------------------------ the shapes
@gpu
@pytest.mark.parametrize("M,F,D,k", [(1, 1, 16, 1), (16, 16, 64, 8), (17, 33, 1024, 8), (64, 1000, 4096, 8), (3, 8, 256, 8), (9, 50, 208, 4),
                                     (33, 70, 192, 8)])
def test_random_bytes(pkg, M, F, D, k):
    """The smallest everything; one full row tile, one row past it, all four; F == k returns every frame, in order; D = 208 and 192: one
    128-byte line, then a single 64-byte step (and a quarter step) behind it."""
    dist, index = _check(pkg, _rand((M, D), 100 + M), _rand((F, D), 200 + F), k)
    if F == k:
        assert torch.equal(index.sort(dim=1).values, torch.arange(F).expand(M, F))


@gpu
def test_k_tail_of_a_28x28_plane(pkg):
    """784 = 12 * 64 + 16: the last k step is a quarter full; 17 frames are one tile and one frame."""
    q, f = _case("tail784")
    _check(pkg, q, f, 5, ref=_ref("tail784", q, f, 5))


@gpu
def test_largest_and_zero_distance_in_one_call(pkg):
    M, F, D, k = 2, 40, 16384, 4
    q, f = torch.zeros((M, D), dtype=torch.uint8), torch.full((F, D), 255, dtype=torch.uint8)
    f[7], f[20], f[39] = 0, 0, 0
    dist, index = _check(pkg, q, f, k)
    assert dist.tolist() == [[0, 0, 0, 1065369600]] * M and index.tolist() == [[7, 20, 39, 0]] * M


@gpu
def test_thousands_of_ties_go_to_the_lowest_indices(pkg):
    M, F, D, k = 5, 5000, 16, 8
    g = torch.Generator().manual_seed(31)
    templates = torch.randint(0, 2, (8, D), generator=g).to(torch.uint8) * 255
    f = templates[torch.randint(0, 8, (F,), generator=g)]
    q = templates[torch.randint(0, 8, (M,), generator=g)].clone()
    q[4, 3] ^= 255                                           # one query that equals no template
    dist, index = _check(pkg, q, f, k)
    assert (dist[:4] == 0).all() and (index[:, 1:] > index[:, :-1]).all()


@gpu
def test_identical_frames_return_the_first_indices(pkg):
    M, F, D, k = 4, 100, 64, 8
    f = _rand((1, D), 41).expand(F, D).contiguous()
    dist, index = _check(pkg, _rand((M, D), 42), f, k)
    assert index.tolist() == [list(range(k))] * M and (dist == dist[:, :1]).all()


@gpu
@pytest.mark.parametrize("name,M,F,D,k", [("big4096", 16, 30000, 4096, 8), ("big1024", 16, 200000, 1024, 8)])
def test_many_blocks_with_planted_copies(pkg, name, M, F, D, k):
    """Many blocks, a wave's walk over several tile groups, the merge: the copies come back at distance 0, and where a query's copy sits
    at two indices the lower one comes first."""
    q, f = _case(name) if name == "big4096" else _planted(M, F, D, 50)
    dist, index = _check(pkg, q, f, k, ref=_ref(name, q, f, k) if name == "big4096" else None)
    assert dist[0, :2].tolist() == [0, 0] and index[0, :2].tolist() == [0, F // 2]
    assert dist[1, 0] == 0 and index[1, 0] == F - 1 and dist[1, 1] > 0
    assert dist[2, :2].tolist() == [0, 0] and index[2, :2].tolist() == [F // 3, 2 * F // 3 + 5]
    assert (dist[3:, 0] > 0).all()


@gpu
def test_sparse_planes_with_bright_blobs(pkg):
    q, f = _blobs(16, 20000, 64, 60)
    assert float((f == 0).float().mean()) > 0.94
    _check(pkg, q, f, 5)


# ------------------------------------------------------------------------------------------ lut
def _step_lut(pkg, f, classes=4):
    D = importlib.import_module("moving-mnist-vae_amd.data")
    fit = D._fit_counts(np.bincount(f.numpy().reshape(-1), minlength=256), classes)
    lut = torch.from_numpy(fit.lut.copy())
    assert (lut[1:] >= lut[:-1]).all() and int(lut.max()) == classes - 1
    return lut


@gpu
@pytest.mark.parametrize("name,k", [("tail784", 5), ("big4096", 8)])
@pytest.mark.parametrize("table", ["steps", "permutation"])
def test_lut_is_applied_to_the_frames_per_byte(pkg, name, k, table):
    """A monotone step table (byte -> k-means label, the queries in label space) and a random permutation of 0..255 (nothing about the
    table may be assumed)."""
    q, f = _case(name)
    lut = _step_lut(pkg, f) if table == "steps" else torch.randperm(256, generator=torch.Generator().manual_seed(7)).to(torch.uint8)
    ql = lut[q.long()]
    dist, index = _check(pkg, ql, f, k, lut=lut, ref=_ref(name, ql, f, k, lut, tag=table))
    if name == "big4096":
        F = f.shape[0]
        assert dist[2, :2].tolist() == [0, 0] and index[2, :2].tolist() == [F // 3, 2 * F // 3 + 5]
    d2, i2 = pkg.nearest_frames(ql.cuda(), _dev(f), k=k, lut=lut.cuda())          # the table from either device
    assert torch.equal(d2.cpu(), dist) and torch.equal(i2.cpu(), index)


# ------------------------------------------------------------------------------------------ views, clips
@gpu
def test_leading_axes_are_flattened(pkg):
    n = 50
    clips = _rand((n, 20, 8, 8), 70)
    picks = [(0, 0), (17, 13), (49, 19)]
    q = torch.stack([clips[c, t] for c, t in picks])
    want = nearest_ref(q, clips, 6)
    for queries in (q, q[:, None], q.reshape(3, 64)):
        dist, index = pkg.nearest_frames(queries.cuda(), clips.cuda(), k=6)
        assert torch.equal(dist.cpu(), want[0]) and torch.equal(index.cpu(), want[1])
    clip, frame = np.divmod(index.cpu().numpy()[:, 0], 20)
    assert list(zip(clip.tolist(), frame.tolist())) == picks and (dist[:, 0] == 0).all()
    shifted = torch.zeros(8 + clips.numel(), dtype=torch.uint8)
    shifted[8:] = clips.reshape(-1)
    view = shifted.cuda()[8:].view(n, 20, 8, 8)              # 8 bytes off the allocation's alignment
    dist, index = pkg.nearest_frames(q.cuda(), view, k=6)
    assert torch.equal(dist.cpu(), want[0]) and torch.equal(index.cpu(), want[1])


@gpu
def test_moving_mnist_clips_as_frames(pkg):
    arr = _rand((6, 20, 16, 16), 80).numpy()                 # the dataset file's (N, C, W, H)
    loader = pkg.MovingMNISTClips(arr, None, 2, "cuda")
    q = loader.clips[[2, 5], [5, 19]]
    dist, index = pkg.nearest_frames(q, loader, k=4)
    want = nearest_ref(q.cpu(), loader.clips.cpu(), 4)
    assert torch.equal(dist.cpu(), want[0]) and torch.equal(index.cpu(), want[1])
    assert index[:, 0].tolist() == [2 * 20 + 5, 5 * 20 + 19] and dist[:, 0].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------ writes, determinism
def _align(n, a=256):
    return (n + a - 1) // a * a


@gpu
@pytest.mark.parametrize("M,F,D,k,with_lut", [(17, 33, 1024, 8, False), (6, 17, 784, 5, True), (16, 5000, 64, 3, False), (9, 50, 208, 4, True)])
def test_writes_stay_inside_their_arrays(pkg, M, F, D, k, with_lut):
    """out_dist, out_index and a scratch of exactly mmvae_nearest_frames_scratch_bytes are carved out of one buffer filled with 0xA5,
    256 guard bytes (or more) around each; every byte outside the three regions keeps its value."""
    L = _L()
    q, f = _rand((M, D), 90), _rand((F, D), 91)
    lut = torch.randperm(256, generator=torch.Generator().manual_seed(3)).to(torch.uint8) if with_lut else None
    nbytes = L.lib().mmvae_nearest_frames_scratch_bytes(M, F, D, k)
    assert nbytes > 0
    guard = 256
    o_dist = guard
    o_index = _align(o_dist + M * k * 4 + guard)
    o_scr = _align(o_index + M * k * 8 + guard)
    total = o_scr + nbytes + guard
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    dq, df, dl = q.cuda(), f.cuda(), None if lut is None else lut.cuda()
    base = buf.data_ptr()
    assert base % 256 == 0
    rc = L.lib().mmvae_nearest_frames(dq.data_ptr(), M, df.data_ptr(), F, D, L.ptr(dl), k, base + o_dist, base + o_index, base + o_scr, nbytes,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.lib().mmvae_last_error()
    torch.cuda.synchronize()
    host = buf.cpu()
    dist = host[o_dist:o_dist + M * k * 4].view(torch.int32).view(M, k)
    index = host[o_index:o_index + M * k * 8].view(torch.int64).view(M, k)
    want = nearest_ref(q, f, k, lut)
    assert torch.equal(dist, want[0]) and torch.equal(index, want[1])
    outside = torch.ones(total, dtype=torch.bool)
    for lo, n in ((o_dist, M * k * 4), (o_index, M * k * 8), (o_scr, nbytes)):
        outside[lo:lo + n] = False
    assert int(outside.sum()) == total - M * k * 12 - nbytes
    assert (host[outside] == 0xA5).all()
    rc = L.lib().mmvae_nearest_frames(dq.data_ptr(), M, df.data_ptr(), F, D, L.ptr(dl), k, base + o_dist, base + o_index, base + o_scr, nbytes - 1,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == -3                                          # MMVAE_ERR_WORKSPACE, nothing enqueued


@gpu
def test_same_bits_every_run_and_on_any_stream(pkg):
    q, f = _case("big4096")
    dq, df = q.cuda(), _dev(f)
    a = pkg.nearest_frames(dq, df, k=8)
    b = pkg.nearest_frames(dq, df, k=8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = pkg.nearest_frames(dq, df, k=8)
    side.synchronize()
    torch.cuda.synchronize()
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
    want = _ref("big4096", q, f, 8)
    assert torch.equal(a[0].cpu(), want[0]) and torch.equal(a[1].cpu(), want[1])


@gpu
def test_python_surface_refuses_device_tensors_too(pkg):
    q, f = torch.zeros((4, 8, 8), dtype=torch.uint8, device="cuda"), torch.zeros((30, 8, 8), dtype=torch.uint8, device="cuda")
    for fn in (pkg.nearest_frames, pkg.neighbour_sheet):
        for kw, what in ((dict(k=0), "k=0"), (dict(k=9), "k=9"), (dict(lut=torch.zeros(3, dtype=torch.uint8)), "lut")):
            with pytest.raises(ValueError, match=what):
                fn(q, f, **kw)
        with pytest.raises(ValueError, match="M=65"):
            fn(torch.zeros((65, 8, 8), dtype=torch.uint8, device="cuda"), f)
        with pytest.raises(ValueError, match="do not match"):
            fn(q.view(4, 4, 16), f)
        with pytest.raises(ValueError, match="GPU"):
            fn(q.cpu(), f)
    with pytest.raises(ValueError, match="k=8"):
        pkg.neighbour_sheet(q, f, k=8)
    with pytest.raises(ValueError, match="square"):
        pkg.neighbour_sheet(q.view(4, 4, 16), f.view(30, 4, 16))


# ------------------------------------------------------------------------------------------ the sheet
def _strip(planes, S):
    """(M, S*S) planes stacked vertically: the (M * S, S) bytes of one sheet column."""
    return planes.reshape(-1, S)


@gpu
def test_neighbour_sheet_through_the_image_path(pkg):
    M, F, S, k = 4, 100, 8, 3
    q, f = _rand((M, S, S), 110), _rand((F, S, S), 111)
    f[40] = q[1]
    for lut in (None, torch.randperm(256, generator=torch.Generator().manual_seed(5)).to(torch.uint8)):
        sheet, dist, index = pkg.neighbour_sheet(q.cuda(), f.cuda(), k=k, lut=lut)
        want = nearest_ref(q, f, k, lut)
        assert torch.equal(dist.cpu(), want[0]) and torch.equal(index.cpu(), want[1])
        assert sheet.dtype == torch.uint8 and tuple(sheet.shape) == (M * S, (k + 1) * S) and sheet.is_cuda
        sheet = sheet.cpu()
        assert torch.equal(sheet[:, :S], _strip(q, S))
        shown = f if lut is None else lut[f.long()]
        for j in range(1, k + 1):
            assert torch.equal(sheet[:, j * S:(j + 1) * S], _strip(shown[want[1][:, j - 1]], S)), j
        if lut is None:
            assert want[1][1, 0] == 40 and torch.equal(sheet[S:2 * S, :S], sheet[S:2 * S, S:2 * S])      # query 1 beside its copy


@gpu
def test_neighbour_sheet_through_a_display_lut(pkg):
    M, F, S, k = 5, 64, 16, 7
    q, f = _rand((M, S * S), 120), _rand((F, 1, S, S), 121)
    lut = _step_lut(pkg, f)
    ql = lut[q.long()]
    grey = pkg.gray_lut(4)
    sheet, dist, index = pkg.neighbour_sheet(ql.cuda(), f.cuda(), k=k, lut=lut, display_lut=grey)
    want = nearest_ref(ql, f, k, lut)
    assert torch.equal(dist.cpu(), want[0]) and torch.equal(index.cpu(), want[1])
    sheet = sheet.cpu()
    assert tuple(sheet.shape) == (M * S, (k + 1) * S)
    assert torch.equal(sheet[:, :S], _strip(grey[ql.long()], S))
    labels = lut[f.reshape(F, S * S).long()]
    for j in range(1, k + 1):
        assert torch.equal(sheet[:, j * S:(j + 1) * S], _strip(grey[labels[want[1][:, j - 1]].long()], S)), j


@gpu
def test_plot_neighbours_writes_the_sheet(pkg, tmp_path):
    q, f = _rand((3, 8, 8), 130), _rand((50, 8, 8), 131)
    sheet, dist, index = pkg.plot_neighbours(q.cuda(), f.cuda(), str(tmp_path / "plots"), 2, 7, k=4)
    path = tmp_path / "plots" / "neighbours-2-7.png"
    assert path.is_file() and sorted(os.listdir(tmp_path / "plots")) == ["neighbours-2-7.png"]
    assert np.array_equal(_decode_png_gray(path.read_bytes()), sheet.cpu().numpy())
    again = pkg.neighbour_sheet(q.cuda(), f.cuda(), k=4)
    assert torch.equal(again[0], sheet) and torch.equal(again[1], dist) and torch.equal(again[2], index)
    want = nearest_ref(q, f, 4)
    assert torch.equal(dist.cpu(), want[0]) and torch.equal(index.cpu(), want[1])
