"""GPU: mmvae_knn_cross through cross_neighbours / ball_counts against the CPU references of tests/knn_ref.py.  Every comparison is
torch.equal on integers.  The shapes are the smallest at which the tiling can go wrong: rows and columns that straddle the 128 x 128
block tile and its 64 x 64 wave quarters, a partial last 64-byte k step, several column ranges meeting in the merge, the largest
distance; random bytes on both sides with Na != Nb, so a swapped A / B lane assignment cannot pass."""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from knn_ref import ball_counts_ref, dist_matrix, knn_cross_ref, tie_case  # noqa: E402

gpu = pytest.mark.gpu
SHAPES = {"tie": (5, 37, 16), "tail784": (259, 517, 784), "d4096": (300, 700, 4096), "ranges": (200, 5000, 64), "maxd": (17, 19, 16384)}


def _L():
    return importlib.import_module("moving-mnist-vae_amd._lib")


def _S():
    return importlib.import_module("moving-mnist-vae_amd.samples")


def _rand(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


_CASES = {}


def _case(name):
    """(a, b, exact distance matrix, reference for k = 8 or all columns) on the host, built once per session and left unchanged."""
    if name not in _CASES:
        if name == "tie":
            a, b = tie_case()
        elif name == "square":                                # a = b with duplicate rows: the duplicate stays, the self pair goes
            a = _rand((259, 784), 40)
            a[200], a[101], a[258] = a[7], a[100], a[0]
            b = a
        else:
            Na, Nb, D = SHAPES[name]
            a, b = _rand((Na, D), 30 + D % 97), _rand((Nb, D), 31 + D % 97)
            if name == "maxd":                                # the largest distance 16384 * 65025 and the largest signed cross term
                a[0], a[1], b[0], b[1], b[2] = 0, 255, 255, 0, 255
        d = dist_matrix(a, b)
        _CASES[name] = (a, b, d, knn_cross_ref(a, b, 8, name == "square"))
    return _CASES[name]


def _radii(d, seed):
    """One radius per column, drawn from that column's exact distances: many comparisons hit equality."""
    rows = torch.randint(0, d.shape[0], (d.shape[1],), generator=torch.Generator().manual_seed(seed))
    return d[rows, torch.arange(d.shape[1])].clone()


@gpu
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("name", list(SHAPES))
def test_k_nearest_equals_the_reference(pkg, name, k):
    a, b, _, (rd, ri) = _case(name)
    dist, index = pkg.cross_neighbours(a.cuda(), b.cuda(), k=k)
    assert dist.dtype == torch.int32 and index.dtype == torch.int64 and dist.shape == index.shape == (a.shape[0], k)
    assert torch.equal(dist.cpu(), rd[:, :k]) and torch.equal(index.cpu(), ri[:, :k])
    if name == "tie":
        assert dist[2, 0] == 0 and index[2].tolist()[:min(k, 2)] == [3, 30][:min(k, 2)]
    if name == "maxd":
        assert int(dist_matrix(a, b).max()) == 16384 * 65025


@gpu
def test_the_column_split_meets_in_the_merge(pkg):
    """(200, 5000, 64) is cut into several column ranges (read back from the plan, not assumed); their partial lists meet in the merge."""
    Na, Nb, D = SHAPES["ranges"]
    L = _L()
    ranges = L.knn_cross_ranges(Na, Nb)
    assert ranges >= 2
    up16 = lambda v: (v + 15) // 16 * 16
    assert L.lib().mmvae_knn_cross_scratch_bytes(Na, Nb, D, 3, 1) == up16(4 * Na) + up16(4 * Nb) + 2 * ranges * Na * 3 * 8 + up16(2 * ranges * Na * 4)
    a, b, _, (rd, ri) = _case("ranges")
    rows = ri[:, 0] // 128                                              # the nearest columns do come from different ranges
    assert rows.unique().numel() >= 2
    dist, index = pkg.cross_neighbours(a.cuda(), b.cuda(), k=8)
    assert torch.equal(dist.cpu(), rd) and torch.equal(index.cpu(), ri)


@gpu
@pytest.mark.parametrize("k", [1, 3, 8])
def test_exclude_self_keeps_the_duplicate_and_drops_the_self_pair(pkg, k):
    a, _, _, (rd, ri) = _case("square")
    dev = a.cuda()
    dist, index = pkg.cross_neighbours(dev, dev, k=k, exclude_self=True)
    assert torch.equal(dist.cpu(), rd[:, :k]) and torch.equal(index.cpu(), ri[:, :k])
    assert not bool((index.cpu() == torch.arange(a.shape[0])[:, None]).any())
    assert dist[7, 0] == 0 and index[7, 0] == 200 and dist[200, 0] == 0 and index[200, 0] == 7 and index[258, 0] == 0
    plain = pkg.cross_neighbours(dev, dev, k=1)
    assert torch.equal(plain[0].cpu(), torch.zeros((259, 1), dtype=torch.int32))
    assert plain[1].cpu()[:, 0].tolist() == [min(i, {200: 7, 101: 100, 258: 0}.get(i, i)) for i in range(259)]


@gpu
@pytest.mark.parametrize("name", list(SHAPES) + ["square"])
def test_ball_counts_inclusive_and_exact(pkg, name):
    a, b, d, _ = _case(name)
    excl = name == "square"
    da, db = a.cuda(), b.cuda()
    Nb = b.shape[0]
    for dtype in (torch.int32, torch.int64):
        radius = _radii(d, 50).to(dtype)
        ref = ball_counts_ref(a, b, radius, excl)
        got = pkg.ball_counts(da, db, radius.cuda(), exclude_self=excl)
        assert got.dtype == torch.int32 and got.shape == (a.shape[0],)
        assert torch.equal(got.cpu(), ref)
    assert int(ref.sum()) > Nb                                          # the radii do catch something
    zero = pkg.ball_counts(da, db, torch.zeros(Nb, dtype=torch.int32, device="cuda"), exclude_self=excl)
    assert torch.equal(zero.cpu(), ball_counts_ref(a, b, torch.zeros(Nb, dtype=torch.int64), excl))
    if name in ("tie", "square"):
        assert int(zero.sum()) > 0                                      # distance 0 lies inside a ball of radius 0
    for big in (torch.full((Nb,), int(d.max()), dtype=torch.int32), torch.full((Nb,), 2 ** 40, dtype=torch.int64)):
        every = pkg.ball_counts(da, db, big.cuda(), exclude_self=excl)
        assert torch.equal(every.cpu(), torch.full((a.shape[0],), Nb - 1 if excl else Nb, dtype=torch.int32))


@gpu
@pytest.mark.parametrize("name", ["tail784", "ranges", "square"])
def test_a_combined_call_returns_the_bits_of_the_two_separate_calls(pkg, name):
    a, b, d, (rd, ri) = _case(name)
    excl = name == "square"
    S = _S()
    da, db, radius = a.cuda(), b.cuda(), _radii(d, 51).to(torch.int32).cuda()
    dist, index, count = S._cross_launch(da, db, 3, excl, radius)
    d_only, i_only = pkg.cross_neighbours(da, db, k=3, exclude_self=excl)
    c_only = pkg.ball_counts(da, db, radius, exclude_self=excl)
    assert torch.equal(dist, d_only) and torch.equal(index, i_only) and torch.equal(count, c_only)
    assert torch.equal(dist.cpu(), rd[:, :3]) and torch.equal(count.cpu(), ball_counts_ref(a, b, radius.cpu(), excl))


@gpu
@pytest.mark.parametrize("name", ["tie", "maxd", "tail784"])
def test_up_to_64_rows_equal_nearest_frames(pkg, name):
    a, b, _, _ = _case(name)
    a = a[:64]
    k = 5
    dist, index = pkg.cross_neighbours(a.cuda(), b.cuda(), k=k)
    nd, ni = pkg.nearest_frames(a.cuda(), b.cuda().unsqueeze(1), k=k)
    assert torch.equal(dist, nd) and torch.equal(index, ni)


@gpu
def test_same_bits_every_run(pkg):
    a, b, d, _ = _case("ranges")
    S = _S()
    da, db, radius = a.cuda(), b.cuda(), _radii(d, 52).to(torch.int32).cuda()
    first = S._cross_launch(da, db, 8, False, radius)
    second = S._cross_launch(da, db, 8, False, radius)
    assert all(torch.equal(x, y) for x, y in zip(first, second))


@gpu
def test_nothing_is_written_outside_the_outputs_and_the_scratch(pkg):
    """out_dist, out_index, out_count and a scratch of exactly mmvae_knn_cross_scratch_bytes are carved out of one buffer filled with
    0xA5, 256 guard bytes between and around them; afterwards every guard byte is intact and every output element was written."""
    L = _L()
    a, b, d, (rd, ri) = _case("tail784")
    (Na, D), Nb, k = a.shape, b.shape[0], 3
    da, db, radius = a.cuda(), b.cuda(), _radii(d, 53).to(torch.int32).cuda()
    nbytes = L.lib().mmvae_knn_cross_scratch_bytes(Na, Nb, D, k, 1)
    assert nbytes > 0
    G = 256
    sizes = [Na * k * 4, Na * k * 8, Na * 4, nbytes]
    offs, pos = [], G
    for s in sizes:
        offs.append(pos)
        pos += (s + 255) // 256 * 256 + G
    buf = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    assert base % 16 == 0
    o_dist, o_index, o_count, o_scr = offs
    rc = L.lib().mmvae_knn_cross(da.data_ptr(), Na, db.data_ptr(), Nb, D, k, 0, base + o_dist, base + o_index, radius.data_ptr(),
                                 base + o_count, base + o_scr, nbytes, L.cur_stream())
    assert rc == 0, L.lib().mmvae_last_error()
    torch.cuda.synchronize()
    host = buf.cpu()
    inside = torch.zeros(pos, dtype=torch.bool)
    for o, s in zip(offs, sizes):
        inside[o:o + s] = True
    assert bool((host[~inside] == 0xA5).all())
    dist = host[o_dist:o_dist + sizes[0]].view(torch.int32).view(Na, k)
    index = host[o_index:o_index + sizes[1]].view(torch.int64).view(Na, k)
    count = host[o_count:o_count + sizes[2]].view(torch.int32)
    assert torch.equal(dist, rd[:, :k]) and torch.equal(index, ri[:, :k])
    assert torch.equal(count, ball_counts_ref(a, b, radius.cpu(), False))
    rc = L.lib().mmvae_knn_cross(da.data_ptr(), Na, db.data_ptr(), Nb, D, k, 0, base + o_dist, base + o_index, radius.data_ptr(),
                                 base + o_count, base + o_scr, nbytes - 1, L.cur_stream())
    assert rc == -3 and str(nbytes) in L.lib().mmvae_last_error().decode()
