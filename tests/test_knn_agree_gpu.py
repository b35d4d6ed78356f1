"""GPU: the two exact k-NN paths agree.  nearest_frames (no lut) and cross_neighbours share the key, the k-best list, the tie rule and
the merge round (csrc/knn_select.hpp); on the same bytes both must return the bits of the CPU reference, hence each other's.  The
shapes are the smallest that reach each mechanism of both kernels."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from knn_ref import knn_cross_ref, tie_case  # noqa: E402

gpu = pytest.mark.gpu
# (M, F, D, k).  tie: planted ties, a zero distance at two indices, a single quarter k step.  (17, 33, 208): a row past one 16-row tile,
# one frame past two column tiles, one 128-byte line + a 64-byte step + a quarter step.  (64, 300, 784): all four row tiles of the scan,
# columns across three 128-column tiles of the sweep, the quarter-full last k step.  (3, 8, 256): F == k, every column is returned and
# both merges meet their unused slots.
CASES = [("tie", 1), ("tie", 8), ((17, 33, 208), 8), ((64, 300, 784), 5), ((3, 8, 256), 8)]


def _bytes(shape):
    if shape == "tie":
        return tie_case()
    M, F, D = shape
    g = torch.Generator().manual_seed(1000 * M + F)
    return torch.randint(0, 256, (M, D), dtype=torch.uint8, generator=g), torch.randint(0, 256, (F, D), dtype=torch.uint8, generator=g)


@gpu
@pytest.mark.parametrize("shape,k", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_nearest_frames_and_cross_neighbours_return_the_same_bits(pkg, shape, k):
    q, f = _bytes(shape)
    want_d, want_i = knn_cross_ref(q, f, k)
    dq, df = q.cuda(), f.cuda()
    nd, ni = pkg.nearest_frames(dq, df.unsqueeze(1), k=k)           # frames as [F, 1, D]: planes of 1 x D
    cd, ci = pkg.cross_neighbours(dq, df, k=k)
    assert nd.dtype == cd.dtype == torch.int32 and ni.dtype == ci.dtype == torch.int64 and nd.shape == cd.shape == (q.shape[0], k)
    assert torch.equal(nd, cd) and torch.equal(ni, ci)
    assert torch.equal(nd.cpu(), want_d) and torch.equal(ni.cpu(), want_i)
    assert torch.equal(cd.cpu(), want_d) and torch.equal(ci.cpu(), want_i)
