"""CPU references of both exact k-NN entry points (mmvae_nearest_frames, mmvae_knn_cross) and of the sample-quality scores built on the
sweep.  Everything is exact: the distances are integers far below 2^53 formed in float64, the scores are ratios of two exact integers
formed in float64."""
import numpy as np
import torch

I64_MAX = torch.iinfo(torch.int64).max


def dist_matrix(a, b, lut=None, chunk=8192):
    """int64 (Na, Nb): |a|^2 + |t(b)|^2 - 2 a t(b)^T in float64 (every value and partial sum stays far below 2^53, so it is exact),
    ``chunk`` rows of ``b`` at a time.  ``lut`` (256 uint8) is t, applied to ``b`` only; every leading axis of ``b`` is flattened."""
    a = a.reshape(a.shape[0], -1).cpu().double()
    b, an, parts = b.reshape(-1, a.shape[1]).cpu(), (a * a).sum(1)[:, None], []
    for lo in range(0, b.shape[0], chunk):
        c = (b[lo:lo + chunk] if lut is None else lut.cpu()[b[lo:lo + chunk].long()]).double()
        parts.append((an + (c * c).sum(1)[None, :] - 2.0 * (a @ c.T)).to(torch.int64))
    return torch.cat(parts, dim=1)


def _masked(a, b, exclude_diagonal, lut=None, chunk=8192):
    d = dist_matrix(a, b, lut, chunk)
    if exclude_diagonal:
        n = min(d.shape)
        d[torch.arange(n), torch.arange(n)] = I64_MAX
    return d


def knn_cross_ref(a, b, k, exclude_diagonal=False, lut=None, chunk=8192):
    """(dist int32 (Na, k), index int64 (Na, k)): the diagonal set to the int64 maximum when excluded, a STABLE sort along the columns
    (equal distances keep the lower index first), the first k."""
    sd, idx = torch.sort(_masked(a, b, exclude_diagonal, lut, chunk), dim=1, stable=True)
    return sd[:, :k].to(torch.int32).contiguous(), idx[:, :k].contiguous()


def ball_counts_ref(a, b, radius, exclude_diagonal=False):
    """int32 (Na,): #{ j : d(i, j) <= radius[j] }, the pair (i, i) left out when excluded (its distance is the int64 maximum)."""
    d = _masked(a, b, exclude_diagonal)
    return (d <= radius.cpu().to(torch.int64)[None, :]).sum(1).to(torch.int32)


def knn_cross_brute(a, b, k, exclude_diagonal=False, radius=None, lut=None):
    """The definition itself: an int64 double loop, then the k smallest (d, j) pairs.  (dist, index, count or None)."""
    a = a.reshape(a.shape[0], -1).tolist()
    b, t = b.reshape(-1, len(a[0])).tolist(), list(range(256)) if lut is None else lut.tolist()
    dist, index, count = [], [], []
    for i, ra in enumerate(a):
        pairs = [(sum((x - t[y]) ** 2 for x, y in zip(ra, rb)), j) for j, rb in enumerate(b) if not (exclude_diagonal and i == j)]
        best = sorted(pairs)[:k]
        dist.append([p[0] for p in best])
        index.append([p[1] for p in best])
        if radius is not None:
            count.append(sum(1 for d, j in pairs if d <= int(radius[j])))
    return (torch.tensor(dist, dtype=torch.int32).reshape(len(a), k), torch.tensor(index, dtype=torch.int64).reshape(len(a), k),
            torch.tensor(count, dtype=torch.int32) if radius is not None else None)


def sample_quality_ref(real, fake, k):
    """The scores of ``sample_quality`` restated on the pooled distance matrix of cat(real, fake), in numpy: a dict of float64."""
    nr, nf = real.shape[0], fake.shape[0]
    pooled = torch.cat([real.reshape(nr, -1).cpu(), fake.reshape(nf, -1).cpu()])
    d = dist_matrix(pooled, pooled).numpy()
    n = nr + nf
    is_real = np.arange(n) < nr
    loo = d.copy()
    loo[np.arange(n), np.arange(n)] = np.iinfo(np.int64).max
    # NND_k(x in S): the k-th smallest distance from x to the other points of its own set
    nnd = np.empty(n, dtype=np.int64)
    nnd[:nr] = np.sort(loo[:nr, :nr], axis=1)[:, k - 1]
    nnd[nr:] = np.sort(loo[nr:, nr:], axis=1)[:, k - 1]
    d_fr, d_rf = d[nr:, :nr], d[:nr, nr:]                     # rows: samples against real frames; real frames against samples
    f_in_r = d_fr <= nnd[:nr][None, :]                        # d(f, r) <= NND_k(r)
    r_in_f = d_rf <= nnd[nr:][None, :]                        # d(r, f) <= NND_k(f)
    # leave-one-out 1-NN on the pooled set: the nearest other point in the order (d, pooled index); a stable argsort is that order
    nearest = np.argsort(loo, axis=1, kind="stable")[:, 0]
    right = is_real[nearest] == is_real
    f64 = np.float64
    return {"precision": f64(f_in_r.any(1).sum()) / f64(nf), "recall": f64(r_in_f.any(1).sum()) / f64(nr),
            "density": f64(f_in_r.sum()) / f64(k * nf), "coverage": f64((d_rf.min(1) <= nnd[:nr]).sum()) / f64(nr),
            "accuracy": f64(right.sum()) / f64(n), "accuracy_real": f64(right[:nr].sum()) / f64(nr),
            "accuracy_fake": f64(right[nr:].sum()) / f64(nf)}


def tie_case():
    """(a (5, 16), b (37, 16)) random bytes with a planted tie between two columns, four identical columns and a row of ``a`` that
    equals two columns (distance 0 at two indices)."""
    g = torch.Generator().manual_seed(4)
    a = torch.randint(0, 256, (5, 16), dtype=torch.uint8, generator=g)
    b = torch.randint(0, 256, (37, 16), dtype=torch.uint8, generator=g)
    b[20], b[3], b[30] = b[11], a[2], a[2]
    b[5:9] = torch.tensor([0, 255] * 8, dtype=torch.uint8)
    return a, b
