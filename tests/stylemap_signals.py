"""Deterministic inputs of the style-map tests (tests/test_style_map_cpu.py, tests/test_style_map_gpu.py): every set is
a function of its seed alone, in float64."""
import torch


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def gaussian_blobs(seed, n_blobs, per_blob, dim, centre_std=3.0, scale=1.0):
    """``n_blobs`` unit Gaussians of ``per_blob`` points each, centres N(0, centre_std^2), everything times ``scale``
    -> (x [n_blobs * per_blob, dim], labels); the points are in blob order."""
    g = _gen(seed)
    centres = torch.randn(n_blobs, dim, generator=g, dtype=torch.float64) * centre_std
    x = centres.repeat_interleave(per_blob, 0) + torch.randn(n_blobs * per_blob, dim, generator=g, dtype=torch.float64)
    return x * scale, torch.arange(n_blobs).repeat_interleave(per_blob)


def blob_set(seed=0):
    """The 6 x 50, D = 32 set of the t-SNE acceptance tests."""
    return gaussian_blobs(seed, 6, 50, 32)


def points(seed, n, dim, scale=1.0):
    """n points of a handful of blobs (n need not divide evenly): the affinity and gradient cases."""
    g = _gen(seed)
    nb = max(1, min(5, n // 3))
    centres = torch.randn(nb, dim, generator=g, dtype=torch.float64) * 3.0
    which = torch.randint(0, nb, (n,), generator=g)
    return (centres[which] + torch.randn(n, dim, generator=g, dtype=torch.float64)) * scale


def grid_points(seed, n, dim, side=5):
    """Integer-grid points in [0, side)^dim: sums of them and of their squares are exact in float32, ties are
    common."""
    return torch.randint(0, side, (n, dim), generator=_gen(seed)).to(torch.float64)


def knn_purity(y, labels, k=10):
    """Share of the k nearest neighbours (in the map y) that carry the point's own label."""
    y = y.detach().double().cpu()
    d = torch.cdist(y, y)
    d.fill_diagonal_(float("inf"))
    nn = d.topk(k, largest=False).indices
    return float((labels[nn] == labels[:, None]).double().mean())


def row_perplexity(p_cond):
    """exp(entropy) of every row of a conditional P (zeros skipped)."""
    p = p_cond.double()
    h = -(torch.where(p > 0, p * torch.log(torch.where(p > 0, p, torch.ones_like(p))), torch.zeros_like(p))).sum(1)
    return torch.exp(h)
