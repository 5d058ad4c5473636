"""csrc/k_stylemap.hip (exact t-SNE and k-means in fp32) against the float64 torch references of ``ops.reference``.

Numerics convention (as for tests/test_prosody_transfer_gpu.py): the yardstick of a case is the float32 torch
reference's own deviation from the float64 reference on the same inputs, the maximum over 8 seeds; the kernel may deviate
from float64 by up to 8 times that (hardware log2 / exp2 are about 1 ulp against libm's 0.5; the kernels add in
sequence where torch adds pairwise), with a floor of 2^-20 max(1, max |oracle|).  Every comparison prints its figures
(``TSNENUM`` lines) before it asserts.  The references of a case are computed once and shared; the t-SNE references run
as float64 / float32 torch on the GPU (the same code as on the CPU), the k-means references on the CPU."""
import functools
import math

import pytest
import torch

from stylemap_signals import blob_set, gaussian_blobs, grid_points, knn_purity, points, row_perplexity
from speakingstyle_amd import ops
from speakingstyle_amd.ops import hip
from speakingstyle_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SEEDS = 8
MARGIN = 8.0
NS = (7, 63, 64, 65, 257, 1000)
DS = (1, 3, 80, 512)


def check(tag, name, got, oracle, yard):
    """``got`` (per seed) against ``oracle`` (per seed) on the yardstick ``yard``: print, then assert."""
    top = max(float(o.abs().max()) for o in oracle)
    err = max(float((g.double() - o).abs().max()) for g, o in zip(got, oracle))
    floor = 2.0 ** -20 * max(1.0, top)
    print(f"TSNENUM {tag} {name}: |oracle| {top:.3e} ref32 {yard:.3e} hip {err:.3e} floor {floor:.3e}")
    assert all(bool(torch.isfinite(g).all()) for g in got), (tag, name)
    assert err <= max(MARGIN * yard, floor), (tag, name)


def yardstick(r32, r64):
    return max(float((a.double() - b).abs().max()) for a, b in zip(r32, r64))


# ------------------------------------------------------------------ affinities
def affinity_case(xs, perp, tag):
    """xs: the 8 seeds' float64 inputs on the GPU."""
    c64 = [ref.tsne_conditional(x, perp)[0] for x in xs]
    c32 = [ref.tsne_conditional(x.float(), perp)[0] for x in xs]
    j64 = [(c + c.t()) / (c + c.t()).sum() for c in c64]
    j32 = [(c + c.t()) / (c + c.t()).sum() for c in c32]
    cond = [hip.tsne_affinities(x.float(), perp, joint=False) for x in xs]
    joint = [ops.tsne_affinities(x.float(), perp) for x in xs]
    check(tag, "conditional", cond, c64, yardstick(c32, c64))
    check(tag, "joint", joint, j64, yardstick(j32, j64))
    for p in joint:
        assert p.dtype == torch.float32 and torch.equal(p, p.t()) and float(p.diagonal().abs().max()) == 0.0
        assert abs(float(p.double().sum()) - 1.0) <= 1e-5 and float(p.min()) >= 0.0
    for c in cond:
        h = row_perplexity(c).log()
        # the kernel stops at 1e-5 on its own fp32 evaluation of H <= log 30 = 3.4: 64 sequential terms per thread,
        # an 8-level tree, log2 and the final division, each 2^-24 relative -> under 3e-5 in all, typically 1e-6
        assert float((h - math.log(perp)).abs().max()) <= 1e-5 + 3e-5, tag


@pytest.mark.parametrize("dim", DS)
@pytest.mark.parametrize("n", NS)
def test_affinities_against_float64(n, dim):
    xs = [points(7919 * s + 31 * n + dim, n, dim).cuda() for s in range(SEEDS)]
    for perp in sorted({2.0, min(30.0, (n - 1) / 3)}):
        affinity_case(xs, perp, f"affinities N={n} D={dim} perplexity={perp:g}")


def test_affinities_of_duplicated_points():
    xs = []
    for s in range(SEEDS):
        x = points(100 + s, 90, 8)
        xs.append(torch.cat([x, x[:40]]).cuda())
    affinity_case(xs, 12.0, "affinities duplicates N=130 D=8")


def test_affinities_where_unshifted_float32_exponentials_underflow():
    xs = [points(200 + s, 257, 32, scale=30.0).cuda() for s in range(SEEDS)]
    assert float(ref.pairwise_sqdist(xs[0]).max()) > 1e4  # exp(-1e4) is zero in float32 and in float64
    affinity_case(xs, 20.0, "affinities scale=30 N=257 D=32")


# ------------------------------------------------------------------ gradient, KL, one step
@functools.lru_cache(maxsize=None)
def gradient_inputs(n, scale):
    out = []
    for s in range(SEEDS):
        P = ref.tsne_affinities(points(4001 * s + n, n, 3).cuda(), min(30.0, (n - 1) / 3))
        y = (points(17 * s + n + 5, n, 2) * scale / 3.0).cuda()
        out.append((P, y))
    return out


@pytest.mark.parametrize("scale", [1e-4, 10.0])
@pytest.mark.parametrize("n", NS)
def test_gradient_and_kl_against_float64(n, scale):
    cases = gradient_inputs(n, scale)
    for ex in (1.0, 12.0):
        r64 = [ref.tsne_gradient(P, y, ex) for P, y in cases]
        r32 = [ref.tsne_gradient(P.float(), y.float(), ex) for P, y in cases]
        got = [ops.tsne_gradient(P.float(), y.float(), ex) for P, y in cases]
        for k, name in enumerate(("attr", "rep", "zrow", "grad")):
            assert got[0][k].shape == r64[0][k].shape and got[0][k].dtype == torch.float32
            check(f"gradient N={n} y~{scale:g} exaggeration={ex:g}", name, [g[k] for g in got], [r[k] for r in r64],
                  yardstick([r[k] for r in r32], [r[k] for r in r64]))
    k64 = [ref.tsne_kl(P, y).reshape(1) for P, y in cases]
    k32 = [ref.tsne_kl(P.float(), y.float()).reshape(1) for P, y in cases]
    got = [ops.tsne_kl(P.float(), y.float()).reshape(1) for P, y in cases]
    check(f"kl N={n} y~{scale:g}", "kl", got, k64, yardstick(k32, k64))


@pytest.mark.parametrize("n", NS)
def test_one_update_step_against_float64(n):
    cases = gradient_inputs(n, 10.0)
    lr, mom, ex = ref.tsne_learning_rate(n), 0.8, 12.0
    states = []
    for s, (P, y) in enumerate(cases):
        g = torch.Generator().manual_seed(300 + s)
        upd = torch.randn(n, 2, generator=g, dtype=torch.float64).cuda()
        gains = (0.01 + 2.0 * torch.rand(n, 2, generator=g, dtype=torch.float64)).cuda()
        states.append((upd, gains))

    def step(P, y, upd, gains):
        return ref.tsne_step(ref.tsne_gradient(P, y, ex)[3], y, upd, gains, mom, lr)

    r64 = [step(P, y, u, g) for (P, y), (u, g) in zip(cases, states)]
    r32 = [step(P.float(), y.float(), u.float(), g.float()) for (P, y), (u, g) in zip(cases, states)]
    got = [hip.tsne_step(P.float(), y.float(), u.float(), g.float(), ex, mom, lr) for (P, y), (u, g) in zip(cases, states)]
    for k, name in enumerate(("y", "update", "gains")):
        check(f"step N={n}", name, [g[k] for g in got], [r[k] for r in r64],
              yardstick([r[k] for r in r32], [r[k] for r in r64]))


# ------------------------------------------------------------------ the whole descent
KW = dict(perplexity=30.0, n_iter=500, exag_iter=250, kl_every=50)


@functools.lru_cache(maxsize=None)
def blob_reference_kls():
    """S: the final KL of the float64 reference, of the float32 reference and of 4 float64 runs from starts perturbed
    by 1e-9."""
    x, _ = blob_set(0)
    xg = x.cuda()
    y0 = ref.tsne_init(xg, "pca")
    S = [ref.tsne(xg, **KW)[1][-1], ref.tsne(xg.float(), **KW)[1][-1]]
    for s in range(4):
        g = torch.Generator().manual_seed(50 + s)
        jog = y0 + 1e-9 * torch.randn(300, 2, generator=g, dtype=torch.float64).cuda()
        S.append(ref.tsne(xg, init=jog, **KW)[1][-1])
    return S


def test_tsne_on_the_blob_set():
    x, labels = blob_set(0)
    S = blob_reference_kls()
    y, trace = ops.tsne(x.float().cuda(), **KW)
    again = ops.tsne(x.float().cuda(), **KW)
    purity = knn_purity(y, labels)
    bound = max(S) + (max(S) - min(S))
    print(f"TSNENUM tsne blobs: S {[round(v, 5) for v in S]} bound {bound:.5f} hip final KL {trace[-1]:.5f} "
          f"purity {purity:.4f} trace {[round(v, 4) for v in trace]}")
    assert y.dtype == torch.float32 and y.is_cuda and y.shape == (300, 2) and len(trace) == 10
    assert torch.equal(y, again[0]) and trace == again[1]
    assert all(b <= a for a, b in zip(trace[4:], trace[5:]))
    assert purity >= 0.99
    assert trace[-1] <= bound


# ------------------------------------------------------------------ k-means
@pytest.mark.parametrize("dim", [1, 80, 512])
@pytest.mark.parametrize("k", [1, 2, 64])
@pytest.mark.parametrize("n", [64, 65, 1000])
def test_kmeans_on_integer_grids_is_the_float32_reference_bitwise(n, k, dim):
    x = grid_points(1000 * n + 10 * k + dim, n, dim).float()
    labels, cent, its = ref.kmeans(x, k)
    got = ops.kmeans(x.cuda(), k)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[1].shape == (k, dim)
    assert got[2] == its
    assert torch.equal(got[0].cpu(), labels)
    assert torch.equal(got[1].cpu(), cent)
    again = ops.kmeans(x.cuda(), k)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    capped = ops.kmeans(x.cuda(), k, n_iter=1)
    one = ref.kmeans(x, k, n_iter=1)
    assert capped[2] == 1 and torch.equal(capped[0].cpu(), one[0]) and torch.equal(capped[1].cpu(), one[1])


def test_kmeans_on_blobs_against_float64():
    sets = [gaussian_blobs(60 + s, 6, 50, 32)[0] for s in range(SEEDS)] + \
           [gaussian_blobs(80 + s, 5, 77, 200)[0] for s in range(SEEDS)]
    for group, k in ((sets[:SEEDS], 6), (sets[SEEDS:], 5)):
        r64 = [ref.kmeans(x, k) for x in group]
        r32 = [ref.kmeans(x.float(), k) for x in group]
        got = [ops.kmeans(x.float().cuda(), k) for x in group]
        for g, r in zip(got, r64):
            assert torch.equal(g[0].cpu(), r[0]) and g[2] == r[2]
        check(f"kmeans blobs N={group[0].shape[0]} D={group[0].shape[1]} k={k}", "centroids",
              [g[1].cpu() for g in got], [r[1] for r in r64], yardstick([r[1] for r in r32], [r[1] for r in r64]))


# ------------------------------------------------------------------ limits
def test_limits_are_refused_on_the_gpu():
    with pytest.raises(ValueError, match="TSNE_MAX_N"):
        ops.tsne_affinities(torch.zeros(ref.TSNE_MAX_N + 1, 2, device="cuda"), 30.0)
    with pytest.raises(ValueError, match="TSNE_MAX_N"):
        ops.tsne(torch.zeros(ref.TSNE_MAX_N + 1, 2, device="cuda"))
    with pytest.raises(ValueError, match="perplexity"):
        ops.tsne_affinities(torch.zeros(30, 2, device="cuda"), 10.0)
    with pytest.raises(ValueError, match="perplexity"):
        ops.tsne_affinities(torch.zeros(30, 2, device="cuda"), 1.0)
    with pytest.raises(ValueError, match="N = 6"):
        ops.tsne(torch.zeros(6, 2, device="cuda"), 2.0)
    for shape, k, word in (((10, 4), 0, "k = 0"), ((10, 4), 65, "k = 65"), ((10, 4), 11, "exceeds N"),
                           ((10, 513), 2, "D = 513")):
        with pytest.raises(ValueError, match=word):
            ops.kmeans(torch.zeros(*shape, device="cuda"), k)


def test_the_largest_problem_runs():
    """N = TSNE_MAX_N = 16384: the distance row fills the 64 KiB of LDS the perplexity kernel asks for."""
    n = ref.TSNE_MAX_N
    x = points(9, n, 3).float().cuda()
    cond = hip.tsne_affinities(x, 30.0, joint=False)
    rows = torch.arange(0, n, n // 64)[:64]
    h = row_perplexity(cond[rows.cuda()].cpu()).log()
    worst = float((h - math.log(30.0)).abs().max())
    print(f"TSNENUM largest N={n}: worst |H - log 30| over 64 rows {worst:.3e}")
    assert float(cond[rows.cuda(), rows.cuda()].abs().max()) == 0.0
    assert worst <= 1e-5 + 3e-5  # the bound of affinity_case
    del cond
    P = ops.tsne_affinities(x, 30.0)
    assert abs(float(P.double().sum()) - 1.0) <= 1e-5
    sub = P[:512, :512]
    assert torch.equal(sub, sub.t()) and torch.equal(P[rows.cuda()][:, 16000:], P[16000:][:, rows.cuda()].t())
