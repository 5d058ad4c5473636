"""csrc/k_dtw.hip against ``ops.reference.dtw`` in float64, at the lane, strip and block edges of the kernel.

Cost bound: relative (Tx + Ty + D + 8) * 2^-23.  The total is a sum of at most Tx + Ty - 1 non-negative fp32 local
costs (one rounding per path cell, a min adds none) and each local cost is a square root of a sum of D non-negative
squares; the bound is that rounding budget, not a measured figure.  Every comparison prints its figures (``DTWNUM``
lines) and also holds the CPU fp32 reference to the bound, so the yardstick is known to be rounding-level.  Paths are
judged by validity and by their float64 cost (a near-tie may pick another path of equal cost); the integer-valued
tie cases are exact in fp32 and must match the reference path cell for cell."""
import functools

import pytest
import torch

from speakingstyle_amd import ops
from speakingstyle_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 13), (1, 7, 13), (7, 1, 13), (2, 2, 1), (63, 65, 13), (64, 64, 80), (65, 130, 13), (129, 70, 80),
          (257, 300, 13)]
TIE_SHAPES = [(5, 9), (64, 65), (130, 67)]
STEPS = ((1, 1), (1, 0), (0, 1))


def bound(Tx, Ty, D):
    return (Tx + Ty + D + 8) * 2.0 ** -23


@functools.lru_cache(maxsize=None)
def inputs(Tx, Ty, D):
    """Speech-like pairs above 8 frames (y = a time-warped copy of x + 0.3 * noise), random ones below."""
    g = torch.Generator().manual_seed(Tx * 100003 + Ty * 101 + D)
    x = torch.randn(Tx, D, generator=g)
    if max(Tx, Ty) <= 8:
        return x, torch.randn(Ty, D, generator=g)
    src = torch.round(torch.arange(Ty, dtype=torch.float64) * ((Tx - 1) / max(Ty - 1, 1))).long()
    return x, x[src] + 0.3 * torch.randn(Ty, D, generator=g)


@functools.lru_cache(maxsize=None)
def oracle(Tx, Ty, D):
    """(float64 cost, CPU fp32 cost, float64 local costs) of a case, computed once."""
    x, y = inputs(Tx, Ty, D)
    c64 = float(ref.dtw(x.double(), y.double(), [Tx], [Ty])[0][0])
    c32 = float(ref.dtw(x, y, [Tx], [Ty])[0][0])
    d = x.double().unsqueeze(1) - y.double().unsqueeze(0)
    return c64, c32, torch.sqrt((d * d).sum(-1))


def tie_inputs(Tx, Ty, dtype):
    g = torch.Generator().manual_seed(Tx * 1000 + Ty)
    x = torch.randint(0, 3, (Tx, 1), generator=g).to(dtype)
    y = torch.randint(0, 3, (Ty, 1), generator=g).to(dtype)
    return x, y


def check_path(path, plen, Tx, Ty):
    n = int(plen)
    assert max(Tx, Ty) <= n <= Tx + Ty - 1
    cells = path[:n].tolist()
    assert cells[0] == [0, 0] and cells[-1] == [Tx - 1, Ty - 1]
    for a, b in zip(cells, cells[1:]):
        assert (b[0] - a[0], b[1] - a[1]) in STEPS, (a, b)
    assert bool((path[n:] == -1).all())
    return cells


def packed(cases):
    xs, ys = zip(*(inputs(*c) for c in cases))
    return torch.cat(xs).cuda(), torch.cat(ys).cuda(), [c[0] for c in cases], [c[1] for c in cases]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_cost_and_path(case):
    Tx, Ty, D = case
    x, y = inputs(*case)
    c64, c32, local = oracle(*case)
    cost, path, plen = ops.dtw(x.cuda(), y.cuda(), [Tx], [Ty])
    assert cost.is_cuda and path.is_cuda and plen.is_cuda
    assert cost.dtype == torch.float32 and path.dtype == torch.int32 and plen.dtype == torch.int32
    assert path.shape == (1, Tx + Ty - 1, 2)
    tol = bound(*case) * max(c64, 1e-30)
    cells = check_path(path[0].cpu(), plen[0], Tx, Ty)
    along = float(sum(local[i, j] for i, j in cells))
    print(f"DTWNUM cost Tx={Tx} Ty={Ty} D={D} float64={c64:.9e} cpu_fp32_err={abs(c32 - c64) / max(c64, 1e-30):.3e} "
          f"hip_err={abs(float(cost[0]) - c64) / max(c64, 1e-30):.3e} path_err={abs(along - c64) / max(c64, 1e-30):.3e} "
          f"bound={bound(*case):.3e} path_len={int(plen[0])}")
    assert abs(c32 - c64) <= tol      # the yardstick itself is rounding-level
    assert abs(float(cost[0]) - c64) <= tol
    assert abs(along - c64) <= tol    # the kernel's path is an optimal one up to rounding


@pytest.mark.parametrize("shape", TIE_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_integer_ties_match_the_reference_path(shape):
    Tx, Ty = shape
    x, y = tie_inputs(Tx, Ty, torch.float32)
    c_ref, p_ref, l_ref = ref.dtw(x.double(), y.double(), [Tx], [Ty])
    cost, path, plen = ops.dtw(x.cuda(), y.cuda(), [Tx], [Ty])
    print(f"DTWNUM ties Tx={Tx} Ty={Ty} float64={float(c_ref[0])} hip={float(cost[0])} path_len={int(plen[0])}")
    assert float(cost[0]) == float(c_ref[0])  # differences, squares and |d| are exact in fp32 here
    assert torch.equal(plen.cpu(), l_ref) and torch.equal(path.cpu(), p_ref)


def test_batch_is_bitwise_each_pair_alone_and_repeatable():
    cases = [(Tx, Ty, 13) for Tx, Ty, _ in SHAPES]
    x, y, xl, yl = packed(cases)
    cost, path, plen = ops.dtw(x, y, xl, yl)
    again = ops.dtw(x, y, xl, yl)
    for a, b in zip((cost, path, plen), again):
        assert torch.equal(a, b)
    assert path.shape == (len(cases), max(xl) + max(yl) - 1, 2)
    for p, case in enumerate(cases):
        xa, ya = inputs(*case)
        c1, p1, l1 = ops.dtw(xa.cuda(), ya.cuda(), [case[0]], [case[1]])
        n = int(l1[0])
        assert torch.equal(c1[0], cost[p]) and n == int(plen[p]), case
        assert torch.equal(p1[0, :n], path[p, :n]) and bool((path[p, n:] == -1).all()), case


def test_chunked_by_the_workspace_budget_is_bitwise_the_same():
    cases = [(Tx, Ty, 13) for Tx, Ty, _ in SHAPES]
    x, y, xl, yl = packed(cases)
    assert sum(a * b for a, b in zip(xl, yl)) > 50000
    whole = ops.dtw(x, y, xl, yl)
    for budget in (50000, 1):  # a few pairs per launch; one pair per launch
        for a, b in zip(whole, ops.dtw(x, y, xl, yl, plane_budget=budget)):
            assert torch.equal(a, b), budget


def test_plane_size_matches_the_kernel_library():
    from speakingstyle_amd.ops import hip

    for Tx, Ty, _ in SHAPES + [(800, 850, 13), (64, 1, 1), (1, 64, 1)]:
        assert hip.dtw_plane_bytes(Tx, Ty) == int(hip.lib().ssamd_dtw_plane_bytes(Tx, Ty))


def test_reference_backend_on_device_tensors_agrees():
    case = (65, 130, 13)
    x, y = inputs(*case)
    c64 = oracle(*case)[0]
    got = ops.dtw(x.cuda(), y.cuda(), [case[0]], [case[1]])
    ops.set_backend("reference")
    try:
        want = ops.dtw(x.cuda(), y.cuda(), [case[0]], [case[1]])
    finally:
        ops.set_backend(None)
    assert all(t.is_cuda for t in got + want)
    assert abs(float(got[0][0]) - float(want[0][0])) <= bound(*case) * c64
    check_path(want[1][0].cpu(), want[2][0], case[0], case[1])


def test_rejected_inputs():
    x = torch.zeros(4, 13, device="cuda")
    with pytest.raises(ValueError):
        ops.dtw(x, x, [4, 0], [3, 1])
    with pytest.raises(ValueError):
        ops.dtw(torch.zeros(4, 81, device="cuda"), torch.zeros(4, 81, device="cuda"), [4], [4])
    with pytest.raises(TypeError):
        ops.dtw(x.double(), x.double(), [4], [4])


def test_long_y_takes_the_large_lds_path():
    # Ty floats of strip hand-over plus the y ring pass 64 KiB of LDS: the launch opts in to the larger allocation.
    # One x row has a closed form: every move is (i, j-1), the cost is sum_j |x0 - y_j|.
    Ty = 15000
    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(1, 1, generator=g), torch.randn(Ty, 1, generator=g)
    cost, path, plen = ops.dtw(x.cuda(), y.cuda(), [1], [Ty])
    want = float((x.double() - y.double()).abs().sum())
    print(f"DTWNUM long Ty={Ty} float64={want:.9e} hip_err={abs(float(cost[0]) - want) / want:.3e} "
          f"bound={bound(1, Ty, 1):.3e}")
    assert abs(float(cost[0]) - want) <= bound(1, Ty, 1) * want
    assert int(plen[0]) == Ty and path.shape == (1, Ty, 2)
    assert bool((path[0, :, 0] == 0).all()) and torch.equal(path[0, :, 1].cpu(), torch.arange(Ty, dtype=torch.int32))
