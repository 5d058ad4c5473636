"""``ops.reference.dtw`` (the CPU path and the oracle of csrc/k_dtw.hip): brute force over every warping path,
path validity, the tie rule, identity, and a mixed-length batch against each pair alone."""
import itertools

import numpy as np
import pytest
import torch

from speakingstyle_amd import ops
from speakingstyle_amd.ops import reference as ref

STEPS = ((1, 1), (1, 0), (0, 1))
TIE_SHAPES = [(5, 9), (64, 65), (130, 67)]


def local_cost(x, y):
    d = x.double().unsqueeze(1) - y.double().unsqueeze(0)
    return torch.sqrt((d * d).sum(-1)).numpy()


def check_path(path, plen, Tx, Ty):
    """A valid warping path of its stated length, padded with -1."""
    n = int(plen)
    cells = path[:n].tolist()
    assert cells[0] == [0, 0] and cells[-1] == [Tx - 1, Ty - 1]
    for a, b in zip(cells, cells[1:]):
        assert (b[0] - a[0], b[1] - a[1]) in STEPS, (a, b)
    assert max(Tx, Ty) <= n <= Tx + Ty - 1
    assert bool((path[n:] == -1).all())
    return cells


def brute_force(c):
    """Cheapest warping path of a small cost matrix by enumerating all of them."""
    Tx, Ty = c.shape
    best = [np.inf]

    def walk(i, j, acc):
        acc += c[i, j]
        if i == Tx - 1 and j == Ty - 1:
            best[0] = min(best[0], acc)
            return
        for di, dj in STEPS:
            if i + di < Tx and j + dj < Ty:
                walk(i + di, j + dj, acc)

    walk(0, 0, 0.0)
    return best[0]


def tie_inputs(Tx, Ty, dtype):
    g = torch.Generator().manual_seed(Tx * 1000 + Ty)
    x = torch.randint(0, 3, (Tx, 1), generator=g).to(dtype)
    y = torch.randint(0, 3, (Ty, 1), generator=g).to(dtype)
    return x, y


@pytest.mark.parametrize("D", [1, 3])
def test_brute_force_small(D):
    g = torch.Generator().manual_seed(D)
    for Tx, Ty in itertools.product(range(1, 6), repeat=2):
        x = torch.randn(Tx, D, generator=g, dtype=torch.float64)
        y = torch.randn(Ty, D, generator=g, dtype=torch.float64)
        cost, path, plen = ref.dtw(x, y, [Tx], [Ty])
        assert cost.dtype == torch.float64 and path.dtype == torch.int32 and plen.dtype == torch.int32
        assert path.shape == (1, Tx + Ty - 1, 2)
        c = local_cost(x, y)
        want = brute_force(c)
        assert abs(float(cost[0]) - want) <= 1e-12 * max(1.0, want), (Tx, Ty)
        cells = check_path(path[0], plen[0], Tx, Ty)
        along = sum(c[i, j] for i, j in cells)
        assert abs(along - want) <= 1e-12 * max(1.0, want), (Tx, Ty)  # the returned path is an optimal one


@pytest.mark.parametrize("shape", TIE_SHAPES)
def test_tie_rule_fp32_equals_float64(shape):
    Tx, Ty = shape
    x, y = tie_inputs(Tx, Ty, torch.float64)
    c64, p64, l64 = ref.dtw(x, y, [Tx], [Ty])
    c32, p32, l32 = ref.dtw(x.float(), y.float(), [Tx], [Ty])
    check_path(p64[0], l64[0], Tx, Ty)
    assert float(c64[0]) == float(c32[0]) == round(float(c64[0]))  # integer costs: exact in both
    assert torch.equal(p64, p32) and torch.equal(l64, l32)


def test_tie_rule_all_equal_3x3():
    x = torch.ones(3, 2)
    cost, path, plen = ref.dtw(x, x.clone(), [3], [3])
    assert int(plen[0]) == 3 and float(cost[0]) == 0.0
    assert path[0, :3].tolist() == [[0, 0], [1, 1], [2, 2]]  # every candidate ties: the diagonal wins
    assert bool((path[0, 3:] == -1).all())


def plain_dtw(c):
    """The recurrence as two plain loops with the tie rule spelled out: diagonal, then (i-1, j), then (i, j-1)."""
    Tx, Ty = c.shape
    A = np.full((Tx, Ty), np.inf)
    back = np.zeros((Tx, Ty), dtype=np.int64)
    for i in range(Tx):
        for j in range(Ty):
            cands = [A[i - 1, j - 1] if i and j else (0.0 if i == j == 0 else np.inf),
                     A[i - 1, j] if i else np.inf, A[i, j - 1] if j else np.inf]
            k = 0
            if cands[1] < cands[k]:
                k = 1
            if cands[2] < cands[k]:
                k = 2
            A[i, j], back[i, j] = c[i, j] + cands[k], k
    i, j, cells = Tx - 1, Ty - 1, []
    while True:
        cells.append([i, j])
        if i == j == 0:
            break
        k = back[i, j]
        i, j = i - (k != 2), j - (k != 1)
    return A[-1, -1], cells[::-1], back


@pytest.mark.parametrize("shape", TIE_SHAPES)
def test_tie_rule_against_plain_loops(shape):
    Tx, Ty = shape
    x, y = tie_inputs(Tx, Ty, torch.float32)
    want, cells, back = plain_dtw(local_cost(x, y))
    cost, path, plen = ref.dtw(x, y, [Tx], [Ty])
    assert float(cost[0]) == want
    assert path[0, :int(plen[0])].tolist() == cells
    # the inputs exercise the rule: the path takes all three moves
    assert {int(back[i, j]) for i, j in cells[1:]} == {0, 1, 2}


def test_self_alignment_is_the_diagonal():
    g = torch.Generator().manual_seed(3)
    for T in (1, 2, 17, 70):
        x = torch.randn(T, 13, generator=g)
        cost, path, plen = ref.dtw(x, x.clone(), [T], [T])
        assert float(cost[0]) == 0.0 and int(plen[0]) == T
        assert torch.equal(path[0, :T, 0], torch.arange(T, dtype=torch.int32))
        assert torch.equal(path[0, :T, 1], torch.arange(T, dtype=torch.int32))


def test_mixed_batch_equals_pairs_alone():
    g = torch.Generator().manual_seed(5)
    shapes = [(1, 1), (9, 4), (1, 6), (30, 41), (5, 1)]
    xs = [torch.randn(a, 7, generator=g) for a, _ in shapes]
    ys = [torch.randn(b, 7, generator=g) for _, b in shapes]
    cost, path, plen = ops.dtw(torch.cat(xs), torch.cat(ys), [a for a, _ in shapes], [b for _, b in shapes])
    assert path.shape == (5, 30 + 41 - 1, 2)
    for p, (x, y) in enumerate(zip(xs, ys)):
        c1, p1, l1 = ref.dtw(x, y, [x.shape[0]], [y.shape[0]])
        assert float(c1[0]) == float(cost[p]) and int(l1[0]) == int(plen[p])
        n = int(l1[0])
        assert torch.equal(p1[0, :n], path[p, :n]) and bool((path[p, n:] == -1).all())
        check_path(path[p], plen[p], x.shape[0], y.shape[0])


def test_zero_length_pair_is_rejected():
    x, y = torch.zeros(3, 2), torch.zeros(3, 2)
    with pytest.raises(ValueError, match="pair 1"):
        ref.dtw(x, y, [3, 0], [2, 1])
    with pytest.raises(ValueError):
        ops.dtw(x, y, [3], [0])
