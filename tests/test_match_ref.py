"""tests/match_ref.py against a brute force over every (cluster, community) pair with
fractions.Fraction, the uniqueness of the pair (inter, csize), the two crafted inputs of the GPU
tests, and fastconsensus_amd.core's helpers against the reference's (no GPU)."""
from fractions import Fraction

import numpy as np
import pytest

from tests import match_ref as mr


def brute(labs, part):
    """Every (k, d) with a common member: the largest Fraction J, among equal J the largest C."""
    labs = np.atleast_2d(labs)
    ids = sorted(set(part.tolist()))
    inter = np.zeros((len(labs), len(ids)), np.int32)
    csize = np.zeros((len(labs), len(ids)), np.int32)
    for r, row in enumerate(labs):
        for i, k in enumerate(ids):
            mem = part == k
            best = None
            for d in set(row.tolist()):
                com = row == d
                c, t = int((mem & com).sum()), int(com.sum())
                if c == 0:
                    continue
                key = (Fraction(c, int(mem.sum()) + t - c), c)
                if best is None or key > best[0]:
                    best = (key, c, t)
                else:
                    assert key != best[0] or t == best[2]           # equal J and equal C force equal t
            inter[r, i], csize[r, i] = best[1], best[2]
    return np.array(ids), np.array([(part == k).sum() for k in ids], np.int64), inter, csize


def random_case(rng):
    n = int(rng.integers(1, 61))
    n_r = int(rng.integers(1, 6))
    part = rng.integers(0, int(rng.integers(1, 8)), n) * int(rng.integers(1, 4))      # sparse ids too
    labs = np.stack([rng.integers(0, int(rng.integers(1, 7)), n) for _ in range(n_r)])
    return labs, part


@pytest.mark.parametrize("seed", range(40))
def test_against_fractions(seed):
    labs, part = random_case(np.random.default_rng(seed))
    for got, exp in zip(mr.match(labs, part), brute(labs, part)):
        assert np.array_equal(got, exp)


def test_many_ties():
    """equal-sized blocks: most clusters have several communities of the same J"""
    rng = np.random.default_rng(1)
    ties = 0
    for _ in range(30):
        part = np.repeat(np.arange(6), 10)
        labs = np.stack([rng.permutation(np.repeat(np.arange(12), 5)) for _ in range(3)])
        got, exp = mr.match(labs, part), brute(labs, part)
        for g, e in zip(got, exp):
            assert np.array_equal(g, e)
        for r in range(3):
            for k in range(6):
                js = [Fraction(int(((part == k) & (labs[r] == d)).sum()),
                               10 + 5 - int(((part == k) & (labs[r] == d)).sum())) for d in range(12)]
                ties += js.count(max(js)) > 1
    assert ties > 100


@pytest.mark.parametrize("seed", range(10))
def test_relabelling_leaves_the_pair(seed):
    rng = np.random.default_rng(100 + seed)
    labs, part = random_case(rng)
    base = mr.match(labs, part)
    perm = rng.permutation(int(labs.max()) + 1)
    again = mr.match(perm[labs], part)
    assert np.array_equal(base[2], again[2]) and np.array_equal(base[3], again[3])
    order = rng.permutation(len(part))                                  # and of the node order
    moved = mr.match(labs[:, order], part[order])
    assert np.array_equal(base[2], moved[2]) and np.array_equal(base[3], moved[3])


@pytest.mark.parametrize("a_low", [True, False])
def test_exact_tie_input(a_low):
    part, lab = mr.exact_tie(16, a_low)
    assert Fraction(1, 4 + 1 - 1) == Fraction(2, 4 + 6 - 2)
    ids, size, inter, csize = mr.match(lab, part)
    assert (size[0], inter[0, 0], csize[0, 0]) == (4, 2, 6)
    assert np.array_equal(brute(lab, part)[2], inter) and np.array_equal(brute(lab, part)[3], csize)
    a, b = lab[0], lab[1]
    assert (a < b) == a_low and (lab == a).sum() == 1 and (lab == b).sum() == 6


def test_near_tie_input():
    part, lab = mr.near_tie()
    c1, u1, c2, u2 = 4000, 8001 + 7998 - 4000, 4001, 8001 + 8002 - 4001
    assert (u1, u2) == (11999, 12002) and c1 * u2 - c2 * u1 == 1
    assert np.float32(c1) / np.float32(u1) == np.float32(c2) / np.float32(u2)     # float32 cannot tell them apart
    assert np.bincount(lab).tolist() == [7998, 8002] and (part == 0).sum() == 8001
    assert np.bincount(lab[part == 0]).tolist() == [4000, 4001]
    ids, size, inter, csize = mr.match(lab, part)
    assert (size[0], inter[0, 0], csize[0, 0]) == (8001, 4000, 7998)
    assert np.all(size[1:] == 1) and np.all(inter[0, 1:] == 1)
    assert np.array_equal(csize[0, 1:], np.bincount(lab)[lab[8001:]])


def test_core_helpers_restate_the_reference():
    from fastconsensus_amd import core
    rng = np.random.default_rng(5)
    for _ in range(20):
        labs, part = random_case(rng)
        ids, size, inter, csize = mr.match(labs, part)
        exp = mr.summary(inter, size, csize)
        got = core.match_summary(inter, size, csize)
        assert sorted(got) == sorted(exp)
        for k in exp:
            assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape and np.all(got[k] == exp[k]), k
        # F1 = 2 J / (1 + J): four roundings of at most half an ulp each on the right-hand side
        assert np.allclose(got["f1"], 2 * got["jaccard"] / (1 + got["jaccard"]), rtol=8 * 2.0 ** -53, atol=0)
        assert np.all(got["recovered"] + got["dissolved"] <= len(labs))
    # the thresholds are integer compares: J = 3/4 counts as recovered, J = 1/2 as dissolved
    assert core.recovered([[3]], [4], [3]).tolist() == [1] and core.recovered([[2]], [3], [3]).tolist() == [0]
    assert core.dissolved([[2]], [4], [2]).tolist() == [1] and core.dissolved([[3]], [5], [3]).tolist() == [0]
    assert core.recovered([[2]], [4], [2], num=1, den=2).tolist() == [1]


def test_two_halves_against_half_the_runs():
    """The issue's motivating pair: a cluster every run splits in two equal halves, and one that
    half the runs contain exactly and the other half shatter, have the same pair-count consensus
    but not the same stability."""
    part = np.zeros(40, np.int64)
    halves = np.stack([np.repeat([0, 1], 20)] * 4)
    exact = np.stack([np.zeros(40, np.int64)] * 2 + [np.arange(40)] * 2)
    a = mr.match(halves, part)
    b = mr.match(exact, part)
    assert mr.stability(a[2], a[1], a[3]).tolist() == [0.5] and mr.recovered(a[2], a[1], a[3]).tolist() == [0]
    assert mr.recovered(b[2], b[1], b[3]).tolist() == [2] and mr.dissolved(b[2], b[1], b[3]).tolist() == [2]
