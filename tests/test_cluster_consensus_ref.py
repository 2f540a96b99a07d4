"""tests/cluster_consensus_ref.py (the contingency identities) against the brute-force sums over
the co-association matrix of tests/coassoc_ref.py, and its invariants.  CPU only."""
import numpy as np
import pytest

from tests import cluster_consensus_ref as ccr
from tests import coassoc_ref as car
from tests import consensus_ref as cr
from tests import golden_io


def brute(labs, part):
    """pairs and item from the full matrix"""
    part = np.asarray(part)
    full = car.matrix(labs, np.arange(len(part))).astype(np.int64)
    ids = np.unique(part)
    same = part[:, None] == part[None, :]
    item = (full * same).sum(1)
    pairs = np.array([full[np.ix_(part == c, part == c)].sum() for c in ids], np.int64)
    return ids, pairs, item


def consensus_labels(case, labs, theta=0.5):
    u, v = cr.canonical_edges(case.edges_file[:, 0], case.edges_file[:, 1])
    return cr.partition(case.N, u, v, theta, labels=labs)["labels"]


def check_invariants(labs, part):
    n_r = len(labs)
    ids, size, pairs, item = ccr.sums(labs, part)
    assert pairs.dtype == np.int64 and item.dtype == np.int64
    assert int(item.sum()) == int(pairs.sum())
    assert np.all(n_r * size <= pairs) and np.all(pairs <= n_r * size * size)
    assert np.array_equal(size, np.bincount(np.searchsorted(ids, part)))
    return ids, size, pairs, item


@pytest.mark.parametrize("batch", [0, -1])
def test_lfr1k_against_the_matrix(batch):
    case = golden_io.load("lfr1k_louvain_np20")
    labs = case.cd_batches[batch]
    for part in (consensus_labels(case, labs), labs[0]):
        ids, size, pairs, item = check_invariants(labs, part)
        bids, bpairs, bitem = brute(labs, part)
        assert np.array_equal(ids, bids) and np.array_equal(pairs, bpairs) and np.array_equal(item, bitem)


def test_karate_against_the_matrix():
    case = golden_io.load("karate_louvain_np50")
    for batch in (0, -1):
        labs = case.cd_batches[batch]
        for part in (consensus_labels(case, labs), labs[0], np.arange(case.N) % 3 * 11 + 2):
            ids, size, pairs, item = check_invariants(labs, part)
            bids, bpairs, bitem = brute(labs, part)
            assert np.array_equal(ids, bids) and np.array_equal(pairs, bpairs) and np.array_equal(item, bitem)


def test_partition_equal_to_every_replica():
    part = np.random.default_rng(1).integers(0, 7, 300)
    labs = np.stack([part * 3 + 1] * 5)                       # the same partition under other label values
    _, size, pairs, item = check_invariants(labs, part)
    assert np.array_equal(pairs, 5 * size * size)
    assert np.array_equal(item, 5 * size[part])
    cc = ccr.cluster_consensus(pairs, size, 5)
    assert np.all(cc[size > 1] == 1.0)


def test_singletons():
    labs = np.random.default_rng(2).integers(0, 4, (6, 50))
    ids, size, pairs, item = check_invariants(labs, np.arange(50))
    assert len(ids) == 50 and np.all(size == 1)
    assert np.array_equal(pairs, np.full(50, 6)) and np.array_equal(item, np.full(50, 6))
    assert np.all(np.isnan(ccr.cluster_consensus(pairs, size, 6)))
    assert np.all(np.isnan(ccr.item_consensus(item, size, 6)))


def test_normalisation_is_the_mean_off_diagonal_entry():
    labs = np.random.default_rng(3).integers(0, 3, (9, 120))
    part = np.random.default_rng(4).integers(0, 5, 120) * 10
    ids, size, pairs, item = ccr.sums(labs, part)
    full = car.matrix(labs, np.arange(120)).astype(np.float64) / 9
    cc = ccr.cluster_consensus(pairs, size, 9)
    ic = ccr.item_consensus(item, size[np.searchsorted(ids, part)], 9)
    for j, c in enumerate(ids):
        mem = np.flatnonzero(part == c)
        sub = full[np.ix_(mem, mem)]
        off = (sub.sum() - np.trace(sub)) / (len(mem) * (len(mem) - 1))
        assert abs(cc[j] - off) < 1e-12
        for v in mem[:5]:
            assert abs(ic[v] - (full[v, mem].sum() - 1.0) / (len(mem) - 1)) < 1e-12
    assert np.array_equal(ccr.item_sums(car.matrix, labs, np.arange(120), part, ids)[np.arange(120),
                                                                                    np.searchsorted(ids, part)], item)


def test_package_normalisation_equals_the_reference():
    from fastconsensus_amd import core
    rng = np.random.default_rng(5)
    size = rng.integers(1, 40, 200)
    size[:10] = 1
    for nt in (1, 7, 20, 2048):
        pairs = np.array([rng.integers(nt * s, nt * s * s + 1) for s in size], np.int64)
        item = np.array([rng.integers(nt, nt * s + 1) for s in size], np.int64)
        a, b = core.cluster_consensus(pairs, size, nt), ccr.cluster_consensus(pairs, size, nt)
        assert a.dtype == np.float64 and ccr.same_floats(a, b) and np.array_equal(np.isnan(a), size == 1)
        a, b = core.item_consensus(item, size, nt), ccr.item_consensus(item, size, nt)
        assert a.dtype == np.float64 and ccr.same_floats(a, b) and np.array_equal(np.isnan(a), size == 1)


def test_same_floats_helper():
    a = np.array([1.0, np.nan, 0.5])
    assert ccr.same_floats(a, a.copy())
    assert not ccr.same_floats(a, np.array([1.0, 0.0, 0.5]))
    assert not ccr.same_floats(a, np.array([1.0, np.nan, 0.25]))
