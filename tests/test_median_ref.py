"""The median-partition refinement without a GPU: tests/median_ref.py against the brute-force
co-association matrix, the exact additivity of the accepted moves' gains, and core.median_moves
against median_ref.moves array for array."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import cluster_consensus_ref as ccr
from tests import coassoc_ref as car
from tests import consensus_ref as cr
from tests import golden_io
from tests import median_ref as mr
from tests import vote_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = ["lfr1k_louvain_np20", "lfr1k_mu03_lpm_np20", "karate_louvain_np50"]


def golden_cases():
    """(labs, part) for every golden labeling: batches 0 and -1, the 0.5 consensus and replica 0"""
    for name in GOLDEN:
        case = golden_io.load(name)
        u, v = cr.canonical_edges(case.edges_file[:, 0], case.edges_file[:, 1])
        for batch in (0, -1):
            labs = case.cd_batches[batch]
            yield name, batch, labs, cr.partition(case.N, u, v, 0.5, labels=labs)["labels"]
            yield name, batch, labs, labs[0]


def random_cases():
    """n = 60, R in {1, 5}, K in {1, 7, 60}"""
    for R in (1, 5):
        for K in (1, 7, 60):
            rng = np.random.default_rng(100 * R + K)
            labs = rng.integers(0, 5, (R, 60))
            part = rng.permutation(60) if K == 60 else rng.integers(0, K, 60) * (3 if K == 7 else 1)
            yield "random", (R, K), labs, part


def candidates(labs, part, rng=None):
    """the refinement's own (v, top[v]) for top != P, plus (rng given) random occurring clusters"""
    top = vr.vote(labs, part)["top"]
    nodes = np.flatnonzero(top != part)
    clusters = top[nodes]
    if rng is not None:
        extra = rng.integers(0, len(part), 2 * len(part))
        nodes = np.r_[nodes, extra]
        clusters = np.r_[clusters, rng.choice(np.unique(part), len(extra))]
    return nodes, clusters


def core_moves(labs, part, nodes, clusters):
    from fastconsensus_amd.core import median_moves
    item = ccr.sums(labs, part)[3]
    return median_moves(part, nodes, clusters, mr.affinity(labs, part, nodes, clusters), item, len(labs))


def same_moves(a, b):
    assert sorted(a) == sorted(b) == ["accepted", "alone", "gain", "labels", "proposed"]
    assert a["labels"].dtype == b["labels"].dtype == np.int32 and np.array_equal(a["labels"], b["labels"])
    for f in ("gain", "proposed", "accepted", "alone"):
        assert isinstance(a[f], int) and a[f] == b[f], f


# ------------------------------------------------------------------ affinity
def test_affinity_is_the_coassociation_row_sum():
    case = golden_io.load("lfr1k_louvain_np20")
    labs = case.cd_batches[0]
    part = labs[3]
    rng = np.random.default_rng(1)
    nodes = rng.integers(0, case.N, 300)
    clusters = rng.choice(np.r_[np.unique(part), 999], 300)           # 999 does not occur
    assert 999 not in part and (clusters == 999).any()
    got = mr.affinity(labs, part, nodes, clusters)
    for p in range(300):
        members = np.flatnonzero(part == clusters[p])
        assert got[p] == car.matrix(labs, [nodes[p]], members).sum() if len(members) else got[p] == 0
    own = mr.affinity(labs, part, np.arange(case.N), part)
    assert np.array_equal(own, ccr.sums(labs, part)[3])                # aff(v, P(v)) = item_pairs


# ------------------------------------------------------------------ the objective's delta
def test_objective_changes_by_twice_the_gain():
    moved = 0
    for name, tag, labs, part in list(golden_cases()) + list(random_cases()):
        rng = np.random.default_rng(5)
        for extra in (None, rng):
            nodes, clusters = candidates(labs, part, extra)
            mv = mr.moves(labs, part, nodes, clusters)
            assert mr.objective(labs, mv["labels"]) - mr.objective(labs, part) == 2 * mv["gain"], (name, tag)
            assert (mv["labels"] != part).sum() == mv["accepted"] <= mv["proposed"]
            assert mv["gain"] >= mv["accepted"] and mv["alone"] <= mv["accepted"]
            moved += mv["accepted"]
    assert moved > 0
    # and round after round
    case = golden_io.load("karate_louvain_np50")
    ref = mr.refine(case.cd_batches[0], case.cd_batches[0][0])
    assert ref["converged"] and ref["rounds"] == 3 and ref["objective"] == [7564, 7596, 7692, 7768]
    assert [b - a for a, b in zip(ref["objective"], ref["objective"][1:])] == [2 * g for g in ref["gain_per_round"]]
    assert ref["mean_rand"][1] > ref["mean_rand"][0]


def test_mean_rand_is_the_mean_rand_index():
    rng = np.random.default_rng(8)
    labs, part = rng.integers(0, 4, (3, 30)), rng.integers(0, 5, 30)
    same_p = part[:, None] == part[None, :]
    rand = []
    for lab in labs:
        agree = (same_p == (lab[:, None] == lab[None, :])).sum() - 30      # ordered pairs i != j
        rand.append(agree / (30 * 29))
    got = mr.mean_rand(mr.objective(labs, part), mr.sum_sq(labs), 30, 3)
    assert abs(got - np.mean(rand)) < 1e-12
    from fastconsensus_amd import core
    assert core.mean_rand(mr.objective(labs, part), mr.sum_sq(labs), 30, 3) == got
    ids, size, pairs, item = ccr.sums(labs, part)
    assert core.median_objective(pairs.sum(), size, 3) == mr.objective(labs, part)
    assert isinstance(core.median_objective(pairs.sum(), size, 3), int)


# ------------------------------------------------------------------ core.median_moves against the reference
def test_core_moves_on_golden_and_random_labelings():
    accepted = 0
    for name, tag, labs, part in list(golden_cases()) + list(random_cases()):
        for extra in (None, np.random.default_rng(6)):
            nodes, clusters = candidates(labs, part, extra)
            ref = mr.moves(labs, part, nodes, clusters)
            same_moves(core_moves(labs, part, nodes, clusters), ref)
            accepted += ref["accepted"]
    assert accepted > 0


def test_tie_between_two_clusters_takes_the_smaller_id():
    # clusters 2 = {0, 1, 2}, 6 = {3, 4}, 5 = {5, 6}; node 0 is with 3, 4, 5, 6 in the one replica
    part = np.array([2, 2, 2, 6, 6, 5, 5])
    labs = np.array([[0, 1, 1, 0, 0, 0, 0]])
    for order in ((6, 5), (5, 6)):
        nodes, clusters = np.array([0, 0]), np.array(order)
        ref = mr.moves(labs, part, nodes, clusters)
        assert ref["accepted"] == 1 and ref["alone"] == 0 and np.array_equal(ref["labels"], [5, 2, 2, 6, 6, 5, 5])
        same_moves(core_moves(labs, part, nodes, clusters), ref)


def test_tie_between_a_cluster_and_alone_takes_the_cluster():
    # cluster 4 = {0, 1, 2}, cluster 3 = {3, 4}; one replica puts node 0 with 3 and 4, one leaves it alone:
    # R = 2, aff(0, 3) = 2, pull(0, 3) = 2 * 2 - 2 * 2 = 0 = the pull of a new singleton;
    # pull_own(0) = 2 (2 - 2) - 2 * 2 = -4: both gains are 4, and nobody else gains by moving
    part = np.array([4, 4, 4, 3, 3])
    labs = np.array([[0, 1, 1, 0, 0], [0, 1, 1, 2, 2]])
    ref = mr.moves(labs, part, [0], [3])
    assert (ref["gain"], ref["proposed"], ref["accepted"], ref["alone"]) == (4, 1, 1, 0)
    assert np.array_equal(ref["labels"], [3, 4, 4, 3, 3])
    same_moves(core_moves(labs, part, [0], [3]), ref)
    # a third replica that leaves it alone: pull(0, 3) = 4 - 6 = -2, pull_own = -6: alone wins, 6 to 4,
    # and takes the smallest unused id
    labs = np.array([[0, 1, 1, 0, 0], [0, 1, 1, 2, 2], [0, 1, 1, 2, 2]])
    ref = mr.moves(labs, part, [0], [3])
    assert (ref["gain"], ref["proposed"], ref["accepted"], ref["alone"]) == (6, 1, 1, 1)
    assert np.array_equal(ref["labels"], [0, 4, 4, 3, 3])
    same_moves(core_moves(labs, part, [0], [3]), ref)


def test_a_source_that_is_another_move_s_target():
    # 0 wants from cluster 1 into 2, 3 wants from cluster 2 into 8: they share cluster 2, one is accepted
    part = np.array([1, 1, 1, 2, 2, 2, 8, 8, 8])
    labs = np.array([[0, 1, 1, 0, 0, 0, 2, 2, 2], [0, 1, 1, 3, 0, 0, 3, 3, 3], [0, 1, 1, 3, 0, 0, 3, 3, 3]])
    nodes, clusters = np.array([0, 3]), np.array([2, 8])
    ref = mr.moves(labs, part, nodes, clusters)
    assert ref["proposed"] == 2 and ref["accepted"] == 1
    assert mr.objective(labs, ref["labels"]) - mr.objective(labs, part) == 2 * ref["gain"]
    same_moves(core_moves(labs, part, nodes, clusters), ref)
    # the next round takes the other
    nxt = mr.moves(labs, ref["labels"], nodes, clusters)
    assert nxt["accepted"] == 1 and not np.array_equal(nxt["labels"], ref["labels"])
    same_moves(core_moves(labs, ref["labels"], nodes, clusters), nxt)


def test_candidate_cluster_absent_from_labels():
    from fastconsensus_amd.core import median_moves
    part = np.array([0, 0, 2, 2])
    labs = np.array([[0, 1, 1, 1]])
    for bad in (1, 3):
        with pytest.raises(ValueError):
            mr.moves(labs, part, [0], [bad])
        with pytest.raises(ValueError):
            median_moves(part, [0], [bad], [0], ccr.sums(labs, part)[3], 1)


def test_core_refine_follows_the_reference():
    """core.median_refine is the same loop around any three calls (here the references')"""
    from fastconsensus_amd.core import median_refine
    rng = np.random.default_rng(12)
    truth = rng.integers(0, 5, 150)
    labs = np.stack([np.where(rng.random(150) < 0.2, rng.integers(0, 5, 150), truth) for _ in range(7)])
    start = np.where(rng.random(150) < 0.3, rng.integers(0, 5, 150), truth)

    def cluster(lab):
        ids, size, pairs, item = ccr.sums(labs, lab)
        return {"size": size, "cluster_pairs": pairs, "item_pairs": item}

    for cap in (64, 2):
        got = median_refine(None, start, max_rounds=cap, vote=lambda lab: vr.vote(labs, lab), cluster_consensus=cluster,
                            item_affinity=lambda lab, nd, cl: {"aff": mr.affinity(labs, lab, nd, cl)},
                            sum_sq=mr.sum_sq(labs))
        want = mr.refine(labs, start, max_rounds=cap)
        assert want["rounds"] >= 2 and want["converged"] == (cap == 64)
        for f in want:
            assert np.array_equal(got[f], want[f]), f
        assert got["labels"].dtype == np.int32 and all(isinstance(x, int) for x in got["objective"])


# ------------------------------------------------------------------ the C interface
def header_struct_size(name):
    src = open(os.path.join(ROOT, "include", "fastconsensus_amd.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    width = {"int64_t": 8, "uint64_t": 8, "double": 8, "int32_t": 4}
    return sum(width[t] * len(names.split(",")) for t, names in re.findall(r"(\w+)\s+([\w,\s]+);", body))


def test_ctypes_struct_matches_the_header():
    from fastconsensus_amd import _lib
    assert header_struct_size("fc_cluster_info") == ctypes.sizeof(_lib.ClusterInfo)      # the parser's own check
    assert header_struct_size("fc_affinity_info") == ctypes.sizeof(_lib.AffinityInfo) == 32
    assert [f for f, _ in _lib.AffinityInfo._fields_] == ["k", "queried_clusters", "slow_lookups", "n_r", "pad"]
    assert "fc_item_affinity" in _lib.SYMBOLS and "fc_item_affinity_timing" in _lib.SYMBOLS
