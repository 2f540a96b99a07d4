"""The cluster merges without a GPU: tests/merge_ref.py against the brute-force co-association
matrix and the cluster consensus, the exact additivity of the accepted merges' gains, the recorded
trajectories on the golden labelings, and core.merge_moves against merge_ref.moves."""
import numpy as np
import pytest

from tests import cluster_consensus_ref as ccr
from tests import coassoc_ref as car
from tests import consensus_ref as cr
from tests import golden_io
from tests import median_ref as mr
from tests import merge_ref as gr

GOLDEN = ["lfr1k_louvain_np20", "lfr1k_mu03_lpm_np20", "karate_louvain_np50"]


def graph_of(case):
    return cr.canonical_edges(case.edges_file[:, 0], case.edges_file[:, 1])


def strict_cut(case, labs):
    """components of the edges every labeling keeps inside a community"""
    u, v = graph_of(case)
    return cr.partition(case.N, u, v, 1.0, labels=labs)["labels"]


def same_partition(p, q):
    """equal up to the names of the clusters"""
    cells = len(set(zip(np.asarray(p).tolist(), np.asarray(q).tolist())))
    return cells == len(np.unique(p)) == len(np.unique(q))


def all_pairs(part):
    ids = np.unique(part)
    a, b = np.meshgrid(ids, ids, indexing="ij")
    return a.reshape(-1), b.reshape(-1)


# ------------------------------------------------------------------ cross
def test_cross_is_the_coassociation_block_sum():
    case = golden_io.load("karate_louvain_np50")
    labs = case.cd_batches[0]
    part = strict_cut(case, labs)
    a, b = all_pairs(part)
    got = gr.cross(labs, part, a, b)
    for p in range(len(a)):
        block = car.matrix(labs, np.flatnonzero(part == a[p]), np.flatnonzero(part == b[p]))
        assert got[p] == int(block.astype(np.int64).sum())
    assert np.array_equal(gr.cross(labs, part, [0, 60, 1], [60, 60, 0]), [0, 0, got[len(np.unique(part))]])


@pytest.mark.parametrize("name", GOLDEN)
def test_cross_diagonal_is_the_cluster_consensus_pair_sum(name):
    case = golden_io.load(name)
    for batch in (0, -1):
        labs = case.cd_batches[batch]
        for part in (labs[0], strict_cut(case, labs)):
            ids, _, pairs, _ = ccr.sums(labs, part)
            assert np.array_equal(gr.cross(labs, part, ids, ids), pairs)


# ------------------------------------------------------------------ additivity
@pytest.mark.parametrize("name", GOLDEN)
def test_every_round_changes_the_objective_by_twice_its_gain(name):
    case = golden_io.load(name)
    u, v = graph_of(case)
    for b in range(len(case.cd_batches)):
        labs = case.cd_batches[b]
        for part in (labs[0], strict_cut(case, labs)):
            ref = gr.refine(labs, part, case.N, u, v)
            assert ref["converged"] and len(ref["objective"]) == ref["rounds"] + 1
            for r in range(ref["rounds"]):
                assert ref["objective"][r + 1] - ref["objective"][r] == 2 * ref["gain_per_round"][r] > 0
                assert ref["k_per_round"][r] - ref["k_per_round"][r + 1] == ref["accepted_per_round"][r]


# ------------------------------------------------------------------ the recorded trajectories
def trajectory(name, batch, start):
    case = golden_io.load(name)
    u, v = graph_of(case)
    labs = case.cd_batches[batch]
    part = {"strict": lambda: strict_cut(case, labs), "replica0": lambda: labs[0],
            "singletons": lambda: np.arange(case.N)}[start]()
    return labs, gr.refine(labs, part, case.N, u, v)


# (case, batch, start) -> k before and after, F before and after, rounds, first round's pairs / proposed / accepted
TRAJECTORIES = {
    ("lfr1k_louvain_np20", 0, "strict"): (139, 24, 908600, 1039252, 11, (1866, 305, 49)),
    ("lfr1k_louvain_np20", 0, "replica0"): (23, 21, 947652, 969420, 1, (253, 2, 2)),
    ("lfr1k_louvain_np20", 0, "singletons"): (1000, 25, 20000, 1039504, 18, (13637, 5531, 444)),
    ("lfr1k_louvain_np20", -1, "singletons"): (1000, 31, 20000, 1046200, 15, (13637, 5286, 438)),
    ("karate_louvain_np50", 0, "strict"): (20, 8, 3600, 7848, 5, (45, 19, 6)),
}


@pytest.mark.parametrize("key", sorted(TRAJECTORIES), ids=lambda k: "%s-%d-%s" % k)
def test_recorded_trajectory(key):
    k0, k1, f0, f1, rounds, first = TRAJECTORIES[key]
    labs, ref = trajectory(*key)
    assert (ref["k_per_round"][0], ref["k_per_round"][-1]) == (k0, k1)
    assert (ref["objective"][0], ref["objective"][-1]) == (f0, f1)
    assert ref["rounds"] == rounds and ref["converged"]
    assert (ref["pairs_per_round"][0], ref["proposed_per_round"][0], ref["accepted_per_round"][0]) == first
    assert ref["objective"][-1] == mr.objective(labs, ref["labels"])


def test_singletons_reach_the_replicas_common_partition():
    case = golden_io.load("lfr1k_louvain_np20")
    labs, ref = trajectory("lfr1k_louvain_np20", -1, "singletons")
    assert all(mr.objective(labs, lab) == 1046200 for lab in labs)
    assert same_partition(ref["labels"], labs[0])


def test_fixpoints_of_the_rule():
    for name in ("lfr1k_louvain_np20", "karate_louvain_np50"):
        case = golden_io.load(name)
        u, v = graph_of(case)
        labs = case.cd_batches[-1]
        assert gr.refine(labs, labs[0], case.N, u, v)["rounds"] == 0
    case = golden_io.load("karate_louvain_np50")
    u, v = graph_of(case)
    assert gr.refine(case.cd_batches[0], case.cd_batches[0][0], case.N, u, v)["rounds"] == 0
    # past median_refine's fixpoint on karate (7,768)
    assert trajectory("karate_louvain_np50", 0, "strict")[1]["objective"][-1] > 7768


# ------------------------------------------------------------------ community graph
def test_community_graph_of_singletons_is_the_edge_list():
    for name in ("karate_louvain_np50", "lfr1k_louvain_np20"):
        case = golden_io.load(name)
        u, v = graph_of(case)
        cg = gr.community_graph(case.N, u, v, None, np.arange(case.N))
        assert cg["npairs"] == len(u)
        assert np.array_equal(cg["a"], u) and np.array_equal(cg["b"], v)
        assert (cg["edges"] == 1).all() and (cg["weight"] == 1).all()
        one = gr.community_graph(case.N, u, v, None, np.zeros(case.N, np.int64))
        assert one["npairs"] == 0 and len(one["a"]) == 0


def test_community_graph_weights_and_sparse_ids():
    u, v, w = [0, 0, 1, 2, 3], [1, 2, 3, 3, 4], [5, 0, 2, 7, 1]
    cg = gr.community_graph(5, u, v, w, [40, 40, 7, 7, 9])
    assert cg["a"].tolist() == [7, 7] and cg["b"].tolist() == [9, 40]
    assert cg["weight"].tolist() == [1, 2] and cg["edges"].tolist() == [1, 2]


# ------------------------------------------------------------------ core.merge_moves
def same_moves(a, b):
    assert sorted(a) == sorted(b) == ["accepted", "gain", "labels", "proposed"]
    assert a["labels"].dtype == b["labels"].dtype == np.int32 and np.array_equal(a["labels"], b["labels"])
    for f in ("gain", "proposed", "accepted"):
        assert isinstance(a[f], int) and a[f] == b[f], f


@pytest.mark.parametrize("name", GOLDEN)
def test_core_merge_moves_equals_the_reference(name):
    from fastconsensus_amd.core import merge_moves
    case = golden_io.load(name)
    u, v = graph_of(case)
    labs = case.cd_batches[0]
    rng = np.random.default_rng(3)
    for part in (strict_cut(case, labs), labs[0], rng.permutation(case.N)[strict_cut(case, labs)]):
        cg = gr.community_graph(case.N, u, v, None, part)
        # both orders, duplicates, a == b and an id that does not occur (its size is 0)
        free = int(np.setdiff1d(np.arange(case.N), part)[0]) if len(np.unique(part)) < case.N else int(part[0])
        a = np.r_[cg["b"], cg["a"], cg["a"][:5], part[:3], free]
        b = np.r_[cg["a"], cg["b"], cg["b"][:5], part[:3], part[0]]
        x = gr.cross(labs, part, a, b)
        got = merge_moves(part, a, b, x, len(labs))
        same_moves(got, gr.moves(part, a, b, x, len(labs)))
        same_moves(got, gr.moves(part, cg["a"], cg["b"], gr.cross(labs, part, cg["a"], cg["b"]), len(labs)))
        assert mr.objective(labs, got["labels"]) - mr.objective(labs, part) == 2 * got["gain"]


def test_core_between_consensus():
    from fastconsensus_amd.core import between_consensus
    out = between_consensus([6, 0, 5], [2, 3, 0], [3, 1, 4], 2)
    assert out[0] == 0.5 and out[1] == 0.0 and np.isnan(out[2])
