"""The mid-size case of tests/analysis_mid.py, without a GPU: it reaches every cap it was built for
(so tests/test_gpu_analysis_mid.py is not empty), its two sparse references equal the brute-force
ones where those still run, and it is the same on every build."""
import numpy as np
import pytest

from tests import analysis_mid as am
from tests import cluster_consensus_ref as ccr
from tests import coassoc_ref as car
from tests import golden_io
from tests import median_ref as mr

RELATION = {">": lambda a, b: a > b, "==": lambda a, b: a == b, "<=": lambda a, b: a <= b}


@pytest.fixture(scope="module")
def lfr():
    return golden_io.load("lfr1k_louvain_np20")


def test_caps_are_read_from_the_sources():
    k = am.caps()
    assert set(k) >= {"SC_GRID", "LCAP", "CHUNK", "k_cc_total", "k_vc_slow", "k_ia_lookup"}
    assert all(isinstance(x, int) and x > 0 for x in k.values())
    with pytest.raises(AssertionError):
        am.const("score.h", "SC_NO_SUCH_CONSTANT")


def test_every_cap_is_reached():
    case = am.case()
    got = am.reached(case)
    assert len(got) >= 35
    missed = {name: x for name, x in got.items() if not RELATION[x[1]](x[0], x[2])}
    assert not missed, missed


def test_hist_by_signature_equals_brute_force(lfr):
    rng = np.random.default_rng(3)
    for labs in (lfr.cd_batches[0], lfr.cd_batches[-1]):
        for nodes in (np.arange(lfr.N), rng.choice(lfr.N, 700, replace=False), rng.integers(0, lfr.N, 300)):
            assert np.array_equal(am.hist_by_signature(labs, nodes), car.hist(labs, nodes))
    # crafted: 2,000 listed nodes (some twice) of few signatures, as the mid-size case's
    case = am.case()
    nodes = np.r_[case["ca_nodes"][:1990], case["ca_nodes"][:10]]
    exp = car.hist(case["ca_labs"], nodes)
    assert np.array_equal(am.hist_by_signature(case["ca_labs"], nodes), exp)
    assert (exp[1:-1] > 0).any() and exp[0] > 0 and exp[-1] > 0 and exp.sum() == 2000 * 1999 // 2
    assert np.array_equal(am.hist_by_signature(case["ca_labs"], nodes[:1]), np.zeros(am.CA_N_R + 1, np.int64))


def test_sparse_affinity_equals_the_dense_tables(lfr):
    rng = np.random.default_rng(5)
    labs = lfr.cd_batches[0]
    for part in (lfr.cd_batches[-1][2], rng.integers(0, 40, lfr.N) * 3 + 1, rng.permutation(lfr.N)):
        nodes = rng.integers(0, lfr.N, 3000)
        clusters = np.r_[part[rng.integers(0, lfr.N, 2000)], part[nodes[2000:2900]], rng.integers(0, lfr.N, 100)]
        exp = mr.affinity(labs, part, nodes, clusters)
        assert np.array_equal(am.sparse_affinity(labs, part, nodes, clusters), exp)
        assert exp.any()
    # every node against its own cluster is cluster consensus' item sum
    part = lfr.cd_batches[-1][2]
    assert np.array_equal(am.sparse_affinity(labs, part, np.arange(lfr.N), part), ccr.sums(labs, part)[3])


def test_lane_overflow_on_a_crafted_partition():
    part = np.repeat([0, 1, 2], [9, 8, 20])
    labs = np.stack([np.arange(37), np.zeros(37, np.int64)])
    over = am.lane_overflow(am.cluster_cells(labs, part)[2], np.array([9, 8, 20]), 8, 16)
    assert over.tolist() == [[True, False, True], [False, False, True]]


def test_build_is_deterministic():
    case = am.case()
    again = am.build(refs=False)
    assert set(again) <= set(case)
    for name, x in again.items():
        assert np.array_equal(case[name], x), name
        assert np.asarray(case[name]).dtype == np.asarray(x).dtype, name
    own = case["aff_own20"]
    assert np.array_equal(own, case["cc20"]["item"])           # two references, one quantity
