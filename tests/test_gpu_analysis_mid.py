"""The analysis calls on the device at mid size: the case of tests/analysis_mid.py (N = 400,003,
about 800 k edges, 20 and 70 labelings, a partition of 270 k clusters) on one engine with the
default options, every result against the numpy references.  Here every clamped grid makes a second
trip, the clusters A and C leave the register path at the default length cap while B (exactly the
cap) stays on it, the fallbacks fill more than one chunk, and pairs[B], pairs_total, sum_sq, tot_sq
and the co-association histogram pass 2^32 -- tests/test_analysis_mid_cases.py checks, without a GPU,
that the inputs do reach each of these.  Integers compare with np.array_equal; the floats of the
scores keep tests/test_gpu_score.py's bounds.

fc_community_quality takes the five partitions of tests/quality_mid.py on the same engine: more
clusters than k_ql_records' shards cover in one trip, a one-component cluster of 349,029 nodes, a
cluster of 732 parts (tests/test_quality_mid_cases.py checks these without a GPU).

Not reached here: a co-association matrix of more than 2^31 entries (a 9 GB buffer on a shared
card); the largest matrix is 4,099 x 4,001.  The 128-bit carry of tot_sq needs 2M > 2^32:
tests/test_gpu_wide_weight_analysis.py reaches it on a 3,000-node graph."""
import numpy as np
import pytest

from tests import analysis_mid as am
from tests import cluster_consensus_ref as ccr
from tests import consensus_levels_ref as lref
from tests import quality_mid as qm
from tests import score_ref
from tests import vote_ref as vr
from tests.test_gpu_community_quality import same as same_quality
from tests.test_gpu_consensus import same as same_partition
from tests.test_gpu_consensus_levels import same_record

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 7                                    # an engine seed whose node map is not the identity
PART_INTS = ("k", "max_size", "sum_sq", "in_weight", "tot_sq")


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


@pytest.fixture(scope="module")
def case(fcmod):
    c = am.case().compute_all()             # every reference here, so that no test's time holds one
    print("references: %.1f s" % sum(c.seconds.values()), {k: round(v, 2) for k, v in c.seconds.items() if v >= 0.5})
    yield c
    am.case.cache_clear()                   # about 1 GB of host arrays


class Mid:
    """the module's engine and which labelings it holds"""

    def __init__(self, eng, case):
        self.eng, self.case, self.held = eng, case, None

    def use(self, name):
        if self.held != name:
            self.eng.set_labels(self.case[name])
            self.held = name
        return self.eng


@pytest.fixture(scope="module")
def mid(fcmod, case):
    with fcmod.Engine(seed=SEED) as eng:
        eng.load_graph(case["n"], case["u"], case["v"])
        assert eng.m == len(case["u"]) and not np.array_equal(eng.node_map(), np.arange(case["n"]))
        yield Mid(eng, case)


# ------------------------------------------------------------------ 1. cluster and item consensus
@pytest.mark.parametrize("n_r", [20, 70])
def test_cluster_consensus(mid, case, n_r):
    ref = case["cc%d" % n_r]
    part = case["part"]
    got = mid.use("labs%d" % n_r).cluster_consensus(part)
    ids, size, pairs, item = ref["ids"], ref["size"], ref["pairs"], ref["item"]
    assert got["ids"].dtype == np.int32 and np.array_equal(got["ids"], ids)
    assert got["size"].dtype == np.int64 and np.array_equal(got["size"], size)
    wrong = np.flatnonzero(got["cluster_pairs"] != pairs)
    assert not len(wrong), (len(wrong), ids[wrong[:5]], got["cluster_pairs"][wrong[:5]], pairs[wrong[:5]])
    wrong = np.flatnonzero(got["item_pairs"] != item)
    assert not len(wrong), (len(wrong), wrong[:5], got["item_pairs"][wrong[:5]], item[wrong[:5]])
    assert got["cluster_pairs"].dtype == got["item_pairs"].dtype == np.int64
    assert got["k"] == len(ids) > 262_144 and got["n_r"] == n_r
    assert got["max_size"] == size.max() and got["singletons"] == (size == 1).sum()
    assert got["pairs_total"] == int(pairs.sum()) == int(item.sum()) > 1 << 32
    assert got["slow_members"] == ref["slow_members"]
    b = np.searchsorted(ids, case["ids_cab"][2])
    assert size[b] == 16384 and not ref["over"][:, b].any() and got["cluster_pairs"][b] > 1 << 32   # on the register path
    own = size[np.searchsorted(ids, part)]
    assert ccr.same_floats(got["cluster_consensus"], ccr.cluster_consensus(pairs, size, n_r))
    assert ccr.same_floats(got["item_consensus"], ccr.item_consensus(item, own, n_r))


# ------------------------------------------------------------------ 2. vote
@pytest.mark.parametrize("n_r", [20, 70])
def test_vote_map(mid, case, n_r):
    mapped, communities = (case["vote20"]["mapped"], case["vote20"]["mapped_communities"]) if n_r == 20 else case["map70"]
    m = mid.use("labs%d" % n_r).vote_map(case["part"])
    assert m["mapped"].dtype == torch.int32 and tuple(m["mapped"].shape) == (n_r, case["n"])
    got = m["mapped"].cpu().numpy()
    wrong = np.argwhere(got != mapped)
    assert not len(wrong), (len(wrong), wrong[:5])
    assert (m["k"], m["mapped_communities"], m["n_total"]) == (len(case["cc20"]["ids"]), communities, n_r)
    assert m["slow_members"] == case["cc%d" % n_r]["slow_members"]      # the lanes cluster consensus leaves, too


def test_vote(mid, case):
    ref = case["vote20"]
    got = mid.use("labs20").vote(case["part"])
    for f, r in (("top", "top"), ("top_votes", "top_votes"), ("own_votes", "own")):
        assert got[f].dtype == np.int32
        wrong = np.flatnonzero(got[f] != ref[r])
        assert not len(wrong), (f, len(wrong), wrong[:5], got[f][wrong[:5]], ref[r][wrong[:5]])
    assert got["own_hist"].dtype == np.int64 and np.array_equal(got["own_hist"], ref["own_hist"])
    for f in vr.INFO:
        assert got[f] == ref[f], (f, got[f], ref[f])
    assert got["slow_nodes"] == (ref["distinct"] > 8).sum() > 4096
    assert got["slow_members"] == case["cc20"]["slow_members"]
    assert np.array_equal(got["confidence"], ref["own"] / np.float64(20))
    assert ref["tied"] > 4096 and ref["moved"] > 4096 and 0 < ref["unanimous"] < case["n"]     # the inputs


# ------------------------------------------------------------------ 3. item affinity
def affinity(mid, case, n_r, nodes, clusters, exp):
    ref = case["cc%d" % n_r]
    got = mid.use("labs%d" % n_r).item_affinity(case["part"], nodes, clusters)
    assert got["aff"].dtype == np.int64 and got["aff"].shape == (len(nodes),)
    wrong = np.flatnonzero(got["aff"] != exp)
    assert not len(wrong), (len(wrong), wrong[:5], got["aff"][wrong[:5]], exp[wrong[:5]])
    assert got["k"] == len(ref["ids"]) and got["n_r"] == n_r
    assert got["queried_clusters"] == len(np.intersect1d(clusters, case["part"]))
    # the (query, replica) pairs of the fallback: the overflowed lanes of each query's cluster
    assert got["slow_lookups"] == int(ref["over"].sum(0)[np.searchsorted(ref["ids"], clusters)].sum())
    return got


def test_item_affinity_of_every_node_with_its_own_cluster(mid, case):
    got = affinity(mid, case, 20, case["all_nodes"], case["part"], case["aff_own20"])
    assert got["queried_clusters"] == got["k"] > 8192
    assert got["slow_lookups"] == case["cc20"]["slow_members"]
    assert np.array_equal(got["aff"], case["cc20"]["item"])


@pytest.mark.parametrize("n_r", [20, 70])
def test_item_affinity_of_the_refinement_candidates(mid, case, n_r):
    assert len(case["cand_nodes"]) > 4096
    affinity(mid, case, n_r, case["cand_nodes"], case["cand_clusters"], case["aff_cand%d" % n_r])


@pytest.mark.parametrize("n_r", [20, 70])
def test_item_affinity_into_the_long_clusters(mid, case, n_r):
    got = affinity(mid, case, n_r, case["q_nodes"], case["q_clusters"], case["aff_q%d" % n_r])
    assert got["queried_clusters"] == 3 and got["aff"].max() > 16384 and (got["aff"] == 0).any()


# ------------------------------------------------------------------ 4. scoring
def test_score_partitions(mid, case):
    got = mid.use("labs20").score_partitions("input")
    bound = score_ref.float_bound(case["n"])
    for r, exp in enumerate(case["parts20"]):
        for f in PART_INTS:
            assert int(got[f][r]) == exp[f], (r, f, int(got[f][r]), exp[f])
        assert abs(got["entropy"][r] - exp["entropy"]) <= bound, (r, got["entropy"][r], exp["entropy"])
        assert abs(got["modularity"][r] - exp["modularity"]) <= 1e-15, (r, got["modularity"][r], exp["modularity"])
    assert max(p["sum_sq"] for p in case["parts20"]) > 1 << 32 and max(p["tot_sq"] for p in case["parts20"]) > 1 << 32


def test_score_pairs(mid, case):
    eng = mid.use("labs20")
    eng.set_reference(case["reference"])
    try:
        rec = eng.score_pairs(list(am.SCORE_PAIRS))
    finally:
        eng.set_reference(None)
    bound = score_ref.float_bound(case["n"])
    assert len(rec) == len(am.SCORE_PAIRS)
    for x, tag, exp in zip(rec, am.SCORE_PAIRS, case["pairs20"]):
        assert (int(x["a"]), int(x["b"])) == tag
        print(tag, "cells", int(x["cells"]), "sum_sq", int(x["sum_sq"]), "slow", int(x["slow_members"]),
              "mi err", abs(x["mi"] - exp["mi"]), "nmi err", abs(x["nmi"] - exp["nmi"]), "ari err",
              abs(x["ari"] - exp["ari"]), "bound", bound)
        for f in ("cells", "sum_sq"):
            assert int(x[f]) == exp[f], (tag, f, int(x[f]), exp[f])
        assert abs(x["mi"] - exp["mi"]) <= bound, (tag, x["mi"], exp["mi"])
        assert exp["h_mean"] >= 1.0
        assert abs(x["nmi"] - exp["nmi"]) <= bound / exp["h_mean"], (tag, x["nmi"], exp["nmi"])
        assert abs(x["ari"] - exp["ari"]) <= 1e-15, (tag, x["ari"], exp["ari"])
    assert rec[0]["sum_sq"] > 1 << 32
    assert rec[1]["slow_members"] > 262_144 and rec[1]["cells"] > 262_144      # the giant community against singletons


# ------------------------------------------------------------------ 5. consensus partition and hierarchy
@pytest.mark.parametrize("i", range(len(am.THETAS)))
def test_consensus_partition(mid, case, i):
    exp = case["partitions"][i]
    same_partition(mid.use("labs20").consensus_partition(am.THETAS[i]), exp, am.THETAS[i])
    assert 8192 < exp["k"] < case["n"] and exp["max_size"] > 1000 and (exp["support_hist"] > 0).sum() >= 15


def test_consensus_levels(mid, case, fcmod):
    eng = mid.use("labs20")
    lev = eng.consensus_levels("input")
    birth, up = case["tree"]
    rec = case["levels"]
    assert lev["n_total"] == 20 and len(lev["levels"]) == 21
    assert lev["birth"].dtype == lev["up"].dtype == np.int32
    assert np.array_equal(lev["birth"], birth) and np.array_equal(lev["up"], up)
    for s in range(21):
        same_record(lev["levels"][s], rec[s], s)
    assert lev["best_level"] == lref.best_level(rec)
    assert lev["best_theta"] == lref.theta_of(lev["best_level"], 20)
    for s, exp in zip(am.CUT_LEVELS, case["cuts"]):
        lab, k = eng.consensus_cut(s)
        assert lab.dtype == np.int32 and np.array_equal(lab, exp), s
        assert k == rec[s]["k"] == int(exp.max()) + 1, s
        assert np.array_equal(fcmod.cut_tree(lev["birth"], lev["up"], s), exp), s
    assert len({r["k"] for r in rec}) >= 15                                  # the input: a tree of many levels


# ------------------------------------------------------------------ 6. co-association
def test_coassoc_hist(mid, case):
    k = len(case["ca_nodes"])
    assert k >= 92_700
    hist = mid.use("ca_labs").coassoc_hist(case["ca_nodes"])
    assert hist.dtype == np.int64 and np.array_equal(hist, case["ca_hist"]), (hist, case["ca_hist"])
    assert int(hist.sum()) == k * (k - 1) // 2 > 1 << 32 and hist.max() > 1 << 32 and (hist[1:-1] > 0).all()


def test_coassoc_pairs(mid, case):
    got = mid.use("labs20").coassoc_pairs(case["ca_pairs"])
    assert got.dtype == torch.int32 and len(case["ca_pairs"]) == 300_000
    assert np.array_equal(got.cpu().numpy(), case["ca_pairs_ref"])
    assert len(np.unique(case["ca_pairs_ref"])) > 10


def test_coassociation_matrix(mid, case):
    a, b = case["ca_a"], case["ca_b"]
    assert (len(a), len(b)) == (4099, 4001)                                  # 65 x 63 tiles, nb no multiple of 4
    got = mid.use("labs20").coassociation(a, b)
    assert got.dtype == torch.int32 and tuple(got.shape) == (4099, 4001)
    wrong = np.argwhere(got.cpu().numpy() != case["ca_matrix"])
    assert not len(wrong), (len(wrong), wrong[:5])
    assert len(np.unique(case["ca_matrix"])) > 10


# ------------------------------------------------------------------ 7. community quality
@pytest.fixture(scope="module")
def quality(case):
    q = qm.case()                           # the five references here, so that no test's time holds one
    yield q
    qm.case.cache_clear()


@pytest.mark.parametrize("which", qm.NAMES)
def test_community_quality(mid, quality, fcmod, which):
    P, ref = quality[which]
    same_quality(mid.eng.community_quality(P), ref)
    assert np.array_equal(fcmod.split_disconnected(mid.eng, P), ref["split"])


def test_community_quality_fold_waves(fcmod, case, quality):
    """k_ql_fold retires one distinct cluster of a wave's 64 storage slots per turn.  The default
    storage order comes from an ordering pass and cannot be read back, so this engine keeps the
    identity storage (FC_OPT_STORE = 0): slot i holds internal vertex i and node_map() tells which
    nodes share a wave.  Then the fine row has waves of 64 distinct clusters (64 turns, no fold) and
    the coarse row waves that lie wholly inside one cluster (one turn, every fold over 64 lanes).
    No wave lies wholly inside C: under a random numbering that needs 64 of its 16 % in a row."""
    with fcmod.Engine(seed=SEED) as eng:
        eng.set_option("store", 0)
        eng.load_graph(case["n"], case["u"], case["v"])
        order = np.argsort(eng.node_map())                   # order[i] = the node of internal vertex i
        fine = qm.wave_clusters(order, quality["fine"][0])
        coarse = qm.wave_clusters(order, quality["coarse"][0])
        in_c = (case["part"] == case["ids_cab"][0])[order[:len(order) // 64 * 64]].reshape(-1, 64).all(1)
        print("waves of 64 distinct clusters (fine row): %d; waves inside one cluster (coarse row): %d; waves inside C: %d"
              % ((fine == 64).sum(), (coarse == 1).sum(), in_c.sum()))
        assert (fine == 64).any() and (coarse == 1).any()
        for which in ("fine", "coarse", "part"):
            P, ref = quality[which]
            same_quality(eng.community_quality(P), ref)
