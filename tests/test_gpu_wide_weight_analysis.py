"""The analysis calls that read edge weights -- fc_score_partitions, fc_consensus_levels,
fc_community_quality, fc_community_graph -- on working graphs whose sums pass 2^32 and 2^64, and on
working graphs of weights 0 and 1.

The consensus runs of the other tests give weights of at most 20, so no 64-bit sum of these calls
ever needed its upper half and tot_sq never its upper word; and no test had a graph whose largest
weight is 1 but which holds a weight-0 edge, where "the largest weight is 1" is not "every weight
is 1".  tests/weighted_graph.py writes chosen int32 weights into the working graph; the weightings:

    tot64       the boundary-degree graph with in-block weights around 2^18: 2M > 2^32
    wide_total  two of its blocks around 2^22, the others 2^10: two communities whose volume and
                2 in_weight pass 2^32, so their d^2 alone passes 2^64 (tot_sq_hi != 0)
    hubs        the hub graph (rows of 3,000 entries), every weight 2^30: a row sum past 2^32, even
                one 16-lane share of it; 2M > 2^32
    zero_one    the boundary-degree graph, and LFR-1k: 1 on a seeded ~70 % of the edges, 0 elsewhere
    all_zero    karate, every weight 0: M2 == 0

Each asserts what it has to reach from the graph read back and the CPU references before the device
is asked.  The labelings are installed with set_labels; every compared value is an integer and is
compared exactly, the modularity as tests/test_gpu_score.py and tests/test_gpu_consensus_levels.py
compare it."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import consensus_ref as cref
from tests import golden_io
from tests import merge_ref
from tests import quality_ref as qr
from tests import score_ref
from tests.test_gpu_cd_wide_weights import (WIDE_TOTAL_BLOCKS, WIDE_TOTAL_K, WIDE_TOTAL_LIGHT_K, WIDE_TOTAL_MAX,
                                            _base_blocks, _heavy_blocks, level_weights)
from tests.test_gpu_community_quality import same, sparse_ids
from tests.test_gpu_consensus_levels import check as check_levels
from tests.test_gpu_parity import _heavy_graph
from tests.test_gpu_rl_decide_widths import BLOCKS, EDGES, N
from tests.twin_graph import internal_graph
from tests.weighted_graph import weighted_engine

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 131
ITERATION = 3
TWO32, TWO64 = 1 << 32, 1 << 64
PART_INTS = ("k", "max_size", "sum_sq", "in_weight", "tot_sq")
LABELINGS = ("blocks", "one", "singletons", "moved")          # what set_labels installs, in this order
PARTITIONS = LABELINGS + ("sparse", "halves", "sides")
WIDE = ("wide_total", "tot64", "hubs")
ZERO_ONE = ("zero_one", "zero_one_lfr")


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


# ------------------------------------------------------------------ the weightings
def zero_one_weights(u, v):
    return (np.random.default_rng(7).random(len(u)) < 0.7).astype(np.int32)


def weighting(name):
    """(n, edges [m][2], planted blocks [n], weight_of_edge)"""
    if name in ("tot64", "wide_total", "zero_one"):
        blocks = _base_blocks()
        if name == "tot64":
            return N, EDGES, blocks, lambda u, v: level_weights(blocks[u] == blocks[v], 18, 1 << 21)
        if name == "zero_one":
            return N, EDGES, blocks, zero_one_weights
        block_k = np.full(BLOCKS + 1, WIDE_TOTAL_LIGHT_K)
        block_k[list(WIDE_TOTAL_BLOCKS)] = WIDE_TOTAL_K
        return N, EDGES, blocks, lambda u, v: level_weights(blocks[u] == blocks[v], WIDE_TOTAL_K, WIDE_TOTAL_MAX,
                                                            k_edge=block_k[blocks[u]])
    if name == "hubs":
        n, e = _heavy_graph(5, 3000)
        return n, e, _heavy_blocks(5, n), lambda u, v: np.full(len(u), 1 << 30, np.int32)
    if name == "zero_one_lfr":
        lfr = golden_io.load("lfr1k_louvain_np20")
        return lfr.N, lfr.edges_file, np.asarray(lfr.cd_batches[-1][0]), zero_one_weights
    assert name == "all_zero"
    karate = golden_io.load("karate_louvain_np50")
    return karate.N, karate.edges_file, np.asarray(karate.cd_batches[-1][0]), lambda u, v: np.zeros(len(u), np.int32)


def two_sides(n, u, v, w, sweeps=2):
    """Two clusters with a heavy cut between them, so that one pair of the community graph carries
    more than half of the graph's weight: from the parity split, every node in turn goes to the
    side that holds less of its neighbours' weight."""
    side = (np.arange(n) & 1).astype(np.int32)
    ends, other, wt = np.concatenate([u, v]), np.concatenate([v, u]), np.concatenate([w, w]).astype(np.int64)
    o = np.argsort(ends, kind="stable")
    other, wt, start = other[o], wt[o], np.searchsorted(ends[o], np.arange(n + 1))
    for _ in range(sweeps):
        for x in range(n):
            row = slice(start[x], start[x + 1])
            on1 = side[other[row]] == 1
            side[x] = int(wt[row][~on1].sum() >= wt[row][on1].sum())
    return side


def partitions(n, blocks, u, v, w):
    """The four labelings (the planted blocks, one community, singletons, the blocks with a seeded
    10 % of the nodes moved), the moved one under sparse ids, every block cut in two halves, and
    two_sides."""
    blocks = np.unique(blocks, return_inverse=True)[1].ravel().astype(np.int32)
    rng = np.random.default_rng(5)
    pick = rng.random(n) < 0.1
    moved = blocks.copy()
    moved[pick] = rng.integers(0, int(blocks.max()) + 1, int(pick.sum()))
    return {"blocks": blocks, "one": np.zeros(n, np.int32), "singletons": np.arange(n, dtype=np.int32),
            "moved": moved, "sparse": sparse_ids(moved, n).astype(np.int32),
            "halves": (2 * blocks + (np.arange(n) & 1)).astype(np.int32), "sides": two_sides(n, u, v, w)}


class Case:
    """One weighting: the engine, the working graph read back, the partitions and every reference,
    with what the weighting has to reach asserted from those alone."""

    def __init__(self, fcmod, name):
        self.name = name
        self.n, edges, blocks, weight_of_edge = weighting(name)
        self.eng, _, (self.u, self.v, self.w) = weighted_engine(fcmod, self.n, edges, weight_of_edge, SEED)
        n, u, v, w = self.n, self.u, self.v, self.w
        self.P = partitions(n, blocks, u, v, w)
        self.labs = np.stack([self.P[x] for x in LABELINGS])
        self.m2 = 2 * int(w.astype(np.int64).sum())
        self.quality = {x: qr.quality(n, u, v, w, p) for x, p in self.P.items()}
        self.cgraph = {x: merge_ref.community_graph(n, u, v, w, p) for x, p in self.P.items()}
        self.parts = [score_ref.part(row, u, v, w) for row in self.labs]
        self.reached()

    def reached(self):
        name, w, q = self.name, self.w, self.quality
        one, blocks = q["one"], q["blocks"]
        row = int((one["node_in"] + one["node_out"]).max())                 # the heaviest CSR row
        deg = int(np.bincount(np.concatenate([self.u, self.v])).max())
        print("%s: max w %d, 2M %d, largest volume %d, largest 2 in_weight %d, largest tot_sq %d, heaviest row %d "
              "(%d entries), largest pair weight %d, cut weight of the singletons %d"
              % (name, w.max(), self.m2, blocks["volume"].max(), 2 * blocks["in_weight"].max(),
                 max(p["tot_sq"] for p in self.parts), row, deg,
                 max(int(g["weight"].max()) for g in self.cgraph.values() if g["npairs"]), q["singletons"]["cut_weight"]))
        assert self.parts[1]["tot_sq"] == self.m2 ** 2 and one["total_degree"] == self.m2
        if name in WIDE:
            assert self.m2 > TWO32 and self.parts[1]["tot_sq"] >= TWO64
        if name == "wide_total":
            heavy = np.searchsorted(blocks["ids"], WIDE_TOTAL_BLOCKS)
            assert (blocks["volume"][heavy] > TWO32).all() and (2 * blocks["in_weight"][heavy] > TWO32).all()
            assert all(int(d) ** 2 >= TWO64 for d in blocks["volume"][heavy])   # each alone sets tot_sq_hi
            assert self.parts[0]["tot_sq"] >= TWO64
            assert self.cgraph["sides"]["weight"].max() > TWO32 and q["sides"]["cut_weight"] > TWO32
        if name == "hubs":
            assert (w == 1 << 30).all() and row > TWO32 and -(-deg // 16) * (1 << 30) > TWO32
        if name in ZERO_ONE:
            assert w.max() == 1 and (w == 0).any() and self.m2 < 2 * len(w)
            for x, p in self.P.items():     # a weight-0 edge inside a cluster (the singletons have no edge inside)
                inside = p[self.u] == p[self.v]
                assert x == "singletons" or (inside & (w == 0)).any(), x
        if name == "all_zero":
            assert self.m2 == 0 and len(w) > 0 and not w.any()


_cases = {}


@pytest.fixture(scope="module")
def case(fcmod):
    """name -> Case, each built once for the module"""
    def get(name):
        if name not in _cases:
            _cases[name] = Case(fcmod, name)
        return _cases[name]
    yield get
    for c in _cases.values():
        c.eng.close()
    _cases.clear()


# ------------------------------------------------------------------ the four calls, working graph
@pytest.mark.parametrize("name", WIDE + ZERO_ONE)
def test_score_partitions(case, name):
    c = case(name)
    c.eng.set_labels(c.labs)
    got = c.eng.score_partitions("working")
    for r, exp in enumerate(c.parts):
        for f in PART_INTS:
            assert int(got[f][r]) == exp[f], (LABELINGS[r], f, int(got[f][r]), exp[f])
        assert abs(got["modularity"][r] - exp["modularity"]) <= 1e-15, (r, got["modularity"][r], exp["modularity"])
    if name in WIDE:
        assert int(got["tot_sq"][1]) == c.m2 ** 2 >= TWO64


@pytest.mark.parametrize("name", WIDE + ZERO_ONE)
def test_consensus_levels(case, name):
    c = case(name)
    c.eng.set_labels(c.labs)
    sup = cref.support(c.labs, c.u, c.v)
    lev, rec = check_levels(c.eng, c.n, c.u, c.v, sup, len(LABELINGS), graph="working", w=c.w)
    assert (lev["levels"]["bucket_edges"] > 0).sum() >= 2
    if name in WIDE:
        assert max(r["tot_sq"] for r in rec) >= TWO64 and max(r["in_weight"] for r in rec) > TWO32


@pytest.mark.parametrize("which", PARTITIONS)
@pytest.mark.parametrize("name", WIDE + ZERO_ONE)
def test_community_quality(case, name, which):
    c = case(name)
    ref = c.quality[which]
    got = c.eng.community_quality(c.P[which], graph="working")
    same(got, ref)
    assert (got["in_weight_total"], got["cut_weight"], got["total_degree"]) == \
        (int(ref["in_weight"].sum()), ref["cut_weight"], c.m2)
    assert np.array_equal(got["cut"], ref["cut"])


@pytest.mark.parametrize("which", PARTITIONS)
@pytest.mark.parametrize("name", WIDE + ZERO_ONE)
def test_community_graph(case, name, which):
    c = case(name)
    ref = c.cgraph[which]
    got = c.eng.community_graph(c.P[which], graph="working")
    assert got["npairs"] == ref["npairs"]
    for f in ("a", "b", "weight", "edges"):
        assert got[f].dtype == ref[f].dtype and np.array_equal(got[f], ref[f]), f
    assert int(got["weight"].sum()) == c.quality[which]["cut_weight"]


@pytest.mark.parametrize("name", WIDE + ZERO_ONE)
def test_the_input_graph_is_still_unit_weight(case, name):
    c = case(name)
    c.eng.set_labels(c.labs)
    got = c.eng.score_partitions("input")
    for r, row in enumerate(c.labs):
        exp = score_ref.part(row, c.u, c.v)
        for f in PART_INTS:
            assert int(got[f][r]) == exp[f], (LABELINGS[r], f, int(got[f][r]), exp[f])
        assert abs(got["modularity"][r] - exp["modularity"]) <= 1e-15
    for which in ("moved", "sparse"):
        same(c.eng.community_quality(c.P[which]), qr.quality(c.n, c.u, c.v, None, c.P[which]))


# ------------------------------------------------------------------ every weight 0
def test_all_zero(case):
    """M2 == 0: modularity 0.0 at every level and in every row, conductance NaN, no division."""
    c = case("all_zero")
    eng = c.eng
    eng.set_labels(c.labs)
    got = eng.score_partitions("working")
    for r, exp in enumerate(c.parts):
        for f in PART_INTS:
            assert int(got[f][r]) == exp[f], (LABELINGS[r], f)
        assert exp["in_weight"] == exp["tot_sq"] == 0 and got["modularity"][r] == 0.0 == exp["modularity"]
    lev, rec = check_levels(eng, c.n, c.u, c.v, cref.support(c.labs, c.u, c.v), len(LABELINGS), graph="working", w=c.w)
    assert all(float(x) == 0.0 for x in lev["levels"]["modularity"]) and lev["best_level"] == len(LABELINGS)
    for which in PARTITIONS:
        q = eng.community_quality(c.P[which], graph="working")
        same(q, c.quality[which])
        assert q["total_degree"] == q["cut_weight"] == q["in_weight_total"] == 0 and np.isnan(q["conductance"]).all()
        g = eng.community_graph(c.P[which], graph="working")
        for f in ("a", "b", "weight", "edges"):
            assert np.array_equal(g[f], c.cgraph[which][f]), (which, f)
        assert not g["weight"].any() and int(g["edges"].sum()) + int(q["in_edges"].sum()) == len(c.w)   # every edge counted


# ------------------------------------------------------------------ CD on weights 0 and 1
def _cd_batch(fcmod, name, algo, n_r=6):
    """One batch on a fresh engine with the weighting's working graph, bit for bit against the CPU
    twin (engine_leiden for Leiden, engine_cd otherwise), which is plain int64 C and reads every weight."""
    n, edges, _, weight_of_edge = weighting(name)
    eng, sigma, (u, v, w) = weighted_engine(fcmod, n, edges, weight_of_edge, SEED)
    with eng:
        assert w.max() == 1 and (w == 0).any()
        g_int, _ = internal_graph(eng, n)
        twin = orc.engine_leiden if algo == 3 else lambda *a: orc.engine_cd(algo, *a)
        exp, _ = twin(g_int, n_r, 0, ITERATION, SEED)
        exp = exp[:, sigma]
        assert len(np.unique(exp[0])) < n // 2, "the twin moved nothing"
        eng.cd(algo, 0, n_r, n_r, ITERATION)
        got = eng.get_labels(n_r)
        bad = [(r, int((got[r] != exp[r]).sum())) for r in range(n_r) if not np.array_equal(got[r], exp[r])]
        assert not bad, "(replica, nodes that differ): %s" % bad


@pytest.mark.parametrize("name", ZERO_ONE)
def test_leiden_reads_the_zero_weights(fcmod, name):
    _cd_batch(fcmod, name, 3)


@pytest.mark.parametrize("name", ZERO_ONE)
def test_louvain_reads_the_zero_weights(fcmod, name):
    """the control: cd_unit_weights has always asked for M2 == 2 m"""
    _cd_batch(fcmod, name, 0)
