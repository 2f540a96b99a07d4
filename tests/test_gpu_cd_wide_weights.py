"""CD on graphs whose weights reach the paths no consensus run of a small graph does.

Two thresholds split the Louvain kernels, and both are far above what 20 or 300 labelings of a
3 000-node graph produce:

* the replica-lane decide packs (label << wbits) | weight into a sortable 31-bit key; when
  (N - 1) << wbits >= 2^31 RlRun launches k_rl_decide_lds instead (rows staged in LDS, equal labels
  merged by a triangular scan);
* with 2M > 2^31 - 1 the community totals are 8 bytes wide: cd_rl_fits sends Louvain batches to
  cd.hip, which takes its <true, int64_t> instantiations (k_v from kdeg, no packed (Sigma, hash)
  minimum, the generic tie pass), while LPA -- which ignores the weights -- stays on the replica
  lanes.

fc_consensus_apply takes the per-edge counts from a caller's device buffer and, for FC_ALGO_LPM,
writes them as the new weights unchanged; with tau = 0 every edge is kept and with no closure
pairs the graph keeps its edges.  So the step API gives the working graph any int32 weights: the
tests weight the boundary-degree graph of test_gpu_rl_decide_widths (every sorting-network width,
the first heavy row) and the hub graph of test_gpu_parity, assert from the graph read back which
side of each threshold it lies on, and hold every labeling bit for bit to the CPU twin, which is
plain int64 C with no packing.

With every block weighted alike no community total needs more than 32 bits (the refusal at
max k_v * 2M >= 4e18 bounds 2M, and a community holds about a thirtieth of it), so one further
weighting puts nearly all the weight into two blocks: their communities' totals pass 2^32.

Weights come from a few discrete levels, so that equal summed weights -- candidate ties at the
largest weight -- occur; one level equals the n_p_total of the fc_cd calls, the weight whose
own-label entries cd.hip sums by ballot (kacc * w0).
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_gpu_parity import TAILS, _engine, _heavy_graph
from tests.test_gpu_rl_decide_widths import BLOCK, BLOCKS, BOUNDARY_DEGREES, EDGES, LAYOUTS, N, PER_DEGREE
from tests.twin_graph import internal_graph
from tests.weighted_graph import weighted_engine

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 131
ITERATION = 3
I31 = (1 << 31) - 1
GAIN_LIMIT = 4.0e18       # cd.hip: max k_v * 2M below it, or exact int64 gains are refused
OUT_LEVELS = (1, 3, 1 << 10, 1 << 11, 1 << 12)

# regime -> (k: in-block levels 2^k, 2^k + 1, 2^(k+1); the weight of 8 edges, the graph's largest)
REGIMES = {
    "pack_edge": (14, (1 << 19) - 1),
    "lds": (14, 1 << 19),
    "tot64": (18, 1 << 21),
    "near_limit": (20, 1 << 22),
    "refused": (22, 1 << 24),
}
# Community totals past 32 bits.  With every block weighted alike a community holds about 2M / 30,
# and max k_v * 2M < 4e18 keeps that below 2^32 on a graph of this size; so two blocks take k = 22
# and the other blocks k = 10: each of the two then holds nearly half of 2M.
WIDE_TOTAL_K, WIDE_TOTAL_LIGHT_K, WIDE_TOTAL_BLOCKS, WIDE_TOTAL_MAX = 22, 10, (3, 17), 1 << 23
# the hub graph: 19 of 20 edges join two blocks, so the out-of-block levels carry 2M past 2^31
HEAVY_K, HEAVY_MAX = 18, 1 << 20
HEAVY_OUT_LEVELS = (1, 3, 1 << 16, 1 << 17, 1 << 18)


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


def _base_blocks():
    """Planted block of every vertex of the boundary-degree graph.  The probe vertices lie outside
    the 30 blocks: their rows carry the out-of-block levels, so the largest k_v is a block
    vertex's (about 30 in-block entries), which is what lets 2M pass 2^31 sixteen-fold before
    max k_v * 2M reaches the refusal."""
    assert N == BLOCKS * BLOCK + PER_DEGREE * len(BOUNDARY_DEGREES)
    return np.arange(N) // BLOCK


def _heavy_blocks(seed, n):
    """The blocks _heavy_graph draws first from its generator (it does not return them)."""
    return np.random.default_rng(seed).integers(0, 60, n)


def level_weights(same_block, k, w_max, out_levels=OUT_LEVELS, k_edge=None):
    """One weight per edge, in the order given: in-block edges from {2^k, 2^k + 1, 2^(k+1)} (k_edge:
    an edge's own k, at most k), the others from out_levels, and 8 edges spread over the list set to
    w_max.  The draws depend on the edge list and k alone, so two regimes of one k differ in those 8
    weights only."""
    rng = np.random.default_rng(1000 + k)
    m = len(same_block)
    base = np.int64(1) << (np.full(m, k, np.int64) if k_edge is None else np.asarray(k_edge, np.int64))
    pick = rng.integers(0, 3, m)
    w_in = np.where(pick == 0, base, np.where(pick == 1, base + 1, 2 * base))
    w_out = np.array(out_levels, np.int64)[rng.integers(0, len(out_levels), m)]
    w = np.where(same_block, w_in, w_out)
    w[np.linspace(0, m - 1, 8).astype(np.int64)] = w_max
    assert w.max() == w_max
    return w.astype(np.int32)


class Weighted:
    """An engine whose working graph carries chosen weights, and what the tests assert of it."""

    def __init__(self, fcmod, n, edges, blocks, k, w_max, out_levels=OUT_LEVELS, block_k=None):
        """block_k: the k of every block where the blocks differ (at most k)."""
        self.n, self.n_p = n, 1 << k            # n_p_total of the fc_cd calls: an in-block level
        # weighted_engine asserts that the weights were written edge for edge and that every row
        # kept its degree (the boundary-degree probes survive)
        self.eng, sigma, (u2, v2, w2) = weighted_engine(
            fcmod, n, edges,
            lambda u, v: level_weights(blocks[u] == blocks[v], k, w_max, out_levels,
                                       None if block_k is None else np.asarray(block_k)[blocks[u]]),
            SEED, n_p=self.n_p)
        self.g_int, self.sigma = internal_graph(self.eng, n)
        np.testing.assert_array_equal(self.sigma, sigma)
        self.deg = np.bincount(np.concatenate([u2, v2]), minlength=n)
        self.max_w = int(w2.max())
        self.wbits = self.max_w.bit_length()
        self.m2 = 2 * int(w2.astype(np.int64).sum())
        kdeg = np.bincount(np.concatenate([u2, v2]), np.concatenate([w2, w2]).astype(np.float64), minlength=n)
        self.kdeg = kdeg.astype(np.int64)                       # exact: every sum is far below 2^53
        self.max_kdeg = int(self.kdeg.max())
        assert (w2 == self.n_p).any(), "no edge of weight n_p_total"

    def packs(self):
        return ((self.n - 1) << self.wbits) < (1 << 31)

    def gain_product(self):
        return float(self.max_kdeg) * float(self.m2)


def _regime(fcmod, regime):
    """The boundary-degree graph weighted for a regime, with the regime's predicate asserted."""
    k, w_max = REGIMES[regime]
    g = Weighted(fcmod, N, EDGES, _base_blocks(), k, w_max)
    for d in BOUNDARY_DEGREES:
        assert (g.deg == d).sum() >= PER_DEGREE, "no vertices of degree %d" % d
    print("%s: wbits %d, 2M %d, max k_v %d, max k_v * 2M %.3g" % (regime, g.wbits, g.m2, g.max_kdeg, g.gain_product()))
    if regime == "pack_edge":
        assert g.wbits == 19 and g.packs() and g.m2 <= I31
    elif regime == "lds":
        assert g.wbits == 20 and not g.packs() and g.m2 <= I31
    elif regime == "tot64":
        assert g.m2 > I31 and g.gain_product() < GAIN_LIMIT
    elif regime == "near_limit":
        assert g.m2 > I31 and 2.0e18 <= g.gain_product() < GAIN_LIMIT
    else:
        assert g.gain_product() >= GAIN_LIMIT
    return g


_expected = {}


def _twin(name, g, algo, n_r, **kw):
    """The twin's labelings in node order, computed once per (graph, algorithm, batch, options)."""
    key = (name, algo, n_r) + tuple(sorted(kw.items()))
    if key not in _expected:
        exp, _ = orc.engine_cd(algo, g.g_int, n_r, 0, ITERATION, SEED, **kw)
        exp = exp[:, g.sigma]
        exp.setflags(write=False)
        assert len(np.unique(exp[0])) < g.n // 2, "the twin moved nothing"
        _expected[key] = exp
    return _expected[key]


def _check(name, g, algo, n_r, **kw):
    """The batch, then its shard [1, 1 + n_r // 2), bit for bit against the twin."""
    eng = g.eng
    exp = _twin(name, g, algo, n_r, **kw)
    eng.cd(algo, 0, n_r, g.n_p, ITERATION)
    np.testing.assert_array_equal(eng.get_labels(n_r), exp)
    k = n_r // 2
    eng.cd(algo, 1, k, g.n_p, ITERATION)
    np.testing.assert_array_equal(eng.get_labels(k), exp[1:1 + k])
    eng.close()


# the layouts of test_gpu_rl_decide_widths plus 13 replicas (lane groups of 16, 4 vertices per wave)
RL_LAYOUTS = LAYOUTS + [(13, None)]


@pytest.mark.parametrize("engine", [1, 2])
@pytest.mark.parametrize("n_r,u1", RL_LAYOUTS)
@pytest.mark.parametrize("regime", ["pack_edge", "lds"])
def test_rl_decide_both_sides_of_the_packing_limit(fcmod, regime, n_r, u1, engine, monkeypatch):
    """Louvain on the replica-lane kernels with 19-bit weights (WM_WIDE keys up to bit 30) and with
    20-bit ones, which no longer pack (k_rl_decide_lds at every lane layout, its counters flushed
    per bank): the replica-lane engine, and the hybrid, which hands that state to cd.hip."""
    if u1 is not None:
        monkeypatch.setenv("FC_RL_U1", u1)
    g = _regime(fcmod, regime)
    kw = _engine(g.eng, engine)
    _check(regime, g, 0, n_r, **kw)


def test_rl_lpa_ignores_the_weights_that_do_not_pack(fcmod):
    """LPA reads no weight, so its keys pack whatever the graph's weights are."""
    g = _regime(fcmod, "lds")
    kw = _engine(g.eng, 1)
    _check("lds", g, 1, 64, **kw)


@pytest.mark.parametrize("engine", [0, 2])
@pytest.mark.parametrize("coarsen", [0, 8])
@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("prune_mark", [0, 1])
@pytest.mark.parametrize("regime", ["tot64", "near_limit"])
def test_cd_int64_totals_bit_exact_vs_twin(fcmod, regime, prune_mark, tail, coarsen, engine):
    """2M past 2^31 - 1: Louvain runs on cd.hip's <true, int64_t> kernels, the classic engine as it
    is and the hybrid through cd_run(..., shared_full = 1) -- the multi-kernel rounds and the tail
    kernel, with and without coarse rounds, up to max k_v * 2M just below the refusal."""
    g = _regime(fcmod, regime)
    kw = _engine(g.eng, engine, tail, coarsen)
    g.eng.set_option("prune_mark", prune_mark)
    _check(regime, g, 0, 6, prune_mark=prune_mark, **kw)


@pytest.mark.parametrize("engine", [0, 2])
@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("hub_deg", [300, 3000])
def test_cd_int64_totals_heavy_rows_bit_exact(fcmod, hub_deg, tail, engine):
    """Hubs past the 64-entry path (300 entries: k_decide_heavy<true, int64_t> with its LDS table)
    and past the 2048-entry one (3000: the global scratch table) with 8-byte totals.  The hubs'
    k_v is the largest by far, so the levels are set by the product asserted here."""
    n, e = _heavy_graph(5, hub_deg)
    g = Weighted(fcmod, n, e, _heavy_blocks(5, n), HEAVY_K, HEAVY_MAX, HEAVY_OUT_LEVELS)
    print("hubs of %d: 2M %d, max k_v %d, max k_v * 2M %.3g" % (hub_deg, g.m2, g.max_kdeg, g.gain_product()))
    assert (64 < g.deg.max() <= 2048) if hub_deg == 300 else g.deg.max() > 2048
    assert g.m2 > I31 and g.gain_product() < GAIN_LIMIT
    kw = _engine(g.eng, engine, tail)
    _check("hubs%d" % hub_deg, g, 0, 6, **kw)


@pytest.mark.parametrize("engine", [0, 2])
@pytest.mark.parametrize("tail", TAILS)
def test_cd_community_totals_past_32_bits(fcmod, tail, engine):
    """Two blocks carry nearly all the weight, so the totals of their communities pass 2^32 while
    max k_v * 2M stays below the refusal: the 8-byte totals are needed in full, in the gathered
    Sigma, in the scores and in k_apply's updates (asserted of the twin's labelings: a community
    of every replica holds more than 2^32)."""
    block_k = np.full(BLOCKS + 1, WIDE_TOTAL_LIGHT_K)
    block_k[list(WIDE_TOTAL_BLOCKS)] = WIDE_TOTAL_K
    g = Weighted(fcmod, N, EDGES, _base_blocks(), WIDE_TOTAL_K, WIDE_TOTAL_MAX, block_k=block_k)
    print("wide totals: 2M %d, max k_v %d, max k_v * 2M %.3g" % (g.m2, g.max_kdeg, g.gain_product()))
    assert g.m2 > I31 and g.gain_product() < GAIN_LIMIT
    kw = _engine(g.eng, engine, tail)
    for lab in _twin("wide_total", g, 0, 6, **kw):
        assert np.bincount(lab, g.kdeg.astype(np.float64)).max() > float(1 << 32)
    _check("wide_total", g, 0, 6, **kw)


@pytest.mark.parametrize("engine", [1, 2])
@pytest.mark.parametrize("n_r", [6, 64])
def test_rl_lpa_with_int64_totals_bit_exact(fcmod, n_r, engine):
    """cd_rl_fits: 2M past 2^31 - 1 sends Louvain to cd.hip but not LPA, which the replica-lane
    kernels still run, the replica-lane engine throughout and the hybrid for the full sweeps."""
    g = _regime(fcmod, "tot64")
    kw = _engine(g.eng, engine)
    _check("tot64", g, 1, n_r, **kw)


def _input_graph_still_runs(g):
    """After a refusal: the same engine, back on its input graph, against the twin."""
    eng = g.eng
    eng.reset_graph()
    eng.cd(0, 0, 6, 6, 1)
    g_int = orc.EdgeGraph.from_lines(N, np.stack([g.sigma[EDGES[:, 0]], g.sigma[EDGES[:, 1]]], 1))
    exp, _ = orc.engine_cd(0, g_int, 6, 0, 1, SEED)
    np.testing.assert_array_equal(eng.get_labels(6), exp[:, g.sigma])
    eng.close()


def test_cd_refuses_gains_past_int64(fcmod):
    """max k_v * 2M >= 4e18: a gain could overflow int64, so Louvain is refused (FC_ELIMIT)."""
    g = _regime(fcmod, "refused")
    with pytest.raises(fcmod.FastConsensusError, match="edge weights too large for exact int64 modularity gains") as ei:
        g.eng.cd(0, 0, 6, g.n_p, ITERATION)
    assert ei.value.code == -5 and "ELIMIT" in str(ei.value)
    _input_graph_still_runs(g)


def test_leiden_refuses_int64_totals(fcmod):
    """Leiden keeps int32 totals at every level: 2M past 2^31 - 1 is refused (FC_ELIMIT)."""
    g = _regime(fcmod, "tot64")
    with pytest.raises(fcmod.FastConsensusError, match="total edge weight must stay below 2\\^30") as ei:
        g.eng.cd(3, 0, 6, g.n_p, ITERATION)
    assert ei.value.code == -5 and "ELIMIT" in str(ei.value)
    _input_graph_still_runs(g)
