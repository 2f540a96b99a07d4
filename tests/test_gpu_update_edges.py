"""The consensus update on the device where no whole run reaches: the inputs of tests/
update_edge_graphs.py through the step API, against the CPU model (tests/cpu_engine.OracleEngine
on the engine's own node map, which is never the identity here), bit for bit: the candidates,
their co-membership counts, what the applies return, and (u, v, w, age) of the graph after
closure_apply.  Everything is integer; there are no tolerances.  tests/test_update_edge_cases.py
checks, without a GPU, that each input reaches its path:

    caps     k_cgraph_old / k_cgraph_new past the 2048 x 256 entries of one trip (clo_append), and
             the merge and rebuild of 1.9 M edges
    star     one hot neighbourhood: long C rows, many entries per row and block, clo_insert on keys
             drawn again and again; with FC_CLO_PACK 1 and 0
    hub      the binary search of has_edge_row on kept rows and on C rows
    sharded  k_closure_insert on lists that hold one key from several ranks, in any rank order
    chain    repair chains 63 deep on the LDS path and the multi-block path, with every edge
             dropped: graph_merge_next's empty kept list
    ring     0, 1 and fewer attempts than closure blocks; closure_set_pairs with a self pair,
             repeats, edges and the empty list
    lanes    every lane-group width of k_pair_partial, both rules
    keep     the float64 keep rule where tau * n_p is whole, rounds above or rounds below"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import golden_io
from tests import update_edge_graphs as ug
from tests.test_gpu_parity import _sharded_closure, dev_i32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


def engine_for(fcmod, case):
    eng = fcmod.Engine(seed=case.seed)
    eng.load_graph(case.n, case.u, case.v)
    sigma = eng.node_map()
    assert not np.array_equal(sigma, np.arange(case.n)), "default relabel: the node map is not the identity"
    return eng, sigma


def device_update(eng, algo, rnd):
    eng.set_labels(rnd.lab)
    part = dev_i32(eng.m)
    eng.consensus_partial(algo, part)
    return eng.consensus_apply(algo, rnd.n_p, rnd.tau, ug.DELTA, part)


def device_close(eng, algo, rnd, it, nc):
    """closure_partial and closure_apply on the engine's nc candidates -> (counts, conv, m, graph)"""
    cnt = dev_i32(nc)
    eng.closure_partial(cnt)
    conv, m = eng.closure_apply(algo, rnd.n_p, ug.DELTA, cnt if algo != 1 else None, it)
    return cnt[:nc].cpu().numpy(), conv, m, eng.get_graph()


def same_round(applied, nc, closed, rec):
    """one iteration of the device against the model's Record"""
    counts, conv2, m, graph = closed
    assert applied == (rec.conv1, rec.kept_m, rec.unconv)
    assert nc == len(rec.cu)
    np.testing.assert_array_equal(counts, rec.counts)
    assert (conv2, m) == (rec.conv2, rec.m)
    for got, exp in zip(graph, rec.graph):
        np.testing.assert_array_equal(got, exp)


def run_case(fcmod, case, algo, sample=None):
    """every round of the case on a fresh engine; sample(eng, attempts, it) draws the candidates
    (default: closure_sample).  Returns the last round's graph."""
    eng, sigma = engine_for(fcmod, case)
    recs = ug.twin(case, algo, sigma)
    try:
        for it, (rnd, rec) in enumerate(zip(case.rounds, recs)):
            applied = device_update(eng, algo, rnd)
            nc = eng.closure_sample(rnd.attempts, it) if sample is None else sample(eng, rnd.attempts, it)
            closed = device_close(eng, algo, rnd, it, nc)
            same_round(applied, nc, closed, rec)
    finally:
        eng.close()
    return closed[3]


def sharded(world, seed):
    rng = np.random.default_rng(seed)

    def sample(eng, attempts, it):
        assert it == 0                                 # _sharded_closure draws iteration 0
        return _sharded_closure(eng, attempts, world, rng)
    return sample


# ------------------------------------------------------------------ a. closure past the grid caps
@pytest.fixture(scope="module")
def caps_case():
    yield ug.caps()
    ug.forget("caps")


@pytest.mark.parametrize("algo", [0, 1])
def test_closure_past_the_grid_caps(fcmod, caps_case, algo):
    cap = 2048 * 256                                   # consensus.hip clo_append: both grids stop at 2048 blocks of 256
    assert ug.grid_cap() == cap
    u, _, _, age = run_case(fcmod, caps_case, algo)
    f = ug.closure_facts(caps_case, algo, ug.twin(caps_case, algo)[0])
    print("caps, algo %d: candidates per block %s, graph %d edges" % (algo, f["per_block"], len(u)))
    assert max(f["new_entries"] if algo == 0 else f["old_entries"]) > cap
    assert len(u) > 1_800_000 and (age >> orc.AGE_ITER_SHIFT == 1).sum() == f["candidates"]


def test_closure_past_the_grid_caps_sharded(fcmod, caps_case):
    run_case(fcmod, caps_case, 0, sharded(3, 1))


# ------------------------------------------------------------------ b, c. hot rows
@pytest.mark.parametrize("pack", ["1", "0"])
@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("name", ["star", "hub"])
def test_closure_hot_rows(fcmod, name, algo, pack, monkeypatch):
    monkeypatch.setenv("FC_CLO_PACK", pack)            # read when the engine is created
    run_case(fcmod, getattr(ug, name)(), algo)


# ------------------------------------------------------------------ d. sharded closure
@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("name", ["star", "hub"])
def test_closure_hot_rows_sharded(fcmod, name, algo):
    case = getattr(ug, name)()
    single = run_case(fcmod, case, algo)
    split = run_case(fcmod, case, algo, sharded(3, 3 + algo))
    for a, b in zip(single, split):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ e. deep repair chains
@pytest.mark.parametrize("n,repaired", [(3_000, 1_523), (20_000, 10_158)])
def test_repair_deep_chains_with_every_edge_dropped(fcmod, n, repaired):
    case = ug.chain(n)
    u, v, w, age = run_case(fcmod, case, 0)
    assert len(u) == repaired                          # repair edges alone: the kept list was empty
    assert (age >= (2 << orc.AGE_ITER_SHIFT) + orc.AGE_REPAIR_OFFSET).all()
    _, sweeps = ug.jacobi(ug.chain_targets(n))
    assert sweeps > 8


# ------------------------------------------------------------------ f. degenerate attempt counts
@pytest.mark.parametrize("algo", [0, 1])
def test_closure_degenerate_attempt_counts(fcmod, algo):
    for attempts in ug.RING_ATTEMPTS:
        run_case(fcmod, ug.ring(attempts), algo)


@pytest.mark.parametrize("algo", [0, 1])
def test_closure_set_pairs_edge_lists(fcmod, algo):
    case = ug.ring(0)
    rnd = case.rounds[0]
    eng, sigma = engine_for(fcmod, case)
    try:
        for pairs in (ug.RING_PAIRS, np.zeros((0, 2), np.int32), ug.RING_PAIRS[::-1]):
            cpu = ug.new_twin(case, sigma)
            eng.reset_graph()
            applied = ug.twin_update(cpu, algo, rnd)
            assert device_update(eng, algo, rnd) == applied
            w = ug.twin_set_pairs(cpu, algo, rnd, pairs)
            nc = eng.closure_set_pairs(pairs, 0)
            assert nc == len(cpu.cand[0]) == (2 if len(pairs) else 0)
            rec = ug.twin_close(cpu, algo, rnd, 0, applied)
            same_round(applied, nc, device_close(eng, algo, rnd, 0, nc), rec)
            if algo == 0:
                np.testing.assert_array_equal(rec.counts, w)       # closure_from_pairs' own weights
    finally:
        eng.close()


# ------------------------------------------------------------------ g. lane groups of k_pair_partial
@pytest.fixture(scope="module")
def lfr():
    case = golden_io.load("lfr1k_louvain_np20")
    g = orc.EdgeGraph.from_lines(case.N, case.edges_file)
    rng = np.random.default_rng(8)
    pairs = rng.integers(0, case.N, (3000, 2)).astype(np.int32)
    return case, g, pairs


@pytest.mark.parametrize("n_r", ug.LANE_N_R)
def test_pair_partial_lane_groups(fcmod, lfr, n_r):
    case, g, pairs = lfr
    with fcmod.Engine(seed=5) as eng:
        eng.set_option("relabel", 0)                   # edge order = get_graph's canonical order
        eng.load_graph(case.N, case.edges_file[:, 0], case.edges_file[:, 1])
        assert np.array_equal(eng.node_map(), np.arange(case.N)) and eng.m == g.m
        cu, cv, _, _ = orc.closure_from_pairs(0, g, pairs, np.zeros((1, g.N), np.int32), 1)
        order = np.lexsort((cv, cu))
        cu, cv = cu[order], cv[order]
        assert len(cu) > 2000
        for name, lab in ug.lanes(n_r, case.N):
            eng.reset_graph()
            eng.set_labels(lab)
            for algo in (0, 1):
                part = dev_i32(g.m)
                eng.consensus_partial(algo, part)
                exp = ug.pair_partial(lab, g.u, g.v, algo)
                np.testing.assert_array_equal(part.cpu().numpy(), exp, err_msg="n_r %d, set %s, algo %d" % (n_r, name, algo))
                if name != "random":                   # the only replica that splits anything sits at `name`
                    assert set(np.unique(exp)) == ({-1, name} if algo == 0 else {n_r - 1, n_r})
            eng.consensus_apply(1, n_r, 0.0, ug.DELTA, part)       # every edge kept
            assert eng.closure_set_pairs(pairs, 0) == len(cu)
            cnt = dev_i32(len(cu))
            eng.closure_partial(cnt)
            np.testing.assert_array_equal(cnt.cpu().numpy(), ug.pair_partial(lab, cu, cv, 1), err_msg="n_r %d, set %s" % (n_r, name))


# ------------------------------------------------------------------ h. the keep rule at float edges
@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("tau,n_p", ug.KEEP_RULES)
def test_keep_rule_at_float_edges(fcmod, tau, n_p, algo):
    case = ug.keep(tau, n_p)
    rnd = case.rounds[0]
    eng, sigma = engine_for(fcmod, case)
    try:
        conv, kept, unc = device_update(eng, algo, rnd)
        ku, kv, kw, _ = eng.get_nextgraph()
    finally:
        eng.close()
    w = ug.pair_partial(rnd.lab, case.u, case.v, 1)    # the path's edges are in canonical order; prior weight 1 is not in {0, n_p}
    keep = np.array([not (int(x) < tau * n_p) for x in w])
    np.testing.assert_array_equal(orc.threshold(w, tau, n_p), keep)
    np.testing.assert_array_equal(ku, case.u[keep])    # get_nextgraph: node ids, canonical order
    np.testing.assert_array_equal(kv, case.v[keep])
    np.testing.assert_array_equal(kw, w[keep])
    oc, ocnt = orc.check(w[keep], n_p, ug.DELTA)
    assert (kept, unc) == (int(keep.sum()), ocnt)
    assert conv == (oc if algo == 2 else False)        # the lpm loop has no check after the threshold
    rec = ug.twin(case, algo, sigma)[0]
    assert (conv, kept, unc) == (rec.conv1, rec.kept_m, rec.unconv)
