"""The inputs of tests/update_edge_graphs.py, without a GPU: from the CPU model alone (tests/
cpu_engine.OracleEngine, orc.closure_sample_pairs, orc.closure_from_pairs) each reaches the path
of the consensus update it was built for, so tests/test_gpu_update_edges.py is not empty.  The
conditions are requirements on the inputs: a changed seed or size must still meet them.  Each test
prints the facts it asserts (pytest -s)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import golden_io
from tests import update_edge_graphs as ug


def node_map(case):
    sigma = orc.device_sigma(case.n, case.seed)
    assert not np.array_equal(sigma, np.arange(case.n)), "the engine's numbering must not be the identity"
    return sigma


# ------------------------------------------------------------------ a. closure past the grid caps
def test_the_grid_cap_is_read_from_clo_append():
    assert ug.grid_cap() == 2048 * 256            # consensus.hip clo_append: og, ng <= 2048 blocks of TB = 256


def test_caps_pass_the_closure_grids():
    case = ug.caps()
    node_map(case)
    cap = ug.grid_cap()
    try:
        f0 = ug.closure_facts(case, 0, ug.twin(case, 0)[0])
        f1 = ug.closure_facts(case, 1, ug.twin(case, 1)[0])
    finally:
        ug.forget("caps")
    print("caps, algo 0: candidates per block", f0["per_block"], "longest C row", f0["longest_c_row"])
    print("caps, algo 1: candidates per block", f1["per_block"], "before the last block", f1["before_last"])
    assert (f0["blocks"], f1["blocks"]) == (4, 16)
    # algo 0: k_cgraph_new's second trip in block 0, k_cgraph_old's in block 2
    assert 2 * f0["per_block"][0] > cap
    assert 2 * sum(f0["per_block"][:2]) > cap
    assert f0["new_entries"][0] > cap and f0["old_entries"][1] > cap      # the same, as the kernels count
    # algo 1: k_cgraph_old's in the later blocks (its last launch moves the blocks before the last but one)
    assert 2 * f1["before_last"] > cap
    assert f1["old_entries"][-1] > cap and max(f1["new_entries"]) <= cap
    assert f0["longest_kept_row"] > 16 and f0["long_row_candidates"] > 1000


# ------------------------------------------------------------------ b. one hot neighbourhood
@pytest.mark.parametrize("algo", [0, 1])
def test_star_is_one_hot_neighbourhood(algo):
    case = ug.star()
    sigma = node_map(case)
    rec = ug.twin(case, algo)[0]
    f = ug.closure_facts(case, algo, rec)
    d = ug.draw_facts(case, algo, rec)
    print("star, algo %d: %d candidates from %d valid draws; per block %s; most entries one block adds to a C row %d; "
          "longest C row %d; candidates drawn by more than one of 3 ranks, per block %s"
          % (algo, f["candidates"], d["valid_draws"], f["per_block"], f["row_gain"], f["longest_c_row"], d["shared_by_ranks"]))
    leaves = case.n - 1
    assert f["candidates"] == leaves * (leaves - 1) // 2 == 780        # every leaf pair
    assert sigma[0] not in rec.cu and sigma[0] not in rec.cv
    assert d["valid_draws"] > 10 * f["candidates"]                     # clo_insert meets most keys again
    assert f["row_gain"] > 16                                          # the counting loops of k_cgraph_old / _new
    assert f["longest_c_row"] > 16                                     # has_edge_row's binary search on a C row
    if algo == 0:
        assert max(d["shared_by_ranks"]) >= 100                        # k_closure_insert: one key from several ranks


# ------------------------------------------------------------------ c. a hub among ordinary rows
@pytest.mark.parametrize("algo", [0, 1])
def test_hub_has_long_kept_and_c_rows(algo):
    case = ug.hub()
    sigma = node_map(case)
    rec = ug.twin(case, algo)[0]
    f = ug.closure_facts(case, algo, rec)
    print("hub, algo %d: %d candidates, per block %s; hub row %d; candidates whose smaller end has a kept row > 16: %d; "
          "longest C row %d" % (algo, f["candidates"], f["per_block"], rec.kept.degrees()[sigma[0]],
                                f["long_row_candidates"], f["longest_c_row"]))
    assert rec.kept.degrees()[sigma[0]] >= 5000
    assert f["long_row_candidates"] >= 1000                            # the binary search on kept rows
    assert f["longest_c_row"] > 16


# ------------------------------------------------------------------ e. deep repair chains
@pytest.mark.parametrize("n,repaired", [(3_000, 1_523), (20_000, 10_158)])
def test_chain_drops_everything_and_repairs_deep(n, repaired):
    case = ug.chain(n)
    sigma = node_map(case)
    first, second = ug.twin(case, 0)
    np.testing.assert_array_equal(first.graph[2], ug.chain_weights(n))       # round 0 builds the sawtooth
    assert first.kept_m == n - 1 and first.repaired == 0 and len(first.cu) == 0
    assert second.kept_m == 0 and second.kept.m == 0 and len(second.cu) == 0  # the kept graph is empty
    isolates = int((second.kept.degrees() == 0).sum())
    target = ug.chain_targets(n)
    active, sweeps = ug.jacobi(target)
    print("chain %d: kept %d, isolates %d, Jacobi sweeps %d, repaired %d" % (n, second.kept.m, isolates, sweeps, second.repaired))
    assert isolates == n and (n <= 16384) == (n == 3_000)                     # ISO_LDS: the LDS path / the multi-block path
    assert sweeps > 8                                                         # the host loop of repair() goes round again
    assert second.repaired == repaired == int(active.sum()) == second.m       # graph_merge_next: no kept edge, added ones
    # the restatement names the model's repair edges, weights and ages (node order through npos)
    x = np.flatnonzero(active)
    y = target[x]
    o = np.lexsort((np.maximum(x, y), np.minimum(x, y)))
    u, v, w, age = second.graph
    np.testing.assert_array_equal(u, np.minimum(x, y)[o])
    np.testing.assert_array_equal(v, np.maximum(x, y)[o])
    np.testing.assert_array_equal(w, ug.chain_weights(n)[np.minimum(x, y)[o]])
    np.testing.assert_array_equal(age, (2 << orc.AGE_ITER_SHIFT) + orc.AGE_REPAIR_OFFSET + x[o])
    assert (np.diff(sigma[:64]) < 0).any()                                    # internal ids do not follow node order


# ------------------------------------------------------------------ f. degenerate attempt counts
def test_ring_attempt_counts_cover_the_block_rule():
    blocks = {(a, algo): ug.blocks_of(algo, a)[0] for a in ug.RING_ATTEMPTS for algo in (0, 1)}
    print("ring: blocks by (attempts, algo)", blocks)
    assert [blocks[a, 0] for a in ug.RING_ATTEMPTS] == [1, 1, 3, 4, 4, 4, 4]
    assert [blocks[a, 1] for a in ug.RING_ATTEMPTS] == [1, 1, 3, 5, 15, 16, 16]
    assert ug.RING_N == 1 << 6                                                # ids fill key_bits exactly
    for a in ug.RING_ATTEMPTS:
        for algo in (0, 1):
            case = ug.ring(a)
            rec = ug.twin(case, algo)[0]
            assert rec.kept.m == ug.RING_N and rec.repaired == 0
            assert len(rec.cu) <= a and rec.m == ug.RING_N + len(rec.cu)
            if a == 1:
                assert len(rec.cu) == 1                                       # every node of a ring has two neighbours
            if a:
                assert (case.n - 1) in np.concatenate([rec.kept.u, rec.kept.v])


def test_ring_pair_list_holds_every_kind():
    case = ug.ring(0)
    cpu = ug.new_twin(case, node_map(case))
    ug.twin_update(cpu, 0, case.rounds[0])
    w = ug.twin_set_pairs(cpu, 0, case.rounds[0], ug.RING_PAIRS)
    cu, cv, cf = cpu.cand
    got = sorted((int(min(a, b)), int(max(a, b)), int(f)) for a, b, f in zip(cpu.npos[cu], cpu.npos[cv], cf))
    assert got == [(1, 63, 5), (61, 63, 0)]          # self pair, repeats, ring edges dropped; first occurrence kept
    assert len(w) == 2
    assert ug.twin_set_pairs(cpu, 0, case.rounds[0], np.zeros((0, 2), np.int32)).size == 0 and len(cpu.cand[0]) == 0


# ------------------------------------------------------------------ g. lane groups
def test_lane_groups_are_all_reached():
    groups = {n_r: ug.lane_group(n_r) for n_r in ug.LANE_N_R}
    print("k_pair_partial lanes per edge by n_r:", groups)
    assert set(groups.values()) == {1, 2, 4, 8, 16}
    assert groups[5] == 2 and groups[9] == 4 and groups[17] == 8 and groups[65] == 16
    assert (129 + 3) // 4 > 2 * 16                    # a lane makes a third trip
    n = golden_io.load("lfr1k_louvain_np20").N
    for n_r in ug.LANE_N_R:
        pos = ug.lane_positions(n_r)
        assert 0 in pos and n_r - 1 in pos
        if n_r >= 4:
            assert {p % 4 for p in pos} == {0, 1, 2, 3}
        sets = ug.lanes(n_r, n)
        assert [name for name, _ in sets] == ["random"] + pos
        for name, lab in sets[1:]:
            assert lab.shape == (n_r, n) and (np.delete(lab, name, axis=0) == 0).all() and len(np.unique(lab[name])) == 3


def test_pair_partial_restatement():
    lab = np.array([[0, 0, 1, 1], [0, 1, 1, 1], [0, 0, 0, 2]], np.int32)
    u, v = np.array([0, 1, 2, 0]), np.array([1, 2, 3, 0])
    assert ug.pair_partial(lab, u, v, 0).tolist() == [1, 0, 2, -1]
    assert ug.pair_partial(lab, u, v, 1).tolist() == [2, 2, 2, 3]
    case = golden_io.load("lfr1k_louvain_np20")
    g = orc.EdgeGraph.from_lines(case.N, case.edges_file)
    lab = case.cd_batches[0]
    np.testing.assert_array_equal(ug.pair_partial(lab, g.u, g.v, 1), orc.consensus(1, g, lab, case.n_p))


# ------------------------------------------------------------------ h. the keep rule
def test_keep_rule_products_round_as_stated():
    assert 0.7 * 10 == 7.0 and 0.1 * 30 == 3.0 and 0.2 * 5 == 1.0 and 0.6 * 5 == 3.0   # the weight at the cut is kept
    assert 0.07 * 100 == 0.14 * 50 == 7.000000000000001 > 7    # rounds above 7: weight 7 is dropped
    assert 0.58 * 50 == 28.999999999999996 < 29                # rounds below 29: weight 29 is kept
    assert {(0.7, 10), (0.2, 5), (0.6, 5), (0.1, 30), (0.07, 100), (0.58, 50)} <= set(ug.KEEP_RULES)
    for tau, n_p in ug.KEEP_RULES:
        case = ug.keep(tau, n_p)
        rec = ug.twin(case, 1)[0]
        w = ug.pair_partial(case.rounds[0].lab, case.u, case.v, 1)
        assert set(w.tolist()) == set(range(n_p + 1))          # every weight occurs
        keep = np.array([not (int(x) < tau * n_p) for x in w])
        np.testing.assert_array_equal(orc.threshold(w, tau, n_p), keep)
        assert rec.kept_m == int(keep.sum()) and rec.unconv == orc.check(w[keep], n_p, ug.DELTA)[1]
        cut = int(np.ceil(tau * n_p))
        assert keep[w == cut].all() and not keep[w == cut - 1].any()
    assert ug.twin(ug.keep(0.7, 10), 1)[0].kept.w.min() == 7
    assert ug.twin(ug.keep(0.07, 100), 1)[0].kept.w.min() == 8
    assert ug.twin(ug.keep(0.58, 50), 1)[0].kept.w.min() == 29
