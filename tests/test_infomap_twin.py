"""The CPU twin of device Infomap (oracle/fc_oracle.c orc_engine_infomap, orc.engine_infomap), on
its own: no GPU.  The device is compared with it label for label in
tests/test_gpu_infomap_twin.py; that comparison is exact only where the twin counts no ambiguity,
so the conditions it rests on are asserted here, on any machine.

The twin restates leiden.hip's Infomap sequentially with applies by recomputation (module flows,
exit weights and Q from scratch after every bucket) and deltas in long double.  All Infomap state is
integer, so the device must agree wherever a decision is no near-tie.  Candidates with identical
integer inputs (exit_B, flow_B, w_to_B) are an exact tie (one pure function on identical arguments:
identical doubles on the device), resolved by hash then id; the others are ordered by the long
double delta.  A decision is AMBIGUOUS when a candidate with different integer inputs lies within
EPS = 1e-12 of the best delta or the best delta within EPS of the threshold -1e-10; EPS is 100 to
200 times the bound on the device's error in one delta (11 terms p log2 p, fc_log2 within 2.5 ulp:
below 1e-14; derivation beside IT_EPS in fc_oracle.c), derived and never tuned.  Two trials of a
replica within 1e-9 bits whose partitions differ are an ambiguous trial choice; trials of EQUAL
partitions are not (the device may pick either: the same renumbered labels).  Every case counts
zero of both.  A case that does not gets another seed (tests/infomap_graphs.py), never a relaxed
condition.  DESIGN.md "Leiden and Infomap" says the same.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.infomap_graphs import (CPU_CASES, INFOMAP_CASES, LISTS_OFF_CASE, THRESHOLD_A, InfomapCase, infomap_twin,
                                  topology)
from tests.leiden_graphs import codelength, plogp


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: c.id)
def test_zero_ambiguity(case):
    """No ambiguous decision and no ambiguous trial choice: a condition, not a tolerance."""
    tw = infomap_twin(case)
    for r, row in enumerate(tw.traces):
        for j, t in enumerate(row):
            print("%s replica %d trial %d: L %.9f | %s" % (case.id, case.rbegin + r, j, tw.trial_codelength[r, j],
                                                          t.summary()))
    print("%s: smallest margins: runner-up %.3g, threshold %.3g bits (EPS 1e-12); chosen trials %s, equivalent %s" % (
        case.id, min(t.margin_runner_up for t in tw.all_traces()), min(t.margin_threshold for t in tw.all_traces()),
        tw.best.tolist(), tw.equivalent.sum(1).tolist()))
    assert tw.ambiguous() == (0, 0)
    assert all(t.levels >= 2 for t in tw.all_traces())                       # at least two levels everywhere


def test_cases_reach_their_paths():
    """The preconditions of tests/test_gpu_infomap_twin.py, from the twin's trace: a graph that
    stops reaching the kernel path it is there for fails here."""
    dec, mov = np.zeros((2, 7), np.int64), np.zeros((2, 7), np.int64)
    adjacent = np.zeros(2, np.int64)
    levels_differ = False
    for case in CPU_CASES:
        tw = infomap_twin(case)
        tr = tw.all_traces()
        d, m = tw.decisions(), tw.moved()
        dec += d
        mov += m
        adjacent += sum(t.adjacent_movers for t in tr)
        levels_differ |= len({t.levels for t in tr}) > 1
        if case.d > 64:
            k = orc.leiden_class(case.d)
            # the hub's class is decided on the input graph and on an aggregate level, and moves
            assert d[0, k] > 0 and d[1, k] > 0 and m[0, k] > 0, (case.id, d.tolist(), m.tolist())
        if case.d > 128:
            # block_best_info's / wave_scan_info's (hash, id) order: an exact tie wider than a wave
            # that decided a move (only the hub's row has that many candidates), in every trial
            assert all(t.wide_ties_moved > 0 for t in tr), (case.id, [t.widest_tie for t in tr])
        if case.graph == "dense":
            # k_lv_heavy's own-weight accumulation (s_wown): in every trial, rows past 512 entries that
            # decide from inside a module holding some of their neighbours, and some of them move
            # (the path only: this case's labels do not depend on that weight, the d = 700 shard's do)
            assert all(t.heavy_own_weight > 1000 for t in tr), (case.id, [t.heavy_own_weight for t in tr])
            assert m[0, 3] > 0, (case.id, m.tolist())
        if case.graph == "lfr1k_consensus":
            w = topology(case)[2]
            assert w.max() > 1 and (w == 0).any(), "weights past 1 and weight-0 closure edges: both ignored"
        if case.graph == "lfr1k_weighted":
            assert topology(case)[2].max() > 1 and min(len(np.unique(x)) for x in tw.labels) > 1
        if case.d == 700 and case.rbegin:
            # the one case whose LABELS depend on k_lv_heavy's own weight: a hub that decides from
            # inside a module holding some of its neighbours
            assert sum(t.heavy_own_weight for t in tr) > 0, (case.id, [t.heavy_own_weight for t in tr])
        if case.graph == "threshold":
            # the -INFO_MIN_GAIN threshold: in every replica a best delta inside (-1e-10, -EPS) is held
            # back, and the held vertex ends in A, not in B where `delta < 0` would have sent it
            assert all(t.held_negative > 0 for t in tr), (case.id, [t.held_negative for t in tr])
            assert all(x[0] == x[1] and x[0] != x[1 + THRESHOLD_A] for x in tw.labels)
        if case.buckets > 1024 or case is LISTS_OFF_CASE:
            # the per-replica launch map (bmap grids) runs only on unlisted passes of the input graph
            assert case.count * case.trials > 1 and tw.partial_passes[0] > 0, (case.id, tw.partial_passes.tolist())
    print("decided", dec.tolist(), "moved", mov.tolist(), "adjacent movers", adjacent.tolist())
    assert (dec.sum(0) > 0).all() and (mov.sum(0) > 0).all()                 # every class decided AND moved
    assert (dec[:, 3:] > 0).all()                                            # classes past 512 on both kinds of level
    assert (adjacent > 0).all()        # lv_move's edge between two movers: 16-lane (input), 64-lane (aggregate)
    assert levels_differ               # finished replicas are dropped and the union rescanned


def _node_term(n, e):
    deg = np.bincount(e.ravel(), minlength=n).astype(np.float64)
    return float(plogp(deg / deg.sum()).sum())


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: c.id)
def test_codelength_is_the_map_equation(case):
    """The twin's codelength of every trial is the float64 two-level map equation of its labels,
    less the constant node term; the chosen trial is the earliest of the smallest."""
    tw = infomap_twin(case)
    n, e, _ = topology(case)
    nt = _node_term(n, e)
    for r in range(case.count):
        for j in range(case.trials):
            assert abs(tw.trial_codelength[r, j] - (codelength(n, e, tw.trial_labels[r, j]) + nt)) < 1e-9
        assert tw.codelength[r] == tw.trial_codelength[r].min()
        assert np.array_equal(tw.labels[r], tw.trial_labels[r, tw.best[r]])
        assert tw.labels[r].min() >= 0 and tw.labels[r].max() < n


def test_twin_lfr1k_vs_restatement():
    """The bounds test_infomap_lfr1k_vs_restatement applies to the device (LFR-1k, 16 replicas of 10
    trials): mean codelength within 0.5 % of the core restatement's and of igraph's full
    partition's (stored), mean NMI to planted >= theirs - 0.02."""
    from tests.test_infomap import full_restatement, lfr, nmi
    n, e, planted = lfr(1000, 0.4)
    g = orc.EdgeGraph.from_lines(n, e)
    tw = orc.engine_infomap(g, 16, 0, 0, 11)
    ref = [orc.infomap(g, seed=s)[0] for s in range(8)]
    full = full_restatement("lfr1k_mu04")
    Lt = np.mean([codelength(n, e, x) for x in tw.labels])
    Lr = np.mean([codelength(n, e, x) for x in ref])
    nt = np.mean([nmi(planted, x) for x in tw.labels])
    nr = np.mean([nmi(planted, x) for x in ref])
    print("infomap LFR-1k twin L %.4f NMI %.4f | core restatement L %.4f NMI %.4f | full L %.4f NMI %.4f"
          % (Lt, nt, Lr, nr, full["L_mean"], full["nmi_mean"]))
    assert abs(Lt - Lr) <= 0.005 * Lr
    assert abs(Lt - full["L_mean"]) <= 0.005 * full["L_mean"]
    assert nt >= nr - 0.02 and nt >= full["nmi_mean"] - 0.02


def test_twin_deterministic_and_independent_of_sharding():
    """Two runs are equal, and replicas 2..4 of a 6-replica batch equal the same replicas alone."""
    case = [c for c in INFOMAP_CASES if c.graph == "lfr1k" and c.count == 6][0]
    n, e, _ = topology(case)
    g = orc.EdgeGraph.from_lines(n, e)
    full = orc.engine_infomap(g, 6, 0, 4, 99, trials=2)
    again = orc.engine_infomap(g, 6, 0, 4, 99, trials=2)
    part = orc.engine_infomap(g, 3, 2, 4, 99, trials=2)
    assert np.array_equal(full.trial_labels, again.trial_labels)
    assert np.array_equal(full.trial_codelength, again.trial_codelength)
    assert np.array_equal(full.trial_labels[2:5], part.trial_labels)
    assert np.array_equal(full.codelength[2:5], part.codelength) and np.array_equal(full.best[2:5], part.best)
    assert len({x.tobytes() for x in full.labels}) > 1                      # the replicas differ
    other = orc.engine_infomap(g, 3, 2, 5, 99, trials=2)                    # the iteration keys the streams
    assert not np.array_equal(other.trial_labels, part.trial_labels)


def test_twin_independent_of_row_entry_order():
    """Permuting the entries inside every CSR row changes nothing: sums commute and candidates are
    ranked by a total order, which is why the device's hash-table row order cannot matter."""
    case = InfomapCase(700, 2, seed=5)
    n, e, _ = topology(case)
    g = orc.EdgeGraph.from_lines(n, e)
    rowptr, col, cw = g.csr()
    rng = np.random.default_rng(5)
    col2 = col.copy()
    for v in range(n):
        col2[rowptr[v]:rowptr[v + 1]] = rng.permutation(col[rowptr[v]:rowptr[v + 1]])
    assert not np.array_equal(col, col2)

    class Shuffled:
        N = n

        def __init__(self, c):
            self.c = c

        def csr(self):
            return rowptr, self.c, cw
    a = orc.engine_infomap(Shuffled(col), 2, 0, 0, 5, trials=2)
    b = orc.engine_infomap(Shuffled(col2), 2, 0, 0, 5, trials=2)
    assert np.array_equal(a.trial_labels, b.trial_labels) and np.array_equal(a.trial_codelength, b.trial_codelength)
