"""Device Infomap (leiden.hip, the MODE_INFO instances) against its sequential CPU twin
(oracle/fc_oracle.c orc_engine_infomap), label for label: the four k_lv_decide variants and the four
k_lv_heavy tiers, the exit-weight bookkeeping of lv_move under simultaneous moves (16 lanes per
mover on the input graph, 64 above it and for heavy rows), wave_scan_info's compaction,
block_best_info, the -INFO_MIN_GAIN threshold (the `threshold` case: a best delta of -9.7e-12 that
must be held back, and whose vertex ends elsewhere if it is not), the bucket lists against the
unlisted scan, the per-replica launch map, the aggregation by modules and the best-of-trials choice.

There is no tolerance anywhere.  All Infomap state is integer; only the comparison of candidates is
in doubles, and the twin (long double deltas, applies by recomputation from scratch) counts every
decision whose outcome the device's rounding could change: a candidate with different integer
inputs within EPS = 1e-12 of the best delta, or a best delta within EPS of the threshold -1e-10 (EPS:
100 to 200 times the bound on the device's error, derived beside IT_EPS in fc_oracle.c), and every
pair of trials within 1e-9 bits whose partitions differ.  Every case here counts zero of both
(asserted without a GPU in tests/test_infomap_twin.py, and again here on the graph and numbering the
engine really used), so the device's labels are determined: get_labels() must equal the twin's, and
get_labels(renumber=True) orc.renumber of them.  One freedom remains, and only it: trials of a
replica that end in the SAME partition have codelengths equal up to the summation order, so the
device may keep either; the renumbered labels are the same, the final-level ids are those of one of
these trials (InfomapTwin.accepts).  That each graph reaches the path it is here for is asserted
from the twin's trace in tests/test_infomap_twin.py and confirmed here from the engine's byte
counters.  DESIGN.md "Leiden and Infomap" says the same.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import golden_io
from tests.infomap_graphs import (CHILD_CASES, CONSENSUS_NP, G2_OFF_CASE, INFOMAP_CASES, LISTS_OFF_CASE,
                                  RELABEL_CASE, infomap_twin)
from tests.leiden_graphs import WEIGHTED_NP

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


def dev_i32(n):
    return torch.zeros(max(int(n), 1), dtype=torch.int32, device="cuda")


def run_infomap(eng, case):
    """Loads the case's graph into `eng` (whose seed is case.seed) and runs it.  Returns (labels,
    renumbered labels, stats of the Infomap run alone, the working graph (n, u, v, w) the run saw,
    the engine's node map)."""
    if case.buckets:
        eng.set_params(buckets=case.buckets)
    eng.set_option("infomap_trials", case.trials)
    if case.relabel != 1:
        eng.set_option("relabel", case.relabel)
    if case.graph == "lfr1k_consensus":
        # one lpm-style consensus step of the step API: co-membership weights, weight-0 closure edges
        gc = golden_io.load("lfr1k_lpm_np20")
        n, e = gc.N, gc.edges_file
        eng.load_graph(n, e[:, 0], e[:, 1])
        eng.cd(1, 0, CONSENSUS_NP, CONSENSUS_NP, 0)
        part = dev_i32(eng.m)
        eng.consensus_partial(1, part)
        eng.consensus_apply(1, CONSENSUS_NP, gc.tau, gc.delta, part)
        cnt = dev_i32(eng.closure_set_pairs(gc.pair_batches[0], 0))
        eng.closure_partial(cnt)
        eng.closure_apply(1, CONSENSUS_NP, gc.delta, cnt, 0)
    elif case.graph == "lfr1k_weighted":
        # one Louvain iteration of the step API, as tests/test_gpu_leiden_twin.py builds it
        gc = golden_io.load("lfr1k_louvain_np20")
        n, e = gc.N, gc.edges_file
        eng.load_graph(n, e[:, 0], e[:, 1])
        eng.cd(0, 0, WEIGHTED_NP, WEIGHTED_NP, 0)
        part = dev_i32(eng.m)
        eng.consensus_partial(0, part)
        eng.consensus_apply(0, WEIGHTED_NP, gc.tau, gc.delta, part)
        cnt = dev_i32(eng.closure_set_pairs(gc.pair_batches[0], 0))
        eng.closure_partial(cnt)
        eng.closure_apply(0, WEIGHTED_NP, gc.delta, cnt, 0)
    else:
        n, e = case.edges()
        eng.load_graph(n, e[:, 0], e[:, 1])
    u, v, w, _ = eng.get_graph()
    eng.collect_timing()                                   # counters from here on: the Infomap run's
    eng.cd(4, case.rbegin, case.count, case.total, case.iteration)
    lab = eng.get_labels(case.count)
    ren = eng.get_labels(case.count, renumber=True)
    return lab, ren, eng.collect_timing(), (n, u, v, w), eng.node_map()


def device_infomap(fc, case):
    """Runs the case on a new engine (run_infomap)."""
    with fc.Engine(seed=case.seed) as eng:
        return run_infomap(eng, case)


def check_case(case, lab, ren, st, graph, sigma):
    tw = infomap_twin(case, graph, sigma)
    for r, row in enumerate(tw.traces):
        for j, t in enumerate(row):
            print("%s replica %d trial %d%s: L %.9f | %s" % (
                case.id, case.rbegin + r, j, " (chosen)" if j == tw.best[r] else "", tw.trial_codelength[r, j],
                t.summary()))
    # the twin determines the device's labels only where it counts no ambiguity (also asserted, for
    # the graphs the oracle can build alone, in tests/test_infomap_twin.py)
    assert tw.ambiguous() == (0, 0), "ambiguous (decisions, trial choices): this case needs another seed"
    assert all(t.levels >= 2 for t in tw.all_traces())
    dec = tw.decisions()
    # device-side confirmation of the path: the heavy kernels' byte counter moves exactly when the
    # twin decided a row of more than 512 entries
    assert st["lv_decide_bytes"] > 0
    assert (st["lv_heavy_bytes"] > 0) == bool(dec[:, 3:].any()), (st["lv_heavy_bytes"], dec.tolist())
    if case.d:
        assert (st["lv_heavy_bytes"] > 0) == (case.d > 512)
    if case.graph == "lfr1k_consensus":
        assert graph[3].max() > 1 and (graph[3] == 0).any(), "not the weighted working graph"
    if case.graph == "lfr1k_weighted":
        assert graph[3].max() > 1, "no weight past 1: not the weighted working graph"
    exp = tw.labels
    bad = [(r, int((lab[r] != exp[r]).sum())) for r in range(case.count) if not tw.accepts(r, lab[r])]
    assert not bad, "replicas (local index, vertices differing from the chosen trial) %s" % bad
    assert np.array_equal(ren, orc.renumber(exp))
    if tw.equivalent.sum() == case.count:                      # no two trials of one partition: nothing is left open
        assert np.array_equal(lab, exp)


@pytest.mark.parametrize("case", INFOMAP_CASES + [RELABEL_CASE], ids=lambda c: c.id)
def test_infomap_bit_exact_vs_twin(fcmod, case):
    check_case(case, *device_infomap(fcmod, case))


@pytest.mark.parametrize("case", [LISTS_OFF_CASE, G2_OFF_CASE], ids=lambda c: c.id)
def test_infomap_switch_off_bit_exact_vs_twin(fcmod, case):
    """FC_INFO_LISTS=0: every bucket launch scans the union (input graph: the per-replica launch map
    once some replicas have stopped moving) in place of the compacted bucket lists.  FC_LV_G2=0:
    rows of 65..128 entries on k_lv_decide<.., LWS, 1> in place of the two-vertex-per-wave variant.
    Each switch is read once per process, so the run is a fresh child process."""
    out = subprocess.run([sys.executable, "-c",
                          "import json, sys; sys.path.insert(0, %r)\n"
                          "import fastconsensus_amd as fc\n"
                          "from tests import test_gpu_infomap_twin as t\n"
                          "lab, ren, st, g, sigma = t.device_infomap(fc, t.CHILD_CASES[%r])\n"
                          "print('RUN', json.dumps([lab.tolist(), ren.tolist(), st, sigma.tolist()]))\n"
                          % (ROOT, case.id)],
                         env=dict(os.environ, **case.env), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lab, ren, st, sigma = json.loads([l for l in out.stdout.splitlines() if l.startswith("RUN ")][-1][4:])
    n, e = case.edges()
    g = orc.EdgeGraph.from_lines(n, e)
    check_case(case, np.array(lab, np.int32), np.array(ren, np.int32), st, (n, g.u, g.v, g.w),
               np.array(sigma, np.int32))
