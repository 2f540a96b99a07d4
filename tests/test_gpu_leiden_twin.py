"""Device Leiden (leiden.hip) against its sequential CPU twin (oracle/fc_oracle.c
orc_engine_leiden), label for label: every decide variant of k_lv_decide, the four tiers of
k_lv_heavy and k_ag_rows_heavy, the weighted path, bucket counts, a shard of a larger batch.
Everything is integer, so there are no tolerances.  That each graph reaches the path it is here
for is asserted from the twin's trace in tests/test_leiden.py (no GPU) and confirmed here from
the engine's own byte counters.

Infomap runs on the same graphs here for its weak properties only: range, determinism, sharding,
and a codelength no worse than the two trivial partitions.  Its label-for-label comparison is in
tests/test_gpu_infomap_twin.py, against its own twin (orc_engine_infomap: all Infomap state is
integer, and the twin counts the decisions the floating-point deltas could leave open).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import golden_io
from tests.leiden_graphs import (G2_OFF_CASE, INFOMAP_D, LEIDEN_CASES, WEIGHTED_NP, LeidenCase, codelength,
                                 leiden_twin)

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


def run_leiden(eng, case):
    """Loads the case's graph into `eng` (whose seed is case.seed) and runs it.  Returns (labels,
    renumbered labels, stats of the Leiden run alone, the working graph (n, u, v, w) the run saw,
    the engine's node map)."""
    if case.buckets:
        eng.set_params(buckets=case.buckets)
    if case.graph == "lfr1k_weighted":
        # one Louvain iteration of the step API: consensus weights up to WEIGHTED_NP
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
    eng.collect_timing()                                   # counters from here on: the Leiden run's
    eng.cd(3, case.rbegin, case.count, case.total, case.iteration)
    lab = eng.get_labels(case.count)
    ren = eng.get_labels(case.count, renumber=True)
    return lab, ren, eng.collect_timing(), (n, u, v, w), eng.node_map()


def device_leiden(fc, case):
    """Runs the case on a new engine (run_leiden)."""
    with fc.Engine(seed=case.seed) as eng:
        return run_leiden(eng, case)


def check_case(case, lab, ren, st, graph, sigma):
    exp, tr = leiden_twin(case, graph, sigma)
    for r, t in enumerate(tr):
        print("%s replica %d: %s" % (case.id, case.rbegin + r, t.summary()))
    assert all(t.levels >= 2 for t in tr)
    dec = sum(t.decisions for t in tr)
    # device-side confirmation of the path: the heavy kernels' byte counter moves exactly when the
    # twin decided a row of more than 512 entries
    assert st["lv_decide_bytes"] > 0
    assert (st["lv_heavy_bytes"] > 0) == bool(dec[:, 3:].any()), (st["lv_heavy_bytes"], dec.tolist())
    if case.d:
        assert (st["lv_heavy_bytes"] > 0) == (case.d > 512)
    if case.graph == "lfr1k_weighted":
        assert graph[3].max() > 1, "no weight past 1: not the weighted path"
    bad = [(r, int((lab[r] != exp[r]).sum())) for r in range(case.count) if not np.array_equal(lab[r], exp[r])]
    assert not bad, "replicas (local index, differing vertices) %s" % bad
    assert np.array_equal(lab, exp)
    assert np.array_equal(ren, orc.renumber(exp))


@pytest.mark.parametrize("case", LEIDEN_CASES, ids=lambda c: c.id)
def test_leiden_bit_exact_vs_twin(fcmod, case):
    check_case(case, *device_leiden(fcmod, case))


def test_leiden_g2_off_bit_exact_vs_twin(fcmod):
    """FC_LV_G2=0: rows of 65..128 entries on k_lv_decide<.., LWS, 1> (one vertex per wave) in
    place of the two-vertex-per-wave variant; the switch is read once per process, so the run
    is a child process."""
    case = G2_OFF_CASE
    out = subprocess.run([sys.executable, "-c",
                          "import json, sys; sys.path.insert(0, %r)\n"
                          "import fastconsensus_amd as fc\n"
                          "from tests import test_gpu_leiden_twin as t\n"
                          "lab, ren, st, g, sigma = t.device_leiden(fc, t.G2_OFF_CASE)\n"
                          "print('RUN', json.dumps([lab.tolist(), ren.tolist(), st, sigma.tolist()]))\n" % ROOT],
                         env=dict(os.environ, FC_LV_G2="0"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lab, ren, st, sigma = json.loads([l for l in out.stdout.splitlines() if l.startswith("RUN ")][-1][4:])
    n, e = case.edges()
    g = orc.EdgeGraph.from_lines(n, e)
    check_case(case, np.array(lab, np.int32), np.array(ren, np.int32), st, (n, g.u, g.v, g.w),
               np.array(sigma, np.int32))


# ------------------------------------------------------------------ Infomap on the same graphs
def device_infomap(fc, n, e, count, seed, rbegin=0, total=None):
    with fc.Engine(seed=seed) as eng:
        eng.set_option("infomap_trials", 2)
        eng.load_graph(n, e[:, 0], e[:, 1])
        eng.cd(4, rbegin, count, total or count, 0)
        return eng.get_labels(count, renumber=True)


@pytest.mark.parametrize("d", INFOMAP_D)
def test_infomap_on_hub_graphs(fcmod, d):
    """Rows of 100, 700 and 5000 entries through the Infomap instances of the decide and heavy
    kernels: labels in range, two runs equal, a replica alone equals the same replica of the batch,
    and the float64 map-equation codelength of every device labeling is not above that of the
    all-singletons partition or of the one-module partition."""
    case = LeidenCase(d, 3, seed=29)
    n, e = case.edges()
    a = device_infomap(fcmod, n, e, 3, case.seed)
    b = device_infomap(fcmod, n, e, 3, case.seed)
    one = device_infomap(fcmod, n, e, 1, case.seed, rbegin=1, total=3)
    assert a.min() >= 0 and a.max() < n
    assert np.array_equal(a, b)
    assert np.array_equal(a[1:2], one)
    trivial = min(codelength(n, e, np.arange(n)), codelength(n, e, np.zeros(n, np.int64)))
    for x in a:
        L = codelength(n, e, x)
        print("infomap d=%d: %d modules, %.6f bits (trivial partitions: %.6f)" % (d, x.max() + 1, L, trivial))
        assert L <= trivial
