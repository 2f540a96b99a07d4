"""Leiden branch (fast_consensus.py:204-258, final pass :385-388, CD :121-123).

leidenalg is absent (requirements.txt pins it; not installed, not vendored), so its CD is
"parity unpinned": the oracle restates the published algorithm (oracle/fc_oracle.c
orc_leiden: queue-based move, constrained refinement, aggregation by the refined
partition) and the device is held to it statistically, with the tolerances written in each
test.  What the reference's loop does around the CD is deterministic and pinned here:
on integer-labelled graphs the str-keyed lookups (:97, :217) never match, so the loop
converges at check #1 after one iteration and the result is n_p Leiden runs on G -- recorded
by running the reference's leiden branch itself (karate/lfr1k_leiden_np20 fixtures,
tests/golden/make_golden.py r03, leidenalg and the process pool stubbed).
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def connected_communities(N, e, lab):
    """Leiden guarantees connected communities: every community induces a connected subgraph."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    same = lab[e[:, 0]] == lab[e[:, 1]]
    a = sp.coo_matrix((np.ones(int(same.sum())), (e[same, 0], e[same, 1])), shape=(N, N))
    ncomp, comp = connected_components(a, directed=False)
    # a community is connected iff all its members share one component of the in-community graph
    pairs = np.unique(np.stack([lab, comp], 1), axis=0)
    return len(pairs) == len(np.unique(lab))


def nmi(a, b):
    from sklearn.metrics import normalized_mutual_info_score
    return normalized_mutual_info_score(a, b)


def lfr(n, mu, seed=42):
    from fastconsensus_amd import synth
    u, v, planted = synth.lfr(n, mu, seed=seed)
    return n, np.stack([u, v], 1), planted


# ------------------------------------------------------------------------------ CPU: oracle
def test_oracle_leiden_beats_level0_and_connects():
    """The restatement's multi-level optimum has higher modularity than python-louvain's level
    0 on the same graph, and every community is connected (the Leiden guarantee)."""
    n, e, planted = lfr(1000, 0.4)
    g = orc.EdgeGraph.from_lines(n, e)
    ld, levels = orc.cd_batch(orc.LEIDEN, 8, g, seed=3)
    lv, _ = orc.cd_batch(orc.LOUVAIN, 8, g, seed=3)
    ql = np.mean([orc.modularity(g, x) for x in ld])
    q0 = np.mean([orc.modularity(g, x) for x in lv])
    assert ql >= q0 - 1e-9, (ql, q0)
    assert all(levels >= 1)
    assert np.mean([nmi(planted, x) for x in ld]) > 0.95
    for x in ld:
        assert connected_communities(n, e, x)
        assert x.min() == 0 and x.max() + 1 == len(np.unique(x))


def test_oracle_leiden_karate():
    e = np.loadtxt(os.path.join(golden_io.GOLDEN, "karate_club.txt"), dtype=np.int64)[:, :2]
    nodes, e = np.unique(e, return_inverse=True)
    e = e.reshape(-1, 2).astype(np.int32)
    g = orc.EdgeGraph.from_lines(len(nodes), e)
    ld, _ = orc.cd_batch(orc.LEIDEN, 16, g, seed=1)
    q = [orc.modularity(g, x) for x in ld]
    # karate's modularity optimum is 0.4198 (4 communities); Leiden reaches >= 0.40 every run
    assert min(q) >= 0.40 and max(q) <= 0.4199
    for x in ld:
        assert connected_communities(len(nodes), e, x)


def test_cover_matches_igraph_vertex_cover_usage():
    """core.Cover: what the reference reads from as_cover() (fast_consensus.py:123, :461-466)."""
    from fastconsensus_amd.core import Cover, labels_to_output
    c = Cover(np.array([2, 2, 0, 1, 1, 1, 0]))
    assert len(c) == 3
    assert list(c) == [[3, 4, 5], [0, 1], [2, 6]]      # size-descending, ties by first vertex
    assert c.membership == [[1], [1], [2], [0], [0], [0], [2]]
    assert c.sizes() == [3, 2, 2]
    # node labels -> igraph vertex ids = rank in sorted(G.nodes()) (nx_to_igraph :47)
    out = labels_to_output("leiden", np.array([5, 3, 4]), np.array([[0, 1, 1]], np.int32))
    assert list(out[0]) == [[0, 1], [2]]   # vertices 0,1 = nodes 3,4; vertex 2 = node 5


def test_cli_leiden_writer(tmp_path):
    """:463-466: the leiden output file holds '{vertex+1}\\t{cluster+1}' per vertex; the
    memberships directory is created and left empty."""
    from fastconsensus_amd.cli import build_parser, write_outputs
    from fastconsensus_amd.core import Cover
    args = build_parser().parse_args(["-f", "x", "--alg", "leiden", "-np", "2"])
    args.t = 0.2
    write_outputs(args, [Cover(np.array([1, 0, 0])), Cover(np.array([0, 0, 0]))], root=str(tmp_path))
    d = tmp_path / "out_partitions_t0.2_d0.02_np2"
    assert (d / "1").read_text() == "1\t2\n2\t1\n3\t1\n"
    assert (d / "2").read_text() == "1\t1\n2\t1\n3\t1\n"
    assert os.listdir(tmp_path / "memberships_t0.2_d0.02_np2") == []


@pytest.mark.parametrize("name", golden_io.LEIDEN_CASES)
def test_reference_leiden_branch_exit(name):
    """The reference's own leiden branch, run with leidenalg and the process pool stubbed
    (make_golden.py r03): on int-labelled graphs the first check (:229) sees an EMPTY graph --
    every weight stayed 0 (:213-221: int nodes never match the str(vertex id) keys of :97)
    and :223-227 removed every edge -- and converges; the result is the final pass (:385-388):
    n_p more Leiden runs on the unchanged input graph.  The engine's leiden loop is exactly
    this (fc_run(FC_ALGO_LEIDEN): one iteration, exit at check #1, final graph = G)."""
    case = golden_io.load(name)
    assert case.algo == 3 and case.meta["n_checks"] == 1 and case.checks[0][1] is True
    assert len(case.checks[0][0]) == 0                        # the checked graph is empty
    assert case.meta["n_cd_batches"] == 2                     # the loop's batch + the final pass
    fin, last = case.z["final_labels"], case.cd_batches[1]
    for a, b in zip(fin, last):                               # the output IS the final-pass CD
        assert len(np.unique(np.stack([a, b], 1), axis=0)) == len(np.unique(a)) == len(np.unique(b))


# ------------------------------------------------------------------------------ CPU: the twin
# orc.engine_leiden restates leiden.hip sequentially (oracle/fc_oracle.c orc_engine_leiden); the
# device is compared with it label for label in tests/test_gpu_leiden_twin.py.  Here: the twin
# itself is a sound Leiden, does not depend on what the device's hash tables may reorder, and the
# graphs of the GPU comparison reach the kernel paths they are meant to reach.
def _lfr1k():
    case = golden_io.load("lfr1k_louvain_np20")
    return case.N, case.edges_file


def test_twin_lfr1k_vs_restatement():
    """Tolerances of test_leiden_lfr1k_vs_restatement (the device's): mean modularity within 0.01
    of the sequential restatement, community count within 25 %; every community connected,
    labels contiguous after renumbering and within [0, n) before."""
    n, e = _lfr1k()
    g = orc.EdgeGraph.from_lines(n, e)
    tw, tr = orc.engine_leiden(g, 16, 0, 0, 11)
    ref, _ = orc.cd_batch(orc.LEIDEN, 16, g, seed=5)
    qt, qr = (np.mean([orc.modularity(g, x) for x in L]) for L in (tw, ref))
    kt, kr = (np.mean([len(np.unique(x)) for x in L]) for L in (tw, ref))
    print("twin LFR-1k Q %.4f k %.1f | restatement Q %.4f k %.1f" % (qt, kt, qr, kr))
    assert abs(qt - qr) <= 0.01
    assert abs(kt - kr) <= 0.25 * kr
    assert all(t.levels >= 2 for t in tr)
    for x, y in zip(tw, orc.renumber(tw)):
        assert x.min() >= 0 and x.max() < n
        assert connected_communities(n, e, x)
        assert y.min() == 0 and y.max() + 1 == len(np.unique(x))


@pytest.mark.parametrize("graph", ["lfr1k", 700])
def test_twin_independent_of_row_entry_order(graph):
    """Permuting the entries inside every CSR row leaves every label unchanged: sums commute and
    candidates are ranked by a total order, the stated reason why the device's hash-table order
    (aggregated rows) cannot matter."""
    from tests.leiden_graphs import hub_cliques
    n, e = _lfr1k() if graph == "lfr1k" else hub_cliques(graph, seed=3)
    g = orc.EdgeGraph.from_lines(n, e)
    rng = np.random.default_rng(5)
    if graph == "lfr1k":                                        # the weighted path too
        g = orc.EdgeGraph(n, g.u, g.v, rng.integers(1, 4, g.m), g.age)
    rowptr, col, cw = g.csr()
    col2, cw2 = col.copy(), cw.copy()
    for v in range(n):
        p = rng.permutation(int(rowptr[v + 1] - rowptr[v])) + rowptr[v]
        col2[rowptr[v]:rowptr[v + 1]], cw2[rowptr[v]:rowptr[v + 1]] = col[p], cw[p]
    assert not np.array_equal(col, col2)

    class Shuffled:
        N = n

        def __init__(self, c, w):
            self.c, self.w = c, w

        def csr(self):
            return rowptr, self.c, self.w
    a, _ = orc.engine_leiden(Shuffled(col, cw), 4, 0, 2, 23)
    b, _ = orc.engine_leiden(Shuffled(col2, cw2), 4, 0, 2, 23)
    assert np.array_equal(a, b)


def test_twin_independent_of_sharding():
    """Replicas 2..4 of a 6-replica batch equal the same replicas computed alone."""
    n, e = _lfr1k()
    g = orc.EdgeGraph.from_lines(n, e)
    full, _ = orc.engine_leiden(g, 6, 0, 1, 99)
    part, _ = orc.engine_leiden(g, 3, 2, 1, 99)
    assert np.array_equal(full[2:5], part)
    assert len({x.tobytes() for x in full}) > 1                 # the replicas differ


def test_twin_louvain_threshold_parameter():
    """tw_replica's stop threshold is a parameter now: engine_cd keeps python-louvain's 1e-7, so
    its labels are what they were (golden: the twin's own earlier output is the device's, checked
    bit for bit by the GPU parity tests); Leiden's level 0 runs on past it."""
    n, e = _lfr1k()
    g = orc.EdgeGraph.from_lines(n, e)
    _, sw = orc.engine_cd(0, g, 4, 0, 0, 7, shared=0)
    _, tr = orc.engine_leiden(g, 4, 0, 0, 7)
    assert all(int(t.move_sweeps[0]) >= int(s) for t, s in zip(tr, sw))


def test_gpu_twin_cases_reach_their_paths():
    """The preconditions of tests/test_gpu_leiden_twin.py, from the twin's trace (no GPU): a graph
    that stops reaching the kernel path it is there for fails here, on any machine."""
    from tests.leiden_graphs import LEIDEN_CASES, G2_OFF_CASE, leiden_twin, weighted_graph_cpu
    heavy_move = heavy_refine = levels_differ = False
    for case in LEIDEN_CASES + [G2_OFF_CASE]:
        lab, tr = leiden_twin(case)
        dec = sum(t.decisions for t in tr)
        mov = sum(t.moved for t in tr)
        agg = sum(t.agg for t in tr)
        print(case.id, "|", " || ".join(t.summary() for t in tr))
        assert all(t.levels >= 2 for t in tr), case.id                        # at least two levels everywhere
        levels_differ |= len({t.levels for t in tr}) > 1
        if case.graph == "lfr1k_weighted":
            assert weighted_graph_cpu(case)[3].max() > 1, "no weight past 1: not the weighted path"
        if case.d > 64:
            k = orc.leiden_class(case.d)
            assert (dec[:, k] > 0).all(), (case.id, dec.tolist())              # its class, in all three modes
        if case.d > 512:
            k = orc.leiden_class(case.d)
            assert agg[k] > 0, (case.id, agg.tolist())                         # a member-row sum in its tier
            heavy_move |= bool(mov[2, 3:].any())
            heavy_refine |= bool(mov[:2, 3:].any())
    # a heavy kernel that always answers "stay" would be caught: heavy rows do move, in both modes
    assert heavy_move and heavy_refine
    # the path that drops finished replicas and rescans: a batch whose replicas finish at different levels
    assert levels_differ


# ------------------------------------------------------------------------------ device
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


def device_leiden(fcmod, n, e, count, seed, rbegin=0, total=None):
    with fcmod.Engine(seed=seed) as eng:
        eng.load_graph(n, e[:, 0], e[:, 1])
        eng.cd(3, rbegin, count, total or count, 0)
        return eng.get_labels(count)


# Tolerances (C2-size LFR-1k, 32 replicas): mean modularity within 0.01 of the sequential
# restatement, mean NMI to planted >= restatement - 0.03, community count within 25 %;
# every device community connected.
@pytest.mark.gpu
def test_leiden_lfr1k_vs_restatement(fcmod):
    n, e, planted = lfr(1000, 0.4)
    g = orc.EdgeGraph.from_lines(n, e)
    dev = device_leiden(fcmod, n, e, 32, seed=11)
    ref, _ = orc.cd_batch(orc.LEIDEN, 32, g, seed=5)
    s = lambda L: (np.mean([orc.modularity(g, x) for x in L]), np.mean([nmi(planted, x) for x in L]),
                   np.mean([len(np.unique(x)) for x in L]))
    qd, nd, kd = s(dev)
    qr, nr, kr = s(ref)
    print("leiden LFR-1k device Q %.4f NMI %.4f k %.1f | restatement Q %.4f NMI %.4f k %.1f" % (qd, nd, kd, qr, nr, kr))
    assert abs(qd - qr) <= 0.01
    assert nd >= nr - 0.03
    assert abs(kd - kr) <= 0.25 * kr
    for x in dev:
        assert connected_communities(n, e, x)


# Tolerances (C3 LFR-100k, 8 device / 4 restatement replicas): mean modularity within 0.01,
# community count within 25 %, every device community connected.
@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_leiden_lfr100k_vs_restatement(fcmod):
    n, e, planted = lfr(100_000, 0.5)
    g = orc.EdgeGraph.from_lines(n, e)
    dev = device_leiden(fcmod, n, e, 8, seed=21)
    ref, _ = orc.cd_batch(orc.LEIDEN, 4, g, seed=7, nthreads=4)
    qd = np.mean([orc.modularity(g, x) for x in dev])
    qr = np.mean([orc.modularity(g, x) for x in ref])
    kd = np.mean([len(np.unique(x)) for x in dev])
    kr = np.mean([len(np.unique(x)) for x in ref])
    q0 = np.mean([orc.modularity(g, x) for x in orc.cd_batch(orc.LOUVAIN, 4, g, seed=7, nthreads=4)[0]])
    print("leiden LFR-100k device Q %.4f k %.1f | restatement Q %.4f k %.1f | louvain level 0 Q %.4f" %
          (qd, kd, qr, kr, q0))
    assert abs(qd - qr) <= 0.01
    assert qd > q0                      # aggregation levels beat level 0
    assert abs(kd - kr) <= 0.25 * kr
    for x in dev[:2]:
        assert connected_communities(n, e, x)


@pytest.mark.gpu
def test_leiden_independent_of_sharding_and_deterministic(fcmod):
    n, e, _ = lfr(1000, 0.4)
    full = device_leiden(fcmod, n, e, 6, seed=99)
    again = device_leiden(fcmod, n, e, 6, seed=99)
    part = device_leiden(fcmod, n, e, 2, seed=99, rbegin=3, total=6)
    assert np.array_equal(full, again)
    assert np.array_equal(full[3:5], part)


@pytest.mark.gpu
def test_leiden_run_semantics(fcmod):
    """fc_run(leiden): one iteration, exit at check #1, n_p final runs on G (whose labels
    equal the final-pass CD), partition_edges = n_p*m; sharded driver equal."""
    n, e, _ = lfr(1000, 0.4)
    from fastconsensus_amd.distributed import run_sharded
    with fcmod.Engine(seed=5) as eng:
        eng.load_graph(n, e[:, 0], e[:, 1])
        labels, st = eng.run(3, 10, 0.2, 0.02)
        m = eng.m
        sh, st2 = run_sharded(eng, 3, 10, 0.2, 0.02)
        eng.cd(3, 0, 10, 10, 0x40000000)
        direct = eng.get_labels(10, renumber=True)
    assert st["iterations"] == 1 and st["exit_check"] == 1 and st["m_final"] == m
    assert st["partition_edges"] == 10 * m
    assert np.array_equal(labels, direct) and np.array_equal(sh, labels)
    assert st2["iterations"] == 1 and st2["exit_check"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", golden_io.LEIDEN_CASES)
def test_leiden_run_matches_reference_fixture(fcmod, name):
    """fc_run(FC_ALGO_LEIDEN) against the reference-run fixture: the same number of loop
    iterations (CD batches before the final pass), the same exit check, and a final graph equal
    to the input graph with unit weights (the graph the reference's final pass ran on)."""
    case = golden_io.load(name)
    e = case.edges_file
    with fcmod.Engine(seed=7) as eng:
        eng.load_graph(case.N, e[:, 0], e[:, 1])
        m0 = eng.m
        u0, v0, _, _ = eng.get_graph()
        labels, st = eng.run(3, case.n_p, case.tau, case.delta)
        u, v, w, _ = eng.get_graph()
    assert st["iterations"] == case.meta["n_cd_batches"] - 1
    assert st["exit_check"] == 1 and case.checks[-1][1]
    assert m0 == case.meta["m"] and st["m_final"] == case.meta["m"]
    assert np.array_equal(u, u0) and np.array_equal(v, v0) and (w == 1).all()
    assert labels.shape == (case.n_p, case.N)


@pytest.mark.gpu
def test_fast_consensus_leiden_returns_covers(fcmod):
    import networkx as nx
    G = nx.read_edgelist(golden_io.GOLDEN + "/karate_club.txt", nodetype=int)
    out = fcmod.fast_consensus(G, algorithm="leiden", n_p=8, seed=2)
    assert len(out) == 8
    verts = set(range(G.number_of_nodes()))
    for cov in out:
        clusters = list(cov)
        assert sorted(v for c in clusters for v in c) == sorted(verts)
        sizes = [len(c) for c in clusters]
        assert sizes == sorted(sizes, reverse=True)
        assert len(cov.membership) == G.number_of_nodes()


@pytest.mark.gpu
def test_cli_leiden_end_to_end_on_device(fcmod, tmp_path):
    shutil.copy(os.path.join(golden_io.GOLDEN, "karate_club.txt"), tmp_path / "karate.txt")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "fast_consensus.py"), "-f", "karate.txt", "--alg",
                        "leiden", "-np", "5"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    outd = tmp_path / "out_partitions_t0.2_d0.02_np5"
    assert sorted(os.listdir(outd), key=int) == ["1", "2", "3", "4", "5"]
    n = len({int(x) for ln in open(tmp_path / "karate.txt") for x in ln.split()[:2]})
    for fn in os.listdir(outd):
        rows = [ln.split("\t") for ln in (outd / fn).read_text().splitlines()]
        assert [int(r[0]) for r in rows] == list(range(1, n + 1))
        assert min(int(r[1]) for r in rows) == 1
    assert os.listdir(tmp_path / "memberships_t0.2_d0.02_np5") == []


@pytest.mark.gpu
@pytest.mark.parametrize("algo", [3, 4])
def test_multilevel_edge_cases(fcmod, algo):
    """Isolated nodes, an edgeless graph and disjoint components (Leiden: 3, Infomap: 4): labels
    stay in [0, n), isolated nodes alone, components never merged."""
    # two triangles + a path, plus isolated nodes 9..11
    e = np.array([[0, 1], [1, 2], [0, 2], [3, 4], [4, 5], [3, 5], [6, 7], [7, 8]], np.int32)
    n = 12
    with fcmod.Engine(seed=3) as eng:
        eng.load_graph(n, e[:, 0], e[:, 1])
        eng.cd(algo, 0, 4, 4, 0)
        lab = eng.get_labels(4, renumber=True)
    for x in lab:
        assert x.min() >= 0 and x.max() < n
        for a_, b_ in [(0, 3), (3, 6), (0, 6)]:
            assert x[a_] != x[b_]                      # components never share a community
        assert len({x[9], x[10], x[11]}) == 3 and not set(x[9:]) & set(x[:9])
        assert x[0] == x[1] == x[2] and x[3] == x[4] == x[5]
    with fcmod.Engine(seed=3) as eng:                 # no edges at all: singletons
        eng.load_graph(5, np.zeros(0, np.int32), np.zeros(0, np.int32))
        eng.cd(algo, 0, 2, 2, 0)
        lab = eng.get_labels(2, renumber=True)
    assert (lab == np.arange(5)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("algo", [0, 1, 3, 4])
def test_run_on_edgeless_graph(fcmod, algo):
    """An edgeless G: every algorithm returns singletons (python-louvain returns one community
    per node for a graph without edges; the loop converges on the empty graph)."""
    with fcmod.Engine(seed=1) as eng:
        eng.load_graph(6, np.zeros(0, np.int32), np.zeros(0, np.int32))
        labels, st = eng.run(algo, 3, 0.2, 0.02)
    assert (labels == np.arange(6)).all() and st["m_final"] == 0
