"""The consensus hierarchy on the device (fc_consensus_levels / fc_consensus_cut) against
tests/consensus_levels_ref.py and against fc_consensus_partition at every level's threshold: the
tree, every field of every level record, the best level and the cuts, bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import consensus_levels_ref as lref
from tests import consensus_ref as cref
from tests import golden_io

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE, ELIMIT = -1, -4, -5
INTS = ("bucket_edges", "k", "max_size", "singletons", "in_weight")


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


@pytest.fixture(scope="module")
def lfr():
    case = golden_io.load("lfr1k_louvain_np20")
    u, v = cref.canonical_edges(case.edges_file[:, 0], case.edges_file[:, 1])
    return case, u, v


def engine(fcmod, n, u, v, labels=None, seed=1):
    eng = fcmod.Engine(seed=seed)
    eng.load_graph(n, u, v)
    if labels is not None:
        eng.set_labels(labels)
    return eng


def engine_order(eng, cu, cv):
    """positions of the canonical edges (cu, cv) in the engine's edge order of the input graph:
    sorted by the internal ids (smaller, larger) of their ends"""
    sig = eng.node_map().astype(np.int64)
    a, b = sig[cu], sig[cv]
    return np.lexsort((np.maximum(a, b), np.minimum(a, b)))


def to_device(eng, cu, cv, sup):
    """canonical-order supports -> the int32 device tensor fc_consensus_levels takes"""
    s = np.asarray(sup, np.int64)[engine_order(eng, cu, cv)] if len(sup) else np.zeros(1, np.int64)
    return torch.from_numpy(s.astype(np.int32)).to("cuda:0")


def canon(u, v, sup):
    """(cu, cv, sup) of distinct edges in canonical order"""
    lo, hi = np.minimum(u, v).astype(np.int64), np.maximum(u, v).astype(np.int64)
    o = np.lexsort((hi, lo))
    return lo[o], hi[o], np.asarray(sup, np.int64)[o]


def same_record(got, exp, tag):
    for f in INTS:
        assert int(got[f]) == exp[f], (tag, f, int(got[f]), exp[f])
    assert (int(got["tot_sq_hi"]) << 64) | int(got["tot_sq_lo"]) == exp["tot_sq"], tag
    assert float(got["modularity"]) == exp["modularity"], (tag, float(got["modularity"]), exp["modularity"])


def check(eng, n, cu, cv, sup, nt, dev=None, graph="input", w=None, cuts=None):
    """one consensus_levels call against the reference; `cuts`: the levels whose labels are compared
    with the reference cut, cut_tree and consensus_partition at theta_of(level) (None: every level)"""
    from fastconsensus_amd import cut_tree, theta_of
    lev = eng.consensus_levels(graph, dev_support=dev, n_total=None if dev is None else nt)
    birth, up = lref.tree(n, cu, cv, sup, nt)
    rec = lref.level_records(n, cu, cv, sup, nt, w=w, birth=birth, up=up)
    assert lev["n_total"] == nt and len(lev["levels"]) == nt + 1
    assert lev["birth"].dtype == lev["up"].dtype == np.int32
    assert np.array_equal(lev["birth"], birth) and np.array_equal(lev["up"], up)
    for s in range(nt + 1):
        same_record(lev["levels"][s], rec[s], s)
    assert lev["best_level"] == lref.best_level(rec)
    assert lev["best_theta"] == lref.theta_of(lev["best_level"], nt)
    for s in range(nt + 1) if cuts is None else cuts:
        lab, k = eng.consensus_cut(s)
        exp = lref.cut(birth, up, s)
        assert lab.dtype == np.int32 and np.array_equal(lab, exp), s
        assert k == rec[s]["k"] == int(exp.max()) + 1, s
        assert np.array_equal(cut_tree(lev["birth"], lev["up"], s), exp), s
        part = eng.consensus_partition(theta_of(s, nt), graph, dev_support=dev, n_total=None if dev is None else nt)
        assert np.array_equal(part["labels"], exp), s
        assert (part["k"], part["max_size"], part["singletons"]) == (rec[s]["k"], rec[s]["max_size"],
                                                                     rec[s]["singletons"]), s
    return lev, rec


# ------------------------------------------------------------------ 1. golden labelings
@pytest.mark.parametrize("batch", [0, -1])
@pytest.mark.parametrize("name", ["lfr1k_louvain_np20", "karate_louvain_np50", "lfr1k_mu055_lpm_np20",
                                  "lfr1k_lpm_np20"])
def test_golden_labelings(fcmod, name, batch):
    case = golden_io.load(name)
    e = case.edges_file
    u, v = cref.canonical_edges(e[:, 0], e[:, 1])
    labs = case.cd_batches[batch]
    sup = cref.support(labs, u, v)
    with engine(fcmod, case.N, e[:, 0], e[:, 1], labs) as eng:
        dev = eng.consensus_support("input")
        assert np.array_equal(dev.cpu().numpy(), sup[engine_order(eng, u, v)])     # the order the tests hand supports in
        lev, rec = check(eng, case.N, u, v, sup, case.n_p)
        if (name, batch) == ("lfr1k_louvain_np20", 0):
            assert lev["best_level"] == 12 and int((lev["levels"]["bucket_edges"] > 0).sum()) == 21
        if (name, batch) == ("karate_louvain_np50", 0):
            assert lev["best_level"] == 31 and int((lev["levels"]["bucket_edges"] > 0).sum()) == 16
        again = eng.consensus_levels("input", dev_support=dev, n_total=case.n_p)    # the support handed in
        assert all(np.array_equal(again[k], lev[k]) for k in lev)


# ------------------------------------------------------------------ 2. against fc_score_partitions
@pytest.mark.parametrize("graph", ["input", "working"])
def test_level_records_equal_the_scores_of_the_cuts(fcmod, lfr, graph):
    case, cu, cv = lfr
    e = case.edges_file
    with engine(fcmod, case.N, e[:, 0], e[:, 1], seed=11) as eng:
        w = None
        if graph == "working":
            eng.run(0, 20, 0.2, 0.02)
            cu, cv, w, _ = eng.get_graph()
            assert int(w.max()) > 1
            labs = eng.get_labels(20)
        else:
            labs = case.cd_batches[0]
            eng.set_labels(labs)
        sup = cref.support(labs, cu, cv)
        picks = sorted({0, 1, 7, 12, 19, 20})
        lev, _ = check(eng, case.N, cu, cv, sup, 20, graph=graph, w=w, cuts=picks)
        cuts = np.stack([eng.consensus_cut(s)[0] for s in picks])
        eng.set_labels(cuts)
        sc = eng.score_partitions(graph)
        for i, s in enumerate(picks):
            r = lev["levels"][s]
            for f in ("k", "max_size", "in_weight"):
                assert int(sc[f][i]) == int(r[f]), (s, f)
            assert int(sc["tot_sq"][i]) == (int(r["tot_sq_hi"]) << 64) | int(r["tot_sq_lo"]), s
            assert float(sc["modularity"][i]) == float(r["modularity"]), s


# ------------------------------------------------------------------ 3. the bucket kernel
def bucket_supports(kind, m, nt):
    rng = np.random.default_rng(nt)
    if kind == "uniform":
        return rng.integers(0, nt + 1, m)
    if kind == "equal":
        return np.full(m, nt // 2, np.int64)
    if kind == "distinct":
        return np.arange(m) % (nt + 1)
    return np.where(rng.random(m) < 0.5, 0, nt)          # extremes


@pytest.mark.parametrize("nt", [1, 2, 63, 64, 65, 2048])
def test_bucket_kernel(fcmod, lfr, nt):
    """supports handed in (engine order) on the LFR-1k graph, m = 13,637 edges: not a multiple of 64"""
    case, cu, cv = lfr
    e = case.edges_file
    m = len(cu)
    assert m % 64 != 0
    cuts = sorted({0, 1, nt // 2, nt - 1, nt})
    with engine(fcmod, case.N, e[:, 0], e[:, 1]) as eng:
        order = engine_order(eng, cu, cv)
        for kind in ("uniform", "equal", "distinct", "extremes"):
            sup = np.empty(m, np.int64)
            sup[order] = bucket_supports(kind, m, nt)        # the pattern in the order the kernel reads
            lev, rec = check(eng, case.N, cu, cv, sup, nt, dev=to_device(eng, cu, cv, sup), cuts=cuts)
            assert np.array_equal(lev["levels"]["bucket_edges"], np.bincount(sup, minlength=nt + 1)), kind
        keep = eng.consensus_cut(nt // 2)
        bad = sup.copy()
        bad[order[m - 1]] = nt + 1                           # one value outside [0, n_total], in the last wave
        rc, clean = raw_levels(eng, case.N, 0, to_device(eng, cu, cv, bad), nt)
        assert (rc, clean) == (EINVAL, True)
        again = eng.consensus_cut(nt // 2)                   # the earlier tree is still the context's
        assert np.array_equal(again[0], keep[0]) and again[1] == keep[1]


# ------------------------------------------------------------------ 4. tree shapes
def shape(name):
    """(n, u, v, sup, n_total) in the shape's own node ids"""
    rng = np.random.default_rng(len(name))
    if name == "path":                                   # every level merges fragments of a flattened forest
        n = 65536
        u, v = np.arange(n - 1), np.arange(1, n)
        return n, u, v, u % 8, 7
    if name == "star":
        n = 20001
        return n, np.zeros(n - 1, np.int64), np.arange(1, n), rng.integers(0, 17, n - 1), 16
    if name == "ladder":                                 # chain depth 2048: the longest cut and join walks
        n = 2049
        u = np.arange(n - 1)
        return n, u, u + 1, u, 2048
    if name == "triangles":                              # the third edge joins above its own support
        a = np.arange(0, 3000, 3)
        u, v = np.concatenate([a, a, a + 1]), np.concatenate([a + 1, a + 2, a + 2])
        return 3000, u, v, np.concatenate([np.full(2000, 5), np.zeros(1000, np.int64)]), 5
    if name == "edgeless":
        return 100, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), 3
    assert name == "tail"                                # nodes 30..49 appear in no edge
    u, v = cref.canonical_edges(rng.integers(0, 30, 40), rng.integers(0, 30, 40))
    return 50, u, v, rng.integers(0, 5, len(u)), 4


@pytest.mark.parametrize("name,permute", [("path", True), ("star", True), ("ladder", False), ("ladder", True),
                                          ("triangles", True), ("edgeless", False), ("tail", False)])
def test_tree_shapes(fcmod, name, permute):
    n, u, v, sup, nt = shape(name)
    if permute:
        p = np.random.default_rng(len(name)).permutation(n)
        u, v = p[u], p[v]
    cu, cv, sup = canon(u, v, sup)
    cuts = None if nt <= 16 else [0, 1, 2, 1023, 1024, 2046, 2047, 2048]
    with engine(fcmod, n, u, v) as eng:
        lev, rec = check(eng, n, cu, cv, sup, nt, dev=to_device(eng, cu, cv, sup), cuts=cuts)
    if name == "ladder" and not permute:
        assert np.array_equal(lev["birth"], np.arange(-1, n - 1)) and np.array_equal(lev["up"][1:], np.arange(n - 1))
        assert [int(r["k"]) for r in lev["levels"][[0, 1, 2047, 2048]]] == [1, 2, 2048, 2049]
    if name == "triangles":
        j = lref.join_levels(cu, cv, lev["birth"], lev["up"])
        assert int((j > sup).sum()) == 1000 and np.all(lev["levels"]["in_weight"] == 3000)
        assert [int(x) for x in lev["levels"]["k"]] == [1000] * 6 and lev["best_level"] == 5
    if name == "edgeless":
        assert np.all(lev["levels"]["k"] == n) and np.all(lev["levels"]["singletons"] == n)
        assert np.all(lev["levels"]["modularity"] == 0.0) and lev["best_level"] == nt
        assert np.all(lev["birth"] == -1) and np.array_equal(lev["up"], np.arange(n))
    if name == "path":
        assert [int(x) for x in lev["levels"]["k"]] == [rec[s]["k"] for s in range(8)] and rec[0]["k"] == 1


# ------------------------------------------------------------------ 5. determinism
def test_two_calls_give_identical_bytes(fcmod, lfr):
    case, _, _ = lfr
    e = case.edges_file
    with engine(fcmod, case.N, e[:, 0], e[:, 1], case.cd_batches[0]) as eng:
        a = eng.consensus_levels()
        ca = [eng.consensus_cut(s)[0].tobytes() for s in range(21)]
        b = eng.consensus_levels()
        cb = [eng.consensus_cut(s)[0].tobytes() for s in range(21)]
    for k in ("birth", "up", "levels"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["best_level"] == b["best_level"] and ca == cb


# ------------------------------------------------------------------ 6. read-only
def test_consensus_levels_is_read_only(fcmod, lfr):
    case, _, _ = lfr
    e = case.edges_file
    n_p, L = 20, len(lfr[1])

    def steps(eng, probe):
        for it in range(2):
            eng.cd(0, 0, n_p, n_p, it)
            probe(eng)
            part = torch.empty(eng.m, dtype=torch.int32, device="cuda:0")
            eng.consensus_partial(0, part)
            probe(eng)
            eng.consensus_apply(0, n_p, 0.2, 0.02, part)
            probe(eng)
            nc = eng.closure_sample(L, it)
            probe(eng)
            cnt = None
            if nc > 0:
                cnt = torch.zeros(nc, dtype=torch.int32, device="cuda:0")
                eng.closure_partial(cnt)
            probe(eng)
            eng.closure_apply(0, n_p, 0.02, cnt, it)
            probe(eng)

    def probe(eng):
        lev = eng.consensus_levels("input")
        eng.consensus_cut(lev["best_level"])
        eng.consensus_levels("working")
        eng.consensus_cut(n_p)

    with engine(fcmod, case.N, e[:, 0], e[:, 1], seed=9) as a, engine(fcmod, case.N, e[:, 0], e[:, 1], seed=9) as b:
        steps(a, probe)
        steps(b, lambda eng: None)
        assert all(np.array_equal(x, y) for x, y in zip(a.get_graph(), b.get_graph()))
        assert all(np.array_equal(x, y) for x, y in zip(a.get_nextgraph(), b.get_nextgraph()))
        assert np.array_equal(a.get_labels(n_p), b.get_labels(n_p))
        sa, sb = a.score_partitions("working"), b.score_partitions("working")
        assert all(np.array_equal(sa[k], sb[k]) for k in sa)


# ------------------------------------------------------------------ 7. errors
def raw_levels(eng, n, graph, sup, n_total, rows=4):
    """the C call with sentinel-filled outputs -> (code, outputs untouched)"""
    birth = np.full(n, -7, np.int32)
    up = np.full(n, -7, np.int32)
    levels = np.full(64 * rows, 0x5a, np.uint8)
    best = np.full(1, -7, np.int32)
    rc = eng._L.fc_consensus_levels(eng._ctx, graph, None if sup is None else sup.data_ptr(), n_total,
                                    birth.ctypes.data, up.ctypes.data, levels.ctypes.data,
                                    best.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    clean = bool((birth == -7).all() and (up == -7).all() and (levels == 0x5a).all() and best[0] == -7)
    return rc, clean


def raw_cut(eng, n, level):
    labels = np.full(n, -7, np.int32)
    k = ctypes.c_int64(-7)
    rc = eng._L.fc_consensus_cut(eng._ctx, level, labels.ctypes.data, ctypes.byref(k))
    return rc, bool((labels == -7).all() and k.value == -7)


def test_errors(fcmod, lfr):
    case, _, _ = lfr
    e = case.edges_file
    n = case.N
    with fcmod.Engine(seed=1) as eng:                                   # no graph loaded
        assert raw_levels(eng, 10, 0, None, 0) == (ESTATE, True)
        assert raw_cut(eng, 10, 0) == (ESTATE, True)
    with engine(fcmod, n, e[:, 0], e[:, 1]) as eng:                     # a graph, no labelings, no support
        assert raw_levels(eng, n, 0, None, 0) == (ESTATE, True)
        assert raw_cut(eng, n, 0) == (ESTATE, True)                     # no levels call yet
        with pytest.raises(fcmod.FastConsensusError) as ei:
            eng.consensus_levels()
        assert ei.value.code == ESTATE
        eng.set_labels(case.cd_batches[0][:3])
        for graph in (-1, 2, 7):
            assert raw_levels(eng, n, graph, None, 0) == (EINVAL, True), graph
        sup = eng.consensus_support("input")
        for nt in (0, -3):
            assert raw_levels(eng, n, 0, sup, nt) == (EINVAL, True), nt
        assert raw_levels(eng, n, 0, sup, 2049, rows=2050) == (ELIMIT, True)
        assert raw_levels(eng, n, 0, sup, 2) == (EINVAL, True)          # supports of 3 with n_total = 2
        assert raw_cut(eng, n, 0) == (ESTATE, True)                     # none of those left a tree
        with pytest.raises(ValueError):
            eng.consensus_levels(dev_support=sup)                       # dev_support without n_total
        with pytest.raises(ValueError):
            eng.consensus_levels("kept")
        assert raw_levels(eng, n, 0, sup, 3) == (0, False)
        for level in (-1, 4, 2049):
            assert raw_cut(eng, n, level) == (EINVAL, True), level
        assert raw_cut(eng, n, 3) == (0, False)
        eng.load_graph(n, e[:, 0], e[:, 1])                             # the tree belonged to the old graph
        assert raw_cut(eng, n, 3) == (ESTATE, True)


# ------------------------------------------------------------------ 8. public surface
def test_fast_consensus_best(fcmod, lfr):
    case, cu, cv = lfr
    e = case.edges_file
    nodes = np.arange(case.N) * 2 + 5
    g = fcmod.IdGraph(nodes, e[:, 0], e[:, 1])
    parts, sc, cons = fcmod.fast_consensus(g, "louvain", n_p=20, seed=3, scores=True, consensus="best")
    lv, levels = cons["level"], cons["levels"]
    assert cons["theta"] == fcmod.theta_of(lv, 20) and len(levels) == 21
    assert np.array_equal(cons["labels"], fcmod.cut_tree(cons["birth"], cons["up"], lv))
    assert sc["consensus_modularity"] == float(levels["modularity"][lv])
    w2 = 2 * len(cu)
    keys = [2 * int(r["in_weight"]) * w2 - ((int(r["tot_sq_hi"]) << 64) | int(r["tot_sq_lo"])) for r in levels]
    assert keys[lv] == max(keys) and all(keys[s] < keys[lv] for s in range(lv + 1, 21))
    labs = np.array([[p[x] for x in nodes.tolist()] for p in parts])
    sup = cref.support(labs, cu, cv)
    rec = lref.level_records(case.N, cu, cv, sup, 20)
    assert lv == lref.best_level(rec)
    for s in range(21):
        same_record(levels[s], rec[s], s)
    for k in ("support_hist", "node_in", "node_out", "stability", "k", "kept_edges", "partition"):
        assert k in cons
    assert cons["partition"] == dict(zip(nodes.tolist(), cons["labels"].tolist()))


def test_float_consensus_is_unchanged(fcmod, lfr):
    case, _, _ = lfr
    e = case.edges_file
    g = fcmod.IdGraph(np.arange(case.N), e[:, 0], e[:, 1])
    parts, cons = fcmod.fast_consensus(g, "louvain", n_p=20, seed=3, consensus=0.5)
    with fcmod.Engine(seed=3) as eng:
        eng.set_option("store", fcmod.core.store_order_pays(20, 0))
        eng.set_option("relabel", fcmod.core.relabel_for(0))
        eng.load_graph(g.n, g.u, g.v)
        eng.run(0, 20, 0.2, 0.02)
        exp = eng.consensus_partition(0.5)
    assert sorted(k for k in cons if k != "partition") == sorted(exp)
    for k, want in exp.items():
        assert np.array_equal(cons[k], want), k


def test_cli_consensus_levels(fcmod, tmp_path):
    path = os.path.join(golden_io.GOLDEN, "karate_club.txt")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "fast_consensus.py"), "-f", path, "-np", "10", "--seed", "5",
                        "--consensus-levels"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    g = fcmod.IdGraph.from_edgelist_file(path)
    with fcmod.Engine(seed=5) as eng:
        eng.load_graph(g.n, g.u, g.v)
        eng.run(0, 10, 0.2, 0.02)
        lev = eng.consensus_levels()
        exp = eng.consensus_cut(lev["best_level"])[0]
    d = tmp_path / "consensus_t0.2_d0.02_np10"
    rows = [ln.split("\t") for ln in (d / "levels.tsv").read_text().splitlines()]
    assert len(rows) == 11 and [int(r[0]) for r in rows] == list(range(11))
    assert [int(r[3]) for r in rows] == [int(x) for x in lev["levels"]["k"]]
    assert [float(r[6]) for r in rows] == [float(x) for x in lev["levels"]["modularity"]]
    by_node = dict(zip(g.labels.tolist(), exp.tolist()))
    lines = [list(map(int, ln.split())) for ln in (d / "partition").read_text().splitlines()]
    assert len(lines) == int(exp.max()) + 1
    for c, members in enumerate(lines):
        assert members and all(by_node[x] == c for x in members)
    mem = [tuple(map(int, ln.split("\t"))) for ln in (d / "membership").read_text().splitlines()]
    assert mem == sorted((k + 1, c + 1) for k, c in by_node.items())
