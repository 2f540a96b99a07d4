"""The consensus partition on the device (fc_consensus_support / fc_consensus_partition) against
tests/consensus_ref.py: labels, histogram, node sums and every info integer bit for bit;
stability exactly (both sides divide the same integers)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import consensus_ref as cref
from tests import golden_io, score_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THETAS = (0.5, 0.8, 1.0)


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


def same(got, exp, tag=""):
    for f in ("labels", "support_hist", "node_in", "node_out"):
        assert got[f].dtype == (np.int32 if f == "labels" else np.int64), (tag, f)
        assert np.array_equal(got[f], exp[f]), (tag, f)
    for f in cref.INFO_INTS:
        assert int(got[f]) == exp[f], (tag, f, int(got[f]), exp[f])
    assert got["cut"] == exp["cut"], tag
    assert np.array_equal(got["stability"], exp["stability"]), tag
    assert got["passes"] <= 64, tag


# ------------------------------------------------------------------ 1. golden labelings
@pytest.mark.parametrize("batch", [0, -1])
@pytest.mark.parametrize("name", ["lfr1k_louvain_np20", "lfr1k_mu03_lpm_np20", "karate_louvain_np50",
                                  "lfr1k_lpm_np20"])
def test_golden_labelings(fcmod, name, batch):
    case = golden_io.load(name)
    e = case.edges_file
    u, v = cref.canonical_edges(e[:, 0], e[:, 1])
    labs = case.cd_batches[batch]
    with engine(fcmod, case.N, e[:, 0], e[:, 1], labs) as eng:
        sup = eng.consensus_support("input").cpu().numpy()
        assert np.array_equal(np.bincount(sup, minlength=case.n_p + 1),
                              np.bincount(cref.support(labs, u, v), minlength=case.n_p + 1))
        for theta in THETAS:
            exp = cref.partition(case.N, u, v, theta, labels=labs)
            same(eng.consensus_partition(theta), exp, (name, batch, theta))


# ------------------------------------------------------------------ 2. working graph
def test_working_graph(fcmod, lfr):
    case, _, _ = lfr
    e = case.edges_file
    with engine(fcmod, case.N, e[:, 0], e[:, 1], seed=11) as eng:
        eng.run(0, 20, 0.2, 0.02)
        m = eng.m
        part = torch.empty(m, dtype=torch.int32, device="cuda:0")
        eng.consensus_partial(1, part)
        sup = eng.consensus_support("working")
        assert sup.shape == (m,) and torch.equal(sup, part)
        u, v, w, _ = eng.get_graph()
        labs = eng.get_labels(20)
        assert int(w.max()) > 1                      # a consensus graph, not G
        for theta in (0.5, 1.0):
            same(eng.consensus_partition(theta, "working"), cref.partition(case.N, u, v, theta, labels=labs), theta)


# ------------------------------------------------------------------ 3. replica counts of the count kernel
@pytest.mark.parametrize("n_r", [1, 3, 4, 5, 17, 64, 65])
def test_replica_counts(fcmod, lfr, n_r):
    case, u, v = lfr
    e = case.edges_file
    labs = np.random.default_rng(n_r).integers(0, 2, (n_r, case.N))
    with engine(fcmod, case.N, e[:, 0], e[:, 1], labs) as eng:
        exp = cref.partition(case.N, u, v, 0.5, labels=labs)
        assert 0 < exp["kept_edges"] < exp["edges"] or n_r == 1
        same(eng.consensus_partition(0.5), exp, n_r)


# ------------------------------------------------------------------ 4. shapes of the components kernel
def shape(name):
    """(n, u, v) with node ids randomly permuted"""
    if name == "path":
        n = 65536
        u, v = np.arange(n - 1), np.arange(1, n)
    elif name == "star":
        n = 20001
        u, v = np.zeros(n - 1, np.int64), np.arange(1, n)
    elif name == "triangles":
        n = 3000
        a = np.arange(0, n, 3)
        u, v = np.concatenate([a, a, a + 1]), np.concatenate([a + 1, a + 2, a + 2])
    elif name == "grid":
        s = 256
        n = s * s
        idx = np.arange(n).reshape(s, s)
        u = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
        v = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    elif name == "tree":
        n = 2 ** 16 - 1                                # complete binary tree of depth 15
        v = np.arange(1, n)
        u = (v - 1) // 2
    elif name == "edgeless":
        n = 100
        u = v = np.zeros(0, np.int64)
    elif name == "tail":
        n = 50                                         # nodes 30..49 appear in no edge
        rng = np.random.default_rng(3)
        return n, rng.integers(0, 30, 40), rng.integers(0, 30, 40)
    p = np.random.default_rng(len(name)).permutation(n)
    return n, p[u], p[v]


@pytest.mark.parametrize("name", ["path", "star", "triangles", "grid", "tree", "edgeless", "tail"])
def test_component_shapes(fcmod, name):
    n, u, v = shape(name)
    cu, cv = cref.canonical_edges(u, v)
    one = np.zeros((1, n), np.int32)
    exp = cref.partition(n, cu, cv, 1.0, labels=one)
    assert exp["kept_edges"] == len(cu)
    with engine(fcmod, n, u, v, one) as eng:
        got = eng.consensus_partition(1.0)
        same(got, exp, name)
        assert got["passes"] == (1 if len(cu) else 0)
    if name in ("path", "star", "grid", "tree"):
        assert exp["k"] == 1 and exp["max_size"] == n
    if name == "triangles":
        assert (exp["k"], exp["max_size"], exp["singletons"]) == (1000, 3, 0)
    if name == "edgeless":
        assert (exp["k"], exp["singletons"]) == (n, n)


def test_theta_zero_keeps_every_edge(fcmod, lfr):
    case, u, v = lfr
    e = case.edges_file
    labs = np.random.default_rng(0).integers(0, 50, (6, case.N))
    exp = cref.partition(case.N, u, v, 0.0, labels=labs)
    assert exp["kept_edges"] == exp["edges"] and exp["split_edges"] > 0
    assert np.array_equal(exp["labels"], cref.components(case.N, u, v))
    with engine(fcmod, case.N, e[:, 0], e[:, 1], labs) as eng:
        same(eng.consensus_partition(0.0), exp)


# ------------------------------------------------------------------ 5. float boundary
@pytest.mark.parametrize("n_total,theta,s,kept", [(10, 0.7, 7, True), (20, 0.8, 16, True), (25, 0.28, 7, False)])
def test_float_boundary(fcmod, lfr, n_total, theta, s, kept):
    """s - 1 all-equal labelings, one recorded partition A and n_total - s copies of another, B: an
    edge that A joins and B splits has support exactly s.  0.7 * 10 and 0.8 * 20 are exact in
    float64 (support on the cut: kept); 0.28 * 25 = 7.000000000000001 drops support 7."""
    case, u, v = lfr
    e = case.edges_file
    assert (theta * float(n_total) > s) == (not kept)
    a, b = case.cd_batches[0][0], case.cd_batches[-1][3]
    labs = np.stack([np.zeros(case.N, np.int64)] * (s - 1) + [a] + [b] * (n_total - s))
    exp = cref.partition(case.N, u, v, theta, labels=labs)
    hist = exp["support_hist"]
    assert hist[s] > 0 and hist[s - 1] > 0
    assert exp["kept_edges"] == int(hist[s if kept else s + 1:].sum())
    with engine(fcmod, case.N, e[:, 0], e[:, 1], labs) as eng:
        same(eng.consensus_partition(theta), exp)


# ------------------------------------------------------------------ 6. sharding invariance
def test_sharded_support_equals_one_engine(fcmod, lfr):
    case, _, _ = lfr
    e = case.edges_file
    labs = case.cd_batches[0]
    with engine(fcmod, case.N, e[:, 0], e[:, 1], labs[:12]) as a, \
            engine(fcmod, case.N, e[:, 0], e[:, 1], labs[12:]) as b, \
            engine(fcmod, case.N, e[:, 0], e[:, 1], labs) as whole:
        total = a.consensus_support("input") + b.consensus_support("input")
        assert torch.equal(total, whole.consensus_support("input"))
        for theta in THETAS:
            exp = whole.consensus_partition(theta)
            for eng in (a, b):
                got = eng.consensus_partition(theta, dev_support=total, n_total=20)
                assert sorted(got) == sorted(exp)
                for k in exp:
                    assert np.array_equal(got[k], exp[k]), (theta, k)


# ------------------------------------------------------------------ 7. read-only
def test_consensus_partition_is_read_only(fcmod, lfr):
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
        eng.consensus_partition(0.5, "input")
        eng.consensus_partition(0.8, "working")
        eng.score_pairs([(0, 1)])

    with engine(fcmod, case.N, e[:, 0], e[:, 1], seed=9) as a, engine(fcmod, case.N, e[:, 0], e[:, 1], seed=9) as b:
        steps(a, probe)
        steps(b, lambda eng: None)
        assert all(np.array_equal(x, y) for x, y in zip(a.get_graph(), b.get_graph()))
        assert all(np.array_equal(x, y) for x, y in zip(a.get_nextgraph(), b.get_nextgraph()))
        assert np.array_equal(a.get_labels(n_p), b.get_labels(n_p))
        sa, sb = a.score_partitions("working"), b.score_partitions("working")
        assert all(np.array_equal(sa[k], sb[k]) for k in sa)


# ------------------------------------------------------------------ 8. errors
def raw_partition(eng, n, graph, sup, n_total, agreement, hist_len=4):
    """the C call with sentinel-filled outputs -> (code, outputs untouched)"""
    labels = np.full(n, -7, np.int32)
    hist = np.full(hist_len, -7, np.int64)
    nin = np.full(n, -7, np.int64)
    nout = np.full(n, -7, np.int64)
    info = np.full(72, 0x5a, np.uint8)
    rc = eng._L.fc_consensus_partition(eng._ctx, graph, None if sup is None else sup.data_ptr(), n_total, agreement,
                                       labels.ctypes.data, hist.ctypes.data, nin.ctypes.data, nout.ctypes.data,
                                       info.ctypes.data)
    clean = bool((labels == -7).all() and (hist == -7).all() and (nin == -7).all() and (nout == -7).all()
                 and (info == 0x5a).all())
    return rc, clean


def test_errors(fcmod, lfr):
    case, _, _ = lfr
    e = case.edges_file
    n = case.N
    EINVAL, ESTATE, ELIMIT = -1, -4, -5
    with fcmod.Engine(seed=1) as eng:                                   # no graph loaded
        assert raw_partition(eng, 10, 0, None, 0, 0.5) == (ESTATE, True)
        assert eng._L.fc_consensus_support(eng._ctx, 0, None) == ESTATE
    with engine(fcmod, n, e[:, 0], e[:, 1]) as eng:                     # a graph, no labelings
        assert raw_partition(eng, n, 0, None, 0, 0.5) == (ESTATE, True)
        buf = torch.full((eng.m,), -7, dtype=torch.int32, device="cuda:0")
        assert eng._L.fc_consensus_support(eng._ctx, 0, buf.data_ptr()) == ESTATE
        with pytest.raises(fcmod.FastConsensusError) as ei:
            eng.consensus_partition(0.5)
        assert ei.value.code == ESTATE
        eng.set_labels(case.cd_batches[0][:3])
        for bad in (-0.1, 1.5, float("nan"), float("inf")):
            assert raw_partition(eng, n, 0, None, 0, bad) == (EINVAL, True), bad
        for graph in (-1, 2, 7):
            assert raw_partition(eng, n, graph, None, 0, 0.5) == (EINVAL, True), graph
            assert eng._L.fc_consensus_support(eng._ctx, graph, buf.data_ptr()) == EINVAL
        sup = eng.consensus_support("input")
        for nt in (0, -3):
            assert raw_partition(eng, n, 0, sup, nt, 0.5) == (EINVAL, True), nt
        assert raw_partition(eng, n, 0, sup, 2049, 0.5, hist_len=2050) == (ELIMIT, True)
        assert raw_partition(eng, n, 0, sup, 2, 0.5) == (EINVAL, True)   # supports of 3 with n_total = 2
        assert bool((buf == -7).all())
        assert raw_partition(eng, n, 0, sup, 3, 0.5) == (0, False)
        with pytest.raises(ValueError):
            eng.consensus_partition(0.5, "kept")
        with pytest.raises(ValueError):
            eng.consensus_partition(0.5, dev_support=sup)


# ------------------------------------------------------------------ 9. drop-in
def test_fast_consensus_consensus(fcmod, lfr):
    case, u, v = lfr
    e = case.edges_file
    planted = np.load(os.path.join(golden_io.GOLDEN, "lfr1k_mu04_planted.npy"))
    nodes = np.arange(case.N) * 2 + 5                                    # caller's node labels
    g = fcmod.IdGraph(nodes, e[:, 0], e[:, 1])
    kw = dict(n_p=20, seed=3, scores=True, truth=planted)
    parts0, sc0 = fcmod.fast_consensus(g, "louvain", **kw)
    parts, sc, cons = fcmod.fast_consensus(g, "louvain", consensus=0.5, **kw)
    assert parts == parts0 and set(sc0) < set(sc)
    # the float scores are sums whose order is not fixed where the scoring fallback adds them with
    # atomics (nmi_truth differs in the last bits between two identical calls); each call is within
    # float_bound / h_mean of the exact value and h_mean > 2 nats here, so two calls are within
    # float_bound of each other.  Everything made of integers is equal.
    bound = score_ref.float_bound(case.N)
    for k in sc0:
        if np.asarray(sc0[k]).dtype.kind == "f":
            assert np.abs(np.asarray(sc[k]) - np.asarray(sc0[k])).max() <= bound, k
        else:
            assert np.array_equal(sc[k], sc0[k]), k
    p4 = fcmod.fast_consensus(g, "louvain", n_p=20, seed=3, consensus=0.5, return_stats=True)
    assert len(p4) == 3 and p4[0] == parts and "iterations" in p4[1]
    assert np.array_equal(p4[2]["labels"], cons["labels"])
    labs = np.array([[p[x] for x in nodes.tolist()] for p in parts])
    same(cons, cref.partition(case.N, u, v, 0.5, labels=labs))
    assert cons["partition"] == dict(zip(nodes.tolist(), cons["labels"].tolist()))
    cl = cons["labels"]
    bound = score_ref.float_bound(case.N)
    assert sc["nmi_consensus"].shape == sc["ari_consensus"].shape == (20,)
    for r in range(20):
        exp = score_ref.pair(cl, labs[r])
        assert abs(sc["nmi_consensus"][r] - exp["nmi"]) <= bound / exp["h_mean"], r
        assert abs(sc["ari_consensus"][r] - exp["ari"]) <= 1e-15, r
    assert abs(sc["consensus_modularity"] - score_ref.part(cl, e[:, 0], e[:, 1])["modularity"]) <= 1e-15
    t = score_ref.pair(planted, cl)
    assert abs(sc["consensus_nmi_truth"] - t["nmi"]) <= bound / t["h_mean"]
    assert abs(sc["consensus_ari_truth"] - t["ari"]) <= 1e-15


# ------------------------------------------------------------------ 10. command line
def test_cli_consensus(fcmod, tmp_path):
    path = os.path.join(golden_io.GOLDEN, "karate_club.txt")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "fast_consensus.py"), "-f", path, "-np", "10", "--seed", "5",
                        "--consensus", "0.5"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == ["consensus_t0.2_d0.02_np10", "memberships_t0.2_d0.02_np10",
                                            "out_partitions_t0.2_d0.02_np10"]
    g = fcmod.IdGraph.from_edgelist_file(path)
    with fcmod.Engine(seed=5) as eng:
        eng.load_graph(g.n, g.u, g.v)
        eng.run(0, 10, 0.2, 0.02)
        exp = eng.consensus_partition(0.5)["labels"]
    by_node = dict(zip(g.labels.tolist(), exp.tolist()))
    d = tmp_path / "consensus_t0.2_d0.02_np10"
    mem = [tuple(map(int, ln.split("\t"))) for ln in (d / "membership").read_text().splitlines()]
    assert mem == sorted((k + 1, c + 1) for k, c in by_node.items())
    lines = [list(map(int, ln.split())) for ln in (d / "partition").read_text().splitlines()]
    assert len(lines) == int(exp.max()) + 1
    for c, members in enumerate(lines):
        assert members and all(by_node[x] == c for x in members)
    assert sorted(x for members in lines for x in members) == sorted(by_node)
