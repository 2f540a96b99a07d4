"""fc_community_quality on the device against tests/quality_ref.py, and the entry points that run
it.  Every compared value is an integer and is compared exactly."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import golden_io
from tests import quality_ref as qr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 7                                    # an engine seed whose node map is not the identity
SENTINEL = -77


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


@pytest.fixture(scope="module")
def lfr():
    return golden_io.load("lfr1k_louvain_np20")


@pytest.fixture(scope="module")
def lfr_edges(lfr):
    e = lfr.edges_file
    return e[:, 0].astype(np.int64), e[:, 1].astype(np.int64)


def engine(fcmod, n, u, v, labels=None, seed=SEED):
    eng = fcmod.Engine(seed=seed)
    eng.load_graph(n, u, v)
    assert n < 3 or not np.array_equal(eng.node_map(), np.arange(n))
    if labels is not None:
        eng.set_labels(labels)
    return eng


@pytest.fixture(scope="module")
def lfr_eng(fcmod, lfr, lfr_edges):
    """one engine on the LFR-1k graph with the last CD batch as its labelings"""
    with engine(fcmod, lfr.N, *lfr_edges, labels=lfr.cd_batches[-1]) as eng:
        yield eng


def same(got, ref, nodes=True, split=True):
    """the dict of Engine.community_quality against the dict of quality_ref.quality"""
    for f in qr.FIELDS:
        assert got[f].dtype == np.int64 and np.array_equal(got[f], ref[f]), f
    for f in qr.INFO:
        assert got[f] == ref[f], f
    if nodes:
        assert got["node_in"].dtype == np.int64 and np.array_equal(got["node_in"], ref["node_in"])
        assert got["node_out"].dtype == np.int64 and np.array_equal(got["node_out"], ref["node_out"])
    if split:
        assert got["split"].dtype == np.int32 and np.array_equal(got["split"], ref["split"])


def raw(fcmod, eng, labels, graph=0, want=("out", "node_in", "node_out", "split", "info"), device=False):
    """The C call itself: the outputs named in `want` prefilled with a sentinel, the others NULL.
    Returns (return code, {name: array})."""
    from fastconsensus_amd import _lib
    n = len(labels)
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    bufs = {"out": np.full(max(n, 1), SENTINEL, _lib.COMMUNITY_RECORD),
            "node_in": np.full(n, SENTINEL, np.int64), "node_out": np.full(n, SENTINEL, np.int64),
            "split": np.full(n, SENTINEL, np.int32), "info": np.full(8, SENTINEL, np.int64)}
    if device:
        for k in ("node_in", "node_out", "split"):
            bufs[k] = torch.as_tensor(bufs[k]).cuda()
        torch.cuda.synchronize()
    args = [_lib.ptr(bufs[k]) if k in want else None for k in ("out", "node_in", "node_out", "split", "info")]
    rc = eng._L.fc_community_quality(eng._ctx, graph, _lib.ptr(lab), *args)
    if device:
        for k in ("node_in", "node_out", "split"):
            bufs[k] = bufs[k].cpu().numpy()
    return rc, bufs


def untouched(bufs):
    return all(np.all(b == SENTINEL) if b.dtype.names is None else all(np.all(b[f] == SENTINEL) for f in b.dtype.names)
               for b in bufs.values())


# ------------------------------------------------------------------ LFR-1k, input graph
def sparse_ids(lab, n):
    """dense ranks r -> r * 7 % n (injective: 7 and n are coprime), the last cluster to id n - 1"""
    r = np.unique(lab, return_inverse=True)[1].ravel()
    k = int(r.max()) + 1
    ids = (np.arange(k) * 7) % n
    assert math.gcd(7, n) == 1 and len(set(ids.tolist())) == k and n - 1 not in ids
    ids[k - 1] = n - 1
    return ids[r]


def lfr_partitions(fcmod, lfr, eng):
    from fastconsensus_amd.core import best_consensus
    rep = lfr.cd_batches[-1][3]
    return {"replica": rep, "best": best_consensus(eng)["labels"], "sparse": sparse_ids(rep, lfr.N),
            "one": np.zeros(lfr.N, np.int32), "singletons": np.arange(lfr.N, dtype=np.int32)}


@pytest.mark.parametrize("which", ["replica", "best", "sparse", "one", "singletons"])
def test_lfr_input_graph(fcmod, lfr, lfr_edges, lfr_eng, which):
    P = lfr_partitions(fcmod, lfr, lfr_eng)[which]
    ref = qr.quality(lfr.N, *lfr_edges, None, P)
    got = lfr_eng.community_quality(P)
    same(got, ref)
    if which == "sparse":
        assert got["ids"][-1] == lfr.N - 1 and got["k"] < lfr.N // 7
    if which == "one":
        assert got["k"] == 1 and got["cut"].tolist() == [0] and math.isnan(got["conductance"][0])
    if which == "singletons":
        assert got["k"] == got["singletons"] == got["parts"] == lfr.N and np.all(got["in_weight"] == 0)
        assert np.all(np.isnan(got["density"]))
    if which == "replica":
        sc = {k: x[3] for k, x in lfr_eng.score_partitions("input").items()}       # the replica P is
        assert int(got["in_weight"].sum()) == got["in_weight_total"] == int(sc["in_weight"])
        assert sum(int(x) ** 2 for x in got["volume"]) == int(sc["tot_sq"])
        # Summation order only.  Each of the k shares is formed with at most 4 roundings of values
        # below 1 (two quotients, a square, a difference) and their sum adds at most k - 1 more of
        # partial sums below 2; the scorer rounds the exact rational once: 8 k ulps of 1.0 in all.
        assert abs(float(got["modularity_share"].sum()) - float(sc["modularity"])) <= 8 * got["k"] * 2.0 ** -53
        assert np.array_equal(got["mixing"], fcmod.mixing(ref["node_in"], ref["node_out"]), equal_nan=True)
        assert np.array_equal(got["conductance"], fcmod.conductance(ref["cut"], ref["volume"], ref["total_degree"]),
                              equal_nan=True)
        assert np.array_equal(got["density"], fcmod.density(ref["in_edges"], ref["size"]), equal_nan=True)


def test_moved_node_disconnects_its_new_community(fcmod, lfr, lfr_edges, lfr_eng):
    """What a one-node move of vote_refine / median_refine can do: a node reassigned to a community
    it has no neighbour in.  The reference decides what must happen; the device must agree."""
    u, v = lfr_edges
    P = np.array(lfr.cd_batches[-1][0], np.int32)
    before = qr.quality(lfr.N, u, v, None, P)
    whole = before["ids"][(before["components"] == 1) & (before["size"] >= 3)]
    x = 0
    nbr_labels = set(P[np.concatenate([v[u == x], u[v == x]])].tolist())
    target = next(int(c) for c in whole.tolist() if c not in nbr_labels and c != P[x])
    moved = P.copy()
    moved[x] = target
    ref = qr.quality(lfr.N, u, v, None, moved)
    at = int(np.searchsorted(ref["ids"], target))
    assert ref["components"][at] == 2 and ref["min_in_degree"][at] == 0          # the reference, on the CPU
    assert ref["largest_component"][at] == ref["size"][at] - 1
    got = lfr_eng.community_quality(moved)
    same(got, ref)
    assert got["components"][at] == 2 and got["split"][x] != got["split"][np.flatnonzero(P == target)[0]]


# ------------------------------------------------------------------ working graph
@pytest.mark.parametrize("algo,tau", [(0, 0.2), (1, 0.8)])
def test_working_graph(fcmod, lfr, lfr_edges, algo, tau):
    with engine(fcmod, lfr.N, *lfr_edges) as eng:
        eng.set_option("max_iters", 1)                       # the loop stops on a weighted working graph
        labels, _ = eng.run(algo, 20, tau, 0.02)
        u, v, w, _ = eng.get_graph()
        assert (w > 1).any() if algo == 0 else (w == 0).any()
        for P in (labels[0], labels[7], np.zeros(lfr.N, np.int32)):
            ref = qr.quality(lfr.N, u, v, w, P)
            same(eng.community_quality(P, graph="working"), ref)
            same(eng.community_quality(P), qr.quality(lfr.N, *lfr_edges, None, P))     # the input graph is still G
        one = qr.quality(lfr.N, u, v, w, np.zeros(lfr.N, np.int32))
        assert one["in_edges"][0] == len(u) and one["in_weight"][0] == int(w.sum())    # weight-0 edges are counted


# ------------------------------------------------------------------ crafted graph
def crafted():
    """184 nodes: a path of 129 (cluster 0); a star with 40 leaves (1); two hubs of exactly 16 and 17
    neighbours on the path, not adjacent to each other (2); five nodes hung on star leaves, pairwise
    non-adjacent (3); two disjoint triangles under one id (4); an isolated node (5)."""
    e = [(i, i + 1) for i in range(128)]
    e += [(129, 130 + i) for i in range(40)]
    e += [(170, i) for i in range(16)] + [(171, 20 + i) for i in range(17)]
    e += [(172 + i, 130 + i) for i in range(5)]
    e += [(177, 178), (178, 179), (177, 179), (180, 181), (181, 182), (180, 182)]
    n = 184
    P = np.zeros(n, np.int32)
    P[129:170], P[170:172], P[172:177], P[177:183], P[183] = 1, 2, 3, 4, 5
    e = np.array(e, np.int64)
    return n, e[:, 0], e[:, 1], P


def test_crafted_graph(fcmod):
    n, u, v, P = crafted()
    ref = qr.quality(n, u, v, None, P)
    assert ref["components"].tolist() == [1, 1, 2, 5, 2, 1] and ref["largest_component"].tolist() == [129, 41, 1, 1, 3, 1]
    assert ref["min_in_degree"].tolist() == [1, 1, 0, 0, 2, 0] and ref["in_edges"].tolist() == [128, 40, 0, 0, 6, 0]
    deg = np.bincount(np.concatenate([u, v]), minlength=n)
    assert (deg[170], deg[171], deg[129], deg[183]) == (16, 17, 40, 0)
    with engine(fcmod, n, u, v) as eng:                     # a context with no labelings
        got = eng.community_quality(P)
        same(got, ref)
        assert math.isnan(got["mixing"][183]) and not np.isnan(got["mixing"][:183]).any()
        assert got["disconnected"] == 3 and got["parts"] == 12
        sp = fcmod.split_disconnected(eng, P)
        assert np.array_equal(sp, ref["split"])
        again = eng.community_quality(sp)
        assert again["disconnected"] == 0 and np.all(again["components"] == 1)
        assert np.array_equal(again["split"], sp) and np.array_equal(fcmod.split_disconnected(eng, sp), sp)
        # ids that are not dense, and the path cut into clusters that straddle the wave boundaries
        Q = (P * 31 + 5).astype(np.int32)
        Q[60:70], Q[120:129] = 183, 0
        same(eng.community_quality(Q), qr.quality(n, u, v, None, Q))


def test_graph_without_edges(fcmod):
    n = 70
    none = np.zeros(0, np.int32)
    P = (np.arange(n) % 3).astype(np.int32)
    ref = qr.quality(n, none, none, None, P)
    with engine(fcmod, n, none, none, seed=3) as eng:
        for graph in ("input", "working"):
            got = eng.community_quality(P, graph=graph)
            same(got, ref)
            assert np.array_equal(got["components"], got["size"]) and got["parts"] == n
            for f in ("volume", "in_weight", "in_edges", "min_in_degree", "cut", "node_in", "node_out"):
                assert not got[f].any(), f
            assert got["total_degree"] == 0 and np.all(got["largest_component"] == 1)


# ------------------------------------------------------------------ outputs and errors
def test_null_outputs_and_device_buffers(fcmod, lfr, lfr_edges, lfr_eng):
    P = np.array(lfr.cd_batches[-1][5], np.int32)
    names = ("out", "node_in", "node_out", "split", "info")
    rc, full = raw(fcmod, lfr_eng, P)
    assert rc == 0
    ref = qr.quality(lfr.N, *lfr_edges, None, P)
    k = int(full["info"][0])
    assert k == ref["k"] and np.array_equal(full["out"]["components"][:k], ref["components"])
    assert np.all(full["out"]["id"][k:] == SENTINEL)                     # only k records are written
    assert full["info"].tolist() == [ref[f] for f in qr.INFO]
    assert np.array_equal(full["split"], ref["split"]) and np.array_equal(full["node_in"], ref["node_in"])
    for drop in names:
        want = tuple(x for x in names if x != drop)
        rc, b = raw(fcmod, lfr_eng, P, want=want)
        assert rc == 0
        for x in want:
            assert np.array_equal(b[x], full[x]), (drop, x)
    for only in names:                                                   # each output alone: the other phases are skipped
        rc, b = raw(fcmod, lfr_eng, P, want=(only,))
        assert rc == 0 and np.array_equal(b[only], full[only]), only
    rc, _ = raw(fcmod, lfr_eng, P, want=())
    assert rc == 0
    rc, dev = raw(fcmod, lfr_eng, P, device=True)
    assert rc == 0
    for x in names:
        assert np.array_equal(dev[x], full[x]), x


def test_errors_write_nothing(fcmod, lfr, lfr_eng):
    from fastconsensus_amd import _lib
    P = np.array(lfr.cd_batches[-1][5], np.int32)
    for bad, at in ((-1, 17), (lfr.N, lfr.N - 1)):
        Q = P.copy()
        Q[at] = bad
        rc, b = raw(fcmod, lfr_eng, Q)
        msg = _lib.load().fc_last_error().decode()
        assert rc == -1 and "index %d" % at in msg and str(bad) in msg and untouched(b)
        with pytest.raises(fcmod.FastConsensusError) as ei:
            lfr_eng.community_quality(Q)
        assert ei.value.code == -1 and "index %d" % at in str(ei.value)
    rc, b = raw(fcmod, lfr_eng, P, graph=7)
    assert rc == -1 and untouched(b)
    with pytest.raises(ValueError):
        lfr_eng.community_quality(P, graph="other")
    with pytest.raises(ValueError):
        lfr_eng.community_quality(P[:-1])
    rc = lfr_eng._L.fc_community_quality(lfr_eng._ctx, 0, None, None, None, None, None, None)
    assert rc == -1 and "null labels" in _lib.load().fc_last_error().decode()
    with fcmod.Engine(seed=SEED) as eng:                                 # no graph
        rc, b = raw(fcmod, eng, P)
        assert rc == -4 and untouched(b)
        ms = (ctypes.c_double * 4)(*([-1.0] * 4))
        assert eng._L.fc_community_quality_timing(eng._ctx, ms) == 0 and list(ms) == [0.0] * 4


def test_timing(fcmod, lfr, lfr_edges):
    P = np.array(lfr.cd_batches[-1][5], np.int32)
    with engine(fcmod, lfr.N, *lfr_edges) as eng:
        eng.set_timing(True)
        got = eng.community_quality(P)
        ms = eng.community_quality_timing()
        assert list(ms) == ["labels", "rows", "fold", "components"] and all(x > 0 for x in ms.values())
        assert eng.collect_timing()["consensus_ms"] >= sum(ms.values()) * 0.99
        eng.set_timing(False)
        same(eng.community_quality(P, nodes=False, split=False), qr.quality(lfr.N, *lfr_edges, None, P), False, False)
        assert eng.community_quality_timing() == dict.fromkeys(ms, 0.0)
    # a phase nothing asks for does not run: the split alone never allocates what the rows and the
    # fold write into (the memory the context holds is the observable)
    with engine(fcmod, lfr.N, *lfr_edges) as eng:
        sp = fcmod.split_disconnected(eng, P)
        assert np.array_equal(sp, got["split"])
        held = fcmod.device_bytes()
        assert np.array_equal(fcmod.split_disconnected(eng, P), sp) and fcmod.device_bytes() == held
        eng.community_quality(P)
        assert fcmod.device_bytes() > held


# ------------------------------------------------------------------ read-only
def test_read_only_and_memory(fcmod, lfr, lfr_edges):
    base = fcmod.device_bytes()
    P = np.array(lfr.cd_batches[-1][5], np.int32)
    res = []
    for call in (True, False):
        eng = engine(fcmod, lfr.N, *lfr_edges)
        eng.set_option("max_iters", 2)
        first, _ = eng.run(0, 20, 0.2, 0.02)
        first = first.copy()
        lv = eng.consensus_levels()
        if call:
            a = eng.community_quality(P, graph="working")
            b = eng.community_quality(P, graph="working")
            for f in qr.FIELDS + ("node_in", "node_out", "split"):
                assert np.array_equal(a[f], b[f]), f
            u, v, w, _ = eng.get_graph()
            same(a, qr.quality(lfr.N, u, v, w, P))
            eng.community_quality(first[0])
        held = fcmod.device_bytes()
        cut = eng.consensus_cut(int(lv["best_level"]))
        res.append((first, eng.get_labels(20), cut, eng.get_graph(), eng.run(0, 20, 0.2, 0.02)[0].copy()))
        assert held > base
        eng.close()
        assert fcmod.device_bytes() == base
    (f1, l1, c1, g1, r1), (f2, l2, c2, g2, r2) = res
    assert np.array_equal(f1, f2) and np.array_equal(l1, l2) and np.array_equal(r1, r2)
    assert np.array_equal(c1[0], c2[0]) and c1[1] == c2[1]
    assert all(np.array_equal(x, y) for x, y in zip(g1, g2))


# ------------------------------------------------------------------ entry points
def test_fast_consensus_flag(fcmod, lfr, lfr_edges):
    e = lfr.edges_file
    G = fcmod.IdGraph(np.arange(lfr.N), e[:, 0], e[:, 1])
    parts, cons = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus="best", quality=True)
    same(cons["quality"], qr.quality(lfr.N, *lfr_edges, None, cons["labels"]))
    parts2, cons2 = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus="best")
    assert parts2 == parts and sorted(set(cons) - set(cons2)) == ["quality"]
    for k in cons2:
        if isinstance(cons2[k], np.ndarray) and cons2[k].dtype.kind in "iuf":
            assert np.array_equal(cons2[k], cons[k], equal_nan=cons2[k].dtype.kind == "f"), k
    parts3, cons3 = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus="best", vote=True, median=True,
                                         quality=True)
    assert parts3 == parts
    for key, of in (("quality", "labels"), ("voted_quality", "voted"), ("median_quality", "median")):
        same(cons3[key], qr.quality(lfr.N, *lfr_edges, None, cons3[of]))
    with pytest.raises(ValueError):
        fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, quality=True)


def test_run_sharded_flag(fcmod, lfr, lfr_edges):
    """the sharded driver on one rank: the consensus dict gains the quality of its partition"""
    from fastconsensus_amd.distributed import run_sharded
    with engine(fcmod, lfr.N, *lfr_edges) as eng:
        labels, st, cons = run_sharded(eng, 0, 20, 0.2, 0.02, consensus="best", quality=True)
        same(cons["quality"], qr.quality(lfr.N, *lfr_edges, None, cons["labels"]))
        assert "voted_quality" not in cons and "median_quality" not in cons
        labels2, st2, cons2 = run_sharded(eng, 0, 20, 0.2, 0.02, consensus="best")
        assert np.array_equal(labels, labels2) and sorted(set(cons) - set(cons2)) == ["quality"]
        with pytest.raises(ValueError):
            run_sharded(eng, 0, 20, 0.2, 0.02, quality=True)


def test_cli_flag(fcmod, tmp_path, monkeypatch, capsys):
    from fastconsensus_amd import cli
    graph = os.path.join(golden_io.GOLDEN, "karate_club.txt")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as ei:
        cli.main(["-f", graph, "-np", "20", "--seed", "5", "--quality"])
    assert "--consensus" in str(ei.value.code) and not os.listdir(str(tmp_path))
    suffix = "t0.2_d0.02_np20"
    d = tmp_path / ("consensus_" + suffix)
    base = ["-f", graph, "-np", "20", "--seed", "5", "--consensus", "0.5", "--vote", "--median"]
    cli.main(base)
    old = sorted(os.listdir(str(d)))
    plain = {f: (d / f).read_bytes() for f in old}
    runs = {f: (tmp_path / ("memberships_" + suffix) / f).read_bytes() for f in os.listdir(str(tmp_path / ("memberships_" + suffix)))}
    cli.main(base + ["--quality"])
    assert capsys.readouterr().out == ""
    new = ["median_quality.tsv", "quality.tsv", "split_membership", "voted_quality.tsv"]
    assert sorted(os.listdir(str(d))) == sorted(old + new)
    assert all((d / f).read_bytes() == plain[f] for f in old)                    # the old files, byte for byte
    assert all((tmp_path / ("memberships_" + suffix) / f).read_bytes() == b for f, b in runs.items())
    g = fcmod.IdGraph.from_edgelist_file(graph)
    names = [str(x + 1) for x in g.labels.tolist()]                       # the engine's node order

    def column(path, col=1):
        rows = {line.split("\t")[0]: line.split("\t")[col] for line in path.read_text().splitlines()}
        assert sorted(rows) == sorted(names)
        return np.array([int(rows[a]) - 1 for a in names])

    def table(path, ref):
        rows = [line.split("\t") for line in path.read_text().splitlines()]
        ints = np.array([[int(r[i]) for i in (0, 1, 2, 3, 4, 7, 8)] for r in rows], np.int64)
        want = np.stack([ref["ids"] + 1] + [ref[f] for f in ("size", "in_weight", "cut", "volume", "components",
                                                              "largest_component")], 1)
        assert np.array_equal(ints, want)
        flo = np.array([[float(r[5]), float(r[6])] for r in rows])
        assert np.array_equal(flo[:, 0], fcmod.conductance(ref["cut"], ref["volume"], ref["total_degree"]), equal_nan=True)
        assert np.array_equal(flo[:, 1], fcmod.density(ref["in_edges"], ref["size"]), equal_nan=True)

    u, v = g.u.astype(np.int64), g.v.astype(np.int64)
    ref = qr.quality(g.n, u, v, None, column(d / "membership"))
    table(d / "quality.tsv", ref)
    assert np.array_equal(column(d / "split_membership"), ref["split"])
    assert [l.split("\t")[0] for l in (d / "split_membership").read_text().splitlines()] == \
        [l.split("\t")[0] for l in (d / "membership").read_text().splitlines()]
    table(d / "median_quality.tsv", qr.quality(g.n, u, v, None, column(d / "median_membership")))
    # vote.tsv: node label, community+1, voted community+1, ... in node order
    voted = np.array([int(l.split("\t")[2]) - 1 for l in (d / "vote.tsv").read_text().splitlines()])
    table(d / "voted_quality.tsv", qr.quality(g.n, u, v, None, voted))
