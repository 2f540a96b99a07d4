"""fc_community_graph, fc_cluster_coassoc and core.merge_refine on the device against
tests/merge_ref.py on the golden graphs.  Everything is an integer: every comparison is
np.array_equal or ==."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import consensus_ref as cr
from tests import golden_io
from tests import median_ref as mr
from tests import merge_ref as gr
from tests import quality_ref as qr
from tests.test_gpu_cluster_consensus import crafted
from tests.test_gpu_community_quality import sparse_ids

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 7                                    # an engine seed whose node map is not the identity
SENTINEL = -7
INFO = ("k", "listed_clusters", "walked_members", "slow_lookups", "n_r")
CG_KEYS = ["a", "b", "edges", "npairs", "weight"]


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


@functools.lru_cache(maxsize=None)
def case_of(name):
    case = golden_io.load(name)
    u, v = cr.canonical_edges(case.edges_file[:, 0], case.edges_file[:, 1])
    return case, u, v


@pytest.fixture(scope="module")
def lfr():
    return case_of("lfr1k_louvain_np20")[0]


def engine(fcmod, case, labels=None, seed=SEED):
    e = case.edges_file
    eng = fcmod.Engine(seed=seed)
    eng.load_graph(case.N, e[:, 0], e[:, 1])
    assert case.N < 100 or not np.array_equal(eng.node_map(), np.arange(case.N))
    if labels is not None:
        eng.set_labels(labels)
    return eng


@pytest.fixture
def lfr_eng(fcmod, lfr):
    with engine(fcmod, lfr, lfr.cd_batches[0]) as eng:
        yield eng


@functools.lru_cache(maxsize=None)
def strict_cut(name, batch=0):
    case, u, v = case_of(name)
    return cr.partition(case.N, u, v, 1.0, labels=case.cd_batches[batch])["labels"]


def partitions(name):
    case = case_of(name)[0]
    rep = np.asarray(case.cd_batches[0][0], np.int32)
    return {"replica0": rep, "strict": strict_cut(name), "singletons": np.arange(case.N, dtype=np.int32),
            "one": np.full(case.N, 5, np.int32), "sparse": sparse_ids(strict_cut(name), case.N)}


# ------------------------------------------------------------------ community graph
def same_graph(got, ref):
    assert sorted(got) == CG_KEYS
    assert got["npairs"] == ref["npairs"] and isinstance(got["npairs"], int)
    for f, t in (("a", np.int32), ("b", np.int32), ("weight", np.int64), ("edges", np.int64)):
        assert got[f].dtype == t and np.array_equal(got[f], ref[f]), f


def raw_graph(eng, labels, graph=0, capacity=None, want=("a", "b", "weight", "edges"), device=False, guard=3,
              count=True):
    """The C call itself: the outputs named in `want` prefilled with a sentinel, the others NULL.
    Returns (return code, npairs, {name: array})."""
    from fastconsensus_amd import _lib
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
    cap = eng.graph_info()[1] if capacity is None else capacity
    bufs = {"a": np.full(cap + guard, SENTINEL, np.int32), "b": np.full(cap + guard, SENTINEL, np.int32),
            "weight": np.full(cap + guard, SENTINEL, np.int64), "edges": np.full(cap + guard, SENTINEL, np.int64)}
    if device:
        bufs = {k: torch.as_tensor(b).cuda() for k, b in bufs.items()}
        torch.cuda.synchronize()
    npairs = ctypes.c_int64(SENTINEL)
    args = [_lib.ptr(bufs[k]) if k in want else None for k in ("a", "b", "weight", "edges")]
    rc = eng._L.fc_community_graph(eng._ctx, graph, _lib.ptr(lab), cap, *args, ctypes.byref(npairs) if count else None)
    if device:
        bufs = {k: b.cpu().numpy() for k, b in bufs.items()}
    return rc, npairs.value, bufs


def untouched(bufs):
    return all(np.all(b == SENTINEL) for b in bufs.values())


@pytest.mark.parametrize("which", ["replica0", "strict", "singletons", "one", "sparse"])
@pytest.mark.parametrize("name", ["karate_louvain_np50", "lfr1k_louvain_np20"])
def test_community_graph_input(fcmod, name, which):
    case, u, v = case_of(name)
    P = partitions(name)[which]
    ref = gr.community_graph(case.N, u, v, None, P)
    with engine(fcmod, case) as eng:                      # a graph and nothing else
        got = eng.community_graph(P)
        same_graph(got, ref)
        if which == "singletons":
            assert got["npairs"] == len(u) and np.array_equal(got["a"], u) and (got["edges"] == 1).all()
        if which == "one":
            assert got["npairs"] == 0
        if which == "sparse":
            assert len(np.unique(P)) < int(P.max()) and got["npairs"] > 0
        # the identities with the community quality
        q = eng.community_quality(P)
        cut = np.zeros(case.N, np.int64)
        np.add.at(cut, got["a"], got["weight"])
        np.add.at(cut, got["b"], got["weight"])
        assert np.array_equal(cut[q["ids"]], q["volume"] - 2 * q["in_weight"]) and cut.sum() == 2 * q["cut_weight"]
        assert int(got["weight"].sum()) == q["cut_weight"]
        # the C call: device outputs, a subset of the outputs, the size query, a capacity one short
        k = ref["npairs"]
        for device in (False, True):
            rc, n, bufs = raw_graph(eng, P, device=device)
            assert rc == 0 and n == k
            for f in ("a", "b", "weight", "edges"):
                assert np.array_equal(bufs[f][:k], ref[f]) and np.all(bufs[f][k:] == SENTINEL), f
        rc, n, bufs = raw_graph(eng, P, want=("b", "edges"), capacity=k)
        assert rc == 0 and n == k and np.array_equal(bufs["b"][:k], ref["b"]) and np.array_equal(bufs["edges"][:k], ref["edges"])
        assert untouched({f: bufs[f] for f in ("a", "weight")}) and np.all(bufs["b"][k:] == SENTINEL)
        rc, n, bufs = raw_graph(eng, P, want=(), capacity=0)
        assert rc == 0 and n == k and untouched(bufs)
        if k:
            for device in (False, True):
                rc, n, bufs = raw_graph(eng, P, capacity=k - 1, device=device)
                assert rc == -1 and n == k and untouched(bufs)
                assert str(k) in eng._L.fc_last_error().decode()
        same_graph(eng.community_graph(P), ref)


@pytest.mark.parametrize("algo,tau", [(0, 0.2), (1, 0.8)])
@pytest.mark.parametrize("name", ["karate_louvain_np50", "lfr1k_louvain_np20"])
def test_community_graph_working(fcmod, name, algo, tau):
    case, u0, v0 = case_of(name)
    with engine(fcmod, case) as eng:
        eng.set_option("max_iters", 1)                       # the loop stops on a weighted working graph
        labels, _ = eng.run(algo, 20, tau, 0.02)
        u, v, w, _ = eng.get_graph()
        if name.startswith("lfr"):
            assert (w > 1).any() if algo == 0 else (w == 0).any()
        for P in (labels[0], labels[7], np.arange(case.N, dtype=np.int32), np.zeros(case.N, np.int32)):
            ref = gr.community_graph(case.N, u, v, w, P)
            got = eng.community_graph(P, graph="working")
            same_graph(got, ref)
            q = eng.community_quality(P, graph="working")
            assert int(got["weight"].sum()) == q["cut_weight"]
            same_graph(eng.community_graph(P), gr.community_graph(case.N, u0, v0, None, P))   # the input graph is still G
        single = eng.community_graph(np.arange(case.N), graph="working")
        assert single["npairs"] == len(u) and int(single["weight"].sum()) == int(w.sum())   # weight-0 edges are pairs


def test_community_graph_errors(fcmod, lfr):
    n = lfr.N
    P = np.asarray(lfr.cd_batches[0][0], np.int32)
    with fcmod.Engine(seed=SEED) as eng:                                    # no graph
        rc, k, bufs = raw_graph(eng, P, capacity=10)
        assert rc == -4 and k == SENTINEL and untouched(bufs)
    with engine(fcmod, lfr) as eng:
        for bad in (n, -1):
            lab = P.copy()
            lab[321] = bad
            rc, k, bufs = raw_graph(eng, lab)
            assert rc == -1 and k == SENTINEL and untouched(bufs) and "index 321" in eng._L.fc_last_error().decode()
        rc, k, bufs = raw_graph(eng, None)
        assert rc == -1 and k == SENTINEL and untouched(bufs)
        rc, k, bufs = raw_graph(eng, P, count=False)
        assert rc == -1 and untouched(bufs)
        rc, k, bufs = raw_graph(eng, P, graph=2)
        assert rc == -1 and k == SENTINEL and untouched(bufs)
        with pytest.raises(ValueError):
            eng.community_graph(P, graph="kept")
        assert eng._L.fc_community_graph_timing(eng._ctx, None) == -1
        eng.set_timing(True)
        try:
            eng.community_graph(P)
            t = eng.community_graph_timing()
            assert list(t) == ["labels", "emit", "sort", "pairs"] and all(x > 0.0 for x in t.values())
        finally:
            eng.collect_timing()
            eng.set_timing(False)
        eng.community_graph(P)
        assert eng.community_graph_timing() == dict.fromkeys(["labels", "emit", "sort", "pairs"], 0.0)


# ------------------------------------------------------------------ pair co-association
def flagged_lanes(labs, part, lcap=16384, slow=False):
    """{cluster id: the replicas its list leaves to the fallback}: all of them past the length cap (or
    with FC_SCORE_SLOW), else the replicas that give its members more than 8 labels"""
    C, _ = mr.tables(labs, part)
    size = np.bincount(np.asarray(part, np.int64))
    out = {}
    for c in np.unique(part).tolist():
        out[c] = len(C) if slow or size[c] > lcap else sum(int((t[c] > 0).sum()) > 8 for t in C)
    return out


def expected_info(labs, part, a, b, lcap=16384, slow=False):
    """listed clusters, walked members and slow lookups from the contingency cells: the larger
    cluster of a pair lists (a on equal sizes), the smaller walks"""
    size = np.bincount(np.asarray(part, np.int64), minlength=len(part))
    flagged = flagged_lanes(labs, part, lcap, slow)
    listed, walked, lookups = set(), 0, 0
    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        if size[x] == 0 or size[y] == 0:
            continue
        lst, wlk = (x, y) if size[x] >= size[y] else (y, x)
        listed.add(lst)
        walked += int(size[wlk])
        lookups += int(size[wlk]) * flagged[lst]
    return len(listed), walked, lookups


def check(eng, labs, part, a, b, lcap=16384, slow=False):
    """Engine.cluster_coassoc against the reference on the labelings `labs`"""
    labs, part = np.asarray(labs), np.asarray(part)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    got = eng.cluster_coassoc(part, a, b)
    assert sorted(got) == sorted(INFO + ("x",))
    assert got["x"].dtype == np.int64 and got["x"].shape == (len(a),)
    assert np.array_equal(got["x"], gr.cross(labs, part, a, b))
    assert got["k"] == len(np.unique(part)) and got["n_r"] == len(labs)
    assert (got["listed_clusters"], got["walked_members"], got["slow_lookups"]) == \
        expected_info(labs, part, a, b, lcap, slow)
    return got


def every_pair(part, rng, absent=True):
    """every pair a <= b of the clusters of part, in both orders and with duplicates, shuffled; plus
    pairs with an id that does not occur"""
    ids = np.unique(part)
    a, b = np.triu_indices(len(ids))
    a, b = ids[a], ids[b]
    a, b = np.r_[a, b, a[::3]], np.r_[b, a, b[::3]]
    if absent:
        free = np.setdiff1d(np.arange(len(part)), part)[:2]
        a, b = np.r_[a, free[0], ids[0], free[0]], np.r_[b, ids[-1], free[1], free[0]]
    order = rng.permutation(len(a))
    return a[order], b[order]


def seventy(case):
    """70 labelings: the case's 3 x 20 batches plus the first 10 rows again, ids renamed"""
    labs = np.concatenate([np.concatenate(case.cd_batches[:3]), case.cd_batches[0][:10]])
    assert labs.shape == (70, case.N)
    perm = np.random.default_rng(70).permutation(case.N)
    return perm[labs].astype(np.int32)


def test_pairs_of_replica0(fcmod, lfr, lfr_eng):
    labs = lfr.cd_batches[0]
    part = np.asarray(labs[0])
    assert len(np.unique(part)) == 23
    # register path and fallback in one call: one cluster has lanes with more than 8 labels
    C, _ = mr.tables(labs, part)
    most = np.array([[int((t[c] > 0).sum()) for t in C] for c in np.unique(part)])
    assert ((most > 8).any(1)).sum() == 1 and most.max() == 17
    a, b = every_pair(part, np.random.default_rng(1))
    got = check(lfr_eng, labs, part, a, b)
    assert got["slow_lookups"] > 0 and got["listed_clusters"] == 23
    diag = np.flatnonzero((a == b) & np.isin(a, part))
    cc = lfr_eng.cluster_consensus(part)
    assert np.array_equal(got["x"][diag], cc["cluster_pairs"][np.searchsorted(cc["ids"], a[diag])])
    assert not got["x"][~(np.isin(a, part) & np.isin(b, part))].any()
    # npairs = 0 launches nothing
    none = lfr_eng.cluster_coassoc(part, [], [])
    assert none["x"].shape == (0,) and none["k"] == 23 and none["listed_clusters"] == none["walked_members"] == 0
    with pytest.raises(ValueError):
        lfr_eng.cluster_coassoc(part, [1, 2], [5])


def test_two_banks(fcmod, lfr):
    labs = seventy(lfr)
    rng = np.random.default_rng(2)
    with engine(fcmod, lfr, labs) as eng:
        check(eng, labs, lfr.cd_batches[0][0], *every_pair(lfr.cd_batches[0][0], rng))
        part = strict_cut("lfr1k_louvain_np20")              # 139 clusters: the pairs of its community graph
        g = eng.community_graph(part)
        check(eng, labs, part, np.r_[g["a"], g["b"][:40]], np.r_[g["b"], g["a"][:40]])
        # co-association does not see the renaming: the first 20 rows are batch 0
        eng.set_labels(labs[:20])
        part = lfr.cd_batches[0][0]
        a, b = every_pair(part, rng)
        assert np.array_equal(eng.cluster_coassoc(part, a, b)["x"], gr.cross(lfr.cd_batches[0], part, a, b))


def test_halves_and_one_cluster(fcmod, lfr, lfr_eng):
    labs = lfr.cd_batches[0]
    halves = (np.arange(lfr.N) >= lfr.N // 2).astype(np.int32)
    got = check(lfr_eng, labs, halves, [0, 0, 1, 1], [1, 0, 0, 1])
    assert got["x"][0] == got["x"][2] == 277415 and got["x"][1] == 295382
    assert got["slow_lookups"] == 4 * 500 * 20                              # all through the fallback
    one = np.full(lfr.N, 77, np.int32)
    got = check(lfr_eng, labs, one, [77, 77, 3], [77, 77, 77])
    assert got["x"][0] == sum(int((np.bincount(lab) ** 2).sum()) for lab in labs) and got["x"][2] == 0


@pytest.mark.parametrize("env", [{}, {"FC_SCORE_LCAP": "64"}, {"FC_SCORE_SLOW": "1"}, {"FC_SCORE_CHUNK": "1"},
                                 {"FC_SCORE_LCAP": "64", "FC_SCORE_CHUNK": "1"}],
                         ids=lambda e: "-".join(sorted(e)) or "default")
def test_fallback_switches(fcmod, lfr, monkeypatch, env):
    """the crafted clusters (1, 2, 8, 9, 63, 64, 65, 257 and the rest): a side past the cap against
    a short one in both argument orders, two long sides, the ninth label on a short list"""
    part, labs, d, sizes = crafted(lfr.N, 12, (1, 8, 9, 12), seed=2)
    a, b = every_pair(part, np.random.default_rng(4))
    for k, val in env.items():
        monkeypatch.setenv(k, val)      # read when the engine is created
    lcap, slow = int(env.get("FC_SCORE_LCAP", 16384)), "FC_SCORE_SLOW" in env
    with engine(fcmod, lfr, labs) as eng:
        got = check(eng, labs, part, a, b, lcap, slow)
        assert got["slow_lookups"] > 0
        if slow:
            assert got["slow_lookups"] == got["walked_members"] * len(labs)
        # the 257-cluster (past a cap of 64) against the 9-cluster (short) and against the rest (long)
        big, short, rest = 7, 3, 8
        assert sizes[big] == 257 and sizes[short] == 9 and sizes[rest] > 257
        check(eng, labs, part, [big, short, big, rest], [short, big, rest, big], lcap, slow)
    if env == {"FC_SCORE_CHUNK": "1"}:
        assert (d > 8).sum() * sizes[sizes >= 9].sum() > lfr.N       # more keys than one chunk's window


# ------------------------------------------------------------------ read-only
def test_read_only(fcmod, lfr):
    labs = lfr.cd_batches[0]
    part = strict_cut("lfr1k_louvain_np20")
    res = []
    for use in (False, True):
        with engine(fcmod, lfr, labs) as eng:
            if use:
                g = eng.community_graph(part)
                eng.cluster_coassoc(part, g["a"], g["b"])
                eng.community_graph(labs[3], graph="working")
                fcmod.merge_refine(eng, part)
            res.append((eng.get_labels(20), eng.get_graph(), eng.cd(0, 0, 4, 4, 0), eng.get_labels(4)))
    for x, y in zip(res[0], res[1]):
        if isinstance(x, tuple):
            assert all(np.array_equal(p, q) for p, q in zip(x, y))
        elif x is not None:
            assert np.array_equal(x, y)


# ------------------------------------------------------------------ errors
def raw_pairs(eng, part, a, b, guard=3, npairs=None, out=True):
    """fc_cluster_coassoc into a caller buffer with guard elements: (rc, out, info)"""
    npairs = len(a) if npairs is None else npairs
    buf = torch.full((max(min(npairs, 1 << 20), 0) + guard,), SENTINEL, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    info = (ctypes.c_int64 * 5)(*([SENTINEL] * 5))
    arr = [None if x is None else np.ascontiguousarray(x, dtype=np.int32) for x in (part, a, b)]
    lab, pa, pb = (None if x is None else x.ctypes.data for x in arr)
    rc = eng._L.fc_cluster_coassoc(eng._ctx, lab, npairs, pa, pb, buf.data_ptr() if out else None, ctypes.addressof(info))
    return rc, buf.cpu().numpy(), list(info)


def test_pair_errors(fcmod, lfr):
    n = lfr.N
    labs = lfr.cd_batches[0]
    part = np.asarray(labs[0], np.int32)
    a, b = np.arange(20), np.arange(20)[::-1].copy()

    def clean(res):
        return np.all(res[1] == SENTINEL) and res[2] == [SENTINEL] * 5

    with engine(fcmod, lfr) as eng:
        res = raw_pairs(eng, part, a, b)                                    # no labelings
        assert res[0] == -4 and clean(res)
        eng.set_labels(labs)
        rc, out, info = raw_pairs(eng, part, a, b)
        assert rc == 0 and np.array_equal(out[:20], gr.cross(labs, part, a, b)) and np.all(out[20:] == SENTINEL)
        assert info[0] == 23 and info[4] == 20                              # n_r in the low half, pad 0
        rc, out, info = raw_pairs(eng, part, a[:0], b[:0])
        assert rc == 0 and np.all(out == SENTINEL) and info[:4] == [23, 0, 0, 0]
        for what, at in (("part", 123), ("a", 17), ("b", 3)):
            for bad in (n, -1):
                args = {"part": part.copy(), "a": a.copy(), "b": b.copy()}
                args[what][at] = bad
                res = raw_pairs(eng, args["part"], args["a"], args["b"])
                assert res[0] == -1 and clean(res) and "index %d" % at in eng._L.fc_last_error().decode(), (what, bad)
        for args in ((None, a, b), (part, None, b), (part, a, None)):      # NULL pointers
            res = raw_pairs(eng, *args, npairs=20)
            assert res[0] == -1 and clean(res)
        res = raw_pairs(eng, part, a, b, out=False)
        assert res[0] == -1 and clean(res)
        res = raw_pairs(eng, part, a, b, npairs=-1)
        assert res[0] == -1 and clean(res)
        res = raw_pairs(eng, part, a, b, npairs=2 ** 31)                    # too many pairs: before any is read
        assert res[0] == -5 and clean(res)
        assert eng._L.fc_cluster_coassoc_timing(eng._ctx, None) == -1
        bad = part.copy()
        bad[123] = n
        with pytest.raises(fcmod.FastConsensusError) as ei:
            eng.cluster_coassoc(bad, a, b)
        assert ei.value.code == -1 and "index 123" in str(ei.value)
        eng.set_timing(True)
        try:
            halves = (np.arange(n) >= n // 2).astype(np.int32)
            eng.cluster_coassoc(halves, [0], [1])
            t = eng.cluster_coassoc_timing()
            assert list(t) == ["pairs", "count", "fallback"] and all(x > 0.0 for x in t.values())
        finally:
            eng.collect_timing()
            eng.set_timing(False)
        check(eng, labs, part, a, b)                                        # and the engine still works
        assert eng.cluster_coassoc_timing() == dict.fromkeys(["pairs", "count", "fallback"], 0.0)
        eng.set_labels(np.zeros((2049, n), np.int32))                       # more than 2048 local replicas
        res = raw_pairs(eng, part, a, b)
        assert res[0] == -5 and clean(res)
    with fcmod.Engine(seed=SEED) as eng:                                    # no graph
        res = raw_pairs(eng, part, a, b)
        assert res[0] == -4 and clean(res)


# ------------------------------------------------------------------ merge_refine
REFINE_KEYS = ["accepted_per_round", "converged", "gain_per_round", "k_per_round", "labels", "mean_rand", "objective",
               "pairs_per_round", "proposed_per_round", "rounds"]


def same_refine(got, ref, labs):
    assert sorted(got) == REFINE_KEYS
    assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], ref["labels"])
    for f in ("rounds", "converged", "objective", "pairs_per_round", "proposed_per_round", "accepted_per_round",
              "gain_per_round", "k_per_round"):
        assert got[f] == ref[f], f
    for f in ("objective", "pairs_per_round", "proposed_per_round", "accepted_per_round", "gain_per_round", "k_per_round"):
        assert all(type(x) is int for x in got[f]), f
    assert got["objective"][-1] == mr.objective(labs, got["labels"])
    T, n, R = mr.sum_sq(labs), len(got["labels"]), len(labs)
    assert got["mean_rand"] == (mr.mean_rand(got["objective"][0], T, n, R), mr.mean_rand(got["objective"][-1], T, n, R))


# (case, batch, start) -> k after, F before and after, rounds, first round's pairs / proposed / accepted
TRAJECTORIES = {
    ("lfr1k_louvain_np20", 0, "strict"): (24, 908600, 1039252, 11, (1866, 305, 49)),
    ("lfr1k_louvain_np20", 0, "replica0"): (21, 947652, 969420, 1, (253, 2, 2)),
    ("lfr1k_louvain_np20", 0, "singletons"): (25, 20000, 1039504, 18, (13637, 5531, 444)),
    ("lfr1k_louvain_np20", -1, "singletons"): (31, 20000, 1046200, 15, (13637, 5286, 438)),
    ("karate_louvain_np50", 0, "strict"): (8, 3600, 7848, 5, (45, 19, 6)),
}


@pytest.mark.parametrize("key", sorted(TRAJECTORIES), ids=lambda k: "%s-%d-%s" % k)
def test_merge_refine_trajectory(fcmod, key):
    name, batch, start = key
    case, u, v = case_of(name)
    labs = case.cd_batches[batch]
    part = {"strict": lambda: strict_cut(name, batch), "replica0": lambda: labs[0],
            "singletons": lambda: np.arange(case.N)}[start]()
    k1, f0, f1, rounds, first = TRAJECTORIES[key]
    with engine(fcmod, case, labs) as eng:
        got = fcmod.merge_refine(eng, part)
        same_refine(got, gr.refine(labs, part, case.N, u, v), labs)
        assert got["converged"] and got["rounds"] == rounds and got["k_per_round"][-1] == k1
        assert (got["objective"][0], got["objective"][-1]) == (f0, f1)
        assert (got["pairs_per_round"][0], got["proposed_per_round"][0], got["accepted_per_round"][0]) == first
        again = fcmod.merge_refine(eng, got["labels"])
        assert again["rounds"] == 0 and again["converged"] and again["objective"] == [f1]
        short = fcmod.merge_refine(eng, part, max_rounds=2)
        assert short["rounds"] == min(2, rounds) and short["converged"] == (rounds < 2)
        assert short["objective"] == got["objective"][:short["rounds"] + 1]


def test_merge_refine_fixpoints_and_candidates(fcmod):
    case, u, v = case_of("karate_louvain_np50")
    labs = case.cd_batches[0]
    with engine(fcmod, case, labs) as eng:
        got = fcmod.merge_refine(eng, labs[0])                              # a fixpoint of the rule
        same_refine(got, gr.refine(labs, labs[0], case.N, u, v), labs)
        assert got["rounds"] == 0 and got["converged"] and np.array_equal(got["labels"], labs[0])
        # candidates of the caller's: a pair of lists, or a callable
        part = strict_cut("karate_louvain_np50")
        ids = np.unique(part)
        a, b = np.repeat(ids, len(ids)), np.tile(ids, len(ids))
        wide = fcmod.merge_refine(eng, part, candidates=(a, b), max_rounds=1)
        ref = gr.moves(part, a, b, gr.cross(labs, part, a, b), len(labs))
        assert np.array_equal(wide["labels"], ref["labels"]) and wide["gain_per_round"] == [ref["gain"]]
        assert wide["pairs_per_round"] == [len(a)] and wide["proposed_per_round"] == [ref["proposed"]]
        assert wide["objective"][1] == mr.objective(labs, wide["labels"])
        every = fcmod.merge_refine(eng, part, candidates=(a, b))            # the ids that vanish give 0
        assert every["converged"] and every["objective"][-1] == mr.objective(labs, every["labels"])
        seen = []

        def adjacent(lab):
            seen.append(len(np.unique(lab)))
            g = gr.community_graph(case.N, u, v, None, lab)
            return g["a"], g["b"]

        own = fcmod.merge_refine(eng, part, candidates=adjacent)
        same_refine(own, gr.refine(labs, part, case.N, u, v), labs)
        assert seen == own["k_per_round"]
        none = fcmod.merge_refine(eng, part, candidates=lambda lab: ([], []))
        assert none["rounds"] == 0 and none["converged"] and none["objective"] == [3600]


def test_recovery(fcmod, lfr):
    """ten clusters of a fixpoint split in two: one round puts them back"""
    case, u, v = case_of("lfr1k_louvain_np20")
    labs = case.cd_batches[-1]
    orig = np.asarray(labs[0], np.int32)
    ids, size = np.unique(orig, return_counts=True)
    assert len(ids) == 31
    pick = np.random.default_rng(11).permutation(ids[size >= 6])[:10]
    free = np.setdiff1d(np.arange(case.N), orig)
    part = orig.copy()
    for c, f in zip(pick.tolist(), free.tolist()):
        part[np.flatnonzero(orig == c)[1::2]] = f
    with engine(fcmod, case, labs) as eng:
        assert fcmod.merge_refine(eng, orig)["rounds"] == 0
        got = fcmod.merge_refine(eng, part)
        same_refine(got, gr.refine(labs, part, case.N, u, v), labs)
        assert got["rounds"] == 1 and got["converged"] and got["objective"] == [776240, 1046200]
        assert (got["pairs_per_round"], got["proposed_per_round"], got["accepted_per_round"]) == ([719], [10], [10])
        cells = set(zip(got["labels"].tolist(), orig.tolist()))
        assert len(cells) == 31 == len(np.unique(got["labels"]))            # the original up to names
        assert fcmod.merge_refine(eng, got["labels"])["rounds"] == 0


# ------------------------------------------------------------------ entry points
KEYS = ["merged", "merged_accepted", "merged_k", "merged_mean_rand", "merged_objective", "merged_rounds"]


def same_result(cons, labs, start, case_name="lfr1k_louvain_np20"):
    case, u, v = case_of(case_name)
    ref = gr.refine(labs, start, case.N, u, v)
    assert cons["merged"].dtype == np.int32 and np.array_equal(cons["merged"], ref["labels"])
    assert cons["merged_objective"] == ref["objective"] and cons["merged_rounds"] == ref["rounds"]
    assert cons["merged_accepted"] == ref["accepted_per_round"] and cons["merged_k"] == ref["k_per_round"]
    assert cons["merged_objective"][-1] == mr.objective(labs, cons["merged"])
    T, n, R = mr.sum_sq(labs), case.N, len(labs)
    assert cons["merged_mean_rand"] == (mr.mean_rand(ref["objective"][0], T, n, R), mr.mean_rand(ref["objective"][-1], T, n, R))


def test_fast_consensus_flag(fcmod, lfr):
    e = lfr.edges_file
    G = fcmod.IdGraph(np.arange(lfr.N), e[:, 0], e[:, 1])
    parts, cons = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus=1.0, merge=True)
    labs = np.array([[p[x] for x in range(lfr.N)] for p in parts])
    same_result(cons, labs, cons["labels"])
    parts2, cons2 = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus=1.0)
    assert parts2 == parts and np.array_equal(cons2["labels"], cons["labels"])
    assert sorted(set(cons) - set(cons2)) == KEYS
    assert all(np.array_equal(cons[k], cons2[k]) if isinstance(cons2[k], np.ndarray) else True for k in cons2)
    parts3, cons3 = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus=1.0, vote=True, median=True,
                                         quality=True, merge=True)
    assert parts3 == parts
    same_result(cons3, labs, cons3["median"])                            # from the last refinement made
    parts4, cons4 = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus=1.0, vote=True, median=True,
                                         quality=True)
    assert sorted(set(cons3) - set(cons4)) == sorted(KEYS + ["merged_quality"])
    ref = qr.quality(lfr.N, *cr.canonical_edges(e[:, 0], e[:, 1]), None, cons3["merged"])
    assert all(np.array_equal(cons3["merged_quality"][f], ref[f]) for f in qr.FIELDS)
    parts5, cons5 = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus=1.0, vote=True, merge=True)
    same_result(cons5, labs, cons5["voted"])
    with pytest.raises(ValueError):
        fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, merge=True)


def test_run_sharded_flag(fcmod, lfr):
    """the sharded driver on one rank: the consensus dict gains the merged partition"""
    from fastconsensus_amd.distributed import run_sharded
    with engine(fcmod, lfr) as eng:
        labels, st, cons = run_sharded(eng, 0, 20, 0.2, 0.02, consensus=1.0, merge=True)
        same_result(cons, labels, cons["labels"])
        labels2, st2, cons2 = run_sharded(eng, 0, 20, 0.2, 0.02, consensus=1.0)
        assert np.array_equal(labels2, labels) and sorted(set(cons) - set(cons2)) == KEYS
        with pytest.raises(ValueError):
            run_sharded(eng, 0, 20, 0.2, 0.02, merge=True)


def test_cli_flag(fcmod, tmp_path, monkeypatch, capsys):
    from fastconsensus_amd import cli
    graph = os.path.join(golden_io.GOLDEN, "karate_club.txt")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as ei:
        cli.main(["-f", graph, "-np", "20", "--seed", "5", "--merge"])
    assert "--consensus" in str(ei.value.code) and not os.listdir(str(tmp_path))
    suffix = "t0.2_d0.02_np20"
    d = tmp_path / ("consensus_" + suffix)
    cli.main(["-f", graph, "-np", "20", "--seed", "5", "--consensus", "1.0"])
    assert sorted(os.listdir(str(d))) == ["membership", "partition"]     # no new files without the flag
    plain = (d / "membership").read_text()
    cli.main(["-f", graph, "-np", "20", "--seed", "5", "--consensus", "1.0", "--merge"])
    assert capsys.readouterr().out == ""
    assert sorted(os.listdir(str(d))) == ["membership", "merge.tsv", "merge_membership", "partition"]
    assert (d / "membership").read_text() == plain
    g = fcmod.IdGraph.from_edgelist_file(graph)
    names = [str(x + 1) for x in g.labels.tolist()]

    def column(path):
        rows = dict(line.split() for line in path.read_text().splitlines())
        assert sorted(rows) == sorted(names)
        return [int(rows[a]) - 1 for a in names]

    part = np.array(column(d / "membership"))
    labs = np.array([column(tmp_path / ("memberships_" + suffix) / str(i)) for i in range(20)])
    u, v = cr.canonical_edges(g.u, g.v)
    ref = gr.refine(labs, part, g.n, u, v)
    assert [a for a, _ in (line.split() for line in (d / "merge_membership").read_text().splitlines())] == \
        [a for a, _ in (line.split() for line in plain.splitlines())]
    assert column(d / "merge_membership") == ref["labels"].tolist()
    tsv = [[int(x) for x in line.split("\t")] for line in (d / "merge.tsv").read_text().splitlines()]
    assert [r[0] for r in tsv] == list(range(ref["rounds"] + 1)) and [r[1] for r in tsv] == ref["objective"]
    assert [r[2] for r in tsv] == ref["k_per_round"]
    assert [r[3:] for r in tsv] == [[0, 0, 0]] + [list(x) for x in zip(ref["pairs_per_round"], ref["proposed_per_round"],
                                                                      ref["accepted_per_round"])]
    cli.main(["-f", graph, "-np", "20", "--seed", "5", "--consensus", "1.0", "--merge", "--quality"])
    assert sorted(os.listdir(str(d))) == ["membership", "merge.tsv", "merge_membership", "merged_quality.tsv", "partition",
                                          "quality.tsv", "split_membership"]
