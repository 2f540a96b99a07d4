"""fc_item_affinity on the device against tests/median_ref.py on the LFR-1k golden graph.
Everything is an integer: every comparison is np.array_equal."""
import ctypes
import gc

import numpy as np
import pytest

from tests import coassoc_ref as car
from tests import consensus_ref as cr
from tests import golden_io
from tests import median_ref as mr
from tests.test_gpu_cluster_consensus import crafted

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 7                                    # an engine seed whose node map is not the identity
INFO = ("k", "queried_clusters", "slow_lookups", "n_r")
PHASES = ["queries", "count", "fallback"]


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


@pytest.fixture(scope="module")
def lfr():
    return golden_io.load("lfr1k_louvain_np20")


def engine(fcmod, case, labels=None, seed=SEED):
    e = case.edges_file
    eng = fcmod.Engine(seed=seed)
    eng.load_graph(case.N, e[:, 0], e[:, 1])
    if labels is not None:
        eng.set_labels(labels)
    return eng


@pytest.fixture
def rand_eng(fcmod, lfr):
    """an engine on the LFR-1k graph for the tests that install their own labelings (closed after each:
    test_reuse_and_memory counts the bytes every live engine holds)"""
    with engine(fcmod, lfr) as eng:
        assert not np.array_equal(eng.node_map(), np.arange(lfr.N))
        yield eng


def check(eng, labs, part, nodes, clusters, slow=None):
    """Engine.item_affinity against the reference on the labelings `labs`"""
    labs, part = np.asarray(labs), np.asarray(part)
    nodes, clusters = np.asarray(nodes, np.int64), np.asarray(clusters, np.int64)
    got = eng.item_affinity(part, nodes, clusters)
    assert sorted(got) == sorted(INFO + ("aff",))
    assert got["aff"].dtype == np.int64 and got["aff"].shape == (len(nodes),)
    assert np.array_equal(got["aff"], mr.affinity(labs, part, nodes, clusters))
    assert got["k"] == len(np.unique(part)) and got["n_r"] == len(labs)
    assert got["queried_clusters"] == len(np.intersect1d(clusters, part))
    if slow is not None:
        assert got["slow_lookups"] == slow
    return got


def all_against(part, rng, per_cluster=3):
    """queries from members and from non-members into every cluster of part"""
    nodes, clusters = [], []
    for c in np.unique(part):
        inside, outside = np.flatnonzero(part == c), np.flatnonzero(part != c)
        for pool in (inside, outside):
            if len(pool):
                pick = rng.choice(pool, min(per_cluster, len(pool)), replace=False)
                nodes += pick.tolist()
                clusters += [c] * len(pick)
    order = rng.permutation(len(nodes))
    return np.array(nodes)[order], np.array(clusters)[order]


def slow_of(part, clusters, d, lcap=16384):
    """the (query, replica) pairs of the fallback for crafted(): every lane of a cluster past the cap,
    the lanes with more than 8 labels (d > 8) of a cluster of 9 or more"""
    size = np.bincount(part)[clusters]
    return int((np.where(size > lcap, len(d), np.where(size >= 9, (d > 8).sum(), 0))).sum())


# ------------------------------------------------------------------ 1. golden labelings
@pytest.mark.parametrize("batch", [0, -1])
@pytest.mark.parametrize("name", ["lfr1k_louvain_np20", "lfr1k_mu03_lpm_np20", "karate_louvain_np50"])
def test_golden_labelings(fcmod, name, batch):
    case = golden_io.load(name)
    labs = case.cd_batches[batch]
    n = case.N
    u, v = cr.canonical_edges(case.edges_file[:, 0], case.edges_file[:, 1])
    rng = np.random.default_rng(3)
    with engine(fcmod, case, labs) as eng:
        assert name.startswith("karate") or not np.array_equal(eng.node_map(), np.arange(n))
        for part in (cr.partition(n, u, v, 0.5, labels=labs)["labels"], labs[0]):
            part = np.asarray(part)
            unused = np.setdiff1d(np.arange(n), part)
            top = eng.vote(part)["top"]
            everyone = np.arange(n)
            nodes = np.tile(everyone, 4)
            clusters = np.r_[part, top, rng.choice(np.unique(part), n), rng.choice(unused, n)]
            got = check(eng, labs, part, nodes, clusters)
            assert np.array_equal(got["aff"][:n], eng.cluster_consensus(part)["item_pairs"])
            assert not got["aff"][3 * n:].any() and got["aff"][:n].min() >= len(labs)


# ------------------------------------------------------------------ 2. replica counts
@pytest.mark.parametrize("n_r", [1, 3, 63, 64, 65, 130])
def test_replica_counts(rand_eng, lfr, n_r):
    rng = np.random.default_rng(n_r)
    labs = rng.integers(0, 3, (n_r, lfr.N))
    rand_eng.set_labels(labs)
    part = rng.integers(0, 40, lfr.N)
    nodes, clusters = all_against(part, rng, 5)
    check(rand_eng, labs, part, nodes, clusters, slow=0)


# ------------------------------------------------------------------ 3. the register list's edge
def test_register_list_edge(rand_eng, lfr):
    rng = np.random.default_rng(2)
    part, labs, d, sizes = crafted(lfr.N, 70, (1, 8, 9, 12))
    rand_eng.set_labels(labs)
    nodes, clusters = all_against(part, rng)
    slow = slow_of(part, clusters, d)
    assert slow == (d > 8).sum() * (np.bincount(part)[clusters] >= 9).sum() > 0
    check(rand_eng, labs, part, nodes, clusters, slow=slow)
    part, labs, d, sizes = crafted(lfr.N, 70, (1, 8, 5, 8), seed=1)
    rand_eng.set_labels(labs)
    nodes, clusters = all_against(part, rng)
    check(rand_eng, labs, part, nodes, clusters, slow=0)


# ------------------------------------------------------------------ 4. the fallback switches
@pytest.mark.parametrize("env", [{"FC_SCORE_LCAP": "64"}, {"FC_SCORE_SLOW": "1"}, {"FC_SCORE_CHUNK": "1"},
                                 {"FC_SCORE_LCAP": "64", "FC_SCORE_CHUNK": "1"}])
def test_fallback_switches(fcmod, lfr, monkeypatch, env):
    part, labs, d, sizes = crafted(lfr.N, 12, (1, 8, 9, 12), seed=2)
    nodes, clusters = all_against(part, np.random.default_rng(4), 4)
    with engine(fcmod, lfr, labs) as eng:
        base = check(eng, labs, part, nodes, clusters, slow=slow_of(part, clusters, d))
        assert base["slow_lookups"] > 0
    for k, val in env.items():
        monkeypatch.setenv(k, val)      # read when the engine is created
    if "FC_SCORE_SLOW" in env:
        slow = len(d) * len(nodes)
    else:
        slow = slow_of(part, clusters, d, int(env.get("FC_SCORE_LCAP", 16384)))
    if env == {"FC_SCORE_CHUNK": "1"}:
        assert slow == base["slow_lookups"]                          # the same lanes, in more than one chunk
        assert (d > 8).sum() * sizes[sizes >= 9].sum() > lfr.N       # more keys than one chunk's window
    else:
        assert slow > base["slow_lookups"]                           # the 65- and 257-clusters whole
    with engine(fcmod, lfr, labs) as eng:
        got = check(eng, labs, part, nodes, clusters, slow=slow)
    assert np.array_equal(got["aff"], base["aff"])


# ------------------------------------------------------------------ 5. query-segment shapes
def raw(eng, part, nodes, clusters, guard=3, npairs=None):
    """fc_item_affinity into a caller buffer with guard elements: (rc, out, info)"""
    npairs = len(nodes) if npairs is None else npairs
    out = torch.full((max(npairs, 0) + guard,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    info = (ctypes.c_int64 * 4)(*([-7] * 4))
    arr = [None if a is None else np.ascontiguousarray(a, dtype=np.int32) for a in (part, nodes, clusters)]
    lab, nd, cl = (None if a is None else a.ctypes.data for a in arr)
    rc = eng._L.fc_item_affinity(eng._ctx, lab, npairs, nd, cl, out.data_ptr(), ctypes.addressof(info))
    return rc, out.cpu().numpy(), list(info)


def test_query_segment_shapes(rand_eng, lfr):
    n = lfr.N
    rng = np.random.default_rng(9)
    labs = np.stack([rng.permutation(n) % 7 for _ in range(5)])
    rand_eng.set_labels(labs)
    # per-cluster query counts: the groups of four and the 64-query batches; cluster 9 gets none
    counts = (0, 1, 3, 4, 5, 63, 64, 65, 257)
    part = rng.integers(0, 10, n)
    clusters = np.repeat(np.arange(len(counts)), counts)
    nodes = rng.integers(0, n, len(clusters))
    order = rng.permutation(len(clusters))
    got = check(rand_eng, labs, part, nodes[order], clusters[order], slow=0)
    assert got["queried_clusters"] == 8 and got["k"] == 10
    # duplicated pairs, one node against every cluster
    check(rand_eng, labs, part, np.r_[nodes[:9], nodes[:9], nodes[:9]], np.r_[clusters[-9:], clusters[-9:], clusters[-9:]])
    got = check(rand_eng, labs, part, np.full(10, 321), np.arange(10), slow=0)
    assert got["aff"].sum() == sum((lab == lab[321]).sum() for lab in labs)
    # K = 1 (seven labels per lane: the list holds them), K = n
    got = check(rand_eng, labs, np.full(n, 3), np.arange(n), np.full(n, 3), slow=0)
    assert got["k"] == 1 and got["queried_clusters"] == 1
    perm = rng.permutation(n)
    got = check(rand_eng, labs, perm, np.r_[np.arange(n), np.arange(n)], np.r_[perm, np.roll(perm, 1)], slow=0)
    assert got["k"] == n and np.array_equal(got["aff"][:n], np.full(n, 5))
    # sparse ids; ids that do not occur give 0; the guard elements stay
    sparse = np.array([5, 900, 17])[rng.integers(0, 3, n)]
    qn, qc = rng.integers(0, n, 200), np.array([5, 17, 900, 6, 0, 999])[rng.integers(0, 6, 200)]
    got = check(rand_eng, labs, sparse, qn, qc)
    assert got["queried_clusters"] == 3 and not got["aff"][~np.isin(qc, [5, 17, 900])].any()
    rc, out, info = raw(rand_eng, sparse, qn, qc)
    assert rc == 0 and np.array_equal(out[:200], got["aff"]) and np.array_equal(out[200:], [-7] * 3)
    assert info[:3] == [got[f] for f in INFO[:3]] and info[3] == 5       # n_r in the low half, pad 0
    # npairs = 0 launches nothing and writes nothing
    rc, out, info = raw(rand_eng, sparse, np.zeros(0), np.zeros(0))
    assert rc == 0 and np.array_equal(out, [-7] * 3) and info[:3] == [3, 0, 0]
    got = rand_eng.item_affinity(sparse, [], [])
    assert got["aff"].shape == (0,) and got["k"] == 3 and got["queried_clusters"] == 0
    with pytest.raises(ValueError):
        rand_eng.item_affinity(sparse, [1, 2], [5])


# ------------------------------------------------------------------ 6. read-only
def test_read_only(fcmod, lfr):
    labs = lfr.cd_batches[0]
    ref = lfr.cd_batches[-1][3]
    rng = np.random.default_rng(4)
    sample = rng.choice(lfr.N, 50, replace=False)
    with engine(fcmod, lfr, labs) as eng:
        eng.set_reference(ref)
        pairs = np.stack([np.full(20, -1), np.arange(20)], 1)
        before = (eng.get_labels(20), eng.score_pairs(pairs), eng.coassociation(sample).cpu().numpy())
        for part in (lfr.cd_batches[-1][0], labs[5]):
            nodes, clusters = all_against(part, rng)
            check(eng, labs, part, nodes, clusters)
        after = (eng.get_labels(20), eng.score_pairs(pairs), eng.coassociation(sample).cpu().numpy())
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2])
        assert before[1].tobytes() == after[1].tobytes()
        assert np.array_equal(before[2], car.matrix(labs, sample))


# ------------------------------------------------------------------ 7. reuse and memory
def test_reuse_and_memory(fcmod, lfr):
    labs = lfr.cd_batches[0]
    part = lfr.cd_batches[-1][2]
    nodes, clusters = all_against(part, np.random.default_rng(5))
    with engine(fcmod, lfr, labs) as eng:
        fresh = eng.item_affinity(part, nodes, clusters)
    with engine(fcmod, lfr) as eng:
        eng.run(0, 20, 0.2, 0.02)
        eng.score_partitions()
        own = eng.get_labels(20)[3]
        eng.cluster_consensus(eng.consensus_partition()["labels"])
        eng.vote(own)
        eng.item_affinity(own, np.arange(lfr.N), own)
        eng.reset_graph()
        eng.set_labels(labs)
        used = eng.item_affinity(part, nodes, clusters)
        assert fcmod.device_bytes() > 0
    for f in INFO + ("aff",):
        assert np.array_equal(used[f], fresh[f]), f
    gc.collect()
    assert fcmod.device_bytes() == 0


# ------------------------------------------------------------------ 8. errors
def test_errors(fcmod, lfr):
    n = lfr.N
    labs = lfr.cd_batches[0]
    part = labs[0]
    nodes, clusters = np.arange(40), part[np.arange(40) + 7]

    def untouched(res):
        return np.all(res[1] == -7) and res[2] == [-7] * 4

    def message(eng):
        return eng._L.fc_last_error().decode()

    with engine(fcmod, lfr) as eng:
        res = raw(eng, part, nodes, clusters)                               # no labelings
        assert res[0] == -4 and untouched(res)
        eng.set_labels(labs)
        for what, at in (("part", 123), ("nodes", 17), ("clusters", 31)):
            args = {"part": part.copy(), "nodes": nodes.copy(), "clusters": clusters.copy()}
            for bad in (n, -1):
                args[what][at] = bad
                res = raw(eng, args["part"], args["nodes"], args["clusters"])
                assert res[0] == -1 and untouched(res) and "index %d" % at in message(eng), (what, bad)
        bad = part.copy()
        bad[123] = n
        with pytest.raises(fcmod.FastConsensusError) as ei:
            eng.item_affinity(bad, nodes, clusters)
        assert ei.value.code == -1 and "index 123" in str(ei.value)
        for args in ((None, nodes, clusters), (part, None, clusters), (part, nodes, None)):   # NULL pointers
            res = raw(eng, *args, npairs=40)
            assert res[0] == -1 and untouched(res)
        info = (ctypes.c_int64 * 4)(*([-7] * 4))
        lab = np.ascontiguousarray(part, dtype=np.int32)
        nd, cl = (np.ascontiguousarray(a, dtype=np.int32) for a in (nodes, clusters))
        rc = eng._L.fc_item_affinity(eng._ctx, lab.ctypes.data, 40, nd.ctypes.data, cl.ctypes.data, None,
                                     ctypes.addressof(info))               # NULL output
        assert rc == -1 and list(info) == [-7] * 4
        res = raw(eng, part, nodes, clusters, npairs=-1)
        assert res[0] == -1 and untouched(res)
        rc = eng._L.fc_item_affinity(eng._ctx, lab.ctypes.data, 2 ** 31, nd.ctypes.data, cl.ctypes.data, None,
                                     ctypes.addressof(info))               # too many queries: before any is read
        assert rc == -5 and list(info) == [-7] * 4
        assert eng._L.fc_item_affinity_timing(eng._ctx, None) == -1
        check(eng, labs, part, nodes, clusters)                             # and the engine still works
        eng.set_labels(np.zeros((2049, n), np.int32))                       # more than 2048 local replicas
        res = raw(eng, part, nodes, clusters)
        assert res[0] == -5 and untouched(res)
    with fcmod.Engine(seed=SEED) as eng:                                    # no graph
        res = raw(eng, part, nodes, clusters)
        assert res[0] == -4 and untouched(res)


# ------------------------------------------------------------------ 9. timing
def test_timing(rand_eng, lfr):
    part, labs, d, sizes = crafted(lfr.N, 12, (1, 8, 9, 12))
    rand_eng.set_labels(labs)
    nodes, clusters = all_against(part, np.random.default_rng(6))
    assert rand_eng.item_affinity(part, nodes, clusters)["slow_lookups"] > 0
    rand_eng.set_timing(True)
    try:
        rand_eng.item_affinity(part, nodes, clusters)
        t = rand_eng.item_affinity_timing()
        assert list(t) == PHASES and all(x > 0.0 for x in t.values())
    finally:
        rand_eng.collect_timing()
        rand_eng.set_timing(False)
    rand_eng.item_affinity(part, nodes, clusters)
    assert rand_eng.item_affinity_timing() == dict.fromkeys(PHASES, 0.0)
