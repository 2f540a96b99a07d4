"""Cluster-wise Jaccard best match on the device (fc_cluster_match) against tests/match_ref.py.
Everything is an integer: every comparison is np.array_equal, and the derived float arrays (the same
integers through the same float64 operations) compare with ==.  The launch clamps, several chunks at
the default FC_SCORE_CHUNK and cross products past 2^32 are in tests/test_gpu_match_mid.py."""
import ctypes
import os

import numpy as np
import pytest

from tests import consensus_ref as cr
from tests import golden_io
from tests import match_ref as mr
from tests.test_gpu_cluster_consensus import PLANTED, SEED, crafted, engine, expected_slow

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INFO = ("k", "max_size", "singletons", "perfect", "inter_total", "slow_members", "n_r")
DERIVED = ("jaccard", "f1", "stability", "recovered", "dissolved")
RUN_KEYS = ["match_csize", "match_dissolved", "match_inter", "match_recovered", "match_stability"]


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
def rand_eng(fcmod, lfr):
    """one engine on the LFR-1k graph for the tests that install their own labelings"""
    with engine(fcmod, lfr) as eng:
        assert not np.array_equal(eng.node_map(), np.arange(lfr.N))
        yield eng


def planted_of(case, name):
    planted = np.load(os.path.join(golden_io.GOLDEN, PLANTED[name]))
    return planted[case.z["nodes"]] if "nodes" in case.z and len(planted) != case.N else planted


def check(eng, labs, part, slow=None, other=False):
    """Engine.cluster_match(part) against the reference on the labelings `labs`; other: `labs` is
    one labeling, handed in as `other`"""
    labs = np.atleast_2d(np.asarray(labs))
    ids, size, inter, csize = mr.match(labs, part)
    got = eng.cluster_match(part, other=labs[0]) if other else eng.cluster_match(part)
    assert sorted(got) == sorted(INFO + DERIVED + ("ids", "size", "inter", "csize"))
    assert got["ids"].dtype == np.int32 and np.array_equal(got["ids"], ids)
    assert got["size"].dtype == np.int64 and np.array_equal(got["size"], size)
    for f, exp in (("inter", inter), ("csize", csize)):
        assert got[f].dtype == np.int32 and got[f].shape == exp.shape and np.array_equal(got[f], exp), f
    assert got["k"] == len(ids) and got["max_size"] == size.max() and got["singletons"] == (size == 1).sum()
    assert got["n_r"] == len(labs) and got["inter_total"] == inter.astype(np.int64).sum()
    assert got["perfect"] == ((inter == size[None, :]) & (csize == size[None, :])).sum()
    assert np.all(inter >= 1) and np.all(inter <= np.minimum(size[None, :], csize))
    for f, exp in mr.summary(inter, size, csize).items():
        assert got[f].dtype == exp.dtype and got[f].shape == exp.shape and np.all(got[f] == exp), f
    if slow is not None:
        assert got["slow_members"] == slow
    return got


# ------------------------------------------------------------------ 1. golden labelings
@pytest.mark.parametrize("batch", [0, -1])
@pytest.mark.parametrize("name", ["lfr1k_louvain_np20", "lfr1k_mu03_lpm_np20", "karate_louvain_np50"])
def test_golden_labelings(fcmod, name, batch):
    case = golden_io.load(name)
    labs = case.cd_batches[batch]
    u, v = cr.canonical_edges(case.edges_file[:, 0], case.edges_file[:, 1])
    parts = [cr.partition(case.N, u, v, 0.5, labels=labs)["labels"]]
    if name in PLANTED:
        parts.append(planted_of(case, name))
    with engine(fcmod, case, labs) as eng:
        for part in parts:
            assert len(part) == case.N
            check(eng, labs, part)
        # a replica against the labelings that contain it: its own row is a perfect match throughout
        got = check(eng, labs, labs[0])
        assert np.array_equal(got["inter"][0], got["size"]) and np.array_equal(got["csize"][0], got["size"])
        assert got["perfect"] >= got["k"] and np.all(got["jaccard"][0] == 1.0) and np.all(got["recovered"] >= 1)


# ------------------------------------------------------------------ 2. replica counts
@pytest.mark.parametrize("n_r", [1, 3, 63, 64, 65, 130])
def test_replica_counts(rand_eng, lfr, n_r):
    rng = np.random.default_rng(n_r)
    labs = rng.integers(0, 3, (n_r, lfr.N))
    rand_eng.set_labels(labs)
    check(rand_eng, labs, rng.integers(0, 40, lfr.N), slow=0)


# ------------------------------------------------------------------ 3. the register list's edge
def test_register_list_edge(rand_eng, lfr):
    part, labs, d, sizes = crafted(lfr.N, 70, (1, 8, 9, 12))
    rand_eng.set_labels(labs)
    slow = expected_slow(d, sizes)
    assert slow == (d > 8).sum() * sizes[sizes >= 9].sum() > 0
    check(rand_eng, labs, part, slow=slow)
    part, labs, d, sizes = crafted(lfr.N, 70, (1, 8, 5, 8), seed=1)
    rand_eng.set_labels(labs)
    check(rand_eng, labs, part, slow=0)


# ------------------------------------------------------------------ 4. the length cap and the fallback
@pytest.mark.parametrize("env", [{"FC_SCORE_LCAP": "64"}, {"FC_SCORE_SLOW": "1"}, {"FC_SCORE_CHUNK": "1"},
                                 {"FC_SCORE_LCAP": "64", "FC_SCORE_CHUNK": "1"}])
def test_length_cap_and_fallback(fcmod, lfr, monkeypatch, env):
    part, labs, d, sizes = crafted(lfr.N, 12, (1, 8, 9, 12), seed=2)
    with engine(fcmod, lfr, labs) as eng:
        base = check(eng, labs, part, slow=expected_slow(d, sizes))
    for k, val in env.items():
        monkeypatch.setenv(k, val)      # read when the engine is created
    if "FC_SCORE_SLOW" in env:
        slow = len(d) * lfr.N
    else:
        slow = expected_slow(d, sizes, int(env.get("FC_SCORE_LCAP", 16384)))
    if env == {"FC_SCORE_CHUNK": "1"}:
        assert slow == base["slow_members"] > lfr.N                # more keys than one chunk's window
    else:
        assert slow > base["slow_members"]                         # the 65- and 257-clusters whole
    if "FC_SCORE_CHUNK" in env:
        assert slow > 2 * lfr.N                                    # several chunks: the groups of one cluster are spread over them
    with engine(fcmod, lfr, labs) as eng:
        got = check(eng, labs, part, slow=slow)
    for f in ("ids", "size", "inter", "csize"):
        assert np.array_equal(got[f], base[f]), f


# ------------------------------------------------------------------ 5. the exact tie
@pytest.mark.parametrize("slow", [False, True])
@pytest.mark.parametrize("a_low", [True, False])
def test_exact_tie(fcmod, lfr, monkeypatch, a_low, slow):
    part, lab = mr.exact_tie(lfr.N, a_low)
    if slow:
        monkeypatch.setenv("FC_SCORE_SLOW", "1")
    with engine(fcmod, lfr, lab[None, :]) as eng:
        got = check(eng, lab, part, slow=lfr.N if slow else 0)
        assert (got["size"][0], got["inter"][0, 0], got["csize"][0, 0]) == (4, 2, 6)
        assert np.array_equal(check(eng, lab, part, other=True)["inter"], got["inter"])


# ------------------------------------------------------------------ 6. the near-tie float32 cannot see
@pytest.mark.parametrize("slow", [False, True])
def test_near_tie(fcmod, monkeypatch, slow):
    n = 16000
    part, lab = mr.near_tie(n)
    if slow:
        monkeypatch.setenv("FC_SCORE_SLOW", "1")
    with fcmod.Engine(seed=SEED) as eng:
        eng.load_graph(n, np.arange(n, dtype=np.int32), ((np.arange(n) + 1) % n).astype(np.int32))     # a ring
        eng.set_labels(lab[None, :])
        got = check(eng, lab, part, slow=n if slow else 0)           # 8001 <= FC_SCORE_LCAP: the register path decides
        assert (got["size"][0], got["inter"][0, 0], got["csize"][0, 0]) == (8001, 4000, 7998)


# ------------------------------------------------------------------ 7. shapes
def test_shapes(rand_eng, lfr):
    n = lfr.N
    rng = np.random.default_rng(9)
    labs = np.stack([rng.permutation(n) % (12 if r < 3 else 4) for r in range(5)])
    rand_eng.set_labels(labs)
    got = check(rand_eng, labs, np.full(n, 3), slow=3 * n)          # K = 1: the rows of twelve labels overflow
    assert got["k"] == 1 and np.array_equal(got["ids"], [3])
    part = rng.permutation(n)
    got = check(rand_eng, labs, part, slow=0)                       # K = n
    node = np.argsort(part)                                         # cluster k is node node[k]
    assert got["k"] == n and np.all(got["inter"] == 1)
    assert np.array_equal(got["csize"], np.stack([np.bincount(row)[row[node]] for row in labs]))
    sparse = np.array([5, 900, 17])[rng.integers(0, 3, n)]
    got = check(rand_eng, labs, sparse)
    assert np.array_equal(got["ids"], [5, 17, 900])
    assert np.array_equal(got["size"], [(sparse == c).sum() for c in (5, 17, 900)])
    # ld > K: the first K entries of each row are written, everything else keeps the sentinel
    di = torch.full((7, 8), -7, dtype=torch.int32, device="cuda:0")
    dc = torch.full((7, 8), -7, dtype=torch.int32, device="cuda:0")
    got2 = rand_eng.cluster_match(sparse, dev_inter=di, dev_csize=dc)
    for dev, f in ((di, "inter"), (dc, "csize")):
        h = dev.cpu().numpy()
        assert np.array_equal(h[:5, :3], got[f]) and np.all(h[:5, 3:] == -7) and np.all(h[5:] == -7), f
        assert np.array_equal(got2[f], got[f])
    # ld < K: FC_EINVAL, the buffers untouched, the cluster count reported
    di.fill_(-7)
    dc.fill_(-7)
    torch.cuda.synchronize()
    info = (ctypes.c_int64 * 7)(*([-7] * 7))
    lab32 = np.ascontiguousarray(sparse, np.int32)
    for bi, bc in ((di, dc), (di, None), (None, dc)):
        rc = rand_eng._L.fc_cluster_match(rand_eng._ctx, lab32.ctypes.data, None, 2, None, None,
                                          bi.data_ptr() if bi is not None else None,
                                          bc.data_ptr() if bc is not None else None, ctypes.addressof(info))
        assert rc == -1 and list(info) == [3] + [-7] * 6
        assert bool((di == -7).all()) and bool((dc == -7).all())
    # both buffers NULL: ld is ignored
    from fastconsensus_amd import _lib
    info = _lib.MatchInfo()
    rc = rand_eng._L.fc_cluster_match(rand_eng._ctx, lab32.ctypes.data, None, 0, None, None, None, None,
                                      ctypes.addressof(info))
    assert rc == 0 and {k: getattr(info, k) for k in INFO} == {k: got[k] for k in INFO}


# ------------------------------------------------------------------ 8. `other`
def test_other(fcmod, lfr):
    planted = planted_of(lfr, "lfr1k_louvain_np20")
    stored = lfr.cd_batches[-1][4]
    with engine(fcmod, lfr) as eng:                                 # no labelings
        assert eng.replica_info()[0] == 0
        a = check(eng, stored, planted, other=True)
        b = check(eng, planted, stored, other=True)
        assert a["n_r"] == b["n_r"] == 1 and a["inter_total"] != b["inter_total"]
        assert eng.replica_info()[0] == 0
        f1 = mr.f1(a["inter"], a["size"], a["csize"])
        assert a["f1"].shape == (1, a["k"]) and np.all(a["f1"] == f1)
    labs = lfr.cd_batches[0]
    with engine(fcmod, lfr, labs) as eng:
        before = eng.get_labels(20)
        check(eng, stored, planted, other=True)
        check(eng, labs, planted)                                   # and the labelings still answer
        assert np.array_equal(eng.get_labels(20), before)


# ------------------------------------------------------------------ 9. read-only
def test_read_only(fcmod, lfr):
    labs = lfr.cd_batches[0]
    ref = lfr.cd_batches[-1][3]
    nodes = np.random.default_rng(4).choice(lfr.N, 50, replace=False)
    with engine(fcmod, lfr, labs) as eng:
        eng.set_reference(ref)
        pairs = np.stack([np.full(20, -1), np.arange(20)], 1)
        before = (eng.get_labels(20), eng.score_pairs(pairs), eng.coassociation(nodes).cpu().numpy())
        check(eng, labs, lfr.cd_batches[-1][0])
        check(eng, labs[5], labs[7], other=True)
        after = (eng.get_labels(20), eng.score_pairs(pairs), eng.coassociation(nodes).cpu().numpy())
        assert before[0].tobytes() == after[0].tobytes() and before[2].tobytes() == after[2].tobytes()
        assert before[1].tobytes() == after[1].tobytes()


# ------------------------------------------------------------------ 10. errors
def test_errors(fcmod, lfr):
    n = lfr.N
    labs = lfr.cd_batches[0]
    di = torch.full((20, n), -7, dtype=torch.int32, device="cuda:0")
    dc = torch.full((20, n), -7, dtype=torch.int32, device="cuda:0")
    ids = np.full(n, -7, np.int32)
    size = np.full(n, -7, np.int64)
    info = (ctypes.c_int64 * 7)(*([-7] * 7))

    def call(eng, labels, other):
        return eng._L.fc_cluster_match(eng._ctx, None if labels is None else labels.ctypes.data,
                                       None if other is None else other.ctypes.data, n, ids.ctypes.data,
                                       size.ctypes.data, di.data_ptr(), dc.data_ptr(), ctypes.addressof(info))

    def untouched():
        return bool((di == -7).all()) and bool((dc == -7).all()) and bool(np.all(ids == -7)) and \
            bool(np.all(size == -7)) and list(info) == [-7] * 7

    lab0 = np.ascontiguousarray(labs[0], np.int32)
    bad = lab0.copy()
    bad[123] = n
    with engine(fcmod, lfr) as eng:
        with pytest.raises(fcmod.FastConsensusError) as ei:        # no labelings and no `other`
            eng.cluster_match(lab0, dev_inter=di, dev_csize=dc)
        assert ei.value.code == -4 and untouched()
        eng.set_labels(labs)
        with pytest.raises(fcmod.FastConsensusError) as ei:        # an id equal to n in labels
            eng.cluster_match(bad, dev_inter=di, dev_csize=dc)
        assert ei.value.code == -1 and "index 123" in str(ei.value) and "labels" in str(ei.value) and untouched()
        with pytest.raises(fcmod.FastConsensusError) as ei:        # an id equal to n in other
            eng.cluster_match(lab0, other=bad, dev_inter=di, dev_csize=dc)
        assert ei.value.code == -1 and "index 123" in str(ei.value) and "other" in str(ei.value) and untouched()
        assert call(eng, bad, None) == -1 and untouched()
        assert call(eng, None, None) == -1 and call(eng, None, lab0) == -1 and untouched()
        check(eng, labs, labs[0])                                  # and the engine still works
    with fcmod.Engine(seed=SEED) as eng:                           # no graph
        assert call(eng, lab0, None) == -4 and call(eng, lab0, lab0) == -4 and untouched()


# ------------------------------------------------------------------ 11. timing
def test_timing(rand_eng, lfr):
    part, labs, d, sizes = crafted(lfr.N, 12, (1, 8, 9, 12))
    names = ["segments", "sizes", "match", "fallback"]
    rand_eng.set_labels(labs)
    rand_eng.set_timing(True)
    try:
        rand_eng.cluster_match(part)
        t = rand_eng.cluster_match_timing()
        assert list(t) == names and all(x > 0.0 for x in t.values())
    finally:
        rand_eng.collect_timing()
        rand_eng.set_timing(False)
    rand_eng.cluster_match(part)
    assert rand_eng.cluster_match_timing() == dict.fromkeys(names, 0.0)


# ------------------------------------------------------------------ 12. entry points
def test_fast_consensus_flag(fcmod, lfr):
    e = lfr.edges_file
    G = fcmod.IdGraph(np.arange(lfr.N), e[:, 0], e[:, 1])
    truth = planted_of(lfr, "lfr1k_louvain_np20") * 2 + 11           # ids the engine never sees
    parts, cons = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus="best", match=True, truth=truth)
    labs = np.array([[p[x] for x in range(lfr.N)] for p in parts])
    with engine(fcmod, lfr, labs) as eng:
        exp = check(eng, labs, cons["labels"])
    for f in ("inter", "csize", "stability", "recovered", "dissolved"):
        assert cons["match_" + f].dtype == exp[f].dtype and np.all(cons["match_" + f] == exp[f]), f
    # truth_match: the roles swapped -- the planted partition's clusters, the consensus labels as the row
    ids, size, inter, csize = mr.match(cons["labels"], truth)
    tm = cons["truth_match"]
    assert sorted(tm) == ["csize", "f1", "ids", "inter", "jaccard", "mean_f1", "size"]
    assert np.array_equal(tm["ids"], ids) and np.array_equal(tm["size"], size)
    assert np.array_equal(tm["inter"], inter[0]) and np.array_equal(tm["csize"], csize[0])
    assert np.all(tm["jaccard"] == mr.jaccard(inter[0], size, csize[0]))
    assert np.all(tm["f1"] == mr.f1(inter[0], size, csize[0])) and tm["mean_f1"] == float(tm["f1"].mean())
    parts2, cons2 = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus="best", truth=truth)
    assert parts2 == parts and sorted(set(cons) - set(cons2)) == RUN_KEYS + ["truth_match"]
    assert not set(cons2) - set(cons)
    for k, v in cons2.items():
        assert type(v) is type(cons[k]), k
        if isinstance(v, np.ndarray):
            assert v.dtype == cons[k].dtype and v.tobytes() == cons[k].tobytes(), k
        else:
            assert v == cons[k], k
    parts3, cons3 = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus="best", match=True)
    assert sorted(set(cons3) - set(cons2)) == RUN_KEYS
    with pytest.raises(ValueError):
        fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, match=True)


def test_cli_flag(fcmod, tmp_path, monkeypatch, capsys):
    from fastconsensus_amd import cli
    graph = os.path.join(golden_io.GOLDEN, "karate_club.txt")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as ei:
        cli.main(["-f", graph, "-np", "20", "--seed", "5", "--match"])
    assert "--consensus" in str(ei.value.code) and not os.listdir(str(tmp_path))
    cli.main(["-f", graph, "-np", "20", "--seed", "5", "--consensus", "0.5", "--match"])
    assert capsys.readouterr().out == ""
    suffix = "t0.2_d0.02_np20"
    d = tmp_path / ("consensus_" + suffix)
    assert sorted(os.listdir(str(d))) == ["cluster_match.tsv", "membership", "partition"]
    # the n_p partitions and the consensus partition as the run wrote them: node+1 <TAB> community+1
    lines = [line.split() for line in (d / "membership").read_text().splitlines()]
    names = [a for a, _ in lines]
    part = np.array([int(b) - 1 for _, b in lines])
    labs = []
    for i in range(20):
        rows = dict(line.split() for line in (tmp_path / ("memberships_" + suffix) / str(i)).read_text().splitlines())
        labs.append([int(rows[a]) for a in names])
    ids, size, inter, csize = mr.match(np.array(labs), part)
    s = mr.summary(inter, size, csize)
    rows = [line.split("\t") for line in (d / "cluster_match.tsv").read_text().splitlines()]
    assert [[int(r[0]), int(r[1]), int(r[3]), int(r[4])] for r in rows] == \
        [list(x) for x in zip((ids + 1).tolist(), size.tolist(), s["recovered"].tolist(), s["dissolved"].tolist())]
    assert [float(r[2]) for r in rows] == s["stability"].tolist()
