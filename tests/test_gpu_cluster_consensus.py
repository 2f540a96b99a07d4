"""Cluster and item consensus on the device (fc_cluster_consensus) against
tests/cluster_consensus_ref.py.  Everything is an integer: every comparison is np.array_equal, and
the two normalised arrays (the same integers through the same float64 operations) compare with ==
under their NaN masks."""
import ctypes
import os

import numpy as np
import pytest

from tests import cluster_consensus_ref as ccr
from tests import coassoc_ref as car
from tests import consensus_ref as cr
from tests import golden_io

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 7                                    # an engine seed whose node map is not the identity
INFO = ("k", "max_size", "singletons", "pairs_total", "slow_members", "n_r")
PLANTED = {"lfr1k_louvain_np20": "lfr1k_mu04_planted.npy", "lfr1k_mu03_lpm_np20": "lfr1k_mu03_synth_planted.npy"}


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


@pytest.fixture(scope="module")
def rand_eng(fcmod, lfr):
    """one engine on the LFR-1k graph for the tests that install their own labelings"""
    with engine(fcmod, lfr) as eng:
        assert not np.array_equal(eng.node_map(), np.arange(lfr.N))
        yield eng


def check(eng, labs, part, slow=None):
    """Engine.cluster_consensus(part) against the reference on the labelings `labs`"""
    labs = np.asarray(labs)
    n_r, n = labs.shape
    ids, size, pairs, item = ccr.sums(labs, part)
    got = eng.cluster_consensus(part)
    assert sorted(got) == sorted(INFO + ("ids", "size", "cluster_pairs", "item_pairs", "cluster_consensus",
                                         "item_consensus"))
    assert got["ids"].dtype == np.int32 and np.array_equal(got["ids"], ids)
    assert got["size"].dtype == np.int64 and np.array_equal(got["size"], size)
    assert got["cluster_pairs"].dtype == np.int64 and np.array_equal(got["cluster_pairs"], pairs)
    assert got["item_pairs"].dtype == np.int64 and np.array_equal(got["item_pairs"], item)
    assert got["k"] == len(ids) and got["max_size"] == size.max() and got["singletons"] == (size == 1).sum()
    assert got["pairs_total"] == pairs.sum() == item.sum() and got["n_r"] == n_r
    assert np.all(n_r * size <= pairs) and np.all(pairs <= n_r * size * size)
    own = size[np.searchsorted(ids, part)]
    assert ccr.same_floats(got["cluster_consensus"], ccr.cluster_consensus(pairs, size, n_r))
    assert ccr.same_floats(got["item_consensus"], ccr.item_consensus(item, own, n_r))
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
    parts = [cr.partition(case.N, u, v, 0.5, labels=labs)["labels"], labs[0]]
    if name in PLANTED:
        planted = np.load(os.path.join(golden_io.GOLDEN, PLANTED[name]))
        parts.append(planted[case.z["nodes"]] if "nodes" in case.z and len(planted) != case.N else planted)
    with engine(fcmod, case, labs) as eng:
        for part in parts:
            assert len(part) == case.N
            check(eng, labs, part)
        # a replica against itself and the others: its own lane holds one label per cluster
        assert check(eng, labs, labs[0])["cluster_pairs"].min() >= labs.shape[0]


# ------------------------------------------------------------------ 2. replica counts
@pytest.mark.parametrize("n_r", [1, 3, 63, 64, 65, 130])
def test_replica_counts(rand_eng, lfr, n_r):
    rng = np.random.default_rng(n_r)
    labs = rng.integers(0, 3, (n_r, lfr.N))
    rand_eng.set_labels(labs)
    check(rand_eng, labs, rng.integers(0, 40, lfr.N), slow=0)


# ------------------------------------------------------------------ 3. the register list's edge
SIZES = (1, 2, 8, 9, 63, 64, 65, 257)


def crafted(n, n_r, ds, seed=0):
    """Clusters of the SIZES and a remainder, scattered over the nodes; replica r labels the j-th
    member of every cluster j mod d_r (d_r cycling through ds): min(size, d_r) labels per cluster and
    lane, the same label values in every cluster.  Returns part, labs, d [n_r], the cluster sizes."""
    sizes = np.array(SIZES + (n - sum(SIZES),))
    order = np.random.default_rng(seed).permutation(n)
    part = np.empty(n, np.int64)
    j = np.empty(n, np.int64)
    at = 0
    for c, s in enumerate(sizes):
        part[order[at:at + s]] = c
        j[order[at:at + s]] = np.arange(s)
        at += s
    d = np.array([ds[r % len(ds)] for r in range(n_r)])
    return part, j[None, :] % d[:, None], d, sizes


def expected_slow(d, sizes, lcap=16384):
    over = sizes > lcap
    return int(len(d) * sizes[over].sum() + (d > 8).sum() * sizes[(sizes >= 9) & ~over].sum())


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
    with engine(fcmod, lfr, labs) as eng:
        got = check(eng, labs, part, slow=slow)
    for f in ("ids", "size", "cluster_pairs", "item_pairs"):
        assert np.array_equal(got[f], base[f]), f


# ------------------------------------------------------------------ 5. shapes
def test_shapes(rand_eng, lfr):
    n = lfr.N
    rng = np.random.default_rng(9)
    labs = np.stack([rng.permutation(n) % 12 for _ in range(5)])
    rand_eng.set_labels(labs)
    got = check(rand_eng, labs, np.full(n, 3), slow=5 * n)          # K = 1: twelve labels per lane
    assert got["k"] == 1 and np.array_equal(got["ids"], [3])
    got = check(rand_eng, labs, rng.permutation(n), slow=0)         # K = N
    assert got["k"] == n and np.array_equal(got["cluster_pairs"], np.full(n, 5))
    assert np.array_equal(got["item_pairs"], np.full(n, 5)) and np.all(np.isnan(got["cluster_consensus"]))
    sparse = np.array([5, 900, 17])[rng.integers(0, 3, n)]
    got = check(rand_eng, labs, sparse)
    assert np.array_equal(got["ids"], [5, 17, 900])
    assert np.array_equal(got["size"], [(sparse == c).sum() for c in (5, 17, 900)])
    # the caller's buffers: pairs of the K clusters, then zeros; items in node order
    dc = torch.full((n + 3,), -7, dtype=torch.int64, device="cuda:0")
    di = torch.full((n + 3,), -7, dtype=torch.int64, device="cuda:0")
    got2 = rand_eng.cluster_consensus(sparse, dev_cluster=dc, dev_item=di)
    dc, di = dc.cpu().numpy(), di.cpu().numpy()
    assert np.array_equal(dc[:3], got["cluster_pairs"]) and not dc[3:n].any() and np.array_equal(dc[n:], [-7] * 3)
    assert np.array_equal(di[:n], got["item_pairs"]) and np.array_equal(di[n:], [-7] * 3)
    assert np.array_equal(got2["item_pairs"], got["item_pairs"])


# ------------------------------------------------------------------ 6. read-only
def test_read_only(fcmod, lfr):
    labs = lfr.cd_batches[0]
    ref = lfr.cd_batches[-1][3]
    nodes = np.random.default_rng(4).choice(lfr.N, 50, replace=False)
    with engine(fcmod, lfr, labs) as eng:
        eng.set_reference(ref)
        pairs = np.stack([np.full(20, -1), np.arange(20)], 1)
        before = (eng.get_labels(20), eng.score_pairs(pairs), eng.coassociation(nodes).cpu().numpy())
        check(eng, labs, lfr.cd_batches[-1][0])
        check(eng, labs, labs[5])
        after = (eng.get_labels(20), eng.score_pairs(pairs), eng.coassociation(nodes).cpu().numpy())
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2])
        assert before[1].tobytes() == after[1].tobytes()
        assert np.array_equal(before[2], car.matrix(labs, nodes))


# ------------------------------------------------------------------ 7. item consensus with other clusters
def test_item_consensus(fcmod, lfr):
    labs = lfr.cd_batches[0]
    part = labs[2]
    rng = np.random.default_rng(6)
    nodes = rng.choice(lfr.N, 40, replace=False)
    own = part[nodes[:3]]
    clusters = np.r_[own, rng.choice(np.setdiff1d(np.unique(part), own), 6 - len(own), replace=False)]
    with engine(fcmod, lfr, labs) as eng:
        got = eng.item_consensus(nodes, part, clusters)
        assert got.dtype == np.int64 and got.shape == (40, 6)
        assert np.array_equal(got, ccr.item_sums(car.matrix, labs, nodes, part, clusters))
        every = np.unique(part)
        full = eng.item_consensus(nodes, part, every)
        cc = eng.cluster_consensus(part)
        assert np.array_equal(full[np.arange(40), np.searchsorted(every, part[nodes])], cc["item_pairs"][nodes])


# ------------------------------------------------------------------ 8. errors
def test_errors(fcmod, lfr):
    n = lfr.N
    labs = lfr.cd_batches[0]
    dc = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    di = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")

    def untouched():
        return bool((dc == -7).all()) and bool((di == -7).all())

    with engine(fcmod, lfr) as eng:
        with pytest.raises(fcmod.FastConsensusError) as ei:        # no labelings
            eng.cluster_consensus(labs[0], dev_cluster=dc, dev_item=di)
        assert ei.value.code == -4 and untouched()
        eng.set_labels(labs)
        bad = labs[0].copy()
        bad[123] = n
        with pytest.raises(fcmod.FastConsensusError) as ei:        # an id equal to n
            eng.cluster_consensus(bad, dev_cluster=dc, dev_item=di)
        assert ei.value.code == -1 and "index 123" in str(ei.value) and untouched()
        ids = np.full(n, -7, np.int32)
        size = np.full(n, -7, np.int64)
        info = (ctypes.c_int64 * 6)(*([-7] * 6))
        rc = eng._L.fc_cluster_consensus(eng._ctx, None, ids.ctypes.data, size.ctypes.data, dc.data_ptr(),
                                         di.data_ptr(), ctypes.addressof(info))
        assert rc == -1 and untouched() and np.all(ids == -7) and np.all(size == -7) and list(info) == [-7] * 6
        check(eng, labs, labs[0])                                  # and the engine still works
    with fcmod.Engine(seed=SEED) as eng:                           # no graph
        rc = eng._L.fc_cluster_consensus(eng._ctx, labs[0].ctypes.data, None, None, None, None, None)
        assert rc == -4


# ------------------------------------------------------------------ 9. timing
def test_timing(rand_eng, lfr):
    part, labs, d, sizes = crafted(lfr.N, 12, (1, 8, 9, 12))
    rand_eng.set_labels(labs)
    rand_eng.set_timing(True)
    try:
        rand_eng.cluster_consensus(part)
        t = rand_eng.cluster_consensus_timing()
        assert list(t) == ["segments", "count", "fallback"] and all(x >= 0.0 for x in t.values())
        assert t["segments"] > 0.0 and t["count"] > 0.0 and t["fallback"] > 0.0
    finally:
        rand_eng.collect_timing()
        rand_eng.set_timing(False)
    rand_eng.cluster_consensus(part)
    assert rand_eng.cluster_consensus_timing() == {"segments": 0.0, "count": 0.0, "fallback": 0.0}


# ------------------------------------------------------------------ 10. entry points
def test_fast_consensus_flag(fcmod, lfr):
    e = lfr.edges_file
    G = fcmod.IdGraph(np.arange(lfr.N), e[:, 0], e[:, 1])
    parts, cons = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus="best", cluster_consensus=True)
    labs = np.array([[p[x] for x in range(lfr.N)] for p in parts])
    with engine(fcmod, lfr, labs) as eng:
        exp = check(eng, labs, cons["labels"])
    for f in ("cluster_pairs", "item_pairs"):
        assert cons[f].dtype == np.int64 and np.array_equal(cons[f], exp[f])
    for f in ("cluster_consensus", "item_consensus"):
        assert ccr.same_floats(cons[f], exp[f])
    parts2, cons2 = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus="best")
    assert parts2 == parts and np.array_equal(cons2["labels"], cons["labels"])
    assert sorted(set(cons) - set(cons2)) == ["cluster_consensus", "cluster_pairs", "item_consensus", "item_pairs"]
    with pytest.raises(ValueError):
        fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, cluster_consensus=True)


def test_cli_flag(fcmod, tmp_path, monkeypatch, capsys):
    from fastconsensus_amd import cli
    graph = os.path.join(golden_io.GOLDEN, "karate_club.txt")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as ei:
        cli.main(["-f", graph, "-np", "20", "--seed", "5", "--cluster-consensus"])
    assert "--consensus" in str(ei.value.code) and not os.listdir(str(tmp_path))
    cli.main(["-f", graph, "-np", "20", "--seed", "5", "--consensus", "0.5", "--cluster-consensus"])
    assert capsys.readouterr().out == ""
    suffix = "t0.2_d0.02_np20"
    d = tmp_path / ("consensus_" + suffix)
    assert sorted(os.listdir(str(d))) == ["cluster_consensus.tsv", "item_consensus.tsv", "membership", "partition"]
    # the n_p partitions and the consensus partition as the run wrote them: node+1 <TAB> community+1
    names = [a for a, _ in (line.split() for line in (d / "membership").read_text().splitlines())]
    part = np.array([int(b) - 1 for _, b in (line.split() for line in (d / "membership").read_text().splitlines())])
    labs = []
    for i in range(20):
        rows = dict(line.split() for line in (tmp_path / ("memberships_" + suffix) / str(i)).read_text().splitlines())
        labs.append([int(rows[a]) for a in names])
    ids, size, pairs, item = ccr.sums(np.array(labs), part)
    rows = [line.split("\t") for line in (d / "cluster_consensus.tsv").read_text().splitlines()]
    assert [[int(x) for x in r[:3]] for r in rows] == [[c + 1, s, p] for c, s, p in zip(ids.tolist(), size.tolist(), pairs.tolist())]
    assert ccr.same_floats([float(r[3]) for r in rows], ccr.cluster_consensus(pairs, size, 20))
    rows = {r[0]: r[1:] for r in (line.split("\t") for line in (d / "item_consensus.tsv").read_text().splitlines())}
    assert len(rows) == len(names)
    # membership lists node+1, item_consensus.tsv the node label itself
    got = [rows[str(int(a) - 1)] for a in names]
    assert [[int(r[0]), int(r[1])] for r in got] == [[c + 1, x] for c, x in zip(part.tolist(), item.tolist())]
    own = size[np.searchsorted(ids, part)]
    assert ccr.same_floats([float(r[2]) for r in got], ccr.item_consensus(item, own, 20))
