"""Plurality vote on the device (fc_vote_map / fc_vote_count / fc_vote) against tests/vote_ref.py on
the LFR-1k golden graph.  Everything is an integer: every comparison is np.array_equal."""
import ctypes
import gc
import os

import numpy as np
import pytest

from tests import coassoc_ref as car
from tests import consensus_ref as cr
from tests import golden_io
from tests import vote_ref as vr
from tests.test_gpu_cluster_consensus import crafted, expected_slow

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 7                                    # an engine seed whose node map is not the identity
INFO = ("k", "k_voted", "moved", "unanimous", "tied", "mapped_communities", "slow_members", "slow_nodes", "n_total")
ARRAYS = ("top", "top_votes", "own_votes")
PHASES = ["segments", "map", "map_fallback", "count"]


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


def same(got, ref):
    """the dict of Engine.vote against the dict of vote_ref.vote / count_votes"""
    n, nt = len(ref["top"]), ref["n_total"]
    for f, r in (("top", "top"), ("top_votes", "top_votes"), ("own_votes", "own")):
        assert got[f].dtype == np.int32 and got[f].shape == (n,) and np.array_equal(got[f], ref[r]), f
    assert got["own_hist"].dtype == np.int64 and np.array_equal(got["own_hist"], ref["own_hist"])
    for f in ("k", "k_voted", "moved", "unanimous", "tied", "n_total"):
        assert got[f] == ref[f], f
    assert got["confidence"].dtype == np.float64 and np.array_equal(got["confidence"], ref["own"] / np.float64(nt))
    assert got["slow_nodes"] == (ref["distinct"] > 8).sum()


def check(eng, labs, part, slow_members=None):
    """Engine.vote(part) and Engine.vote_map(part) against the reference on the labelings `labs`"""
    labs = np.asarray(labs)
    ref = vr.vote(labs, part)
    got = eng.vote(part)
    assert sorted(got) == sorted(INFO + ARRAYS + ("own_hist", "confidence"))
    same(got, ref)
    assert got["mapped_communities"] == ref["mapped_communities"]
    m = eng.vote_map(part)
    assert sorted(m) == ["k", "mapped", "mapped_communities", "n_total", "slow_members"]
    assert m["mapped"].dtype == torch.int32 and tuple(m["mapped"].shape) == labs.shape
    assert np.array_equal(m["mapped"].cpu().numpy(), ref["mapped"])
    assert (m["k"], m["mapped_communities"], m["n_total"]) == (ref["k"], ref["mapped_communities"], labs.shape[0])
    assert m["slow_members"] == got["slow_members"]
    if slow_members is not None:
        assert got["slow_members"] == slow_members
    return got, ref


# ------------------------------------------------------------------ 1. golden labelings
@pytest.mark.parametrize("batch", [0, -1])
@pytest.mark.parametrize("name", ["lfr1k_louvain_np20", "lfr1k_mu03_lpm_np20", "karate_louvain_np50"])
def test_golden_labelings(fcmod, name, batch):
    case = golden_io.load(name)
    labs = case.cd_batches[batch]
    u, v = cr.canonical_edges(case.edges_file[:, 0], case.edges_file[:, 1])
    with engine(fcmod, case, labs) as eng:
        assert name.startswith("karate") or not np.array_equal(eng.node_map(), np.arange(case.N))
        check(eng, labs, cr.partition(case.N, u, v, 0.5, labels=labs)["labels"])
        got, ref = check(eng, labs, labs[0])
        if name == "lfr1k_louvain_np20" and batch == 0:
            # not vacuous, and on the vote list's last slot without overflowing it
            assert got["moved"] > 0 and got["tied"] > 0 and ref["distinct"].max() <= 8 and got["slow_nodes"] == 0


# ------------------------------------------------------------------ 2. replica counts
@pytest.mark.parametrize("n_r", [1, 3, 63, 64, 65, 130])
def test_replica_counts(fcmod, lfr, n_r):
    rng = np.random.default_rng(n_r)
    labs = rng.integers(0, 3, (n_r, lfr.N))
    with engine(fcmod, lfr, labs) as eng:
        check(eng, labs, rng.integers(0, 40, lfr.N), slow_members=0)


# ------------------------------------------------------------------ 3. the map's register list edge
def test_map_list_edge(fcmod, lfr):
    part, labs, d, sizes = crafted(lfr.N, 70, (1, 8, 9, 12))
    slow = expected_slow(d, sizes)
    assert slow == (d > 8).sum() * sizes[sizes >= 9].sum() > 0
    with engine(fcmod, lfr, labs) as eng:
        check(eng, labs, part, slow_members=slow)
        part, labs, d, sizes = crafted(lfr.N, 70, (1, 8, 5, 8), seed=1)
        eng.set_labels(labs)
        check(eng, labs, part, slow_members=0)


# ------------------------------------------------------------------ 4. the map's fallback switches
@pytest.mark.parametrize("env", [{"FC_SCORE_LCAP": "64"}, {"FC_SCORE_SLOW": "1"}, {"FC_SCORE_CHUNK": "1"},
                                 {"FC_SCORE_LCAP": "64", "FC_SCORE_CHUNK": "1"}])
def test_map_fallback_switches(fcmod, lfr, monkeypatch, env):
    part, labs, d, sizes = crafted(lfr.N, 12, (1, 8, 9, 12), seed=2)
    with engine(fcmod, lfr, labs) as eng:
        base, _ = check(eng, labs, part, slow_members=expected_slow(d, sizes))
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
        got, _ = check(eng, labs, part, slow_members=slow)
    for f in ARRAYS + ("own_hist",):
        assert np.array_equal(got[f], base[f]), f


# ------------------------------------------------------------------ 5. the vote's register list edge
def vote_edge(n, qs, n_r=70, clusters=40):
    """P: `clusters` equal clusters; every replica equals P except for the nodes x_j (one per entry
    of qs), which replica r puts in cluster (j + r) mod q_j: q_j clusters vote for x_j."""
    part = np.arange(n) % clusters
    labs = np.tile(part, (n_r, 1))
    x = np.arange(len(qs)) * 37 + 11
    for j, q in enumerate(qs):
        labs[:, x[j]] = (j + np.arange(n_r)) % q
    return part, labs, x


def test_vote_list_edge(fcmod, lfr):
    qs = (1, 2, 8, 9, 12, 40) * 2
    part, labs, x = vote_edge(lfr.N, qs)
    with engine(fcmod, lfr, labs) as eng:
        got, ref = check(eng, labs, part, slow_members=0)
        assert np.array_equal(ref["distinct"][x], qs)
        assert got["slow_nodes"] == (ref["distinct"] > 8).sum() == 6
        part, labs, x = vote_edge(lfr.N, (1, 2, 8, 7, 3, 8))
        eng.set_labels(labs)
        got, ref = check(eng, labs, part, slow_members=0)
        assert ref["distinct"].max() == 8 and got["slow_nodes"] == 0


# ------------------------------------------------------------------ 6. ties
def test_ties(fcmod, lfr):
    n = lfr.N
    part = np.full(n, 9)
    part[:5], part[5:10] = 7, 3
    labs = np.ones((1, n), np.int64)
    labs[0, :10] = 0                                               # a community split 5 / 5 between 7 and 3
    with engine(fcmod, lfr, labs) as eng:
        check(eng, labs, part)
        assert np.array_equal(eng.vote_map(part)["mapped"].cpu().numpy()[0], [3] * 10 + [9] * (n - 10))
        # four replicas: node 0 splits 2 / 2 between its own 7 and 3 and keeps 7; node 5 (in 3) splits
        # 2 / 2 between 9 and 7 and takes the smaller; everyone else is unanimous
        mapped = np.tile(part, (4, 1))
        mapped[2:, 0] = 3
        mapped[:2, 5], mapped[2:, 5] = 9, 7
        dev = torch.as_tensor(mapped, dtype=torch.int32, device="cuda:0").contiguous()
        got = eng.vote(part, dev_mapped=dev)
        same(got, vr.count_votes(mapped, part))
        assert got["top"][0] == 7 and got["top"][5] == 7 and got["own_votes"][5] == 0 and got["tied"] == 2
        assert got["moved"] == 1 and got["unanimous"] == n - 2
        assert (got["mapped_communities"], got["slow_members"]) == (0, 0)


# ------------------------------------------------------------------ 7. shapes
def raw_vote(eng, part, n, guard=3):
    """fc_vote into caller buffers with guard elements: (rc, top, top_votes, own_votes, hist, info)"""
    bufs = [torch.full((n + guard,), -7, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()
    n_r = eng.replica_info()[0]
    hist = np.full(n_r + 1 + guard, -7, np.int64)
    info = (ctypes.c_int64 * 9)(*([-7] * 9))
    lab = None if part is None else np.ascontiguousarray(part, dtype=np.int32)
    rc = eng._L.fc_vote(eng._ctx, None if lab is None else lab.ctypes.data, bufs[0].data_ptr(), bufs[1].data_ptr(),
                        bufs[2].data_ptr(), hist.ctypes.data, ctypes.addressof(info))
    return (rc,) + tuple(b.cpu().numpy() for b in bufs) + (hist, list(info))


def test_shapes(fcmod, lfr):
    n = lfr.N
    rng = np.random.default_rng(9)
    labs = np.stack([rng.permutation(n) % 12 for _ in range(5)])
    with engine(fcmod, lfr, labs) as eng:
        got, _ = check(eng, labs, np.full(n, 3), slow_members=5 * n)       # K = 1: twelve labels per lane
        assert got["k"] == 1 and got["moved"] == 0 and got["unanimous"] == n
        got, _ = check(eng, labs, rng.permutation(n), slow_members=0)      # K = N
        assert got["k"] == n
        sparse = np.array([5, 900, 17])[rng.integers(0, 3, n)]
        got, ref = check(eng, labs, sparse)
        assert set(got["top"].tolist()) <= {5, 17, 900}
        rc, top, tv, own, hist, info = raw_vote(eng, sparse, n)
        assert rc == 0
        for a, f in ((top, "top"), (tv, "top_votes"), (own, "own_votes")):
            assert np.array_equal(a[:n], got[f]) and np.array_equal(a[n:], [-7] * 3), f
        assert np.array_equal(hist[:6], got["own_hist"]) and np.array_equal(hist[6:], [-7] * 3)
        assert info[:8] == [got[f] for f in INFO[:8]]


# ------------------------------------------------------------------ 8. fc_vote_count on a given buffer
def test_count_on_a_given_buffer(fcmod, lfr):
    n, n_r = lfr.N, 65
    rng = np.random.default_rng(n_r)
    labs = rng.integers(0, 3, (n_r, n))
    part = rng.integers(0, 40, n) * 2                                      # odd ids do not occur
    with engine(fcmod, lfr, labs) as eng:
        exp = eng.vote(part)
        mapped = eng.vote_map(part)["mapped"]
        with engine(fcmod, lfr) as other:                                   # an engine without labelings
            for buf in (mapped, mapped[torch.as_tensor(rng.permutation(n_r), device="cuda:0")].contiguous()):
                got = other.vote(part, dev_mapped=buf)
                for f in ARRAYS + ("own_hist", "k", "k_voted", "moved", "unanimous", "tied", "slow_nodes", "n_total"):
                    assert np.array_equal(got[f], exp[f]), f
            lab = np.ascontiguousarray(part, dtype=np.int32)
            for foreign in (3, n + 5, -1):                                  # not in P; outside [0, n)
                bad = mapped.clone()
                bad[n_r - 1, 777] = foreign
                outs = [torch.full((n,), -7, dtype=torch.int32, device="cuda:0") for _ in range(3)]
                hist = np.full(n_r + 1, -7, np.int64)
                info = (ctypes.c_int64 * 9)(*([-7] * 9))
                torch.cuda.synchronize()
                rc = other._L.fc_vote_count(other._ctx, lab.ctypes.data, bad.data_ptr(), n_r, outs[0].data_ptr(),
                                            outs[1].data_ptr(), outs[2].data_ptr(), hist.ctypes.data,
                                            ctypes.addressof(info))
                assert rc == -1 and all(bool((o == -7).all()) for o in outs)
                assert np.all(hist == -7) and list(info) == [-7] * 9
            assert np.array_equal(other.vote(part, dev_mapped=mapped)["top"], exp["top"])


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
        check(eng, labs, labs[5])
        after = (eng.get_labels(20), eng.score_pairs(pairs), eng.coassociation(nodes).cpu().numpy())
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2])
        assert before[1].tobytes() == after[1].tobytes()
        assert np.array_equal(before[2], car.matrix(labs, nodes))


# ------------------------------------------------------------------ 10. reuse and memory
def test_reuse_and_memory(fcmod, lfr):
    labs = lfr.cd_batches[0]
    part = lfr.cd_batches[-1][2]
    with engine(fcmod, lfr, labs) as eng:
        fresh = eng.vote(part)
    with engine(fcmod, lfr) as eng:
        eng.run(0, 20, 0.2, 0.02)
        eng.score_partitions()
        eng.cluster_consensus(eng.consensus_partition()["labels"])
        eng.vote(eng.get_labels(20)[3])
        eng.reset_graph()
        eng.set_labels(labs)
        used = eng.vote(part)
        assert fcmod.device_bytes() > 0
    for f in INFO + ARRAYS + ("own_hist",):
        assert np.array_equal(used[f], fresh[f]), f
    gc.collect()
    assert fcmod.device_bytes() == 0


# ------------------------------------------------------------------ 11. errors
def test_errors(fcmod, lfr):
    n = lfr.N
    labs = lfr.cd_batches[0]

    def untouched(res):
        rc, top, tv, own, hist, info = res
        return all(np.all(a == -7) for a in (top, tv, own, hist)) and info == [-7] * 9

    with engine(fcmod, lfr) as eng:
        res = raw_vote(eng, labs[0], n)                                     # no labelings
        assert res[0] == -4 and untouched(res)
        dev = torch.zeros((2, n), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        lab0 = np.ascontiguousarray(labs[0], dtype=np.int32)
        assert eng._L.fc_vote_map(eng._ctx, lab0.ctypes.data, dev.data_ptr(), None) == -4
        assert eng._L.fc_vote_count(eng._ctx, lab0.ctypes.data, dev.data_ptr(), 0, None, None, None, None, None) == -1
        eng.set_labels(labs)
        bad = labs[0].copy()
        bad[123] = n
        res = raw_vote(eng, bad, n)                                         # an id equal to n
        assert res[0] == -1 and untouched(res) and "index 123" in eng._L.fc_last_error().decode()
        with pytest.raises(fcmod.FastConsensusError) as ei:
            eng.vote(bad)
        assert ei.value.code == -1 and "index 123" in str(ei.value)
        res = raw_vote(eng, None, n)                                        # NULL labels
        assert res[0] == -1 and untouched(res)
        check(eng, labs, labs[0])                                           # and the engine still works
    with fcmod.Engine(seed=SEED) as eng:                                    # no graph
        lab0 = np.ascontiguousarray(labs[0], dtype=np.int32)
        assert eng._L.fc_vote(eng._ctx, lab0.ctypes.data, None, None, None, None, None) == -4
        assert eng._L.fc_vote_map(eng._ctx, lab0.ctypes.data, None, None) == -4
        assert eng._L.fc_vote_count(eng._ctx, lab0.ctypes.data, None, 1, None, None, None, None, None) == -4


# ------------------------------------------------------------------ 12. timing
def test_timing(fcmod, lfr):
    # the crafted input runs the map's fallback, vote_edge's the vote's
    part, labs, d, sizes = crafted(lfr.N, 12, (1, 8, 9, 12))
    with engine(fcmod, lfr, labs) as eng:
        assert eng.vote(part)["slow_members"] > 0
        eng.set_timing(True)
        try:
            eng.vote(part)
            t = eng.vote_timing()
            assert list(t) == PHASES and all(x > 0.0 for x in t.values())
            eng.vote_map(part)
            t = eng.vote_timing()
            assert t["segments"] > 0.0 and t["map"] > 0.0 and t["map_fallback"] > 0.0 and t["count"] == 0.0
            part2, labs2, _ = vote_edge(lfr.N, (9, 12, 40))
            eng.set_labels(labs2)
            assert eng.vote(part2)["slow_nodes"] == 3
            t = eng.vote_timing()
            assert list(t) == PHASES and all(x > 0.0 for x in t.values())
            eng.set_labels(labs)
        finally:
            eng.collect_timing()
            eng.set_timing(False)
        eng.vote(part)
        assert eng.vote_timing() == dict.fromkeys(PHASES, 0.0)


# ------------------------------------------------------------------ 13. entry points
def test_fast_consensus_flag(fcmod, lfr):
    e = lfr.edges_file
    G = fcmod.IdGraph(np.arange(lfr.N), e[:, 0], e[:, 1])
    parts, cons = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus="best", vote=True)
    labs = np.array([[p[x] for x in range(lfr.N)] for p in parts])
    ref = vr.refine(labs, cons["labels"])
    assert cons["voted"].dtype == np.int32 and np.array_equal(cons["voted"], ref["labels"])
    assert cons["vote_rounds"] == ref["rounds"] and cons["vote_moved"] == ref["moved_per_round"]
    assert cons["vote_confidence"].dtype == np.float64
    assert np.array_equal(cons["vote_confidence"], ref["own"] / np.float64(20))
    parts2, cons2 = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus="best")
    assert parts2 == parts and np.array_equal(cons2["labels"], cons["labels"])
    assert sorted(set(cons) - set(cons2)) == ["vote_confidence", "vote_moved", "vote_rounds", "voted"]
    with pytest.raises(ValueError):
        fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, vote=True)


def test_run_sharded_flag(fcmod, lfr):
    """the sharded driver on one rank: the consensus dict gains the refined partition"""
    from fastconsensus_amd.distributed import run_sharded
    with engine(fcmod, lfr) as eng:
        labels, st, cons = run_sharded(eng, 0, 20, 0.2, 0.02, consensus="best", vote=True)
        ref = vr.refine(labels, cons["labels"])
        assert cons["voted"].dtype == np.int32 and np.array_equal(cons["voted"], ref["labels"])
        assert cons["vote_rounds"] == ref["rounds"] and cons["vote_moved"] == ref["moved_per_round"]
        assert np.array_equal(cons["vote_confidence"], ref["own"] / np.float64(20))
        with pytest.raises(ValueError):
            run_sharded(eng, 0, 20, 0.2, 0.02, vote=True)


def test_cli_flag(fcmod, tmp_path, monkeypatch, capsys):
    from fastconsensus_amd import cli
    graph = os.path.join(golden_io.GOLDEN, "karate_club.txt")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as ei:
        cli.main(["-f", graph, "-np", "20", "--seed", "5", "--vote"])
    assert "--consensus" in str(ei.value.code) and not os.listdir(str(tmp_path))
    cli.main(["-f", graph, "-np", "20", "--seed", "5", "--consensus", "0.5", "--vote"])
    assert capsys.readouterr().out == ""
    suffix = "t0.2_d0.02_np20"
    d = tmp_path / ("consensus_" + suffix)
    assert sorted(os.listdir(str(d))) == ["membership", "partition", "vote.tsv"]
    # the n_p partitions and the consensus partition as the run wrote them: node+1 <TAB> community+1
    names = [a for a, _ in (line.split() for line in (d / "membership").read_text().splitlines())]
    part = np.array([int(b) - 1 for _, b in (line.split() for line in (d / "membership").read_text().splitlines())])
    labs = []
    for i in range(20):
        rows = dict(line.split() for line in (tmp_path / ("memberships_" + suffix) / str(i)).read_text().splitlines())
        labs.append([int(rows[a]) for a in names])
    ref = vr.vote(np.array(labs), part)
    rows = {r[0]: r[1:] for r in (line.split("\t") for line in (d / "vote.tsv").read_text().splitlines())}
    assert len(rows) == len(names)
    # membership lists node+1, vote.tsv the node label itself
    got = [[int(x) for x in rows[str(int(a) - 1)]] for a in names]
    assert got == [[c + 1, t + 1, o, tv] for c, t, o, tv in zip(part.tolist(), ref["top"].tolist(), ref["own"].tolist(),
                                                                ref["top_votes"].tolist())]
