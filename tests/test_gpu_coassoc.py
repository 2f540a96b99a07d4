"""Co-association on the device (fc_coassociation / fc_coassoc_pairs / fc_coassoc_hist) against
tests/coassoc_ref.py.  Everything is an integer: every comparison is np.array_equal, and pac / cdf
(the same integers through the same float64 operations) compare with ==."""
import os

import numpy as np
import pytest

from tests import coassoc_ref as car
from tests import golden_io

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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
def lfr_full(lfr):
    """(labelings, the full N x N reference matrix) of the first LFR-1k batch (the counts spread over
    0..n_p), computed once"""
    labs = lfr.cd_batches[0]
    full = car.matrix(labs, np.arange(lfr.N))
    full.setflags(write=False)
    return labs, full


@pytest.fixture(scope="module")
def rand_eng(fcmod, lfr):
    """one engine on the LFR-1k graph for the tests that install their own labelings"""
    e = lfr.edges_file
    with engine(fcmod, lfr.N, e[:, 0], e[:, 1]) as eng:
        yield eng


def engine(fcmod, n, u, v, labels=None, seed=1):
    eng = fcmod.Engine(seed=seed)
    eng.load_graph(n, u, v)
    if labels is not None:
        eng.set_labels(labels)
    return eng


def host(t):
    a = t.cpu().numpy()
    assert a.dtype == np.int32
    return a


def spread(n_r, n, seed):
    return np.random.default_rng(seed).integers(0, 3, (n_r, n))


# ------------------------------------------------------------------ 1. golden labelings
@pytest.mark.parametrize("batch", [0, -1])
@pytest.mark.parametrize("name", ["lfr1k_louvain_np20", "lfr1k_mu03_lpm_np20", "karate_louvain_np50"])
def test_golden_labelings(fcmod, name, batch):
    case = golden_io.load(name)
    e = case.edges_file
    labs = case.cd_batches[batch]
    nodes = np.arange(case.N)
    with engine(fcmod, case.N, e[:, 0], e[:, 1], labs) as eng:
        mat = host(eng.coassociation(nodes))
        assert mat.shape == (case.N, case.N)
        assert np.array_equal(mat, car.matrix(labs, nodes))
        assert np.array_equal(np.diag(mat), np.full(case.N, case.n_p))
        assert np.array_equal(mat, mat.T)
        # the graph's own edges: consensus_support is in the engine's edge order -- internal
        # vertex ids, smaller end first, sorted by (smaller, larger)
        u, v, _, _ = eng.get_graph()
        cnt = host(eng.coassoc_pairs(np.stack([u, v], 1)))
        assert np.array_equal(cnt, car.pairs(labs, np.stack([u, v], 1)))
        sigma = eng.node_map()
        lo, hi = np.minimum(sigma[u], sigma[v]), np.maximum(sigma[u], sigma[v])
        assert np.array_equal(cnt[np.lexsort((hi, lo))], host(eng.consensus_support("input")))


# ------------------------------------------------------------------ 2. replica counts
@pytest.mark.parametrize("n_r", [1, 3, 4, 5, 63, 64, 65, 130])
def test_replica_counts(rand_eng, lfr, n_r):
    labs = spread(n_r, lfr.N, n_r)
    nodes = np.random.default_rng(100 + n_r).choice(lfr.N, 200, replace=False)
    rand_eng.set_labels(labs)
    exp = car.matrix(labs, nodes)
    assert len(np.unique(exp)) >= min(n_r, 4)                  # the counts spread, not only 0 and n_r
    assert np.array_equal(host(rand_eng.coassociation(nodes)), exp)
    h = rand_eng.coassoc_hist(nodes)
    assert h.dtype == np.int64 and h.shape == (n_r + 1,)
    assert np.array_equal(h, car.hist(labs, nodes))


# ------------------------------------------------------------------ 3. tile edges
@pytest.mark.parametrize("shape", [(1, 1), (1, 200), (63, 65), (64, 64), (65, 129), (129, 1)])
def test_tile_edges(rand_eng, lfr, lfr_full, shape):
    labs, full = lfr_full
    rand_eng.set_labels(labs)
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    a = rng.choice(lfr.N, shape[0], replace=False)
    b = rng.choice(lfr.N, shape[1], replace=False)
    got = host(rand_eng.coassociation(a, b))
    assert got.shape == shape and np.array_equal(got, full[np.ix_(a, b)])


def test_lists_with_duplicates_and_descending(rand_eng, lfr, lfr_full):
    labs, full = lfr_full
    rand_eng.set_labels(labs)
    rng = np.random.default_rng(8)
    dup = rng.integers(0, 50, 150)                            # 150 draws from 50 nodes
    other = rng.integers(0, lfr.N, 70)
    assert np.array_equal(host(rand_eng.coassociation(dup, other)), full[np.ix_(dup, other)])
    desc = np.arange(lfr.N - 1, lfr.N - 131, -1)
    assert np.array_equal(host(rand_eng.coassociation(desc)), full[np.ix_(desc, desc)])
    none = host(rand_eng.coassociation(dup))
    assert np.array_equal(none, host(rand_eng.coassociation(dup, dup)))
    assert np.array_equal(none, full[np.ix_(dup, dup)])
    out = torch.full((150 * 70 + 5,), -7, dtype=torch.int32, device="cuda:0")
    got = rand_eng.coassociation(dup, other, dev_out=out)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(host(got), full[np.ix_(dup, other)])
    assert np.array_equal(host(out[150 * 70:]), np.full(5, -7))    # nothing past na * nb is written
    assert host(rand_eng.coassociation([], other)).shape == (0, 70)
    assert host(rand_eng.coassoc_pairs(np.zeros((0, 2), np.int32))).shape == (0,)


# ------------------------------------------------------------------ 4. histogram
@pytest.mark.parametrize("k", [0, 1, 2, 64, 65, 130, 1000])
def test_histogram(fcmod, rand_eng, lfr, lfr_full, k):
    labs, _ = lfr_full
    rand_eng.set_labels(labs)
    nodes = np.random.default_rng(k).choice(lfr.N, k, replace=False)
    h = rand_eng.coassoc_hist(nodes)
    exp = car.hist(labs, nodes)
    assert h.dtype == np.int64 and np.array_equal(h, exp)
    assert int(h.sum()) == k * (k - 1) // 2
    assert fcmod.pac(h) == car.pac(h)
    assert np.array_equal(fcmod.consensus_cdf(h), car.cdf(h))
    assert fcmod.pac(h, 0.25, 0.75) == car.pac(h, 0.25, 0.75)


def test_histogram_duplicated_node(rand_eng, lfr, lfr_full):
    labs, _ = lfr_full
    rand_eng.set_labels(labs)
    nodes = np.r_[np.arange(100), 17]                          # positions 17 and 100 hold one node
    h = rand_eng.coassoc_hist(nodes)
    base = rand_eng.coassoc_hist(np.arange(100))
    assert np.array_equal(h, car.hist(labs, nodes))
    extra = h - base                                           # the pairs (i, 100): (17, 100) sits at n_r
    assert extra.sum() == 100 and extra[lfr.n_p] >= 1
    assert np.array_equal(rand_eng.coassoc_hist([5, 5]), np.eye(lfr.n_p + 1, dtype=np.int64)[lfr.n_p])


# ------------------------------------------------------------------ 5. live state
def test_live_state(fcmod, lfr):
    e = lfr.edges_file
    rng = np.random.default_rng(3)
    nodes = rng.choice(lfr.N, 300, replace=False)
    prs = rng.integers(0, lfr.N, (500, 2))
    runs = []
    with engine(fcmod, lfr.N, e[:, 0], e[:, 1], seed=11) as eng:
        for algo, tau in ((0, 0.2), (1, 0.8)):
            out, _ = eng.run(algo, 20, tau, 0.02)
            runs.append(out.copy())
            labs, graph = eng.get_labels(20), eng.get_graph()
            assert np.array_equal(host(eng.coassociation(nodes)), car.matrix(labs, nodes))
            assert np.array_equal(host(eng.coassoc_pairs(prs)), car.pairs(labs, prs))
            assert np.array_equal(eng.coassoc_hist(nodes), car.hist(labs, nodes))
            assert np.array_equal(eng.get_labels(20), labs)
            assert all(np.array_equal(x, y) for x, y in zip(eng.get_graph(), graph))
    with engine(fcmod, lfr.N, e[:, 0], e[:, 1], seed=11) as eng:
        for (algo, tau), exp in zip(((0, 0.2), (1, 0.8)), runs):
            assert np.array_equal(eng.run(algo, 20, tau, 0.02)[0], exp)


def test_timing(rand_eng, lfr, lfr_full):
    rand_eng.set_labels(lfr_full[0])
    rand_eng.set_timing(True)
    try:
        rand_eng.coassociation(np.arange(500))
        t = rand_eng.coassoc_timing()
        assert set(t) == {"ids", "count"} and t["count"] > 0.0 and t["ids"] > 0.0
    finally:
        rand_eng.collect_timing()
        rand_eng.set_timing(False)
    rand_eng.coassociation(np.arange(10))
    assert rand_eng.coassoc_timing() == {"ids": 0.0, "count": 0.0}


# ------------------------------------------------------------------ 6. errors
def test_errors(fcmod, lfr):
    e = lfr.edges_file
    calls = (lambda g: g.coassociation([0, 1]), lambda g: g.coassoc_pairs([(0, 1)]), lambda g: g.coassoc_hist([0, 1]))
    with fcmod.Engine(seed=1) as eng:
        for stage in ("no graph", "no labels"):
            for f in calls:
                with pytest.raises(fcmod.FastConsensusError) as ei:
                    f(eng)
                assert ei.value.code == -4, stage
            eng.load_graph(lfr.N, e[:, 0], e[:, 1])
        labs = lfr.cd_batches[0]
        eng.set_labels(labs)
        for bad in (lfr.N, -1):
            for f in (lambda g: g.coassociation([0, bad]), lambda g: g.coassociation([0], [1, bad]),
                      lambda g: g.coassoc_pairs([(0, 1), (bad, 2)]), lambda g: g.coassoc_hist([3, 4, bad])):
                with pytest.raises(fcmod.FastConsensusError) as ei:
                    f(eng)
                assert ei.value.code == -1 and "index" in str(ei.value)
                assert np.array_equal(host(eng.coassociation([0, 1, 2])), car.matrix(labs, [0, 1, 2]))


# ------------------------------------------------------------------ 7. drop-in
def test_drop_in(fcmod):
    case = golden_io.load("karate_louvain_np50")
    e = case.edges_file
    G = fcmod.IdGraph(np.arange(case.N), e[:, 0], e[:, 1])
    parts, cons, ca = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, coassoc=34, consensus=0.5)
    labs = np.array([[p[x] for x in range(case.N)] for p in parts])
    assert sorted(ca) == ["cdf", "hist", "matrix", "nodes", "order", "pac"]
    assert sorted(ca["nodes"]) == list(range(34))
    assert np.array_equal(ca["nodes"], np.random.default_rng(5).choice(34, size=34, replace=False))
    assert ca["matrix"].dtype == np.int32 and np.array_equal(ca["matrix"], car.matrix(labs, ca["nodes"]))
    assert np.array_equal(ca["hist"], car.hist(labs, ca["nodes"]))
    assert ca["pac"] == car.pac(ca["hist"]) and np.array_equal(ca["cdf"], car.cdf(ca["hist"]))
    by_order = cons["labels"][np.asarray(ca["nodes"])][ca["order"]]
    assert sorted(ca["order"].tolist()) == list(range(34)) and np.all(np.diff(by_order) >= 0)
    plain = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5)
    assert isinstance(plain, list) and plain == parts
    parts2, ca2 = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, coassoc=[33, 0, 2])
    assert parts2 == parts and "order" not in ca2 and ca2["nodes"] == [33, 0, 2]
    assert np.array_equal(ca2["matrix"], car.matrix(labs, [33, 0, 2]))


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for fn in files:
            with open(os.path.join(d, fn), "rb") as f:
                out[os.path.relpath(os.path.join(d, fn), root)] = f.read()
    return out


def test_cli_flag(fcmod, tmp_path, monkeypatch, capsys):
    from fastconsensus_amd import cli
    graph = os.path.join(golden_io.GOLDEN, "karate_club.txt")
    trees = []
    for extra in ([], ["--coassoc", "10"]):
        d = tmp_path / ("with" if extra else "without")
        d.mkdir()
        monkeypatch.chdir(d)
        cli.main(["-f", graph, "-np", "20", "--seed", "5"] + extra)
        trees.append(_tree(str(d)))
    assert capsys.readouterr().out == ""
    plain, flagged = trees
    assert sorted(set(flagged) - set(plain)) == ["coassoc.npy", "coassoc_nodes.txt"]
    assert all(flagged[k] == v for k, v in plain.items())          # the output tree is byte-identical
    mat = np.load(str(tmp_path / "with" / "coassoc.npy"))
    names = (tmp_path / "with" / "coassoc_nodes.txt").read_text().split()
    assert mat.dtype == np.int32 and mat.shape == (10, 10) and len(set(names)) == 10
    assert np.array_equal(np.diag(mat), np.full(10, 20)) and np.array_equal(mat, mat.T)
    # against the memberships the run wrote: node+1 <TAB> community+1 per line, one file per partition
    mem = tmp_path / "with" / "memberships_t0.2_d0.02_np20"
    labs = []
    for i in range(20):
        rows = [line.split() for line in (mem / str(i)).read_text().splitlines()]
        labs.append({str(int(a) - 1): int(b) for a, b in rows})
    exp = np.array([[sum(p[x] == p[y] for p in labs) for y in names] for x in names])
    assert np.array_equal(mat, exp)
