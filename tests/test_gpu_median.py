"""core.median_refine over the device calls (fc_vote, fc_cluster_consensus, fc_item_affinity) against
tests/median_ref.py, and the entry points that run it.  Everything is an integer."""
import os

import numpy as np
import pytest

from tests import golden_io
from tests import median_ref as mr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 7                                    # an engine seed whose node map is not the identity
LISTS = ("objective", "proposed_per_round", "accepted_per_round", "alone_per_round", "gain_per_round")


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
    """the dict of core.median_refine against the dict of median_ref.refine"""
    assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], ref["labels"])
    assert (got["rounds"], got["converged"]) == (ref["rounds"], ref["converged"])
    for f in LISTS:
        assert got[f] == ref[f] and all(isinstance(x, int) for x in got[f]), f
    assert got["mean_rand"] == ref["mean_rand"]


# ------------------------------------------------------------------ recovery
def test_recovery(fcmod, lfr):
    labs = lfr.cd_batches[-1]
    orig = np.asarray(labs[0], np.int64)
    rng = np.random.default_rng(11)
    ids, size = np.unique(orig, return_counts=True)
    pick = rng.permutation(ids[size >= 3])[:20]
    assert len(pick) == 20
    part = orig.copy()
    for a, b in zip(pick[:10], pick[10:]):          # ten nodes from ten clusters into ten others
        part[rng.choice(np.flatnonzero(orig == a))] = b
    assert (part != orig).sum() == 10
    with engine(fcmod, lfr, labs) as eng:
        assert fcmod.median_refine(eng, orig)["rounds"] == 0            # the model's fixpoint
        got = fcmod.median_refine(eng, part)
        assert np.array_equal(got["labels"], orig) and got["rounds"] == 1 and got["converged"]
        assert got["accepted_per_round"] == [10] and got["alone_per_round"] == [0]
        cc = eng.cluster_consensus(orig)
        assert got["objective"][-1] == fcmod.median_objective(cc["pairs_total"], cc["size"], len(labs)) > got["objective"][0]
        assert got["mean_rand"][1] > got["mean_rand"][0]
        same(got, mr.refine(labs, part))
        again = fcmod.median_refine(eng, got["labels"])
        assert again["rounds"] == 0 and again["converged"] and again["objective"] == got["objective"][-1:]


# ------------------------------------------------------------------ trajectory
def test_trajectory(fcmod, lfr):
    labs = lfr.cd_batches[0]
    with engine(fcmod, lfr, labs) as eng:
        got = fcmod.median_refine(eng, labs[0], max_rounds=6)
    ref = mr.refine(labs, labs[0], max_rounds=6)
    same(got, ref)
    assert got["rounds"] == 6 and not got["converged"] and got["accepted_per_round"][0] > 0
    steps = [b - a for a, b in zip(got["objective"], got["objective"][1:])]
    assert all(s > 0 for s in steps) and steps == [2 * g for g in got["gain_per_round"]]
    assert got["objective"][0] == 947652 and sum(got["alone_per_round"]) > 0


def test_karate(fcmod):
    case = golden_io.load("karate_louvain_np50")
    labs = case.cd_batches[0]
    with engine(fcmod, case, labs) as eng:
        got = fcmod.median_refine(eng, labs[0])
        same(got, mr.refine(labs, labs[0]))
        assert got["converged"] and got["rounds"] == 3 and got["objective"] == [7564, 7596, 7692, 7768]
        # candidates of the caller's: a pair of lists, or a callable
        every = np.unique(labs[0])
        nodes, clusters = np.repeat(np.arange(case.N), len(every)), np.tile(every, case.N)
        wide = fcmod.median_refine(eng, labs[0], candidates=(nodes, clusters), max_rounds=1)
        assert wide["objective"][1] - wide["objective"][0] == 2 * wide["gain_per_round"][0]
        assert wide["objective"][1] == mr.objective(labs, wide["labels"])
        assert np.array_equal(wide["labels"], mr.moves(labs, labs[0], nodes, clusters)["labels"])
        none = fcmod.median_refine(eng, labs[0], candidates=lambda lab: ([], []), max_rounds=1)
        assert none["objective"][1] == mr.objective(labs, none["labels"])       # the "alone" moves only


# ------------------------------------------------------------------ entry points
KEYS = ["median", "median_mean_rand", "median_moved", "median_objective", "median_rounds"]


def same_result(cons, labs, start):
    ref = mr.refine(labs, start)
    assert cons["median"].dtype == np.int32 and np.array_equal(cons["median"], ref["labels"])
    assert cons["median_objective"] == ref["objective"] and cons["median_rounds"] == ref["rounds"]
    assert cons["median_moved"] == ref["accepted_per_round"] and cons["median_mean_rand"] == ref["mean_rand"]


def test_fast_consensus_flag(fcmod, lfr):
    e = lfr.edges_file
    G = fcmod.IdGraph(np.arange(lfr.N), e[:, 0], e[:, 1])
    parts, cons = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus="best", median=True)
    labs = np.array([[p[x] for x in range(lfr.N)] for p in parts])
    same_result(cons, labs, cons["labels"])
    parts2, cons2 = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus="best")
    assert parts2 == parts and np.array_equal(cons2["labels"], cons["labels"])
    assert sorted(set(cons) - set(cons2)) == KEYS
    parts3, cons3 = fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, consensus="best", vote=True, median=True)
    assert parts3 == parts
    same_result(cons3, labs, cons3["voted"])                             # with the vote: from its fixpoint
    with pytest.raises(ValueError):
        fcmod.fast_consensus(G, "louvain", n_p=20, seed=5, median=True)


def test_run_sharded_flag(fcmod, lfr):
    """the sharded driver on one rank: the consensus dict gains the refined partition"""
    from fastconsensus_amd.distributed import run_sharded
    with engine(fcmod, lfr) as eng:
        labels, st, cons = run_sharded(eng, 0, 20, 0.2, 0.02, consensus="best", median=True)
        same_result(cons, labels, cons["labels"])
        with pytest.raises(ValueError):
            run_sharded(eng, 0, 20, 0.2, 0.02, median=True)


def test_cli_flag(fcmod, tmp_path, monkeypatch, capsys):
    from fastconsensus_amd import cli
    graph = os.path.join(golden_io.GOLDEN, "karate_club.txt")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as ei:
        cli.main(["-f", graph, "-np", "20", "--seed", "5", "--median"])
    assert "--consensus" in str(ei.value.code) and not os.listdir(str(tmp_path))
    suffix = "t0.2_d0.02_np20"
    d = tmp_path / ("consensus_" + suffix)
    cli.main(["-f", graph, "-np", "20", "--seed", "5", "--consensus", "0.5"])
    assert sorted(os.listdir(str(d))) == ["membership", "partition"]     # no new files without the flag
    plain = (d / "membership").read_text()
    cli.main(["-f", graph, "-np", "20", "--seed", "5", "--consensus", "0.5", "--median"])
    assert capsys.readouterr().out == ""
    assert sorted(os.listdir(str(d))) == ["median.tsv", "median_membership", "membership", "partition"]
    assert (d / "membership").read_text() == plain
    # the n_p partitions and the consensus partition as the run wrote them (node+1 <TAB> community+1),
    # in the engine's node order: the selection breaks ties by node position
    names = [str(x + 1) for x in fcmod.IdGraph.from_edgelist_file(graph).labels.tolist()]

    def column(path):
        rows = dict(line.split() for line in path.read_text().splitlines())
        assert sorted(rows) == sorted(names)
        return [int(rows[a]) - 1 for a in names]

    part = np.array(column(d / "membership"))
    labs = np.array([column(tmp_path / ("memberships_" + suffix) / str(i)) for i in range(20)])
    ref = mr.refine(labs, part)
    assert [a for a, _ in (line.split() for line in (d / "median_membership").read_text().splitlines())] == \
        [a for a, _ in (line.split() for line in plain.splitlines())]
    assert column(d / "median_membership") == ref["labels"].tolist()
    tsv = [[int(x) for x in line.split("\t")] for line in (d / "median.tsv").read_text().splitlines()]
    assert [r[0] for r in tsv] == list(range(ref["rounds"] + 1)) and [r[1] for r in tsv] == ref["objective"]
    assert [r[2:] for r in tsv] == [[0, 0, 0]] + [list(x) for x in zip(ref["proposed_per_round"],
                                                                        ref["accepted_per_round"],
                                                                        ref["alone_per_round"])]
