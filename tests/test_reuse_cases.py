"""CPU-only preconditions of the used-engine tests (tests/test_gpu_engine_reuse.py): the data of
tests/reuse_cases.py is what it claims to be, every reference is computable without a GPU and
deterministic, and every target still reaches the path it is there for."""
import numpy as np
import pytest

from tests import reuse_cases as rc

MUST_FOLLOW_ALL = ("bigger_first", "other_algorithms", "reseeded")


def equal(a, b):
    """== of references: dicts, sequences, arrays (exact), twins and traces by their fields"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    if hasattr(a, "__dict__"):
        return equal(vars(a), vars(b))
    return a == b


def test_ids_are_unique_and_the_matrix_is_generated():
    tids = [t.id for t in rc.TARGETS]
    hids = [h.__name__ for h in rc.HISTORIES]
    assert len(set(tids)) == len(tids) == 11 and len(set(hids)) == len(hids) == 10
    assert hids[0] == "fresh"
    full = {(h, t) for h in hids for t in tids if t in rc.NO_RELOAD.get(h, (t,))}
    assert len(rc.MATRIX) == len(set(rc.MATRIX)) and set(rc.MATRIX) == full - rc.DROPPED
    ids = [rc.pair_id(p) for p in rc.MATRIX]
    assert len(set(ids)) == len(ids) and "louvain_run-after-bigger_first" in ids
    # the cut rule: only pairs of the CD-batch and analysis targets, never after these histories
    assert rc.DROPPED <= full
    for h, t in rc.DROPPED:
        assert t in rc.CUTTABLE and h not in MUST_FOLLOW_ALL and h not in rc.NO_RELOAD, (h, t)
    for h in hids:
        after = {t for hh, t in rc.MATRIX if hh == h}
        if h in rc.NO_RELOAD:
            assert after == set(rc.NO_RELOAD[h])
            continue
        assert after & set(rc.WHOLE_RUNS) and after & set(rc.LEVEL_BATCHES) and "analysis" in after, h
    for t in tids:
        assert {h for h, tt in rc.MATRIX if tt == t} >= set(MUST_FOLLOW_ALL) | {"fresh"}, t


def test_bigger_first_dominates_and_karate_is_below():
    """From numpy alone: the history's graphs hold more nodes, more edges, a longer row and more
    replicas than any target's graph; karate fewer of each."""
    big = [rc.graph_stats(g) for g in rc.bigger_graphs()]
    n_big, m_big, d_big = (max(s[k] for s in big) for k in range(3))
    assert big[0][0] == rc.BIGGER_LFR[0]
    kn, km, kd = rc.graph_stats(rc.karate_graph())
    for t in rc.TARGETS:
        n, m, d = rc.graph_stats(t.graph())
        print("%s: N %d m %d max degree %d replicas %d" % (t.id, n, m, d, t.replicas))
        assert n_big > n > kn and m_big > m > km and d_big > d > kd, t.id
        assert max(rc.BIGGER_NP, rc.BIGGER_CD) > t.replicas >= 3, t.id      # smaller_first holds 3, as the Leiden targets do
        # the LFR-4000 graph alone is above every target in N and m (the hub graph adds the long row)
        assert big[0][0] > n and big[0][1] > m, t.id
    print("bigger_first: %s; karate: %s" % (big, (kn, km, kd)))
    seeds = {t.seed for t in rc.TARGETS}
    assert rc.RESEEDED_CREATE_SEED not in seeds


@pytest.mark.parametrize("target", rc.TARGETS, ids=lambda t: t.id)
def test_reference_is_computable_here_and_deterministic(target):
    from tests import infomap_graphs, leiden_graphs

    def compute():                                        # past every cache: a real computation
        leiden_graphs._twin_cache.clear()
        infomap_graphs._twin_cache.clear()
        return type(target).reference.__wrapped__(target)
    assert equal(compute(), compute())


def test_targets_reach_their_paths():
    run = rc.TARGET["louvain_run"].reference()
    assert run["iterations"] >= 3 and not run["hit_iter_cap"]
    for t in rc.WHOLE_RUNS:
        ref = rc.TARGET[t].reference()
        assert ref["iterations"] >= 1 and not ref["hit_iter_cap"], t
        assert ref["graph"][2].max() > 1 or t == "lpm_run", t             # a weighted final graph
    # the Leiden hub batch decides rows past 512 entries (k_lv_heavy); the weighted one has weights
    hub = rc.TARGET["leiden_hub700"].reference()
    assert sum(tr.decisions for tr in hub["traces"])[:, 3:].any()
    assert all(tr.levels >= 2 for tr in hub["traces"])
    assert rc.TARGET["leiden_weighted"].reference()["working"][3].max() > 1
    for t in ("infomap_hub700", "infomap_lfr1k"):
        tw = rc.TARGET[t].reference()
        assert tw.ambiguous() == (0, 0), t                                 # the twin determines the labels
        assert all(tr.levels >= 2 for tr in tw.all_traces()), t
    assert rc.TARGET["infomap_hub700"].reference().decisions()[:, 3:].any()
    # the 64-replica CD batches: one unit per wave in the replica-lane decide
    for t in ("cd_classic", "cd_replica_lane"):
        ref = rc.TARGET[t].reference()
        assert max(n_r for _, n_r in ref) >= 64 and {a for a, _ in ref} == {0, 1}, t
        assert all(lab.shape[0] == n_r for (_, n_r), lab in ref.items())
        assert not np.array_equal(ref[(0, 64)][0], ref[(0, 64)][1])        # replicas differ
    # the two CD engines are different semantics, not one reference twice
    assert not equal(rc.TARGET["cd_classic"].reference(), rc.TARGET["cd_replica_lane"].reference())
    step = rc.TARGET["step_api"].reference()
    assert step["candidates"] > 0 and step["m1"] > len(step["kept"][0]) and step["kept"][2].max() > 1
    ana = rc.TARGET["analysis"].reference()
    assert (ana["consensus"]["support_hist"] > 0).sum() >= 6              # supports spread over the levels
    assert 0 < ana["consensus"]["kept_edges"] < ana["consensus"]["edges"]
    assert 1 < ana["records"][rc.ANALYSIS_CUT]["k"] < ana["consensus"]["edges"]
    assert len(np.unique(ana["matrix"])) >= 6


def test_labelings_of_no_reload_history_differ_from_the_targets():
    """labels_replaced installs other labelings with the target's row count: stale derived state
    would change the target's result."""
    for t in rc.NO_RELOAD["labels_replaced"]:
        target = rc.TARGET[t]
        n, _ = target.graph()
        other = np.random.default_rng(31).integers(0, 4, (target.rows, n))
        mine = rc.lfr1k().cd_batches[0] if t == "step_api" else target.reference()["labs"]
        assert other.shape == mine.shape and not np.array_equal(other, mine)
