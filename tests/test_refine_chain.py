"""core.check_consensus_flags and core.refine_consensus without an engine: the flag errors word for
word, and the chain vote -> median -> quality -> merge -> match driven by the CPU references
(vote_ref, cluster_consensus_ref, median_ref, merge_ref, match_ref) in place of the engine's calls."""
import itertools

import numpy as np
import pytest

from tests import cluster_consensus_ref as ccr
from tests import match_ref as mtr
from tests import median_ref as mr
from tests import merge_ref as mgr
from tests import vote_ref as vr

# ------------------------------------------------------------------ the flag check
ORDER = ("match", "merge", "quality", "median", "cluster_consensus", "vote")    # the first set one is named
NEEDS = {"match": "match=True needs consensus (a threshold or \"best\")",
         "merge": "merge=True needs consensus (a threshold or \"best\")",
         "quality": "quality=True needs consensus (a threshold or \"best\")",
         "median": "median=True needs consensus (a threshold or \"best\")",
         "cluster_consensus": "cluster_consensus=True needs consensus (a threshold or \"best\")",
         "vote": "vote=True needs consensus (a threshold or \"best\")"}
BEST = 'consensus must be a threshold in [0, 1] or "best"'


def raised(consensus, **flags):
    from fastconsensus_amd.core import check_consensus_flags
    with pytest.raises(ValueError) as e:
        check_consensus_flags(consensus, **flags)
    return str(e.value)


def test_each_flag_alone_and_in_pairs():
    from fastconsensus_amd.core import check_consensus_flags
    for f in ORDER:
        assert raised(None, **{f: True}) == NEEDS[f]
        assert raised(None, **dict({g: False for g in ORDER}, **{f: True})) == NEEDS[f]
    for a, b in itertools.combinations(ORDER, 2):   # a comes first in ORDER
        assert raised(None, **{a: True, b: True}) == NEEDS[a] == raised(None, **{b: True, a: True})
    every = {f: True for f in ORDER}
    assert raised(None, **every) == NEEDS["match"]
    for ok in (0.5, 0, 1.0, "best"):
        assert check_consensus_flags(ok, **every) is None
    assert check_consensus_flags(None) is None and check_consensus_flags(None, **{f: False for f in ORDER}) is None
    assert raised("worst") == BEST == raised("worst", **every) == raised("Best", vote=True)


# ------------------------------------------------------------------ the chain
VOTE_KEYS = {"voted", "vote_confidence", "vote_rounds", "vote_moved"}
MEDIAN_KEYS = {"median", "median_objective", "median_rounds", "median_moved", "median_mean_rand"}
MERGE_KEYS = {"merged", "merged_objective", "merged_rounds", "merged_accepted", "merged_k", "merged_mean_rand"}
MATCH_KEYS = {"match_inter", "match_csize", "match_stability", "match_recovered", "match_dissolved"}
N, R = 48, 5


def case():
    """48 nodes in 4 planted blocks, 5 noisy replicas, a start partition of 9 noisy fragments and a
    sparse random graph (for the merge candidates)"""
    rng = np.random.default_rng(21)
    truth = rng.integers(0, 4, N)
    labs = np.stack([np.where(rng.random(N) < 0.2, rng.integers(0, 4, N), truth) for _ in range(R)])
    start = np.where(rng.random(N) < 0.5, rng.integers(4, 9, N), truth).astype(np.int32)
    e = np.unique(np.sort(rng.integers(0, N, (140, 2)), 1), axis=0)
    e = e[e[:, 0] != e[:, 1]]
    return labs, start, e[:, 0], e[:, 1]


def calls_of(labs, u, v, asked):
    """the engine's calls from the references; `asked` collects what community_quality was asked"""
    def vote(lab):
        r = vr.vote(labs, lab)
        r["confidence"] = r["own"] / r["n_total"]
        return r

    def cluster(lab):
        ids, size, pairs, item = ccr.sums(labs, lab)
        return {"size": size, "cluster_pairs": pairs, "item_pairs": item, "n_total": len(labs)}

    def match(lab):
        ids, size, inter, csize = mtr.match(labs, lab)
        return dict(mtr.summary(inter, size, csize), ids=ids, size=size, inter=inter, csize=csize)

    def quality(lab):
        asked.append(np.array(lab))
        return {"asked": len(asked)}

    return {"vote": vote, "cluster_consensus": cluster,
            "item_affinity": lambda lab, nd, cl: {"aff": mr.affinity(labs, lab, nd, cl)},
            "community_graph": lambda lab: mgr.community_graph(N, u, v, None, lab),
            "cluster_coassoc": lambda lab, a, b: {"x": mgr.cross(labs, lab, a, b)},
            "cluster_match": match, "community_quality": quality, "sum_sq": mr.sum_sq(labs)}


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("flags", [("vote",), ("median",), ("vote", "median"), ("merge",),
                                   ("vote", "median", "merge", "match")], ids="+".join)
@pytest.mark.parametrize("quality", [False, True], ids=["", "quality"])
def test_chain_equals_the_steps_by_hand(flags, quality):
    from fastconsensus_amd.core import (match_result, median_refine, median_result, merge_refine, merge_result,
                                        refine_consensus, vote_refine, vote_result)
    labs, start, u, v = case()
    asked = []
    c = calls_of(labs, u, v, asked)
    base = {"labels": start, "k": 9}
    cons = dict(base)
    assert refine_consensus(None, cons, quality=quality, calls=c, **{f: True for f in flags}) is cons
    # the same steps by hand, each from its documented start
    want, parts = dict(base), [start]
    if "vote" in flags:
        want.update(vote_result(vote_refine(None, start, vote=c["vote"])))
        parts.append(want["voted"])
    if "median" in flags:
        want.update(median_result(median_refine(
            None, want["voted"] if "vote" in flags else start, vote=c["vote"], cluster_consensus=c["cluster_consensus"],
            item_affinity=c["item_affinity"], sum_sq=c["sum_sq"])))
        parts.append(want["median"])
    if "merge" in flags:
        begin = want["median"] if "median" in flags else want["voted"] if "vote" in flags else start
        want.update(merge_result(merge_refine(
            None, begin, community_graph=c["community_graph"], cluster_coassoc=c["cluster_coassoc"],
            cluster_consensus=c["cluster_consensus"], sum_sq=c["sum_sq"])))
        parts.append(want["merged"])
    if "match" in flags:
        want.update(match_result(None, start, cluster_match=c["cluster_match"]))
    keys = set(base)
    for f, ks in (("vote", VOTE_KEYS), ("median", MEDIAN_KEYS), ("merge", MERGE_KEYS), ("match", MATCH_KEYS)):
        keys |= ks if f in flags else set()
    assert set(want) == keys
    if quality:   # labels, voted, median, then merged: the stub numbers its calls
        names = ["quality"] + [f + "_quality" for f in ("voted", "median", "merged") if f in want]
        assert len(asked) == len(parts) and all(np.array_equal(a, p) for a, p in zip(asked, parts))
        want.update({name: {"asked": i + 1} for i, name in enumerate(names)})
    else:
        assert asked == []
    assert set(cons) == set(want)
    for k in want:
        assert same(cons[k], want[k]), k
    # the case does something at every step it takes
    assert "vote" not in flags or (cons["vote_rounds"] >= 1 and not np.array_equal(cons["voted"], start))
    assert "median" not in flags or cons["median_rounds"] >= 1
    assert flags != ("merge",) or cons["merged_rounds"] >= 1   # after vote and median nothing may be left to merge


def test_sum_sq_callable_is_evaluated_before_each_refinement():
    """the sharded driver's sum_sq is a collective: once in front of median, once in front of merge"""
    from fastconsensus_amd.core import refine_consensus
    labs, start, u, v = case()
    log = []
    c = calls_of(labs, u, v, [])
    T = c["sum_sq"]
    for name in ("vote", "cluster_consensus", "community_graph"):
        c[name] = (lambda f, name: lambda *a: (log.append(name), f(*a))[1])(c[name], name)
    c["sum_sq"] = lambda: (log.append("sum_sq"), T)[1]
    cons = refine_consensus(None, {"labels": start}, median=True, merge=True, calls=c)
    assert log.count("sum_sq") == 2 and log[0] == "sum_sq"
    second = len(log) - 1 - log[::-1].index("sum_sq")
    assert "community_graph" not in log[:second] and log[second + 1] == "cluster_consensus"
    plain = refine_consensus(None, {"labels": start}, median=True, merge=True, calls=dict(c, sum_sq=T))
    assert same(cons, plain)
