"""tests/vote_ref.py (np.unique over the nonempty cells) against a brute-force dense contingency
argmax, the vote's identities, both tie rules on hand-built cases, and vote_refine's fixpoint."""
import numpy as np
import pytest

from tests import vote_ref as vr


def brute(labs, part):
    """dense tables and Python loops, straight from the definitions"""
    labs, part = np.asarray(labs), np.asarray(part)
    n_r, n = labs.shape
    ids = sorted(set(part.tolist()))
    mapped = np.empty((n_r, n), np.int64)
    for r in range(n_r):
        for d in set(labs[r].tolist()):
            counts = [int(((part == k) & (labs[r] == d)).sum()) for k in ids]
            mapped[r, labs[r] == d] = ids[int(np.argmax(counts))]        # argmax: the first, so the smallest id
    own = np.empty(n, np.int64)
    top = np.empty(n, np.int64)
    top_votes = np.empty(n, np.int64)
    distinct = np.empty(n, np.int64)
    tied = 0
    for v in range(n):
        votes = {k: int((mapped[:, v] == k).sum()) for k in set(mapped[:, v].tolist())}
        best = max(votes.values())
        leaders = sorted(k for k, x in votes.items() if x == best)
        own[v] = votes.get(int(part[v]), 0)
        top_votes[v] = best
        top[v] = part[v] if part[v] in leaders else leaders[0]
        distinct[v] = len(votes)
        tied += len(leaders) > 1
    return mapped, own, top, top_votes, distinct, tied


@pytest.mark.parametrize("seed", range(6))
def test_reference_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    n, n_r = int(rng.integers(5, 60)), int(rng.integers(1, 12))
    part = rng.integers(0, rng.integers(1, 9), n) * 7 + 3                  # sparse ids
    labs = rng.integers(0, rng.integers(1, 7), (n_r, n)) * 5
    ref = vr.vote(labs, part)
    mapped, own, top, top_votes, distinct, tied = brute(labs, part)
    assert np.array_equal(ref["mapped"], mapped)
    for name, want in (("own", own), ("top", top), ("top_votes", top_votes), ("distinct", distinct)):
        assert np.array_equal(ref[name], want), name
    assert ref["tied"] == tied and ref["moved"] == (top != part).sum() and ref["unanimous"] == (own == n_r).sum()
    assert ref["k"] == len(np.unique(part)) and ref["k_voted"] == len(np.unique(top)) and ref["n_total"] == n_r
    assert ref["mapped_communities"] == sum(len(np.unique(row)) for row in labs)
    assert np.array_equal(ref["own_hist"], np.bincount(own, minlength=n_r + 1))
    # the identities
    assert np.all(ref["own"] <= ref["top_votes"]) and ref["own_hist"].sum() == n
    assert np.all(ref["top_votes"] * ref["distinct"] >= n_r)


def test_replicas_equal_to_the_partition():
    rng = np.random.default_rng(1)
    part = rng.integers(0, 9, 80) * 11
    ref = vr.vote(np.stack([part] * 5), part)
    assert np.array_equal(ref["top"], part) and np.array_equal(ref["own"], np.full(80, 5))
    assert ref["moved"] == 0 and ref["unanimous"] == 80 and ref["tied"] == 0 and np.all(ref["distinct"] == 1)


def test_community_numbering_does_not_matter():
    rng = np.random.default_rng(2)
    part = rng.integers(0, 6, 90)
    labs = rng.integers(0, 8, (7, 90))
    a = vr.vote(labs, part)
    labs2 = labs.copy()
    labs2[3] = rng.permutation(50)[labs[3]]                                # replica 3's communities renumbered
    b = vr.vote(labs2, part)
    for f in ("mapped", "own", "top", "top_votes", "distinct", "own_hist"):
        assert np.array_equal(a[f], b[f]), f
    assert {k: a[k] for k in vr.INFO} == {k: b[k] for k in vr.INFO}


def test_map_tie_takes_the_smallest_id():
    part = np.array([7] * 5 + [3] * 5 + [9] * 2)
    labs = np.array([[0] * 10 + [1] * 2])                                  # community 0: 5 / 5 between 7 and 3
    mapped, communities = vr.map_labelings(labs, part)
    assert np.array_equal(mapped[0], [3] * 10 + [9] * 2) and communities == 2


def test_vote_ties():
    # node 0: 2 / 2 between its own 5 and 2 -> keeps 5; node 1: 2 / 2 between 8 and 2 (not 5) -> 2;
    # node 2: its own cluster loses 1 : 3
    mapped = np.array([[5, 8, 9], [5, 8, 9], [2, 2, 9], [2, 2, 5]])
    ref = vr.count_votes(mapped, np.array([5, 5, 5]))
    assert np.array_equal(ref["top"], [5, 2, 9]) and np.array_equal(ref["top_votes"], [2, 2, 3])
    assert np.array_equal(ref["own"], [2, 0, 1]) and np.array_equal(ref["distinct"], [2, 2, 2])
    assert ref["tied"] == 2 and ref["moved"] == 2 and ref["unanimous"] == 0 and ref["k_voted"] == 3
    assert np.array_equal(ref["own_hist"], [1, 1, 1, 0, 0])


def test_refine_reaches_a_fixpoint():
    rng = np.random.default_rng(3)
    truth = rng.integers(0, 5, 200)
    labs = np.stack([np.where(rng.random(200) < 0.15, rng.integers(0, 5, 200), truth) for _ in range(9)])
    start = rng.integers(0, 12, 200)                                       # twelve fragments of noise
    res = vr.refine(labs, start, max_rounds=50)
    assert res["moved"] == 0 and res["rounds"] == len(res["moved_per_round"]) >= 1
    assert np.array_equal(vr.vote(labs, res["labels"])["top"], res["labels"])
    capped = vr.refine(labs, start, max_rounds=1)
    assert capped["rounds"] == 1 and capped["moved_per_round"] == res["moved_per_round"][:1]


def test_core_vote_refine_follows_the_reference():
    """core.vote_refine is the same loop around any voting function (here the reference's)"""
    from fastconsensus_amd.core import vote_refine
    rng = np.random.default_rng(4)
    labs = rng.integers(0, 4, (6, 120))
    start = rng.integers(0, 9, 120)

    def vote(lab):
        r = vr.vote(labs, lab)
        r["confidence"] = r["own"] / r["n_total"]
        return r

    got, want = vote_refine(None, start, max_rounds=20, vote=vote), vr.refine(labs, start, max_rounds=20)
    assert got["rounds"] == want["rounds"] and got["moved_per_round"] == want["moved_per_round"]
    assert np.array_equal(got["labels"], want["labels"]) and got["labels"].dtype == np.int32
