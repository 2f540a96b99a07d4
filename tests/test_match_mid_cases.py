"""The mid-size case of the cluster match (tests/match_mid.py), without a GPU: its inputs pass the
launch clamps of match.h's kernels, the chunk window of the fallback at the default FC_SCORE_CHUNK and
FC_SCORE_LCAP (so tests/test_gpu_match_mid.py is not empty), every cap read from the csrc sources by
name; its sparse reference equals tests/match_ref.py where the loop reference still runs; and the two
crafted cases do what they were built for: a 32-bit product, or a float32 division, gets them wrong."""
import os

import numpy as np
import pytest

from tests import analysis_mid as am
from tests import consensus_ref as cr
from tests import golden_io
from tests import match_mid as mm
from tests import match_ref as mr

RELATION = {">": lambda a, b: a > b, "==": lambda a, b: a == b, "<=": lambda a, b: a <= b}
MASK = (1 << 32) - 1


@pytest.fixture(scope="module")
def lfr():
    return golden_io.load("lfr1k_louvain_np20")


def test_clamps_are_read_from_the_sources():
    cl = mm.clamps()
    assert sorted(cl) == ["k_cm_fold", "k_cm_scatter", "k_cm_sizes", "k_cm_total"]
    assert all(isinstance(x, int) and x > 0 for x in cl.values())
    # each of the four kernels has one launch, so the clamp read is the one the call runs under
    for kernel in cl:
        assert am._src("match.h").count(kernel + "<<<") == 1, kernel
    # the fallback emits its keys through cluster.h's chunk driver and the match kernel takes
    # score.h's grid: match.h may hold no launch clamp of its own for either
    assert "cell_chunks<false>" in am._src("match.h") and "k_cc_emit<<<" not in am._src("match.h")
    assert am._src("cluster.h").count("k_cc_emit<<<") == 1 and am.caps()["k_cc_emit"] > 0
    assert "k_cm_match<<<dim3(score_count_grid(s.k), banks)" in am._src("match.h")
    assert "std::min<int64_t>((waves + 3) / 4, SC_GRID)" in am._src("score.h")
    # the chunk windows reached() assumes are the ones score_chunk_buffers computes
    assert "b.cap = std::max<int64_t>(2 * c.N, c.score_chunk);" in am._src("score.h")
    assert "b.step = b.cap - c.N;" in am._src("score.h")
    with pytest.raises(AssertionError):
        am.clamp("match.h", "k_cm_no_such_kernel")
    with pytest.raises(AssertionError):
        am.clamp("match.h", "k_cm_total")           # why match_mid keeps a pattern of its own for it


def test_every_cap_is_reached():
    got = mm.reached(am.case())
    for name, x in got.items():
        print(name, x)
    assert len(got) >= 28
    missed = {name: x for name, x in got.items() if not RELATION[x[1]](x[0], x[2])}
    assert not missed, missed


def test_partitions_of_the_case():
    c = am.case()
    k = am.caps()
    sizes = {name: np.unique(mm.partition(c, name), return_counts=True)[1] for name in mm.PARTS}
    assert [len(sizes[name]) for name in mm.PARTS] == [269_747, 18, 358_537]
    assert sizes["coarse"].max() == 358_519 and sizes["fine"].max() <= k["LCAP"]
    size, over, ncell = mm.coarse20()
    giant = int(np.argmax(size))
    assert over[:, giant].all() and ncell[:, giant].min() >= 1          # by length, whatever the row
    T, keys, runs, straddle = mm.fallback_chunks(over, ncell, size, c["n"], k["CHUNK"])
    assert T == int((over * size[None, :]).sum()) and int(runs.sum()) == int(ncell[over].sum())
    print("coarse x labs20: %d fallback keys, %d runs, chunks of %s keys and %s runs, %d items straddle"
          % (T, runs.sum(), keys.tolist(), runs.tolist(), straddle))


def test_fallback_chunks_on_a_crafted_plan():
    """three clusters of 5, 3 and 4 members, 66 rows (two banks); flagged: cluster 0 in rows 0, 1
    and 65, cluster 2 in rows 1 and 64.  N = 6, chunk = 14: cap 14, step 8.  The stream is bank 0:
    (0, row 0) at 0, (0, row 1) at 5, (2, row 1) at 10; bank 1: (0, row 65) at 14, (2, row 64) at 19;
    T = 23.  Chunk 0 owns the starts 0 and 5, chunk 1 the starts 10 and 14, chunk 2 the start 19."""
    size = np.array([5, 3, 4], np.int64)
    over = np.zeros((66, 3), bool)
    over[[0, 1, 65], 0] = True
    over[[1, 64], 2] = True
    ncell = np.zeros((66, 3), np.int32)
    ncell[0, 0], ncell[1, 0], ncell[1, 2], ncell[65, 0], ncell[64, 2] = 2, 5, 1, 3, 4
    T, keys, runs, straddle = mm.fallback_chunks(over, ncell, size, 6, 14)
    assert (T, keys.tolist(), runs.tolist(), straddle) == (23, [14, 14, 7], [7, 4, 4], 2)   # 5..10 and 14..19 cross 8 and 16


def check_same(labs, part, **kw):
    exp = mr.match(labs, part)
    got = mm.match(labs, part, **kw)
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape and np.array_equal(g, e)
    es, gs = mr.summary(exp[2], exp[1], exp[3]), mm.summary(got[2], got[1], got[3])
    assert sorted(gs) == sorted(es)
    for f in es:
        assert gs[f].dtype == es[f].dtype and gs[f].shape == es[f].shape and np.all(gs[f] == es[f]), f
    return got


def test_sparse_reference_equals_match_ref(lfr):
    u, v = cr.canonical_edges(lfr.edges_file[:, 0], lfr.edges_file[:, 1])
    labs = lfr.cd_batches[0]
    planted = np.load(os.path.join(golden_io.GOLDEN, "lfr1k_mu04_planted.npy"))
    rng = np.random.default_rng(5)
    n = lfr.N
    parts = [cr.partition(n, u, v, 0.5, labels=labs)["labels"], planted, labs[0], rng.integers(0, 40, n),
             rng.permutation(n), np.full(n, 3), np.array([5, 900, 17])[rng.integers(0, 3, n)]]
    for part in parts:
        assert len(part) == n
        check_same(labs, part)
        check_same(lfr.cd_batches[-1][4], part)                            # one row, handed in as [n]
    check_same(rng.integers(0, 3, (130, n)), rng.integers(0, 40, n))
    # equal-sized blocks: most clusters have several communities of the same J
    for _ in range(10):
        check_same(np.stack([rng.permutation(np.repeat(np.arange(12), 5)) for _ in range(3)]), np.repeat(np.arange(6), 10))
    for a_low in (True, False):
        ids, size, inter, csize = check_same(*mr.exact_tie(n, a_low)[::-1])
        assert (size[0], inter[0, 0], csize[0, 0]) == (4, 2, 6)
    ids, size, inter, csize = check_same(*mr.near_tie()[::-1])
    assert (size[0], inter[0, 0], csize[0, 0]) == (8001, 4000, 7998)


@pytest.mark.parametrize("name, row", [("part", 4), ("coarse", 5), ("fine", 2)])
def test_sparse_reference_equals_match_ref_on_a_row_of_the_case(name, row):
    """one row is what the loop reference still does at this size: some 400 k cells"""
    c = am.case()
    check_same(c["labs20"][row], mm.partition(c, name))


def test_a_wrong_proposal_is_decided_on_integers():
    """with a float32 proposal near_tie's two candidates are one number and the larger C is proposed,
    which is wrong; the integer check sees it and match_ref.better decides"""
    part, lab = mr.near_tie()
    assert np.float32(4000) / np.float32(11999) == np.float32(4001) / np.float32(12002)
    ids, size, inter, csize = check_same(lab, part, propose=np.float32)
    assert (inter[0, 0], csize[0, 0]) == (4000, 7998)
    for a_low in (True, False):
        part, lab = mm.near_tie_wide(a_low)
        got = mm.match(lab, part, propose=np.float32)
        assert (got[1][0], got[2][0, 0], got[3][0, 0]) == mm.NEAR
        assert all(np.array_equal(g, e) for g, e in zip(got, mm.match(lab, part)))


def masked_better(s, c1, t1, c2, t2):
    """match_ref.better with both products reduced mod 2^32: a 32-bit multiply"""
    a, b = (c1 * (s + t2 - c2)) & MASK, (c2 * (s + t1 - c1)) & MASK
    return a > b or (a == b and c1 > c2)


def best_by(rule, s, cand, reverse):
    best = (0, 0)
    for c, t in (cand[::-1] if reverse else cand):
        if rule(s, c, t, *best):
            best = (c, t)
    return best


@pytest.mark.parametrize("a_low", [True, False])
def test_wide_bites(a_low):
    part, lab = mm.wide(a_low)
    assert len(part) == len(lab) == am.N and part.min() == 0 and part.max() < am.N and lab.max() < am.N
    s, cand = mm.candidates(part, lab)
    assert (s, cand) == (100_000, [(50_000, 50_000), (45_000, 120_000), (5_000, 230_003)])
    a, b = cand[0], cand[1]
    la, lb = lab[0], lab[50_000]
    assert (la < lb) == a_low and (lab == la).sum() == 50_000 and (lab == lb).sum() == 120_000
    assert mm.cross_products(part, lab) == (8_750_000_000, 4_500_000_000) and min(mm.cross_products(part, lab)) > 1 << 32
    assert [x & MASK for x in mm.cross_products(part, lab)] == [160_065_408, 205_032_704]
    assert mr.better(s, *a, *b) and not mr.better(s, *b, *a)
    assert masked_better(s, *b, *a) and not masked_better(s, *a, *b)      # 32-bit products reverse the pair
    for reverse in (False, True):                                          # and the answer, in whatever order they are met
        assert best_by(mr.better, s, cand, reverse) == a
        assert best_by(masked_better, s, cand, reverse) == b
    ids, size, inter, csize = mm.match(lab, part)
    assert (size[0], inter[0, 0], csize[0, 0]) == mm.WIDE == (100_000, 50_000, 50_000)
    assert len(ids) == am.N - 99_999 and np.all(size[1:] == 1) and np.all(inter[0, 1:] == 1)
    assert np.array_equal(csize[0, 1:], np.bincount(lab)[lab[100_000:]])


@pytest.mark.parametrize("a_low", [True, False])
def test_near_tie_wide_bites(a_low):
    c = mm.NEAR_C
    part, lab = mm.near_tie_wide(a_low)
    assert len(part) == len(lab) == am.N == 4 * c + 3 and part.min() == 0 and part.max() < am.N and lab.max() < am.N
    s, cand = mm.candidates(part, lab)
    assert (s, cand) == (2 * c + 1, [(c + 1, 2 * c + 2), (c, 2 * c - 2)])
    b, a = cand
    la, lb = lab[0], lab[c]
    assert (la < lb) == a_low and (lab == la).sum() == 2 * c - 2 and (lab == lb).sum() == 2 * c + 2
    assert sorted(np.bincount(lab)[np.bincount(lab) > 0].tolist()) == [1, 1, 1, 2 * c - 2, 2 * c + 2]
    ua, ub = s + a[1] - a[0], s + b[1] - b[0]
    assert (ua, ub) == (3 * c - 1, 3 * c + 2)
    assert (a[0] * ub, b[0] * ua) == (3 * c * c + 2 * c, 3 * c * c + 2 * c - 1)
    assert sorted(mm.cross_products(part, lab)) == [30_000_199_999, 30_000_200_000]
    assert np.float32(a[0]) / np.float32(ua) == np.float32(b[0]) / np.float32(ub)       # float32 cannot tell them apart
    assert mr.better(s, *a, *b) and not mr.better(s, *b, *a)                             # the integer rule can
    assert b[0] > a[0]                                                                    # and the larger C alone picks B
    ids, size, inter, csize = mm.match(lab, part)
    assert (size[0], inter[0, 0], csize[0, 0]) == mm.NEAR == (200_001, 100_000, 199_998)
    assert len(ids) == 2 * c + 3 and np.all(size[1:] == 1) and np.all(inter[0, 1:] == 1)
    assert np.array_equal(csize[0, 1:], np.bincount(lab)[lab[2 * c + 1:]])
