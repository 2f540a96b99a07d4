"""Device scoring (fc_score_partitions / fc_score_pairs) against tests/score_ref.py.

Every integer field equals the reference bit for bit, on the register path and on the exact
fallback.  Float bounds (score_ref.float_bound(n) = 4 n 2^-53 ln n, 3.1e-12 at n = 1000):
entropy and mi within the bound, nmi within bound / mean entropy where that is >= 1 nat,
modularity and ari within 1e-15 of the exact rational rounded once.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dist_gates, golden_io, score_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_INTS = ("cells", "sum_sq")
PART_INTS = ("k", "max_size", "sum_sq", "in_weight", "tot_sq")


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


@pytest.fixture(scope="module")
def lfr():
    case = golden_io.load("lfr1k_louvain_np20")
    planted = np.load(os.path.join(golden_io.GOLDEN, "lfr1k_mu04_planted.npy"))
    return case, planted


def engine(fcmod, case, labels=None):
    eng = fcmod.Engine(seed=1)
    e = case.edges_file
    eng.load_graph(case.N, e[:, 0], e[:, 1])
    if labels is not None:
        eng.set_labels(labels)
    return eng


_pair_cache = {}


def ref_pair(a, b):
    key = (a.tobytes(), b.tobytes())
    if key not in _pair_cache:
        _pair_cache[key] = score_ref.pair(a, b)
    return _pair_cache[key]


def check_pair(rec, a, b, n):
    exp = ref_pair(np.ascontiguousarray(a), np.ascontiguousarray(b))
    tag = (int(rec["a"]), int(rec["b"]))
    for f in PAIR_INTS:
        assert int(rec[f]) == exp[f], (tag, f, int(rec[f]), exp[f])
    bound = score_ref.float_bound(n)
    assert abs(rec["mi"] - exp["mi"]) <= bound, (tag, rec["mi"], exp["mi"])
    if exp["h_mean"] >= 1.0:
        assert abs(rec["nmi"] - exp["nmi"]) <= bound / exp["h_mean"], (tag, rec["nmi"], exp["nmi"])
    if exp["nmi"] in (0.0, 1.0) and exp["h_mean"] == 0.0:
        assert rec["nmi"] == exp["nmi"], tag
    assert abs(rec["ari"] - exp["ari"]) <= 1e-15, (tag, rec["ari"], exp["ari"])


def check_parts(got, labels, u, v, w, n):
    for r, lab in enumerate(labels):
        exp = score_ref.part(lab, u, v, w)
        for f in PART_INTS:
            assert int(got[f][r]) == exp[f], (r, f, int(got[f][r]), exp[f])
        assert abs(got["entropy"][r] - exp["entropy"]) <= score_ref.float_bound(n), r
        assert abs(got["modularity"][r] - exp["modularity"]) <= 1e-15, (r, got["modularity"][r], exp["modularity"])


# ------------------------------------------------------------------ 1. golden labelings
@pytest.mark.parametrize("name", ["lfr1k_louvain_np20", "lfr1k_lpm_np20", "lfr1k_mu03_lpm_np20",
                                  "karate_louvain_np50"])
def test_golden_labelings(fcmod, name):
    case = golden_io.load(name)
    labs = case.cd_batches[0]
    e = case.edges_file
    with engine(fcmod, case, labs) as eng:
        check_parts(eng.score_partitions("input"), labs, e[:, 0], e[:, 1], None, case.N)
        rec = eng.score_pairs()
        n_r = len(labs)
        assert len(rec) == n_r * (n_r - 1) // 2
        assert [(int(x["a"]), int(x["b"])) for x in rec] == [(a, b) for a in range(n_r) for b in range(a + 1, n_r)]
        for x in rec:
            check_pair(x, labs[x["a"]], labs[x["b"]], case.N)
        if name == "lfr1k_louvain_np20":
            assert (rec["slow_members"] == 0).any()
        if name == "lfr1k_lpm_np20":           # batch 0 holds the single-community labeling
            ones = [r for r in range(n_r) if len(set(labs[r].tolist())) == 1]
            assert ones
            r = ones[0]
            assert eng.score_partitions("input")["k"][r] == 1
            d = eng.score_pairs([[r, r]])[0]
            assert d["nmi"] == 1.0 and d["ari"] == 1.0 and d["cells"] == 1 and d["sum_sq"] == case.N ** 2


# ------------------------------------------------------------------ 2. crafted boundaries
def crafted(n):
    rows, pairs = [], []
    for s in (1, 2, 63, 64, 65, 1000):
        a = np.arange(n, dtype=np.int64)
        a[:s] = 0
        ia = len(rows)
        rows.append(a)
        for d in sorted({x for x in (1, 2, 7, 8, 9, 16, 17, 64, 65, s) if x <= s}):
            b = np.arange(n, dtype=np.int64) + n
            b[:s] = np.arange(s) * d // s
            pairs.append((ia, len(rows), s, d))
            rows.append(b)
    return np.stack(rows), pairs


def test_crafted_boundaries(fcmod, lfr):
    case, _ = lfr
    rows, pairs = crafted(case.N)
    single = np.arange(case.N)
    rows = np.concatenate([rows, single[None], single[None][:, ::-1]])
    i1, i2 = len(rows) - 2, len(rows) - 1
    with engine(fcmod, case, rows) as eng:
        rec = eng.score_pairs([(a, b) for a, b, _, _ in pairs] + [(i1, i2)])
        for x, (a, b, s, d) in zip(rec, pairs):
            check_pair(x, rows[a], rows[b], case.N)
            assert x["cells"] == case.N - s + d
            # the register list holds 8 labels (score.h SC_D): the ninth sends the community's s
            # members of this pair to the fallback; s <= 1000 is below the length cap
            assert x["slow_members"] == (0 if d <= 8 else s), (s, d)
        last = rec[-1]
        assert last["nmi"] == pytest.approx(1.0, abs=score_ref.float_bound(case.N) / np.log(case.N))
        assert last["ari"] == 1.0 and last["cells"] == case.N and last["slow_members"] == 0


# ------------------------------------------------------------------ 3. replica counts
@pytest.mark.parametrize("n_r", [1, 3, 20, 64, 70])
def test_replica_counts(fcmod, lfr, n_r):
    case, _ = lfr
    base = case.cd_batches[0]
    rng = np.random.default_rng(n_r)
    labs = np.stack([rng.permutation(case.N)[base[r % len(base)]] if r >= len(base) else base[r] for r in range(n_r)])
    if n_r > 20:
        labs[21] = golden_io.load("lfr1k_lpm_np20").cd_batches[0][3]
    e = case.edges_file
    with engine(fcmod, case, labs) as eng:
        part = eng.score_partitions("input")
        sel = sorted({0, n_r - 1, n_r // 2, min(21, n_r - 1), min(64, n_r - 1)})
        check_parts({k: v[sel] for k, v in part.items()}, labs[sel], e[:, 0], e[:, 1], None, case.N)
        if n_r == 1:
            assert len(eng.score_pairs()) == 0 and eng.nmi_matrix().tolist() == [[1.0]]
            return
        hi = n_r - 1
        want = [(0, hi), (hi, 0), (hi - 1, hi), (n_r // 2, 0), (min(21, hi), hi)]
        if n_r == 70:
            want += [(64, 65), (65, 64), (0, 69), (69, 0), (63, 64)]
        rec = eng.score_pairs(want)
        for x, (a, b) in zip(rec, want):
            check_pair(x, labs[a], labs[b], case.N)
        by = {(int(x["a"]), int(x["b"])): x for x in rec}
        for a, b in want:
            if (b, a) in by:
                assert all(by[(a, b)][f] == by[(b, a)][f] for f in PAIR_INTS)
        m = eng.nmi_matrix()
        assert m.shape == (n_r, n_r) and np.array_equal(m, m.T) and np.all(np.diag(m) == 1.0)
        assert abs(m[0, hi] - by[(0, hi)]["nmi"]) <= 1e-12


# ------------------------------------------------------------------ 4. reference row
def test_reference_row(fcmod, lfr):
    case, planted = lfr
    labs = case.cd_batches[0][:5]
    with engine(fcmod, case, labs) as eng:
        with pytest.raises(fcmod.FastConsensusError) as ei:
            eng.score_pairs([(-1, 0)])
        assert ei.value.code == -4
        with pytest.raises(fcmod.FastConsensusError) as ei:
            eng.score_pairs([(0, 5)])
        assert ei.value.code == -1
        with pytest.raises(fcmod.FastConsensusError) as ei:
            eng.score_pairs([(-2, 0)])
        assert ei.value.code == -1
        eng.set_reference(np.array(["c%d" % x for x in planted]))   # any ids compare by equality only
        named = eng.score_pairs([(-1, 0)])[0]
        eng.set_reference(planted * 3 + 1)               # 1-based and sparse: compacted on the host
        assert all(named[f] == eng.score_pairs([(-1, 0)])[0][f] for f in PAIR_INTS)
        rec = eng.score_pairs()
        assert len(rec) == 10 + 5 and [int(x["a"]) for x in rec[10:]] == [-1] * 5
        for x in rec[10:]:
            check_pair(x, planted, labs[x["b"]], case.N)
        for x in eng.score_pairs([(2, -1), (-1, -1)]):
            check_pair(x, planted if x["a"] < 0 else labs[x["a"]], planted, case.N)
        eng.set_reference(None)
        assert len(eng.score_pairs()) == 10
        eng.set_reference(planted)
        e = case.edges_file
        eng.load_graph(case.N, e[:, 0], e[:, 1])         # clears the reference (and the labelings)
        eng.set_labels(labs)
        with pytest.raises(fcmod.FastConsensusError) as ei:
            eng.score_pairs([(-1, 0)])
        assert ei.value.code == -4


def test_state_errors(fcmod, lfr):
    case, _ = lfr
    with fcmod.Engine(seed=1) as eng:
        with pytest.raises(fcmod.FastConsensusError) as ei:
            fcmod.core.check(eng._L.fc_score_partitions(eng._ctx, 0, None))
        assert ei.value.code == -4
    with engine(fcmod, case) as eng:                      # a graph, no labelings
        with pytest.raises(fcmod.FastConsensusError) as ei:
            eng.score_pairs([(0, 0)])
        assert ei.value.code == -4


# ------------------------------------------------------------------ 5. weighted graph (and the forced fallback)
def weighted_run(fcmod, case):
    """run -> scores on both graphs and all pairs, as plain ints / floats"""
    with engine(fcmod, case) as eng:
        labels, _ = eng.run(0, 8, 0.2, 0.02)
        got = eng.get_labels(8)
        u, v, w, _ = eng.get_graph()
        work, inp = eng.score_partitions("working"), eng.score_partitions("input")
        rec = eng.score_pairs()
    return labels, got, (u, v, w), work, inp, rec


def ints_of(work, inp, rec):
    return {"working": {f: [int(x) for x in work[f]] for f in PART_INTS},
            "input": {f: [int(x) for x in inp[f]] for f in PART_INTS},
            "pairs": {f: [int(x) for x in rec[f]] for f in PAIR_INTS + ("a", "b")},
            "slow": [int(x) for x in rec["slow_members"]]}


def test_weighted_graph_and_forced_fallback(fcmod, lfr):
    case, _ = lfr
    labels, got, (u, v, w), work, inp, rec = weighted_run(fcmod, case)
    assert int(w.max()) > 1
    e = case.edges_file
    check_parts(work, got, u, v, w, case.N)
    check_parts(inp, got, e[:, 0], e[:, 1], None, case.N)
    for x in rec:
        check_pair(x, got[x["a"]], got[x["b"]], case.N)
    auto = ints_of(work, inp, rec)
    # the same run with every (community, replica) through the exact fallback, in two key
    # chunks per row at the least: same integers
    env = dict(os.environ, FC_SCORE_SLOW="1", FC_SCORE_CHUNK="1")
    out = subprocess.run([sys.executable, "-c",
                          "import json, sys; sys.path.insert(0, %r)\n"
                          "import fastconsensus_amd as fc\n"
                          "from tests import golden_io, test_gpu_score as t\n"
                          "r = t.weighted_run(fc, golden_io.load('lfr1k_louvain_np20'))\n"
                          "print('INTS', json.dumps(t.ints_of(*r[3:])))\n" % ROOT],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    slow = json.loads([l for l in out.stdout.splitlines() if l.startswith("INTS ")][-1][5:])
    assert slow["slow"] == [case.N] * len(rec)
    assert auto["slow"] != slow["slow"]
    for k in ("working", "input", "pairs"):
        assert slow[k] == auto[k], k


def _long_community_rows(n):
    """Row 0: three communities, each longer than FC_SCORE_LCAP, so every pair with it goes through
    the fallback.  Rows 1..7: 10..16 labels inside each of them, in cells of a few hundred members up to
    ~0.7 n / 3 members (n ln n from ~1e3 to ~5e5: the fixed point's integer and fraction parts both in use)."""
    i = np.arange(n, dtype=np.int64)
    span = n // 3 + 1
    a = i // span
    frac = (i % span) / span
    return np.stack([a] + [a * 64 + np.floor((9 + r) * frac ** (1 + r)).astype(np.int64) for r in range(1, 8)])


def test_fallback_log_sum_exact_in_any_order(fcmod, monkeypatch):
    """The fallback adds its n ln n terms exactly, so s_log, mi and nmi do not depend on the order
    or the grouping of the additions: one key chunk per row (default) and eight of them
    (FC_SCORE_CHUNK=1: 2 n keys each, other blocks and launches for the same runs) agree bit for
    bit, and s_log is the exact sum of its terms up to the logarithms' own rounding (2 ulps per
    term and one for the result: 2^-50 relative, against float_bound's 4 n 2^-53 ln n)."""
    n = 200_003
    rows = _long_community_rows(n)
    u = np.arange(n - 1, dtype=np.int32)
    pairs = [(0, r) for r in range(1, 8)]
    recs = []
    for chunk in (None, "1"):
        if chunk:
            monkeypatch.setenv("FC_SCORE_CHUNK", chunk)
        with fcmod.Engine(seed=1) as eng:
            eng.load_graph(n, u, u + 1)
            eng.set_labels(rows)
            recs.append(eng.score_pairs(pairs))
    one, many = recs
    assert (one["slow_members"] == n).all() and (many["slow_members"] == n).all()
    largest, smallest = 0, n
    for x in one:
        check_pair(x, rows[0], rows[x["b"]], n)
        cnt = np.unique(rows[0] * (1 << 20) + rows[x["b"]], return_counts=True)[1]
        exact = math.fsum(float(c) * math.log(float(c)) for c in cnt if c > 1)
        largest, smallest = max(largest, int(cnt.max())), min(smallest, int(cnt.min()))
        print("pair", int(x["b"]), "s_log", x["s_log"], "exact", exact, "rel", abs(x["s_log"] - exact) / exact)
        assert abs(x["s_log"] - exact) <= 2.0 ** -50 * exact
    assert largest > 40_000 and smallest < 1000      # the inputs: long and short cells
    for f in ("s_log", "mi", "nmi", "ari", "cells", "sum_sq"):
        assert np.array_equal(one[f], many[f]), f


# ------------------------------------------------------------------ 6. read-only
def test_scoring_is_read_only(fcmod, lfr):
    case, planted = lfr
    with engine(fcmod, case) as a, engine(fcmod, case) as b:
        la, _ = a.run(0, 8, 0.2, 0.02)
        lb, _ = b.run(0, 8, 0.2, 0.02)
        assert np.array_equal(la, lb)
        ga = a.get_graph()
        a.set_reference(planted)
        a.score_partitions("working"), a.score_partitions("input"), a.score_pairs(), a.nmi_matrix()
        assert np.array_equal(a.get_labels(8, renumber=True), la)
        assert np.array_equal(a.get_labels(8), b.get_labels(8))
        assert all(np.array_equal(x, y) for x, y in zip(ga, a.get_graph()))
        assert all(np.array_equal(x, y) for x, y in zip(a.get_nextgraph(), b.get_nextgraph()))
        la2, sa = a.run(0, 8, 0.2, 0.02)
        lb2, sb = b.run(0, 8, 0.2, 0.02)
        assert np.array_equal(la2, lb2) and sa["iterations"] == sb["iterations"]


# ------------------------------------------------------------------ 7. drop-in
def test_fast_consensus_scores(fcmod, lfr):
    case, planted = lfr
    e = case.edges_file
    g = fcmod.IdGraph(np.arange(case.N), e[:, 0], e[:, 1])
    plain = fcmod.fast_consensus(g, "louvain", n_p=8, seed=3)
    parts, sc = fcmod.fast_consensus(g, "louvain", n_p=8, seed=3, scores=True, truth=planted)
    assert parts == plain
    p3 = fcmod.fast_consensus(g, "louvain", n_p=8, seed=3, scores=True, return_stats=True,
                              truth=dict(zip(range(case.N), planted.tolist())))
    assert len(p3) == 3 and p3[0] == plain and "iterations" in p3[1]
    assert np.array_equal(p3[2]["nmi_truth"], sc["nmi_truth"])
    labs = np.array([[p[x] for x in range(case.N)] for p in parts])
    nmi = sc["nmi"]
    assert nmi.shape == (8, 8) and np.array_equal(nmi, nmi.T) and np.all(np.diag(nmi) == 1.0)
    assert sc["ari"].shape == (8, 8) and np.array_equal(sc["ari"], sc["ari"].T)
    for a in range(8):
        for b in range(a + 1, 8):
            exp = ref_pair(labs[a], labs[b])
            assert abs(nmi[a, b] - dist_gates.nmi(labs[a], labs[b])) <= score_ref.float_bound(case.N) / exp["h_mean"]
            assert abs(sc["ari"][a, b] - exp["ari"]) <= 1e-15
    others = (nmi.sum(1) - 1.0) / 7
    assert sc["medoid"] == int(np.flatnonzero(others == others.max())[0])
    assert sc["mean_pairwise_nmi"] == pytest.approx(nmi[np.triu_indices(8, 1)].mean(), abs=1e-15)
    for r in range(8):
        exp = score_ref.part(labs[r], e[:, 0], e[:, 1])
        assert sc["k"][r] == exp["k"] and abs(sc["modularity"][r] - exp["modularity"]) <= 1e-15
        t = ref_pair(planted, labs[r])
        assert abs(sc["nmi_truth"][r] - t["nmi"]) <= score_ref.float_bound(case.N) / t["h_mean"]
        assert abs(sc["ari_truth"][r] - t["ari"]) <= 1e-15
