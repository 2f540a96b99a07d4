"""fc_cluster_match on the device at mid size: the case of tests/analysis_mid.py (N = 400,003, 20
and 70 labelings) with the partitions of tests/match_mid.py, every integer against the sparse
reference.  Here k_cm_sizes, k_cm_match's x grid, k_cm_total, k_cm_scatter and k_cm_fold make a second
trip; `part` (269,747 clusters) numbers its entries bank * k + cluster with two banks and k past 2^18
and has register and fallback lanes in one call; `coarse` (a giant of 358,519 members) fills two to
seven chunks at the default FC_SCORE_CHUNK, its items straddling the windows; `fine` (358,537
clusters) stays in registers; and the two crafted partitions decide by cross products past 2^32, in
the fallback's fold and, under FC_SCORE_LCAP=262144, in the match kernel's own compare --
tests/test_match_mid_cases.py checks, without a GPU, that the inputs do reach each of these.
Everything is an integer: every comparison is np.array_equal, and the derived float arrays compare
with ==.

Not reached here: rows x ld past 2^31 in the caller's buffers (a 9 GB tensor on a shared card), and
nbk x 64 >= 2^32 slots, which is the fallback plan's FC_ELIMIT branch."""
import functools
import time

import numpy as np
import pytest

from tests import analysis_mid as am
from tests import match_mid as mm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 7                                    # an engine seed whose node map is not the identity
INFO = ("k", "max_size", "singletons", "perfect", "inter_total", "slow_members", "n_r")
DERIVED = ("jaccard", "f1", "stability", "recovered", "dissolved")
ORDERS = [True, False]


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


@pytest.fixture(scope="module")
def case(fcmod):
    c = am.case()
    yield c
    am.case.cache_clear()                   # about 1 GB of host arrays


@pytest.fixture(scope="module")
def refs(case):
    """the references here, so that no test's time holds one: part and coarse against the 70
    labelings (the 20 are their first rows), fine against the 20"""
    t0 = time.perf_counter()
    out, took = {}, {}
    for name, n_r in (("part", am.N_R2), ("coarse", am.N_R2), ("fine", am.N_R)):
        t1 = time.perf_counter()
        out[name] = mm.reference(case["labs%d" % n_r], mm.partition(case, name))
        took["%s x labs%d" % (name, n_r)] = round(time.perf_counter() - t1, 2)
    print("references: %.1f s" % (time.perf_counter() - t0), took)
    return out


class Mid:
    """the module's engine and which labelings it holds"""

    def __init__(self, eng, case):
        self.eng, self.case, self.held = eng, case, None

    def use(self, name, labs=None):
        """install case[name], or the labelings `labs` under the name `name`, unless they are held"""
        if self.held != name:
            self.eng.set_labels(self.case[name] if labs is None else labs)
            self.held = name
        return self.eng


@pytest.fixture(scope="module")
def mid(fcmod, case):
    with fcmod.Engine(seed=SEED) as eng:
        eng.load_graph(case["n"], case["u"], case["v"])
        assert eng.m == len(case["u"]) and not np.array_equal(eng.node_map(), np.arange(case["n"]))
        yield Mid(eng, case)


def check(got, ref):
    """the dict of Engine.cluster_match against a reference of match_mid.reference's shape"""
    ids, size, inter, csize, over = (ref[f] for f in ("ids", "size", "inter", "csize", "over"))
    assert sorted(got) == sorted(INFO + DERIVED + ("ids", "size", "inter", "csize"))
    assert got["ids"].dtype == np.int32 and np.array_equal(got["ids"], ids)
    assert got["size"].dtype == np.int64 and np.array_equal(got["size"], size)
    for f, exp in (("inter", inter), ("csize", csize)):
        assert got[f].dtype == np.int32 and got[f].shape == exp.shape, f
        wrong = np.argwhere(got[f] != exp)
        assert not len(wrong), (f, len(wrong), wrong[:5].tolist(), [int(got[f][r, k]) for r, k in wrong[:5]],
                                [int(exp[r, k]) for r, k in wrong[:5]])
    assert got["k"] == len(ids) and got["max_size"] == size.max() and got["singletons"] == (size == 1).sum()
    assert got["n_r"] == len(inter) and got["inter_total"] == int(inter.sum(dtype=np.int64))
    assert got["perfect"] == ((inter == size[None, :]) & (csize == size[None, :])).sum()
    assert np.all(inter >= 1) and np.all(inter <= np.minimum(size[None, :], csize))
    for f, exp in mm.summary(inter, size, csize).items():
        assert got[f].dtype == exp.dtype and got[f].shape == exp.shape and np.all(got[f] == exp), f
    assert got["slow_members"] == int((over * size[None, :]).sum())
    return got


# ------------------------------------------------------------------ 1. the natural partitions
@pytest.mark.parametrize("n_r", [am.N_R, am.N_R2])
def test_part(mid, case, refs, n_r):
    """P itself: two trips of the match grid, of k_cm_total and k_cm_scatter; C and A in the fallback
    by length, B exactly at the cap and in registers; with 70 labelings bank 1 of k = 269,747"""
    ref = mm.rows_of(refs["part"], n_r)
    got = check(mid.use("labs%d" % n_r).cluster_match(case["part"]), ref)
    assert got["k"] > 262_144 and 0 < got["slow_members"] < n_r * case["n"]
    ids, over = ref["ids"], ref["over"]
    c, a, b = np.searchsorted(ids, case["ids_cab"])
    assert over[:, [c, a]].all() and not over[:, b].any() and ref["size"][b] == am.caps()["LCAP"]


@pytest.mark.parametrize("n_r", [am.N_R, am.N_R2])
def test_coarse(mid, case, refs, n_r):
    """18 clusters, the giant's 20 or 70 lanes through two or seven chunks of the fallback"""
    ref = mm.rows_of(refs["coarse"], n_r)
    got = check(mid.use("labs%d" % n_r).cluster_match(mm.partition(case, "coarse")), ref)
    cap, step = mm.chunk_windows(case["n"], am.caps()["CHUNK"])
    assert got["k"] == 18 and got["slow_members"] > step
    # its own row (2) and the other coarse rows of the clean family find the giant again
    giant = int(np.argmax(ref["size"]))
    assert got["inter"][2, giant] == got["csize"][2, giant] == ref["size"][giant] == got["max_size"]


def test_fine(mid, case, refs):
    """358,537 clusters, none longer than the cap and none with a ninth label: registers alone"""
    got = check(mid.use("labs20").cluster_match(mm.partition(case, "fine")), refs["fine"])
    assert got["slow_members"] == 0 and got["k"] > 262_144
    assert np.array_equal(got["inter"][3], got["size"]) and np.array_equal(got["csize"][3], got["size"])   # its own row


# ------------------------------------------------------------------ 2. `other` at mid size
def test_other(mid, case, refs):
    """one row and ldT = 1: the fine row against coarse (row 3 of coarse's reference: the giant in
    the fallback) and the coarse row against P (row 2 of P's)"""
    eng = mid.use("labs20")
    before = eng.get_labels(am.N_R)
    a = check(eng.cluster_match(mm.partition(case, "coarse"), other=case["labs70"][3]), mm.rows_of(refs["coarse"], slice(3, 4)))
    b = check(eng.cluster_match(case["part"], other=case["labs70"][2]), mm.rows_of(refs["part"], slice(2, 3)))
    assert a["n_r"] == b["n_r"] == 1 and a["slow_members"] >= a["max_size"] > 262_144 and b["slow_members"] > 0
    assert eng.replica_info()[0] == am.N_R and np.array_equal(eng.get_labels(am.N_R), before)
    check(eng.cluster_match(mm.partition(case, "coarse")), mm.rows_of(refs["coarse"], am.N_R))   # and the labelings still answer


# ------------------------------------------------------------------ 3. cross products past 2^32
@functools.lru_cache(maxsize=None)
def crafted(name, a_low):
    """(part, lab, reference) of a crafted case"""
    part, lab = mm.CRAFTED[name][0](a_low)
    return part, lab, mm.reference(lab, part)


def check_crafted(eng, name, a_low, register):
    part, lab, ref = crafted(name, a_low)
    if register:
        ref = dict(ref, over=np.zeros_like(ref["over"]))
    got = check(eng.cluster_match(part), ref)
    assert got["slow_members"] == (0 if register else mm.CRAFTED[name][1][0])
    assert np.array_equal(check(eng.cluster_match(part, other=lab), ref)["inter"], got["inter"])
    return got


@pytest.mark.parametrize("a_low", ORDERS)
def test_wide_in_the_fallback(mid, a_low):
    """cluster 0 (100,000 members) is longer than the default cap: k_cm_fold's compare decides"""
    got = check_crafted(mid.use(("wide", a_low), crafted("wide", a_low)[1][None, :]), "wide", a_low, False)
    assert (got["size"][0], got["inter"][0, 0], got["csize"][0, 0]) == (100_000, 50_000, 50_000)


@pytest.mark.parametrize("a_low", ORDERS)
def test_near_tie_wide_in_the_fallback(mid, a_low):
    got = check_crafted(mid.use(("near_tie_wide", a_low), crafted("near_tie_wide", a_low)[1][None, :]),
                        "near_tie_wide", a_low, False)
    assert (got["size"][0], got["inter"][0, 0], got["csize"][0, 0]) == (200_001, 100_000, 199_998)


@pytest.fixture(scope="module")
def ring(fcmod):
    """a fresh engine on a ring of N nodes whose list cap holds the crafted clusters: the variable
    is read when the engine is created"""
    n = am.N
    with pytest.MonkeyPatch.context() as monkeypatch:
        monkeypatch.setenv("FC_SCORE_LCAP", str(mm.REGISTER_LCAP))
        with fcmod.Engine(seed=SEED) as eng:
            eng.load_graph(n, np.arange(n, dtype=np.int32), ((np.arange(n) + 1) % n).astype(np.int32))
            yield eng


@pytest.mark.parametrize("a_low", ORDERS)
@pytest.mark.parametrize("name", sorted(mm.CRAFTED))
def test_crafted_on_the_register_path(mid, ring, name, a_low):
    """k_cm_match's own compare on products past 2^32, and the same tables as the fallback's"""
    lab = crafted(name, a_low)[1][None, :]
    ring.set_labels(lab)
    got = check_crafted(ring, name, a_low, True)
    assert (got["size"][0], got["inter"][0, 0], got["csize"][0, 0]) == mm.CRAFTED[name][1]
    slow = mid.use((name, a_low), lab).cluster_match(crafted(name, a_low)[0])
    assert slow["slow_members"] == got["size"][0] and got["slow_members"] == 0
    for f in ("ids", "size", "inter", "csize"):
        assert np.array_equal(got[f], slow[f]), f
