"""fc_community_graph and fc_cluster_coassoc on the device at mid size: the case of
tests/analysis_mid.py (N = 400,003, 797,200 edges, a partition of 269,747 clusters, 20 and 70
labelings) with the pair list of tests/merge_mid.py, every integer against the sparse references.
Here the count kernel's grid makes a second trip, the clusters C and A list past the default length
cap (so their partners go through the fallback, whose lookup kernel passes its clamp), B lists at
exactly the cap and walks under A -- tests/test_merge_mid_cases.py checks, without a GPU, that the
inputs do reach each of these.  More than 2^31 pairs or members are not reached here."""
import numpy as np
import pytest

from tests import analysis_mid as am
from tests import merge_mid as mm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 7                                    # an engine seed whose node map is not the identity


@pytest.fixture(scope="module")
def fcmod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    return fc


@pytest.fixture(scope="module")
def case(fcmod):
    c = am.case()
    c["cc20"], c["cc70"], mm.pairs()        # the references here, so that no test's time holds one
    yield c
    mm.pairs.cache_clear()
    am.case.cache_clear()                   # about 1 GB of host arrays


@pytest.fixture(scope="module")
def eng(fcmod, case):
    with fcmod.Engine(seed=SEED) as e:
        e.load_graph(case["n"], case["u"], case["v"])
        assert e.m == len(case["u"]) and not np.array_equal(e.node_map(), np.arange(case["n"]))
        yield e


def test_community_graph(eng, case):
    ref = mm.pairs()[0]
    got = eng.community_graph(case["part"])                  # before any labeling is installed
    assert got["npairs"] == ref["npairs"] > (1 << 16)
    for f in ("a", "b", "weight", "edges"):
        wrong = np.flatnonzero(got[f] != ref[f])
        assert got[f].dtype == ref[f].dtype and not len(wrong), (f, len(wrong), wrong[:5])
    q = eng.community_quality(case["part"], split=False, nodes=False)
    assert int(got["weight"].sum()) == q["cut_weight"]


def expected(case, n_r, a, b):
    """x and the info fields from the sparse cells of the n_r-labeling case"""
    cc = case["cc%d" % n_r]
    ids, size = cc["ids"], cc["size"]
    lst, wlk = mm.sides(lambda x: size[np.searchsorted(ids, x)], a, b)
    walk = size[np.searchsorted(ids, wlk)]
    flagged = cc["over"].sum(0)[np.searchsorted(ids, lst)]
    return mm.sparse_cross(cc["cells"], a, b), len(np.unique(lst)), int(walk.sum()), int((walk * flagged).sum())


@pytest.mark.parametrize("n_r", [20, 70])
def test_cluster_coassoc(eng, case, n_r):
    g, a, b = mm.pairs()
    if n_r == 70:                                            # the long pairs and a part of the graph's
        keep = np.r_[np.arange(mm.SUBSET_70), np.arange(g["npairs"], len(a))]
        a, b = a[keep], b[keep]
    x, listed, walked, slow = expected(case, n_r, a, b)
    eng.set_labels(case["labs%d" % n_r])
    got = eng.cluster_coassoc(case["part"], a, b)
    wrong = np.flatnonzero(got["x"] != x)
    assert not len(wrong), (len(wrong), wrong[:5], a[wrong[:5]], b[wrong[:5]], got["x"][wrong[:5]], x[wrong[:5]])
    assert (got["k"], got["n_r"]) == (len(case["cc20"]["ids"]), n_r)
    assert (got["listed_clusters"], got["walked_members"], got["slow_lookups"]) == (listed, walked, slow)
    assert slow > 0 and x.max() > 0
    # the diagonal of the long clusters is the cluster consensus' pair sum
    cab = case["ids_cab"].astype(np.int32)
    cc = case["cc%d" % n_r]
    diag = eng.cluster_coassoc(case["part"], cab, cab)["x"]
    assert np.array_equal(diag, cc["pairs"][np.searchsorted(cc["ids"], cab)]) and diag.max() > (1 << 32)
