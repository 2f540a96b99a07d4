"""The mid-size case of the cluster merges (tests/merge_mid.py), without a GPU: its inputs pass the
launch clamps of merge.h's kernels and FC_SCORE_LCAP on the list side (so
tests/test_gpu_merge_mid.py is not empty), every cap read from the csrc headers by name, and its
sparse references equal the dense ones where those still run."""
import numpy as np
import pytest

from tests import analysis_mid as am
from tests import consensus_ref as cr
from tests import golden_io
from tests import merge_mid as mm
from tests import merge_ref as gr

RELATION = {">": lambda a, b: a > b, "==": lambda a, b: a == b, "<=": lambda a, b: a <= b}


@pytest.fixture(scope="module")
def lfr():
    return golden_io.load("lfr1k_louvain_np20")


def test_clamps_are_read_from_the_sources():
    assert am.clamp("merge.h", "k_mc_lookup") > 0
    # merge.h's fallback emits its keys through cluster.h's chunk driver, so the clamp that caps()
    # reads from cluster.h is the one this call runs under: merge.h may hold no launch of its own
    assert "cell_chunks<" in am._src("merge.h") and "k_cc_emit<<<" not in am._src("merge.h")
    assert am._src("cluster.h").count("k_cc_emit<<<") == 1 and am.caps()["k_cc_emit"] > 0
    with pytest.raises(AssertionError):
        am.clamp("merge.h", "k_mc_no_such_kernel")


def test_every_cap_is_reached():
    got = mm.reached(am.case())
    assert len(got) >= 9
    missed = {name: x for name, x in got.items() if not RELATION[x[1]](x[0], x[2])}
    assert not missed, missed


def test_pair_list_of_the_case():
    c = am.case()
    g, a, b = mm.pairs()
    assert c["n"] == 400_003 and len(c["u"]) == 797_200 and len(np.unique(c["part"])) == 269_747
    assert len(a) == len(b) == g["npairs"] + 6 * mm.LONG_COPIES
    assert (g["a"] < g["b"]).all() and int(g["edges"].sum()) == int((c["part"][c["u"]] != c["part"][c["v"]]).sum())
    order = np.lexsort((g["b"], g["a"]))
    assert np.array_equal(order, np.arange(g["npairs"]))                  # ascending by (a, b)


def test_sparse_references_equal_the_dense_ones(lfr):
    u, v = cr.canonical_edges(lfr.edges_file[:, 0], lfr.edges_file[:, 1])
    labs = lfr.cd_batches[0]
    rng = np.random.default_rng(5)
    for part in (labs[0], cr.partition(lfr.N, u, v, 1.0, labels=labs)["labels"], rng.permutation(lfr.N),
                 rng.integers(0, 40, lfr.N) * 3 + 1):
        ref = gr.community_graph(lfr.N, u, v, None, part)
        got = mm.community_graph(lfr.N, u, v, part)
        assert all(np.array_equal(got[f], ref[f]) for f in ("a", "b", "weight", "edges")) and got["npairs"] == ref["npairs"]
        ids = np.unique(part)
        a = np.r_[ref["a"], ref["b"][:50], ids[:20], 999, ids[0]]
        b = np.r_[ref["b"], ref["a"][:50], ids[:20], ids[0], 998]
        exp = gr.cross(labs, part, a, b) * (np.isin(a, part) & np.isin(b, part))
        assert np.array_equal(mm.sparse_cross(am.cluster_cells(labs, part), a, b), exp) and exp.any()
