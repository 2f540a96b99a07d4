"""The mid-size case of tests/quality_mid.py, without a GPU: its partitions reach what they were
built for (so the quality tests of tests/test_gpu_analysis_mid.py are not empty), and the moved
partition is what it says."""
import numpy as np

from tests import analysis_mid as am
from tests import quality_mid as qm
from tests.test_analysis_mid_cases import RELATION


def test_every_condition_is_reached():
    got = qm.reached(am.case())
    for name, x in got.items():
        print("%s: %d %s %d" % ((name,) + x))
    assert len(got) >= 17
    missed = {name: x for name, x in got.items() if not RELATION[x[1]](x[0], x[2])}
    assert not missed, missed


def test_moved_nodes_have_no_edge_into_their_new_cluster():
    c = am.case()
    moved, anchor, nodes = qm.moved_partition(c)
    part, u, v = c["part"], c["u"], c["v"]
    assert (part[nodes] == c["ids_cab"][0]).all() and (moved[nodes] == anchor).all()
    assert (moved != part).sum() == len(nodes) == len(np.unique(nodes))
    is_moved = np.zeros(c["n"], bool)
    is_moved[nodes] = True
    assert not ((is_moved[u] & (part[v] == anchor)) | (is_moved[v] & (part[u] == anchor))).any()
    # so inside the anchor cluster a moved node is joined to other moved nodes at the most
    _, ref = qm.case()["moved"]
    at = int(np.searchsorted(ref["ids"], anchor))
    pairs = int((is_moved[u] & is_moved[v]).sum())
    assert ref["size"][at] == am.ANCHOR_SIZE + len(nodes)
    before = qm.case()["part"][1]
    own = int(before["components"][np.searchsorted(before["ids"], anchor)])      # the anchor's own parts
    assert own + len(nodes) - pairs <= ref["components"][at] <= own + len(nodes)


def test_coarse_split_is_the_split_of_the_coarse_row():
    q = qm.case()
    split, ref = q["coarse_split"]
    assert np.array_equal(split, q["coarse"][1]["split"]) and np.array_equal(ref["split"], split)
    assert ref["k"] == q["coarse"][1]["parts"] and ref["max_size"] == q["coarse"][1]["largest_component"].max()


def test_wave_clusters():
    order = np.arange(200)[::-1].copy()
    labels = np.r_[np.zeros(8, np.int64), np.arange(64), np.full(64, 5), np.arange(64) // 2]
    # waves of the reversed order: nodes 199..136 (32 halves), 135..72 (all 5), 71..8 (0..63); the rest is cut
    assert qm.wave_clusters(order, labels).tolist() == [32, 1, 64]
