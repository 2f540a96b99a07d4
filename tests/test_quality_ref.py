"""The community-quality reference (tests/quality_ref.py) held to hand-computed values, to
tests/score_ref.py and to its own identities; the module-level derivations of core.py; and the
surface of the header and the binding (no GPU needed)."""
import math
import os
import re

import numpy as np
import pytest

from tests import golden_io, score_ref
from tests import quality_ref as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def identities(n, u, v, w, labels, q):
    w = np.ones(len(u), np.int64) if w is None else np.asarray(w, np.int64)
    kdeg = np.zeros(n, np.int64)
    np.add.at(kdeg, u, w)
    np.add.at(kdeg, v, w)
    assert int(q["volume"].sum()) == q["total_degree"] == int(kdeg.sum())
    assert int(q["cut"].sum()) == 2 * q["cut_weight"]
    assert q["in_weight_total"] + q["cut_weight"] == int(w.sum())
    assert np.array_equal(q["node_in"] + q["node_out"], kdeg)
    # split refines P: every part lies in one cluster, and there are `parts` of them
    pairs = np.unique(np.stack([q["split"], np.asarray(labels)], 1), axis=0)
    assert len(pairs) == q["parts"] == int(q["components"].sum()) == int(q["split"].max()) + 1
    assert np.array_equal(q["largest_component"] <= q["size"], np.ones(q["k"], bool))
    again = qr.quality(n, u, v, w, q["split"])
    assert np.all(again["components"] == 1) and np.array_equal(again["split"], q["split"])
    assert again["disconnected"] == 0 and again["k"] == q["parts"]


def test_path_of_five():
    u, v = np.array([0, 1, 2, 3]), np.array([1, 2, 3, 4])
    q = qr.quality(5, u, v, None, [3, 3, 7, 7, 3])             # clusters {0,1,4} (id 3) and {2,3} (id 7)
    assert q["ids"].tolist() == [3, 7] and q["size"].tolist() == [3, 2]
    assert q["components"].tolist() == [2, 1] and q["largest_component"].tolist() == [2, 2]
    assert q["split"].tolist() == [0, 0, 1, 1, 2]
    assert q["volume"].tolist() == [4, 4] and q["in_weight"].tolist() == [1, 1] and q["cut"].tolist() == [2, 2]
    assert q["in_edges"].tolist() == [1, 1] and q["min_in_degree"].tolist() == [0, 1]
    assert q["node_in"].tolist() == [1, 1, 1, 1, 0] and q["node_out"].tolist() == [0, 1, 1, 1, 1]
    assert (q["k"], q["max_size"], q["singletons"], q["parts"], q["disconnected"]) == (2, 3, 0, 3, 1)
    assert (q["in_weight_total"], q["cut_weight"], q["total_degree"]) == (2, 2, 8)
    identities(5, u, v, None, [3, 3, 7, 7, 3], q)
    # ids in the other order: the records follow the ids, the split partition does not change
    back = qr.quality(5, u, v, None, [7, 7, 3, 3, 7])
    assert back["components"].tolist() == [1, 2] and back["split"].tolist() == [0, 0, 1, 1, 2]


def test_weights_and_weight_zero_edges():
    # a triangle 0-1-2 with weights 3, 0, 2 and a pendant 2-3 of weight 5; one cluster {0,1,2}, one {3}
    u, v, w = np.array([0, 1, 0, 2]), np.array([1, 2, 2, 3]), np.array([3, 0, 2, 5])
    q = qr.quality(4, u, v, w, [0, 0, 0, 1])
    assert q["in_weight"].tolist() == [5, 0] and q["in_edges"].tolist() == [3, 0]     # the weight-0 edge counts
    assert q["volume"].tolist() == [15, 5] and q["cut"].tolist() == [5, 5]
    assert q["min_in_degree"].tolist() == [2, 0] and q["components"].tolist() == [1, 1]
    # the weight-0 edge connects: without edge 0-1 of weight 3, nodes 1 and 2 hang together by it alone
    q2 = qr.quality(4, u[1:], v[1:], w[1:], [0, 0, 0, 1])
    assert q2["components"].tolist() == [1, 1]
    q3 = qr.quality(4, u[2:], v[2:], w[2:], [0, 0, 0, 1])
    assert q3["components"].tolist() == [2, 1] and q3["split"].tolist() == [0, 1, 0, 2]
    identities(4, u, v, w, [0, 0, 0, 1], q)


@pytest.mark.parametrize("name", ["karate_louvain_np50", "lfr1k_louvain_np20", "lfr1k_lpm_np20"])
def test_recorded_partitions_against_score_ref(name):
    case = golden_io.load(name)
    e = case.edges_file
    u, v = e[:, 0].astype(np.int64), e[:, 1].astype(np.int64)
    for lab in (case.cd_batches[0][0], case.cd_batches[-1][-1], np.zeros(case.N, np.int64), np.arange(case.N)):
        q = qr.quality(case.N, u, v, None, lab)
        sc = score_ref.part(lab, u, v)
        assert q["in_weight_total"] == sc["in_weight"] and q["k"] == sc["k"] and q["max_size"] == sc["max_size"]
        assert sum(int(x) ** 2 for x in q["volume"]) == sc["tot_sq"]
        identities(case.N, u, v, None, lab, q)


def test_derivations():
    import fastconsensus_amd as fc
    case = golden_io.load("karate_louvain_np50")
    e = case.edges_file
    u, v = e[:, 0].astype(np.int64), e[:, 1].astype(np.int64)
    lab = case.cd_batches[0][0]
    q = qr.quality(case.N, u, v, None, lab)
    w2 = q["total_degree"]
    share = fc.modularity_share(q["in_weight"], q["volume"], w2)
    # k <= n terms, each rounded a few times, against the exact rational rounded once
    assert abs(float(share.sum()) - score_ref.part(lab, u, v)["modularity"]) <= 8 * q["k"] * 2.0 ** -53
    cond = fc.conductance(q["cut"], q["volume"], w2)
    for c, vol, x in zip(q["cut"].tolist(), q["volume"].tolist(), cond.tolist()):
        assert x == c / min(vol, w2 - vol)
    assert math.isnan(fc.conductance([0], [w2], w2)[0]) and math.isnan(fc.conductance([0], [0], w2)[0])
    assert fc.density([3, 0, 1], [3, 1, 4]).tolist()[::2] == [1.0, 1 / 6] and math.isnan(fc.density([0], [1])[0])
    mix = fc.mixing([3, 0, 0], [1, 2, 0])
    assert mix[:2].tolist() == [0.25, 1.0] and math.isnan(mix[2])
    assert fc.modularity_share([0], [0], 0).tolist() == [0.0]


def test_header_and_binding_declare_the_quality_call():
    import ctypes
    from fastconsensus_amd import _lib
    src = open(os.path.join(ROOT, "include", "fastconsensus_amd.h")).read()
    for fn in ("fc_community_quality", "fc_community_quality_timing"):
        assert fn in _lib.SYMBOLS and re.search(r"\bint %s\(" % fn, src)
    for struct, fields, py in (("fc_community_record", _lib.COMMUNITY_RECORD.names, None),
                               ("fc_quality_info", [k for k, _ in _lib.QualityInfo._fields_], _lib.QualityInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == list(fields)
        assert "int64_t" in body and "int32_t" not in body
        if py is not None:
            assert ctypes.sizeof(py) == 8 * len(fields)
    assert _lib.COMMUNITY_RECORD.itemsize == 64
    # the reuse paragraph at the top of the header names the call
    assert "fc_community_quality" in src[:src.index("#ifndef FASTCONSENSUS_AMD_H")]
