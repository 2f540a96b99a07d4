"""The scoring reference (tests/score_ref.py) pinned on recorded labelings against
tests/dist_gates.nmi, sklearn's adjusted_rand_score and the oracle's modularity; and the
scoring surface of the header, the ctypes binding and fast_consensus() (no GPU needed)."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest

from tests import dist_gates, golden_io, score_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["lfr1k_louvain_np20", "lfr1k_lpm_np20", "karate_louvain_np50"]
SCORE_FUNCS = ("fc_score_set_reference", "fc_score_partitions", "fc_score_pairs")


@pytest.mark.parametrize("name", CASES)
def test_pair_reference_matches_nmi_and_sklearn_ari(name):
    from sklearn.metrics import adjusted_rand_score
    labs = golden_io.load(name).cd_batches[0][:12]
    for a, b in itertools.combinations_with_replacement(range(len(labs)), 2):
        got = score_ref.pair(labs[a], labs[b])
        assert abs(got["nmi"] - dist_gates.nmi(labs[a], labs[b])) <= 1e-14, (a, b)
        assert abs(got["ari"] - adjusted_rand_score(labs[a], labs[b])) <= 1e-14, (a, b)
        back = score_ref.pair(labs[b], labs[a])
        assert (got["cells"], got["sum_sq"]) == (back["cells"], back["sum_sq"])


@pytest.mark.parametrize("name", CASES)
def test_modularity_reference_matches_oracle(name):
    from oracle import oracle as orc
    case = golden_io.load(name)
    e = case.edges_file
    g = orc.EdgeGraph.from_lines(case.N, e)
    for lab in case.cd_batches[0]:
        got = score_ref.part(lab, g.u, g.v)
        # the oracle adds k <= N rounded squares
        assert abs(got["modularity"] - orc.modularity(g, lab)) <= case.N * 2.0 ** -53
        assert got["k"] == len(set(lab.tolist())) and got["sum_sq"] >= case.N


def test_single_community_and_singletons():
    one, single = np.zeros(50, np.int64), np.arange(50)
    assert score_ref.pair(one, one)["nmi"] == 1.0 and score_ref.pair(one, one)["ari"] == 1.0
    assert score_ref.pair(single, single)["nmi"] == 1.0 and score_ref.pair(single, single)["ari"] == 1.0
    assert score_ref.pair(one, single)["nmi"] == 0.0 and score_ref.pair(one, single)["ari"] == 0.0
    assert score_ref.part(one)["entropy"] == 0.0


def test_header_and_binding_declare_the_scoring_entry_points():
    from fastconsensus_amd import _lib
    src = open(os.path.join(ROOT, "include", "fastconsensus_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fc_[a-z_]+)\s*\(", src))
    for fn in SCORE_FUNCS:
        assert fn in declared, fn
        assert fn in _lib.SYMBOLS, fn
    for name in ("FC_SCORE_REF", "FC_SCORE_GRAPH_INPUT", "FC_SCORE_GRAPH_WORKING", "fc_part_score", "fc_pair_score"):
        assert re.search(r"\b%s\b" % name, src), name
    assert _lib.FC_SCORE_REF == -1 and _lib.SCORE_GRAPHS == {"input": 0, "working": 1}
    # the ctypes mirrors follow the header's field order
    for struct, cname in ((_lib.PartScore, "fc_part_score"), (_lib.PairScore, "fc_pair_score")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        fields = [f.strip() for decl in re.findall(r"(?:u?int\d+_t|double)\s+([^;]+);", body) for f in decl.split(",")]
        assert fields == [k for k, _ in struct._fields_], cname


def test_fast_consensus_signature_has_keyword_only_scores_and_truth():
    import fastconsensus_amd as fc
    sig = inspect.signature(fc.fast_consensus).parameters
    for name, default in (("scores", False), ("truth", None)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY
        assert sig[name].default is default
    for m in ("set_reference", "score_partitions", "score_pairs", "nmi_matrix"):
        assert callable(getattr(fc.Engine, m))
