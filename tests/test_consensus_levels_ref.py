"""The consensus-hierarchy reference (tests/consensus_levels_ref.py) against the per-threshold
reference (tests/consensus_ref.py) on the recorded labelings, and the host side of the feature:
level_of / theta_of / cut_tree, the header, the binding and the command line (no GPU needed)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fastconsensus_amd as fc
from fastconsensus_amd import level_of, theta_of, cut_tree
from tests import consensus_levels_ref as lref
from tests import consensus_ref as cref
from tests import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["lfr1k_louvain_np20", "karate_louvain_np50", "lfr1k_mu055_lpm_np20", "lfr1k_lpm_np20"]
_cache = {}


def first_batch(name):
    """(case, u, v, sup, birth, up, records) of the fixture's first CD batch, computed once"""
    if name not in _cache:
        case = golden_io.load(name)
        u, v = cref.canonical_edges(case.edges_file[:, 0], case.edges_file[:, 1])
        sup = cref.support(case.cd_batches[0], u, v)
        birth, up = lref.tree(case.N, u, v, sup, case.n_p)
        rec = lref.level_records(case.N, u, v, sup, case.n_p, birth=birth, up=up)
        _cache[name] = (case, u, v, sup, birth, up, rec)
    return _cache[name]


@pytest.mark.parametrize("name", CASES)
def test_every_level_is_the_consensus_partition_at_its_threshold(name):
    case, u, v, sup, birth, up, rec = first_batch(name)
    nt = case.n_p
    assert np.all(birth[up[birth >= 0]] < birth[birth >= 0])
    assert np.array_equal(up[birth < 0], np.flatnonzero(birth < 0))
    j = lref.join_levels(u, v, birth, up)
    assert np.all(j >= sup)
    for s in range(nt + 1):
        exp = cref.partition(case.N, u, v, theta_of(s, nt), sup=sup, n_total=nt)
        assert exp["kept_edges"] == int((sup >= s).sum()), s
        lab = lref.cut(birth, up, s)
        assert np.array_equal(lab, exp["labels"]), s
        assert np.array_equal(cut_tree(birth, up, s), lab), s
        assert int((j >= s).sum()) == int((lab[u] == lab[v]).sum()), s
        r = rec[s]
        assert (r["k"], r["max_size"], r["singletons"]) == (exp["k"], exp["max_size"], exp["singletons"]), s
        assert r["bucket_edges"] == int(exp["support_hist"][s]) and r["in_weight"] == int((lab[u] == lab[v]).sum())
        if r["bucket_edges"] == 0 and s < nt:
            assert {k: x for k, x in r.items() if k != "bucket_edges"} == \
                {k: x for k, x in rec[s + 1].items() if k != "bucket_edges"}, s


def test_recorded_facts():
    _, _, _, _, _, _, rec = first_batch("lfr1k_louvain_np20")
    assert sum(r["bucket_edges"] > 0 for r in rec) == 21
    assert (rec[0]["k"], rec[20]["k"]) == (1, 139)
    assert rec[0]["modularity"] == 0.0 and round(rec[20]["modularity"], 3) == 0.306
    assert lref.best_level(rec) == 12 and round(rec[12]["modularity"], 3) == 0.344
    _, _, _, _, _, _, rec = first_batch("karate_louvain_np50")
    assert sum(r["bucket_edges"] > 0 for r in rec) == 16
    keys = [r["key"] for r in rec]
    assert [s for s in range(51) if keys[s] == max(keys)] == list(range(26, 32))      # a plateau: one partition
    assert lref.best_level(rec) == 31
    _, _, _, _, _, _, rec = first_batch("lfr1k_lpm_np20")
    assert sum(r["bucket_edges"] > 0 for r in rec) == 1                              # degenerate: one level


def test_modularity_restates_the_score_reference_within_an_ulp():
    from tests import score_ref
    case, u, v, sup, birth, up, rec = first_batch("lfr1k_louvain_np20")
    for s in (0, 7, 12, 20):
        exact = score_ref.part(lref.cut(birth, up, s), u, v)
        assert (rec[s]["in_weight"], rec[s]["tot_sq"]) == (exact["in_weight"], exact["tot_sq"])
        assert abs(rec[s]["modularity"] - exact["modularity"]) <= 2.0 ** -52


def test_level_and_theta_round_trip():
    nt = np.repeat(np.arange(1, 2049), np.arange(2, 2050))
    first = np.cumsum(np.arange(2, 2050)) - np.arange(2, 2050)
    s = np.arange(len(nt)) - np.repeat(first, np.arange(2, 2050))
    assert s.min() == 0 and np.array_equal(s[first], np.zeros(2048, np.int64)) and np.all(s <= nt)
    assert int((s == nt).sum()) == 2048
    theta = theta_of(s, nt)
    assert theta.min() == 0.0 and theta.max() < 1.0
    assert np.array_equal(level_of(theta, nt), s)
    for n_total in (1, 7, 50, 2048):
        for lv in range(n_total + 1):
            assert lref.level_of(lref.theta_of(lv, n_total), n_total) == lv
            assert theta_of(lv, n_total) == lref.theta_of(lv, n_total)
            assert level_of(theta_of(lv, n_total), n_total) == lv


@pytest.mark.parametrize("n_total,theta,level", [(10, 0.7, 7), (20, 0.8, 16), (25, 0.28, 8)])
def test_pinned_products_map_to_levels_like_the_keep_rule(n_total, theta, level):
    assert level_of(theta, n_total) == lref.level_of(theta, n_total) == level
    sup = np.arange(n_total + 1)
    keep, _ = cref.kept(sup, n_total, theta)
    assert np.array_equal(keep, sup >= level)


def test_cut_tree_on_a_deep_chain():
    n = 2049                                            # the ladder: birth[t] = up[t] = t - 1
    birth = np.arange(-1, n - 1).astype(np.int32)
    up = np.maximum(np.arange(n) - 1, 0).astype(np.int32)
    for s in (0, 1, 1000, 2047, 2048):
        exp = np.minimum(np.arange(n), s)               # nodes s.. are one community, the rest alone
        assert np.array_equal(cut_tree(birth, up, s), exp), s
        assert np.array_equal(lref.cut(birth, up, s), exp), s


def test_header_and_binding_declare_the_hierarchy():
    from fastconsensus_amd import _lib, core
    src = open(os.path.join(ROOT, "include", "fastconsensus_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fc_[a-z_]+)\s*\(", src))
    for fn in ("fc_consensus_levels", "fc_consensus_cut", "fc_consensus_levels_timing"):
        assert fn in declared and fn in _lib.SYMBOLS, fn
    body = re.search(r"typedef struct fc_level_score \{(.*?)\} fc_level_score;", src, flags=re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"(?:u?int\d+_t|double)\s+([^;]+);", body) for f in decl.split(",")]
    assert fields == [k for k, _ in _lib.LevelScore._fields_]
    assert fields == ["bucket_edges", "k", "max_size", "singletons", "in_weight", "tot_sq_lo", "tot_sq_hi", "modularity"]
    assert ctypes.sizeof(_lib.LevelScore) == core.LEVEL_DTYPE.itemsize == 64


def test_python_surface(tmp_path):
    from fastconsensus_amd import cli
    for m in ("consensus_levels", "consensus_cut", "consensus_levels_timing"):
        assert callable(getattr(fc.Engine, m))
    sig = inspect.signature(fc.Engine.consensus_levels).parameters
    assert [sig[k].default for k in ("graph", "dev_support", "n_total")] == ["input", None, None]
    with pytest.raises(ValueError):
        fc.fast_consensus(fc.IdGraph(np.arange(3), [0], [1]), "louvain", consensus="worst")
    p = cli.build_parser()
    assert p.parse_args(["-f", "x"]).consensus_levels is False
    assert p.parse_args(["-f", "x", "--consensus-levels"]).consensus_levels is True
    args = p.parse_args(["-f", "x", "-t", "0.2", "-np", "2", "--consensus-levels"])
    levels = np.zeros(3, fc.core.LEVEL_DTYPE)
    levels["k"] = [1, 2, 4]
    levels["bucket_edges"] = [1, 0, 2]
    levels["modularity"] = [0.0, 0.25, 0.125]
    cli.write_levels(args, np.array([10, 4, 7, 5]), levels, np.array([0, 1, 0, 1], np.int32), root=str(tmp_path))
    d = tmp_path / "consensus_t0.2_d0.02_np2"
    rows = (d / "levels.tsv").read_text().splitlines()
    assert len(rows) == 3 and rows[0].split("\t") == ["0", "0.0", "1", "1", "0", "0", "0.0"]
    assert rows[1].split("\t") == ["1", "0.25", "0", "2", "0", "0", "0.25"]
    assert (d / "partition").read_text() == "10 7\n4 5\n"
