"""tests/coassoc_ref.py against triple Python loops, pac / cdf on hand-made histograms, and the
co-association surface of the package (symbols, Engine methods, the fast_consensus keyword).
CPU only."""
import inspect

import numpy as np

from tests import coassoc_ref as car
from tests import golden_io


def loops_matrix(labs, a, b):
    out = np.zeros((len(a), len(b)), np.int32)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            for r in range(len(labs)):
                if labs[r][x] == labs[r][y]:
                    out[i, j] += 1
    return out


def test_reference_against_loops():
    case = golden_io.load("karate_louvain_np50")
    labs = case.cd_batches[0]                 # the first batch: the counts spread over 0..50
    assert labs.shape == (50, 34)
    nodes = list(range(case.N))
    full = loops_matrix(labs.tolist(), nodes, nodes)
    got = car.matrix(labs, nodes)
    assert got.dtype == np.int32 and np.array_equal(got, full)
    assert np.array_equal(np.diag(full), np.full(34, 50)) and np.array_equal(full, full.T)
    assert 0 < (full == 0).sum() and ((full > 0) & (full < 50)).sum() > 0      # the counts spread
    a, b = [33, 0, 7, 7, 12], [5, 33, 1]
    assert np.array_equal(car.matrix(labs, a, b), full[np.ix_(a, b)])
    p = np.array([(0, 1), (33, 2), (4, 4), (20, 3)])
    assert np.array_equal(car.pairs(labs, p), full[p[:, 0], p[:, 1]])
    h = np.zeros(51, np.int64)
    for i in range(34):
        for j in range(i + 1, 34):
            h[full[i, j]] += 1
    got = car.hist(labs, nodes)
    assert got.dtype == np.int64 and np.array_equal(got, h) and h.sum() == 34 * 33 // 2
    dup = [3, 9, 3]                      # positions (0, 2) hold one node: that pair counts at n_r
    hd = car.hist(labs, dup)
    assert hd.sum() == 3 and hd[50] >= 1
    assert np.array_equal(car.hist(labs, []), np.zeros(51, np.int64))
    assert np.array_equal(car.hist(labs, [5]), np.zeros(51, np.int64))


def test_pac_and_cdf_by_hand():
    import fastconsensus_amd as fc
    n = 20
    ends = np.zeros(n + 1, np.int64)
    ends[0], ends[n] = 70, 30
    mid = np.zeros(n + 1, np.int64)
    mid[n // 2] = 11
    empty = np.zeros(n + 1, np.int64)
    mixed = np.arange(n + 1, dtype=np.int64)          # 0.1 n = 2 and 0.9 n = 18 are excluded: 3..17
    for f in (car.pac, fc.pac):
        assert f(ends) == 0.0
        assert f(mid) == 1.0
        assert f(empty) == 0.0
        assert f(mixed) == sum(range(3, 18)) / sum(range(21))
        assert f(mixed, 0.0, 1.0) == sum(range(1, 20)) / sum(range(21))
    for f in (car.cdf, fc.consensus_cdf):
        assert np.array_equal(f(empty), np.zeros(n + 1))
        c = f(ends)
        assert c.dtype == np.float64 and np.array_equal(c, np.r_[np.full(n, 0.7), 1.0])
        assert np.array_equal(f(mixed), np.cumsum(mixed) / 210)
    h = np.random.default_rng(5).integers(0, 1000, 65)
    assert car.pac(h) == fc.pac(h) and np.array_equal(car.cdf(h), fc.consensus_cdf(h))


def test_symbols_declared():
    from fastconsensus_amd import _lib
    for name in ("fc_coassociation", "fc_coassoc_pairs", "fc_coassoc_hist", "fc_coassoc_timing"):
        assert name in _lib.SYMBOLS


def test_engine_methods():
    import fastconsensus_amd as fc
    for name in ("coassociation", "coassoc_pairs", "coassoc_hist", "coassoc_timing"):
        assert callable(getattr(fc.Engine, name, None)), name


def test_fast_consensus_keyword():
    import fastconsensus_amd as fc
    p = inspect.signature(fc.fast_consensus).parameters.get("coassoc")
    assert p is not None and p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


def test_cli_flag_is_parsed_and_hidden(tmp_path):
    from fastconsensus_amd import cli
    p = cli.build_parser()
    assert p.parse_args(["-f", "g.txt"]).coassoc is None
    assert p.parse_args(["-f", "g.txt", "--coassoc", "7"]).coassoc == 7
    assert "coassoc" not in p.format_help()
    nodes = np.array([10, 20, 30, 40])
    mat = np.arange(4, dtype=np.int32).reshape(2, 2)
    cli.write_coassoc(nodes, np.array([3, 1]), mat, root=str(tmp_path))
    assert np.array_equal(np.load(str(tmp_path / "coassoc.npy")), mat)
    assert (tmp_path / "coassoc_nodes.txt").read_text() == "40\n20\n"
