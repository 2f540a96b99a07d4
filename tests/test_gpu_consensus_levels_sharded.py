"""run_sharded(..., consensus="best") over two and three ranks (gloo, all on the one GPU): every
rank's result equals, bit for bit, what one engine holding all n_p partitions computes."""
import numpy as np
import pytest

from tests import golden_io
from tests.sharded import run_ranks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_one = {}


def one_engine(n_p, seed):
    """(labelings, consensus_levels dict, best_consensus dict) of one engine, computed once"""
    if not _one:
        import fastconsensus_amd as fc
        case = golden_io.load("lfr1k_louvain_np20")
        e = case.edges_file
        with fc.Engine(device=0, seed=seed) as eng:
            eng.load_graph(case.N, e[:, 0], e[:, 1])
            labels, _ = eng.run(0, n_p, 0.2, 0.02)
            lev = eng.consensus_levels()
            _one["x"] = (labels, lev, fc.core.best_consensus(eng, eng.consensus_support("input"), n_p))
    return _one["x"]


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_equal_one(tmp_path, world):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n_p, seed = 20, 77
    labels, lev, exp = one_engine(n_p, seed)
    prefix = str(tmp_path / "r")
    run_ranks("consensus_levels_worker", [["--n-p", n_p, "--seed", seed, "--out", prefix]] * world, 120)
    z = [np.load(prefix + "_%d.npz" % r) for r in range(world)]
    np.testing.assert_array_equal(z[0]["run_labels"], labels)
    assert 1 < exp["k"] < 1000 and 0 < exp["level"] <= n_p
    for r in range(world):
        assert sorted(k for k in z[r].files if k != "run_labels") == sorted(exp)
        for k, want in exp.items():
            got = z[r][k]
            assert got.dtype == np.asarray(want).dtype and np.array_equal(got, want), (r, k)
        for k in ("birth", "up", "levels"):
            assert np.array_equal(z[r][k], lev[k]), (r, k)
        assert int(z[r]["level"]) == lev["best_level"] and float(z[r]["theta"]) == lev["best_theta"]
