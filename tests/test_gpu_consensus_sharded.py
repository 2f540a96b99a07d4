"""run_sharded(..., consensus=theta) over two ranks (gloo, both on the one GPU): every rank's
consensus result equals, bit for bit, what one engine holding all n_p partitions computes."""
import numpy as np
import pytest

from tests import golden_io
from tests.sharded import run_ranks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def test_two_ranks_equal_one(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    world, n_p, theta, seed = 2, 20, 0.5, 77
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    with fc.Engine(device=0, seed=seed) as eng:
        eng.load_graph(case.N, e[:, 0], e[:, 1])
        labels, _ = eng.run(0, n_p, 0.2, 0.02)
        exp = eng.consensus_partition(theta)
    prefix = str(tmp_path / "r")
    run_ranks("consensus_worker", [["--n-p", n_p, "--theta", theta, "--seed", seed, "--out", prefix]] * world, 120)
    z = [np.load(prefix + "_%d.npz" % r) for r in range(world)]
    np.testing.assert_array_equal(z[0]["run_labels"], labels)
    assert 1 < exp["k"] < case.N
    for r in range(world):
        assert sorted(k for k in z[r].files if k != "run_labels") == sorted(exp)
        for k, want in exp.items():
            got = z[r][k]
            assert got.dtype == np.asarray(want).dtype and np.array_equal(got, want), (r, k)
