"""coassociation_sharded over two ranks (gloo, both on the one GPU): every rank's reduced matrix
equals, bit for bit, what one engine holding all n_p labelings counts; the sharded histogram equals
that engine's fc_coassoc_hist."""
import numpy as np
import pytest

from tests import coassoc_ref as car
from tests import golden_io
from tests.sharded import run_ranks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("n_p,splits", [(20, ((0, 10), (10, 20))), (5, ((0, 3), (3, 5)))])
def test_two_ranks_equal_one(tmp_path, n_p, splits):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    world = len(splits)
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    labs = case.cd_batches[0][:n_p]
    rng = np.random.default_rng(n_p)
    a, b = rng.choice(case.N, 300, replace=False), rng.choice(case.N, 130, replace=False)
    with fc.Engine(device=0, seed=77) as eng:
        eng.load_graph(case.N, e[:, 0], e[:, 1])
        eng.set_labels(labs)
        exp = eng.coassociation(a, b).cpu().numpy()
        exp_sq = eng.coassociation(a).cpu().numpy()
        exp_hist = eng.coassoc_hist(a)
    assert np.array_equal(exp, car.matrix(labs, a, b)) and 0 < exp.min() + 1 <= exp.max() <= n_p
    prefix = str(tmp_path / "r")
    np.savez(prefix + "_lists.npz", a=a, b=b)
    run_ranks("coassoc_worker", [["--n-p", n_p, "--lo", lo, "--hi", hi, "--out", prefix] for lo, hi in splits], 120)
    for r in range(world):
        z = np.load(prefix + "_%d.npz" % r)
        assert z["matrix"].dtype == np.int32 and np.array_equal(z["matrix"], exp), r
        assert np.array_equal(z["square"], exp_sq), r
        assert z["hist"].dtype == np.int64 and np.array_equal(z["hist"], exp_hist), r
