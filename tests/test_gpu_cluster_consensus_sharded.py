"""cluster_consensus_sharded over two and three ranks (gloo, all on the one GPU): every rank's
reduced cluster_pairs and item_pairs, and both normalised arrays, equal what one engine holding all
n_p labelings computes."""
import numpy as np
import pytest

from tests import cluster_consensus_ref as ccr
from tests import golden_io
from tests.sharded import run_ranks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("n_p,splits", [(20, ((0, 10), (10, 20))), (7, ((0, 2), (2, 4), (4, 7)))])
def test_ranks_equal_one(tmp_path, n_p, splits):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    labs = case.cd_batches[0][:n_p]
    part = case.cd_batches[-1][1] * 3 + 2                     # another batch's partition, sparse ids
    with fc.Engine(device=0, seed=77) as eng:
        eng.load_graph(case.N, e[:, 0], e[:, 1])
        eng.set_labels(labs)
        exp = eng.cluster_consensus(part)
    ids, size, pairs, item = ccr.sums(labs, part)
    assert np.array_equal(exp["cluster_pairs"], pairs) and np.array_equal(exp["item_pairs"], item)
    assert (pairs < n_p * size * size).any()                   # the labelings disagree with the partition somewhere
    prefix = str(tmp_path / "r")
    np.save(prefix + "_part.npy", part)
    run_ranks("cluster_consensus_worker", [["--n-p", n_p, "--lo", lo, "--hi", hi, "--out", prefix] for lo, hi in splits],
              120)
    for r in range(len(splits)):
        z = np.load(prefix + "_%d.npz" % r)
        for f in ("ids", "size", "cluster_pairs", "item_pairs"):
            assert z[f].dtype == exp[f].dtype and np.array_equal(z[f], exp[f]), (r, f)
        for f in ("cluster_consensus", "item_consensus"):
            assert z[f].dtype == np.float64 and ccr.same_floats(z[f], exp[f]), (r, f)
