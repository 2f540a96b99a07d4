"""vote_sharded over two and three ranks (gloo, all on the one GPU) with uneven shards: every rank's
vote over the all-gathered `mapped`, and the partition vote_refine reaches through it, are bit-identical
to one engine holding all n_p labelings."""
import numpy as np
import pytest

from tests import golden_io
from tests import vote_ref as vr
from tests.sharded import run_ranks
from tests.vote_worker import FIELDS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("n_p,splits", [(20, ((0, 7), (7, 20))), (7, ((0, 2), (2, 3), (3, 7)))])
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
        exp = eng.vote(part)
        fine = fc.vote_refine(eng, part)
    ref = vr.vote(labs, part)
    assert np.array_equal(exp["top"], ref["top"]) and np.array_equal(exp["own_votes"], ref["own"])
    assert ref["moved"] > 0                                    # the labelings disagree with the partition somewhere
    prefix = str(tmp_path / "r")
    np.save(prefix + "_part.npy", part)
    run_ranks("vote_worker", [["--n-p", n_p, "--lo", lo, "--hi", hi, "--out", prefix] for lo, hi in splits], 120)
    for r in range(len(splits)):
        z = np.load(prefix + "_%d.npz" % r)
        for f in FIELDS:
            got, want = z[f], np.asarray(exp[f])
            assert got.dtype == want.dtype and np.array_equal(got, want), (r, f)
        assert np.array_equal(z["refined"], fine["labels"]) and z["moved_per_round"].tolist() == fine["moved_per_round"]
