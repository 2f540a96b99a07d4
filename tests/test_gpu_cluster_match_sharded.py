"""cluster_match_sharded and run_sharded(match=True) over two and three ranks (gloo, all on the one
GPU), with uneven shards and a rank without replicas: every rank's gathered tables, their summary
and the match keys of the consensus dict are identical to one engine holding all n_p labelings."""
import numpy as np
import pytest

from tests import golden_io
from tests import match_ref as mr
from tests.match_worker import FIELDS, RUN, SCALARS
from tests.sharded import run_ranks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("n_p,splits", [(20, ((0, 7), (7, 20))), (7, ((0, 2), (2, 2), (2, 7)))])
def test_ranks_equal_one(tmp_path, n_p, splits):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    from fastconsensus_amd.distributed import cluster_match_sharded, run_sharded
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    labs = case.cd_batches[0][:n_p]
    part = case.cd_batches[-1][1] * 3 + 2                     # another batch's partition, sparse ids
    with fc.Engine(device=0, seed=77) as eng:
        eng.load_graph(case.N, e[:, 0], e[:, 1])
        eng.set_labels(labs)
        exp = eng.cluster_match(part)
        one = cluster_match_sharded(eng, part, n_p)            # no process group: the one rank's own rows
        labels, st, cons = run_sharded(eng, 0, n_p, 0.2, 0.02, consensus=0.5, match=True)
    ids, size, inter, csize = mr.match(labs, part)
    assert np.array_equal(exp["inter"], inter) and np.array_equal(exp["csize"], csize)
    assert (inter < size[None, :]).any()                       # the labelings disagree with the partition somewhere
    for f in FIELDS:
        assert one[f].dtype == exp[f].dtype and np.array_equal(one[f], exp[f]), f
    for f in SCALARS:
        assert one[f] == exp[f], f
    assert np.array_equal(cons["match_inter"], mr.match(labels, cons["labels"])[2])
    prefix = str(tmp_path / "r")
    np.save(prefix + "_part.npy", part)
    run_ranks("match_worker", [["--n-p", n_p, "--lo", lo, "--hi", hi, "--out", prefix] for lo, hi in splits], 120)
    for r in range(len(splits)):
        z = np.load(prefix + "_%d.npz" % r)
        for f in FIELDS:
            assert z[f].dtype == exp[f].dtype and z[f].shape == exp[f].shape and np.all(z[f] == exp[f]), (r, f)
        for f in SCALARS:
            assert int(z[f]) == exp[f], (r, f)
        for f in RUN:
            assert z["run_" + f].dtype == cons[f].dtype and np.all(z["run_" + f] == cons[f]), (r, f)
