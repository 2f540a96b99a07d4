"""item_affinity_sharded and median_refine_sharded over two and three ranks (gloo, all on the one GPU)
with uneven shards, one of them empty: every rank's affinities and refined partition are bit-identical
to one engine holding all n_p labelings."""
import numpy as np
import pytest

from tests import golden_io
from tests import median_ref as mr
from tests.median_worker import LISTS
from tests.sharded import run_ranks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROUNDS = 3


@pytest.mark.parametrize("n_p,splits", [(20, ((0, 7), (7, 20))), (7, ((0, 2), (2, 3), (3, 7))),
                                        (5, ((0, 5), (5, 5)))])
def test_ranks_equal_one(tmp_path, n_p, splits):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    labs = case.cd_batches[0][:n_p]
    part = labs[0]
    rng = np.random.default_rng(n_p)
    nodes = rng.integers(0, case.N, 700)
    clusters = rng.choice(np.r_[np.unique(part), 999], 700)
    with fc.Engine(device=0, seed=77) as eng:
        eng.load_graph(case.N, e[:, 0], e[:, 1])
        eng.set_labels(labs)
        aff = eng.item_affinity(part, nodes, clusters)
        exp = fc.median_refine(eng, part, max_rounds=ROUNDS)
    assert np.array_equal(aff["aff"], mr.affinity(labs, part, nodes, clusters))
    ref = mr.refine(labs, part, max_rounds=ROUNDS)
    assert np.array_equal(exp["labels"], ref["labels"]) and exp["objective"] == ref["objective"]
    assert exp["rounds"] >= 1 and exp["accepted_per_round"][0] > 0 and exp["n_total"] == n_p
    prefix = str(tmp_path / "r")
    np.savez(prefix + "_in.npz", part=part, nodes=nodes, clusters=clusters)
    run_ranks("median_worker", [["--n-p", n_p, "--lo", lo, "--hi", hi, "--rounds", ROUNDS, "--out", prefix]
                                for lo, hi in splits], 120)
    for r in range(len(splits)):
        z = np.load(prefix + "_%d.npz" % r)
        assert z["aff"].dtype == np.int64 and np.array_equal(z["aff"], aff["aff"]), r
        assert int(z["slow_lookups"]) == aff["slow_lookups"]
        assert z["labels"].dtype == np.int32 and np.array_equal(z["labels"], exp["labels"]), r
        assert (int(z["rounds"]), bool(z["converged"]), int(z["n_total"])) == (exp["rounds"], exp["converged"], n_p)
        for f in LISTS:
            assert z[f].tolist() == list(exp[f]), (r, f)
