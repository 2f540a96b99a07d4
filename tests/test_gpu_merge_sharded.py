"""cluster_coassoc_sharded, merge_refine_sharded and run_sharded(merge=True) over two ranks (gloo,
both on the one GPU) with uneven shards: every rank's pair sums, merged partition and consensus dict
are bit-identical to one engine holding all 20 labelings."""
import numpy as np
import pytest

from tests import consensus_ref as cr
from tests import golden_io
from tests import merge_ref as gr
from tests.merge_worker import LISTS, RUN
from tests.sharded import run_ranks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def test_ranks_equal_one(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fastconsensus_amd as fc
    from fastconsensus_amd.distributed import run_sharded
    n_p, splits = 20, ((0, 7), (7, 20))
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    u, v = cr.canonical_edges(e[:, 0], e[:, 1])
    labs = case.cd_batches[0]
    part = cr.partition(case.N, u, v, 1.0, labels=labs)["labels"]
    g = gr.community_graph(case.N, u, v, None, part)
    a, b = np.r_[g["a"], g["b"][:50], 999], np.r_[g["b"], g["a"][:50], part[0]]
    with fc.Engine(device=0, seed=77) as eng:
        eng.load_graph(case.N, e[:, 0], e[:, 1])
        eng.set_labels(labs)
        x = eng.cluster_coassoc(part, a, b)
        exp = fc.merge_refine(eng, part)
        labels, st, cons = run_sharded(eng, 0, n_p, 0.2, 0.02, consensus="best", merge=True)
    assert 999 not in part and np.array_equal(x["x"], gr.cross(labs, part, a, b))
    ref = gr.refine(labs, part, case.N, u, v)
    assert np.array_equal(exp["labels"], ref["labels"]) and exp["objective"] == ref["objective"]
    assert exp["rounds"] == 11 and exp["objective"][-1] == 1039252
    prefix = str(tmp_path / "r")
    np.savez(prefix + "_in.npz", part=part, a=a, b=b)
    run_ranks("merge_worker", [["--n-p", n_p, "--lo", lo, "--hi", hi, "--out", prefix] for lo, hi in splits], 120)
    for r in range(len(splits)):
        z = np.load(prefix + "_%d.npz" % r)
        assert z["x"].dtype == np.int64 and np.array_equal(z["x"], x["x"]), r
        assert int(z["slow_lookups"]) == x["slow_lookups"]
        assert z["labels"].dtype == np.int32 and np.array_equal(z["labels"], exp["labels"]), r
        assert (int(z["rounds"]), bool(z["converged"])) == (exp["rounds"], exp["converged"])
        for f in LISTS:
            assert z[f].tolist() == list(exp[f]), (r, f)
        assert np.array_equal(z["cons_labels"], cons["labels"]), r
        for f in RUN:
            assert np.array_equal(z["run_" + f], np.array(cons[f])), (r, f)
