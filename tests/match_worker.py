#!/usr/bin/env python3
"""One rank of cluster_match_sharded and run_sharded(match=True) with a real HIP engine (test
infrastructure of tests/test_gpu_cluster_match_sharded.py; gloo, every rank on cuda:0).  The rank
installs rows [lo, hi) of the first n_p golden LFR-1k labelings (none when lo == hi) and writes
<out>_<rank>.npz: the gathered tables and their summary for the partition in <out>_part.npy, and the
match keys of the consensus dict of a whole sharded run.

    python -m tests.match_worker --rank R --world W --port P --n-p NP --lo LO --hi HI --out PREFIX
"""
import numpy as np

from tests.sharded import rank_main

FIELDS = ("ids", "size", "inter", "csize", "jaccard", "f1", "stability", "recovered", "dissolved")
SCALARS = ("k", "max_size", "singletons", "perfect", "inter_total", "slow_members", "n_r")
RUN = ("labels", "match_inter", "match_csize", "match_stability", "match_recovered", "match_dissolved")


def arguments(ap):
    for name in ("n-p", "lo", "hi"):
        ap.add_argument("--" + name, type=int, required=True)


def body(a):
    import torch
    import fastconsensus_amd as fc
    from fastconsensus_amd.distributed import cluster_match_sharded, run_sharded
    from tests import golden_io
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    part = np.load(a.out + "_part.npy")
    with fc.Engine(device=0, seed=77) as eng:
        eng.load_graph(case.N, e[:, 0].copy(), e[:, 1].copy())
        if a.hi > a.lo:
            eng.set_labels(case.cd_batches[0][:a.n_p][a.lo:a.hi])
        res = cluster_match_sharded(eng, part, a.n_p, device="cuda")
        labels, st, cons = run_sharded(eng, 0, a.n_p, 0.2, 0.02, consensus=0.5, match=True)
        torch.cuda.synchronize()
        np.savez(a.out + "_%d.npz" % a.rank, **{k: res[k] for k in FIELDS}, **{k: np.int64(res[k]) for k in SCALARS},
                 **{"run_" + k: cons[k] for k in RUN})


if __name__ == "__main__":
    rank_main(body, arguments)
