#!/usr/bin/env python3
"""One rank of cluster_coassoc_sharded, merge_refine_sharded and run_sharded(merge=True) with a real
HIP engine (test infrastructure of tests/test_gpu_merge_sharded.py; gloo, every rank on cuda:0).
The rank installs rows [lo, hi) of the first n_p golden LFR-1k labelings (none when lo == hi) and
writes <out>_<rank>.npz: the pair sums of the lists in <out>_in.npz (part, a, b), what
merge_refine_sharded reaches from `part`, and the consensus dict of a whole sharded run.

    python -m tests.merge_worker --rank R --world W --port P --n-p NP --lo LO --hi HI --out PREFIX
"""
import numpy as np

from tests.sharded import rank_main

LISTS = ("objective", "pairs_per_round", "proposed_per_round", "accepted_per_round", "gain_per_round", "k_per_round",
         "mean_rand")
RUN = ("merged", "merged_objective", "merged_rounds", "merged_accepted", "merged_k", "merged_mean_rand")


def arguments(ap):
    for name in ("n-p", "lo", "hi"):
        ap.add_argument("--" + name, type=int, required=True)


def body(a):
    import torch
    import fastconsensus_amd as fc
    from fastconsensus_amd.distributed import cluster_coassoc_sharded, merge_refine_sharded, run_sharded
    from tests import golden_io
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    z = np.load(a.out + "_in.npz")
    with fc.Engine(device=0, seed=77) as eng:
        eng.load_graph(case.N, e[:, 0].copy(), e[:, 1].copy())
        if a.hi > a.lo:
            eng.set_labels(case.cd_batches[0][:a.n_p][a.lo:a.hi])
        x = cluster_coassoc_sharded(eng, z["part"], z["a"], z["b"], device="cuda")
        ref = merge_refine_sharded(eng, z["part"], a.n_p, device="cuda")
        labels, st, cons = run_sharded(eng, 0, a.n_p, 0.2, 0.02, consensus="best", merge=True)
        torch.cuda.synchronize()
        np.savez(a.out + "_%d.npz" % a.rank, x=x["x"], slow_lookups=x["slow_lookups"], labels=ref["labels"],
                 rounds=ref["rounds"], converged=ref["converged"], cons_labels=cons["labels"],
                 **{k: np.array(ref[k]) for k in LISTS}, **{"run_" + k: np.array(cons[k]) for k in RUN})


if __name__ == "__main__":
    rank_main(body, arguments)
