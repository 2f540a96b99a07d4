#!/usr/bin/env python3
"""One rank of item_affinity_sharded and median_refine_sharded with a real HIP engine (test
infrastructure of tests/test_gpu_median_sharded.py; gloo, every rank on cuda:0).  The rank installs
rows [lo, hi) of the first n_p golden LFR-1k labelings (none when lo == hi) and writes
<out>_<rank>.npz: the affinities of the queries in <out>_in.npz (part, nodes, clusters) and what
median_refine_sharded reaches from `part` in `rounds` rounds at the most.

    python -m tests.median_worker --rank R --world W --port P --n-p NP --lo LO --hi HI --rounds K --out PREFIX
"""
import numpy as np

from tests.sharded import rank_main

LISTS = ("objective", "proposed_per_round", "accepted_per_round", "alone_per_round", "gain_per_round", "mean_rand")


def arguments(ap):
    for name in ("n-p", "lo", "hi", "rounds"):
        ap.add_argument("--" + name, type=int, required=True)


def body(a):
    import torch
    import fastconsensus_amd as fc
    from fastconsensus_amd.distributed import item_affinity_sharded, median_refine_sharded
    from tests import golden_io
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    z = np.load(a.out + "_in.npz")
    with fc.Engine(device=0, seed=77) as eng:
        eng.load_graph(case.N, e[:, 0].copy(), e[:, 1].copy())
        if a.hi > a.lo:
            eng.set_labels(case.cd_batches[0][:a.n_p][a.lo:a.hi])
        aff = item_affinity_sharded(eng, z["part"], z["nodes"], z["clusters"], device="cuda")
        ref = median_refine_sharded(eng, z["part"], a.n_p, device="cuda", max_rounds=a.rounds)
        torch.cuda.synchronize()
        np.savez(a.out + "_%d.npz" % a.rank, aff=aff["aff"], slow_lookups=aff["slow_lookups"], labels=ref["labels"],
                 rounds=ref["rounds"], converged=ref["converged"], n_total=ref["n_total"],
                 **{k: np.array(ref[k]) for k in LISTS})


if __name__ == "__main__":
    rank_main(body, arguments)
