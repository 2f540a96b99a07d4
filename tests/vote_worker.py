#!/usr/bin/env python3
"""One rank of vote_sharded with a real HIP engine (test infrastructure of
tests/test_gpu_vote_sharded.py; gloo, every rank on cuda:0).  The rank installs rows [lo, hi) of the
first n_p golden LFR-1k labelings and writes <out>_<rank>.npz: the vote's arrays and info fields for
the partition in <out>_part.npy, and the partition vote_refine reaches from it over vote_sharded.

    python -m tests.vote_worker --rank R --world W --port P --n-p NP --lo LO --hi HI --out PREFIX
"""
import numpy as np

from tests.sharded import rank_main

FIELDS = ("top", "top_votes", "own_votes", "own_hist", "confidence", "k", "k_voted", "moved", "unanimous", "tied",
          "mapped_communities", "slow_members", "slow_nodes", "n_total")


def arguments(ap):
    for name in ("n-p", "lo", "hi"):
        ap.add_argument("--" + name, type=int, required=True)


def body(a):
    import torch
    import fastconsensus_amd as fc
    from fastconsensus_amd.distributed import vote_sharded
    from fastconsensus_amd.core import vote_refine
    from tests import golden_io
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    part = np.load(a.out + "_part.npy")
    with fc.Engine(device=0, seed=77) as eng:
        eng.load_graph(case.N, e[:, 0].copy(), e[:, 1].copy())
        eng.set_labels(case.cd_batches[0][:a.n_p][a.lo:a.hi])
        res = vote_sharded(eng, part, a.n_p, device="cuda")
        ref = vote_refine(eng, part, vote=lambda lab: vote_sharded(eng, lab, a.n_p, device="cuda"))
        torch.cuda.synchronize()
        np.savez(a.out + "_%d.npz" % a.rank, refined=ref["labels"], moved_per_round=np.array(ref["moved_per_round"]),
                 **{k: res[k] for k in FIELDS})


if __name__ == "__main__":
    rank_main(body, arguments)
