#!/usr/bin/env python3
"""One rank of cluster_consensus_sharded with a real HIP engine (test infrastructure of
tests/test_gpu_cluster_consensus_sharded.py; gloo, every rank on cuda:0).  The rank installs rows
[lo, hi) of the first n_p golden LFR-1k labelings and writes <out>_<rank>.npz: the reduced integers
and the two normalised arrays for the partition in <out>_part.npy.

    python -m tests.cluster_consensus_worker --rank R --world W --port P --n-p NP --lo LO --hi HI --out PREFIX
"""
import numpy as np

from tests.sharded import rank_main


def arguments(ap):
    for name in ("n-p", "lo", "hi"):
        ap.add_argument("--" + name, type=int, required=True)


def body(a):
    import torch
    import fastconsensus_amd as fc
    from fastconsensus_amd.distributed import cluster_consensus_sharded
    from tests import golden_io
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    part = np.load(a.out + "_part.npy")
    with fc.Engine(device=0, seed=77) as eng:
        eng.load_graph(case.N, e[:, 0].copy(), e[:, 1].copy())
        eng.set_labels(case.cd_batches[0][:a.n_p][a.lo:a.hi])
        res = cluster_consensus_sharded(eng, part, a.n_p, device="cuda")
        torch.cuda.synchronize()
        np.savez(a.out + "_%d.npz" % a.rank, **{k: res[k] for k in ("ids", "size", "cluster_pairs", "item_pairs",
                                                                    "cluster_consensus", "item_consensus")})


if __name__ == "__main__":
    rank_main(body, arguments)
