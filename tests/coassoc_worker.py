#!/usr/bin/env python3
"""One rank of coassociation_sharded with a real HIP engine (test infrastructure of
tests/test_gpu_coassoc_sharded.py; gloo, every rank on cuda:0).  The rank installs rows [lo, hi) of
the first n_p golden LFR-1k labelings and writes <out>_<rank>.npz: the reduced matrix of the node
lists in <out>_lists.npz and the histogram taken from the reduced square matrix.

    python -m tests.coassoc_worker --rank R --world W --port P --n-p NP --lo LO --hi HI --out PREFIX
"""
import numpy as np

from tests.sharded import rank_main


def arguments(ap):
    for name in ("n-p", "lo", "hi"):
        ap.add_argument("--" + name, type=int, required=True)


def body(a):
    import torch
    import fastconsensus_amd as fc
    from fastconsensus_amd.distributed import coassoc_hist_sharded, coassociation_sharded
    from tests import golden_io
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    lists = np.load(a.out + "_lists.npz")
    with fc.Engine(device=0, seed=77) as eng:
        eng.load_graph(case.N, e[:, 0].copy(), e[:, 1].copy())
        eng.set_labels(case.cd_batches[0][:a.n_p][a.lo:a.hi])
        mat = coassociation_sharded(eng, lists["a"], lists["b"], device="cuda")
        sq = coassociation_sharded(eng, lists["a"], device="cuda")
        hist = coassoc_hist_sharded(eng, lists["a"], a.n_p, device="cuda")
        torch.cuda.synchronize()
        np.savez(a.out + "_%d.npz" % a.rank, matrix=mat.cpu().numpy(), square=sq.cpu().numpy(), hist=hist)


if __name__ == "__main__":
    rank_main(body, arguments)
