#!/usr/bin/env python3
"""One rank of run_sharded(..., consensus=theta) with a real HIP engine (test infrastructure of
tests/test_gpu_consensus_sharded.py; gloo, every rank on cuda:0).  Writes <out>_<rank>.npz: the
rank's consensus result, and on rank 0 the labelings.

    python -m tests.consensus_worker --rank R --world W --port P --n-p NP --theta T --seed S --out PREFIX
"""
import numpy as np

from tests.sharded import rank_main


def arguments(ap):
    ap.add_argument("--n-p", type=int, required=True)
    ap.add_argument("--theta", type=float, required=True)
    ap.add_argument("--seed", type=int, required=True)


def body(a):
    import torch
    import fastconsensus_amd as fc
    from fastconsensus_amd.distributed import run_sharded
    from tests import golden_io
    case = golden_io.load("lfr1k_louvain_np20")
    e = case.edges_file
    with fc.Engine(device=0, seed=a.seed) as eng:
        eng.load_graph(case.N, e[:, 0].copy(), e[:, 1].copy())
        labels, st, cons = run_sharded(eng, 0, a.n_p, 0.2, 0.02, device="cuda", consensus=a.theta)
        torch.cuda.synchronize()
        rec = {k: np.asarray(v) for k, v in cons.items()}
        if a.rank == 0:
            rec["run_labels"] = labels
        np.savez(a.out + "_%d.npz" % a.rank, **rec)


if __name__ == "__main__":
    rank_main(body, arguments)
