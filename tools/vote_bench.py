"""Time fc_vote on the headline workload: LFR-1M (mu 0.5), louvain, n_p = 64.

    python tools/vote_bench.py [--n 1000000] [--n-p 64] [--repeats 5] [--host-replicas 8]
                               [--out profiles/vote_lfr1m_np64.json]

One fast_consensus run leaves 64 labelings on the device.  Four partitions are then voted on: the
best level of the consensus hierarchy, its strictest level (n_p: only unanimous edges join), replica
0, and level 0 (the components of the input graph: one cluster far longer than the length cap, so
the map's exact fallback).  Per partition: one warm-up call, `repeats` timed calls of the C entry
point with preallocated outputs, the median and the range, fc_synchronize before and after each
timed region (timing off); then `repeats` calls with timing on for the per-phase medians
(fc_vote_timing); then vote_refine's rounds and moved-per-round.  No time is fixed in advance; the
call is recorded against two yardsticks:
  * fc_cluster_consensus on the same partition in the same session, by the same protocol: both
    walk labT by the clusters of the partition;
  * tests/vote_ref.py on the host for the same labelings, timed on `host-replicas` replicas and
    scaled to n_p (marked EXTRAPOLATED when fewer than n_p are timed).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("segments", "map", "map_fallback", "count")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--mu", type=float, default=0.5)
    ap.add_argument("--n-p", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-replicas", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vote_lfr1m_np64.json"))
    args = ap.parse_args()

    import torch

    import fastconsensus_amd as fc
    from fastconsensus_amd import _lib, synth
    from fastconsensus_amd.build import built_hash
    from fastconsensus_amd.core import best_consensus, store_order_pays
    from tests import vote_ref as vr

    u, v, _ = synth.lfr(args.n, args.mu, seed=args.seed)
    n, n_p = args.n, args.n_p
    med = lambda xs: float(np.median(xs))

    def timed(eng, call):
        """one warm-up, then `repeats` calls between fc_synchronize: seconds"""
        call()
        ts = []
        for _ in range(args.repeats):
            eng._L.fc_synchronize(eng._ctx)
            t0 = time.perf_counter()
            call()
            eng._L.fc_synchronize(eng._ctx)
            ts.append(time.perf_counter() - t0)
        return {"median": med(ts), "min": min(ts), "max": max(ts), "all": ts}

    cases = []
    with fc.Engine(seed=args.seed) as eng:
        eng.set_option("store", store_order_pays(n_p, 0))
        eng.load_graph(n, u, v)
        labels, stats = eng.run(0, n_p, 0.2, 0.02)
        best = best_consensus(eng)
        parts = [("best_level", best["labels"]), ("strictest_level", eng.consensus_cut(n_p)[0]),
                 ("replica_0", labels[0]), ("level_0_components", eng.consensus_cut(0)[0])]
        top, tv, own = (torch.empty(n, dtype=torch.int32, device="cuda:0") for _ in range(3))
        dc = torch.empty(n, dtype=torch.int64, device="cuda:0")
        di = torch.empty(n, dtype=torch.int64, device="cuda:0")
        ids = np.empty(n, np.int32)
        size = np.empty(n, np.int64)
        hist = np.zeros(n_p + 1, np.int64)
        torch.cuda.synchronize()
        info = _lib.VoteInfo()
        cinfo = _lib.ClusterInfo()
        for name, part in parts:
            part = np.ascontiguousarray(part, np.int32)

            def call():
                _lib.check(eng._L.fc_vote(eng._ctx, part.ctypes.data, top.data_ptr(), tv.data_ptr(), own.data_ptr(),
                                          hist.ctypes.data, ctypes.addressof(info)))

            def call_cc():
                _lib.check(eng._L.fc_cluster_consensus(eng._ctx, part.ctypes.data, ids.ctypes.data, size.ctypes.data,
                                                       dc.data_ptr(), di.data_ptr(), ctypes.addressof(cinfo)))

            t_vote = timed(eng, call)
            t_cc = timed(eng, call_cc)
            eng.set_timing(True)
            ph = {p: [] for p in PHASES}
            for _ in range(args.repeats):
                call()
                t = eng.vote_timing()
                eng.collect_timing()                                  # hands the events back to the pool
                for p in PHASES:
                    ph[p].append(t[p] * 1e-3)
            eng.set_timing(False)
            d = info.as_dict()
            assert int(hist.sum()) == n and d["unanimous"] == int(hist[n_p])
            ref = fc.vote_refine(eng, part)
            hr = min(args.host_replicas, n_p)
            t0 = time.perf_counter()
            vr.vote(labels[:hr], part)
            host_s = (time.perf_counter() - t0) * n_p / hr
            cases.append({
                "partition": name, "info": d, "own_hist": hist.tolist(),
                "mean_confidence": float(own.to(torch.float64).mean().item()) / n_p,
                "call_s": t_vote,
                "phase_s": {p: {"median": med(ph[p]), "all": ph[p]} for p in PHASES},
                "slow_share": d["slow_members"] / (n * n_p),
                "cluster_consensus_call_s": t_cc,
                "ratio_to_cluster_consensus": t_vote["median"] / t_cc["median"],
                "host_reference": {"what": "tests/vote_ref.vote, %d replicas%s" %
                                   (hr, "" if hr == n_p else ", EXTRAPOLATED to %d" % n_p),
                                   "extrapolated": hr != n_p, "s": host_s},
                "speedup_vs_host": host_s / t_vote["median"],
                "refine": {"rounds": ref["rounds"], "moved_per_round": ref["moved_per_round"],
                           "k_after": int(len(np.unique(ref["labels"]))), "fixpoint": ref["moved"] == 0},
            })
    res = {
        "workload": {"n": n, "m": int(len(u)), "mu": args.mu, "algo": "louvain", "n_p": n_p, "seed": args.seed,
                     "run_iterations": int(stats["iterations"]), "best_level": int(best["level"])},
        "library": built_hash(),
        "protocol": "per partition 1 warm-up + %d timed calls of fc_vote with preallocated outputs, median and range, "
                    "fc_synchronize around each (timing off); fc_cluster_consensus on the same partition by the same "
                    "protocol; then %d calls with timing on for the phase medians (HIP events, fc_vote_timing); then "
                    "vote_refine (max_rounds 16)" % (args.repeats, args.repeats),
        "best_buffer_bytes": 8 * n * min(n_p, 64),
        "mapped_buffer_bytes": 4 * n * n_p,
        "partitions": cases,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
