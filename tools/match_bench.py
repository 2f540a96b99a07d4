"""Time fc_cluster_match on the headline workload: LFR-1M (mu 0.5), louvain, n_p = 64.

    python tools/match_bench.py [--n 1000000] [--n-p 64] [--repeats 5] [--out profiles/match_lfr1m_np64.json]

One fast_consensus run leaves 64 labelings on the device.  Three partitions are then matched against
them: the best level of the consensus hierarchy, one cluster of all nodes (longer than the length cap:
every (member, replica) pair through the exact fallback) and n singletons (the widest tables).
Per partition: one warm-up call, `repeats` timed calls of the C entry point with preallocated
outputs, the median and the range, fc_synchronize before and after each timed region (timing
off); then `repeats` calls with timing on for the per-phase medians (fc_cluster_match_timing).
The number it is set against is fc_cluster_consensus on the same partition in the same process,
measured the same way, the calls alternating: it shares the segment phase and the list walk.  Both
times, their ratio and both calls' phase medians are recorded; nothing is compared with a figure
fixed in advance.
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

PHASES = ("segments", "sizes", "match", "fallback")
CC_PHASES = ("segments", "count", "fallback")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--mu", type=float, default=0.5)
    ap.add_argument("--n-p", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_lfr1m_np64.json"))
    args = ap.parse_args()

    import torch

    import fastconsensus_amd as fc
    from fastconsensus_amd import _lib, synth
    from fastconsensus_amd.build import built_hash
    from fastconsensus_amd.core import best_consensus, store_order_pays

    u, v, _ = synth.lfr(args.n, args.mu, seed=args.seed)
    n, n_p = args.n, args.n_p
    med = lambda xs: float(np.median(xs))      # noqa: E731
    cases = []
    with fc.Engine(seed=args.seed) as eng:
        eng.set_option("store", store_order_pays(n_p, 0))
        eng.load_graph(n, u, v)
        labels, stats = eng.run(0, n_p, 0.2, 0.02)
        best = best_consensus(eng)
        parts = [("best_level", best["labels"]), ("one_cluster", np.zeros(n, np.int32)),
                 ("singletons", np.arange(n, dtype=np.int32))]
        ids = np.empty(n, np.int32)
        size = np.empty(n, np.int64)
        dc = torch.empty(n, dtype=torch.int64, device="cuda:0")
        di = torch.empty(n, dtype=torch.int64, device="cuda:0")
        info = _lib.MatchInfo()
        cinfo = _lib.ClusterInfo()
        for name, part in parts:
            part = np.ascontiguousarray(part, np.int32)
            k = len(np.unique(part))
            inter = torch.empty((n_p, k), dtype=torch.int32, device="cuda:0")
            csize = torch.empty((n_p, k), dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()

            def match():
                _lib.check(eng._L.fc_cluster_match(eng._ctx, part.ctypes.data, None, k, ids.ctypes.data, size.ctypes.data,
                                                   inter.data_ptr(), csize.data_ptr(), ctypes.addressof(info)))

            def consensus():
                _lib.check(eng._L.fc_cluster_consensus(eng._ctx, part.ctypes.data, ids.ctypes.data, size.ctypes.data,
                                                       dc.data_ptr(), di.data_ptr(), ctypes.addressof(cinfo)))

            match()                                                   # warm-up: buffers, code objects
            consensus()
            ts = {"match": [], "consensus": []}
            for _ in range(args.repeats):                             # alternating: both see the same neighbours
                for key, call in (("match", match), ("consensus", consensus)):
                    eng._L.fc_synchronize(eng._ctx)
                    t0 = time.perf_counter()
                    call()
                    eng._L.fc_synchronize(eng._ctx)
                    ts[key].append(time.perf_counter() - t0)
            eng.set_timing(True)
            ph = {p: [] for p in PHASES}
            cph = {p: [] for p in CC_PHASES}
            for _ in range(args.repeats):
                match()
                t = eng.cluster_match_timing()
                consensus()
                c = eng.cluster_consensus_timing()
                eng.collect_timing()                                  # hands the events back to the pool
                for p in PHASES:
                    ph[p].append(t[p] * 1e-3)
                for p in CC_PHASES:
                    cph[p].append(c[p] * 1e-3)
            eng.set_timing(False)
            assert int(info.k) == k == int(cinfo.k) and int(info.n_r) == n_p
            hi, hc = inter.cpu().numpy(), csize.cpu().numpy()
            assert int(hi.astype(np.int64).sum()) == info.inter_total and hi.min() >= 1 and np.all(hi <= hc)
            s = fc.core.match_summary(hi, size[:k], hc)
            tm, tc = med(ts["match"]), med(ts["consensus"])
            case = {
                "partition": name, "k": k, "max_size": int(info.max_size), "singletons": int(info.singletons),
                "match_s": {"median": tm, "min": min(ts["match"]), "max": max(ts["match"]), "all": ts["match"]},
                "cluster_consensus_s": {"median": tc, "min": min(ts["consensus"]), "max": max(ts["consensus"]),
                                        "all": ts["consensus"]},
                "match_over_cluster_consensus": tm / tc,
                "match_phase_s": {p: {"median": med(ph[p]), "all": ph[p]} for p in PHASES},
                "cluster_consensus_phase_s": {p: {"median": med(cph[p]), "all": cph[p]} for p in CC_PHASES},
                "slow_members": int(info.slow_members), "slow_share": int(info.slow_members) / (n * n_p),
                "perfect": int(info.perfect), "inter_total": int(info.inter_total),
                "mean_stability": float(s["stability"].mean()),
                "recovered_in_all": int((s["recovered"] == n_p).sum()), "dissolved_in_all": int((s["dissolved"] == n_p).sum()),
            }
            print(json.dumps(case), flush=True)
            cases.append(case)
            del inter, csize
    res = {
        "workload": {"n": n, "m": int(len(u)), "mu": args.mu, "algo": "louvain", "n_p": n_p, "seed": args.seed,
                     "run_iterations": int(stats["iterations"]), "best_level": int(best["level"])},
        "library": built_hash(),
        "protocol": "per partition 1 warm-up + %d timed calls each of fc_cluster_match and fc_cluster_consensus, "
                    "alternating, preallocated outputs, median and range, fc_synchronize around each (timing off); then "
                    "%d calls each with timing on for the phase medians (HIP events)" % (args.repeats, args.repeats),
        "partitions": cases,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["workload"]))


if __name__ == "__main__":
    main()
