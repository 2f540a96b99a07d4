"""Time fc_cluster_consensus on the headline workload: LFR-1M (mu 0.5), louvain, n_p = 64.

    python tools/cluster_consensus_bench.py [--n 1000000] [--n-p 64] [--repeats 5] [--host-replicas 8]
                                            [--out profiles/cluster_consensus_lfr1m_np64.json]

One fast_consensus run leaves 64 labelings on the device.  Three partitions are then scored against
them: the best level of the consensus hierarchy, level 0 of the hierarchy (the components of the
input graph: one cluster far longer than the length cap, so the large-cluster path), and replica 0.
Per partition: one warm-up call, `repeats` timed calls of the C entry point with preallocated
outputs, the median and the range, fc_synchronize before and after each timed region (timing
off); then `repeats` calls with timing on for the per-phase medians (fc_cluster_consensus_timing).
Beside each:
  * the TWO-ROW-PASS cost profiles/score_lfr1m_np64.json implies: the all-pairs scoring call makes
    n_p - 1 row passes (sort, segments, one walk of labT), so 2 * score_pairs_s / (n_p - 1) is what
    two walks of labT cost there -- this call walks it twice (list build, item lookup);
  * tests/cluster_consensus_ref.py on the host for the same labelings, timed on `host-replicas`
    replicas and scaled to n_p (marked EXTRAPOLATED when fewer than n_p are timed);
  * slow_members / (N n_p), the share of (member, replica) pairs the exact fallback handled;
  * the bytes model: per member and bank 4 bytes of vertex id, the labT row (4 ldT bytes) read
    twice, 16 bytes of atomics.
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

HBM_PEAK = 8.0e12   # bytes/s, the figure DESIGN.md's roofline table uses
PHASES = ("segments", "count", "fallback")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--mu", type=float, default=0.5)
    ap.add_argument("--n-p", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-replicas", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_consensus_lfr1m_np64.json"))
    args = ap.parse_args()

    import torch

    import fastconsensus_amd as fc
    from fastconsensus_amd import _lib, synth
    from fastconsensus_amd.build import built_hash
    from fastconsensus_amd.core import best_consensus, store_order_pays
    from tests import cluster_consensus_ref as ccr

    with open(os.path.join(ROOT, "profiles", "score_lfr1m_np64.json")) as f:
        score = json.load(f)
    two_rows = 2 * score["score_pairs_s"]["median"] / (score["workload"]["n_p"] - 1)

    u, v, _ = synth.lfr(args.n, args.mu, seed=args.seed)
    n, n_p = args.n, args.n_p
    ldT = (n_p + 3) & ~3
    banks = (n_p + 63) // 64
    med = lambda xs: float(np.median(xs))
    cases = []
    with fc.Engine(seed=args.seed) as eng:
        eng.set_option("store", store_order_pays(n_p, 0))
        eng.load_graph(n, u, v)
        labels, stats = eng.run(0, n_p, 0.2, 0.02)
        best = best_consensus(eng)
        parts = [("best_level", best["labels"]), ("level_0_components", eng.consensus_cut(0)[0]),
                 ("replica_0", labels[0])]
        ids = np.empty(n, np.int32)
        size = np.empty(n, np.int64)
        dc = torch.empty(n, dtype=torch.int64, device="cuda:0")
        di = torch.empty(n, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        info = _lib.ClusterInfo()
        for name, part in parts:
            part = np.ascontiguousarray(part, np.int32)

            def call():
                _lib.check(eng._L.fc_cluster_consensus(eng._ctx, part.ctypes.data, ids.ctypes.data, size.ctypes.data,
                                                       dc.data_ptr(), di.data_ptr(), ctypes.addressof(info)))

            call()                                                    # warm-up: buffers, code objects
            ts = []
            for _ in range(args.repeats):
                eng._L.fc_synchronize(eng._ctx)
                t0 = time.perf_counter()
                call()
                eng._L.fc_synchronize(eng._ctx)
                ts.append(time.perf_counter() - t0)
            eng.set_timing(True)
            ph = {p: [] for p in PHASES}
            for _ in range(args.repeats):
                call()
                t = eng.cluster_consensus_timing()
                eng.collect_timing()                                  # hands the events back to the pool
                for p in PHASES:
                    ph[p].append(t[p] * 1e-3)
            eng.set_timing(False)
            item = di.cpu().numpy()
            k = int(info.k)
            assert int(item.sum()) == info.pairs_total == int(dc[:k].sum().item())
            hr = min(args.host_replicas, n_p)
            t0 = time.perf_counter()
            ccr.sums(labels[:hr], part)
            host_s = (time.perf_counter() - t0) * n_p / hr
            fast = n * n_p - int(info.slow_members)                   # (member, replica) pairs of the count kernel
            model = banks * n * (4 + 2 * 4 * ldT + 16)
            t = med(ts)
            cases.append({
                "partition": name, "k": k, "max_size": int(info.max_size), "singletons": int(info.singletons),
                "call_s": {"median": t, "min": min(ts), "max": max(ts), "all": ts},
                "phase_s": {p: {"median": med(ph[p]), "all": ph[p]} for p in PHASES},
                "slow_members": int(info.slow_members), "slow_share": int(info.slow_members) / (n * n_p),
                "count_kernel_member_replicas": fast,
                "bytes_model_per_call": model, "bytes_model_per_s_of_count_phase": model / max(med(ph["count"]), 1e-12),
                "frac_of_hbm_peak_of_count_phase": model / max(med(ph["count"]), 1e-12) / HBM_PEAK,
                "ratio_to_two_row_passes": t / two_rows,
                "host_reference": {"what": "tests/cluster_consensus_ref.sums, %d replicas%s" %
                                   (hr, "" if hr == n_p else ", EXTRAPOLATED to %d" % n_p),
                                   "extrapolated": hr != n_p, "s": host_s},
                "speedup_vs_host": host_s / t,
                "mean_cluster_consensus": float(np.nanmean(fc.cluster_consensus(dc[:k].cpu().numpy(), size[:k], n_p)))
                if (size[:k] > 1).any() else None,
            })
    res = {
        "workload": {"n": n, "m": int(len(u)), "mu": args.mu, "algo": "louvain", "n_p": n_p, "seed": args.seed,
                     "run_iterations": int(stats["iterations"]), "best_level": int(best["level"])},
        "library": built_hash(),
        "protocol": "per partition 1 warm-up + %d timed calls of fc_cluster_consensus with preallocated outputs, median "
                    "and range, fc_synchronize around each (timing off); then %d calls with timing on for the phase "
                    "medians (HIP events, fc_cluster_consensus_timing)" % (args.repeats, args.repeats),
        "bytes_model": "banks * n * (4 vertex id + 2 * 4 * ldT labT row read twice + 16 atomics)",
        "two_row_pass_s": two_rows,
        "two_row_pass_from": "profiles/score_lfr1m_np64.json: 2 * score_pairs_s.median / (n_p - 1) (library %s)"
                             % score.get("library"),
        "partitions": cases,
        "hbm_peak_bytes_per_s": HBM_PEAK,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
