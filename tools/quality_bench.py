"""Time fc_community_quality on the headline workload: LFR-1M (mu 0.5), louvain, n_p = 64.

    python tools/quality_bench.py [--n 1000000] [--n-p 64] [--repeats 5]
                                  [--out profiles/quality_lfr1m_np64.json]

One fast_consensus run leaves the working graph (the converged consensus graph with its weights)
beside the input graph.  On each of the two graphs and for each of three partitions -- the
consensus="best" partition, one cluster of all nodes, all singletons -- the C entry point is timed
with every output requested and preallocated: one warm-up call, `repeats` timed calls, the median
and the range, fc_synchronize before and after each timed region (timing off); then `repeats` calls
with timing on for the per-phase medians (fc_community_quality_timing: labels, rows, fold,
components).  Beside them stands the "node sums" phase of fc_consensus_partition (agreement 0.5) on
the same graph and engine, by the same protocol: the existing kernel that walks the same rows with
the same 16 lanes per row.  The ratios rows / node_sums and fold / node_sums are recorded; no time
is fixed in advance.
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

PHASES = ("labels", "rows", "fold", "components")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--mu", type=float, default=0.5)
    ap.add_argument("--n-p", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_lfr1m_np64.json"))
    args = ap.parse_args()

    import fastconsensus_amd as fc
    from fastconsensus_amd import _lib, synth
    from fastconsensus_amd.build import built_hash
    from fastconsensus_amd.core import best_consensus, store_order_pays

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

    cases, sums = [], {}
    with fc.Engine(seed=args.seed) as eng:
        eng.set_option("store", store_order_pays(n_p, 0))
        eng.load_graph(n, u, v)
        _, stats = eng.run(0, n_p, 0.2, 0.02)
        best = best_consensus(eng)
        parts = [("best", best["labels"]), ("one_cluster", np.zeros(n, np.int32)),
                 ("singletons", np.arange(n, dtype=np.int32))]
        rec = np.empty(n, _lib.COMMUNITY_RECORD)
        nin, nout, split = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.int32)
        info = _lib.QualityInfo()
        for graph in ("input", "working"):
            gid = _lib.SCORE_GRAPHS[graph]
            eng.set_timing(True)
            ns = []
            for _ in range(args.repeats + 1):
                eng.consensus_partition(0.5, graph=graph)
                ns.append(eng.consensus_timing()["node_sums"] * 1e-3)
                eng.collect_timing()                                  # hands the events back to the pool
            eng.set_timing(False)
            sums[graph] = {"median": med(ns[1:]), "all": ns[1:]}
            for name, part in parts:
                part = np.ascontiguousarray(part, np.int32)

                def call():
                    _lib.check(eng._L.fc_community_quality(eng._ctx, gid, part.ctypes.data, rec.ctypes.data,
                                                           nin.ctypes.data, nout.ctypes.data, split.ctypes.data,
                                                           ctypes.addressof(info)))

                t = timed(eng, call)
                eng.set_timing(True)
                ph = {p: [] for p in PHASES}
                for _ in range(args.repeats):
                    call()
                    x = eng.community_quality_timing()
                    eng.collect_timing()
                    for p in PHASES:
                        ph[p].append(x[p] * 1e-3)
                eng.set_timing(False)
                phase = {p: {"median": med(ph[p]), "all": ph[p]} for p in PHASES}
                cases.append({
                    "graph": graph, "partition": name, "edges": int(eng.graph_info()[1 if graph == "working" else 2]),
                    "info": {k: int(getattr(info, k)) for k, _ in info._fields_},
                    "call_s": t, "phase_s": phase, "node_sums_s": sums[graph],
                    "rows_over_node_sums": phase["rows"]["median"] / sums[graph]["median"],
                    "fold_over_node_sums": phase["fold"]["median"] / sums[graph]["median"],
                })
    res = {
        "workload": {"n": n, "m": int(len(u)), "mu": args.mu, "algo": "louvain", "n_p": n_p, "seed": args.seed,
                     "run_iterations": int(stats["iterations"]), "best_level": int(best["level"])},
        "library": built_hash(),
        "protocol": "per case 1 warm-up + %d timed calls of fc_community_quality with every output requested into "
                    "preallocated host arrays, median and range, fc_synchronize around each (timing off); then %d calls "
                    "with timing on for the phase medians (HIP events, fc_community_quality_timing); node_sums_s: the "
                    "node-sums phase of fc_consensus_partition(0.5) on the same graph, 1 warm-up + %d calls with timing on"
                    % (args.repeats, args.repeats, args.repeats),
        "community_quality": cases,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
