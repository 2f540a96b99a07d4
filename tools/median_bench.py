"""Time fc_item_affinity and median_refine on the headline workload: LFR-1M (mu 0.5), louvain, n_p = 64.

    python tools/median_bench.py [--n 1000000] [--n-p 64] [--repeats 5] [--rounds 16]
                                 [--out profiles/median_lfr1m_np64.json]

One fast_consensus run leaves 64 labelings on the device.  On the best level of the consensus
hierarchy, its strictest level (n_p: only unanimous edges join) and replica 0, fc_item_affinity is
timed twice: with the refinement's own candidates ((v, top[v]) for the nodes whose plurality cluster
is not their own: few queries into few clusters) and with one query per node into its `top` (n
queries, every cluster queried).  Level 0 (the components of the input graph: one cluster far longer
than the length cap) takes the all-nodes queries through the exact fallback.  Per case: one warm-up
call, `repeats` timed calls of the C entry point with a preallocated output, the median and the
range, fc_synchronize before and after each timed region (timing off); then `repeats` calls with
timing on for the per-phase medians (fc_item_affinity_timing).  fc_cluster_consensus and fc_vote on
the same partition, in the same session and by the same protocol, stand beside them: the count
kernel's walk is fc_cluster_consensus'.  Then one whole median_refine per partition (`rounds` rounds
at the most): rounds, objective, the mean Rand pair, wall time and the share of it spent outside the
three engine calls (the selection on the host).  No time is fixed in advance.
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

PHASES = ("queries", "count", "fallback")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--mu", type=float, default=0.5)
    ap.add_argument("--n-p", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median_lfr1m_np64.json"))
    args = ap.parse_args()

    import torch

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

    cases, refines = [], []
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
        out = torch.empty(n, dtype=torch.int64, device="cuda:0")
        ids = np.empty(n, np.int32)
        size = np.empty(n, np.int64)
        hist = np.zeros(n_p + 1, np.int64)
        torch.cuda.synchronize()
        vinfo, cinfo, ainfo = _lib.VoteInfo(), _lib.ClusterInfo(), _lib.AffinityInfo()
        for name, part in parts:
            part = np.ascontiguousarray(part, np.int32)

            def call_vote():
                _lib.check(eng._L.fc_vote(eng._ctx, part.ctypes.data, top.data_ptr(), tv.data_ptr(), own.data_ptr(),
                                          hist.ctypes.data, ctypes.addressof(vinfo)))

            def call_cc():
                _lib.check(eng._L.fc_cluster_consensus(eng._ctx, part.ctypes.data, ids.ctypes.data, size.ctypes.data,
                                                       dc.data_ptr(), di.data_ptr(), ctypes.addressof(cinfo)))

            t_vote = timed(eng, call_vote)
            t_cc = timed(eng, call_cc)
            htop = top.cpu().numpy()
            item = di.cpu().numpy()
            everyone = np.arange(n, dtype=np.int32)
            moved = np.flatnonzero(htop != part).astype(np.int32)
            queries = [("all_nodes_into_top", everyone, htop)]
            if name != "level_0_components":
                queries.insert(0, ("refinement_candidates", moved, htop[moved]))
            for qname, nodes, clusters in queries:
                nodes, clusters = np.ascontiguousarray(nodes, np.int32), np.ascontiguousarray(clusters, np.int32)

                def call():
                    _lib.check(eng._L.fc_item_affinity(eng._ctx, part.ctypes.data, len(nodes), nodes.ctypes.data,
                                                       clusters.ctypes.data, out.data_ptr(), ctypes.addressof(ainfo)))

                t_aff = timed(eng, call)
                eng.set_timing(True)
                ph = {p: [] for p in PHASES}
                for _ in range(args.repeats):
                    call()
                    t = eng.item_affinity_timing()
                    eng.collect_timing()                              # hands the events back to the pool
                    for p in PHASES:
                        ph[p].append(t[p] * 1e-3)
                eng.set_timing(False)
                d = ainfo.as_dict()
                if qname == "all_nodes_into_top":                     # where top is the node's own: item_pairs
                    same = htop == part
                    assert np.array_equal(out.cpu().numpy()[same], item[same])
                cases.append({
                    "partition": name, "queries": qname, "npairs": int(len(nodes)), "info": d,
                    "call_s": t_aff, "phase_s": {p: {"median": med(ph[p]), "all": ph[p]} for p in PHASES},
                    "slow_share": d["slow_lookups"] / max(len(nodes) * n_p, 1),
                    "cluster_consensus_call_s": t_cc, "vote_call_s": t_vote,
                    "ratio_to_cluster_consensus": t_aff["median"] / t_cc["median"],
                })
            if name == "level_0_components":
                continue
            spent = [0.0]

            def clocked(fn):
                def run(*a):
                    t0 = time.perf_counter()
                    r = fn(*a)
                    spent[0] += time.perf_counter() - t0
                    return r
                return run

            t0 = time.perf_counter()
            ref = fc.median_refine(eng, part, max_rounds=args.rounds, vote=clocked(eng.vote),
                                   cluster_consensus=clocked(eng.cluster_consensus),
                                   item_affinity=clocked(eng.item_affinity))
            wall = time.perf_counter() - t0
            refines.append({
                "partition": name, "max_rounds": args.rounds, "rounds": ref["rounds"], "converged": ref["converged"],
                "objective": ref["objective"], "mean_rand": list(ref["mean_rand"]),
                "proposed_per_round": ref["proposed_per_round"], "accepted_per_round": ref["accepted_per_round"],
                "alone_per_round": ref["alone_per_round"], "k_before": int(len(np.unique(part))),
                "k_after": int(len(np.unique(ref["labels"]))), "wall_s": wall, "engine_calls_s": spent[0],
                "host_share": 1.0 - spent[0] / wall,
            })
    res = {
        "workload": {"n": n, "m": int(len(u)), "mu": args.mu, "algo": "louvain", "n_p": n_p, "seed": args.seed,
                     "run_iterations": int(stats["iterations"]), "best_level": int(best["level"])},
        "library": built_hash(),
        "protocol": "per case 1 warm-up + %d timed calls of fc_item_affinity with a preallocated output, median and "
                    "range, fc_synchronize around each (timing off); fc_cluster_consensus and fc_vote on the same "
                    "partition by the same protocol; then %d calls with timing on for the phase medians (HIP events, "
                    "fc_item_affinity_timing); then one median_refine (max_rounds %d), engine_calls_s the time inside "
                    "Engine.vote / cluster_consensus / item_affinity (their downloads included)"
                    % (args.repeats, args.repeats, args.rounds),
        "item_affinity": cases,
        "median_refine": refines,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
