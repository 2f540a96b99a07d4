"""Time fc_community_graph, fc_cluster_coassoc and merge_refine on the headline workload: LFR-1M
(mu 0.5), louvain, n_p = 64.

    python tools/merge_bench.py [--n 1000000] [--n-p 64] [--repeats 5] [--rounds 64]
                                [--out profiles/merge_lfr1m_np64.json]

One fast_consensus run leaves 64 labelings on the device.  On the best level of the consensus
hierarchy, its strictest level (n_p: only unanimous edges join) and replica 0: fc_community_graph
with device outputs, fc_cluster_coassoc on that graph's pairs, and one whole merge_refine (`rounds`
rounds at the most).  Per call: one warm-up, `repeats` timed calls of the C entry point with
preallocated outputs, the median and the range, fc_synchronize before and after each timed region
(timing off); then `repeats` calls with timing on for the per-phase medians (HIP events).

The comparison that decides whether the count kernel earns its place: the same X(a, b) by the route
the library had before, fc_item_affinity with one query (v, list side) per member v of the walk
side, summed per pair on the host -- on the pairs of the best level's community graph (the first
10^5 when the query list would pass 5 * 10^7), both routes downloading their result, alternated
twice in one session (new, old, new, old).  The old route's query list is built outside its timed
region.  No time is fixed in advance.
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

CG_PHASES = ("labels", "emit", "sort", "pairs")
MC_PHASES = ("pairs", "count", "fallback")
QUERY_LIMIT = 50_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--mu", type=float, default=0.5)
    ap.add_argument("--n-p", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_lfr1m_np64.json"))
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

    def phases(eng, call, getter, names):
        eng.set_timing(True)
        ph = {p: [] for p in names}
        for _ in range(args.repeats):
            call()
            t = getter()
            eng.collect_timing()                              # hands the events back to the pool
            for p in names:
                ph[p].append(t[p] * 1e-3)
        eng.set_timing(False)
        return {p: {"median": med(ph[p]), "all": ph[p]} for p in names}

    graphs, coassocs, refines, compare = [], [], [], None
    with fc.Engine(seed=args.seed) as eng:
        eng.set_option("store", store_order_pays(n_p, 0))
        eng.load_graph(n, u, v)
        labels, stats = eng.run(0, n_p, 0.2, 0.02)
        print("run done", file=sys.stderr, flush=True)
        m = eng.graph_info()[2]
        best = best_consensus(eng)
        parts = [("best_level", best["labels"]), ("strictest_level", eng.consensus_cut(n_p)[0]), ("replica_0", labels[0])]
        da, db = (torch.empty(m, dtype=torch.int32, device="cuda:0") for _ in range(2))
        dw, de = (torch.empty(m, dtype=torch.int64, device="cuda:0") for _ in range(2))
        out = torch.empty(max(m, n), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        cnt = ctypes.c_int64(0)
        pinfo, ainfo = _lib.ClusterPairInfo(), _lib.AffinityInfo()
        for name, part in parts:
            part = np.ascontiguousarray(part, np.int32)

            def call_cg():
                _lib.check(eng._L.fc_community_graph(eng._ctx, 0, part.ctypes.data, m, da.data_ptr(), db.data_ptr(),
                                                     dw.data_ptr(), de.data_ptr(), ctypes.byref(cnt)))

            t_cg = timed(eng, call_cg)
            npairs = int(cnt.value)
            a = np.ascontiguousarray(da[:npairs].cpu().numpy())
            b = np.ascontiguousarray(db[:npairs].cpu().numpy())
            graphs.append({"partition": name, "k": int(len(np.unique(part))), "npairs": npairs,
                           "cut_edges": int(de[:npairs].sum().item()), "call_s": t_cg,
                           "phase_s": phases(eng, call_cg, eng.community_graph_timing, CG_PHASES)})

            def call_mc():
                _lib.check(eng._L.fc_cluster_coassoc(eng._ctx, part.ctypes.data, npairs, a.ctypes.data, b.ctypes.data,
                                                     out.data_ptr(), ctypes.addressof(pinfo)))

            t_mc = timed(eng, call_mc)
            d = pinfo.as_dict()
            coassocs.append({"partition": name, "npairs": npairs, "info": d, "call_s": t_mc,
                             "phase_s": phases(eng, call_mc, eng.cluster_coassoc_timing, MC_PHASES),
                             "slow_share": d["slow_lookups"] / max(d["walked_members"] * n_p, 1)})

            if name == "best_level":
                # the route the library had before: one item-affinity query per walk-side member
                ids, size = np.unique(part, return_counts=True)
                take = npairs
                sa, sb = size[np.searchsorted(ids, a)], size[np.searchsorted(ids, b)]
                if int(np.minimum(sa, sb).sum()) > QUERY_LIMIT:
                    take = min(npairs, 100_000)
                pa, pb = a[:take].copy(), b[:take].copy()
                t0 = time.perf_counter()
                a_lists = sa[:take] >= sb[:take]
                lst, wlk = np.where(a_lists, pa, pb), np.where(a_lists, pb, pa)
                order = np.argsort(part, kind="stable")
                start = np.searchsorted(part[order], ids)
                wr = np.searchsorted(ids, wlk)
                rep = size[wr]
                first = np.cumsum(rep) - rep
                nodes = order[np.repeat(start[wr] - first, rep) + np.arange(int(rep.sum()))].astype(np.int32)
                clusters = np.repeat(lst, rep).astype(np.int32)
                build_s = time.perf_counter() - t0
                qout = torch.empty(len(nodes), dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                res = {}

                def route_new():
                    _lib.check(eng._L.fc_cluster_coassoc(eng._ctx, part.ctypes.data, take, pa.ctypes.data, pb.ctypes.data,
                                                         out.data_ptr(), ctypes.addressof(pinfo)))
                    res["new"] = out[:take].cpu().numpy()

                def route_old():
                    _lib.check(eng._L.fc_item_affinity(eng._ctx, part.ctypes.data, len(nodes), nodes.ctypes.data,
                                                       clusters.ctypes.data, qout.data_ptr(), ctypes.addressof(ainfo)))
                    res["old"] = np.add.reduceat(qout.cpu().numpy(), first)

                blocks = [("cluster_coassoc", timed(eng, route_new)), ("item_affinity_route", timed(eng, route_old)),
                          ("cluster_coassoc", timed(eng, route_new)), ("item_affinity_route", timed(eng, route_old))]
                assert np.array_equal(res["new"], res["old"])
                new = [t for k, b_ in blocks if k == "cluster_coassoc" for t in b_["all"]]
                old = [t for k, b_ in blocks if k == "item_affinity_route" for t in b_["all"]]
                compare = {"partition": name, "pairs": int(take), "of_pairs": npairs, "queries": int(len(nodes)),
                           "query_build_s": build_s, "blocks": [{"route": k, **b_} for k, b_ in blocks],
                           "cluster_coassoc_s": {"median": med(new), "min": min(new), "max": max(new)},
                           "item_affinity_route_s": {"median": med(old), "min": min(old), "max": max(old)},
                           "speedup": med(old) / med(new), "wins_by_more_than_the_ranges": min(old) > max(new),
                           "equal_results": True}

            spent = [0.0]

            def clocked(fn):
                def run(*args_):
                    t0 = time.perf_counter()
                    r = fn(*args_)
                    spent[0] += time.perf_counter() - t0
                    return r
                return run

            t0 = time.perf_counter()
            ref = fc.merge_refine(eng, part, max_rounds=args.rounds, community_graph=clocked(eng.community_graph),
                                  cluster_coassoc=clocked(eng.cluster_coassoc),
                                  cluster_consensus=clocked(eng.cluster_consensus), sum_sq=0)
            wall = time.perf_counter() - t0
            refines.append({
                "partition": name, "max_rounds": args.rounds, "rounds": ref["rounds"], "converged": ref["converged"],
                "objective_before": ref["objective"][0], "objective_after": ref["objective"][-1],
                "k_per_round": ref["k_per_round"], "pairs_per_round": ref["pairs_per_round"],
                "proposed_per_round": ref["proposed_per_round"], "accepted_per_round": ref["accepted_per_round"],
                "wall_s": wall, "engine_calls_s": spent[0], "host_share": 1.0 - spent[0] / wall,
            })
            print("%s done" % name, file=sys.stderr, flush=True)
    res = {
        "workload": {"n": n, "m": int(len(u)), "mu": args.mu, "algo": "louvain", "n_p": n_p, "seed": args.seed,
                     "run_iterations": int(stats["iterations"]), "best_level": int(best["level"])},
        "library": built_hash(),
        "protocol": "per call 1 warm-up + %d timed calls of the C entry point with preallocated outputs, median and "
                    "range, fc_synchronize around each (timing off); then %d calls with timing on for the phase medians "
                    "(HIP events); the comparison alternates the two routes twice (new, old, new, old), each block by "
                    "the same protocol, both routes downloading their result, the old one summing per pair on the host; "
                    "then one merge_refine (max_rounds %d), engine_calls_s the time inside Engine.community_graph / "
                    "cluster_coassoc / cluster_consensus (their downloads included)"
                    % (args.repeats, args.repeats, args.rounds),
        "community_graph": graphs,
        "cluster_coassoc": coassocs,
        "item_affinity_comparison": compare,
        "merge_refine": refines,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
