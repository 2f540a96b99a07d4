"""Time the consensus partition on the headline workload: LFR-1M (mu 0.5), louvain, n_p = 64.

    python tools/consensus_bench.py [--n 1000000] [--n-p 64] [--theta 0.5] [--repeats 7]
                                    [--out profiles/consensus_lfr1m_np64.json] [--no-host]

One fast_consensus run leaves 64 labelings on the device.  Then, with the engine's timing on:
  * the phases of fc_consensus_partition on the input graph, from the HIP events the library
    records at the phase boundaries (fc_consensus_timing): one warm-up call, `repeats` timed
    calls, the median of each phase;
  * yardstick 1: fc_consensus_support on the working graph against a bare
    fc_consensus_partial(FC_ALGO_LPM) -- the same kernel on the same graph -- alternating,
    each timed by the events of the consensus_ms slot;
  * yardstick 2: each phase's algorithmic bytes (phase_bytes below) over its time, against the
    HBM peak;
  * the whole call on the host clock (it ends in a device synchronise and includes the downloads
    of labels and node sums);
  * the host alternative for context: the download of the n_p * n labels plus
    tests/consensus_ref.py, whose result must equal the device's.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes/s, the figure DESIGN.md's roofline table uses
PHASES = ("support", "histogram", "components", "renumber", "node_sums")


def phase_bytes(n, m, kept, n_r):
    """Algorithmic bytes per phase (what the algorithm has to move once, no cache credit)."""
    ldT = (n_r + 3) & ~3
    return {
        # edge ends, both label rows of every edge, the count
        "support": m * (8 + 2 * 4 * ldT + 4),
        # the counts
        "histogram": m * 4,
        # init (parent), hook (count + ends per edge; node ids and two parents per kept edge, one
        # parent written per union, < n of them), flatten (parent read + written, flag)
        "components": n * 4 + m * 12 + kept * 16 + n * 4 + n * 12,
        # scan (flag read, rank written), label (root, rank and node id per node and per internal
        # vertex, both label arrays, sizes), size statistics
        "renumber": n * 8 + n * 32 + n * 4,
        # per adjacency entry: neighbour, edge id, its count, the neighbour's label; per row: bounds,
        # own label, node id, two sums
        "node_sums": 2 * m * 16 + n * 32,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--mu", type=float, default=0.5)
    ap.add_argument("--n-p", type=int, default=64)
    ap.add_argument("--theta", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_lfr1m_np64.json"))
    args = ap.parse_args()

    import torch

    import fastconsensus_amd as fc
    from fastconsensus_amd import synth
    from fastconsensus_amd.build import built_hash
    from fastconsensus_amd.core import store_order_pays
    from tests import consensus_ref as cref

    u, v, _ = synth.lfr(args.n, args.mu, seed=args.seed)
    n_p, theta = args.n_p, args.theta
    med = lambda xs: float(np.median(xs))
    with fc.Engine(seed=args.seed) as eng:
        eng.set_option("store", store_order_pays(n_p, 0))
        eng.load_graph(args.n, u, v)
        labels, stats = eng.run(0, n_p, 0.2, 0.02)
        _, m_work, m_in = eng.graph_info()
        eng.set_timing(True)

        # phases of the whole call on the input graph
        res = eng.consensus_partition(theta)                      # warm-up: buffers, code objects
        phases = {k: [] for k in PHASES}
        wall = []
        for _ in range(args.repeats):
            eng._L.fc_synchronize(eng._ctx)
            t0 = time.perf_counter()
            res = eng.consensus_partition(theta)
            wall.append(time.perf_counter() - t0)
            for k, x in eng.consensus_timing().items():
                phases[k].append(x * 1e-3)
        eng.collect_timing()

        # yardstick 1: the support entry point against the bare count, working graph, alternating
        a = torch.empty(max(m_work, 1), dtype=torch.int32, device="cuda:0")
        b = torch.empty(max(m_work, 1), dtype=torch.int32, device="cuda:0")
        eng.consensus_support("working", a)
        eng.consensus_partial(fc.core.FC_ALGO_LPM, b)
        same_counts = bool(torch.equal(a, b))
        eng.collect_timing()
        t_sup, t_bare = [], []
        for _ in range(args.repeats):
            eng.consensus_support("working", a)
            t_sup.append(eng.collect_timing()["consensus_ms"] * 1e-3)
            eng.consensus_partial(fc.core.FC_ALGO_LPM, b)
            t_bare.append(eng.collect_timing()["consensus_ms"] * 1e-3)
        eng.set_timing(False)

        # the host alternative: download every labeling, then the reference
        host = None
        if not args.no_host:
            eng._L.fc_synchronize(eng._ctx)
            t0 = time.perf_counter()
            labs = eng.get_labels(n_p)
            t_down = time.perf_counter() - t0
            t0 = time.perf_counter()
            cu, cv = cref.canonical_edges(u, v)
            exp = cref.partition(args.n, cu, cv, theta, labels=labs)
            t_ref = time.perf_counter() - t0
            equal = all(np.array_equal(res[k], exp[k]) for k in ("labels", "support_hist", "node_in", "node_out")) \
                and all(int(res[k]) == exp[k] for k in cref.INFO_INTS)
            host = {"what": "download of n_p * n labels + tests/consensus_ref.py (numpy + a Python union-find)",
                    "download_s": t_down, "reference_s": t_ref, "total_s": t_down + t_ref,
                    "equals_device_result": bool(equal)}

    nbytes = phase_bytes(args.n, m_in, int(res["kept_edges"]), n_p)
    ph = {}
    for k in PHASES:
        t = med(phases[k])
        ph[k] = {"median_s": t, "all_s": phases[k], "bytes_model": nbytes[k],
                 "bytes_per_s": nbytes[k] / t if t > 0 else None,
                 "frac_of_hbm_peak": nbytes[k] / t / HBM_PEAK if t > 0 else None}
    device_s = sum(ph[k]["median_s"] for k in PHASES)
    ldT = (n_p + 3) & ~3
    work_bytes = m_work * (8 + 2 * 4 * ldT + 4)
    out = {
        "workload": {"n": args.n, "m_input": int(m_in), "m_working": int(m_work), "mu": args.mu, "algo": "louvain",
                     "n_p": n_p, "theta": theta, "seed": args.seed, "run_iterations": int(stats["iterations"])},
        "library": built_hash(),
        "protocol": "1 warm-up + %d timed calls, medians; phases from HIP events at the phase boundaries "
                    "(fc_consensus_timing); support vs bare count alternating, events of the consensus_ms slot; "
                    "whole call on the host clock around a call that ends in a device synchronise" % args.repeats,
        "result": {k: int(res[k]) for k in ("edges", "kept_edges", "unanimous_edges", "split_edges", "k", "max_size",
                                            "singletons", "passes")},
        "mean_stability": float(res["stability"].mean()),
        "phases": ph,
        "device_phases_total_s": device_s,
        "whole_call_host_clock_s": {"median": med(wall), "all": wall,
                                    "includes": "downloads of labels, node_in, node_out (20 n bytes) and host synchronises"},
        "yardstick_support_vs_bare_count": {
            "graph": "working", "bytes_model": work_bytes, "same_counts": same_counts,
            "consensus_support_s": {"median": med(t_sup), "all": t_sup},
            "consensus_partial_lpm_s": {"median": med(t_bare), "all": t_bare},
            "ratio": med(t_sup) / med(t_bare),
            "bytes_per_s": work_bytes / med(t_sup), "frac_of_hbm_peak": work_bytes / med(t_sup) / HBM_PEAK},
        "hbm_peak_bytes_per_s": HBM_PEAK,
        "host_alternative": host,
        "speedup_vs_host_alternative": (host["total_s"] / med(wall)) if host else None,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
