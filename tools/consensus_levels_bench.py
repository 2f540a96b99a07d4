"""Time the consensus hierarchy on the headline workload: LFR-1M (mu 0.5), louvain, n_p = 64.

    python tools/consensus_levels_bench.py [--n 1000000] [--n-p 64] [--repeats 7]
                                           [--out profiles/consensus_levels_lfr1m_np64.json]

One fast_consensus run leaves 64 labelings on the device; their support on the input graph is
taken once (fc_consensus_support) and handed to both sides.  Then, alternating in one session:
  * the hierarchy: one fc_consensus_levels call (tree to device buffers, the level records to the
    host); its phases from the HIP events the library records at the phase boundaries
    (fc_consensus_levels_timing), the whole call on the host clock;
  * the yardstick, the only way to this family of partitions without the hierarchy: one
    fc_consensus_partition(dev_support, theta_of(level)) call per nonempty level (labels to a
    device buffer, no node sums); the device time is the sum of its phases
    (fc_consensus_timing) over the levels, the loop on the host clock.
One warm-up of each, then `repeats` timed rounds, medians and ranges.  Each phase's algorithmic
bytes (phase_bytes below) over its time stand against the HBM peak.  Before timing, every
nonempty level's cut is checked against the loop's labels.
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
PHASES = ("bucket", "tree", "statistics", "join_levels")
LOOP_PHASES = ("support", "histogram", "components", "renumber", "node_sums")


def phase_bytes(n, m, live, absorbed):
    """Algorithmic bytes per phase (what the algorithm has to move once, no cache credit).
    live: nonempty levels; absorbed: roots that stopped being roots, over all levels (< n)."""
    return {
        # histogram (the counts), offsets (nothing to speak of), scatter (the counts twice, the ids)
        "bucket": m * 4 + m * 8 + m * 4,
        # init (node id, degree; parent, birth, up, size, degree sum), hooks (id, ends, node ids and
        # two parents per edge, each edge once), a flatten per nonempty level (parent and birth of
        # every node), and per absorbed root its record, totals and the root's totals
        "tree": n * 36 + m * 28 + live * n * 8 + absorbed * 44,
        # the sharded per-level counters
        "statistics": (live + 1) * 256 * 7 * 8,
        # per edge: ends, node ids, birth and up of both ends (the walk's first step)
        "join_levels": m * 32,
    }


def rng(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "all": [float(x) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--mu", type=float, default=0.5)
    ap.add_argument("--n-p", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_levels_lfr1m_np64.json"))
    args = ap.parse_args()

    import torch

    import fastconsensus_amd as fc
    from fastconsensus_amd import _lib, synth
    from fastconsensus_amd.build import built_hash
    from fastconsensus_amd.core import LEVEL_DTYPE, store_order_pays, theta_of

    u, v, _ = synth.lfr(args.n, args.mu, seed=args.seed)
    n, n_p = args.n, args.n_p
    with fc.Engine(seed=args.seed) as eng:
        eng.set_option("store", store_order_pays(n_p, 0))
        eng.load_graph(n, u, v)
        _, stats = eng.run(0, n_p, 0.2, 0.02)
        _, _, m_in = eng.graph_info()
        sup = eng.consensus_support("input")
        dev = lambda: torch.empty(n, dtype=torch.int32, device="cuda:0")
        birth, up, lab = dev(), dev(), dev()
        levels = np.zeros(n_p + 1, LEVEL_DTYPE)
        best = ctypes.c_int32()
        info = _lib.ConsensusInfo()
        L, ctx = eng._L, eng._ctx
        torch.cuda.synchronize()
        eng.set_timing(True)

        def hierarchy():
            _lib.check(L.fc_consensus_levels(ctx, 0, sup.data_ptr(), n_p, birth.data_ptr(), up.data_ptr(),
                                             levels.ctypes.data, ctypes.byref(best)))

        def loop(live, into=None):
            dev_s = 0.0
            for i, s in enumerate(live):
                out = lab if into is None else into[i]
                _lib.check(L.fc_consensus_partition(ctx, 0, sup.data_ptr(), n_p, theta_of(s, n_p), out.data_ptr(),
                                                    None, None, None, ctypes.addressof(info)))
                dev_s += sum(eng.consensus_timing().values()) * 1e-3
            return dev_s

        hierarchy()                                               # warm-up: buffers, code objects
        live = [int(s) for s in np.flatnonzero(levels["bucket_edges"] > 0)]
        per_level = [dev() for _ in live]
        loop(live, per_level)                                     # warm-up, and the labels to check against
        same = all(bool(torch.equal(torch.from_numpy(eng.consensus_cut(s)[0]).to("cuda:0"), per_level[i]))
                   for i, s in enumerate(live))
        del per_level
        ph = {k: [] for k in PHASES}
        wall_h, wall_l, dev_l = [], [], []
        for _ in range(args.repeats):
            L.fc_synchronize(ctx)
            t0 = time.perf_counter()
            hierarchy()
            wall_h.append(time.perf_counter() - t0)
            for k, x in eng.consensus_levels_timing().items():
                ph[k].append(x * 1e-3)
            L.fc_synchronize(ctx)
            t0 = time.perf_counter()
            d = loop(live)
            wall_l.append(time.perf_counter() - t0)
            dev_l.append(d)
        eng.collect_timing()
        eng.set_timing(False)

    k = levels["k"].astype(np.int64)
    absorbed = np.concatenate([k[1:] - k[:-1], [n - k[-1]]])       # roots that level s took away
    nbytes = phase_bytes(n, m_in, len(live), int(absorbed.sum()))
    phases = {}
    for name in PHASES:
        t = float(np.median(ph[name]))
        phases[name] = dict(rng(ph[name]), bytes_model=nbytes[name], bytes_per_s=nbytes[name] / t if t > 0 else None,
                            frac_of_hbm_peak=nbytes[name] / t / HBM_PEAK if t > 0 else None)
    dev_h = [sum(ph[name][i] for name in PHASES) for i in range(args.repeats)]
    out = {
        "workload": {"n": n, "m_input": int(m_in), "mu": args.mu, "algo": "louvain", "n_p": n_p, "seed": args.seed,
                     "run_iterations": int(stats["iterations"])},
        "library": built_hash(),
        "protocol": "support taken once; 1 warm-up of each side, then %d rounds alternating one fc_consensus_levels "
                    "call with one fc_consensus_partition call per nonempty level at theta_of(level); device times "
                    "from the in-library HIP events, whole calls on the host clock around calls that end in a "
                    "device synchronise" % args.repeats,
        "nonempty_levels": len(live),
        "levels_equal_loop_labels": bool(same),
        "best_level": int(best.value),
        "levels": {f: [float(x) if f == "modularity" else int(x) for x in levels[f]]
                   for f in ("bucket_edges", "k", "max_size", "singletons", "in_weight", "modularity")},
        "absorbed_roots_per_level": [int(x) for x in absorbed],
        "flatten_nodes_read_per_level": n,
        "hierarchy": {"phases": phases, "device_s": rng(dev_h), "host_clock_s": rng(wall_h)},
        "loop_of_partitions": {"device_s": rng(dev_l), "host_clock_s": rng(wall_l), "calls": len(live)},
        "ratio_loop_over_hierarchy": {"device": float(np.median(dev_l) / np.median(dev_h)),
                                      "host_clock": float(np.median(wall_l) / np.median(wall_h))},
        "hierarchy_is_faster": bool(np.median(wall_l) > np.median(wall_h)),
        "hbm_peak_bytes_per_s": HBM_PEAK,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
