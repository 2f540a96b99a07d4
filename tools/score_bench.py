"""Time the device scoring on the headline workload: LFR-1M (mu 0.5), louvain, n_p = 64.

    python tools/score_bench.py [--n 1000000] [--n-p 64] [--repeats 5] [--out profiles/score_lfr1m_np64.json]

One fast_consensus run leaves 64 labelings on the device; then fc_score_partitions and the
all-pairs fc_score_pairs are timed apart: one warm-up call each, `repeats` timed calls, the median,
fc_synchronize before and after each timed region (both calls also end in a device synchronise).
The host baseline is tests/dist_gates.nmi on 8 sampled pairs, scaled to the pair count
(extrapolated, and labelled so).  labT bytes: the labels of the wanted lanes (see main).
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


def timed(eng, fn, repeats):
    fn()                                             # warm-up: buffers allocated, code objects loaded
    out = []
    for _ in range(repeats):
        eng._L.fc_synchronize(eng._ctx)
        t0 = time.perf_counter()
        res = fn()
        eng._L.fc_synchronize(eng._ctx)
        out.append(time.perf_counter() - t0)
    return res, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--mu", type=float, default=0.5)
    ap.add_argument("--n-p", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_lfr1m_np64.json"))
    args = ap.parse_args()

    import fastconsensus_amd as fc
    from fastconsensus_amd import synth
    from fastconsensus_amd.build import built_hash
    from fastconsensus_amd.core import store_order_pays
    from tests import dist_gates

    u, v, planted = synth.lfr(args.n, args.mu, seed=args.seed)
    n_p = args.n_p
    with fc.Engine(seed=args.seed) as eng:
        eng.set_option("store", store_order_pays(n_p, 0))
        eng.load_graph(args.n, u, v)
        labels, stats = eng.run(0, n_p, 0.2, 0.02)
        part, t_part = timed(eng, lambda: eng.score_partitions("input"), args.repeats)
        rec, t_pairs = timed(eng, eng.score_pairs, args.repeats)
        eng.set_reference(planted)
        truth, t_truth = timed(eng, lambda: eng.score_pairs(
            np.stack([np.full(n_p, -1), np.arange(n_p)], 1)), args.repeats)
    npairs = len(rec)
    ldT = (n_p + 3) & ~3
    # row a of the all-pairs call reads only the lanes b > a (the others issue no load): the
    # bytes asked for are sum_a (n_p - 1 - a) labels per vertex; whole rows (ldT labels, what a
    # pass costs when every lane is wanted) are the upper figure
    labt_bytes = args.n * 4 * (n_p * (n_p - 1) // 2)
    labt_bytes_rows = (n_p - 1) * args.n * ldT * 4
    med_pairs, med_part = float(np.median(t_pairs)), float(np.median(t_part))

    rng = np.random.default_rng(0)
    sample = rng.choice(npairs, size=min(args.host_pairs, npairs), replace=False)
    t0 = time.perf_counter()
    host = [dist_gates.nmi(labels[rec["a"][i]], labels[rec["b"][i]]) for i in sample]
    host_s = (time.perf_counter() - t0) / len(sample)
    err = max(abs(h - rec["nmi"][i]) for h, i in zip(host, sample))

    out = {
        "workload": {"n": args.n, "m": int(len(u)), "mu": args.mu, "algo": "louvain", "n_p": n_p, "seed": args.seed,
                     "run_iterations": int(stats["iterations"])},
        "library": built_hash(),
        "protocol": "1 warm-up + %d timed calls each, median; fc_synchronize around each" % args.repeats,
        "score_partitions_s": {"median": med_part, "all": t_part},
        "score_pairs_s": {"median": med_pairs, "all": t_pairs, "pairs": npairs},
        "score_truth_pairs_s": {"median": float(np.median(t_truth)), "all": t_truth, "pairs": int(len(truth))},
        "labT_bytes_model": "wanted lanes only: n * 4 * n_p (n_p - 1) / 2; whole_rows = (n_p - 1) * n * ldT * 4",
        "labT_bytes_per_call": labt_bytes,
        "labT_bytes_per_s": labt_bytes / med_pairs,
        "labT_frac_of_hbm_peak_whole_call": labt_bytes / med_pairs / HBM_PEAK,
        "labT_bytes_per_call_whole_rows": labt_bytes_rows,
        "labT_frac_of_hbm_peak_whole_rows": labt_bytes_rows / med_pairs / HBM_PEAK,
        "fallback_share_of_vertices": float(rec["slow_members"].sum()) / (npairs * args.n),
        "pairs_with_fallback": int((rec["slow_members"] > 0).sum()),
        "mean_pairwise_nmi": float(rec["nmi"].mean()),
        "mean_modularity": float(part["modularity"].mean()),
        "mean_nmi_truth": float(truth["nmi"].mean()),
        "host_baseline": {"what": "tests/dist_gates.nmi, %d sampled pairs, EXTRAPOLATED to %d pairs" % (len(sample), npairs),
                          "s_per_pair": host_s, "extrapolated_s": host_s * npairs,
                          "max_abs_nmi_difference": float(err)},
        "speedup_vs_host_extrapolated": host_s * npairs / med_pairs,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
