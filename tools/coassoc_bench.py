"""Time the co-association calls on the headline workload: LFR-1M (mu 0.5), louvain, n_p = 64.

    python tools/coassoc_bench.py [--n 1000000] [--n-p 64] [--repeats 11]
                                  [--out profiles/coassoc_lfr1m_np64.json]

One fast_consensus run leaves 64 labelings on the device.  Then, with the engine's timing on, each
line is one warm-up call and `repeats` timed calls, the median of the `count` phase the library
brackets with HIP events (fc_coassoc_timing):
  * the matrix of k = 1024, 4096, 16384 random nodes, and beside each the WRITE FLOOR: the call's
    time over a hipMemsetAsync of the same output buffer (HIP events on the caller's stream, same
    protocol) -- the cheapest way to touch every output byte once;
  * the histogram of k = 16384 and 65536 random nodes (no matrix);
  * 10 M random node pairs, and beside it the PAIR FLOOR: its time per pair over that of
    fc_consensus_support("input") per edge -- the same count kernel fed sorted edge ends instead of
    random pairs, so the ratio is what random rows cost.
Nothing is gated: the parent commit has no such call to compare against.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes/s, the figure DESIGN.md's roofline table uses


def hip_runtime():
    """The HIP runtime torch has loaded (for hipMemsetAsync)."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    if not paths:
        raise RuntimeError("no HIP runtime loaded")
    lib = ctypes.CDLL(paths[0])
    lib.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    lib.hipMemsetAsync.restype = ctypes.c_int
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--mu", type=float, default=0.5)
    ap.add_argument("--n-p", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--matrix-k", type=int, nargs="*", default=[1024, 4096, 16384])
    ap.add_argument("--hist-k", type=int, nargs="*", default=[16384, 65536])
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coassoc_lfr1m_np64.json"))
    args = ap.parse_args()
    if args.repeats < 10:
        raise SystemExit("--repeats must be at least 10")

    import torch

    import fastconsensus_amd as fc
    from fastconsensus_amd import synth
    from fastconsensus_amd.build import built_hash
    from fastconsensus_amd.core import store_order_pays

    u, v, _ = synth.lfr(args.n, args.mu, seed=args.seed)
    n_p = args.n_p
    ldT = (n_p + 3) & ~3
    rng = np.random.default_rng(args.seed)
    med = lambda xs: float(np.median(xs))
    hip = hip_runtime()
    out = {"matrix": [], "hist": []}
    with fc.Engine(seed=args.seed) as eng:
        eng.set_option("store", store_order_pays(n_p, 0))
        eng.load_graph(args.n, u, v)
        _, stats = eng.run(0, n_p, 0.2, 0.02)
        _, _, m_in = eng.graph_info()
        eng.set_timing(True)

        def timed(call):
            call()                                                # warm-up: buffers, code objects
            eng.collect_timing()
            ts = []
            for _ in range(args.repeats):
                call()
                ts.append(eng.coassoc_timing()["count"] * 1e-3)
                eng.collect_timing()                              # hands the events back to the pool
            return ts

        check = None
        for k in args.matrix_k:
            nodes = rng.choice(args.n, k, replace=False)
            buf = torch.empty(k * k, dtype=torch.int32, device="cuda:0")
            ts = timed(lambda: eng.coassociation(nodes, dev_out=buf))
            stream = torch.cuda.current_stream()
            tm = []
            for i in range(args.repeats + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc = hip.hipMemsetAsync(buf.data_ptr(), 0, 4 * k * k, stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                assert rc == 0
                if i:
                    tm.append(e0.elapsed_time(e1) * 1e-3)
            nbytes_in, nbytes_out = 2 * k * 4 * ldT, 4 * k * k
            t = med(ts)
            out["matrix"].append({
                "k": k, "count_s": {"median": t, "all": ts}, "memset_s": {"median": med(tm), "all": tm},
                "write_floor_ratio": t / med(tm), "bytes_in": nbytes_in, "bytes_out": nbytes_out,
                "bytes_per_s": (nbytes_in + nbytes_out) / t, "frac_of_hbm_peak": (nbytes_in + nbytes_out) / t / HBM_PEAK,
                "pair_replica_compares_per_s": k * k * n_p / t})
            if k == args.matrix_k[-1]:                            # the histogram of the same list from the matrix
                mat = eng.coassociation(nodes, dev_out=buf)
                iu = torch.triu_indices(k, k, offset=1, device="cuda:0")
                from_matrix = torch.bincount(mat[iu[0], iu[1]].to(torch.int64), minlength=n_p + 1).cpu().numpy()
                check = bool(np.array_equal(from_matrix, eng.coassoc_hist(nodes)))
                del mat, iu
            del buf
            torch.cuda.empty_cache()

        for k in args.hist_k:
            nodes = rng.choice(args.n, k, replace=False)
            res = {}
            ts = timed(lambda: res.update(h=eng.coassoc_hist(nodes)))
            h = res["h"]
            t = med(ts)
            out["hist"].append({"k": k, "pairs": k * (k - 1) // 2, "count_s": {"median": t, "all": ts},
                                "pair_replica_compares_per_s": k * (k - 1) // 2 * n_p / t,
                                "pac": fc.pac(h), "hist_sum_ok": int(h.sum()) == k * (k - 1) // 2})

        prs = rng.integers(0, args.n, (args.pairs, 2)).astype(np.int32)
        pbuf = torch.empty(args.pairs, dtype=torch.int32, device="cuda:0")
        tp = timed(lambda: eng.coassoc_pairs(prs, dev_out=pbuf))
        sbuf = torch.empty(max(m_in, 1), dtype=torch.int32, device="cuda:0")
        eng.consensus_support("input", sbuf)
        eng.collect_timing()
        tsup = []
        for _ in range(args.repeats):
            eng.consensus_support("input", sbuf)
            tsup.append(eng.collect_timing()["consensus_ms"] * 1e-3)
        eng.set_timing(False)
    per_pair, per_edge = med(tp) / args.pairs, med(tsup) / m_in
    res = {
        "workload": {"n": args.n, "m_input": int(m_in), "mu": args.mu, "algo": "louvain", "n_p": n_p,
                     "seed": args.seed, "run_iterations": int(stats["iterations"])},
        "library": built_hash(),
        "protocol": "per line 1 warm-up + %d timed calls, the median; the count phase from HIP events at its "
                    "boundaries (fc_coassoc_timing); the memset from HIP events on the caller's stream; "
                    "consensus_support from the events of the consensus_ms slot" % args.repeats,
        "matrix": out["matrix"], "hist": out["hist"],
        "hist_equals_bincount_of_matrix": check,
        "pairs": {"npairs": args.pairs, "count_s": {"median": med(tp), "all": tp}, "s_per_pair": per_pair,
                  "consensus_support_input_s": {"median": med(tsup), "all": tsup}, "s_per_edge": per_edge,
                  "pair_floor_ratio": per_pair / per_edge,
                  "bytes_per_pair": 8 + 2 * 4 * ldT + 4, "bytes_per_s": (8 + 2 * 4 * ldT + 4) / per_pair},
        "hbm_peak_bytes_per_s": HBM_PEAK,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
