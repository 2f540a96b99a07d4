"""Numpy restatement of the cluster merges (fc_community_graph, fc_cluster_coassoc,
core.merge_moves, core.merge_refine), written independently of core.py: dense per-replica
contingency tables (median_ref.tables) and plain loops for the selection -- TEST INFRASTRUCTURE
ONLY.  Everything is a Python int.

    X(a, b)    = sum_r sum_d C_r[a][d] C_r[b][d]
    gain(a, b) = 2 X(a, b) - R s_a s_b
    F(P with a and b joined) - F(P) = 2 gain(a, b)
"""
import numpy as np

from tests import median_ref


def community_graph(N, u, v, w, part):
    """Edges (u, v, w) of an undirected graph in node ids, each once, no loops (w None: all 1);
    part: [N], any integer ids.  The dict of Engine.community_graph: the cluster pairs a < b joined
    by an edge, ascending by (a, b), with the joining edges' summed weight and their number."""
    part = np.asarray(part, np.int64)
    assert part.shape == (N,)
    w = [1] * len(u) if w is None else np.asarray(w).tolist()
    acc = {}
    for x, y, z in zip(np.asarray(u).tolist(), np.asarray(v).tolist(), w):
        a, b = int(part[x]), int(part[y])
        if a == b:
            continue
        key = (min(a, b), max(a, b))
        cell = acc.setdefault(key, [0, 0])
        cell[0] += int(z)
        cell[1] += 1
    keys = sorted(acc)
    return {"a": np.array([k[0] for k in keys], np.int32), "b": np.array([k[1] for k in keys], np.int32),
            "weight": np.array([acc[k][0] for k in keys], np.int64),
            "edges": np.array([acc[k][1] for k in keys], np.int64), "npairs": len(keys)}


def cross(labs, part, a, b):
    """int64 [npairs]: X(a[p], b[p]); 0 when an id does not occur"""
    C, _ = median_ref.tables(labs, part)
    rows = C[0].shape[0]
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    ok = (a < rows) & (b < rows)
    out = np.zeros(len(a), np.int64)
    for t in C:
        out[ok] += (t[a[ok]] * t[b[ok]]).sum(1)
    return out


def moves(part, a, b, x, R):
    """One round of the selection rule on the candidate pairs (a[p], b[p]) with x[p] = X(a, b): the
    dict of core.merge_moves (labels int32, gain, proposed, accepted)."""
    part = [int(p) for p in np.asarray(part).tolist()]
    size = {}
    for p in part:
        size[p] = size.get(p, 0) + 1
    seen, kept = set(), []
    for ca, cb, cx in zip(np.asarray(a).tolist(), np.asarray(b).tolist(), np.asarray(x).tolist()):
        lo, hi = min(ca, cb), max(ca, cb)
        if lo == hi or (lo, hi) in seen:
            continue
        seen.add((lo, hi))
        gain = 2 * int(cx) - R * size.get(lo, 0) * size.get(hi, 0)
        if gain > 0:
            kept.append((-gain, lo, hi))
    kept.sort()
    used, into, total, accepted = set(), {}, 0, 0
    for g, lo, hi in kept:
        if lo in used or hi in used:
            continue
        used.update((lo, hi))
        into[hi] = lo
        total -= g
        accepted += 1
    return {"labels": np.array([into.get(p, p) for p in part], np.int32), "gain": total, "proposed": len(kept),
            "accepted": accepted}


def refine(labs, part, N, u, v, max_rounds=64, w=None):
    """core.merge_refine with the community graph of (u, v, w) as the candidates; the objective of
    every round is evaluated directly (median_ref.objective), so the dict also proves the
    additivity.  Returns labels, rounds, converged, objective, pairs_per_round, proposed_per_round,
    accepted_per_round, gain_per_round, k_per_round."""
    labs = np.asarray(labs, np.int64)
    part = np.asarray(part, np.int32)
    R = len(labs)
    objective = [median_ref.objective(labs, part)]
    ks = [len(np.unique(part))]
    pairs, proposed, accepted, gains = [], [], [], []
    converged = False
    while len(accepted) < max_rounds:
        cg = community_graph(N, u, v, w, part)
        mv = moves(part, cg["a"], cg["b"], cross(labs, part, cg["a"], cg["b"]), R)
        if mv["accepted"] == 0:
            converged = True
            break
        part = mv["labels"]
        pairs.append(cg["npairs"]); proposed.append(mv["proposed"]); accepted.append(mv["accepted"])
        gains.append(mv["gain"])
        objective.append(median_ref.objective(labs, part))
        ks.append(len(np.unique(part)))
    return {"labels": part, "rounds": len(accepted), "converged": converged, "objective": objective,
            "pairs_per_round": pairs, "proposed_per_round": proposed, "accepted_per_round": accepted,
            "gain_per_round": gains, "k_per_round": ks}
