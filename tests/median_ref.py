"""Numpy restatement of the median-partition refinement (fc_item_affinity, core.median_moves,
core.median_refine), written independently of core.py: dense per-replica contingency tables and
plain loops for the selection.  Everything is a Python int.

    aff(v, k)   = sum_r C_r[k][lab_r(v)]
    F(P)        = 2 sum_r sum_{k,d} C_r[k][d]^2 - R sum_k s_k^2
    gain(v->b)  = (2 aff(v, b) - R s_b) - (2 (aff(v, P(v)) - R) - R (s_P(v) - 1))
"""
import numpy as np

from tests import vote_ref


def tables(labs, part):
    """(C, dense): C[r][k, d] = the members of cluster k that replica r labels d, with the
    replica's labels renumbered densely (dense[r], so that a table has one column per community)"""
    labs, part = np.asarray(labs, np.int64), np.asarray(part, np.int64)
    rows = int(part.max()) + 1
    C, dense = [], []
    for lab in labs:
        d = np.unique(lab, return_inverse=True)[1].reshape(-1)
        t = np.zeros((rows, int(d.max()) + 1), np.int64)
        np.add.at(t, (part, d), 1)
        C.append(t)
        dense.append(d)
    return C, np.array(dense)


def affinity(labs, part, nodes, clusters):
    """int64 [npairs]: aff(nodes[p], clusters[p]); 0 for a cluster id that does not occur"""
    C, labs = tables(labs, part)
    out = np.zeros(len(nodes), np.int64)
    for p, (v, k) in enumerate(zip(np.asarray(nodes).tolist(), np.asarray(clusters).tolist())):
        if k < C[0].shape[0]:
            out[p] = sum(int(C[r][k, labs[r, v]]) for r in range(len(labs)))
    return out


def objective(labs, part):
    """F(P) as a Python int"""
    labs = np.asarray(labs, np.int64)
    agree = sum(int((t * t).sum()) for t in tables(labs, part)[0])
    size = np.bincount(np.asarray(part, np.int64))
    return 2 * agree - len(labs) * int((size * size).sum())


def sum_sq(labs):
    """T: the replicas' summed squared community sizes"""
    return sum(int((np.bincount(np.asarray(lab, np.int64)) ** 2).sum()) for lab in np.asarray(labs))


def mean_rand(F, T, n, R):
    return 1.0 if n < 2 else 1.0 - (T - F) / (R * n * (n - 1))


def moves(labs, part, nodes, clusters):
    """One round of the selection rule on the candidates (nodes[p], clusters[p]): the dict of
    core.median_moves (labels int32, gain, proposed, accepted, alone)."""
    labs, part = np.asarray(labs, np.int64), np.asarray(part, np.int64)
    R, n = labs.shape
    C, labs = tables(labs, part)
    size = np.bincount(part, minlength=n).tolist()
    part_l = part.tolist()
    targets = {v: set() for v in range(n)}             # every node may go alone
    for v, b in zip(np.asarray(nodes).tolist(), np.asarray(clusters).tolist()):
        if not 0 <= b < n or size[b] == 0:
            raise ValueError("candidate cluster %d does not occur" % b)
        if b != part_l[v]:
            targets[v].add(b)

    def aff(v, k):
        return sum(int(C[r][k, labs[r, v]]) for r in range(R))

    kept = []
    for v in sorted(targets):
        a = part_l[v]
        own = 2 * (aff(v, a) - R) - R * (size[a] - 1)
        best_g, best_b = None, None
        for b in sorted(targets[v]):                    # ascending: the smallest id keeps a tie
            g = 2 * aff(v, b) - R * size[b] - own
            if best_g is None or g > best_g:
                best_g, best_b = g, b
        if size[a] > 1 and (best_g is None or -own > best_g):   # alone loses a tie to a cluster
            best_g, best_b = -own, None
        if best_g is not None and best_g > 0:
            kept.append((v, best_b, best_g))
    kept.sort(key=lambda m: (-m[2], m[0]))
    winner = {}
    for i, (v, b, g) in enumerate(kept):
        winner.setdefault(part_l[v], i)
        if b is not None:
            winner.setdefault(b, i)
    new = part.copy()
    gain, accepted, solo = 0, 0, []
    for i, (v, b, g) in enumerate(kept):
        if winner[part_l[v]] != i or (b is not None and winner[b] != i):
            continue
        accepted += 1
        gain += g
        if b is None:
            solo.append(v)
        else:
            new[v] = b
    free = [c for c in range(n) if size[c] == 0]
    for v, c in zip(sorted(solo), free):
        new[v] = c
    return {"labels": new.astype(np.int32), "gain": gain, "proposed": len(kept), "accepted": accepted,
            "alone": len(solo)}


def refine(labs, part, max_rounds=64):
    """core.median_refine with the default candidates (v, top[v]) of vote_ref.vote"""
    labs = np.asarray(labs, np.int64)
    part = np.asarray(part, np.int64)
    R, n = labs.shape
    obj = [objective(labs, part)]
    proposed, accepted, alone, gains = [], [], [], []
    converged = False
    while len(accepted) < max_rounds:
        top = vote_ref.vote(labs, part)["top"]
        nodes = np.flatnonzero(top != part)
        mv = moves(labs, part, nodes, top[nodes])
        if mv["accepted"] == 0:
            converged = True
            break
        proposed.append(mv["proposed"]); accepted.append(mv["accepted"]); alone.append(mv["alone"])
        gains.append(mv["gain"])
        part = mv["labels"].astype(np.int64)
        obj.append(objective(labs, part))
    T = sum_sq(labs)
    return {"labels": part.astype(np.int32), "rounds": len(accepted), "converged": converged, "objective": obj,
            "proposed_per_round": proposed, "accepted_per_round": accepted, "alone_per_round": alone,
            "gain_per_round": gains, "mean_rand": (mean_rand(obj[0], T, n, R), mean_rand(obj[-1], T, n, R))}
