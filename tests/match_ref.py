"""CPU reference of fc_cluster_match, written from the definition: for a partition P with clusters k
of size s_k and a labeling r with community sizes t_r(d) and contingency cells C_r[k][d] (the
members of k that r labels d),

    J_r(k, d) = C / (s_k + t_r(d) - C)                      best_r(k) = the d of largest J_r(k, d)
    inter[r][k] = C_r[k][best_r(k)]                         csize[r][k] = t_r(best_r(k))

The cells come from np.unique on the (P, lab_r) pairs, the sizes from bincount, and the choice is
made on Python integers: C1 * U2 against C2 * U1 with U = s + t - C, among equal fractions the larger
C.  The derived helpers are restated here independently of fastconsensus_amd.core (the same float64
operations on the same integers, so the results compare with ==)."""
import numpy as np


def better(s, c1, t1, c2, t2):
    """(c1, t1) beats (c2, t2) as the match of a cluster of s members (Python ints, no overflow)"""
    a, b = c1 * (s + t2 - c2), c2 * (s + t1 - c1)
    return a > b or (a == b and c1 > c2)


def match(labs, part):
    """labs [n_r][n] (or [n]: one row), part [n] (any integer ids).  Returns ids (the distinct ids,
    ascending), size int64[K], inter int32[n_r][K], csize int32[n_r][K]."""
    labs = np.atleast_2d(np.asarray(labs))
    part = np.asarray(part)
    ids, dense, size = np.unique(part, return_inverse=True, return_counts=True)
    dense = dense.reshape(-1).astype(np.int64)
    k = len(ids)
    inter = np.zeros((len(labs), k), np.int32)
    csize = np.zeros((len(labs), k), np.int32)
    for r, row in enumerate(labs):
        _, d = np.unique(row, return_inverse=True)
        d = d.reshape(-1).astype(np.int64)
        t = np.bincount(d)
        nd = len(t)
        cell, cnt = np.unique(dense * nd + d, return_counts=True)     # the nonempty (cluster, label) cells
        best = [(0, 0)] * k
        for x, c in zip(cell.tolist(), cnt.tolist()):
            kk, dd = divmod(x, nd)
            if better(int(size[kk]), c, int(t[dd]), *best[kk]):
                best[kk] = (c, int(t[dd]))
        inter[r] = [b[0] for b in best]
        csize[r] = [b[1] for b in best]
    return ids, size.astype(np.int64), inter, csize


def jaccard(inter, size, csize):
    inter, size, csize = (np.asarray(x).astype(np.int64) for x in (inter, size, csize))
    return inter / (size + csize - inter)


def f1(inter, size, csize):
    inter, size, csize = (np.asarray(x).astype(np.int64) for x in (inter, size, csize))
    return 2 * inter / (size + csize)


def stability(inter, size, csize):
    return np.atleast_2d(jaccard(inter, size, csize)).mean(axis=0)


def recovered(inter, size, csize, num=3, den=4):
    """rows with J >= num / den per cluster, on Python integers"""
    inter, csize = np.atleast_2d(inter), np.atleast_2d(csize)
    return np.array([sum(den * int(c) >= num * (int(s) + int(t) - int(c)) for c, t in zip(inter[:, k], csize[:, k]))
                     for k, s in enumerate(np.asarray(size).tolist())], np.int64)


def dissolved(inter, size, csize, num=1, den=2):
    """rows with J <= num / den per cluster, on Python integers"""
    inter, csize = np.atleast_2d(inter), np.atleast_2d(csize)
    return np.array([sum(den * int(c) <= num * (int(s) + int(t) - int(c)) for c, t in zip(inter[:, k], csize[:, k]))
                     for k, s in enumerate(np.asarray(size).tolist())], np.int64)


def summary(inter, size, csize):
    return {"jaccard": jaccard(inter, size, csize), "f1": f1(inter, size, csize),
            "stability": stability(inter, size, csize), "recovered": recovered(inter, size, csize),
            "dissolved": dissolved(inter, size, csize)}


def exact_tie(n, a_low):
    """The exact tie on n >= 16 nodes: one cluster of 4 members (nodes 0..3) and a cluster of the
    rest.  Community A holds member 0 alone (size 1, J = 1/4); community B holds members 1, 2 and
    four outsiders (size 6, J = 2/8); member 3 sits with every other outsider.  a_low: A's label
    below B's, else above.  Returns part, lab; the answer for cluster 0 is (2, 6): the larger C."""
    part = np.array([0] * 4 + [1] * (n - 4))
    la, lb = (2, 9) if a_low else (9, 2)
    lab = np.full(n, 5)
    lab[0] = la
    lab[[1, 2, 4, 5, 6, 7]] = lb
    return part, lab


def near_tie(n=16000):
    """The near-tie that float32 cannot see: one cluster of 8001 members; community A has C = 4000
    of them and 3998 outsiders (t = 7998), community B C = 4001 and 4001 outsiders (t = 8002);
    4000 * 12002 - 4001 * 11999 = 1, so A wins by one part in 5e7, while float32(4000) / float32(11999)
    == float32(4001) / float32(12002) and the larger-C rule would then pick B.  The other 7999 nodes
    are clusters of their own.  The four numbers use up all 16000 nodes, so the labeling has exactly
    these two communities.  Returns part, lab (0 = A, 1 = B); the answer for the big cluster is
    (4000, 7998)."""
    assert n == 16000
    part = np.empty(n, np.int64)
    part[:8001] = 0
    part[8001:] = np.arange(1, 8000)
    lab = np.empty(n, np.int64)
    lab[:4000] = 0
    lab[4000:8001] = 1
    lab[8001:8001 + 3998] = 0
    lab[8001 + 3998:] = 1
    return part, lab
