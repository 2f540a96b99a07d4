"""Numpy / Python-int restatement of the scoring definitions of include/fastconsensus_amd.h
(fc_part_score, fc_pair_score) -- TEST INFRASTRUCTURE ONLY.  Integer sums are Python ints, the
modularity and the ARI are exact rationals rounded once."""
from fractions import Fraction
from math import log

import numpy as np


def compact(x):
    return np.unique(np.asarray(x), return_inverse=True)[1].ravel().astype(np.int64)


def _s_log(counts):
    c = counts[counts > 1].astype(np.float64)
    return float(np.sum(c * np.log(c)))


def part(labels, u=None, v=None, w=None):
    """k, max_size, sum_sq, s_log, entropy and -- with the edges (u, v[, w]) of an undirected
    graph, each once -- in_weight, tot_sq and modularity."""
    lab = compact(labels)
    n = lab.size
    sizes = np.bincount(lab)
    out = {"k": int(sizes.size), "max_size": int(sizes.max()), "sum_sq": sum(int(s) ** 2 for s in sizes),
           "s_log": _s_log(sizes)}
    out["entropy"] = log(n) - out["s_log"] / n
    if u is not None:
        u, v = np.asarray(u), np.asarray(v)
        w = np.ones(len(u), np.int64) if w is None else np.asarray(w, np.int64)
        same = lab[u] == lab[v]
        out["in_weight"] = int(w[same].sum())
        kdeg = np.zeros(n, np.int64)
        np.add.at(kdeg, u, w)
        np.add.at(kdeg, v, w)
        tot = np.zeros(sizes.size, np.int64)
        np.add.at(tot, lab, kdeg)
        out["tot_sq"] = sum(int(t) ** 2 for t in tot)
        w2 = int(kdeg.sum())
        out["modularity"] = float(Fraction(2 * out["in_weight"] * w2 - out["tot_sq"], w2 * w2)) if w2 else 0.0
    return out


def pair(a, b):
    """cells, sum_sq, s_log, mi, nmi, ari of the contingency table of two labelings."""
    ia, ib = compact(a), compact(b)
    n = ia.size
    kb = int(ib.max()) + 1
    cnt = np.unique(ia * kb + ib, return_counts=True)[1]
    pa, pb = part(a), part(b)
    out = {"cells": int(cnt.size), "sum_sq": sum(int(x) ** 2 for x in cnt), "s_log": _s_log(cnt)}
    mi = log(n) + (out["s_log"] - pa["s_log"] - pb["s_log"]) / n
    out["mi"] = mi = max(mi, 0.0)
    out["h_mean"] = (pa["entropy"] + pb["entropy"]) / 2
    out["nmi"] = 1.0 if pa["k"] == 1 and pb["k"] == 1 else (mi / out["h_mean"] if mi > 0 else 0.0)
    s_ij, s_a, s_b, t = (out["sum_sq"] - n) // 2, (pa["sum_sq"] - n) // 2, (pb["sum_sq"] - n) // 2, n * (n - 1) // 2
    num, den = 2 * (s_ij * t - s_a * s_b), (s_a + s_b) * t - 2 * s_a * s_b
    out["ari"] = 1.0 if den == 0 else float(Fraction(num, den))
    return out


def float_bound(n):
    """Absolute error bound of entropy and mi: recursive summation of three sums of <= n
    non-negative terms <= ln n each, plus one ulp per logarithm."""
    return 4 * n * 2.0 ** -53 * log(n)
