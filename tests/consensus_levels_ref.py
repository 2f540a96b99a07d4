"""CPU reference of the consensus hierarchy (fc_consensus_levels / fc_consensus_cut): numpy and a
Python union-find that takes the edges in descending support, on top of tests/consensus_ref.py.
Everything is an exact integer; `modularity` restates the library's rounding (the two integers
converted to the x86 extended format, divided there, then rounded to float64)."""
from fractions import Fraction

import numpy as np


def level_of(theta, n_total):
    """smallest integer s with not (float(s) < theta * float(n_total))"""
    cut = float(theta) * float(n_total)
    s = 0
    while float(s) < cut:
        s += 1
    return s


def theta_of(level, n_total):
    return (level - 0.5) / n_total if level >= 1 else 0.0


def tree(n, u, v, sup, n_total):
    """(birth, up) int32[n].  root_s(t) is the smallest node of t's component at level s (the edges
    with support >= s); birth[t] = the largest s with root_s(t) != t (-1: never), up[t] =
    root_birth(t).  The union-find hooks the larger root under the smaller, so a node stops being
    a root exactly at its birth level; its `up` is read once that level's edges are all in."""
    u = np.asarray(u, np.int64)
    v = np.asarray(v, np.int64)
    sup = np.asarray(sup, np.int64)
    assert len(sup) == 0 or (sup.min() >= 0 and sup.max() <= n_total)
    parent = list(range(n))
    birth = np.full(n, -1, np.int32)
    up = np.arange(n, dtype=np.int32)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    order = np.argsort(-sup, kind="stable")
    su, sv, ss = u[order].tolist(), v[order].tolist(), sup[order].tolist()
    i, m = 0, len(ss)
    while i < m:
        s = ss[i]
        born = []
        while i < m and ss[i] == s:
            a, b = find(su[i]), find(sv[i])
            if a != b:
                hi, lo = max(a, b), min(a, b)
                parent[hi] = lo
                born.append(hi)
            i += 1
        for t in born:
            birth[t] = s
            up[t] = find(t)
    return birth, up


def cut(birth, up, level):
    """labels int32[n] of level `level`: walk up while birth >= level, number the roots in node order"""
    birth = np.asarray(birth)
    up = np.asarray(up, np.int64)
    x = np.arange(len(birth), dtype=np.int64)
    while True:
        go = birth[x] >= level
        if not go.any():
            break
        x[go] = up[x[go]]
    rank = np.cumsum(x == np.arange(len(birth))) - 1
    return rank[x].astype(np.int32)


def join_levels(u, v, birth, up):
    """j(e) int64[m]: the largest level at which e's ends share a component (-1: never).  With
    birth[a] >= birth[b]: j(a, b) = min(birth[a], j(up[a], b))."""
    birth = np.asarray(birth, np.int64)
    up = np.asarray(up, np.int64)
    a = np.asarray(u, np.int64).copy()
    b = np.asarray(v, np.int64).copy()
    j = np.full(len(a), np.iinfo(np.int64).max, np.int64)
    while True:
        live = np.flatnonzero((a != b) & (j >= 0))
        if not len(live):
            break
        la, lb = a[live], b[live]
        step_a = birth[la] >= birth[lb]
        x = np.where(step_a, la, lb)
        j[live] = np.minimum(j[live], birth[x])                 # -1 when both are roots of H
        a[live] = np.where(step_a, up[la], la)
        b[live] = np.where(step_a, lb, up[lb])
    return j


def _round_bits(x, bits):
    """the Fraction x rounded to `bits` significant bits, ties to even"""
    if x == 0:
        return x
    if x < 0:
        return -_round_bits(-x, bits)
    e = x.numerator.bit_length() - x.denominator.bit_length() - bits
    while x >= Fraction(2) ** (e + bits):
        e += 1
    while x < Fraction(2) ** (e + bits - 1):
        e -= 1
    scaled = x / Fraction(2) ** e
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return n * Fraction(2) ** e


def modularity(in_weight, tot_sq, w2):
    """(double)((long double)(2 in W2 - tot_sq) / (long double)(W2 W2)), 64-bit significands"""
    if w2 == 0:
        return 0.0
    num = _round_bits(Fraction(2 * in_weight * w2 - tot_sq), 64)
    den = _round_bits(Fraction(w2 * w2), 64)
    return float(_round_bits(_round_bits(num / den, 64), 53))


FIELDS = ("bucket_edges", "k", "max_size", "singletons", "in_weight", "tot_sq", "modularity", "key")


def level_records(n, u, v, sup, n_total, w=None, birth=None, up=None):
    """One dict per level 0..n_total (FIELDS; tot_sq and key = 2 in_weight W2 - tot_sq as Python
    ints).  Sizes and degree sums follow a second union-find from the top level down; in_weight is
    the weight of the edges with j(e) >= s."""
    u = np.asarray(u, np.int64)
    v = np.asarray(v, np.int64)
    sup = np.asarray(sup, np.int64)
    w = np.ones(len(u), np.int64) if w is None else np.asarray(w, np.int64)
    if birth is None:
        birth, up = tree(n, u, v, sup, n_total)
    deg = np.zeros(n, np.int64)
    np.add.at(deg, u, w)
    np.add.at(deg, v, w)
    w2 = int(deg.sum())
    jw = np.zeros(n_total + 1, np.int64)
    j = join_levels(u, v, birth, up)
    np.add.at(jw, j[j >= 0], w[j >= 0])
    hist = np.bincount(sup, minlength=n_total + 1)
    parent = list(range(n))
    size = [1] * n
    tot = [int(d) for d in deg]

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    order = np.argsort(-sup, kind="stable")
    su, sv, ss = u[order].tolist(), v[order].tolist(), sup[order].tolist()
    k, mx, single, inw = n, 1, n, 0
    tot_sq = sum(t * t for t in tot)
    out = [None] * (n_total + 1)
    i = 0
    for s in range(n_total, -1, -1):
        while i < len(ss) and ss[i] == s:
            a, b = find(su[i]), find(sv[i])
            if a != b:
                hi, lo = max(a, b), min(a, b)
                parent[hi] = lo
                single -= (size[hi] == 1) + (size[lo] == 1)
                tot_sq += 2 * tot[hi] * tot[lo]
                size[lo] += size[hi]
                tot[lo] += tot[hi]
                mx = max(mx, size[lo])
                k -= 1
            i += 1
        inw += int(jw[s])
        out[s] = {"bucket_edges": int(hist[s]), "k": k, "max_size": mx, "singletons": single, "in_weight": inw,
                  "tot_sq": tot_sq, "modularity": modularity(inw, tot_sq, w2), "key": 2 * inw * w2 - tot_sq}
    return out


def best_level(records):
    """the level of the largest key; the highest level among equal keys"""
    best = max(r["key"] for r in records)
    return max(s for s, r in enumerate(records) if r["key"] == best)
