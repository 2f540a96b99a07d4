"""CPU reference of the consensus partition (fc_consensus_support / fc_consensus_partition):
plain numpy and a Python union-find.  Everything is an exact integer except `cut` (one float64
product) and `stability` (one float64 division of two integers per node)."""
import numpy as np


def canonical_edges(u, v):
    """Unique undirected edges without self loops, u < v, sorted by (u, v)."""
    u = np.asarray(u, np.int64)
    v = np.asarray(v, np.int64)
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    keep = lo != hi
    if not keep.any():
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    e = np.unique(np.stack([lo[keep], hi[keep]], 1), axis=0)
    return e[:, 0], e[:, 1]


def support(labels, u, v):
    """support(e) = number of labelings r with labels[r][u] == labels[r][v]; int64[m]."""
    labels = np.asarray(labels)
    out = np.zeros(len(u), np.int64)
    step = 1 << 18                                   # edges per slice: bounds the [n_r][slice] temporaries
    for lo in range(0, len(u), step):
        sl = slice(lo, lo + step)
        out[sl] = (labels[:, u[sl]] == labels[:, v[sl]]).sum(0)
    return out


def kept(sup, n_total, agreement):
    """The float64 keep rule: not (float(support) < agreement * float(n_total))."""
    cut = float(agreement) * float(n_total)
    return ~(np.asarray(sup).astype(np.float64) < cut), cut


def components(n, u, v):
    """Labels 0..k-1 of the connected components, numbered by each component's smallest node."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(np.asarray(u).tolist(), np.asarray(v).tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    root = np.fromiter((find(x) for x in range(n)), np.int64, count=n)   # the smallest node of the component
    is_root = root == np.arange(n)
    rank = np.cumsum(is_root) - 1
    return rank[root].astype(np.int32)


def stability(node_in, node_out):
    tot = node_in + node_out
    out = np.ones(len(tot), np.float64)
    nz = tot != 0
    out[nz] = node_in[nz] / tot[nz]
    return out


def partition(n, u, v, agreement, labels=None, sup=None, n_total=None):
    """u, v: the canonical edges of H (node ids).  Either `labels` [n_r][n] (support counted,
    n_total = n_r) or `sup` [m] with `n_total`.  Returns what Engine.consensus_partition does."""
    u = np.asarray(u, np.int64)
    v = np.asarray(v, np.int64)
    if sup is None:
        labels = np.asarray(labels)
        n_total = len(labels)
        sup = support(labels, u, v)
    sup = np.asarray(sup, np.int64)
    keep, cut = kept(sup, n_total, agreement)
    lab = components(n, u[keep], v[keep])
    hist = np.bincount(sup, minlength=n_total + 1).astype(np.int64)
    same = lab[u] == lab[v] if len(u) else np.zeros(0, bool)
    node_in = np.zeros(n, np.int64)
    node_out = np.zeros(n, np.int64)
    for end in (u, v):
        np.add.at(node_in, end[same], sup[same])
        np.add.at(node_out, end[~same], sup[~same])
    sizes = np.bincount(lab, minlength=1)
    return {"labels": lab, "support_hist": hist, "node_in": node_in, "node_out": node_out,
            "stability": stability(node_in, node_out),
            "edges": int(len(u)), "kept_edges": int(keep.sum()), "unanimous_edges": int(hist[n_total]),
            "split_edges": int(hist[0]), "k": int(lab.max()) + 1, "max_size": int(sizes.max()),
            "singletons": int((sizes == 1).sum()), "n_total": int(n_total), "cut": cut}


INFO_INTS = ("edges", "kept_edges", "unanimous_edges", "split_edges", "k", "max_size", "singletons", "n_total")
