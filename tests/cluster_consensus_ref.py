"""CPU reference of fc_cluster_consensus, written from the contingency definition: with C_r[k][d]
the number of members of cluster k of the partition P that labeling r labels d,

    pairs[k] = sum_r sum_d C_r[k][d]^2        item[v] = sum_r C_r[P(v)][lab_r(v)]

plain numpy, exact int64.  The two float64 normalisations are restated here independently of
fastconsensus_amd.core (the same operations in the same order, so the results compare with ==)."""
import numpy as np


def sums(labs, part):
    """labs [n_r][n], part [n] (any integer ids).  Returns ids (the distinct ids, ascending), size
    int64[K], pairs int64[K], item int64[n]."""
    labs = np.asarray(labs)
    part = np.asarray(part)
    ids, dense, size = np.unique(part, return_inverse=True, return_counts=True)
    dense = dense.reshape(-1).astype(np.int64)
    pairs = np.zeros(len(ids), np.int64)
    item = np.zeros(len(part), np.int64)
    for row in labs:
        _, d = np.unique(row, return_inverse=True)
        d = d.reshape(-1).astype(np.int64)
        cell = dense * (int(d.max()) + 1) + d                 # one id per nonempty (cluster, label) cell
        _, inv, cnt = np.unique(cell, return_inverse=True, return_counts=True)
        cnt = cnt.astype(np.int64)
        own = cnt[inv.reshape(-1)]                            # C_r[P(v)][lab_r(v)] per node
        item += own
        np.add.at(pairs, dense, own)                          # sum over a cell's members of its count = count^2
    return ids, size.astype(np.int64), pairs, item


def cluster_consensus(pairs, size, n_total):
    """(pairs - n_total size) / (n_total size (size - 1)), NaN where size = 1"""
    out = np.full(len(pairs), np.nan, np.float64)
    for i, (p, s) in enumerate(zip(np.asarray(pairs).tolist(), np.asarray(size).tolist())):
        if s > 1:
            out[i] = np.int64(p - n_total * s) / np.int64(n_total * s * (s - 1))
    return out


def item_consensus(item, size_of_own, n_total):
    """(item - n_total) / (n_total (size_of_own - 1)), NaN where the size is 1"""
    out = np.full(len(item), np.nan, np.float64)
    for i, (x, s) in enumerate(zip(np.asarray(item).tolist(), np.asarray(size_of_own).tolist())):
        if s > 1:
            out[i] = np.int64(x - n_total) / np.int64(n_total * (s - 1))
    return out


def item_sums(matrix_fn, labs, nodes, part, clusters):
    """int64 [len(nodes)][len(clusters)]: sum over the members u of each cluster of coassoc(node, u),
    from the brute-force matrix (matrix_fn = coassoc_ref.matrix)."""
    part = np.asarray(part)
    out = np.zeros((len(nodes), len(clusters)), np.int64)
    for j, c in enumerate(clusters):
        mem = np.flatnonzero(part == c)
        if len(mem):
            out[:, j] = matrix_fn(labs, nodes, mem).astype(np.int64).sum(1)
    return out


def same_floats(a, b):
    """== under the NaN masks"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all(a[~np.isnan(a)] == b[~np.isnan(b)]))
