"""Numpy restatement of fc_community_quality (include/fastconsensus_amd.h) with a small Python
union-find -- TEST INFRASTRUCTURE ONLY.  Every value is an integer."""
import numpy as np

FIELDS = ("ids", "size", "volume", "in_weight", "in_edges", "min_in_degree", "components", "largest_component", "cut")
INFO = ("k", "max_size", "singletons", "parts", "disconnected", "in_weight_total", "cut_weight", "total_degree")


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def quality(n, u, v, w, labels):
    """Edges (u, v, w) of an undirected graph in node ids, each once, no loops; labels: [n], any
    integer ids.  Returns the fields of Engine.community_quality (clusters in ascending id order,
    the split partition numbered by each part's smallest node)."""
    u, v = np.asarray(u, np.int64).reshape(-1), np.asarray(v, np.int64).reshape(-1)
    w = np.ones(len(u), np.int64) if w is None else np.asarray(w, np.int64).reshape(-1)
    labels = np.asarray(labels, np.int64)
    assert labels.shape == (n,) and not np.any(u == v)
    ids, lab = np.unique(labels, return_inverse=True)
    lab = lab.ravel()
    k = len(ids)
    same = lab[u] == lab[v]
    node_in, node_out, deg_in = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for end in (u, v):
        np.add.at(node_in, end[same], w[same])
        np.add.at(node_out, end[~same], w[~same])
        np.add.at(deg_in, end[same], 1)
    volume = np.zeros(k, np.int64)
    np.add.at(volume, lab, node_in + node_out)
    in_weight = np.zeros(k, np.int64)
    np.add.at(in_weight, lab[u[same]], w[same])
    in_edges = np.bincount(lab[u[same]], minlength=k).astype(np.int64)
    min_in = np.full(k, np.iinfo(np.int64).max)
    np.minimum.at(min_in, lab, deg_in)
    parent = list(range(n))
    for a, b in zip(u[same].tolist(), v[same].tolist()):
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)      # the root is the smallest node of its part
    root = np.array([_find(parent, x) for x in range(n)], np.int64)
    is_root = root == np.arange(n)
    split = (np.cumsum(is_root) - 1)[root].astype(np.int32)
    psize = np.bincount(split)
    components = np.bincount(lab[is_root], minlength=k).astype(np.int64)
    largest = np.zeros(k, np.int64)
    np.maximum.at(largest, lab[is_root], psize[split[is_root]])
    size = np.bincount(lab, minlength=k).astype(np.int64)
    cut = volume - 2 * in_weight
    return {"ids": ids.astype(np.int64), "size": size, "volume": volume, "in_weight": in_weight, "in_edges": in_edges,
            "min_in_degree": min_in, "components": components, "largest_component": largest, "cut": cut,
            "node_in": node_in, "node_out": node_out, "split": split,
            "k": k, "max_size": int(size.max()), "singletons": int((size == 1).sum()),
            "parts": int(is_root.sum()), "disconnected": int((components > 1).sum()),
            "in_weight_total": int(in_weight.sum()), "cut_weight": int(w[~same].sum()),
            "total_degree": int(2 * w.sum())}
