"""The mid-size case of tests/analysis_mid.py for the cluster merges (tests/test_merge_mid_cases.py,
tests/test_gpu_merge_mid.py): the community graph of its partition P (269,747 clusters) on its
797,200 edges, and the pair list of fc_cluster_coassoc: that graph's pairs plus the pairs among the
long clusters C (66,000 members), A (16,500, just past FC_SCORE_LCAP), B (exactly FC_SCORE_LCAP) and
a small neighbour of B, the long pairs repeated so that the fallback's lookup kernel passes its
launch clamp.  The references are sparse (analysis_mid.cluster_cells): no dense table of
269,747 rows is built.  analysis_mid.py itself is imported, not changed."""
import functools

import numpy as np

from tests import analysis_mid as am

LONG_COPIES = 40            # copies of each of the four long pairs
SUBSET_70 = 100_000         # pairs of the community graph the 70-labeling run takes


def community_graph(n, u, v, part):
    """merge_ref.community_graph for unit weights without the Python loop"""
    ids, dense = am.dense_ids(part)
    K = len(ids)
    x, y = dense[np.asarray(u, np.int64)], dense[np.asarray(v, np.int64)]
    cut = x != y
    key, cnt = np.unique(np.minimum(x, y)[cut] * K + np.maximum(x, y)[cut], return_counts=True)
    return {"a": ids[key // K].astype(np.int32), "b": ids[key % K].astype(np.int32),
            "weight": cnt.astype(np.int64), "edges": cnt.astype(np.int64), "npairs": len(key)}


def sparse_cross(cells, a, b):
    """merge_ref.cross without the dense tables: X(a, b) = sum_r sum_d C_r[a][d] C_r[b][d] from the
    replicas' nonempty cells (analysis_mid.cluster_cells); per pair the cluster with fewer cells is
    expanded and each of its cells looked up in the other's; 0 when an id does not occur."""
    ids, _, per = cells
    K = len(ids)
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    ra, rb = np.searchsorted(ids, a), np.searchsorted(ids, b)
    known = (ra < K) & (rb < K)
    known &= (ids[np.minimum(ra, K - 1)] == a) & (ids[np.minimum(rb, K - 1)] == b)
    ra, rb = ra[known], rb[known]
    out = np.zeros(len(a), np.int64)
    if not len(ra):
        return out
    for cell, cnt, _, D in per:
        start = np.searchsorted(cell // D, np.arange(K + 1))           # the cells of cluster k: [start[k], start[k + 1])
        ncell = np.diff(start)
        swap = ncell[ra] > ncell[rb]
        e, o = np.where(swap, rb, ra), np.where(swap, ra, rb)
        rep = ncell[e]                                                  # >= 1: a cluster that occurs has a cell
        first = np.cumsum(rep) - rep
        idx = np.repeat(start[e] - first, rep) + np.arange(int(rep.sum()))
        key = np.repeat(o, rep) * D + cell[idx] % D
        pos = np.minimum(np.searchsorted(cell, key), len(cell) - 1)
        out[known] += np.add.reduceat(np.where(cell[pos] == key, cnt[idx] * cnt[pos], 0), first)
    return out


def sides(size_of, a, b):
    """(list side, walk side) per pair as fc_cluster_coassoc chooses them: the larger cluster lists,
    a on equal sizes"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    a_lists = size_of(a) >= size_of(b)
    return np.where(a_lists, a, b), np.where(a_lists, b, a)


@functools.lru_cache(maxsize=None)
def pairs():
    """(community graph of P, a, b): the pair list of the case, the same on every call"""
    c = am.case()
    g = community_graph(c["n"], c["u"], c["v"], c["part"])
    C, A, B = (int(x) for x in c["ids_cab"])
    # a small neighbour of B in the community graph
    near = np.r_[g["b"][g["a"] == B], g["a"][g["b"] == B]]
    ids, size = np.unique(c["part"], return_counts=True)
    small = int(next(x for x in near.tolist() if size[np.searchsorted(ids, x)] <= 8))
    la = np.tile([C, A, A, B, B, small], LONG_COPIES)
    lb = np.tile([A, C, B, A, small, B], LONG_COPIES)
    return g, np.r_[g["a"], la].astype(np.int32), np.r_[g["b"], lb].astype(np.int32)


def reached(c):
    """{name: (value, relation, cap)}: per launch clamp and list cap of merge.h's kernels, the
    quantity of the case that must stand in `relation` to it, from the inputs and the references
    alone, and the cap itself, read from the csrc headers by name."""
    k = am.caps()
    tb = k["TB"]
    g, a, b = pairs()
    cc = c["cc20"]
    ids, size = cc["ids"], cc["size"]
    size_of = lambda x: size[np.searchsorted(ids, x)]      # noqa: E731
    lst, wlk = sides(size_of, a, b)
    flagged = cc["over"].sum(0)[np.searchsorted(ids, lst)]                   # lanes of the list side left to the fallback
    C, A, B = (int(x) for x in c["ids_cab"])
    long_rank = np.searchsorted(ids, [C, A])
    return {
        "SC_GRID: listed clusters (k_mc_count)": (len(np.unique(lst)), ">", 4 * k["SC_GRID"]),
        "k_mc_lookup: (pair, walk member) threads": (int(size_of(wlk)[flagged > 0].sum()), ">",
                                                     am.clamp("merge.h", "k_mc_lookup") * tb),
        "k_cc_emit: fallback keys of C and A, 70 labelings, first chunk":
            (min(max(2 * c["n"], k["CHUNK"]), int((c["cc70"]["over"][:, long_rank] * size[None, long_rank]).sum())), ">",
             k["k_cc_emit"] * tb),
        # k_mg_emit, k_mg_pairs, k_mc_orient and k_mc_work launch one thread per element (no clamp):
        # the case gives them more than one wave, block and 2^16 elements
        "unclamped kernels: edges, pairs": (min(len(c["u"]), g["npairs"], len(a)), ">", 1 << 16),
        "LCAP: C lists": (int(size_of(np.array([C]))[0]) * int(C in lst), ">", k["LCAP"]),
        "LCAP: A lists": (int(size_of(np.array([A]))[0]) * int(A in lst), ">", k["LCAP"]),
        "LCAP: B lists at the cap": (int(size_of(np.array([B]))[0]) * int(B in lst), "==", k["LCAP"]),
        "LCAP: B walks under A": (int(((lst == A) & (wlk == B)).sum()), ">", 0),
        "pairs with a register list and pairs with a fallback list": (int((flagged == 0).sum()) * int((flagged > 0).sum()), ">", 0),
    }
