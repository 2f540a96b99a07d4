"""CPU reference of fc_vote_map / fc_vote_count / fc_vote, written from the definitions: with
C_r[k][d] the number of nodes v with P(v) = k and lab_r(v) = d,

    map_r(d)     = the cluster k of largest C_r[k][d], the smallest id among equals
    mapped[r][v] = map_r(lab_r(v))
    votes_v(k)   = the number of r with mapped[r][v] = k        own[v] = votes_v(P(v))
    top_votes[v] = max_k votes_v(k)
    top[v]       = the cluster reaching it: P(v) when it is among several, else the smallest id
    distinct[v]  = the number of clusters with a vote

plain numpy, exact integers; cells are found with np.unique, never with a dense table."""
import numpy as np

INFO = ("k", "k_voted", "moved", "unanimous", "tied", "mapped_communities", "n_total")


def _first_of_group(group):
    """mask of the first element of every run of the sorted array `group`"""
    m = np.ones(len(group), bool)
    m[1:] = group[1:] != group[:-1]
    return m


def map_labelings(labs, part):
    """labs [n_r][n], part [n] (any integer ids).  Returns mapped int64 [n_r][n] (ids of part) and
    the sum over the replicas of their community counts."""
    labs = np.asarray(labs)
    part = np.asarray(part)
    ids, dense = np.unique(part, return_inverse=True)
    dense = dense.reshape(-1).astype(np.int64)
    K = len(ids)
    out = np.empty(labs.shape, np.int64)
    communities = 0
    for r, row in enumerate(labs):
        _, d = np.unique(row, return_inverse=True)
        d = d.reshape(-1).astype(np.int64)
        cell, cnt = np.unique(d * K + dense, return_counts=True)      # the nonempty cells (d, k)
        cd, ck = cell // K, cell % K
        order = np.lexsort((ck, -cnt, cd))                            # by d, then largest count, then smallest k
        first = order[_first_of_group(cd[order])]
        best = np.empty(int(d.max()) + 1, np.int64)
        best[cd[first]] = ck[first]
        out[r] = ids[best[d]]
        communities += len(first)
    return out, communities


def count_votes(mapped, part):
    """mapped [n_total][n] (ids of part), part [n].  Returns a dict: own, top, top_votes, distinct
    (int64 [n]), own_hist int64 [n_total + 1] and k, k_voted, moved, unanimous, tied, n_total."""
    mapped = np.asarray(mapped).astype(np.int64)
    part = np.asarray(part).astype(np.int64)
    nt, n = mapped.shape
    span = int(max(mapped.max(), part.max())) + 1
    node = np.broadcast_to(np.arange(n, dtype=np.int64), (nt, n))
    cell, votes = np.unique((node * span + mapped).reshape(-1), return_counts=True)   # the cells (node, cluster)
    cn, ck = cell // span, cell % span
    is_p = ck == part[cn]
    distinct = np.bincount(cn, minlength=n)
    own = np.zeros(n, np.int64)
    own[cn[is_p]] = votes[is_p]
    order = np.lexsort((ck, ~is_p, -votes, cn))    # by node, most votes, P(v) before the others, smallest id
    first = order[_first_of_group(cn[order])]
    top = np.empty(n, np.int64)
    top_votes = np.empty(n, np.int64)
    top[cn[first]] = ck[first]
    top_votes[cn[first]] = votes[first]
    leaders = np.bincount(cn[votes == top_votes[cn]], minlength=n)
    return {"own": own, "top": top, "top_votes": top_votes, "distinct": distinct,
            "own_hist": np.bincount(own, minlength=nt + 1).astype(np.int64),
            "k": len(np.unique(part)), "k_voted": len(np.unique(top)), "moved": int((top != part).sum()),
            "unanimous": int((own == nt).sum()), "tied": int((leaders > 1).sum()), "n_total": nt}


def vote(labs, part):
    """map_labelings then count_votes: the dict of count_votes plus mapped and mapped_communities"""
    mapped, communities = map_labelings(labs, part)
    out = count_votes(mapped, part)
    out["mapped"] = mapped
    out["mapped_communities"] = communities
    return out


def refine(labs, part, max_rounds=16):
    """part <- top until nothing moves or the cap is reached.  Returns the last vote's dict (its
    `labels` are the partition it was made on), rounds and moved_per_round."""
    part = np.asarray(part).astype(np.int64)
    moved = []
    while True:
        res = vote(labs, part)
        res["labels"] = part
        if res["moved"] == 0 or len(moved) >= max_rounds:
            break
        moved.append(res["moved"])
        part = res["top"]
    res["rounds"] = len(moved)
    res["moved_per_round"] = moved
    return res
