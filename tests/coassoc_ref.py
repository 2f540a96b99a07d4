"""CPU reference of the co-association calls (fc_coassociation / fc_coassoc_pairs /
fc_coassoc_hist) and of pac / consensus_cdf: plain numpy.  Everything is an exact integer except
the two float64 divisions of pac and cdf, restated here independently of fastconsensus_amd.core."""
import numpy as np

CHUNK = 16          # replicas per slice: bounds the [chunk][na][nb] boolean temporaries


def matrix(labs, a, b=None):
    """int32 [na][nb]: the number of labelings r with labs[r][a[i]] == labs[r][b[j]]."""
    labs = np.asarray(labs)
    a = np.asarray(a, np.int64).reshape(-1)
    b = a if b is None else np.asarray(b, np.int64).reshape(-1)
    out = np.zeros((len(a), len(b)), np.int64)
    for lo in range(0, len(labs), CHUNK):
        sl = labs[lo:lo + CHUNK]
        out += (sl[:, a][:, :, None] == sl[:, b][:, None, :]).sum(0)
    return out.astype(np.int32)


def pairs(labs, p):
    """int32 [npairs]: the number of labelings that put p[i][0] and p[i][1] together."""
    labs = np.asarray(labs)
    p = np.asarray(p, np.int64).reshape(-1, 2)
    return (labs[:, p[:, 0]] == labs[:, p[:, 1]]).sum(0).astype(np.int32)


def hist(labs, nodes):
    """int64 [n_r + 1]: bincount of the matrix's strict upper triangle (position pairs i < j)."""
    labs = np.asarray(labs)
    m = matrix(labs, nodes)
    iu = np.triu_indices(len(m), 1)
    return np.bincount(m[iu], minlength=len(labs) + 1).astype(np.int64)


def pac(h, lo=0.1, hi=0.9):
    """sum of h[s] over lo * n < s < hi * n (n = len(h) - 1, float64 comparisons) over h.sum()."""
    n = len(h) - 1
    total = sum(int(x) for x in h)
    if total == 0:
        return 0.0
    amb = sum(int(h[s]) for s in range(n + 1) if float(s) > float(lo) * float(n) and float(s) < float(hi) * float(n))
    return amb / total


def cdf(h):
    """cumsum(h) / h.sum() in float64; zeros when h.sum() == 0."""
    h = np.asarray(h, np.int64)
    total = int(h.sum())
    if total == 0:
        return np.zeros(len(h), np.float64)
    return np.cumsum(h) / total
