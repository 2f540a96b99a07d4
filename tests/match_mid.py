"""The mid-size case of tests/analysis_mid.py for the cluster match (tests/test_match_mid_cases.py,
tests/test_gpu_match_mid.py): three natural partitions matched against its 20 and 70 labelings,

    part     P itself: 269,747 clusters, C and A past FC_SCORE_LCAP, B exactly at it
    coarse   labs70[2]: 18 clusters, a giant of 358,519 members with 270 k .. 358 k cells per row
    fine     labs70[3]: 358,537 clusters, every one on the register path

and two crafted partitions on the same N = 400,003 nodes, each with one labeling row and in both
label orders, whose deciding cross products lie past 2^32 (wide, near_tie_wide).  The reference is
match_ref.match without the Python loop over the cells: a float64 maximum proposes the best cell per
cluster, int64 products decide.  analysis_mid.py is imported, not changed."""
import functools

import numpy as np

from tests import analysis_mid as am
from tests import match_ref as mr

PARTS = ("part", "coarse", "fine")
WIDE = (100_000, 50_000, 50_000)                    # the crafted clusters' (size, inter, csize)
NEAR_C = 100_000
NEAR = (2 * NEAR_C + 1, NEAR_C, 2 * NEAR_C - 2)
REGISTER_LCAP = 262_144                             # the FC_SCORE_LCAP under which the crafted clusters stay in registers


# ------------------------------------------------------------------ the sparse reference
def _beats(s, c1, u1, c2, u2):
    """match_ref.better on int64 arrays, by the unions u = s + t - c (the products stay below 2^63)"""
    a, b = c1 * u2, c2 * u1
    return (a > b) | ((a == b) & (c1 > c2))


def match(labs, part, propose=np.float64):
    """match_ref.match (same arguments, same return types) without the loop over the cells.  Per row
    the best cell of a cluster is proposed in float64 (the largest C / U, then the largest C) and
    then checked on integers: no cell of the cluster may beat it under match_ref.better's rule.  A
    cluster where the proposal fails is decided by match_ref.better on Python ints.  propose: the
    float type of the proposal (the tests pass float32 to make proposals fail)."""
    labs = np.atleast_2d(np.asarray(labs))
    ids, dense, size = np.unique(np.asarray(part), return_inverse=True, return_counts=True)
    dense = dense.reshape(-1).astype(np.int64)
    size = size.astype(np.int64)
    K = len(ids)
    inter = np.zeros((len(labs), K), np.int32)
    csize = np.zeros((len(labs), K), np.int32)
    for r, row in enumerate(labs):
        _, d = np.unique(row, return_inverse=True)
        d = d.reshape(-1).astype(np.int64)
        t = np.bincount(d).astype(np.int64)
        nd = len(t)
        cell, C = np.unique(dense * nd + d, return_counts=True)       # the nonempty cells, by cluster
        C = C.astype(np.int64)
        kk = cell // nd
        T = t[cell % nd]
        U = size[kk] + T - C
        assert int(C.max()) * int(U.max()) < 1 << 63
        start = np.searchsorted(kk, np.arange(K))                       # every cluster has a cell
        J = C.astype(propose) / U.astype(propose)
        top = J == np.maximum.reduceat(J, start)[kk]
        bc = np.maximum.reduceat(np.where(top, C, 0), start)
        bt = np.minimum.reduceat(np.where(top & (C == bc[kk]), T, np.iinfo(np.int64).max), start)
        lost = np.unique(kk[_beats(size[kk], C, U, bc[kk], (size + bt - bc)[kk])])
        end = np.r_[start[1:], len(kk)]
        for k in lost.tolist():                                         # the float proposal was wrong: Python ints
            best = (0, 0)
            for c, tt in zip(C[start[k]:end[k]].tolist(), T[start[k]:end[k]].tolist()):
                if mr.better(int(size[k]), c, tt, *best):
                    best = (c, tt)
            bc[k], bt[k] = best
        inter[r], csize[r] = bc, bt
    return ids, size, inter, csize


def recovered(inter, size, csize, num=3, den=4):
    """match_ref.recovered on int64 arrays: rows with den * C >= num * (s + t - C) per cluster"""
    inter, csize = np.atleast_2d(inter).astype(np.int64), np.atleast_2d(csize).astype(np.int64)
    return (den * inter >= num * (np.asarray(size, np.int64)[None, :] + csize - inter)).sum(0).astype(np.int64)


def dissolved(inter, size, csize, num=1, den=2):
    """match_ref.dissolved on int64 arrays: rows with den * C <= num * (s + t - C) per cluster"""
    inter, csize = np.atleast_2d(inter).astype(np.int64), np.atleast_2d(csize).astype(np.int64)
    return (den * inter <= num * (np.asarray(size, np.int64)[None, :] + csize - inter)).sum(0).astype(np.int64)


def summary(inter, size, csize):
    """match_ref.summary; its three float arrays are numpy expressions already, the two counts loop
    over clusters x rows there and are restated above"""
    return {"jaccard": mr.jaccard(inter, size, csize), "f1": mr.f1(inter, size, csize),
            "stability": mr.stability(inter, size, csize), "recovered": recovered(inter, size, csize),
            "dissolved": dissolved(inter, size, csize)}


def lanes(labs, part):
    """(over, ncell), [rows][K] each: the (cluster, row) lanes the register path leaves to the
    fallback (analysis_mid.lane_overflow at the sources' SC_D and default FC_SCORE_LCAP) and the
    nonempty cells of every lane, eight rows at a time so that only their cells are held"""
    k = am.caps()
    size = np.unique(part, return_counts=True)[1].astype(np.int64)
    labs = np.atleast_2d(np.asarray(labs))
    over, ncell = [], []
    for lo in range(0, len(labs), 8):
        per = am.cluster_cells(labs[lo:lo + 8], part)[2]
        over.append(am.lane_overflow(per, size, k["SC_D"], k["LCAP"]))
        ncell += [np.bincount(cell // D, minlength=len(size)).astype(np.int32) for cell, _, _, D in per]
    return np.concatenate(over), np.stack(ncell)


# ------------------------------------------------------------------ the partitions
def partition(c, name):
    """one of PARTS from the case of analysis_mid"""
    return {"part": c["part"], "coarse": c["labs70"][2], "fine": c["labs70"][3]}[name]


def reference(labs, part):
    """what the GPU tests compare with: match() plus the lanes the fallback takes"""
    ids, size, inter, csize = match(labs, part)
    return {"ids": ids, "size": size, "inter": inter, "csize": csize, "over": lanes(labs, part)[0]}


def rows_of(ref, rows):
    """the reference of the first `rows` labelings (or of the rows of a slice) from one of more"""
    rows = rows if isinstance(rows, slice) else slice(0, rows)
    return dict(ref, inter=ref["inter"][rows], csize=ref["csize"][rows], over=ref["over"][rows])


def _labels(a_low):
    return (2, 9) if a_low else (9, 2)


def wide(a_low, n=am.N):
    """A cluster whose two leading candidates have both cross products past 2^32, and reducing the
    products mod 2^32 reverses the comparison.  Cluster 0 has s = 100,000 members (nodes 0..99,999).
    Community A holds 50,000 of them and nobody else (C = t = 50,000); community B holds 45,000 of
    them and 75,000 outsiders (C = 45,000, t = 120,000); the 5,000 remaining members sit with every
    other node in one community (C = 5,000, t = 230,003: J = 0.015).  A's 50,000 x 175,000 = 8.75e9
    beats B's 45,000 x 100,000 = 4.5e9, and mod 2^32 it is 1.60e8 against 2.05e8.  (With 40,000
    members and 20,000 outsiders in B the 32-bit products are reversed as well, but B's product,
    4.0e9, is still below 2^32.)  Every other node is a cluster of its own.  a_low: A's label below
    B's, else above.  Returns part, lab; the answer for cluster 0 is WIDE = (100,000, 50,000, 50,000)."""
    part = np.arange(n, dtype=np.int64) - 99_999
    part[:100_000] = 0
    la, lb = _labels(a_low)
    lab = np.full(n, 5, np.int64)
    lab[:50_000] = la
    lab[50_000:95_000] = lb
    lab[100_000:175_000] = lb
    return part, lab


def near_tie_wide(a_low, n=am.N):
    """match_ref.near_tie scaled to c = 100,000: cluster 0 has 2c + 1 members; community A has C = c
    of them and c - 2 outsiders (t = 2c - 2), community B C = c + 1 and c + 1 outsiders (t = 2c + 2).
    The cross products are 3c^2 + 2c and 3c^2 + 2c - 1, about 3.0e10: A wins by a part in 3e10, which
    float32 division cannot see, and the larger-C rule alone would pick B.  That uses 4c nodes; the
    three left over are clusters and communities of their own, as every outsider is a cluster of its
    own.  a_low: A's label below B's, else above.  Returns part, lab; the answer for cluster 0 is
    NEAR = (200,001, 100,000, 199,998)."""
    c = NEAR_C
    assert n == 4 * c + 3
    part = np.arange(n, dtype=np.int64) - 2 * c
    part[:2 * c + 1] = 0
    la, lb = _labels(a_low)
    lab = np.empty(n, np.int64)
    lab[:c] = la
    lab[c:2 * c + 1] = lb
    lab[2 * c + 1:3 * c - 1] = la
    lab[3 * c - 1:4 * c] = lb
    lab[4 * c:] = [20, 21, 22]
    return part, lab


CRAFTED = {"wide": (wide, WIDE), "near_tie_wide": (near_tie_wide, NEAR)}


def candidates(part, lab):
    """(s, [(C, t) per community of cluster 0, by descending C]) of a crafted case, on Python ints"""
    member = part == 0
    t = np.bincount(lab)
    d, C = np.unique(lab[member], return_counts=True)
    return int(member.sum()), sorted(((int(c), int(t[x])) for x, c in zip(d, C)), reverse=True)


def cross_products(part, lab):
    """the two products better() compares for the two largest candidates of cluster 0"""
    s, cand = candidates(part, lab)
    (c1, t1), (c2, t2) = cand[:2]
    return c1 * (s + t2 - c2), c2 * (s + t1 - c1)


# ------------------------------------------------------------------ what the case reaches
def total_clamp():
    """k_cm_total's grid clamp: its nblk(...) argument holds a cast, which analysis_mid.clamp's
    pattern does not read"""
    return int(am._one(r"k_cm_total<<<std::min<\w+>\(nblk\([^,;]*\), (\d+)u?\)", "match.h").group(1))


def clamps():
    return {"k_cm_sizes": am.clamp("match.h", "k_cm_sizes"), "k_cm_fold": am.clamp("match.h", "k_cm_fold"),
            "k_cm_scatter": am.clamp("match.h", "k_cm_scatter"), "k_cm_total": total_clamp()}


def chunk_windows(n, chunk):
    """(cap, step) as score_chunk_buffers computes them: up to cap keys a chunk, one chunk every
    step keys of the stream"""
    cap = max(2 * n, chunk)
    return cap, cap - n


def fallback_chunks(over, ncell, size, n, chunk):
    """The fallback's chunks as cell_chunks walks them.  The items are the flagged (cluster, row)
    lanes in the stream's order (bank of 64 rows, cluster, lane), each of size[cluster] keys and
    ncell runs; chunk j owns the items that start in [j * step, (j + 1) * step) and launches on
    min(cap, T - j * step) keys.  Returns (T, keys per chunk, runs per chunk, the items whose keys
    straddle the end of their chunk's window)."""
    lens, runs = [], []
    for b in range(0, len(over), 64):
        o = over[b:b + 64].T                                           # [K][lanes]: cluster-major
        lens.append(np.broadcast_to(size[:, None], o.shape)[o])
        runs.append(ncell[b:b + 64].T[o])
    lens, runs = np.concatenate(lens).astype(np.int64), np.concatenate(runs).astype(np.int64)
    start = np.cumsum(lens) - lens
    T = int(lens.sum())
    cap, step = chunk_windows(n, chunk)
    nchunks = -(-T // step)
    owner = start // step
    keys = np.array([min(cap, T - j * step) for j in range(nchunks)], np.int64)
    per = np.bincount(owner, weights=runs, minlength=nchunks).astype(np.int64)
    straddle = int((start + lens > (owner + 1) * step).sum())
    return T, keys, per, straddle


@functools.lru_cache(maxsize=None)
def coarse20():
    """(size, over, ncell) of `coarse` against the 20 labelings"""
    c = am.case()
    coarse = partition(c, "coarse")
    return (np.unique(coarse, return_counts=True)[1].astype(np.int64),) + lanes(c["labs20"], coarse)


def reached(c):
    """{name: (value, relation, cap)}: per launch clamp, list cap and chunk window of match.h's
    kernels and of the chunk driver under them, the quantity of the case that must stand in
    `relation` to it, from the inputs and the references alone, and the cap itself, read from the
    csrc sources by name."""
    k = am.caps()
    tb, n = k["TB"], c["n"]
    cl = clamps()
    cc20 = c["cc20"]
    ids, size, over = cc20["ids"], cc20["size"], cc20["over"]
    K = len(ids)
    rank = {x: int(np.searchsorted(ids, i)) for x, i in zip("CAB", c["ids_cab"])}
    k_fine = len(np.unique(partition(c, "fine")))
    banks20, banks70 = -(-am.N_R // 64), -(-am.N_R2 // 64)
    csize, cover, cncell = coarse20()
    T, keys, runs, straddle = fallback_chunks(cover, cncell, csize, n, k["CHUNK"])
    cap, step = chunk_windows(n, k["CHUNK"])
    two32 = 1 << 32
    out = {
        "k_cm_sizes: N x n_r <= N x ldT elements (labs20)": (n * am.N_R, ">", cl["k_cm_sizes"] * tb),
        "k_cm_match: clusters of part": (K, ">", 4 * k["SC_GRID"]),
        "k_cm_match: clusters of fine": (k_fine, ">", 4 * k["SC_GRID"]),
        "k_cm_match: clusters of part in the second bank (labs70)": ((banks70 - 1) * K, ">", 4 * k["SC_GRID"]),
        "entry numbering: bank 1 with k above 2^18 (part, labs70)": ((banks70 - 1) * K, ">", 262_144),
        "k_cm_total: rows x K (part, labs20)": (am.N_R * K, ">", cl["k_cm_total"] * tb),
        "k_cm_scatter: banks x K x 64 with a flagged lane (part, labs20)":
            (banks20 * K * 64 * int(over.any()), ">", cl["k_cm_scatter"] * tb),
        "k_cm_fold: runs of the fullest chunk (coarse, labs20)": (int(runs.max()), ">", cl["k_cm_fold"] * tb),
        "k_cc_emit: keys of the first chunk (coarse, labs20)": (int(keys[0]), ">", k["k_cc_emit"] * tb),
        "chunks: fallback keys of coarse, labs20, against one chunk's step": (T, ">", step),
        "chunks: at least two": (len(keys), ">", 1),
        "chunks: items whose keys straddle the end of a window": (straddle, ">", 0),
        "chunks: the default chunk, not the 2N floor": (k["CHUNK"], ">", 2 * n),
        "LCAP: the cluster C": (int(size[rank["C"]]), ">", k["LCAP"]),
        "LCAP: the cluster A": (int(size[rank["A"]]), ">", k["LCAP"]),
        "LCAP: C's and A's lanes in the fallback": (int(over[:, [rank["C"], rank["A"]]].sum()), "==", 2 * am.N_R),
        "LCAP: the cluster B": (int(size[rank["B"]]), "==", k["LCAP"]),
        "LCAP: B's lanes on the register path": (int((~over[:, rank["B"]]).sum()), "==", am.N_R),
        "a register lane and a fallback lane in one call (part, labs20)": (int(over.sum()) * int((~over).sum()), ">", 0),
        "SC_D: lanes of clusters within LCAP that overflow the list": (int(over[:, size <= k["LCAP"]].sum()), ">", 0),
    }
    for name, (make, (s, _, _)) in CRAFTED.items():
        for a_low in (True, False):
            tag = "%s(a_low=%s)" % (name, a_low)
            out[tag + ": the smaller cross product"] = (min(cross_products(*make(a_low))), ">", two32)
        out[name + ": cluster 0 in the fallback at the default cap"] = (s, ">", k["LCAP"])
        out[name + ": cluster 0 on the register path at FC_SCORE_LCAP=%d" % REGISTER_LCAP] = (s, "<=", REGISTER_LCAP)
    return out
