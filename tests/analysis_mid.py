"""One deterministic mid-size case for the analysis calls (tests/test_analysis_mid_cases.py,
tests/test_gpu_analysis_mid.py): N = 400,003 nodes, about 800 k edges, 70 labelings (the first 20
are the 20-replica case) and a partition P, laid out so that every grid clamp, list cap and 64-bit
sum of csrc/{score,cluster,vote,affinity,components,levels,coassoc}.h is passed -- see reached().
Built with numpy from a fixed seed, no file read; case() keeps one copy per process and computes each
reference (REFS) once, when it is first asked for.

The layout, in "position" order (a random permutation then scatters the positions over node ids):

    C        66,000 nodes   one cluster of P (> 65,536); whole in the clean rows, cut in 20+ pieces by the noisy ones
    A        16,500 nodes   one cluster of P just past FC_SCORE_LCAP; every row cuts it in 2..6 pieces
    B        16,384 nodes   one cluster of P of exactly FC_SCORE_LCAP members; whole in 9 rows of 10
    G0..G11  300 each       twelve anchor clusters, whole in every row
    X        5,000 nodes    singletons of P; row r puts x_j into the community of G[(j + r) % 12]: 12 clusters vote for it
    medium   ~3,000 clusters of 2..200 members
    single   the rest       singletons of P

Row r is, by r % 10: 0, 1 clean (P itself; from row 10 on with 1 % noise), 2 coarse (C, the medium
clusters and the singletons in one giant community), 3 fine (every node of C, medium and single
alone), 4..9 noisy (C in pieces, a fraction of medium and single moved to ~3000 noise communities;
row 7 also cuts B in two)."""
import functools
import os
import re
import time

import numpy as np

from tests import cluster_consensus_ref as ccr
from tests import coassoc_ref as car
from tests import consensus_levels_ref as lref
from tests import consensus_ref as cref
from tests import score_ref
from tests import vote_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastconsensus_amd", "csrc")

SEED = 20240611
N = 400_003
N_R, N_R2 = 20, 70
SIZE_C, SIZE_A, SIZE_B = 66_000, 16_500, 16_384
ANCHORS, ANCHOR_SIZE, SIZE_X = 12, 300, 5_000
MEDIUM = 3_000
M_RANDOM, M_LOCAL = 500_000, 300_000
NOISE_POOL = 3_000
# co-association: its own labelings, few distinct signatures among the listed nodes
CA_N_R, CA_SIGNATURES, CA_FAMILIES, CA_LABELS, CA_K = 12, 3_000, 100, 40, 120_001
CA_PAIRS, CA_NA, CA_NB = 300_000, 4_099, 4_001
SCORE_PAIRS = ((0, 1), (2, 3), (3, 2), (0, 5), (14, 19), (-1, 0), (-1, 7))   # (2, 3): the giant against singletons
THETAS = (0.5, 0.9)
CUT_LEVELS = (10, 18)


# ------------------------------------------------------------------ the sparse references
def dense_ids(x):
    """(ids ascending, dense index per element int64)"""
    ids, inv = np.unique(np.asarray(x), return_inverse=True)
    return ids, inv.reshape(-1).astype(np.int64)


def hist_by_signature(labs, nodes):
    """coassoc_ref.hist without the matrix: the listed positions grouped by signature (the column
    labs[:, node]) with multiplicities c_s; a signature's own pairs agree in all n_r replicas, the
    pairs of two signatures s < t in as many replicas as the signatures do.  int64 [n_r + 1]."""
    labs = np.asarray(labs)
    n_r = len(labs)
    sig, c = np.unique(labs[:, np.asarray(nodes, np.int64).reshape(-1)].T, axis=0, return_counts=True)
    c = c.astype(np.int64)
    hist = np.zeros(n_r + 1, np.int64)
    hist[n_r] += int((c * (c - 1) // 2).sum())
    S = len(sig)
    for lo in range(0, S, 256):
        hi = min(S, lo + 256)
        agree = (sig[lo:hi, None, :] == sig[None, :, :]).sum(2)              # [block][S]
        w = c[lo:hi, None] * c[None, :]
        upper = np.arange(lo, hi)[:, None] < np.arange(S)[None, :]           # s < t
        np.add.at(hist, agree[upper], w[upper])
    return hist


def cluster_cells(labs, part):
    """Per replica the nonempty contingency cells of P: a list of (cell keys ascending = cluster
    rank * D + dense label, counts, dense labels per node, D), plus P's ids and ranks per node."""
    ids, dense = dense_ids(part)
    out = []
    for row in np.asarray(labs):
        _, d = dense_ids(row)
        D = int(d.max()) + 1
        cells, cnt = np.unique(dense * D + d, return_counts=True)
        out.append((cells, cnt.astype(np.int64), d, D))
    return ids, dense, out


def sparse_affinity(labs, part, nodes, clusters, cells=None):
    """median_ref.affinity without the dense tables: aff(v, k) = sum_r C_r[k][lab_r(v)], each cell
    looked up among the replica's nonempty cells; 0 for a cluster id that does not occur."""
    ids, _, per = cluster_cells(labs, part) if cells is None else cells
    nodes = np.asarray(nodes, np.int64).reshape(-1)
    clusters = np.asarray(clusters, np.int64).reshape(-1)
    rank = np.searchsorted(ids, clusters)
    known = (rank < len(ids)) & (ids[np.minimum(rank, len(ids) - 1)] == clusters)
    out = np.zeros(len(nodes), np.int64)
    for cell, cnt, d, D in per:
        key = rank[known] * D + d[nodes[known]]
        pos = np.minimum(np.searchsorted(cell, key), len(cell) - 1)
        out[known] += np.where(cell[pos] == key, cnt[pos], 0)
    return out


def lane_overflow(cells, size, sc_d, lcap):
    """over[r][k]: the (cluster, replica) lanes the register path leaves to the fallback: more than
    sc_d labels in the cluster, or a cluster longer than lcap."""
    K = len(size)
    over = np.zeros((len(cells), K), bool)
    for r, (cell, _, _, D) in enumerate(cells):
        over[r] = (np.bincount(cell // D, minlength=K) > sc_d) | (size > lcap)
    return over


# ------------------------------------------------------------------ the constants of csrc
@functools.lru_cache(maxsize=None)
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, name):
    m = re.search(pattern, _src(name))
    assert m, "csrc/%s no longer holds %r: tests/analysis_mid.py reads its caps from there" % (name, pattern)
    return m


def const(header, name):
    """static constexpr int NAME = value;"""
    return int(_one(r"static constexpr int %s = (\d+);" % name, header).group(1))


def env_default(name):
    """the default of an env_int / env_i64 switch of fc_ctx.h: a literal or 1 << bits"""
    m = _one(r'env_(?:int|i64)\("%s", (?:\(int64_t\))?(\d+)(?: << (\d+))?\)' % name, "fc_ctx.h")
    return int(m.group(1)) << int(m.group(2) or 0)


def clamp(header, kernel):
    """the literal grid clamp of `kernel`'s launch in `header`: std::min<..>(blocks, LITERAL)"""
    return int(_one(r"%s(?:<\w+>)?<<<(?:\(unsigned\))?std::min<\w+>\((?:nblk\([^()]*\)|\w+), (\d+)u?\)" % kernel,
                    header).group(1))


def caps():
    tb = const("consensus.hip", "TB")
    return {"TB": tb, "SC_D": const("score.h", "SC_D"), "VT_D": const("vote.h", "VT_D"),
            "SC_GRID": const("score.h", "SC_GRID"), "CA_T": const("coassoc.h", "CA_T"),
            "LCAP": env_default("FC_SCORE_LCAP"), "CHUNK": env_default("FC_SCORE_CHUNK"),
            "CP_HIST_GRID": const("components.h", "CP_HIST_GRID"), "LV_GRID": const("levels.h", "LV_GRID"),
            "k_cc_total": clamp("cluster.h", "k_cc_total"), "k_vc_flags": clamp("vote.h", "k_vc_flags"),
            "k_ia_slow": clamp("affinity.h", "k_ia_slow"), "k_sc_fold": clamp("score.h", "k_sc_fold"),
            "k_vc_slow": clamp("vote.h", "k_vc_slow"), "k_cc_fold": clamp("cluster.h", "k_cc_fold"),
            "k_vm_fold": clamp("vote.h", "k_vm_fold"), "k_cc_emit": clamp("cluster.h", "k_cc_emit"),
            "k_ia_lookup": clamp("affinity.h", "k_ia_lookup")}


# ------------------------------------------------------------------ the inputs
def _medium_sizes(rng):
    fixed = [2, 3, 8, 9, 10, 63, 64, 65, 100, 150, 199, 200] * 5
    drawn = 2 + np.floor(198 * rng.random(MEDIUM - len(fixed)) ** 24).astype(np.int64)
    return rng.permutation(np.concatenate([np.array(fixed, np.int64), drawn]))


def inputs():
    """The graph, P, the labelings and the query lists: a dict of arrays, the same on every call."""
    rng = np.random.default_rng(SEED)
    perm = rng.permutation(N)                        # position -> node id
    med = _medium_sizes(rng)
    bounds = np.cumsum([0, SIZE_C, SIZE_A, SIZE_B, ANCHORS * ANCHOR_SIZE, SIZE_X, int(med.sum())])
    c0, a0, b0, g0, x0, m0, s0 = bounds
    assert s0 < N
    pos = np.arange(N, dtype=np.int64)
    in_c, in_a, in_b = pos < a0, (pos >= a0) & (pos < b0), (pos >= b0) & (pos < g0)
    in_g, in_x = (pos >= g0) & (pos < x0), (pos >= x0) & (pos < m0)
    loose = pos >= m0                                 # medium and single: what the noise moves
    # P by position: 0 C, 1 A, 2 B, 3..14 anchors, then X, medium, singletons
    dense = np.empty(N, np.int64)
    dense[in_c], dense[in_a], dense[in_b] = 0, 1, 2
    dense[in_g] = 3 + (pos[in_g] - g0) // ANCHOR_SIZE
    dense[in_x] = 3 + ANCHORS + (pos[in_x] - x0)
    at = 3 + ANCHORS + SIZE_X
    dense[m0:s0] = at + np.repeat(np.arange(len(med)), med)
    dense[s0:] = at + len(med) + np.arange(N - s0)
    K = int(dense.max()) + 1
    pid = rng.permutation(np.sort(rng.choice(N, K, replace=False)))   # sparse ids in [0, N), in no order
    anchor_of = lambda r: 3 + (pos[in_x] - x0 + r) % ANCHORS          # noqa: E731

    def row(r):
        kind = r % 10
        raw = dense.copy()
        raw[in_x] = anchor_of(r)
        raw[in_a] = K + rng.integers(0, r % 5 + 2, SIZE_A)
        if kind == 2:
            raw[in_c | loose] = 0
        elif kind == 3:
            raw[in_c | loose] = 2 * K + pos[in_c | loose]
        elif kind >= 4 or r >= 10:
            if kind >= 4:
                pieces = 20 + 3 * r
                raw[in_c] = K + 8 + ((pos[in_c] + 997 * r) % SIZE_C) * pieces // SIZE_C
            q = 0.01 if kind < 4 else 0.03 + 0.02 * kind
            move = loose & (rng.random(N) < q)
            raw[move] = K + 1024 + rng.integers(0, NOISE_POOL, int(move.sum()))
            if kind == 7:
                raw[in_b] = K + 512 + (pos[in_b] - b0 >= SIZE_B // 3)
        _, inv = np.unique(raw, return_inverse=True)
        return rng.permutation(N)[inv.reshape(-1)].astype(np.int32)

    by_pos = np.stack([row(r) for r in range(N_R2)])
    labs = np.empty_like(by_pos)
    labs[:, perm] = by_pos
    part = np.empty(N, np.int32)
    part[perm] = pid[dense]
    # edges: random pairs, and pairs of near positions (so that clusters hold edges)
    ru, rv = rng.integers(0, N, M_RANDOM), rng.integers(0, N, M_RANDOM)
    lu = rng.integers(0, N - 41, M_LOCAL)
    lv = lu + rng.integers(1, 41, M_LOCAL)
    u, v = cref.canonical_edges(perm[np.concatenate([ru, lu])], perm[np.concatenate([rv, lv])])
    # co-association: families of signatures that differ from their base in 0..n_r replicas
    base = rng.integers(0, CA_LABELS, (CA_FAMILIES, CA_N_R))
    sig = base[rng.integers(0, CA_FAMILIES, CA_SIGNATURES)]
    change = rng.random(sig.shape) < rng.random((CA_SIGNATURES, 1))
    sig = np.where(change, rng.integers(0, CA_LABELS, sig.shape), sig)
    ca_labs = np.ascontiguousarray(sig[rng.integers(0, CA_SIGNATURES, N)].T).astype(np.int32)
    ca_nodes = rng.choice(N, CA_K, replace=False)
    ca_nodes[-3:] = ca_nodes[:3]                      # a few listed twice
    # pairs and matrix lists: half of the pairs are near positions, the matrix straddles the end of C
    near = rng.integers(0, N - 41, CA_PAIRS // 2)
    ca_pairs = np.concatenate([rng.integers(0, N, (CA_PAIRS - len(near), 2)),
                               perm[np.stack([near, near + rng.integers(0, 41, len(near))], 1)]])
    ca_a = perm[rng.permutation(np.arange(a0 - 2_000, a0 - 2_000 + CA_NA))]
    ca_b = perm[rng.permutation(np.arange(a0 - 1_500, a0 - 1_500 + CA_NB))]
    q_nodes = np.concatenate([rng.choice(N, 2_000, replace=False) for _ in range(3)] +
                             [perm[c0:c0 + 500], perm[a0:a0 + 500], perm[b0:b0 + 500]])
    q_clusters = np.concatenate([np.repeat(pid[[0, 1, 2]], 2_000), np.repeat(pid[[0, 1, 2]], 500)])
    return {"n": N, "u": u, "v": v, "part": part, "labs70": labs, "reference": labs[11].copy(),
            "ids_cab": pid[[0, 1, 2]].astype(np.int64), "x_nodes": perm[x0:m0].copy(),
            "medium_ids": pid[at:at + len(med)].astype(np.int64),
            "ca_labs": ca_labs, "ca_nodes": ca_nodes.astype(np.int32),
            "ca_pairs": rng.permutation(ca_pairs).astype(np.int32),
            "ca_a": ca_a.astype(np.int32), "ca_b": ca_b.astype(np.int32),
            "q_nodes": q_nodes.astype(np.int32), "q_clusters": q_clusters.astype(np.int32)}


# ------------------------------------------------------------------ the references
def _cluster_case(labs, part, k):
    """cluster_consensus_ref.sums plus the fallback's prediction for the labelings `labs`"""
    ids, size, pairs, item = ccr.sums(labs, part)
    cells = cluster_cells(labs, part)
    over = lane_overflow(cells[2], size, k["SC_D"], k["LCAP"])
    return {"ids": ids, "size": size, "pairs": pairs, "item": item, "cells": cells, "over": over,
            "slow_members": int((over * size[None, :]).sum())}


def _rows(c, i):
    return c["reference"] if i < 0 else c["labs20"][i]


def _affinity(n_r, nodes, clusters):
    return lambda c: sparse_affinity(c["labs%d" % n_r], c["part"], c[nodes], c[clusters], c["cc%d" % n_r]["cells"])


# every reference the GPU tests compare with, by the key it has in the case
REFS = {
    "cc20": lambda c: _cluster_case(c["labs20"], c["part"], caps()),
    "cc70": lambda c: _cluster_case(c["labs70"], c["part"], caps()),
    "vote20": lambda c: vr.vote(c["labs20"], c["part"]),
    "map70": lambda c: vr.map_labelings(c["labs70"], c["part"]),
    # the candidates of core.median_refine's first round: (v, top[v]) where the vote differs from P
    "cand_nodes": lambda c: np.flatnonzero(c["vote20"]["top"] != c["part"]).astype(np.int32),
    "cand_clusters": lambda c: c["vote20"]["top"][c["cand_nodes"]].astype(np.int32),
    "all_nodes": lambda c: np.arange(c["n"], dtype=np.int32),
    "aff_own20": _affinity(20, "all_nodes", "part"),
    "aff_cand20": _affinity(20, "cand_nodes", "cand_clusters"),
    "aff_cand70": _affinity(70, "cand_nodes", "cand_clusters"),
    "aff_q20": _affinity(20, "q_nodes", "q_clusters"),
    "aff_q70": _affinity(70, "q_nodes", "q_clusters"),
    "parts20": lambda c: [score_ref.part(row, c["u"], c["v"]) for row in c["labs20"]],
    "pairs20": lambda c: [score_ref.pair(_rows(c, a), _rows(c, b)) for a, b in SCORE_PAIRS],
    "sup20": lambda c: cref.support(c["labs20"], c["u"], c["v"]),
    "partitions": lambda c: [cref.partition(c["n"], c["u"], c["v"], th, sup=c["sup20"], n_total=N_R) for th in THETAS],
    "tree": lambda c: lref.tree(c["n"], c["u"], c["v"], c["sup20"], N_R),
    "levels": lambda c: lref.level_records(c["n"], c["u"], c["v"], c["sup20"], N_R, birth=c["tree"][0], up=c["tree"][1]),
    "cuts": lambda c: [lref.cut(c["tree"][0], c["tree"][1], s) for s in CUT_LEVELS],
    "ca_hist": lambda c: hist_by_signature(c["ca_labs"], c["ca_nodes"]),
    "ca_pairs_ref": lambda c: car.pairs(c["labs20"], c["ca_pairs"]),
    "ca_matrix": lambda c: np.concatenate([car.matrix(c["labs20"], c["ca_a"][lo:lo + 512], c["ca_b"])
                                           for lo in range(0, CA_NA, 512)]),
}


class Case(dict):
    """inputs() plus the references of REFS, each computed when it is first asked for; `seconds`
    holds what each took (without the references it asked for in turn).  Treat it as read-only."""

    def __init__(self):
        super().__init__(inputs())
        self["labs20"] = self["labs70"][:N_R]
        self.seconds = {}
        self._nested = [0.0]

    def __missing__(self, key):
        t0 = time.perf_counter()
        self._nested.append(0.0)
        self[key] = val = REFS[key](self)
        spent = time.perf_counter() - t0
        self.seconds[key] = spent - self._nested.pop()
        self._nested[-1] += spent
        return val

    def compute_all(self):
        for key in REFS:
            self[key]
        return self


def build(refs=True):
    """The inputs as a dict of arrays; with `refs` a Case with every reference computed."""
    return Case().compute_all() if refs else dict(Case())


@functools.lru_cache(maxsize=None)
def case():
    """one Case per process"""
    return Case()


# ------------------------------------------------------------------ what the case reaches
def _fallback_runs(row_a, row_b, k):
    """(keys, runs) the scoring fallback of the pair (row a, lane b) handles: the members, and the
    distinct b-labels, of a's communities with more than SC_D b-labels or more than LCAP members"""
    _, ia = dense_ids(row_a)
    _, ib = dense_ids(row_b)
    size = np.bincount(ia)
    cell = np.unique(ia * (int(ib.max()) + 1) + ib) // (int(ib.max()) + 1)
    distinct = np.bincount(cell, minlength=len(size))
    over = (distinct > k["SC_D"]) | (size > k["LCAP"])
    return int(size[over].sum()), int(distinct[over].sum())


def reached(c):
    """{name: (value, relation, cap)}: per clamp, list cap and 32-bit limit of the analysis kernels,
    the quantity of the case that must stand in `relation` (">", "==" or "<=") to it, computed from
    the inputs and the references alone, and the cap itself, read from the csrc headers."""
    k = caps()
    tb = k["TB"]
    cc20, cc70, v20 = c["cc20"], c["cc70"], c["vote20"]
    size, labs20 = cc20["size"], c["labs20"]
    rank = {x: int(np.searchsorted(cc20["ids"], i)) for x, i in zip("CAB", c["ids_cab"])}
    member = {x: np.flatnonzero(c["part"] == i) for x, i in zip("CAB", c["ids_cab"])}
    whole = lambda r, x: len(np.unique(labs20[r][member[x]])) == 1          # noqa: E731
    med = np.searchsorted(cc20["ids"], c["medium_ids"])
    med = med[size[med] > k["SC_D"]]                                          # the medium clusters that could overflow
    chunk = max(2 * c["n"], k["CHUNK"])
    keys23, runs23 = _fallback_runs(labs20[2], labs20[3], k)
    bank0 = int((cc70["over"][:64] * cc70["size"][None, :]).sum())            # the vote map works bank by bank
    deg = np.bincount(c["u"], minlength=c["n"]) + np.bincount(c["v"], minlength=c["n"])
    tiles = -(-len(c["ca_nodes"]) // k["CA_T"])
    two32 = 1 << 32
    return {
        "SC_GRID: clusters of P": (len(size), ">", 4 * k["SC_GRID"]),
        "SC_GRID: communities of every scored row": (min(c["parts20"][a]["k"] for a in (0, 3, 14)), ">", 4 * k["SC_GRID"]),
        "SC_GRID: queried clusters": (len(np.unique(c["part"])), ">", 4 * k["SC_GRID"]),
        "score.h edge kernel: edges": (len(c["u"]), ">", k["SC_GRID"] * tb),
        "LCAP: the cluster B": (int(size[rank["B"]]), "==", k["LCAP"]),
        "LCAP: B's lanes on the register path": (int((~cc20["over"][:, rank["B"]]).sum()), "==", N_R),
        "LCAP: the cluster A": (int(size[rank["A"]]), ">", k["LCAP"]),
        "LCAP: the cluster C": (int(size[rank["C"]]), ">", max(k["LCAP"], 65536)),
        "labelings that keep B whole": (sum(whole(r, "B") for r in range(N_R)), ">", 16),
        "nodes of C that rows 0 and 1 both keep together": (len(member["C"]) * (whole(0, "C") and whole(1, "C")), ">", 65536),
        "summed degree of C": (int(deg[member["C"]].sum()), ">", 65536),
        "SC_D: medium lanes past the list": (int(cc20["over"][:, med].sum()), ">", 0),
        "SC_D: medium lanes within the list": (int((~cc20["over"][:, med]).sum()), ">", 0),
        "k_cc_total: clusters": (len(size), ">", k["k_cc_total"] * tb),
        "k_vc_flags: nodes": (c["n"], ">", k["k_vc_flags"] * tb),
        "k_ia_slow: queries x banks": (c["n"] * ((N_R + 63) // 64), ">", k["k_ia_slow"] * tb),
        "k_sc_fold: runs of the pair (2, 3)": (runs23, ">", k["k_sc_fold"] * tb),
        "k_sc_fold: and its keys are one chunk": (keys23, "<=", chunk - c["n"]),
        "k_vc_slow: nodes with more than VT_D voted clusters": (int((v20["distinct"] > k["VT_D"]).sum()), ">", k["k_vc_slow"]),
        "k_cc_fold: fallback pairs, 20 labelings": (cc20["slow_members"], ">", k["k_cc_fold"] * tb),
        "k_vm_fold: fallback pairs, first bank of 70": (bank0, ">", k["k_vm_fold"] * tb),
        "k_cc_emit: keys of the first chunk, 70 labelings": (min(chunk, cc70["slow_members"]), ">", k["k_cc_emit"] * tb),
        "k_ia_lookup: (query, lane) threads": (c["n"] * 64, ">", k["k_ia_lookup"] * tb),
        "chunk budget: fallback pairs, 70 labelings": (cc70["slow_members"], ">", chunk),
        "chunk budget: the vote map's first bank of 70": (bank0, ">", chunk),
        "chunk budget: affinity queries into A, B and C, 70 labelings":
            (int((cc70["over"][:, [rank["A"], rank["C"]]] * cc70["size"][None, [rank["A"], rank["C"]]]).sum()), ">", chunk),
        "CP_HIST_GRID: edges": (len(c["u"]), ">", k["CP_HIST_GRID"] * tb),
        "LV_GRID: edges": (len(c["u"]), ">", k["LV_GRID"] * tb),
        "coassoc.h tile map: tiles of the triangle (136 in the other tests)": (tiles * (tiles + 1) // 2, ">", 10 ** 5),
        "coassoc_hist: distinct signatures": (len(np.unique(c["ca_labs"][:, c["ca_nodes"]].T, axis=0)), "<=", 4096),
        "coassoc_hist: listed nodes": (len(c["ca_nodes"]), ">", 92_699),
        "coassoc_hist: bins other than 0 and n_r": (int((c["ca_hist"][1:-1] > 0).sum()), ">", 0),
        "2^32: pairs[B]": (int(cc20["pairs"][rank["B"]]), ">", two32),
        "2^32: pairs_total": (int(cc20["pairs"].sum()), ">", two32),
        "2^32: sum_sq of the pair (0, 1)": (c["pairs20"][0]["sum_sq"], ">", two32),
        "2^32: sum_sq of a partition": (c["parts20"][0]["sum_sq"], ">", two32),
        "2^32: tot_sq": (c["parts20"][0]["tot_sq"], ">", two32),
        "2^32: coassoc_hist's pairs": (int(c["ca_hist"].sum()), ">", two32),
        "2^32: coassoc_hist's largest bin": (int(c["ca_hist"].max()), ">", two32),
    }
