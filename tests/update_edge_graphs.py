"""Deterministic inputs for the consensus update (threshold, triadic closure, isolate repair,
merge/rebuild) on the paths no whole run reaches, one builder per case, and the CPU model of each:
tests/test_update_edge_cases.py asserts, without a GPU, that every input reaches its path;
tests/test_gpu_update_edges.py compares the device with the CPU model bit for bit.

    caps()       N = 100,000, 600,000 drawn edges, 1,400,000 attempts: the C graph passes the
                 2048 x 256 entries one trip of k_cgraph_old / k_cgraph_new covers (clo_append)
    star()       a centre and 40 leaves, 20,000 attempts: every draw lands in one neighbourhood
    hub()        a centre of 5,000 leaves among 60,000 random edges: long kept rows, long C rows
    chain(n)     a path whose sawtooth weights make repair chains 63 deep, every edge dropped
    ring(k)      64 nodes and 0..17 attempts: fewer attempts than closure blocks
    lanes(n_r)   labelings of the LFR-1k graph for every lane-group width of k_pair_partial
    keep(tau, n_p)   every count weight 0..n_p, for the float64 keep rule

A Case holds the graph and one Round per consensus iteration (labelings in node order, n_p, tau,
attempts).  twin() drives tests/cpu_engine.OracleEngine through the step API on the engine's
internal numbering; facts() reads from its records what the case was built to reach."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

from oracle import oracle as orc
from tests.cpu_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = 0.02

Round = namedtuple("Round", "lab n_p tau attempts")
Case = namedtuple("Case", "name seed n u v rounds")
# one consensus iteration of the CPU model: the kept graph, the candidates (key-sorted, internal
# ids; cf = first attempt), their co-membership counts, what the two applies returned, and the
# graph after closure_apply in node ids (fc_get_graph's order)
Record = namedtuple("Record", "kept cu cv cf counts conv1 kept_m unconv conv2 m repaired graph")


class Buf:
    """what OracleEngine's step calls take for a device buffer: anything with .numpy()"""

    def __init__(self, n):
        self.a = np.zeros(max(int(n), 1), np.int32)

    def numpy(self):
        return self.a


# ------------------------------------------------------------------ the grid cap, read from the source
@functools.lru_cache(maxsize=None)
def grid_cap():
    """entries one trip of k_cgraph_old / k_cgraph_new covers: the block cap of clo_append's two
    launches (consensus.hip) times TB"""
    with open(os.path.join(ROOT, "fastconsensus_amd", "csrc", "consensus.hip")) as f:
        src = f.read()
    tb = re.search(r"static constexpr int TB = (\d+);", src)
    caps = re.findall(r"const unsigned [on]g = \(unsigned\)std::max<int64_t>\(1, std::min<int64_t>\(nblk\(2 \* \w+\), (\d+)\)\);", src)
    assert tb and len(caps) == 2 and caps[0] == caps[1], "consensus.hip clo_append no longer caps its two grids as read here"
    return int(caps[0]) * int(tb.group(1))


# ------------------------------------------------------------------ the inputs
def _random_labels(rng, n_p, n, labels=3):
    return rng.integers(0, labels, (n_p, n)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def caps():
    """(a) closure past the grid caps; tau = 0 keeps every edge, 4 labelings over 3 labels vary
    the closure weights"""
    rng = np.random.default_rng(20250301)
    n, m = 100_000, 600_000
    u, v = rng.integers(0, n, m).astype(np.int32), rng.integers(0, n, m).astype(np.int32)
    return Case("caps", 11, n, u, v, (Round(_random_labels(rng, 4, n), 4, 0.0, 1_400_000),))


@functools.lru_cache(maxsize=None)
def star():
    """(b) one hot neighbourhood: centre 0, leaves 1..40"""
    rng = np.random.default_rng(20250302)
    n = 41
    u, v = np.zeros(n - 1, np.int32), np.arange(1, n, dtype=np.int32)
    return Case("star", 12, n, u, v, (Round(_random_labels(rng, 4, n), 4, 0.0, 20_000),))


@functools.lru_cache(maxsize=None)
def hub():
    """(c) a hub among ordinary rows: centre 0 joined to 5,000 leaves, 60,000 random edges among
    the leaves (mean kept row 25: past has_edge_row's 16)"""
    rng = np.random.default_rng(20250303)
    leaves, m = 5_000, 60_000
    n = leaves + 1
    u = np.concatenate([np.zeros(leaves, np.int64), rng.integers(1, n, m)]).astype(np.int32)
    v = np.concatenate([np.arange(1, n), rng.integers(1, n, m)]).astype(np.int32)
    return Case("hub", 13, n, u, v, (Round(_random_labels(rng, 4, n), 4, 0.0, 60_000),))


CHAIN_NP = 64


def chain_weights(n):
    """w_t of the path's edge (t, t + 1): a sawtooth 63, 62, .., 1, 63, .."""
    return (63 - np.arange(n - 1) % 63).astype(np.int32)


@functools.lru_cache(maxsize=None)
def chain(n):
    """(e) the path 0-1-..-(n-1), n_p = 64.  Round 0 (tau 0, no attempts): replica r splits the
    edge t iff k_t = n_p - w_t >= r, so k_t is the highest replica that does and the Louvain rule
    gives 1 + (n_p - 1 - k_t) = w_t.  Round 1 (tau 1, no attempts): replica 63 puts every node
    alone, the others are constant, so the weights stay (w + n_p - 1 - 63), every edge is dropped
    and every node is an isolate whose target is its lighter edge's other end."""
    w = chain_weights(n)
    k = CHAIN_NP - w
    lab0 = np.zeros((CHAIN_NP, n), np.int32)
    for r in range(CHAIN_NP):
        lab0[r, 1:] = np.cumsum(k >= r)
    lab1 = np.zeros((CHAIN_NP, n), np.int32)
    lab1[CHAIN_NP - 1] = np.arange(n)
    t = np.arange(n - 1, dtype=np.int32)
    return Case("chain%d" % n, 14, n, t, t + 1, (Round(lab0, CHAIN_NP, 0.0, 0), Round(lab1, CHAIN_NP, 1.0, 0)))


def chain_targets(n):
    """the repair target of every node of chain(n): its neighbour over the lighter edge (the two
    weights of an inner node differ, so no tie-break enters)"""
    w = chain_weights(n).astype(np.int64)
    left = np.concatenate([[1 << 30], w])          # weight of (t - 1, t)
    right = np.concatenate([w, [1 << 30]])         # weight of (t, t + 1)
    assert (left != right).all()
    t = np.arange(n)
    return np.where(right < left, t + 1, t - 1)


def jacobi(target):
    """repair()'s fixpoint restated in numpy, every node an isolate: all active at first; a sweep
    marks the targets of the active nodes that come later in node order, and who is marked turns
    inactive.  (active, sweeps until one changes nothing: that last one counted)."""
    n = len(target)
    t = np.arange(n)
    active = np.ones(n, bool)
    sweeps = 1                                      # the first pass: all active
    while True:
        hit = np.zeros(n, bool)
        src = active & (target > t)
        hit[target[src]] = True
        sweeps += 1
        if np.array_equal(~hit, active):
            return active, sweeps
        active = ~hit


RING_N = 64
RING_ATTEMPTS = (0, 1, 3, 5, 15, 16, 17)
# node-id pairs for closure_set_pairs: (61, 63) closes 61-62-63; a self pair; (61, 63) again, both
# ways round; an edge of the ring; (63, 1), which closes 63-0-1; and the ring's last edge (63, 0)
RING_PAIRS = np.array([[61, 63], [5, 5], [61, 63], [63, 61], [10, 11], [63, 1], [63, 0]], np.int32)


@functools.lru_cache(maxsize=None)
def ring(attempts):
    """(f) a ring of 64 nodes (ids fill key_bits exactly), every edge kept"""
    rng = np.random.default_rng(20250306)
    t = np.arange(RING_N, dtype=np.int32)
    return Case("ring%d" % attempts, 15, RING_N, t, (t + 1) % RING_N,
                (Round(_random_labels(rng, 4, RING_N), 4, 0.0, attempts),))


LANE_N_R = (1, 2, 4, 5, 8, 9, 16, 17, 63, 64, 65, 129)


def lane_group(n_r):
    """launch_pair_partial's G: lanes per edge, one 16-byte pack of 4 replicas per lane and trip"""
    chunks, g = (n_r + 3) // 4, 1
    while g < chunks and g < 16:
        g <<= 1
    return g


def lane_positions(n_r):
    """where the crafted labelings put their only non-constant replica: first, last, and the four
    positions of the last whole 16-byte pack (of the only pack if n_r < 4)"""
    q = max(n_r // 4 - 1, 0)
    return sorted({0, n_r - 1} | {p for p in range(4 * q, 4 * q + 4) if p < n_r})


def lanes(n_r, n):
    """(g) labelings [n_r][n] for k_pair_partial: one random set over 3 labels, then per position
    of lane_positions a set whose only replica that splits anything sits there"""
    rng = np.random.default_rng(20250307 + n_r)
    sets = [("random", _random_labels(rng, n_r, n))]
    for p in lane_positions(n_r):
        lab = np.zeros((n_r, n), np.int32)
        lab[p] = rng.integers(0, 3, n)
        sets.append((p, lab))
    return sets


def pair_partial(lab, u, v, algo):
    """consensus_partial / closure_partial in numpy: algo 0 the highest replica that splits the
    pair (-1: none), else the number that keep it together"""
    diff = lab[:, u] != lab[:, v]
    if algo == 0:
        last = lab.shape[0] - 1 - np.argmax(diff[::-1], axis=0)
        return np.where(diff.any(0), last, -1).astype(np.int32)
    return (~diff).sum(0).astype(np.int32)


# (tau, n_p).  The first four products are whole numbers in float64 (0.7 * 10 == 7.0, 0.1 * 30 ==
# 3.0): the weight equal to the cut is kept.  0.07 * 100 and 0.14 * 50 round to 7.000000000000001,
# so weight 7 is dropped; 0.58 * 50 rounds to 28.999999999999996, so weight 29 is kept.
KEEP_RULES = ((0.7, 10), (0.2, 5), (0.6, 5), (0.1, 30), (0.07, 100), (0.14, 50), (0.58, 50))


@functools.lru_cache(maxsize=None)
def keep(tau, n_p):
    """(h) a path of 4 (n_p + 1) + 3 nodes whose edge t is co-clustered by the replicas below
    c_t = t mod (n_p + 1): under the count rule every weight 0..n_p occurs"""
    n = 4 * (n_p + 1) + 3
    c = np.arange(n - 1) % (n_p + 1)
    lab = np.zeros((n_p, n), np.int32)
    for r in range(n_p):
        lab[r, 1:] = np.cumsum(c <= r)
    t = np.arange(n - 1, dtype=np.int32)
    return Case("keep%g_%d" % (tau, n_p), 16, n, t, t + 1, (Round(lab, n_p, tau, 0),))


# ------------------------------------------------------------------ the CPU model
def internal_labels(lab, sigma):
    """OracleEngine.lab holds labels by internal id"""
    li = np.empty_like(lab)
    li[:, sigma] = lab
    return li


def new_twin(case, sigma):
    cpu = OracleEngine(case.seed, sigma=sigma)
    cpu.load_graph(case.n, case.u, case.v)
    return cpu


def twin_update(cpu, algo, rnd):
    """set_labels, consensus_partial, consensus_apply on the CPU model -> (conv, kept, unconv)"""
    cpu.lab = internal_labels(rnd.lab, cpu.sigma)
    cpu.r0 = 0
    part = Buf(cpu.m + 1)
    cpu.consensus_partial(algo, part)
    return cpu.consensus_apply(algo, rnd.n_p, rnd.tau, DELTA, part)


def twin_close(cpu, algo, rnd, it, applied):
    """closure_partial and closure_apply on the model's candidates -> the round's Record"""
    conv1, kept_m, unconv = applied
    cu, cv, cf = cpu.cand
    kept = cpu.kept
    counts = Buf(len(cu))
    cpu.closure_partial(counts)
    conv2, m = cpu.closure_apply(algo, rnd.n_p, DELTA, counts if algo != 1 else None, it)
    return Record(kept, cu, cv, cf, counts.numpy()[:len(cu)].copy(), conv1, kept_m, unconv, conv2, m,
                  m - kept.m - len(cu), cpu.get_graph())


def twin_set_pairs(cpu, algo, rnd, pairs):
    """closure_set_pairs on the CPU model: orc.closure_from_pairs of the node-id pairs, candidates
    key-sorted as the device keeps them; returns closure_from_pairs' own weights in that order"""
    p = cpu.sigma[np.asarray(pairs, np.int32).reshape(-1, 2)]
    cu, cv, cw, cf = orc.closure_from_pairs(algo, cpu.kept, p, cpu.lab, rnd.n_p)
    order = np.lexsort((cv, cu))
    cpu.cand = (cu[order], cv[order], cf[order])
    return cw[order]


_TWINS = {}


def twin(case, algo, sigma=None):
    """The case's rounds on the CPU model, one Record each; sigma: the engine's node map (None:
    orc.device_sigma of the case's seed, which the engine's is pinned to).  One per (case, algo)
    and numbering is kept; treat it as read-only."""
    sigma = orc.device_sigma(case.n, case.seed) if sigma is None else np.asarray(sigma, np.int32)
    got = _TWINS.get((case.name, algo))
    if got is not None and np.array_equal(got[0], sigma):
        return got[1]
    cpu = new_twin(case, sigma)
    recs = []
    for it, rnd in enumerate(case.rounds):
        applied = twin_update(cpu, algo, rnd)
        assert cpu.closure_sample(rnd.attempts, it) == len(cpu.cand[0])
        recs.append(twin_close(cpu, algo, rnd, it, applied))
    _TWINS[(case.name, algo)] = (sigma, recs)
    return recs


def forget(name):
    """drop the kept models of a case (the large one holds some 200 MB)"""
    for key in [k for k in _TWINS if k[0] == name]:
        del _TWINS[key]


# ------------------------------------------------------------------ what a closure reaches
def blocks_of(algo, attempts):
    """(R, the blocks' first attempts and the end): clo_bufs' b.R = min(blocks, attempts)"""
    r = max(1, min(orc.closure_rounds(algo), max(int(attempts), 1)))
    return r, np.array([attempts * b // r for b in range(r + 1)], np.int64)


def sample_pairs(case, algo, rec, it=0):
    """the sampler's pair of every attempt (internal ids; (-1, -1): the node has < 2 neighbours)"""
    return orc.closure_sample_pairs(rec.kept, case.rounds[it].attempts, case.seed, it, orc.closure_rounds(algo))


def closure_facts(case, algo, rec, it=0):
    """From the model's candidates: per block their number; the entries the C graph holds after
    each block that grows it (the last does not: clo_append returns early), which are what
    k_cgraph_new writes in that block and k_cgraph_old moves in the next; the most entries one
    block adds to one C row; the longest C row a block draws from; the kept rows."""
    attempts = case.rounds[it].attempts
    r, bounds = blocks_of(algo, attempts)
    block = np.searchsorted(bounds, rec.cf, side="right") - 1
    per_block = np.bincount(block, minlength=r)[:r]
    grown = block < r - 1
    gain = 0
    for b in range(r - 1):
        ends = np.concatenate([rec.cu[block == b], rec.cv[block == b]])
        if len(ends):
            gain = max(gain, int(np.bincount(ends).max()))
    crow = np.bincount(np.concatenate([rec.cu[grown], rec.cv[grown]]), minlength=case.n)
    kdeg = rec.kept.degrees()
    return {"blocks": r, "per_block": per_block.tolist(), "candidates": int(len(rec.cu)),
            "new_entries": (2 * per_block[:r - 1]).tolist(),
            "old_entries": (2 * np.cumsum(per_block)[:max(r - 2, 0)]).tolist(),
            "before_last": int(per_block[:r - 1].sum()),
            "row_gain": gain, "longest_c_row": int(crow.max()), "longest_kept_row": int(kdeg.max()),
            "long_row_candidates": int((kdeg[rec.cu] > 16).sum())}


def draw_facts(case, algo, rec, world=3, it=0):
    """From the sampler's pairs: the valid draws (a pair of distinct neighbours), and per block the
    candidates drawn in more than one of `world` ranks' sub-ranges (tests/test_gpu_parity.
    _sharded_closure's split): k_closure_insert then meets the key again, in any rank order."""
    pairs = sample_pairs(case, algo, rec, it).astype(np.int64)
    r, bounds = blocks_of(algo, case.rounds[it].attempts)
    key = (np.minimum(pairs[:, 0], pairs[:, 1]) << 32) | np.maximum(pairs[:, 0], pairs[:, 1])
    valid = pairs[:, 0] >= 0
    cand_key = (rec.cu.astype(np.int64) << 32) | rec.cv
    cand_block = np.searchsorted(bounds, rec.cf, side="right") - 1
    shared = []
    for b in range(r):
        t0, t1 = int(bounds[b]), int(bounds[b + 1])
        seen = np.zeros(int((cand_block == b).sum()), np.int64)
        mine = np.sort(cand_key[cand_block == b])
        for g in range(world):
            lo, hi = t0 + (t1 - t0) * g // world, t0 + (t1 - t0) * (g + 1) // world
            k = np.unique(key[lo:hi][valid[lo:hi]])
            seen += np.isin(mine, k)
        shared.append(int((seen > 1).sum()))
    return {"valid_draws": int(valid.sum()), "shared_by_ranks": shared}
