"""The mid-size case of tests/analysis_mid.py for fc_community_quality (tests/test_quality_mid_cases.py,
tests/test_gpu_analysis_mid.py): five partitions of its 400,003 nodes on its 797,200 edges.

    part          P itself: 269,747 clusters, C (66,000 members) in thousands of parts
    coarse        labs70[2]: one giant community of 358,519 nodes, 18 clusters in all
    fine          labs70[3]: 358,537 clusters
    moved         P with a seeded 1 % of C's nodes relabelled to the id of an anchor cluster they
                  have no edge to: each lands there as a part of its own
    coarse_split  the coarse row split into its connected parts (the reference's own split): no
                  cluster of the other four that is longer than 65,536 nodes is one component, the
                  largest part of the giant community is

The reference is quality_ref.quality, computed once per partition and process (under a second each
here: the numpy components routine the issue allowed for was not needed).  analysis_mid.py itself
is imported, not changed."""
import functools

import numpy as np

from tests import analysis_mid as am
from tests import quality_ref as qr

NAMES = ("part", "coarse", "fine", "moved", "coarse_split")
MOVED_SEED, MOVED_FRACTION = 977, 0.01


def shard_blocks():
    """CSH of fc_device.h: k_ql_records' blocks add their totals into shard blockIdx % CSH"""
    return int(am._one(r"constexpr int CSH = (\d+);", "fc_device.h").group(1))


def anchor_ids(part):
    """the twelve anchor clusters of P: the only ones of ANCHOR_SIZE members"""
    ids, size = np.unique(part, return_counts=True)
    ids = ids[size == am.ANCHOR_SIZE]
    assert len(ids) == am.ANCHORS
    return ids


def moved_partition(c):
    """(partition, anchor id, moved nodes)"""
    part, u, v = c["part"], c["u"], c["v"]
    anchor = int(anchor_ids(part)[0])
    touches = np.zeros(c["n"], bool)                      # a neighbour in the anchor cluster
    touches[u[part[v] == anchor]] = True
    touches[v[part[u] == anchor]] = True
    free = np.flatnonzero((part == int(c["ids_cab"][0])) & ~touches)
    nodes = np.random.default_rng(MOVED_SEED).choice(free, int(MOVED_FRACTION * am.SIZE_C), replace=False)
    out = part.copy()
    out[nodes] = anchor
    return out, anchor, nodes


@functools.lru_cache(maxsize=None)
def case():
    """{name: (partition int32[n], quality_ref.quality of it)}, one per process"""
    c = am.case()
    n, u, v = c["n"], c["u"], c["v"]
    P = {"part": c["part"], "coarse": c["labs70"][2], "fine": c["labs70"][3], "moved": moved_partition(c)[0]}
    out = {x: (p, qr.quality(n, u, v, None, p)) for x, p in P.items()}
    split = out["coarse"][1]["split"]
    out["coarse_split"] = (split, qr.quality(n, u, v, None, split))
    return out


def wave_clusters(order, labels):
    """Per wave of 64 storage slots, the number of distinct clusters among its nodes; order[i] = the
    node of slot i.  The last wave (n % 64 slots) is left out."""
    lab = np.asarray(labels)[order[:len(order) // 64 * 64]].reshape(-1, 64)
    lab = np.sort(lab, 1)
    return 1 + (lab[:, 1:] != lab[:, :-1]).sum(1)


def reached(c):
    """{name: (value, relation, cap)} as analysis_mid.reached: from the inputs and quality_ref alone,
    the caps read from the csrc headers by name."""
    k = am.caps()
    per_shard = shard_blocks() * k["TB"]                  # clusters one trip over the shards covers
    q = {x: ref for x, (_, ref) in case().items()}
    _, anchor, nodes = moved_partition(c)
    at = int(np.searchsorted(q["moved"]["ids"], anchor))
    whole = np.flatnonzero((q["coarse_split"]["size"] > 65536) & (q["coarse_split"]["components"] == 1))
    out = {
        "k_ql_records: clusters of P share shards": (q["part"]["k"], ">", per_shard),
        "k_ql_records: clusters of the fine row share shards": (q["fine"]["k"], ">", per_shard),
        "union-find: a one-component cluster longer than 2^16": (len(whole), ">", 0),
        "union-find: and its internal edges": (int(q["coarse_split"]["in_edges"][whole].max()), ">", 1000),
        "union-find: the largest part inside the giant community": (int(q["coarse"]["largest_component"].max()), ">", 65536),
        "parts of the anchor cluster the moved nodes land in": (int(q["moved"]["components"][at]), ">", 100),
        "moved nodes": (len(nodes), "==", 660),
        "coarse_split: parts equal clusters": (q["coarse_split"]["parts"], "==", q["coarse_split"]["k"]),
        "coarse_split: disconnected clusters": (q["coarse_split"]["disconnected"], "==", 0),
    }
    for x in ("part", "coarse", "fine", "moved"):
        out["%s: parts beyond its clusters" % x] = (q[x]["parts"], ">", q[x]["k"])
        out["%s: disconnected clusters" % x] = (q[x]["disconnected"], ">", 0)
    return out
