"""fastconsensus_amd -- MI355X-native fast consensus clustering (Tandon et al., PRE 2019).

Drop-in for ytabatabaee/fastconsensus's ``fast_consensus()`` hot path (louvain + lpm):
the n_p community-detection runs and the consensus-graph update run as hand-written
HIP kernels for gfx950 behind a C-ABI (include/fastconsensus_amd.h).
"""
from ._lib import FastConsensusError  # noqa: F401
from .core import (Engine, IdGraph, between_consensus, check_consensus_graph, cluster_consensus, cluster_stability, conductance, consensus_cdf,  # noqa: F401
                   cut_tree, density, device_bytes, dissolved, fast_consensus, group_to_partition, item_consensus,
                   jaccard, labels_to_output, level_of, match_f1, median_moves, median_objective, median_refine, merge_moves,
                   merge_refine, mixing,
                   modularity_share, pac, recovered, split_disconnected, theta_of, vote_refine)

__version__ = "0.1.0"
