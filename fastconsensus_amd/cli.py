"""Command line drop-in for ``python fast_consensus.py`` (fast_consensus.py:414-466).

Same flags, defaults, validation messages and exit status, same output tree:
``out_partitions_t{tau}_d{delta}_np{n_p}/1..n_p`` and ``memberships_t.../0..n_p-1``
(louvain only; the directory is created for every algorithm).  Additive flags:
``--seed`` (the reference is unseeded), ``--device`` and ``--consensus THETA``, which also writes
the consensus partition (``Engine.consensus_partition``) to ``consensus_t.../partition`` (one
community per line) and ``consensus_t.../membership`` (``node+1<TAB>community+1``, sorted by node).
``--consensus-levels`` picks the threshold itself (``Engine.consensus_levels``): the same two
files hold the level of largest modularity, and ``consensus_t.../levels.tsv`` one row per level.
``--coassoc K`` writes, beside the output tree, ``coassoc.npy`` (the int32 [K, K] consensus matrix
of K nodes drawn by ``numpy.random.default_rng(seed)``, ``Engine.coassociation``) and
``coassoc_nodes.txt`` (their labels, one per line, in the matrix's order).
``--cluster-consensus`` (with ``--consensus`` or ``--consensus-levels``) adds
``consensus_t.../cluster_consensus.tsv`` (``community+1``, size, pair sum, cluster consensus) and
``consensus_t.../item_consensus.tsv`` (node, ``community+1``, item sum, item consensus with its own
community), no header, floats as ``%.17g`` (``Engine.cluster_consensus``).
``--vote`` (with ``--consensus`` or ``--consensus-levels``) votes on the consensus partition
(``Engine.vote``) and adds ``consensus_t.../vote.tsv``: node, ``community+1``, voted
``community+1``, own votes, top votes; one row per node in node order, no header.
``--median`` (with ``--consensus`` or ``--consensus-levels``) refines the consensus partition (the
fixpoint of ``vote_refine`` with ``--vote``) by exact one-element moves towards the median partition
(``median_refine``) and adds ``consensus_t.../median_membership`` (``membership``'s format) and
``consensus_t.../median.tsv``: one row per round, no header: round, objective, proposed, accepted,
alone (round 0: the objective before the first round, then zeros).
``--quality`` (with ``--consensus`` or ``--consensus-levels``) asks the graph about the consensus
communities (``Engine.community_quality``) and adds ``consensus_t.../quality.tsv``: one row per
community, no header: ``community+1``, size, in_weight, cut, volume, conductance, density,
components, largest_component (floats as ``%.17g``); and ``consensus_t.../split_membership``
(``membership``'s format and row order): the partition split into its connected parts,
``part+1``.  With ``--vote`` / ``--median`` it also writes ``voted_quality.tsv`` (of ``vote.tsv``'s
voted column) / ``median_quality.tsv`` (of ``median_membership``), the same columns.
``--merge`` (with ``--consensus`` or ``--consensus-levels``) runs last, on ``median_membership``'s
partition with ``--median``, else on the fixpoint of ``vote_refine`` with ``--vote``, else on the
consensus partition: cluster merges towards the median partition (``merge_refine``).  It adds
``consensus_t.../merge_membership`` (``membership``'s format) and ``consensus_t.../merge.tsv``: one
row per round, no header: round, objective, k, pairs, proposed, accepted (round 0: the objective
and the clusters before the first round, then zeros).  With ``--quality`` it also writes
``merged_quality.tsv`` (of ``merge_membership``), ``quality.tsv``'s columns.
``--match`` (with ``--consensus`` or ``--consensus-levels``) looks for every consensus community in
the n_p partitions (``Engine.cluster_match``: its best match by Jaccard index) and adds
``consensus_t.../cluster_match.tsv``: one row per community, no header: ``community+1``, size,
stability (the mean Jaccard index, ``%.17g``), recovered, dissolved (the partitions with J >= 3/4,
with J <= 1/2).
"""
import argparse
import os
import sys

from ._lib import FC_ALGO_LOUVAIN, FC_ALGO_LOUVAIN_NC
from .core import (ALGORITHMS, OUT_OF_SCOPE, RULES, Engine, IdGraph, algo_id, best_consensus, coassoc_nodes,
                   labels_to_output, median_refine, merge_refine, theta_of, vote_refine)

DEFAULT_TAU = {'louvain': 0.2, 'cnm': 0.7, 'infomap': 0.6, 'lpm': 0.8}   # :426


def check_arguments(args):
    """fast_consensus.py:73-88 -- identical messages."""
    if args.d > 1:
        print('delta is too high. Allowed values are between 0 and 1')
        return False
    if args.d < 0:
        print('delta is too low. Allowed values are between 0 and 1')
        return False
    if args.alg not in ('louvain', 'lpm', 'cnm', 'infomap', 'leiden'):
        print('Incorrect algorithm entered. run with -h for help')
        return False
    if args.t > 1 or args.t < 0:
        print('Incorrect tau. run with -h for help')
        return False
    return True


def build_parser():
    p = argparse.ArgumentParser(description='Process some integers.')
    p.add_argument('-f', metavar='filename', type=str, nargs='?', help='file with edgelist')
    p.add_argument('-np', metavar='n_p', type=int, nargs='?', default=20,
                   help='number of input partitions for the algorithm (Default value: 20)')
    p.add_argument('-t', metavar='tau', type=float, nargs='?', help='used for filtering weak edges')
    p.add_argument('-d', metavar='del', type=float, nargs='?', default=0.02,
                   help='convergence parameter (default = 0.02). Converges when less than delta proportion '
                        'of the edges are with wt = 1')
    p.add_argument('--alg', metavar='alg', type=str, nargs='?', default='louvain',
                   help='choose from \'louvain\' , \'cnm\' , \'lpm\' , \'infomap\' ')
    p.add_argument('--seed', type=int, default=None, help=argparse.SUPPRESS)
    p.add_argument('--device', type=int, default=0, help=argparse.SUPPRESS)
    # extension: the new_consensus.py fork's weight rule (:155-163), louvain only
    p.add_argument('--rule', type=str, default='fast_consensus', choices=RULES, help=argparse.SUPPRESS)
    # extension: also write the consensus partition at this agreement threshold
    p.add_argument('--consensus', type=float, default=None, help=argparse.SUPPRESS)
    # extension: the consensus hierarchy; writes every level's record and the best level's partition
    p.add_argument('--consensus-levels', action='store_true', help=argparse.SUPPRESS)
    # extension: the consensus matrix of K random nodes
    p.add_argument('--coassoc', type=int, default=None, help=argparse.SUPPRESS)
    # extension: cluster and item consensus of the consensus partition
    p.add_argument('--cluster-consensus', action='store_true', help=argparse.SUPPRESS)
    # extension: plurality vote of the partitions on the consensus partition
    p.add_argument('--vote', action='store_true', help=argparse.SUPPRESS)
    # extension: one-element moves of the consensus partition towards the median partition
    p.add_argument('--median', action='store_true', help=argparse.SUPPRESS)
    # extension: per-community structure on the graph and the split into connected parts
    p.add_argument('--quality', action='store_true', help=argparse.SUPPRESS)
    # extension: cluster merges of the consensus partition towards the median partition
    p.add_argument('--merge', action='store_true', help=argparse.SUPPRESS)
    # extension: cluster-wise Jaccard stability of the consensus partition over the partitions
    p.add_argument('--match', action='store_true', help=argparse.SUPPRESS)
    return p


def output_dirs(args):
    suffix = 't' + str(args.t) + '_d' + str(args.d) + '_np' + str(args.np)
    return 'out_partitions_' + suffix, 'memberships_' + suffix


def write_outputs(args, output, root='.'):
    """fast_consensus.py:440-466.  output: list of dict (louvain) or set of frozensets."""
    out_dir, mem_dir = (os.path.join(root, d) for d in output_dirs(args))
    os.makedirs(out_dir, exist_ok=True)
    os.makedirs(mem_dir, exist_ok=True)
    output = list(output)
    if args.alg == 'louvain':
        for i in range(len(output)):
            with open(mem_dir + '/' + str(i), 'w') as f:
                for k, v in sorted(output[i].items()):
                    f.write(str(k + 1) + "\t" + str(v + 1) + '\n')
            part = {}
            for node, c in output[i].items():      # group_to_partition (:55-71)
                part.setdefault(c, []).append(node)
            output[i] = part.values()
    for i, partition in enumerate(output, start=1):
        with open(out_dir + '/' + str(i), 'w') as f:
            if args.alg == 'leiden':   # :463-466 rewrites the file as vertex -> cluster, 1-based
                for j, mem in enumerate(partition.membership):
                    f.write(str(j + 1) + "\t" + str(mem[0] + 1) + '\n')
                continue
            for community in partition:
                print(*community, file=f)


def write_consensus(args, node_labels, labels, root='.'):
    """consensus_t{tau}_d{delta}_np{n_p}/partition (one community per line, like out_partitions)
    and /membership (node+1 <TAB> community+1, sorted by node).  labels: [n] in node order."""
    d = os.path.join(root, 'consensus_' + output_dirs(args)[0][len('out_partitions_'):])
    os.makedirs(d, exist_ok=True)
    nodes = list(node_labels.tolist())
    part = {}
    for node, c in zip(nodes, labels.tolist()):
        part.setdefault(c, []).append(node)
    with open(os.path.join(d, 'partition'), 'w') as f:
        for c in sorted(part):
            print(*part[c], file=f)
    with open(os.path.join(d, 'membership'), 'w') as f:
        for k, v in sorted(zip(nodes, labels.tolist())):
            f.write(str(k + 1) + "\t" + str(v + 1) + '\n')


def write_levels(args, node_labels, levels, labels, root='.'):
    """consensus_t.../levels.tsv beside the best level's partition and membership
    (write_consensus): one row per level 0..n_total, no header, the columns level, theta,
    bucket_edges, k, max_size, singletons, modularity.  levels: the structured array of
    Engine.consensus_levels."""
    write_consensus(args, node_labels, labels, root=root)
    d = os.path.join(root, 'consensus_' + output_dirs(args)[0][len('out_partitions_'):])
    cols = ('bucket_edges', 'k', 'max_size', 'singletons')
    with open(os.path.join(d, 'levels.tsv'), 'w') as f:
        for s, r in enumerate(levels):
            f.write("\t".join([str(s), repr(theta_of(s, len(levels) - 1))] + [str(int(r[c])) for c in cols]
                              + [repr(float(r['modularity']))]) + '\n')


def write_cluster_consensus(args, node_labels, labels, cc, root='.'):
    """consensus_t.../cluster_consensus.tsv (community+1, size, pairs, value; one row per community
    in label order) and /item_consensus.tsv (node label, community+1, item sum, value; one row per
    node in node order): no header, floats as %.17g.  cc: the dict of Engine.cluster_consensus."""
    d = os.path.join(root, 'consensus_' + output_dirs(args)[0][len('out_partitions_'):])
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, 'cluster_consensus.tsv'), 'w') as f:
        for c, n, p, x in zip(cc["ids"].tolist(), cc["size"].tolist(), cc["cluster_pairs"].tolist(),
                              cc["cluster_consensus"].tolist()):
            f.write("%d\t%d\t%d\t%.17g\n" % (c + 1, n, p, x))
    with open(os.path.join(d, 'item_consensus.tsv'), 'w') as f:
        for v, c, p, x in zip(node_labels.tolist(), labels.tolist(), cc["item_pairs"].tolist(),
                              cc["item_consensus"].tolist()):
            f.write("%s\t%d\t%d\t%.17g\n" % (v, c + 1, p, x))


def write_vote(args, node_labels, labels, vt, root='.'):
    """consensus_t.../vote.tsv (node label, community+1, voted community+1, own votes, top votes;
    one row per node in node order, no header).  vt: the dict of Engine.vote on `labels`."""
    d = os.path.join(root, 'consensus_' + output_dirs(args)[0][len('out_partitions_'):])
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, 'vote.tsv'), 'w') as f:
        for v, c, t, o, tv in zip(node_labels.tolist(), labels.tolist(), vt["top"].tolist(), vt["own_votes"].tolist(),
                                  vt["top_votes"].tolist()):
            f.write("%s\t%d\t%d\t%d\t%d\n" % (v, c + 1, t + 1, o, tv))


def write_median(args, node_labels, md, root='.'):
    """consensus_t.../median_membership (node+1 <TAB> community+1, sorted by node, like membership)
    and /median.tsv (round, objective, proposed, accepted, alone; one row per round from round 0,
    the state before the first, no header).  md: the dict of median_refine."""
    d = os.path.join(root, 'consensus_' + output_dirs(args)[0][len('out_partitions_'):])
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, 'median_membership'), 'w') as f:
        for k, v in sorted(zip(node_labels.tolist(), md["labels"].tolist())):
            f.write(str(k + 1) + "\t" + str(v + 1) + '\n')
    rows = zip(md["objective"], [0] + md["proposed_per_round"], [0] + md["accepted_per_round"],
               [0] + md["alone_per_round"])
    with open(os.path.join(d, 'median.tsv'), 'w') as f:
        for r, (obj, p, a, al) in enumerate(rows):
            f.write("%d\t%d\t%d\t%d\t%d\n" % (r, obj, p, a, al))


def write_merge(args, node_labels, mg, root='.'):
    """consensus_t.../merge_membership (node+1 <TAB> community+1, sorted by node, like membership)
    and /merge.tsv (round, objective, k, pairs, proposed, accepted; one row per round from round 0,
    the state before the first, no header).  mg: the dict of merge_refine."""
    d = os.path.join(root, 'consensus_' + output_dirs(args)[0][len('out_partitions_'):])
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, 'merge_membership'), 'w') as f:
        for k, v in sorted(zip(node_labels.tolist(), mg["labels"].tolist())):
            f.write(str(k + 1) + "\t" + str(v + 1) + '\n')
    rows = zip(mg["objective"], mg["k_per_round"], [0] + mg["pairs_per_round"], [0] + mg["proposed_per_round"],
               [0] + mg["accepted_per_round"])
    with open(os.path.join(d, 'merge.tsv'), 'w') as f:
        for r, row in enumerate(rows):
            f.write("%d\t%d\t%d\t%d\t%d\t%d\n" % ((r,) + row))


def write_match(args, cm, root='.'):
    """consensus_t.../cluster_match.tsv (community+1, size, stability, recovered, dissolved; one row
    per community in id order, no header, the float as %.17g).  cm: the dict of Engine.cluster_match."""
    d = os.path.join(root, 'consensus_' + output_dirs(args)[0][len('out_partitions_'):])
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, 'cluster_match.tsv'), 'w') as f:
        for row in zip(cm["ids"].tolist(), cm["size"].tolist(), cm["stability"].tolist(), cm["recovered"].tolist(),
                       cm["dissolved"].tolist()):
            f.write("%d\t%d\t%.17g\t%d\t%d\n" % ((row[0] + 1,) + row[1:]))


def write_quality(args, node_labels, q, name='quality.tsv', split=True, root='.'):
    """consensus_t.../`name` (community+1, size, in_weight, cut, volume, conductance, density,
    components, largest_component; one row per community in id order, no header, floats as %.17g)
    and, with `split`, /split_membership (node+1 <TAB> part+1, sorted by node, like membership).
    q: the dict of Engine.community_quality."""
    d = os.path.join(root, 'consensus_' + output_dirs(args)[0][len('out_partitions_'):])
    os.makedirs(d, exist_ok=True)
    cols = ("size", "in_weight", "cut", "volume", "conductance", "density", "components", "largest_component")
    with open(os.path.join(d, name), 'w') as f:
        for row in zip(q["ids"].tolist(), *(q[c].tolist() for c in cols)):
            f.write("%d\t%d\t%d\t%d\t%d\t%.17g\t%.17g\t%d\t%d\n" % ((row[0] + 1,) + row[1:]))
    if split:
        with open(os.path.join(d, 'split_membership'), 'w') as f:
            for k, v in sorted(zip(node_labels.tolist(), q["split"].tolist())):
                f.write(str(k + 1) + "\t" + str(v + 1) + '\n')


def write_coassoc(node_labels, ids, matrix, root='.'):
    """coassoc.npy (int32 [K, K]) and coassoc_nodes.txt (the K node labels, one per line, in the
    matrix's order), beside the output tree."""
    import numpy as np
    np.save(os.path.join(root, 'coassoc.npy'), matrix)
    with open(os.path.join(root, 'coassoc_nodes.txt'), 'w') as f:
        for x in node_labels[ids].tolist():
            f.write(str(x) + '\n')


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.t is None:
        args.t = DEFAULT_TAU.get(args.alg, 0.2)
    if check_arguments(args) is False:
        sys.exit(0)                               # quit() -> exit status 0 (:430-432)
    if args.consensus is not None and not 0 <= args.consensus <= 1:
        raise SystemExit("--consensus must lie in [0, 1]")
    if args.consensus is not None and args.consensus_levels:
        raise SystemExit("--consensus and --consensus-levels both write the consensus partition: give one")
    for flag in ("cluster_consensus", "vote", "median", "quality", "merge", "match"):
        if getattr(args, flag) and args.consensus is None and not args.consensus_levels:
            raise SystemExit("--%s needs --consensus or --consensus-levels" % flag.replace("_", "-"))
    cons = ca = cc = vt = md = ql = mg = cm = None
    g = IdGraph.from_edgelist_file(args.f)
    if args.coassoc is not None and not 0 <= args.coassoc <= g.n:
        raise SystemExit("--coassoc must lie in [0, %d], the number of nodes" % g.n)
    algo = algo_id(args.alg)
    if algo is None:
        output = None
    else:
        if args.rule == 'new_consensus' and algo == FC_ALGO_LOUVAIN:
            algo = FC_ALGO_LOUVAIN_NC
        with Engine(device=args.device, seed=args.seed) as eng:
            eng.load_graph(g.n, g.u, g.v)
            labels, _ = eng.run(algo, args.np, args.t, args.d)
            if args.consensus is not None:
                cons = eng.consensus_partition(args.consensus)
            if args.consensus_levels:
                cons = best_consensus(eng)
            if args.cluster_consensus:
                cc = eng.cluster_consensus(cons["labels"])
            if args.vote:
                vt = eng.vote(cons["labels"])
            if args.median:
                md = median_refine(eng, vote_refine(eng, cons["labels"])["labels"] if args.vote else cons["labels"])
            if args.quality:
                ql = {"quality.tsv": eng.community_quality(cons["labels"])}
                if vt is not None:
                    ql["voted_quality.tsv"] = eng.community_quality(vt["top"])
                if md is not None:
                    ql["median_quality.tsv"] = eng.community_quality(md["labels"])
            if args.merge:
                start = md["labels"] if md is not None else \
                    vote_refine(eng, cons["labels"])["labels"] if args.vote else cons["labels"]
                mg = merge_refine(eng, start)
                if args.quality:
                    ql["merged_quality.tsv"] = eng.community_quality(mg["labels"])
            if args.match:
                cm = eng.cluster_match(cons["labels"])
            if args.coassoc is not None:
                ids = coassoc_nodes(g.n, args.coassoc, g.labels, args.seed)
                ca = (ids, eng.coassociation(ids).cpu().numpy())
        output = labels_to_output(args.alg, g.labels, labels)
    if output is None:                            # reference: TypeError on len(None)
        raise SystemExit("fast_consensus returned None")
    write_outputs(args, output)
    if cons is not None and args.consensus_levels:
        write_levels(args, g.labels, cons["levels"], cons["labels"])
    elif cons is not None:
        write_consensus(args, g.labels, cons["labels"])
    if cc is not None:
        write_cluster_consensus(args, g.labels, cons["labels"], cc)
    if vt is not None:
        write_vote(args, g.labels, cons["labels"], vt)
    if md is not None:
        write_median(args, g.labels, md)
    if mg is not None:
        write_merge(args, g.labels, mg)
    if cm is not None:
        write_match(args, cm)
    for name, q in (ql or {}).items():
        write_quality(args, g.labels, q, name=name, split=name == 'quality.tsv')
    if ca is not None:
        write_coassoc(g.labels, *ca)


if __name__ == "__main__":
    main()
