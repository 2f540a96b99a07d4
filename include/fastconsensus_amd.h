/*
 * fastconsensus_amd.h -- C-ABI of the MI355X-native fast-consensus engine.
 *
 * The reference (ytabatabaee/fastconsensus, fast_consensus.py) is a Python script with
 * no FFI; its hot path is the while-loop of fast_consensus() (fast_consensus.py:129-411)
 * plus the community-detection calls it makes.  Each entry point below replaces a span
 * of that loop; the replaced reference lines are cited per function.  A host binds this
 * with ctypes (see fastconsensus_amd/_lib.py and INTEGRATION.md).
 *
 * Conventions
 *   - Plain pointers + sizes; no torch or HIP types in signatures (streams are void*).
 *   - Node ids are 0..n-1 in NODE ORDER (first appearance, as networkx read_edgelist
 *     orders nodes); the host keeps the label<->id map.
 *   - Every function returns 0 on success, a negative FC_E* code on error; the message
 *     is in fc_last_error() (thread-local).  There is no CPU fallback: without a usable
 *     gfx950 device fc_create fails with FC_ENODEV.
 *   - One context per host thread; a context is bound to one GPU and is not thread-safe.
 *   - Host arrays are caller-owned and copied; device buffers are context-owned, except
 *     buffers passed as `void* dev_*` which the caller owns (e.g. torch tensors used as
 *     RCCL all-reduce buffers).
 *   - A context is long-lived and may be used again and again.  A result depends on the seed,
 *     the options in force, the loaded graph (with the working graph and the labelings the
 *     calls since fc_load_graph left) and the call's arguments -- and on nothing else the
 *     context did before: not on earlier graphs, replica counts, algorithms, CD engines,
 *     failed or abandoned calls, nor on timing being on (tests/test_gpu_engine_reuse.py).
 *     The documented exceptions: FC_OPT_RELABEL, FC_OPT_STORE and FC_OPT_SEED apply at the
 *     next fc_load_graph; fc_consensus_cut reads the hierarchy of the last
 *     fc_consensus_levels, kept until the next fc_load_graph; fc_load_graph drops the
 *     reference labeling of fc_score_set_reference and the labelings.
 *     fc_community_quality and fc_community_graph depend on the chosen graph and their arguments
 *     alone and leave graph, labelings, reference, hierarchy and random state as they were;
 *     fc_cluster_coassoc reads the labelings as well and leaves the same.  fc_cluster_match
 *     depends on its arguments and, without `other`, on the labelings; it leaves labelings,
 *     reference, hierarchy, working graph and random state as they were.
 */
#ifndef FASTCONSENSUS_AMD_H
#define FASTCONSENSUS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FC_OK 0
#define FC_EINVAL -1      /* bad argument */
#define FC_ENODEV -2      /* no HIP device / not gfx950 */
#define FC_EHIP -3        /* HIP runtime error */
#define FC_ESTATE -4      /* call out of order (e.g. no graph loaded) */
#define FC_ELIMIT -5      /* a size limit was exceeded */

#define FC_ALGO_LOUVAIN 0 /* fast_consensus.py:141-202 (+ final pass :383-384) */
#define FC_ALGO_LPM 1     /* fast_consensus.py:260-310 (+ final pass :391-392) */
#define FC_ALGO_LOUVAIN_NC 2 /* louvain with new_consensus.py's weight rule (:155-163): an edge of
                                weight w not in {0,n_p} gets the plain co-membership count,
                                others keep w; everything else as FC_ALGO_LOUVAIN */
#define FC_ALGO_LEIDEN 3  /* fast_consensus.py:204-258 (+ final pass :385-388): n_p Leiden runs
                             (leidenalg ModularityVertexPartition, n_iterations=1, :121-123).  On the
                             integer-labelled graphs the CLI reads (:434) the loop's membership
                             lookups are keyed by str(vertex) (:97) and never match an int node
                             (:217), so every consensus weight stays 0, :223-227 removes every
                             edge and check #1 (:229) converges on the empty graph: the result is
                             the final pass on G.  fc_run reports that one iteration (exit 1)
                             without running its discarded CD batch.   */
#define FC_ALGO_INFOMAP 4 /* fast_consensus.py:260-310 with the infomap CD (:267-268, final pass
                             :389-390): the lpm loop (co-membership count, threshold, weight-0
                             closure, check after closure) around igraph community_infomap()
                             (unweighted, trials=10): the two-level map-equation core, best of
                             FC_OPT_INFOMAP_TRIALS runs.   */

typedef struct fc_ctx fc_ctx;

typedef struct fc_stats {
    int32_t iterations;       /* consensus iterations executed (while-loop trips)          */
    int32_t exit_check;       /* 1: louvain check #1 (:172-173); 2: check after closure     */
    int32_t hit_iter_cap;     /* 1 if max_iters stopped the loop (the reference never stops) */
    int32_t n_p;
    int64_t m_final;          /* edges of the graph the final pass ran on                  */
    int64_t partition_edges;  /* sum_iter n_p*m_iter + n_p*m_final                           */
    int64_t cd_sweeps;        /* local-moving / LPA sweeps, summed over replicas            */
    int64_t cd_vertex_visits; /* vertices processed by CD kernels, summed over replicas     */
    int64_t cd_edge_visits;   /* adjacency entries scanned by CD kernels                    */
    double cd_ms;             /* device time per phase (filled when timing is enabled)      */
    double consensus_ms;
    double closure_ms;
    double rebuild_ms;
    double decide_ms;         /* light local-moving kernel (the dominant kernel)            */
    int64_t decide_launches;
    int64_t decide_bytes;     /* algorithmic bytes of those launches */
    /* Leiden / Infomap (leiden.hip): the move/refine decide kernel (k_lv_decide) and the
     * block-per-vertex kernel for long rows (k_lv_heavy), timed per launch like decide_ms;
     * bytes per the model in DESIGN.md (counted on the device) */
    double lv_decide_ms;
    int64_t lv_decide_launches;
    int64_t lv_decide_bytes;
    double lv_heavy_ms;
    int64_t lv_heavy_launches;
    int64_t lv_heavy_bytes;
    /* replica-lane decide kernels (cd_rl.hip k_rl_decide*: the full sweeps of the hybrid,
     * FC_OPT_CD_ENGINE=2, and every sweep at 1); decide_* above covers cd.hip's k_decide_light */
    double rl_decide_ms;
    int64_t rl_decide_launches;
    int64_t rl_decide_bytes;
} fc_stats;

/* ---- lifecycle ---------------------------------------------------------------- */
const char* fc_last_error(void);
const char* fc_version(void);
/* Provenance: the 16-hex hash of the sources, header, compile flags and target the library was
 * compiled from (fastconsensus_amd/build.py source_hash, embedded at compile time). */
const char* fc_build_hash(void);
/* device: HIP ordinal; seed: drives every random choice (CD order/ties, closure). */
int fc_create(int device, uint64_t seed, fc_ctx** out);
void fc_destroy(fc_ctx* ctx);
/* Device bytes currently held by this process's engines through their growable buffers
 * (fc_destroy returns a context's whole share). */
int64_t fc_device_bytes(void);
/* Run all work on an external stream (e.g. torch.cuda.current_stream().cuda_stream).
 * NULL restores the context's own stream. */
int fc_set_stream(fc_ctx* ctx, void* hip_stream);
/* Wait for the context's queued work (device buffers written by the step API are then
 * safe to read from another stream). */
int fc_synchronize(fc_ctx* ctx);
/* 0/1: record HIP events around kernels and fill the *_ms fields of fc_stats. */
int fc_set_timing(fc_ctx* ctx, int enable);
/* Fill *stats with everything accumulated since the last call: the *_ms fields and
 * decide_launches from the recorded HIP events (synchronises the stream) and the CD
 * counters (sweeps, visits, decide_bytes) of every fc_run / fc_cd; then reset both. */
int fc_collect_timing(fc_ctx* ctx, fc_stats* stats);
/* Tunables (0 = default): buckets per sweep, max sweeps per CD run, max iterations. */
int fc_set_params(fc_ctx* ctx, int buckets, int max_sweeps, int max_iters);
#define FC_OPT_BUCKETS 1     /* rounds per CD sweep; 0 (default) = per algorithm: 16 for louvain,
                                louvain_nc and Leiden's level-0 move; 32 for lpm (LPA), Infomap
                                and Leiden's refinement; 4 for Leiden's aggregate-level moves.
                                A value >= 1 applies to all of them.                          */
#define FC_OPT_MAX_SWEEPS 2  /* cap on sweeps per CD run (default 200)                      */
#define FC_OPT_MAX_ITERS 3   /* cap on consensus iterations (default 1000)                  */
#define FC_OPT_CHUNK 4       /* CD visit order granularity: 0 per vertex, 16 (default) chunks */
#define FC_OPT_RELABEL 6     /* 1 (default): engine-internal random vertex numbering (set it
                                before fc_load_graph); results are reported in node order.
                                2: numbered in community order (a one-replica Louvain run at
                                load), for infomap runs, whose union levels gather neighbour
                                state by internal id (louvain / lpm need the random numbering:
                                their visit orders are chunks of consecutive ids).  0: identity */
#define FC_OPT_PRUNE 5       /* 1 (default): once a sweep moves < n/4 vertices, later sweeps visit only vertices with a moved
                                neighbour (GVE-Louvain-style pruning); 0: every vertex       */
#define FC_OPT_TAIL_VISITS 7 /* once no replica visits more than this many vertices in a sweep,
                                the remaining sweeps run in one workgroup per replica (-1, the
                                default: per algorithm, 1024 for Louvain, 4096 for LPA; 0 = off).
                                Same results either way.                                          */
#define FC_OPT_COARSEN 8    /* gmax (default 8; 0 = off): a filtered sweep of V vertices runs its buckets in
                                rounds of g (the largest power of two <= gmax, <= buckets, with V*g <= n),
                                so a small sweep is not 32 latency-bound rounds.  Measured neutral on
                                quality (LFR-100k CD modularity/NMI equal at 0/4/8; LFR-1k consensus NMI
                                0.9035 vs 0.9034 at 0/8) and -18 ms on the LFR-1M run.              */
#define FC_OPT_STORE 9       /* label storage order (set it before fc_load_graph).  1 (default): the
                                replicas' label rows are stored in community order (a one-replica
                                Louvain run at load orders the vertices), so the neighbour-label
                                gathers of a sweep hit nearby lines; 0: internal-id order.  Storage
                                only: results are identical either way.                         */
#define FC_OPT_SEED 10       /* replace the seed fc_create took; everything random after the call
                                (the next fc_load_graph's numbering, CD, closure) follows it     */
#define FC_OPT_CLOSURE_ROUNDS 11  /* triadic closure (:175-190, :292-304) samples from a GROWING graph; the
                                L attempts run in this many consecutive blocks, each drawing from the
                                post-threshold graph plus the earlier blocks' closure edges.  0 (the
                                default): per algorithm -- 4 for louvain / louvain_nc, 16 for lpm and
                                infomap (whose weight-0 closure edges shape the next LPA's topology);
                                1 = every attempt from the post-threshold graph only.             */
#define FC_OPT_PRUNE_MARK 12 /* which neighbours a tracked move marks for the next (filtered) sweep.
                                1 (default): on consensus graphs (weights > 1; Louvain and LPA)
                                tracking starts at sweep 1 and, at each tracked sweep's end, a
                                mover marks only the neighbours whose label differs from its own
                                (fast local moving, Traag et al. 2019); unit-weight graphs keep
                                0.  2: the same marks on every graph (the input graph too).
                                0: every neighbour of a mover, tracking from the first sweep
                                that moves < n/4 vertices.                                       */
#define FC_OPT_INFOMAP_TRIALS 13 /* independent Infomap runs per replica, the smallest codelength kept
                                    (default 10, igraph community_infomap's trials)              */
#define FC_OPT_CD_ENGINE 14  /* louvain / lpm CD batches.  0: the classic engine, a random
                                visit order per replica (FC_OPT_COARSEN / FC_OPT_TAIL_VISITS
                                apply).  1: the replica-lane engine (cd_rl.hip) -- every replica of
                                a batch visits the vertices in ONE shared random order per sweep
                                (ties broken per replica), labels node-major, one wave deciding a
                                vertex for up to 64 replicas; no coarse rounds or tail kernel.
                                2 (default): the hybrid -- a replica's sweeps visit the batch's shared order
                                while they are full and its own order from its first filtered
                                (pruned) sweep on; the replica-lane engine runs the full sweeps of a
                                batch of >= FC_OPT_RL_MIN_REPLICAS replicas, cd.hip everything else.
                                All three are bit-exact against oracle/fc_oracle.c orc_engine_cd
                                (shared = 0 / 1 / 2).                                            */
#define FC_OPT_RL_MIN_REPLICAS 15 /* hybrid: the smallest batch whose full sweeps run on the
                                replica-lane engine (default 8).  Speed only: same results.      */
#define FC_OPT_RL_MIN_VERTICES 16 /* hybrid: ... and the smallest graph (default 262144 vertices;
                                below it cd.hip runs the full sweeps too).  Speed only.          */
#define FC_OPT_DENSE_DIV 17  /* hybrid semantics: a filtered sweep that still visits >= n/dense_div
                                vertices keeps the shared order (single-bucket rounds); default 0
                                = the shared order for full sweeps only (twin: dense_div)        */
int fc_set_option(fc_ctx* ctx, int option, int64_t value);

/* ---- graph (replaces nx.read_edgelist + G.copy() + weight reset, :131-136, :434) ---- */
/* Edge list in input order (ids 0..n-1).  Self loops are dropped, duplicates keep their
 * first occurrence (its position defines the edge's networkx adjacency age); all weights
 * are set to 1 (fast_consensus.py:135-136). */
int fc_load_graph(fc_ctx* ctx, int64_t n, int64_t m, const int32_t* u, const int32_t* v);
int fc_graph_info(fc_ctx* ctx, int64_t* n, int64_t* m, int64_t* m_original);
/* The engine's internal vertex numbering: sigma[node id] = internal id (testing aid). */
int fc_get_node_map(fc_ctx* ctx, int32_t* sigma);
/* graph <- the loaded G (device-to-device; fc_run does this itself, like graph = G.copy()
 * at fast_consensus.py:131).  The step API calls it before a new run. */
int fc_reset_graph(fc_ctx* ctx);
/* Copy the working graph `graph` out: canonical (u<v) sorted by (u,v); any pointer may
 * be NULL. */
int fc_get_graph(fc_ctx* ctx, int32_t* u, int32_t* v, int32_t* w, int64_t* age);

/* Copy out the post-threshold `nextgraph` left by fc_consensus_apply (what the reference
 * passes to check #1, fast_consensus.py:172): canonical, sorted, consensus weights. */
int fc_get_nextgraph(fc_ctx* ctx, int64_t* m, int32_t* u, int32_t* v, int32_t* w, int64_t* age);

/* ---- one-shot driver: fast_consensus(G, algorithm, n_p, thresh, delta) (:129-411) --- */
/* Starts from the loaded G every call (G itself is never modified).  labels_out: [n_p][n] final partitions (community ids renumbered 0..k-1 in node
 * order), may be NULL (then fc_get_labels can fetch them). */
int fc_run(fc_ctx* ctx, int algo, int n_p, double tau, double delta, int32_t* labels_out,
           fc_stats* stats);

/* ---- fine-grained steps (distributed driver; parity tests) ------------------------ */
/* Community detection on the working graph for replicas [replica_begin,
 * replica_begin+replica_count) of n_p_total (:148 / :384 louvain level 0, :270 / :392 LPA,
 * :210-211 / :386-387 Leiden, :268 / :390 Infomap).
 * Randomness depends on (seed, global replica index, iteration), not on the sharding. */
int fc_cd(fc_ctx* ctx, int algo, int replica_begin, int replica_count, int n_p_total,
          int iteration);
/* Replay: install host labelings [count][n] as the local replicas (begin = 0).  Every label
 * must lie in [0, n) (community ids are vertex-sized indices on the device); FC_EINVAL
 * otherwise -- a host with arbitrary ids (1-based, sparse, negative) compacts them first
 * (fastconsensus_amd.Engine.set_labels does). */
int fc_set_labels(fc_ctx* ctx, int count, const int32_t* labels);
/* The local replica range the next fc_get_labels exports: count (n_r), first global index
 * and the run's n_p.  count = 0 before any fc_cd / fc_set_labels. */
int fc_replica_info(fc_ctx* ctx, int* count, int* replica_begin, int* n_p_total);
/* Download local labelings [count][n] (in node order) into host memory or a device buffer of
 * the context's GPU; renumber != 0 -> ids 0..k-1 by first node.  capacity: int32 elements
 * the caller's buffer holds; FC_EINVAL if it is below count * n (nothing is written). */
int fc_get_labels(fc_ctx* ctx, int32_t* labels, int64_t capacity, int renumber);
/* Per-edge partial over the local replicas into caller device buffer dev_out (int32[m]):
 * louvain -> largest global replica index whose labels split the edge, or -1
 * (reduce with MAX); lpm and louvain_nc -> number of local replicas co-clustering it
 * (reduce with SUM). */
int fc_consensus_partial(fc_ctx* ctx, int algo, void* dev_out);
/* Apply the reduced partial: consensus weight rule (:150-159 / :273-280), threshold
 * (:163-168 / :284-288) and, for louvain, check #1 (:172).  kept_out/unconv_out: counts. */
int fc_consensus_apply(fc_ctx* ctx, int algo, int n_p, double tau, double delta,
                       const void* dev_partial, int* converged, int64_t* kept_out,
                       int64_t* unconverged_out);
/* Closure candidates: L attempts drawn on the device (:175-184 / :292-300), or recorded
 * pairs (replay, int32[npairs][2]).  n_cand: new distinct absent edges. */
int fc_closure_sample(fc_ctx* ctx, int64_t attempts, int iteration, int64_t* n_cand);
int fc_closure_set_pairs(fc_ctx* ctx, int64_t npairs, const int32_t* pairs, int iteration,
                         int64_t* n_cand);
/* The same device closure (fast_consensus.py:175-184 / :292-300, the growing nextgraph) with
 * each block's attempts split over ranks (multi-GPU: no rank draws all L attempts).
 * fc_closure_begin returns the block count; block b covers attempts
 * [L*b/blocks, L*(b+1)/blocks).  For b = 0, 1, ... in order: every rank draws its sub-range
 * [t_lo, t_hi) with fc_closure_block_sample -> `count` int64 (key, first attempt) pairs in
 * dev_out (FC_EINVAL if more than `capacity`); the ranks' lists are concatenated (any order)
 * and handed to fc_closure_block_add on every rank.  fc_closure_finish then leaves exactly
 * the candidates fc_closure_sample(L) gives, on every rank. */
int fc_closure_begin(fc_ctx* ctx, int64_t attempts, int iteration, int* blocks);
int fc_closure_block_sample(fc_ctx* ctx, int block, int64_t t_lo, int64_t t_hi, void* dev_out,
                            int64_t capacity, int64_t* count);
int fc_closure_block_add(fc_ctx* ctx, int block, const void* dev_in, int64_t count);
int fc_closure_finish(fc_ctx* ctx, int64_t* n_cand);
/* Per-candidate count of local replicas co-clustering it into dev_out (int32[n_cand]). */
int fc_closure_partial(fc_ctx* ctx, void* dev_out);
/* Add closure edges (louvain weight = reduced count (:186-190); lpm weight 0 (:302-304)),
 * isolate repair for louvain (:193-195), swap graph <- nextgraph (:198 / :307) and run
 * the check (:201 / :309). dev_counts may be NULL for lpm. */
int fc_closure_apply(fc_ctx* ctx, int algo, int n_p, double delta, const void* dev_counts,
                     int iteration, int* converged, int64_t* m_out);

/* ---- scoring the local labelings (those left by fc_run, fc_cd or fc_set_labels) ------- */
/* Read-only for everything a later call can observe; all work on the context's stream; local to
 * a rank.  n = nodes, ln = natural logarithm. */
#define FC_SCORE_REF (-1)          /* pair index of the reference labeling */
#define FC_SCORE_GRAPH_INPUT 0     /* the loaded G, unit weights */
#define FC_SCORE_GRAPH_WORKING 1   /* the working graph with its consensus weights */
typedef struct fc_part_score {
    int64_t k;            /* communities */
    int64_t max_size;     /* size of the largest */
    int64_t sum_sq;       /* sum_c size_c^2 */
    int64_t in_weight;    /* sum of w_uv over edges inside a community, each edge once */
    uint64_t tot_sq_lo;   /* sum_c (sum_{v in c} weighted degree_v)^2, exact, 128 bits */
    uint64_t tot_sq_hi;
    double s_log;         /* sum_c size_c ln size_c */
    double entropy;       /* ln n - s_log / n */
    double modularity;    /* 2 in_weight / W2 - tot_sq / W2^2, W2 = total weighted degree; 0 if W2 = 0 */
} fc_part_score;
typedef struct fc_pair_score {
    int32_t a, b;         /* local replica indices, or FC_SCORE_REF */
    int64_t cells;        /* nonzero cells n_ij of the contingency table */
    int64_t sum_sq;       /* sum n_ij^2 */
    int64_t slow_members; /* vertices of this pair the exact fallback handled (diagnostic) */
    double s_log;         /* sum n_ij ln n_ij */
    double mi;            /* ln n + (s_log_ab - s_log_a - s_log_b) / n, clamped at 0 */
    double nmi;           /* mi / ((H_a + H_b) / 2) (sklearn's arithmetic normalisation); 1 when both
                             have one community, else 0 when mi <= 0 */
    double ari;           /* adjusted Rand index from the integer sums; 1 when its denominator is 0 */
} fc_pair_score;
/* Reference labeling [n] in node order, ids in [0, n) (FC_EINVAL otherwise); NULL clears it, and
 * so does fc_load_graph. */
int fc_score_set_reference(fc_ctx* ctx, const int32_t* labels);
/* out[count] (fc_replica_info): one record per local replica on the chosen graph. */
int fc_score_partitions(fc_ctx* ctx, int graph, fc_part_score* out);
/* pairs: int32[npairs][2]; NULL = every a < b among the local replicas, then (FC_SCORE_REF, b) for
 * every b if a reference is set.  *npairs in: the pair count (pairs given) or the capacity of out
 * (pairs NULL); out: records written.  FC_EINVAL (nothing written) for an index out of range or a
 * capacity too small, FC_ESTATE without labelings or for FC_SCORE_REF with no reference.
 * fc_score_partitions and fc_score_pairs return FC_ELIMIT with more than 2048 local replicas. */
int fc_score_pairs(fc_ctx* ctx, const int32_t* pairs, int64_t* npairs, fc_pair_score* out);

/* ---- the consensus partition: components of the agreement graph ---------------------- */
/* H = the chosen graph (FC_SCORE_GRAPH_*).  support(e) = number of labelings that put both ends
 * of edge e in one community; e is kept iff !((double)support(e) < agreement * (double)n_total)
 * (float64, the tau rule's form); the consensus partition is the connected components of
 * (V, kept edges), labelled 0..k-1 by each component's smallest node id (fc_get_labels' renumber
 * convention), so the result is unique.  Read-only for everything a later call can observe; all
 * work on the context's stream (timed in consensus_ms). */
typedef struct fc_consensus_info {
    int64_t edges;            /* edges of H */
    int64_t kept_edges;
    int64_t unanimous_edges;  /* support == n_total */
    int64_t split_edges;      /* support == 0 */
    int64_t k;                /* communities of the consensus partition */
    int64_t max_size;         /* size of the largest */
    int64_t singletons;
    int32_t n_total;          /* the denominator used */
    int32_t passes;           /* launches of the hook kernel over the edge list */
    double cut;               /* agreement * n_total as compared */
} fc_consensus_info;
/* support of every edge of `graph` over the local labelings into dev_out (int32[m], caller-owned),
 * in the engine's edge order -- the order of fc_consensus_partial's output, the same on every
 * context that loaded the same graph with the same seed and options: on FC_SCORE_GRAPH_WORKING it
 * equals fc_consensus_partial(FC_ALGO_LPM).  Reduce with SUM across ranks.  FC_ELIMIT with more
 * than 2048 local replicas. */
int fc_consensus_support(fc_ctx* ctx, int graph, void* dev_out);
/* dev_support NULL: computed from the local labelings (n_total ignored, = their count).  Otherwise
 * int32[m] in that edge order, already reduced over n_total replicas (FC_EINVAL if a value lies
 * outside [0, n_total]).  Any output pointer may be NULL.  labels_out int32[n] in node order;
 * support_hist int64[n_total+1] (host); node_in[v] / node_out[v] int64[n]: the support summed over
 * v's incident edges of H whose other end is / is not in v's consensus community.  labels_out,
 * node_in and node_out may be host memory or device buffers of the context's GPU.
 * FC_EINVAL: agreement outside [0, 1] or NaN, unknown graph, dev_support with n_total < 1;
 * FC_ESTATE: no graph, or neither labelings nor dev_support; FC_ELIMIT: more than 2048 replicas.
 * Nothing is written on error. */
int fc_consensus_partition(fc_ctx* ctx, int graph, const void* dev_support, int n_total, double agreement,
                           int32_t* labels_out, int64_t* support_hist, int64_t* node_in, int64_t* node_out,
                           fc_consensus_info* info);

/* Device time (ms, HIP events) of the phases of the last fc_consensus_partition made with timing
 * enabled (fc_set_timing): ms[5] = support count, histogram, components (init + hook + flatten),
 * renumber + sizes, node sums; a phase that did not run (support given, no node sums asked) and
 * every phase without timing reads 0. */
int fc_consensus_timing(fc_ctx* ctx, double* ms);

/* ---- the consensus hierarchy: every agreement level from one union-find --------------- */
/* Level s (s = 0..n_total) is the connected components of the edges of H with support(e) >= s:
 * level 0 is the components of H, and a lower level is coarser.  With root_s(t) the smallest node
 * of t's component at level s, the levels are the tree
 *   birth[t] = the largest s with root_s(t) != t, or -1 when t is the smallest node of its
 *              component of H;   up[t] = root_{birth[t]}(t), or t when birth[t] == -1
 * (birth[up[t]] < birth[t]): root_s(t) is the end of the walk t -> up[t] -> ... while birth >= s,
 * and the labels of level s number the roots in node order, as fc_consensus_partition does at an
 * agreement whose keep rule is support >= s (agreement = (s - 0.5) / n_total, or 0 for s = 0).
 * Read-only like fc_consensus_partition; all work on the context's stream. */
typedef struct fc_level_score {
    int64_t bucket_edges; /* edges with support == s */
    int64_t k;            /* communities of level s */
    int64_t max_size;     /* size of the largest */
    int64_t singletons;
    int64_t in_weight;    /* sum of w_uv over the edges of H inside a community of level s */
    uint64_t tot_sq_lo;   /* sum_c (sum_{v in c} weighted degree_v)^2, exact, 128 bits */
    uint64_t tot_sq_hi;
    double modularity;    /* fc_part_score's formula from these integers */
} fc_level_score;
/* dev_support / n_total / graph exactly as fc_consensus_partition.  birth, up: int32[n] (host, or
 * device buffers of the context's GPU), levels: fc_level_score[n_total + 1] (host); any may be
 * NULL.  A level without an edge of its support repeats the record of the level above it, with
 * bucket_edges = 0.  *best_level: the level that maximises the exact integer
 * 2 in_weight W2 - tot_sq (modularity's numerator; W2 = total weighted degree), the highest such
 * level among equals.  Error codes as fc_consensus_partition; nothing is written on error.  The
 * tree stays in the context for fc_consensus_cut until the next fc_load_graph. */
int fc_consensus_levels(fc_ctx* ctx, int graph, const void* dev_support, int n_total, int32_t* birth, int32_t* up,
                        fc_level_score* levels, int32_t* best_level);
/* labels of level `level` of the last successful fc_consensus_levels (FC_ESTATE if there is none,
 * FC_EINVAL outside [0, n_total]): labels_out int32[n] in node order, host or device; *k_out
 * communities. */
int fc_consensus_cut(fc_ctx* ctx, int level, int32_t* labels_out, int64_t* k_out);
/* Device time (ms, HIP events) of the phases of the last fc_consensus_levels made with timing
 * enabled: ms[4] = bucket (histogram, offsets, scatter), tree (init, and a hook and a flatten per
 * nonempty level), statistics (fold of the per-level counters), join levels. */
int fc_consensus_levels_timing(fc_ctx* ctx, double* ms);

/* ---- co-association: how many local labelings put two nodes together ------------------- */
/* Node ids are the caller's node order (the columns of fc_get_labels), duplicates and any order
 * allowed; the lists are host arrays.  Every call reads labels only (graph, labelings and random
 * state are afterwards what they were), works on the context's stream and returns after it has
 * finished.  FC_ESTATE: no graph or no labelings; FC_EINVAL: a node id outside [0, n) (the message
 * names the index), checked before anything is launched; FC_ELIMIT: more than 2048 local
 * replicas.  A length of 0 is legal and launches nothing.  Reduce the counts with SUM across
 * ranks. */
/* out[i*nb + j] = #local replicas that put node a[i] and node b[j] together; b == NULL: b = a.
   a, b: host int32 node ids in [0, n); dev_out: device int32[na*nb]. */
int fc_coassociation(fc_ctx* ctx, int64_t na, const int32_t* a, int64_t nb, const int32_t* b, void* dev_out);
/* counts[p] for node pairs (pairs[2p], pairs[2p+1]); dev_out: device int32[npairs] */
int fc_coassoc_pairs(fc_ctx* ctx, int64_t npairs, const int32_t* pairs, void* dev_out);
/* hist[s], s = 0..n_r, over the unordered position pairs i < j of the list; host int64[n_r + 1]
 * (n_r: the local replica count of fc_replica_info).  No matrix is formed: k = 65536 is 2.1 G
 * pairs.  The histogram of a sharded run is not the sum of the ranks' histograms. */
int fc_coassoc_hist(fc_ctx* ctx, int64_t k, const int32_t* nodes, int64_t* hist);
/* Device time (ms, HIP events) of the phases of the last co-association call made with timing
 * enabled: ms[2] = ids (upload and map to internal vertices), count (the kernel). */
int fc_coassoc_timing(fc_ctx* ctx, double* ms);   /* phases of the last call, timing enabled only */

/* ---- cluster and item consensus of a given partition ------------------------------------ */
/* For a partition P of the nodes (a consensus cut, one of the replicas, a ground truth) and the
 * local labelings, with coassoc(i, j) = the number of local replicas that put i and j together:
 *   pairs[k] = sum over the ordered member pairs (i, j) of cluster k, i = j included, of coassoc(i, j)
 *   item[v]  = sum over the members j of v's own cluster, j = v included, of coassoc(v, j)
 * computed from the contingency tables between P and every replica, without the matrix: exact
 * integers in O(n * n_r).  Both are sums over replicas: ranks add theirs (SUM) and normalise by the
 * total replica count: (pairs - n_total size) / (n_total size (size - 1)) is Monti et al.'s cluster
 * consensus m(k), (item - n_total) / (n_total (size - 1)) the item consensus m_i(k) of a node with
 * its own cluster.  Read-only like fc_score_pairs: labelings, reference and random state stay. */
typedef struct fc_cluster_info {
    int64_t k, max_size, singletons;
    int64_t pairs_total;    /* sum_k pairs[k] == sum_v item[v] */
    int64_t slow_members;   /* (member, replica) pairs the exact fallback handled (diagnostic) */
    int32_t n_r, pad;
} fc_cluster_info;
/* labels: host int32[n] in node order, ids in [0, n), not necessarily dense; the K distinct ids are
 * reported ascending.  ids_out, size_out: host arrays of capacity n, the first K entries written.
 * dev_cluster: device int64[n], pairs of the K clusters in that order, then zeros (the same shape on
 * every rank).  dev_item: device int64[n] in node order.  Any output may be NULL.  All work on the
 * context's stream; returns after it finished.  FC_ESTATE: no graph or no labelings; FC_EINVAL:
 * labels NULL or an id outside [0, n) (the message names the index; checked before any launch);
 * FC_ELIMIT: more than 2048 local replicas.  Nothing is written on error. */
int fc_cluster_consensus(fc_ctx* ctx, const int32_t* labels, int32_t* ids_out, int64_t* size_out, void* dev_cluster,
                         void* dev_item, fc_cluster_info* info);
/* Device time (ms, HIP events) of the phases of the last fc_cluster_consensus made with timing
 * enabled: ms[3] = segments (upload, sort, run lengths), count (the register-list kernel),
 * fallback (the exact sort-based path). */
int fc_cluster_consensus_timing(fc_ctx* ctx, double* ms);

/* ---- plurality vote of the labelings on a given partition ------------------------------- */
/* Relabel-and-vote (Dudoit & Fridlyand; Strehl & Ghosh) for a partition P of the nodes (ids in
 * [0, n), not necessarily dense) and labelings lab_r.  With C_r[k][d] = the number of nodes v with
 * P(v) = k and lab_r(v) = d, all integers and all exact:
 *   map_r(d)     = the cluster k of largest C_r[k][d]; among equals the smallest id
 *   mapped[r][v] = map_r(lab_r(v))
 *   votes_v(k)   = the number of r with mapped[r][v] = k;   own[v] = votes_v(P(v))
 *   top_votes[v] = max_k votes_v(k);  top[v] = the cluster reaching it: P(v) when it is among
 *                  several that do, otherwise the smallest id
 * Nothing depends on how a replica numbers its communities.  Only `mapped` depends on which rank
 * holds a replica: a sharded run all-gathers `mapped` in global replica order and counts on every
 * rank (the ranks' `top` cannot be reduced).  Read-only like fc_cluster_consensus; the reuse
 * paragraph at the top of this header holds for these calls too. */
typedef struct fc_vote_info {
    int64_t k;                    /* clusters of P */
    int64_t k_voted;              /* distinct values of top */
    int64_t moved;                /* nodes with top != P */
    int64_t unanimous;            /* nodes with own == n_total */
    int64_t tied;                 /* nodes where more than one cluster reaches top_votes */
    int64_t mapped_communities;   /* sum over the replicas of their community counts (map calls) */
    int64_t slow_members;         /* (member, replica) pairs the map's exact fallback handled */
    int64_t slow_nodes;           /* nodes the vote's sorting fallback handled (more than 8 clusters voted) */
    int32_t n_total, pad;
} fc_vote_info;
/* labels: host int32[n], P in node order.  dev_mapped: device int32[n_r][n], replica-major, node
 * order, values are ids of P.  Fills k, mapped_communities, slow_members and n_total = n_r.
 * FC_ESTATE: no graph or no labelings; FC_ELIMIT: more than 2048 local replicas; FC_EINVAL: labels
 * or dev_mapped NULL, or an id outside [0, n) (the message names the index; checked before any
 * launch).  Nothing is written on error. */
int fc_vote_map(fc_ctx* ctx, const int32_t* labels, void* dev_mapped, fc_vote_info* info);
/* The vote over dev_mapped (device int32[n_total][n] in fc_vote_map's layout, from this rank or
 * gathered); needs a loaded graph (for n) but no labelings.  dev_top, dev_top_votes, dev_own_votes:
 * device int32[n] in node order; own_hist: host int64[n_total + 1], own_hist[s] = the nodes with
 * own == s; any of them may be NULL.  Fills every field of info but the map's three.  FC_ESTATE: no
 * graph; FC_EINVAL: labels or dev_mapped NULL, an id outside [0, n), n_total < 1, or (found on the
 * device, before any output is written) a value of dev_mapped that is not an id occurring in
 * labels; FC_ELIMIT: n_total above 2048. */
int fc_vote_count(fc_ctx* ctx, const int32_t* labels, const void* dev_mapped, int n_total, void* dev_top,
                  void* dev_top_votes, void* dev_own_votes, int64_t* own_hist, fc_vote_info* info);
/* fc_vote_map then fc_vote_count over the local labelings (n_total = n_r), through a buffer the
 * context owns. */
int fc_vote(fc_ctx* ctx, const int32_t* labels, void* dev_top, void* dev_top_votes, void* dev_own_votes,
            int64_t* own_hist, fc_vote_info* info);
/* Device time (ms, HIP events) of the phases of the last of these three calls made with timing
 * enabled: ms[4] = segments (upload, sort, run lengths), map (the register-list kernel and the
 * apply), map fallback (the exact sort-based path), count (the vote and its sorting fallback); a
 * phase the call did not run is 0. */
int fc_vote_timing(fc_ctx* ctx, double* ms);

/* ---- co-association of a node with any cluster of a given partition ---------------------- */
/* For a partition P (ids in [0, n), not necessarily dense) and the local labelings, with
 * C_r[k][d] = the number of members of cluster k that replica r labels d:
 *   aff(v, k) = sum_r C_r[k][lab_r(v)] = sum over the members j of k of coassoc(v, j)
 * v itself counted when P(v) = k, so aff(v, P(v)) is fc_cluster_consensus' item[v].  It is the
 * numerator of Monti et al.'s item consensus m_i(k) for ANY k, and what a one-element move of the
 * median-partition objective needs (DESIGN, "Median partition").  Exact integers from the
 * contingency rows, without the matrix: the cost follows the members of the queried clusters plus
 * the queries.  A sum over replicas: ranks add theirs (SUM).  Read-only like fc_cluster_consensus;
 * the reuse paragraph at the top of this header holds for this call too. */
typedef struct fc_affinity_info {
    int64_t k;                /* clusters of P */
    int64_t queried_clusters; /* distinct clusters of P named by the queries */
    int64_t slow_lookups;     /* (query, replica) pairs the exact fallback answered */
    int32_t n_r, pad;
} fc_affinity_info;
/* out[p] = aff(nodes[p], clusters[p]) over the LOCAL labelings.  labels: host int32[n], P in node
 * order.  nodes, clusters: host int32[npairs], duplicates and any order allowed, a node may appear
 * against many clusters; a cluster id in [0, n) that does not occur in labels gives 0.  dev_out:
 * device int64[npairs].  npairs = 0 launches nothing (the lists and dev_out may then be NULL).
 * FC_ESTATE: no graph or no labelings; FC_ELIMIT: more than 2048 local replicas, or npairs >= 2^31;
 * FC_EINVAL: a NULL pointer, or a node, cluster or label id outside [0, n) (the message names the
 * index; checked before any launch).  Nothing is written on error. */
int fc_item_affinity(fc_ctx* ctx, const int32_t* labels, int64_t npairs, const int32_t* nodes, const int32_t* clusters,
                     void* dev_out, fc_affinity_info* info);
/* Device time (ms, HIP events) of the phases of the last fc_item_affinity made with timing enabled:
 * ms[3] = queries (upload, segments of P, cluster ranks, sort of the queries), count (the
 * register-list kernel), fallback (the exact sort-based path). */
int fc_item_affinity_timing(fc_ctx* ctx, double* ms);

/* ---- community quality of a given partition on the graph ---------------------------------- */
/* H = the chosen graph (FC_SCORE_GRAPH_*), P a partition (ids in [0, n), not necessarily dense: a
 * consensus cut, `voted`, `median`, a replica, a ground truth).  What the GRAPH says about each
 * cluster of P, where fc_cluster_consensus says what the labelings say: internal weight, volume and
 * from them the cut (volume - 2 * in_weight, not stored), conductance, density and the cluster's
 * share of modularity; the number of connected parts of the subgraph its members induce (level-0
 * Louvain and LPA, and the one-node moves of the vote and median refinements, can leave a cluster
 * in several pieces); per node the weight it sends inside and outside its cluster.  Exact
 * integers.  The call reads no labelings: it works on a context that has only loaded a graph, and
 * it is the same on every rank (no collective).  Read-only: the reuse paragraph at the top of
 * this header holds for this call too. */
typedef struct fc_community_record {   /* one record per cluster of P, ids ascending */
    int64_t id, size;
    int64_t volume;          /* sum of the members' weighted degrees in H */
    int64_t in_weight;       /* sum of w over the edges of H with both ends in the cluster, each once */
    int64_t in_edges;        /* the number of those edges (weight-0 edges of the working graph count) */
    int64_t min_in_degree;   /* min over the members of the number of neighbours inside the cluster */
    int64_t components;      /* connected parts of the subgraph of H induced by the members */
    int64_t largest_component;
} fc_community_record;
typedef struct fc_quality_info {
    int64_t k, max_size, singletons;
    int64_t parts;           /* sum of components = clusters of the split partition */
    int64_t disconnected;    /* clusters with components > 1 */
    int64_t in_weight, cut_weight;   /* totals; every cut edge counted once */
    int64_t total_degree;    /* W2 of H */
} fc_quality_info;
/* labels: host int32[n], P in node order.  out: host, capacity n records, the first info->k are
 * written.  node_in[v] / node_out[v]: the weight of v's incident edges whose other end is / is not
 * in P(v), int64[n]; split_out: P refined to the connected parts of each cluster, int32[n], the
 * parts numbered 0..parts-1 by their smallest node id (fc_get_labels' renumber convention).  These
 * three may be host memory or device buffers of the context's GPU.  Any output may be NULL, and a
 * phase whose outputs are all NULL does not run.  FC_ESTATE: no graph; FC_EINVAL: labels NULL, an
 * unknown graph, or an id outside [0, n) (the message names the index; checked before any
 * launch).  Nothing is written on error. */
int fc_community_quality(fc_ctx* ctx, int graph, const int32_t* labels, fc_community_record* out, int64_t* node_in,
                         int64_t* node_out, int32_t* split_out, fc_quality_info* info);
/* Device time (ms, HIP events) of the phases of the last fc_community_quality made with timing
 * enabled: ms[4] = labels (upload, id ranks, sizes), rows (the CSR pass), fold (per-vertex values to
 * per-cluster sums), components (union-find, split partition, parts, records and totals). */
int fc_community_quality_timing(fc_ctx* ctx, double* ms);

/* ---- cluster merges: the community graph of a partition, co-association of cluster pairs --- */
/* The community graph (quotient graph) of a partition P (ids in [0, n), not necessarily dense) on
 * H = the chosen graph (FC_SCORE_GRAPH_*): the distinct unordered pairs of cluster ids (a < b)
 * joined by at least one edge of H, ascending by (a, b), so the result is unique; per pair
 * weight (the sum of w over the joining edges) and edges (their number; weight-0 edges of the
 * working graph count, as in fc_community_record.in_edges).  Per cluster the weights of its pairs
 * sum to volume - 2 in_weight of fc_community_quality, and all weights to its cut_weight.  These
 * are the natural candidates of a merge (DESIGN, "Cluster merges").
 * labels: host int32[n], P in node order.  a_out, b_out int32[capacity], weight_out, edges_out
 * int64[capacity]: host memory or device buffers of the context's GPU, any may be NULL.
 * *npairs_out always receives the number of pairs; with the four outputs NULL the call is the size
 * query.  The call reads no labelings: it works on a context that has only loaded a graph, and it
 * is the same on every rank (no collective).  Read-only: the reuse paragraph at the top of this
 * header holds for this call too.  FC_ESTATE: no graph; FC_EINVAL: labels or npairs_out NULL, an
 * unknown graph, an id outside [0, n) (the message names the index; checked before any launch), or
 * an output given with capacity below the count (nothing is written but the count).  Nothing else
 * is written on error. */
int fc_community_graph(fc_ctx* ctx, int graph, const int32_t* labels, int64_t capacity, void* a_out, void* b_out,
                       void* weight_out, void* edges_out, int64_t* npairs_out);
/* Device time (ms, HIP events) of the phases of the last fc_community_graph made with timing
 * enabled: ms[4] = labels (upload, id ranks), emit (the pass over the edges), sort (radix sort, run
 * lengths, prefix sums), pairs (ranks back to ids). */
int fc_community_graph_timing(fc_ctx* ctx, double* ms);

/* For a partition P and the local labelings, with C_r[k][d] = the number of members of cluster k
 * that replica r labels d:
 *   X(a, b) = sum_r sum_d C_r[a][d] * C_r[b][d] = sum over i in a, j in b of coassoc(i, j)
 * the between-cluster counterpart of fc_cluster_consensus' pairs: X(a, a) is pairs[a], and
 * X(a, b) / (R s_a s_b) the mean consensus between two clusters.  Joining a != b changes the
 * median-partition objective F by 2 (2 X(a, b) - R s_a s_b).  Exact integers from the contingency
 * rows, without the matrix: per pair the larger cluster's rows are listed once for all its
 * partners and the smaller cluster's members are walked.  A sum over replicas: ranks add theirs
 * (SUM).  Read-only like fc_cluster_consensus; the reuse paragraph at the top of this header holds
 * for this call too. */
typedef struct fc_cluster_pair_info {
    int64_t k;                /* clusters of P */
    int64_t listed_clusters;  /* distinct clusters whose (label, count) lists were built */
    int64_t walked_members;   /* members read on the walk side, summed over the pairs */
    int64_t slow_lookups;     /* (walk member, replica) pairs the exact fallback answered */
    int32_t n_r, pad;
} fc_cluster_pair_info;
/* out[p] = X(a[p], b[p]) over the LOCAL labelings.  labels: host int32[n], P in node order.  a, b:
 * host int32[npairs] cluster ids; duplicates, both orders and a[p] == b[p] are allowed; an id in
 * [0, n) that does not occur in labels gives 0.  dev_out: device int64[npairs].  npairs = 0
 * launches nothing (the lists and dev_out may then be NULL).  FC_ESTATE: no graph or no
 * labelings; FC_ELIMIT: more than 2048 local replicas, or npairs >= 2^31; FC_EINVAL: a NULL
 * pointer, or a cluster or label id outside [0, n) (the message names the index; checked before
 * any launch).  Nothing is written on error. */
int fc_cluster_coassoc(fc_ctx* ctx, const int32_t* labels, int64_t npairs, const int32_t* a, const int32_t* b,
                       void* dev_out, fc_cluster_pair_info* info);
/* Device time (ms, HIP events) of the phases of the last fc_cluster_coassoc made with timing
 * enabled: ms[3] = pairs (upload, segments of P, cluster ranks, sides, sort of the pairs), count
 * (the register-list kernel), fallback (the exact sort-based path). */
int fc_cluster_coassoc_timing(fc_ctx* ctx, double* ms);

/* ---- cluster-wise Jaccard best match of a given partition ------------------------------- */
/* For a partition P of the nodes with clusters k of size s_k, and a labeling r with t_r(d) = the
 * nodes (of all n) that r labels d and C_r[k][d] = the members of k that r labels d:
 *   J_r(k, d)   = C / (s_k + t_r(d) - C),   C = C_r[k][d] > 0          the Jaccard index
 *   best_r(k)   = the d of largest J_r(k, d); two fractions are compared exactly as C1 * U2 against
 *                 C2 * U1 with U = s_k + t - C (C <= n < 2^31, U < 2^32: 64-bit products); among
 *                 equal J the larger C (equal J and equal C force equal t)
 *   inter[r][k] = C_r[k][best_r(k)]          csize[r][k] = t_r(best_r(k))
 * Every cluster has a member, so a match exists, and the pair (inter, csize) is unique: it depends
 * neither on how r numbers its communities nor on any floating-point value.  Hennig's cluster-wise
 * stability of k is the mean over r of inter / (s_k + csize - inter); with P a planted partition
 * and one found partition as r, inter / csize, inter / s_k and 2 inter / (s_k + csize) are the
 * best-match precision, recall and F1 of each planted community.  Rows are independent: ranks
 * gather theirs in replica order.  Read-only: the reuse paragraph at the top of this header. */
typedef struct fc_match_info {
    int64_t k, max_size, singletons;
    int64_t perfect;        /* (r, k) with inter == s_k == csize, i.e. J = 1 */
    int64_t inter_total;    /* sum of inter over all (r, k) */
    int64_t slow_members;   /* (member, replica) pairs the exact fallback handled (diagnostic) */
    int32_t n_r, pad;       /* rows written: the local replica count, or 1 with `other` */
} fc_match_info;
/* labels: host int32[n], P in node order, ids in [0, n), not necessarily dense; the K distinct ids
 * are reported ascending.  other: NULL for the local labelings (n_r rows), or one host labeling
 * int32[n] with ids in [0, n), matched as a single row: that form needs a loaded graph but no
 * labelings and leaves the labelings untouched.  ids_out, size_out: host arrays of capacity n, the
 * first K entries written.  dev_inter, dev_csize: device int32, row r at offset r * ld, the first K
 * entries of each row written and the rest left alone.  ld < K with either buffer given is
 * FC_EINVAL, and then only info->k is written (the caller sizes its buffers from it); with both
 * buffers NULL ld is ignored and ids, sizes and info are reported.  Any output may be NULL.  All
 * work on the context's stream; returns after it finished.  FC_ESTATE: no graph, or other == NULL
 * with no labelings; FC_ELIMIT: more than 2048 local replicas; FC_EINVAL: labels NULL, or an id of
 * labels or other outside [0, n) (the message names the array and the index; checked before any
 * launch).  Apart from info->k in the ld case nothing is written on error. */
int fc_cluster_match(fc_ctx* ctx, const int32_t* labels, const int32_t* other, int64_t ld,
                     int32_t* ids_out, int64_t* size_out, void* dev_inter, void* dev_csize, fc_match_info* info);
/* Device time (ms, HIP events) of the phases of the last fc_cluster_match made with timing
 * enabled: ms[4] = segments (upload, sort, run lengths), sizes (the community-size table), match
 * (the register-list kernel), fallback (the exact sort-based path). */
int fc_cluster_match_timing(fc_ctx* ctx, double* ms);   /* ms[4] = segments, sizes, match, fallback */

/* ---- synthetic inputs for benchmarks (host C++, not on the hot path) ---------------- */
/* LFR-like benchmark graph (power-law degrees tau1, community sizes tau2, mixing mu).
 * Writes at most m_cap edges into u/v and the planted community of every node. */
int fc_generate_lfr(int64_t n, double tau1, double tau2, double mu, double avg_deg,
                    int32_t max_deg, int32_t min_comm, int32_t max_comm, uint64_t seed,
                    int64_t m_cap, int32_t* u, int32_t* v, int64_t* m_out, int32_t* planted);
/* Planted-partition SBM: n/block_size blocks, expected internal/external degree. */
int fc_generate_sbm(int64_t n, int32_t block_size, double deg_in, double deg_out,
                    uint64_t seed, int64_t m_cap, int32_t* u, int32_t* v, int64_t* m_out);
/* Edge-list text parser (2+ whitespace-separated int columns; extra columns ignored).
 * Returns labels in node order (first appearance) and edges as ids. Two-phase: call with
 * NULL outputs to get sizes. */
int fc_read_edgelist(const char* path, int64_t* n_out, int64_t* m_out, int64_t* labels,
                     int32_t* u, int32_t* v);

#ifdef __cplusplus
}
#endif
#endif /* FASTCONSENSUS_AMD_H */
