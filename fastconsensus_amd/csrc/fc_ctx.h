// fc_ctx.h -- engine context: device-resident graph, replica state and scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include <chrono>
#include <string>
#include <utility>
#include <vector>

#include "../../include/fastconsensus_amd.h"

namespace fc {

// FC_TRACE: microseconds since the previous trace mark -- one clock shared by every engine
// (cd.hip, cd_rl.hip, leiden.hip), so a line's dt is the work since the line before it;
// reset = true marks a batch start (returns 0)
inline double trace_dt_us(bool reset = false) {
    static std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    const auto now = std::chrono::steady_clock::now();
    const double dt = 1e-3 * (double)std::chrono::duration_cast<std::chrono::nanoseconds>(now - last).count();
    last = now;
    return reset ? 0.0 : dt;
}

void set_error(const std::string& msg);

// Louvain community detection + louvain consensus loop (closure counts, isolate repair,
// check #1): FC_ALGO_LOUVAIN and its new_consensus.py weight-rule variant.
inline bool is_louvain(int algo) { return algo == FC_ALGO_LOUVAIN || algo == FC_ALGO_LOUVAIN_NC; }

struct FcError {
    int code;
    std::string msg;
};

#define FC_HIP(call)                                                                       \
    do {                                                                                   \
        hipError_t _e = (call);                                                            \
        if (_e != hipSuccess) {                                                            \
            (void)hipGetLastError(); /* clear it: library calls (hipcub) re-check it later */ \
            throw ::fc::FcError{FC_EHIP, std::string(#call) + ": " + hipGetErrorString(_e)}; \
        }                                                                                  \
    } while (0)
#define FC_REQUIRE(cond, code, msg)                      \
    do {                                                 \
        if (!(cond)) throw ::fc::FcError{(code), (msg)}; \
    } while (0)

// Environment tunables, read when an engine is created: atoi / atoll of the value (a variable set
// to the empty string gives 0), the default when it is unset; env_flag: set, not empty, not "0..."
inline int env_int(const char* name, int dflt) { const char* s = getenv(name); return s ? atoi(s) : dflt; }
inline int64_t env_i64(const char* name, int64_t dflt) { const char* s = getenv(name); return s ? atoll(s) : dflt; }
inline bool env_flag(const char* name) { const char* s = getenv(name); return s && *s && *s != '0'; }

struct NoCopy {   // what owns a device or runtime resource frees it in its destructor and is never copied
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};

// Growable device buffer (never shrinks; grows by 1.5x), freed with its owner; move-only.
struct DevBuf : NoCopy {
    void* p = nullptr;
    size_t bytes = 0;
    inline static std::atomic<int64_t> held{0};   // bytes of all live buffers (fc_device_bytes): touched when one grows or dies
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }   // both by swap: o leaves with the old block and frees it
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
    ~DevBuf() { release(); }
    template <class T> T* as() const { return static_cast<T*>(p); }
    void ensure(size_t need) {
        if (need <= bytes) return;
        size_t nb = bytes ? bytes + bytes / 2 : 0;
        if (nb < need) nb = need;
        nb = (nb + 255) & ~size_t(255);
        if (p) FC_HIP(hipDeviceSynchronize());  // queued kernels may still use the old buffer
        release();   // p and bytes together: a failed hipMalloc leaves an empty buffer, not a null pointer of the old size
        FC_HIP(hipMalloc(&p, nb));
        bytes = nb;
        held += (int64_t)nb;
    }
    void release() {
        if (p) (void)hipFree(p);
        held -= (int64_t)bytes;
        p = nullptr;
        bytes = 0;
    }
};

// An engine's other raw resources, owned the same way (created by fc_create and timer_begin).
struct OwnStream : NoCopy {
    hipStream_t s = nullptr;
    ~OwnStream() { if (s) (void)hipStreamDestroy(s); }
};
struct PinnedI64 : NoCopy {
    int64_t* p = nullptr;
    operator int64_t*() const { return p; }
    ~PinnedI64() { if (p) (void)hipHostFree(p); }
};
// timed spans (fc_stats *_ms and *_launches, timer_collect)
enum TimerSlot { TS_CD, TS_CONSENSUS, TS_CLOSURE, TS_REBUILD, TS_DECIDE, TS_LV_DECIDE, TS_LV_HEAVY, TS_RL_DECIDE, TS_COUNT };
struct Timer : NoCopy {
    bool on = false;
    std::vector<hipEvent_t> pool;
    std::vector<std::pair<int, int>> spans[TS_COUNT];
    size_t next = 0;
    ~Timer() { for (auto e : pool) (void)hipEventDestroy(e); }
};

// Canonical edge list (u < v in node order, sorted by (u,v)) + symmetric CSR with
// every row sorted ascending.
struct Graph {
    int64_t m = 0;
    DevBuf eu, ev, ew, eage;        // int32, int32, int32, int64  [m]
    DevBuf rowptr, col, cw, ceid;   // int64 [N+1], int32 [2m] x3
    DevBuf crev;                    // int32 [2m]: index of the reverse entry (v->u for u->v)
    DevBuf colp;                    // int32 [2m]: storage slot (Ctx::spos) of col[j]: label gathers
    DevBuf vrec;                    // int4 [N]: row start (m < 2^31), degree, k_v (valid when 2M < 2^31), slot
    DevBuf kdeg;                    // int64 [N] weighted degree
    int64_t M2 = 0;                 // sum of kdeg = 2 * total weight
    int32_t max_deg = 0;
    int64_t max_kdeg = 0;
    int32_t max_w = 0;              // largest edge weight (unit-weight graphs skip the weight loads)
};

// timed phases of one analysis call (Ctx::cp_ms / lv_ms / ca_ms / cc_ms, written by analysis.h's PhaseMarks; vt_ms by vote.h's VoteMarks; ia_ms by affinity.h; mg_ms / mc_ms by merge.h; cm_ms by match.h)
constexpr int CP_PHASES = 5, LV_PHASES = 4, CA_PHASES = 2, CC_PHASES = 3, VT_PHASES = 4, IA_PHASES = 3, QL_PHASES = 4, MG_PHASES = 4, MC_PHASES = 3, CM_PHASES = 4;

// Every resource goes with the member that holds it (fc_destroy synchronises, then deletes).
struct Ctx : NoCopy {
    int device = 0;
    uint64_t seed = 0;
    OwnStream own_stream;
    hipStream_t stream = nullptr;   // own_stream.s, or the caller's (fc_set_stream)
    int64_t N = 0, m_original = 0;
    // internal vertex numbering: internal = sigma[node], node = npos[internal] (a seeded
    // random permutation, or the identity): engine behaviour is independent of input order
    DevBuf sigma, npos;             // int32 [N]
    // label storage maps (int32 [N], slot_maps()): sinv slot -> internal vertex, tpos node
    // position -> slot, snpos slot -> node position; label-row passes walk rows in slot order
    DevBuf sinv, tpos, snpos;
    std::vector<int32_t> h_sigma;
    DevBuf st_u, st_v, st_w, st_age, st_lab;   // host-facing staging (node space)
    int key_bits = 1;               // bits to hold a node id (N <= 2^key_bits)
    Graph g;                        // `graph` (fast_consensus.py:131)
    Graph g0;                       // pristine G as loaded (never modified, like the caller's G)
    // replica state (replica-major [n_r][N])
    int n_r = 0, rbase = 0, n_p_total = 0;
    DevBuf lab, tot, dec, labT;     // int32 [n_r][N], int64 [n_r][N], int32 [n_r][S], int32 [N][ldT]
    DevBuf nlab;                    // int32 [n_r][2m]: label of each adjacency entry's neighbour
    DevBuf aff, vlist, vcnt, track; // pruning: affected flags, per-sweep visit lists, list lengths, modes
    DevBuf mvf;                     // movers of a tracked sweep (prune_mark = 1 on weighted Louvain graphs)
    DevBuf aff_cnt;                 // hybrid: per-replica affected-flag counts at a sweep's start
    // replica-lane engine (cd_rl.hip): per-entry replica masks, list-build scratch, affected /
    // mover bits [banks][N]; labels and totals node-major in labT / tot ([N][ldT])
    DevBuf rl_lmask, rl_vmask, rl_aff, rl_mvf, rl_vlist, rl_vcount;
    // visit mode for sparse sweeps: when visits * rl_visit_div < entries * min(n_r, 64) (0: never)
    int rl_visit_div = env_int("FC_RL_VISIT_DIV", 4);
    // hybrid hand-off into push mode: 0 never, 1 LPA batches (default), 2 every unit-weight batch
    int rl_handoff_push = env_int("FC_RL_HANDOFF_PUSH", 1);
    int cd_engine = 2;              // FC_OPT_CD_ENGINE: 0 classic (cd.hip), 1 replica-lane (cd_rl.hip), 2 hybrid (default)
    // hybrid: the replica-lane engine runs a batch's full sweeps only when it holds this many
    // replicas (8 lanes per vertex at 8: LFR-1M n_p = 8 run 40.3 vs 42.9 ms on cd.hip since the
    // 16-bucket / resident-grid changes; 51.3 vs 46.2 before them)
    int64_t rl_min_replicas = env_i64("FC_RL_MIN_REPLICAS", 8);
    // ... and the graph this many vertices (a bucket of a smaller graph is too few waves for the
    // replica-lane kernels: LFR-100k louvain 45.9 vs 31.2 ms, LFR-1M 175.8 vs 211 ms; at the
    // round-4 end LFR-100k louvain 33.0 vs 26.5, lpm 24.2 vs 16.6 ms)
    int64_t rl_min_vertices = env_i64("FC_RL_MIN_VERTICES", 262144);
    // hybrid semantics: a filtered sweep visiting >= N/dense_div vertices keeps the shared order
    // (without coarse rounds); 0 = never (FC_OPT_DENSE_DIV).  Measured no gain: LFR-1M 175.9 /
    // 177.7 / 176.7 ms at 0 / 2 / 4, SBM-4M 712 / 759 / 722 ms (profiles/r04_dense_ab.txt)
    int dense_div = 0;
    DevBuf rl_tot, rl_state;        // replica-lane totals [N][ldT] and per-replica state (kept apart from cd.hip's)
    DevBuf rl_colw;                 // replica-lane: (col << wbits) | weight per adjacency entry (weights < 256)
    DevBuf rl_slow, rl_slow_cnt;    // replica-lane: one bucket's visits left to the exact kernel
    int ldT = 0;
    bool labT_valid = false;
    DevBuf rep_state;               // per replica: active flag, dq accum, moves, unstable
    DevBuf heavy_list, heavy_cnt, heavy_scratch;
    // consensus / kept graph
    DevBuf wnew, flag, pos;         // int32 [m] (flag/pos also reused for 2m CSR compaction)
    int64_t kept_m = 0;
    DevBuf ku, kv, kw, kage;        // kept canonical list
    DevBuf krowptr, kcol;           // kept CSR (sorted rows)
    DevBuf counters;                // int64 scratch counters
    // closure / repair / merge
    int64_t n_cand = 0;
    DevBuf ckey, cval, ckey2;       // uint64 keys + int64 sample index
    DevBuf cu, cv, cw2, cage;       // closure edges
    DevBuf deg_next, iso, isoflag, target, tw, active, hit;
    int64_t n_iso = 0;
    DevBuf mkey, mkey2, midx, midx2;  // merge sort
    // closure over closure_rounds blocks of attempts (closure_sample): candidate table (uint64
    // key, u64 first attempt), listed slots and their count, accumulated candidates (key,
    // first attempt), the C graph of the earlier blocks' closure edges (CSR rowptr int64
    // [N+1] / col int32, ping-pong), a block's new entries (int32 row offsets + cursors, cols)
    DevBuf clo_rec;                 // closure: per node {kept row start, length, C row start, length}
    // closure sampler reads the packed node records (0: krowptr / crowptr, the path of graphs past
    // 2^31 entries; FC_CLO_PACK=0 lets the tests run it at small sizes)
    int clo_pack = env_int("FC_CLO_PACK", 1);
    DevBuf clo_hkey, clo_list, clo_cnt, clo_akey, clo_aval, clo_rowptr, clo_col, clo_rowptr2, clo_col2,
        clo_nrow, clo_ncol, clo_own, clo_own2;
    int closure_rounds = 0;         // FC_OPT_CLOSURE_ROUNDS; 0 = per algorithm (closure_blocks below)
    int clo_algo = 0;               // algorithm of the last consensus_apply (the kept graph the closure samples)
    // sharded closure (fc_closure_begin / _block_sample / _block_add / _finish): the run's
    // attempts and block count, the next block to add (blocks go in order), -1 = not begun
    int64_t clo_attempts = 0;
    int clo_R = 0, clo_next = -1, clo_iter = 0;
    int prune_mark = 1;             // FC_OPT_PRUNE_MARK: 1 Leiden-style marks on consensus graphs, 2 on every graph, 0 every neighbour
    DevBuf sort_tmp;                // hipcub temporary storage
    DevBuf nodetmp, nodetmp2, nodetmp3;  // int64 [N+1] scratch
    DevBuf part, ccount;            // consensus partial / closure counts (single-GPU driver)
    // params
    int buckets = 0, max_sweeps = 200, max_iters = 1000;   // buckets 0: cd_buckets' default per algorithm
    int chunk = 16;                 // CD order granularity (0 = per vertex), FC_OPT_CHUNK
    int relabel = 1;                // FC_OPT_RELABEL (applies at the next fc_load_graph)
    int64_t apply_blocks = env_i64("FC_APPLY_BLOCKS", 32);   // per replica
    DevBuf tailbuf, tailmark;       // CD tail kernel: worklists [n_r][3N], epoch marks [n_r][N]
    // per replica; 0 = off; -1 (default) = per algorithm: 1024 for Louvain (n_p = 8 share 45.5 ->
    // 44.4 ms against 4096), 4096 for LPA (C3 lpm 24.1 -> 22.2 ms against 1024; profiles/r05_tail_ab.txt)
    int64_t tail_visits = env_i64("FC_TAIL_VISITS", -1);
    bool order_pass = false;        // store_order()'s CD run (int64 totals, see there)
    int store_order = 1;            // FC_OPT_STORE: label rows in community order (slot spos[v])
    int order_sweeps = env_int("FC_ORDER_SWEEPS", 3);   // sweeps of that pass (4 until round 6: LFR-1M load -0.37 ms at 3, same run time)
    // its buckets per sweep: the pass only permutes label storage (results are identical), and
    // 4 big launches per sweep beat 32 small ones (LFR-1M load 9.9 -> 8.0 ms, tools/r03_ordb.sh)
    int order_buckets = env_int("FC_ORDER_BUCKETS", 4);
    DevBuf spos;                    // int32 [N]: storage slot of internal vertex v in every lab row
    int coarsen = 8;                // FC_OPT_COARSEN: 0 off, else the largest g (filtered sweeps in rounds of g buckets)
    double cd_min_dq = 1e-7;        // Louvain sweeps stop below this predicted gain (Leiden's move phase: 0)
    DevBuf lv[64];                  // Leiden level state (leiden.hip)
    int infomap_trials = 10;        // FC_OPT_INFOMAP_TRIALS (igraph community_infomap default)
    int lv_dense_div = env_int("FC_LV_DENSE_DIV", 0);   // leiden.hip level buckets
    // leiden.hip aggregate levels: buckets per move sweep (0: B, the level-0 count)
    int lv_level_b = env_int("FC_LV_LEVEL_B", 4);
    bool info_lists = env_int("FC_INFO_LISTS", 1) != 0;   // Infomap passes: compacted bucket lists (0: every bucket launch scans the union)
    bool lv_g2 = env_int("FC_LV_G2", 1) != 0;   // rows of 65..128 entries: two vertices per wave (256 slots each), not one per wave
    // cd_rl.hip Louvain decide grid: resident waves x rl_grid_mul (0: up to 8192 blocks, as LPA)
    int rl_grid_mul = env_int("FC_RL_GRID_MUL", 1);
    int prune = 1;                  // FC_OPT_PRUNE: visit only vertices whose neighbour moved (once moves < N/4)
    // CD kernel variant that leaves every decision unchanged (A/B switch, default on):
    // own-label entries summed in registers (ballots / wave scan) instead of the LDS table
    int own_ballot = env_int("FC_OWN_BALLOT", 1);
    // sweep-mode thresholds (experiment switches): tracking/pruning after a sweep moving
    // < N/track_div vertices, pull -> push after < N/push_div (0: stay in pull mode)
    int track_div = env_int("FC_TRACK_DIV", 4);
    int push_div = env_int("FC_PUSH_DIV", 4);
    bool trace = env_flag("FC_TRACE");   // per-sweep stderr
    Timer timer;
    fc_stats acc{};                 // accumulated during a run (fc_run)
    fc_stats prof{};                // accumulated since the last fc_collect_timing
    PinnedI64 hpin;                 // pinned host scratch (FC_HPIN_I64 int64)
    // cd_rl.hip decide with one unit per wave (64 local replicas or more): the row as one
    // coalesced load an item ahead, neighbour ids by readlane (A/B switch; same decisions)
    int rl_u1 = env_int("FC_RL_U1", 1);
    // timed decide launches of one bucket share their boundary events (FC_TIMER_CHAIN=0: two each)
    int timer_chain = env_int("FC_TIMER_CHAIN", 1);
    // replica-lane decide launches per bucket: 3 (networks of 16 / 32 / 64 keys), 4 (+48) or 5
    // (+24 and 48) -- per algorithm (cd_rl.hip, degree classes); 2: one launch for the rows of
    // <= 32 and one for 33..64, each kernel picking the narrower network in the launch: the
    // one-unit-per-wave kernels per row, the per-lane ones by the wave's longest row (FC_RL_SPLIT
    // bits 8 and 16, both set by default; a build without them runs 3 for the per-lane layouts)
    int rl_groups_louv = env_int("FC_RL_GROUPS_LOUV", 2);
    int rl_groups_lpa = env_int("FC_RL_GROUPS_LPA", 2);
    // partition scoring (score.h): the reference labeling in slot order, one row's sort / segment
    // buffers (reused row after row), per-block partials, fallback masks, offsets and key chunks
    DevBuf sc_ref, sc_key, sc_val, sc_ulab, sc_cnt, sc_nruns, sc_seg, sc_kd, sc_kp, sc_part, sc_part2, sc_res, sc_want,
        sc_ovf, sc_e1, sc_e2, sc_fk1, sc_fk2, sc_fcnt, sc_rng;
    bool sc_ref_set = false;
    // consensus partition (components.h): support, union-find parents, root flags and their ranks,
    // labels by node and by internal vertex, community sizes, support histogram, per-node sums
    // device time of the last call's phases (timing enabled): support, histogram, components,
    // renumber + sizes, node sums
    double cp_ms[CP_PHASES] = {};
    DevBuf cp_sup, cp_parent, cp_flag, cp_rank, cp_lab, cp_labi, cp_size, cp_hist, cp_nin, cp_nout;
    // consensus hierarchy (levels.h): the tree of the last successful fc_consensus_levels (birth, up
    // by node; lv_valid until the next fc_load_graph) and its scratch: slice cursors, edge ids by
    // support, degree sums by root, sharded per-level counters and their fold, join-level weights
    // device time of the last call's phases (timing enabled): bucket, tree, statistics, join levels
    double lv_ms[LV_PHASES] = {};
    DevBuf lv_birth, lv_up, lv_cursor, lv_bucket, lv_tot, lv_stats, lv_fold, lv_jw;
    bool lv_valid = false;
    int lv_nt = 0;
    // co-association (coassoc.h): the caller's node ids as uploaded, the two lists as internal
    // vertices, the count histogram
    // device time of the last call's phases (timing enabled): ids (upload + map), count
    double ca_ms[CA_PHASES] = {};
    DevBuf ca_ids, ca_va, ca_vb, ca_hist;
    // cluster and item consensus (cluster.h): the caller's partition in slot order (a buffer of its
    // own: sc_ref stays the scorer's), pair sums by cluster, item sums by internal vertex, their
    // total, the fallback's vertex values before and after the sort, the scan of its run lengths
    // device time of the last call's phases (timing enabled): segments, count, fallback
    double cc_ms[CC_PHASES] = {};
    DevBuf cc_row, cc_pairs, cc_item, cc_tot, cc_fv1, cc_fv2, cc_fscan;
    // plurality vote (vote.h): best (count, cluster) per label of one bank of 64 replicas, fc_vote's
    // mapped [n_r][N], the results by node before they are handed out (top, its votes, own votes),
    // id flags of P and of top, the nodes left to the sorting kernel, the own-vote histogram, counters
    // device time of the last call's phases (timing enabled): segments, map, map fallback, count
    double vt_ms[VT_PHASES] = {};
    DevBuf vt_best, vt_mapped, vt_top, vt_tv, vt_own, vt_flag, vt_slow, vt_hist, vt_ctr;
    // item affinity (affinity.h): the query lists as uploaded (nodes, then cluster ids), the nodes as
    // internal vertices, cluster ranks and query indices (by query, then sorted by rank), the queried
    // clusters with their query counts and offsets, counters, the sums before they are handed out
    // device time of the last call's phases (timing enabled): queries, count, fallback
    double ia_ms[IA_PHASES] = {};
    DevBuf ia_ids, ia_qv, ia_key, ia_idx, ia_qc, ia_qcnt, ia_qoff, ia_ctr, ia_out;
    // community quality (quality.h): presence flags of P's ids, their ranks, the ids by rank, dense
    // cluster ranks by node and by internal vertex, cluster sizes, per-node sums before they are
    // handed out, the three per-vertex values, the per-cluster accumulators, the split partition,
    // its part sizes, the records (the union-find runs in cp_parent / cp_flag / cp_rank)
    // device time of the last call's phases (timing enabled): labels, rows, fold, components
    double ql_ms[QL_PHASES] = {};
    DevBuf ql_present, ql_rank, ql_ids, ql_lab, ql_labi, ql_size, ql_nin, ql_nout, ql_vin, ql_vout, ql_vcnt, ql_acc,
        ql_split, ql_psize, ql_rec;
    // cluster merges (merge.h).  Community graph: the cut edges' keys and weights (unsorted, then
    // sorted), run lengths and their scan, the pairs before they are handed out (a | b, weight |
    // edges), counters (it takes its cluster ranks in ql_present / ql_rank / ql_ids / ql_labi)
    // device time of the last call's phases (timing enabled): labels, emit, sort, pairs
    double mg_ms[MG_PHASES] = {};
    DevBuf mg_key, mg_w, mg_cnt, mg_ab, mg_we, mg_ctr;
    // pair co-association: the pair lists as uploaded (a, then b), cluster ranks (of a, of b, of the
    // walk side), list-side ranks and pair indices (by pair, then sorted by rank), the listed
    // clusters with their partner counts and offsets, counters, the sums before they are handed
    // out, the fallback's lookup threads per pair and their scan
    // device time of the last call's phases (timing enabled): pairs, count, fallback
    double mc_ms[MC_PHASES] = {};
    DevBuf mc_ids, mc_rank, mc_key, mc_idx, mc_qc, mc_qcnt, mc_ctr, mc_out, mc_work;
    // cluster match (match.h): `other` as a one-column labT, the community sizes of every replica
    // ([N][ldT] by label), the two tables when the caller gives none, the fallback's best cell per
    // (entry, lane), the two totals (P's slot-order row and the emit's vertex values: cc_row, cc_fv1)
    // device time of the last call's phases (timing enabled): segments, sizes, match, fallback
    double cm_ms[CM_PHASES] = {};
    DevBuf cm_col, cm_csz, cm_inter, cm_csize, cm_best, cm_tot;
    // FC_SCORE_SLOW=1: every (community, replica) through the exact fallback (debug switch; same integers)
    int score_slow = env_int("FC_SCORE_SLOW", 0);
    // longest community one wave streams; longer ones go to the fallback
    int score_lcap = env_int("FC_SCORE_LCAP", 16384);
    // fallback keys per chunk (at least 2 N: an item is up to N keys); 28 bytes of scratch per key
    int64_t score_chunk = env_i64("FC_SCORE_CHUNK", (int64_t)1 << 22);
};

constexpr int FC_HPIN_I64 = 2048;   // pinned host scratch: per-sweep records (cd_rl.hip: boff | voff | n_active)
// State the replica-lane engine hands to cd_run at the first filtered sweep of a hybrid batch
// (FC_OPT_CD_ENGINE=2, cd_rl.hip): fill() writes it in cd.hip's layout on c.stream -- labels
// [n_r][N] in slot order, int32 totals [n_r][N], affected flags as bit words uint32
// [n_r][aw] (aw = (N+31)/32 words per replica; vertex v is bit v & 31 of word v >> 5), track int32
// [4][n_r] (tracked, filtered, push, transition) and active [n_r] -- and the sweeps go on from
// sweep0.  On unit-weight graphs without Leiden-style marks it also writes every neighbour-label
// row nlab [n_r][2m] and starts the replicas in push mode (cd.hip streams the rows instead of
// gathering labels).
struct CDHandoff {
    int sweep0;
    void (*fill)(Ctx& c, const void* user, int32_t* lab, int32_t* tot, uint32_t* aff, int32_t* track, int32_t* active,
                 int32_t* nlab);
    const void* user;
};

// CD buckets per sweep: FC_OPT_BUCKETS when set, else 16 for Louvain (louvain, louvain_nc and
// Leiden's level-0 move phase) and 32 for LPA.  16 buckets (twice the simultaneous deciders)
// cut LFR-1M louvain from 149 to 121 ms with the CPU model's consensus NMI within the reference
// loop's spread (0.912 vs 0.917, reference 0.905 +- 0.035); LPA keeps 32: at its detectability
// edge its bucketed batches must stay within 0.25 of sequential LPA's structured fraction
// (tests/test_gpu_cd_parity.py), and 16 buckets measured 0.28 off (profiles/r04_buckets_ab.txt)
constexpr int CD_BUCKETS_LOUVAIN = 16, CD_BUCKETS_LPA = 32;
// Closure blocks per algorithm (DESIGN, "Triadic closure"): the reference's sampler sees every
// earlier attempt's edge; a block sees only the earlier blocks'.  Louvain's closure edges carry
// co-membership weights and 4 blocks keep its consensus at or above the reference loop's
// (C2 / C3 gates); lpm's (and infomap's) weight-0 closure edges are topology for the next LPA,
// and 4 blocks (+1.7 % candidates vs sequential on the sparse C3 graph) cost 0.0008 consensus
// NMI there -- 16 blocks (+0.5 %) match the reference loop (tools/lpm_ablate.py).
constexpr int CLOSURE_ROUNDS_LOUVAIN = 4, CLOSURE_ROUNDS_LPM = 16;
inline int closure_blocks(const Ctx& c) {
    return c.closure_rounds > 0 ? c.closure_rounds
                                : (is_louvain(c.clo_algo) ? CLOSURE_ROUNDS_LOUVAIN : CLOSURE_ROUNDS_LPM);
}
inline int cd_buckets(const Ctx& c, int algo) {
    return c.buckets > 0 ? c.buckets : (is_louvain(algo) ? CD_BUCKETS_LOUVAIN : CD_BUCKETS_LPA);
}
// What cd.hip and cd_rl.hip must agree on: a hybrid batch starts on one and ends on the other
// (CDHandoff), and the CPU twin reproduces both.
// Per-replica sweep counters: NSH shards of RF u64 fields -- 0 dq, 1 unstable, 2 moves, 3 visits,
// 4 entries, 5 cands, 6 units (cd_rl.hip only); the predicted dQ in 2^40 fixed point
constexpr int NSH = 16;
constexpr int RF = 8;
constexpr double DQ_SCALE = 1099511627776.0;
// Sweep positions: the vertices in a random order, or (chunk > 0) whole chunks of `chunk`
// consecutive vertices in a random chunk order (coalesced per-vertex accesses).  NC positions
// are permuted (chunks: with room for the chunk-grid shift), B buckets of S vertices each cover
// the PN vertex positions.
struct SweepGeom {
    int CH, B;
    int64_t NC, S, PN;
    SweepGeom(const Ctx& c, int algo) : CH(c.chunk) {
        NC = CH ? (c.N + 2 * CH - 2) / CH : c.N;
        B = (int)(cd_buckets(c, algo) < NC ? cd_buckets(c, algo) : NC);
        S = CH ? ((NC + B - 1) / B) * CH : (c.N + B - 1) / B;
        PN = CH ? NC * CH : c.N;
    }
};
// Leiden-style marks (a tracked sweep flags the neighbours that ended in another community than
// the mover, not every neighbour): on consensus graphs, or on every graph with prune_mark = 2
inline bool cd_leiden_marks(const Ctx& c) {
    return (c.g.max_w > 1 || c.prune_mark == 2) && c.prune && c.prune_mark >= 1;
}
// Every weight of g is 1: the one test behind every kernel variant that skips the weight loads.
// max_w == 1 alone is not enough: a working graph may hold weight-0 edges beside its 1s (an lpm or
// infomap step with n_p = 1 keeps agreed edges at 1 and adds closure edges at 0), and each of those
// lowers M2 below 2 m.
inline bool unit_weights(const Graph& g) { return g.max_w == 1 && g.M2 == 2 * g.m; }
// every edge weighs 1 to the decide kernels: LPA ignores the weights, Louvain needs every weight 1
inline bool cd_unit_weights(const Ctx& c, bool louv) { return !louv || unit_weights(c.g); }

// graph.cpp
void graph_load(Ctx& c, int64_t n, int64_t m, const int32_t* u, const int32_t* v);
void graph_build_csr(Ctx& c, Graph& g);
void graph_merge_next(Ctx& c, int64_t n_added);
void graph_copy(Ctx& c, Graph& dst, const Graph& src);
// cd.cpp
// shared_full: full sweeps in the batch's shared order (the hybrid's semantics); h: resume a
// hybrid batch handed over by the replica-lane engine
void cd_run(Ctx& c, int algo, int rbegin, int rcount, int n_p_total, int iteration, int shared_full = 0,
            const CDHandoff* h = nullptr);
// cd_rl.hip: the replica-lane engine (louvain / lpm batches when cd_rl_supported)
bool cd_rl_supported(const Ctx& c, int algo);
void cd_run_rl(Ctx& c, int algo, int rbegin, int rcount, int n_p_total, int iteration, bool hybrid = false);
// FC_OPT_CD_ENGINE=2: full sweeps in one shared order (on the replica-lane engine when the batch
// holds >= rl_min_replicas and the graph fits it), filtered sweeps on cd.hip in per-replica orders
void cd_run_hybrid(Ctx& c, int algo, int rbegin, int rcount, int n_p_total, int iteration);
void store_order(Ctx& c);             // Ctx::spos from a one-replica Louvain run (FC_OPT_STORE)
void slot_maps(Ctx& c);               // Ctx::sinv / tpos / snpos from spos
void graph_slots(Ctx& c, Graph& g);   // g.colp = spos[g.col]
void labels_transpose(Ctx& c);
void labels_to_host(Ctx& c, int32_t* out, bool renumber);   // node order [n_r][N]
void labels_from_host(Ctx& c, int count, const int32_t* in);
void graph_to_host(Ctx& c, int64_t m, const int32_t* u, const int32_t* v, const int32_t* w, const int64_t* age,
                   int32_t* ou, int32_t* ov, int32_t* ow, int64_t* oage);
// leiden.hip: replica-batched Leiden (leidenalg ModularityVertexPartition, n_iterations=1)
void leiden_run(Ctx& c, int rbegin, int rcount, int n_p_total, int iteration);
// igraph Infomap core (two-level map equation, best of `trials`), same layout
void infomap_run(Ctx& c, int rbegin, int rcount, int n_p_total, int iteration);
// consensus.cpp
void consensus_partial(Ctx& c, int algo, int32_t* out);
void consensus_apply(Ctx& c, int algo, int n_p, double tau, const int32_t* partial, int64_t* kept,
                     int64_t* unconv);
void closure_sample(Ctx& c, int64_t attempts, int iteration);
int closure_begin(Ctx& c, int64_t attempts, int iteration);
int64_t closure_block_sample(Ctx& c, int block, int64_t t_lo, int64_t t_hi, int64_t* out, int64_t capacity);
void closure_block_add(Ctx& c, int block, const int64_t* in, int64_t count);
int64_t closure_finish(Ctx& c);
void closure_from_pairs(Ctx& c, int64_t npairs, const int32_t* pairs, int iteration);
void closure_partial(Ctx& c, int32_t* out);
void closure_apply(Ctx& c, int algo, int n_p, const int32_t* counts, int iteration);
int64_t count_unconverged(Ctx& c, const int32_t* w, int64_t m, int n_p);
// score.h (in consensus.hip): labels in node order or null; out[n_r]; pairs validated by the caller
void score_set_reference(Ctx& c, const int32_t* labels);
void score_partitions(Ctx& c, int graph, fc_part_score* out);
void score_pairs(Ctx& c, const int32_t* pairs, int64_t npairs, fc_pair_score* out);
// The analysis headers, included at the end of consensus.hip.  analysis.h holds what they share:
// support_bin, wave_bin_add / wave_bin_rank and PhaseMarks; the union-find (cp_find, uf_hook) and the
// opening of the partition and the hierarchy (cp_open) are components.h's, and levels.h uses them.
// components.h: arguments validated by the caller
void consensus_support(Ctx& c, int graph, int32_t* dev_out);
void consensus_partition(Ctx& c, int graph, const int32_t* dev_support, int n_total, double agreement,
                         int32_t* labels_out, int64_t* hist_out, int64_t* nin_out, int64_t* nout_out,
                         fc_consensus_info* info);
// levels.h: arguments validated by the caller
void consensus_levels(Ctx& c, int graph, const int32_t* dev_support, int n_total, int32_t* birth_out, int32_t* up_out,
                      fc_level_score* levels_out, int32_t* best_out);
void consensus_cut(Ctx& c, int level, int32_t* labels_out, int64_t* k_out);
// coassoc.h: node ids on the host, validated by the caller; b null: b = a
void coassoc_matrix(Ctx& c, int64_t na, const int32_t* a, int64_t nb, const int32_t* b, int32_t* dev_out);
void coassoc_pairs(Ctx& c, int64_t npairs, const int32_t* pairs, int32_t* dev_out);
void coassoc_hist(Ctx& c, int64_t k, const int32_t* nodes, int64_t* hist);
// cluster.h: labels on the host in node order, validated by the caller
void cluster_consensus(Ctx& c, const int32_t* labels, int32_t* ids_out, int64_t* size_out, int64_t* dev_cluster,
                       int64_t* dev_item, fc_cluster_info* info);
// vote.h: labels on the host in node order, validated by the caller; device outputs may be null
void vote_map(Ctx& c, const int32_t* labels, int32_t* dev_mapped, fc_vote_info* info);
void vote_count(Ctx& c, const int32_t* labels, const int32_t* dev_mapped, int n_total, int32_t* dev_top, int32_t* dev_tv,
                int32_t* dev_own, int64_t* own_hist, fc_vote_info* info);
void vote(Ctx& c, const int32_t* labels, int32_t* dev_top, int32_t* dev_tv, int32_t* dev_own, int64_t* own_hist,
          fc_vote_info* info);
// affinity.h: labels and the query lists on the host, validated by the caller; npairs >= 1
void item_affinity(Ctx& c, const int32_t* labels, int64_t npairs, const int32_t* nodes, const int32_t* clusters,
                   int64_t* dev_out, fc_affinity_info* info);
// quality.h: labels on the host in node order, validated by the caller; any output may be null
void community_quality(Ctx& c, int graph, const int32_t* labels, fc_community_record* out, int64_t* nin_out,
                       int64_t* nout_out, int32_t* split_out, fc_quality_info* info);
// merge.h: labels and the pair lists on the host, validated by the caller; npairs >= 1
void community_graph(Ctx& c, int graph, const int32_t* labels, int64_t capacity, int32_t* a_out, int32_t* b_out,
                     int64_t* weight_out, int64_t* edges_out, int64_t* npairs_out);
void cluster_coassoc(Ctx& c, const int32_t* labels, int64_t npairs, const int32_t* a, const int32_t* b, int64_t* dev_out,
                     fc_cluster_pair_info* info);
// match.h: labels and other (or null: the local labelings) on the host, validated by the caller
void cluster_match(Ctx& c, const int32_t* labels, const int32_t* other, int64_t ld, int32_t* ids_out, int64_t* size_out,
                   int32_t* dev_inter, int32_t* dev_csize, fc_match_info* info);
// timing helpers
int timer_begin(Ctx& c);
int timer_end(Ctx& c, TimerSlot slot, int begin_ev);   // returns the end event (-1: off)
void timer_collect(Ctx& c, fc_stats* st);
// scratch helpers
template <class T> inline T* ensure(DevBuf& b, size_t count) {
    b.ensure(count * sizeof(T) + 16);
    return b.as<T>();
}
void sync(Ctx& c);
// zero / fold sharded counters (CSH x F u64 in c.counters); max_mask bit f: max instead of sum
unsigned long long* shards_begin(Ctx& c, int F);
void shards_fold(Ctx& c, int F, unsigned max_mask, int64_t* host_out);
int64_t read_i64(Ctx& c, const int64_t* dev);

constexpr int64_t AGE_ITER_SHIFT = 40;
constexpr int64_t AGE_REPAIR_OFFSET = int64_t(1) << 39;

}  // namespace fc
