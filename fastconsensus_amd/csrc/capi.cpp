// capi.cpp -- extern "C" entry points (include/fastconsensus_amd.h) and the native
// driver loop that replaces fast_consensus()'s while-loop (fast_consensus.py:138-411).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "fc_ctx.h"

namespace fc {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

// ------------------------------------------------------------------ timing
int timer_begin(Ctx& c) {
    Timer& t = c.timer;
    if (!t.on) return -1;
    if (t.next >= t.pool.size()) {
        size_t add = t.pool.empty() ? 4096 : t.pool.size();
        for (t.pool.reserve(t.pool.size() + add); add > 0; --add) {
            hipEvent_t e;
            FC_HIP(hipEventCreate(&e));
            t.pool.push_back(e);
        }
    }
    const int idx = (int)t.next++;
    FC_HIP(hipEventRecord(t.pool[idx], c.stream));
    return idx;
}
int timer_end(Ctx& c, TimerSlot slot, int b) {
    if (b < 0) return -1;
    const int e = timer_begin(c);
    c.timer.spans[slot].push_back({b, e});
    return e;
}
void timer_collect(Ctx& c, fc_stats* st) {
    Timer& t = c.timer;
    double ms[TS_COUNT] = {};
    int64_t launches[TS_COUNT] = {};
    if (!t.pool.empty()) FC_HIP(hipStreamSynchronize(c.stream));
    for (int s = 0; s < TS_COUNT; ++s) {
        for (auto& pr : t.spans[s]) {
            float x = 0.f;
            FC_HIP(hipEventElapsedTime(&x, t.pool[pr.first], t.pool[pr.second]));
            ms[s] += x;
        }
        launches[s] = (int64_t)t.spans[s].size();
        t.spans[s].clear();
    }
    t.next = 0;
    if (st) {
        *st = c.prof;
        st->cd_ms = ms[TS_CD]; st->consensus_ms = ms[TS_CONSENSUS]; st->closure_ms = ms[TS_CLOSURE]; st->rebuild_ms = ms[TS_REBUILD];
        st->decide_ms = ms[TS_DECIDE]; st->decide_launches = launches[TS_DECIDE];
        st->lv_decide_ms = ms[TS_LV_DECIDE]; st->lv_decide_launches = launches[TS_LV_DECIDE];
        st->lv_heavy_ms = ms[TS_LV_HEAVY]; st->lv_heavy_launches = launches[TS_LV_HEAVY];
        st->rl_decide_ms = ms[TS_RL_DECIDE]; st->rl_decide_launches = launches[TS_RL_DECIDE];
    }
    c.prof = fc_stats{};
}

static void bind(Ctx& c) { FC_HIP(hipSetDevice(c.device)); }

static bool known_algo(int algo) {
    return is_louvain(algo) || algo == FC_ALGO_LPM || algo == FC_ALGO_LEIDEN || algo == FC_ALGO_INFOMAP;
}
// community detection of a loop variant (:148 / :270 / :210-211 / :268)
static void run_cd(Ctx& c, int algo, int rbegin, int rcount, int n_p_total, int iteration) {
    if (algo == FC_ALGO_LEIDEN) leiden_run(c, rbegin, rcount, n_p_total, iteration);
    else if (algo == FC_ALGO_INFOMAP) infomap_run(c, rbegin, rcount, n_p_total, iteration);
    else if (c.cd_engine == 2) cd_run_hybrid(c, algo, rbegin, rcount, n_p_total, iteration);
    else if (c.cd_engine == 1 && cd_rl_supported(c, algo)) cd_run_rl(c, algo, rbegin, rcount, n_p_total, iteration);
    else cd_run(c, algo, rbegin, rcount, n_p_total, iteration);
}

}  // namespace fc

using namespace fc;

struct fc_ctx {
    Ctx c;
};

#define FC_API_BEGIN try {
#define FC_API_END                                   \
    }                                                \
    catch (const FcError& e) {                       \
        set_error(e.msg);                            \
        return e.code;                               \
    }                                                \
    catch (const std::exception& e) {                \
        set_error(std::string("exception: ") + e.what()); \
        return FC_EINVAL;                            \
    }                                                \
    return FC_OK;

#define FC_CTX(ctx)                                              \
    if (!(ctx)) { set_error("null context"); return FC_EINVAL; } \
    Ctx& c = (ctx)->c;                                           \
    bind(c);

// the fc_*_timing getters: the device time of the last call's phases (Ctx::cp_ms / lv_ms / ca_ms / cc_ms / cm_ms)
template <int N> static int phase_timing(fc_ctx* ctx, double (Ctx::*src)[N], double* ms) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(ms, FC_EINVAL, "null output buffer");
    for (int i = 0; i < N; ++i) ms[i] = (c.*src)[i];
    FC_API_END
}

// ------------------------------------------------------------------ argument checks
// Every id of a host array lies in [0, n), else FC_EINVAL naming `prefix`, the id and its index.  `what`
// names the array where its length or its address is refused; an entry point with checks of its own
// for those makes them first, in its own order.  Out-of-range ids would be out-of-bounds device
// accesses (they index [N] tables), so they are refused here, before anything is launched.
static void check_ids(const Ctx& c, const char* prefix, const int32_t* ids, int64_t count, const char* what = "ids") {
    FC_REQUIRE(count >= 0, FC_EINVAL, std::string("negative length of ") + what);
    FC_REQUIRE(ids || count == 0, FC_EINVAL, std::string("null ") + what);
    const uint32_t lim = (uint32_t)c.N;
    for (int64_t i = 0; i < count; ++i)
        FC_REQUIRE((uint32_t)ids[i] < lim, FC_EINVAL,
                   std::string(prefix) + " " + std::to_string(ids[i]) + " at index " + std::to_string(i) +
                       " outside [0, n)");
}
// the replicas one analysis call handles (the cell kernels' per-lane state)
static void replica_cap(int count, const char* who, const char* unit = "local replicas") {
    constexpr int MAX_REPLICAS = 2048;
    FC_REQUIRE(count <= MAX_REPLICAS, FC_ELIMIT,
               std::string(who) + " handles at most " + std::to_string(MAX_REPLICAS) + " " + unit);
}
static void score_graph(int graph) {
    FC_REQUIRE(graph == FC_SCORE_GRAPH_INPUT || graph == FC_SCORE_GRAPH_WORKING, FC_EINVAL,
               "graph must be FC_SCORE_GRAPH_INPUT or FC_SCORE_GRAPH_WORKING");
}
// nothing to launch (no queries): the info of an empty call, its cluster count from the host
template <class Info> static void empty_call_info(const Ctx& c, const int32_t* labels, Info* info) {
    if (!info) return;
    std::vector<char> seen((size_t)c.N, 0);
    int64_t k = 0;
    for (int64_t i = 0; i < c.N; ++i)
        if (!seen[labels[i]]) { seen[labels[i]] = 1; ++k; }
    *info = Info{};
    info->k = k; info->n_r = c.n_r;
}

extern "C" {

const char* fc_last_error(void) { return g_err.c_str(); }
const char* fc_version(void) { return "fastconsensus_amd 0.1.0 (gfx950)"; }
#ifndef FC_BUILD_HASH
#define FC_BUILD_HASH "unknown"
#endif
const char* fc_build_hash(void) { return FC_BUILD_HASH; }

int fc_create(int device, uint64_t seed, fc_ctx** out) {
    if (!out) { set_error("null out"); return FC_EINVAL; }
    *out = nullptr;
    FC_API_BEGIN
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        throw FcError{FC_ENODEV, "no HIP device visible (the engine has no CPU fallback)"};
    FC_REQUIRE(device >= 0 && device < n, FC_ENODEV, "device ordinal out of range");
    hipDeviceProp_t prop;
    FC_HIP(hipGetDeviceProperties(&prop, device));
    FC_REQUIRE(std::strstr(prop.gcnArchName, "gfx950") != nullptr, FC_ENODEV,
               std::string("engine is built for gfx950 (MI355X); device is ") + prop.gcnArchName);
    std::unique_ptr<fc_ctx> x(new fc_ctx());   // a failure below frees what the context already owns
    Ctx& c = x->c;
    c.device = device;
    c.seed = seed;
    FC_HIP(hipSetDevice(device));
    FC_HIP(hipStreamCreateWithFlags(&c.own_stream.s, hipStreamNonBlocking));
    c.stream = c.own_stream.s;
    FC_HIP(hipHostMalloc((void**)&c.hpin.p, FC_HPIN_I64 * sizeof(int64_t), hipHostMallocDefault));
    *out = x.release();
    FC_API_END
}

void fc_destroy(fc_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->c.device);
    (void)hipStreamSynchronize(ctx->c.stream);   // in front of every free
    delete ctx;   // buffers, events, pinned scratch and stream: their owners' destructors
}

int64_t fc_device_bytes(void) { return DevBuf::held.load(); }

int fc_set_stream(fc_ctx* ctx, void* s) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_HIP(hipStreamSynchronize(c.stream));
    c.stream = s ? (hipStream_t)s : c.own_stream.s;
    FC_API_END
}

int fc_synchronize(fc_ctx* ctx) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_HIP(hipStreamSynchronize(c.stream));
    FC_API_END
}

int fc_set_timing(fc_ctx* ctx, int enable) {
    FC_CTX(ctx)
    FC_API_BEGIN
    c.timer.on = enable != 0;
    FC_API_END
}

int fc_set_params(fc_ctx* ctx, int buckets, int max_sweeps, int max_iters) {
    FC_CTX(ctx)
    FC_API_BEGIN
    if (buckets > 0) c.buckets = buckets;
    if (max_sweeps > 0) c.max_sweeps = max_sweeps;
    if (max_iters > 0) c.max_iters = max_iters;
    FC_API_END
}

int fc_set_option(fc_ctx* ctx, int option, int64_t value) {
    FC_CTX(ctx)
    FC_API_BEGIN
    switch (option) {
        case FC_OPT_BUCKETS: FC_REQUIRE(value >= 0, FC_EINVAL, "buckets >= 0 (0: per-algorithm default)"); c.buckets = (int)value; break;
        case FC_OPT_MAX_SWEEPS: FC_REQUIRE(value >= 1, FC_EINVAL, "max_sweeps >= 1"); c.max_sweeps = (int)value; break;
        case FC_OPT_MAX_ITERS: FC_REQUIRE(value >= 1, FC_EINVAL, "max_iters >= 1"); c.max_iters = (int)value; break;
        case FC_OPT_CHUNK:
            FC_REQUIRE(value == 0 || value == 16, FC_EINVAL, "chunk must be 0 or 16");
            c.chunk = (int)value;
            break;
        case FC_OPT_PRUNE: c.prune = value != 0; break;
        case FC_OPT_RELABEL: FC_REQUIRE(value >= 0 && value <= 2, FC_EINVAL, "relabel 0, 1 or 2"); c.relabel = (int)value; break;
        case FC_OPT_STORE: c.store_order = value != 0; break;
        case FC_OPT_COARSEN: FC_REQUIRE(value >= 0, FC_EINVAL, "coarsen >= 0"); c.coarsen = (int)value; break;
        case FC_OPT_SEED: c.seed = (uint64_t)value; break;
        case FC_OPT_CLOSURE_ROUNDS: FC_REQUIRE(value >= 0, FC_EINVAL, "closure_rounds >= 1, or 0 (per algorithm)"); c.closure_rounds = (int)value; break;
        case FC_OPT_PRUNE_MARK: FC_REQUIRE(value >= 0 && value <= 2, FC_EINVAL, "prune_mark must be 0, 1 or 2"); c.prune_mark = (int)value; break;
        case FC_OPT_INFOMAP_TRIALS: FC_REQUIRE(value >= 1, FC_EINVAL, "infomap trials >= 1"); c.infomap_trials = (int)value; break;
        case FC_OPT_CD_ENGINE: FC_REQUIRE(value >= 0 && value <= 2, FC_EINVAL, "cd_engine must be 0, 1 or 2"); c.cd_engine = (int)value; break;
        case FC_OPT_RL_MIN_REPLICAS: FC_REQUIRE(value >= 1, FC_EINVAL, "rl_min_replicas >= 1"); c.rl_min_replicas = value; break;
        case FC_OPT_RL_MIN_VERTICES: FC_REQUIRE(value >= 1, FC_EINVAL, "rl_min_vertices >= 1"); c.rl_min_vertices = value; break;
        case FC_OPT_DENSE_DIV: FC_REQUIRE(value >= 0 && value <= 64, FC_EINVAL, "dense_div must be 0..64"); c.dense_div = (int)value; break;
        case FC_OPT_TAIL_VISITS: FC_REQUIRE(value >= -1, FC_EINVAL, "tail_visits >= 0, or -1 (per algorithm)"); c.tail_visits = value; break;
        default: throw FcError{FC_EINVAL, "unknown option"};
    }
    FC_API_END
}

int fc_load_graph(fc_ctx* ctx, int64_t n, int64_t m, const int32_t* u, const int32_t* v) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(m == 0 || (u && v), FC_EINVAL, "null edge arrays");
    graph_load(c, n, m, u, v);
    c.n_r = 0;
    c.sc_ref_set = false;   // a reference labeling belongs to the graph it was set on
    c.lv_valid = false;     // and so does a consensus hierarchy
    FC_API_END
}

int fc_get_node_map(fc_ctx* ctx, int32_t* sigma) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.N > 0 && sigma, FC_ESTATE, "no graph loaded");
    std::memcpy(sigma, c.h_sigma.data(), 4 * (size_t)c.N);
    FC_API_END
}

int fc_reset_graph(fc_ctx* ctx) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    graph_copy(c, c.g, c.g0);
    FC_API_END
}

int fc_graph_info(fc_ctx* ctx, int64_t* n, int64_t* m, int64_t* m0) {
    FC_CTX(ctx)
    FC_API_BEGIN
    if (n) *n = c.N;
    if (m) *m = c.g.m;
    if (m0) *m0 = c.m_original;
    FC_API_END
}

int fc_get_graph(fc_ctx* ctx, int32_t* u, int32_t* v, int32_t* w, int64_t* age) {
    FC_CTX(ctx)
    FC_API_BEGIN
    graph_to_host(c, c.g.m, c.g.eu.as<int32_t>(), c.g.ev.as<int32_t>(), c.g.ew.as<int32_t>(),
                  c.g.eage.as<int64_t>(), u, v, w, age);
    FC_API_END
}

int fc_get_nextgraph(fc_ctx* ctx, int64_t* m_out, int32_t* u, int32_t* v, int32_t* w, int64_t* age) {
    FC_CTX(ctx)
    FC_API_BEGIN
    const int64_t m = c.kept_m;
    if (m_out) *m_out = m;
    if (u || v || w || age)
        graph_to_host(c, m, c.ku.as<int32_t>(), c.kv.as<int32_t>(), c.kw.as<int32_t>(), c.kage.as<int64_t>(), u, v,
                      w, age);
    FC_API_END
}

int fc_cd(fc_ctx* ctx, int algo, int rbegin, int rcount, int n_p_total, int iteration) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(known_algo(algo), FC_EINVAL, "algo must be louvain, lpm, leiden or infomap");
    run_cd(c, algo, rbegin, rcount, n_p_total, iteration);
    FC_API_END
}

int fc_set_labels(fc_ctx* ctx, int count, const int32_t* labels) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    FC_REQUIRE(count >= 1 && labels, FC_EINVAL, "bad labelings");
    check_ids(c, "label", labels, (int64_t)count * c.N);   // they index per-replica [N] tables
    labels_from_host(c, count, labels);
    c.n_r = count; c.rbase = 0; c.n_p_total = count;
    c.labT_valid = false;
    FC_API_END
}

int fc_replica_info(fc_ctx* ctx, int* count, int* rbegin, int* n_p_total) {
    FC_CTX(ctx)
    FC_API_BEGIN
    if (count) *count = c.n_r;
    if (rbegin) *rbegin = c.rbase;
    if (n_p_total) *n_p_total = c.n_p_total;
    FC_API_END
}

int fc_get_labels(fc_ctx* ctx, int32_t* labels, int64_t capacity, int renumber) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.n_r > 0, FC_ESTATE, "no labelings");
    FC_REQUIRE(labels, FC_EINVAL, "null output buffer");
    FC_REQUIRE(capacity >= (int64_t)c.n_r * c.N, FC_EINVAL,
               "output buffer holds " + std::to_string(capacity) + " labels; " + std::to_string(c.n_r) +
                   " replicas x " + std::to_string(c.N) + " nodes needed");
    labels_to_host(c, labels, renumber != 0);
    FC_API_END
}

int fc_consensus_partial(fc_ctx* ctx, int algo, void* dev_out) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(dev_out || c.g.m == 0, FC_EINVAL, "null output buffer");
    consensus_partial(c, algo, (int32_t*)dev_out);
    FC_API_END
}

int fc_consensus_apply(fc_ctx* ctx, int algo, int n_p, double tau, double delta, const void* dev_partial,
                       int* converged, int64_t* kept_out, int64_t* unconv_out) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(n_p >= 1, FC_EINVAL, "n_p must be >= 1");
    int64_t kept = 0, unc = 0;
    consensus_apply(c, algo, n_p, tau, (const int32_t*)dev_partial, &kept, &unc);
    // check_consensus_graph (:34): not converged iff count > delta * number_of_edges
    if (converged) *converged = is_louvain(algo) ? !((double)unc > delta * (double)kept) : 0;
    if (kept_out) *kept_out = kept;
    if (unconv_out) *unconv_out = unc;
    FC_API_END
}

int fc_closure_sample(fc_ctx* ctx, int64_t attempts, int iteration, int64_t* n_cand) {
    FC_CTX(ctx)
    FC_API_BEGIN
    if (attempts < 0) attempts = c.m_original;
    closure_sample(c, attempts, iteration);
    if (n_cand) *n_cand = c.n_cand;
    FC_API_END
}

static int64_t closure_block_t(const Ctx& c, int block) { return c.clo_attempts * block / c.clo_R; }

int fc_closure_begin(fc_ctx* ctx, int64_t attempts, int iteration, int* blocks) {
    FC_CTX(ctx)
    FC_API_BEGIN
    if (attempts < 0) attempts = c.m_original;
    const int R = closure_begin(c, attempts, iteration);
    if (blocks) *blocks = R;
    FC_API_END
}

int fc_closure_block_sample(fc_ctx* ctx, int block, int64_t t_lo, int64_t t_hi, void* dev_out, int64_t capacity,
                            int64_t* count) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.clo_next >= 0, FC_ESTATE, "fc_closure_begin first");
    FC_REQUIRE(block == c.clo_next, FC_ESTATE,
               "closure block " + std::to_string(block) + " sampled before block " + std::to_string(c.clo_next) +
                   " was added");
    FC_REQUIRE(block < c.clo_R, FC_EINVAL, "closure block out of range");
    FC_REQUIRE(t_lo >= closure_block_t(c, block) && t_lo <= t_hi && t_hi <= closure_block_t(c, block + 1), FC_EINVAL,
               "attempt range outside the block");
    FC_REQUIRE(dev_out || t_hi == t_lo, FC_EINVAL, "null output buffer");
    const int64_t k = closure_block_sample(c, block, t_lo, t_hi, (int64_t*)dev_out, capacity);
    if (count) *count = k;
    FC_API_END
}

int fc_closure_block_add(fc_ctx* ctx, int block, const void* dev_in, int64_t count) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.clo_next >= 0 && block == c.clo_next && block < c.clo_R, FC_ESTATE, "closure blocks go in order");
    FC_REQUIRE(count >= 0 && count <= closure_block_t(c, block + 1) - closure_block_t(c, block), FC_EINVAL,
               "more pairs than the block has attempts");
    FC_REQUIRE(dev_in || count == 0, FC_EINVAL, "null input buffer");
    closure_block_add(c, block, (const int64_t*)dev_in, count);
    FC_API_END
}

int fc_closure_finish(fc_ctx* ctx, int64_t* n_cand) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.clo_next >= 0 && c.clo_next == c.clo_R, FC_ESTATE, "closure blocks missing");
    const int64_t k = closure_finish(c);
    if (n_cand) *n_cand = k;
    FC_API_END
}

int fc_closure_set_pairs(fc_ctx* ctx, int64_t npairs, const int32_t* pairs, int iteration, int64_t* n_cand) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(npairs == 0 || pairs, FC_EINVAL, "null pairs");
    std::vector<int32_t> mapped(2 * (size_t)npairs);
    for (int64_t i = 0; i < 2 * npairs; ++i) {
        FC_REQUIRE(pairs[i] >= 0 && pairs[i] < c.N, FC_EINVAL, "pair endpoint out of range");
        mapped[i] = c.h_sigma[pairs[i]];
    }
    closure_from_pairs(c, npairs, mapped.data(), iteration);
    sync(c);
    if (n_cand) *n_cand = c.n_cand;
    FC_API_END
}

int fc_closure_partial(fc_ctx* ctx, void* dev_out) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.n_r > 0, FC_ESTATE, "no labelings");
    closure_partial(c, (int32_t*)dev_out);
    FC_API_END
}

int fc_closure_apply(fc_ctx* ctx, int algo, int n_p, double delta, const void* dev_counts, int iteration,
                     int* converged, int64_t* m_out) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(!is_louvain(algo) || dev_counts || c.n_cand == 0, FC_EINVAL,
               "louvain closure needs co-membership counts");
    closure_apply(c, algo, n_p, (const int32_t*)dev_counts, iteration);
    const int64_t unc = count_unconverged(c, c.g.ew.as<int32_t>(), c.g.m, n_p);
    if (converged) *converged = !((double)unc > delta * (double)c.g.m);
    if (m_out) *m_out = c.g.m;
    FC_API_END
}

int fc_score_set_reference(fc_ctx* ctx, const int32_t* labels) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    if (labels) check_ids(c, "reference label", labels, c.N);
    score_set_reference(c, labels);
    FC_API_END
}

// what fc_consensus_partition and fc_consensus_levels require of the graph id, the support and the state
static void consensus_input(const Ctx& c, int graph, const void* dev_support, int n_total) {
    score_graph(graph);
    FC_REQUIRE(!dev_support || n_total >= 1, FC_EINVAL, "reduced support needs n_total >= 1");
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    FC_REQUIRE(dev_support || c.n_r > 0, FC_ESTATE,
               "no labelings and no support: run fc_run, fc_cd or fc_set_labels first, or pass dev_support");
}

int fc_score_partitions(fc_ctx* ctx, int graph, fc_part_score* out) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    FC_REQUIRE(c.n_r > 0, FC_ESTATE, "no labelings");
    score_graph(graph);
    FC_REQUIRE(out, FC_EINVAL, "null output buffer");
    score_partitions(c, graph, out);
    FC_API_END
}

int fc_score_pairs(fc_ctx* ctx, const int32_t* pairs, int64_t* npairs, fc_pair_score* out) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    FC_REQUIRE(c.n_r > 0, FC_ESTATE, "no labelings");
    FC_REQUIRE(npairs, FC_EINVAL, "null npairs");
    std::vector<int32_t> all;
    int64_t np = *npairs;
    if (!pairs) {   // every a < b among the local replicas, plus (REF, b) when a reference is set
        for (int a = 0; a < c.n_r; ++a)
            for (int b = a + 1; b < c.n_r; ++b) { all.push_back(a); all.push_back(b); }
        if (c.sc_ref_set)
            for (int b = 0; b < c.n_r; ++b) { all.push_back(FC_SCORE_REF); all.push_back(b); }
        np = (int64_t)all.size() / 2;
        FC_REQUIRE(*npairs >= np, FC_EINVAL,
                   "output holds " + std::to_string(*npairs) + " pairs; " + std::to_string(np) + " needed");
        pairs = all.data();
    } else {
        FC_REQUIRE(np >= 0, FC_EINVAL, "negative pair count");
        for (int64_t i = 0; i < 2 * np; ++i) {
            FC_REQUIRE(pairs[i] == FC_SCORE_REF || (pairs[i] >= 0 && pairs[i] < c.n_r), FC_EINVAL,
                       "pair index " + std::to_string(pairs[i]) + " outside the " + std::to_string(c.n_r) +
                           " local replicas");
            FC_REQUIRE(pairs[i] != FC_SCORE_REF || c.sc_ref_set, FC_ESTATE,
                       "FC_SCORE_REF used with no reference set (fc_score_set_reference)");
        }
    }
    FC_REQUIRE(out || np == 0, FC_EINVAL, "null output buffer");
    if (np > 0) score_pairs(c, pairs, np, out);
    *npairs = np;
    FC_API_END
}

int fc_consensus_support(fc_ctx* ctx, int graph, void* dev_out) {
    FC_CTX(ctx)
    FC_API_BEGIN
    score_graph(graph);
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    FC_REQUIRE(c.n_r > 0, FC_ESTATE, "no labelings: run fc_run, fc_cd or fc_set_labels first");
    FC_REQUIRE(dev_out || (graph == FC_SCORE_GRAPH_INPUT ? c.g0.m : c.g.m) == 0, FC_EINVAL, "null output buffer");
    consensus_support(c, graph, (int32_t*)dev_out);
    FC_API_END
}

int fc_consensus_partition(fc_ctx* ctx, int graph, const void* dev_support, int n_total, double agreement,
                           int32_t* labels_out, int64_t* support_hist, int64_t* node_in, int64_t* node_out,
                           fc_consensus_info* info) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(agreement >= 0.0 && agreement <= 1.0, FC_EINVAL, "agreement must lie in [0, 1]");   // NaN fails both
    consensus_input(c, graph, dev_support, n_total);
    consensus_partition(c, graph, (const int32_t*)dev_support, n_total, agreement, labels_out, support_hist, node_in,
                        node_out, info);
    FC_API_END
}

int fc_consensus_timing(fc_ctx* ctx, double* ms) { return phase_timing(ctx, &Ctx::cp_ms, ms); }

int fc_consensus_levels(fc_ctx* ctx, int graph, const void* dev_support, int n_total, int32_t* birth, int32_t* up,
                        fc_level_score* levels, int32_t* best_level) {
    FC_CTX(ctx)
    FC_API_BEGIN
    consensus_input(c, graph, dev_support, n_total);
    consensus_levels(c, graph, (const int32_t*)dev_support, n_total, birth, up, levels, best_level);
    FC_API_END
}

int fc_consensus_cut(fc_ctx* ctx, int level, int32_t* labels_out, int64_t* k_out) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.N > 0 && c.lv_valid, FC_ESTATE, "no consensus hierarchy: call fc_consensus_levels first");
    FC_REQUIRE(level >= 0 && level <= c.lv_nt, FC_EINVAL,
               "level " + std::to_string(level) + " outside [0, " + std::to_string(c.lv_nt) + "]");
    consensus_cut(c, level, labels_out, k_out);
    FC_API_END
}

int fc_consensus_levels_timing(fc_ctx* ctx, double* ms) { return phase_timing(ctx, &Ctx::lv_ms, ms); }

// co-association: the state checks of score_require come first, then every node id on the host
static void coassoc_state(const Ctx& c) {
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    FC_REQUIRE(c.n_r > 0, FC_ESTATE, "no labelings: run fc_run, fc_cd or fc_set_labels first");
}

int fc_coassociation(fc_ctx* ctx, int64_t na, const int32_t* a, int64_t nb, const int32_t* b, void* dev_out) {
    FC_CTX(ctx)
    FC_API_BEGIN
    coassoc_state(c);
    check_ids(c, "a: node", a, na, "a");
    if (b) check_ids(c, "b: node", b, nb, "b");
    const int64_t cols = b ? nb : na;
    FC_REQUIRE(dev_out || na == 0 || cols == 0, FC_EINVAL, "null output buffer");
    coassoc_matrix(c, na, a, nb, b, (int32_t*)dev_out);
    FC_API_END
}

int fc_coassoc_pairs(fc_ctx* ctx, int64_t npairs, const int32_t* pairs, void* dev_out) {
    FC_CTX(ctx)
    FC_API_BEGIN
    coassoc_state(c);
    FC_REQUIRE(npairs >= 0 && npairs < ((int64_t)1 << 40), FC_EINVAL, "bad pair count");
    check_ids(c, "pairs: node", pairs, 2 * npairs, "pairs");
    FC_REQUIRE(dev_out || npairs == 0, FC_EINVAL, "null output buffer");
    coassoc_pairs(c, npairs, pairs, (int32_t*)dev_out);
    FC_API_END
}

int fc_coassoc_hist(fc_ctx* ctx, int64_t k, const int32_t* nodes, int64_t* hist) {
    FC_CTX(ctx)
    FC_API_BEGIN
    coassoc_state(c);
    check_ids(c, "nodes: node", nodes, k, "nodes");
    FC_REQUIRE(hist, FC_EINVAL, "null output buffer");
    coassoc_hist(c, k, nodes, hist);
    FC_API_END
}

int fc_coassoc_timing(fc_ctx* ctx, double* ms) { return phase_timing(ctx, &Ctx::ca_ms, ms); }

int fc_cluster_consensus(fc_ctx* ctx, const int32_t* labels, int32_t* ids_out, int64_t* size_out, void* dev_cluster,
                         void* dev_item, fc_cluster_info* info) {
    FC_CTX(ctx)
    FC_API_BEGIN
    coassoc_state(c);
    replica_cap(c.n_r, "cluster consensus");
    FC_REQUIRE(labels, FC_EINVAL, "null labels");
    check_ids(c, "cluster label", labels, c.N);
    cluster_consensus(c, labels, ids_out, size_out, (int64_t*)dev_cluster, (int64_t*)dev_item, info);
    FC_API_END
}

int fc_cluster_consensus_timing(fc_ctx* ctx, double* ms) { return phase_timing(ctx, &Ctx::cc_ms, ms); }

// plurality vote: the partition's ids on the host, before anything is launched
static void vote_labels(const Ctx& c, const int32_t* labels) {
    FC_REQUIRE(labels, FC_EINVAL, "null labels");
    check_ids(c, "vote label", labels, c.N);
}

int fc_vote_map(fc_ctx* ctx, const int32_t* labels, void* dev_mapped, fc_vote_info* info) {
    FC_CTX(ctx)
    FC_API_BEGIN
    coassoc_state(c);
    replica_cap(c.n_r, "the vote");
    vote_labels(c, labels);
    FC_REQUIRE(dev_mapped, FC_EINVAL, "null dev_mapped");
    vote_map(c, labels, (int32_t*)dev_mapped, info);
    FC_API_END
}

int fc_vote_count(fc_ctx* ctx, const int32_t* labels, const void* dev_mapped, int n_total, void* dev_top,
                  void* dev_top_votes, void* dev_own_votes, int64_t* own_hist, fc_vote_info* info) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    FC_REQUIRE(n_total >= 1, FC_EINVAL, "n_total must be at least 1");
    replica_cap(n_total, "the vote", "replicas");
    vote_labels(c, labels);
    FC_REQUIRE(dev_mapped, FC_EINVAL, "null dev_mapped");
    vote_count(c, labels, (const int32_t*)dev_mapped, n_total, (int32_t*)dev_top, (int32_t*)dev_top_votes,
               (int32_t*)dev_own_votes, own_hist, info);
    FC_API_END
}

int fc_vote(fc_ctx* ctx, const int32_t* labels, void* dev_top, void* dev_top_votes, void* dev_own_votes,
            int64_t* own_hist, fc_vote_info* info) {
    FC_CTX(ctx)
    FC_API_BEGIN
    coassoc_state(c);
    replica_cap(c.n_r, "the vote");
    vote_labels(c, labels);
    vote(c, labels, (int32_t*)dev_top, (int32_t*)dev_top_votes, (int32_t*)dev_own_votes, own_hist, info);
    FC_API_END
}

int fc_vote_timing(fc_ctx* ctx, double* ms) { return phase_timing(ctx, &Ctx::vt_ms, ms); }

int fc_item_affinity(fc_ctx* ctx, const int32_t* labels, int64_t npairs, const int32_t* nodes, const int32_t* clusters,
                     void* dev_out, fc_affinity_info* info) {
    FC_CTX(ctx)
    FC_API_BEGIN
    coassoc_state(c);
    replica_cap(c.n_r, "item affinity");
    FC_REQUIRE(npairs >= 0, FC_EINVAL, "negative query count");
    FC_REQUIRE(npairs < ((int64_t)1 << 31), FC_ELIMIT, "item affinity handles fewer than 2^31 queries a call");
    FC_REQUIRE(labels, FC_EINVAL, "null labels");
    FC_REQUIRE(npairs == 0 || (nodes && clusters), FC_EINVAL, "null query list");
    FC_REQUIRE(npairs == 0 || dev_out, FC_EINVAL, "null output buffer");
    check_ids(c, "cluster label", labels, c.N);
    check_ids(c, "query node", nodes, npairs);
    check_ids(c, "query cluster", clusters, npairs);
    for (double& m : c.ia_ms) m = 0.0;
    if (npairs == 0)
        empty_call_info(c, labels, info);
    else
        item_affinity(c, labels, npairs, nodes, clusters, (int64_t*)dev_out, info);
    FC_API_END
}

int fc_item_affinity_timing(fc_ctx* ctx, double* ms) { return phase_timing(ctx, &Ctx::ia_ms, ms); }

int fc_community_quality(fc_ctx* ctx, int graph, const int32_t* labels, fc_community_record* out, int64_t* node_in,
                         int64_t* node_out, int32_t* split_out, fc_quality_info* info) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    score_graph(graph);
    FC_REQUIRE(labels, FC_EINVAL, "null labels");
    check_ids(c, "cluster label", labels, c.N);
    community_quality(c, graph, labels, out, node_in, node_out, split_out, info);
    FC_API_END
}

int fc_community_quality_timing(fc_ctx* ctx, double* ms) { return phase_timing(ctx, &Ctx::ql_ms, ms); }

int fc_community_graph(fc_ctx* ctx, int graph, const int32_t* labels, int64_t capacity, void* a_out, void* b_out,
                       void* weight_out, void* edges_out, int64_t* npairs_out) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    score_graph(graph);
    FC_REQUIRE(labels, FC_EINVAL, "null labels");
    FC_REQUIRE(npairs_out, FC_EINVAL, "null npairs_out");
    check_ids(c, "cluster label", labels, c.N);
    community_graph(c, graph, labels, capacity, (int32_t*)a_out, (int32_t*)b_out, (int64_t*)weight_out,
                    (int64_t*)edges_out, npairs_out);
    FC_API_END
}

int fc_community_graph_timing(fc_ctx* ctx, double* ms) { return phase_timing(ctx, &Ctx::mg_ms, ms); }

int fc_cluster_coassoc(fc_ctx* ctx, const int32_t* labels, int64_t npairs, const int32_t* a, const int32_t* b,
                       void* dev_out, fc_cluster_pair_info* info) {
    FC_CTX(ctx)
    FC_API_BEGIN
    coassoc_state(c);
    replica_cap(c.n_r, "pair co-association");
    FC_REQUIRE(npairs >= 0, FC_EINVAL, "negative pair count");
    FC_REQUIRE(npairs < ((int64_t)1 << 31), FC_ELIMIT, "pair co-association handles fewer than 2^31 pairs a call");
    FC_REQUIRE(labels, FC_EINVAL, "null labels");
    FC_REQUIRE(npairs == 0 || (a && b), FC_EINVAL, "null pair list");
    FC_REQUIRE(npairs == 0 || dev_out, FC_EINVAL, "null output buffer");
    check_ids(c, "cluster label", labels, c.N);
    check_ids(c, "pair cluster a", a, npairs);
    check_ids(c, "pair cluster b", b, npairs);
    for (double& m : c.mc_ms) m = 0.0;
    if (npairs == 0)
        empty_call_info(c, labels, info);
    else
        cluster_coassoc(c, labels, npairs, a, b, (int64_t*)dev_out, info);
    FC_API_END
}

int fc_cluster_coassoc_timing(fc_ctx* ctx, double* ms) { return phase_timing(ctx, &Ctx::mc_ms, ms); }

int fc_cluster_match(fc_ctx* ctx, const int32_t* labels, const int32_t* other, int64_t ld, int32_t* ids_out,
                     int64_t* size_out, void* dev_inter, void* dev_csize, fc_match_info* info) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    if (!other) {
        FC_REQUIRE(c.n_r > 0, FC_ESTATE, "no labelings: run fc_run, fc_cd or fc_set_labels first, or pass `other`");
        replica_cap(c.n_r, "the cluster match");
    }
    FC_REQUIRE(labels, FC_EINVAL, "null labels");
    check_ids(c, "labels: id", labels, c.N);
    if (other) check_ids(c, "other: id", other, c.N);
    cluster_match(c, labels, other, ld, ids_out, size_out, (int32_t*)dev_inter, (int32_t*)dev_csize, info);
    FC_API_END
}

int fc_cluster_match_timing(fc_ctx* ctx, double* ms) { return phase_timing(ctx, &Ctx::cm_ms, ms); }

int fc_collect_timing(fc_ctx* ctx, fc_stats* st) {
    FC_CTX(ctx)
    FC_API_BEGIN
    timer_collect(c, st);
    FC_API_END
}

int fc_run(fc_ctx* ctx, int algo, int n_p, double tau, double delta, int32_t* labels_out, fc_stats* st) {
    FC_CTX(ctx)
    FC_API_BEGIN
    FC_REQUIRE(known_algo(algo), FC_EINVAL, "algorithm must be louvain, lpm, leiden or infomap (cnm is out of scope)");
    FC_REQUIRE(n_p >= 1, FC_EINVAL, "n_p must be >= 1");
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    const bool louv = is_louvain(algo);
    graph_copy(c, c.g, c.g0);                                         // graph = G.copy() (:131)
    c.acc = fc_stats{};
    fc_stats& a = c.acc;
    a.n_p = n_p;
    if (algo == FC_ALGO_LEIDEN) {
        // fast_consensus.py:204-258 on integer node ids: communities_to_dict keys vertices by
        // str(index) (:97), `node in node_community_lookup` is False for every int node (:217),
        // so nextgraph keeps weight 0 everywhere, :223-227 removes every edge and check #1
        // (:229) sees an empty graph (count 0 > delta*0 is false): converged after one
        // iteration whose CD batch cannot reach the result.  Final pass (:385-388): n_p
        // Leiden runs on `graph` = G with unit weights.
        a.iterations = 1;
        a.exit_check = 1;
        leiden_run(c, 0, n_p, n_p, 0x40000000);
        a.partition_edges += (int64_t)n_p * c.g.m;
        a.m_final = c.g.m;
        if (labels_out) labels_to_host(c, labels_out, true);
        sync(c);
        if (st) *st = a;
        return FC_OK;
    }
    int it = 0;
    for (;;) {
        if (it >= c.max_iters) { a.hit_iter_cap = 1; break; }
        run_cd(c, algo, 0, n_p, n_p, it);                             // :148 / :270 / :268
        int32_t* part = ensure<int32_t>(c.part, c.g.m + 1);
        consensus_partial(c, algo, part);                             // :150-159 / :273-280
        a.partition_edges += (int64_t)n_p * c.g.m;
        int64_t kept = 0, unc = 0;
        consensus_apply(c, algo, n_p, tau, part, &kept, &unc);        // :163-168 / :284-288
        if (louv && !((double)unc > delta * (double)kept)) {          // check #1 (:172-173)
            a.exit_check = 1;
            break;
        }
        closure_sample(c, c.m_original, it);                          // :175-184 / :292-300
        int32_t* cnt = nullptr;
        if (louv && c.n_cand > 0) {
            cnt = ensure<int32_t>(c.ccount, c.n_cand);
            closure_partial(c, cnt);                                  // :186-190
        }
        closure_apply(c, algo, n_p, cnt, it);                         // :193-198 / :307
        const int64_t unc2 = count_unconverged(c, c.g.ew.as<int32_t>(), c.g.m, n_p);
        ++it;
        if (!((double)unc2 > delta * (double)c.g.m)) {                // :201-202 / :309-310
            a.exit_check = 2;
            break;
        }
    }
    a.iterations = it + (a.exit_check == 1 ? 1 : 0);
    run_cd(c, algo, 0, n_p, n_p, 0x40000000 + it);                   // final pass :383-392
    a.partition_edges += (int64_t)n_p * c.g.m;
    a.m_final = c.g.m;
    if (labels_out) {
        labels_to_host(c, labels_out, true);
    }
    sync(c);
    if (st) *st = a;  // *_ms / decide_launches stay 0: fc_collect_timing() fills them
    FC_API_END
}

}  // extern "C"
