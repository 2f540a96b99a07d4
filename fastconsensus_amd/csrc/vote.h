// vote.h -- plurality vote of the local labelings on a given partition P (fc_vote_map /
// fc_vote_count / fc_vote): relabel-and-vote (Dudoit & Fridlyand; Strehl & Ghosh), all integers.
// With C_r[k][d] = the members of cluster k of P that replica r labels d,
//     map_r(d)     = the cluster k of largest C_r[k][d], the smallest id among equals
//     mapped[r][v] = map_r(lab_r(v))
//     votes_v(k)   = the replicas r with mapped[r][v] = k;  own[v] = votes_v(P(v))
//     top[v]       = the cluster of most votes: P(v) when it is among the leaders, else the smallest id
// Included at the end of consensus.hip after cluster.h (its cell_chunks, score.h's segments,
// cell-kernel pieces, fallback plan and ScLabT, analysis.h's wave_bin_add are in scope).
//
// Map: score.h's sc_list_walk (one wave per cluster of P, LANES ARE REPLICAS, the (label, count)
// list of the lane's replica in SC_D registers); at the segment's end the list is the row C_r[k][.]
// and every entry goes to best[lane][label] as one 64-bit atomicMax of
// (count << 32) | (0xffffffff - rank of the cluster in ascending id order): the maximum is (largest
// count, smallest id) whatever the order of arrival.  A lane with a ninth label and every lane of a
// cluster past the length cap go through cluster.h's cell_chunks: the keys sorted and run-length
// encoded chunk by chunk, where a run is one cell C_r[k][d] and makes the same atomicMax.  One bank
// of 64 replicas at a time, so `best` is 8 * N * min(n_r, 64) bytes however many replicas the
// context holds.
// Count: one thread per node over mapped[.][t] (coalesced), a register list of VT_D (id, votes);
// a node with a ninth id is compacted and sorted in LDS by one wave.
#pragma once
#include <algorithm>
#include <climits>
#include <vector>

namespace fc {

static constexpr int VT_D = 8;   // register-resident distinct clusters per node
// Ctx::vt_ctr slots
enum { VT_MOVED, VT_UNANIMOUS, VT_TIED, VT_SLOW, VT_BAD, VT_K, VT_KVOTED, VT_NCOMM, VT_CTRS };

// the spans between consecutive marks, each added to the phase it was marked with (a phase may
// own several spans: the map runs bank after bank); timing enabled only
struct VoteMarks {
    Ctx& c;
    std::vector<int> ev, phase;
    explicit VoteMarks(Ctx& x) : c(x) {
        for (double& m : c.vt_ms) m = 0.0;
    }
    void mark(int ph = -1) {   // -1: a start
        if (!c.timer.on) return;
        ev.push_back(timer_begin(c));
        phase.push_back(ph);
    }
    void collect() {   // after a stream synchronise
        for (size_t i = 1; i < ev.size(); ++i) {
            if (phase[i] < 0) continue;
            float x = 0.f;
            FC_HIP(hipEventElapsedTime(&x, c.timer.pool[ev[i - 1]], c.timer.pool[ev[i]]));
            c.vt_ms[phase[i]] += x;
        }
    }
};

// ------------------------------------------------------------------ map: count kernel (lanes are replicas)
// labT: the bank's first column (lane = replica of the bank, n_rb of them).  best[lane * N + label],
// zeroed by the caller (a cell counts at least 1, so 0 is "no cell yet"); the arrival that finds 0
// counts the community in *ncomm.  ovf[cluster]: the lanes left to the fallback.
__global__ __launch_bounds__(256) void k_vm_count(int64_t k, const int32_t* __restrict__ seg,
                                                  const int32_t* __restrict__ sval,
                                                  const int32_t* __restrict__ labT, int ldT, int n_rb, int lcap,
                                                  int64_t N, unsigned long long* __restrict__ ovf,
                                                  unsigned long long* __restrict__ best,
                                                  unsigned long long* __restrict__ ncomm) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool act = lane < n_rb;
    const int32_t* col = labT + (act ? lane : 0);
    unsigned long long* mine = best + (int64_t)(act ? lane : 0) * N;
    unsigned long long fresh = 0;
    for (int64_t cc = (int64_t)blockIdx.x * 4 + w; cc < k; cc += (int64_t)gridDim.x * 4) {
        const int32_t s0 = seg[cc], s1 = seg[cc + 1], len = s1 - s0;
        bool ov = act && len > lcap;
        if (len <= lcap) {   // wave-uniform
            int32_t key[SC_D];
            int32_t cnt[SC_D];
            sc_list_walk(key, cnt, s0, s1, sval, col, ldT, act, ov, lane);
            if (act && !ov) {
                const unsigned long long low = 0xffffffffull - (unsigned long long)cc;
#pragma unroll
                for (int d = 0; d < SC_D; ++d)
                    if (key[d] >= 0 && (int64_t)key[d] < N)
                        fresh += atomicMax(&mine[key[d]], ((unsigned long long)cnt[d] << 32) | low) == 0ull;
            }
        }
        const unsigned long long mask = __ballot(ov);
        if (lane == 0) ovf[cc] = mask;
    }
    fresh = sc_wave_sum(fresh);
    if (lane == 0 && fresh) atomicAdd(ncomm, fresh);
}
// One run of the sorted fallback keys ((cluster * 64 + lane) << 32 | label) = one cell of `count` members.
__global__ __launch_bounds__(256) void k_vm_fold(const int32_t* __restrict__ nruns,
                                                 const unsigned long long* __restrict__ ukeys,
                                                 const int32_t* __restrict__ counts, int64_t N,
                                                 unsigned long long* __restrict__ best,
                                                 unsigned long long* __restrict__ ncomm) {
    const int64_t n = *nruns;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = ukeys[j];
        if (key == ~0ull) continue;   // the chunk's padding
        const unsigned long long slot = key >> 32, cc = slot >> 6, lab = key & 0xffffffffull;
        if ((int64_t)lab >= N) continue;
        const unsigned long long val = ((unsigned long long)counts[j] << 32) | (0xffffffffull - cc);
        if (atomicMax(&best[(int64_t)(slot & 63ull) * N + (int64_t)lab], val) == 0ull) atomicAdd(ncomm, 1ull);
    }
}
// mapped[lane * N + t] for the bank's replicas, t in node order: one block row (blockIdx.y) per
// replica, so the blocks in flight share one replica's label row (lab, slot order: 4 N bytes) and
// the cells of `best` that replica touches (one 64-byte line per community), both cache-resident;
// a thread per node walking its labT row instead gathers from all 64 replicas' cells at once
// (8 N * 64 bytes, past the last-level cache at a million nodes).
__global__ __launch_bounds__(256) void k_vm_apply(int64_t N, int64_t k, const int32_t* __restrict__ tpos,
                                                  const int32_t* __restrict__ lab,
                                                  const unsigned long long* __restrict__ best,
                                                  const uint32_t* __restrict__ ulab, int32_t* __restrict__ mapped) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, off = (int64_t)blockIdx.y * N;
    if (t >= N) return;
    const int32_t d = lab[off + tpos[t]];
    const uint32_t rank = 0xffffffffu - (uint32_t)best[off + ((uint32_t)d < (uint64_t)N ? d : 0)];
    mapped[off + t] = (int64_t)rank < k ? (int32_t)ulab[rank] : -1;
}
// the exact path of one bank (its entries are the clusters: nbk = k); returns the (member, replica)
// pairs handled here
static int64_t vote_map_fallback(Ctx& c, const ScSeg& s, const int32_t* labT, const unsigned long long* ovf,
                                 unsigned long long* best, unsigned long long* ncomm) {
    const ScPlan p = score_fallback_plan(c, s, s.k, ovf, "too many (cluster, replica) slots for the vote map's fallback");
    if (p.T == 0) return 0;
    cell_chunks<false>(c, s, p, ovf, labT, c.ldT, [&](const CellChunk& ch) {
        k_vm_fold<<<std::min<unsigned>(nblk(ch.n), 4096u), TB, 0, c.stream>>>(ch.nruns, ch.ukeys, ch.counts, c.N, best, ncomm);
    });
    return p.T;
}

// in: P on the device in node order.  mapped: device int32[n_r][N].  Queues the work; the caller
// synchronises and reads vt_ctr[VT_NCOMM].  Returns the fallback's (member, replica) pairs.
static int64_t vote_map_run(Ctx& c, const int32_t* in, int32_t* mapped, int64_t* k_out, VoteMarks& ph) {
    const int64_t N = c.N;
    const int banks = (c.n_r + 63) / 64;
    ph.mark();
    const ScSeg s = partition_segments(c, in);
    ph.mark(0);   // segments
    unsigned long long* best = (unsigned long long*)ensure<uint64_t>(c.vt_best, (size_t)N * std::min(c.n_r, 64));
    unsigned long long* ovf = (unsigned long long*)ensure<uint64_t>(c.sc_ovf, (size_t)s.k + 1);
    unsigned long long* ctr = (unsigned long long*)ensure<uint64_t>(c.vt_ctr, VT_CTRS);
    FC_HIP(hipMemsetAsync(ctr + VT_NCOMM, 0, sizeof(uint64_t), c.stream));
    const int lcap = score_list_cap(c, true), gx = score_count_grid(s.k);
    int64_t slow = 0;
    for (int b = 0; b < banks; ++b) {
        const int n_rb = std::min(64, c.n_r - b * 64);
        const int32_t* labT = c.labT.as<int32_t>() + b * 64;
        FC_HIP(hipMemsetAsync(best, 0, sizeof(uint64_t) * (size_t)N * n_rb, c.stream));
        k_vm_count<<<gx, TB, 0, c.stream>>>(s.k, s.seg, s.sval, labT, c.ldT, n_rb, lcap, N, ovf, best, ctr + VT_NCOMM);
        ph.mark(1);   // map
        slow += vote_map_fallback(c, s, labT, ovf, best, ctr + VT_NCOMM);
        ph.mark(2);   // map fallback
        k_vm_apply<<<dim3(nblk(N), n_rb), TB, 0, c.stream>>>(N, s.k, c.tpos.as<int32_t>(),
                                                             c.lab.as<int32_t>() + (int64_t)b * 64 * N, best,
                                                             c.sc_ulab.as<uint32_t>(), mapped + (int64_t)b * 64 * N);
        ph.mark(1);
    }
    *k_out = s.k;
    return slow;
}

// ------------------------------------------------------------------ count
__global__ void k_vc_present(int64_t N, const int32_t* __restrict__ P, int32_t* __restrict__ present) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N) present[P[t]] = 1;
}
// *out += the nonzero entries of f[0 .. n)
__global__ __launch_bounds__(256) void k_vc_flags(int64_t n, const int32_t* __restrict__ f,
                                                  unsigned long long* __restrict__ out) {
    unsigned long long s = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) s += f[i] != 0;
    s = sc_wave_sum(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}
// One thread per node t (node order).  A value of mapped that is no id of P sets ctr[VT_BAD] and is
// not counted; a node with more than VT_D ids goes to slow_list (ctr[VT_SLOW] is its cursor).
// hist[own] through LDS bins; top_flag[top] = 1.
__global__ __launch_bounds__(256) void k_vc_count(int64_t N, int nt, const int32_t* __restrict__ mapped,
                                                  const int32_t* __restrict__ P, const int32_t* __restrict__ present,
                                                  int32_t* __restrict__ top, int32_t* __restrict__ top_votes,
                                                  int32_t* __restrict__ own_votes, int32_t* __restrict__ top_flag,
                                                  unsigned long long* __restrict__ hist,
                                                  unsigned long long* __restrict__ ctr, int32_t* __restrict__ slow_list) {
    __shared__ unsigned int s_h[SC_MAX_REPLICAS + 1];
    for (int i = threadIdx.x; i <= nt; i += blockDim.x) s_h[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = t < N;
    const int32_t p = in ? P[t] : 0;
    const int32_t* col = mapped + (in ? t : 0);
    int32_t id[VT_D];
    int32_t vo[VT_D];
#pragma unroll
    for (int d = 0; d < VT_D; ++d) { id[d] = -1; vo[d] = 0; }
    bool ov = false, bad = false;
    if (in) {
        for (int r = 0; r < nt; r += 4) {
            int32_t x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = col[(int64_t)(r + j < nt ? r + j : nt - 1) * N];   // four rows in flight
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (r + j >= nt) continue;
                const int32_t y = x[j];
                if ((uint32_t)y >= (uint64_t)N || !present[y]) { bad = true; continue; }
                if (ov) continue;
                bool f = false;
#pragma unroll
                for (int d = 0; d < VT_D; ++d) {
                    const bool h = id[d] == y;
                    vo[d] += h ? 1 : 0;
                    f |= h;
                }
                if (!f) {
                    bool placed = false;
#pragma unroll
                    for (int d = 0; d < VT_D; ++d)
                        if (!placed && id[d] < 0) { id[d] = y; vo[d] = 1; placed = true; }
                    if (!placed) ov = true;
                }
            }
        }
    }
    int own = 0, mx = 0;
#pragma unroll
    for (int d = 0; d < VT_D; ++d) {
        own += id[d] == p ? vo[d] : 0;
        mx = vo[d] > mx ? vo[d] : mx;
    }
    int leaders = 0;
    int32_t tid = INT_MAX;
#pragma unroll
    for (int d = 0; d < VT_D; ++d)
        if (id[d] >= 0 && vo[d] == mx) { ++leaders; tid = id[d] < tid ? id[d] : tid; }
    if (own == mx) tid = p;   // P(v) among the leaders (or no valid vote at all)
    const bool fin = in && !ov;
    if (fin) {
        top[t] = tid; top_votes[t] = mx; own_votes[t] = own;
        top_flag[tid] = 1;
    }
    if (in && ov) slow_list[atomicAdd(&ctr[VT_SLOW], 1ull)] = (int32_t)t;
    const unsigned long long m_moved = __ballot(fin && tid != p), m_una = __ballot(fin && own == nt),
                             m_tied = __ballot(fin && leaders > 1), m_bad = __ballot(bad), act = __ballot(fin);
    if (lane == 0) {
        if (m_moved) atomicAdd(&ctr[VT_MOVED], (unsigned long long)__popcll(m_moved));
        if (m_una) atomicAdd(&ctr[VT_UNANIMOUS], (unsigned long long)__popcll(m_una));
        if (m_tied) atomicAdd(&ctr[VT_TIED], (unsigned long long)__popcll(m_tied));
        if (m_bad) atomicAdd(&ctr[VT_BAD], (unsigned long long)__popcll(m_bad));
    }
    if (act) wave_bin_add(s_h, fin, own, act, lane);   // wave-uniform
    __syncthreads();
    for (int i = threadIdx.x; i <= nt; i += blockDim.x)
        if (s_h[i]) atomicAdd(&hist[i], (unsigned long long)s_h[i]);
}
// The nodes of slow_list, one wave (one block) each: the node's nt values sorted in LDS (M = the
// power of two at or above nt, padded with INT_MAX), then every run's first element walks its run.
// A candidate is (votes, is P(v), 0xffffffff - id) packed in 64 bits: its maximum is the vote rule.
__global__ __launch_bounds__(64) void k_vc_slow(int64_t N, int nt, int M, const int32_t* __restrict__ mapped,
                                                const int32_t* __restrict__ P, const int32_t* __restrict__ slow_list,
                                                int32_t* __restrict__ top, int32_t* __restrict__ top_votes,
                                                int32_t* __restrict__ own_votes, int32_t* __restrict__ top_flag,
                                                unsigned long long* __restrict__ hist,
                                                unsigned long long* __restrict__ ctr) {
    __shared__ int32_t a[SC_MAX_REPLICAS];
    const int lane = threadIdx.x;
    const int64_t ns = (int64_t)ctr[VT_SLOW];
    for (int64_t i = blockIdx.x; i < ns; i += gridDim.x) {
        const int32_t t = slow_list[i], p = P[t];
        for (int j = lane; j < M; j += 64) a[j] = j < nt ? mapped[(int64_t)j * N + t] : INT_MAX;
        __syncthreads();
        for (int k2 = 2; k2 <= M; k2 <<= 1)
            for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
                for (int x = lane; x < M; x += 64) {
                    const int y = x ^ j2;
                    if (y > x) {
                        const int32_t ax = a[x], ay = a[y];
                        if ((ax > ay) == ((x & k2) == 0)) { a[x] = ay; a[y] = ax; }
                    }
                }
                __syncthreads();
            }
        unsigned long long cand = 0;
        int lmax = 0, lcnt = 0, own = 0;
        for (int j = lane; j < nt; j += 64) {
            const int32_t y = a[j];
            if (j > 0 && a[j - 1] == y) continue;
            int e = j + 1;
            while (e < nt && a[e] == y) ++e;
            const int v = e - j;
            const unsigned long long cd = ((unsigned long long)v << 33) | ((unsigned long long)(y == p) << 32) |
                                          (0xffffffffull - (unsigned long long)(uint32_t)y);
            cand = cd > cand ? cd : cand;
            if (v > lmax) { lmax = v; lcnt = 1; }
            else if (v == lmax) ++lcnt;
            if (y == p) own = v;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(cand, o);
            cand = other > cand ? other : cand;
        }
        const int mx = (int)(cand >> 33);
        const unsigned long long leaders = sc_wave_sum((unsigned long long)(lmax == mx ? lcnt : 0));
        own = (int)sc_wave_sum((unsigned long long)own);
        if (lane == 0) {
            const int32_t tid = (int32_t)(0xffffffffu - (uint32_t)cand);
            top[t] = tid; top_votes[t] = mx; own_votes[t] = own;
            if ((uint32_t)tid < (uint64_t)N) top_flag[tid] = 1;
            atomicAdd(&hist[own], 1ull);
            if (tid != p) atomicAdd(&ctr[VT_MOVED], 1ull);
            if (leaders > 1) atomicAdd(&ctr[VT_TIED], 1ull);
        }
        __syncthreads();
    }
}

// in: P on the device in node order; mapped: device int32[nt][N].  Queues the work into the
// context's buffers (vt_top / vt_tv / vt_own, vt_hist, vt_ctr): vote_finish hands them out.
static void vote_count_run(Ctx& c, const int32_t* in, const int32_t* mapped, int nt, VoteMarks& ph) {
    const int64_t N = c.N;
    ph.mark();
    int32_t* top = ensure<int32_t>(c.vt_top, N);
    int32_t* tv = ensure<int32_t>(c.vt_tv, N);
    int32_t* own = ensure<int32_t>(c.vt_own, N);
    int32_t* flag = ensure<int32_t>(c.vt_flag, 2 * N);   // ids of P, then ids of top
    int32_t* slow = ensure<int32_t>(c.vt_slow, N);
    unsigned long long* hist = (unsigned long long*)ensure<uint64_t>(c.vt_hist, nt + 1);
    unsigned long long* ctr = (unsigned long long*)ensure<uint64_t>(c.vt_ctr, VT_CTRS);
    FC_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t) * 2 * (size_t)N, c.stream));
    FC_HIP(hipMemsetAsync(hist, 0, sizeof(uint64_t) * (size_t)(nt + 1), c.stream));
    FC_HIP(hipMemsetAsync(ctr, 0, sizeof(uint64_t) * VT_NCOMM, c.stream));   // the map's counter stays
    k_vc_present<<<nblk(N), TB, 0, c.stream>>>(N, in, flag);
    k_vc_count<<<nblk(N), TB, 0, c.stream>>>(N, nt, mapped, in, flag, top, tv, own, flag + N, hist, ctr, slow);
    int M = 2;
    while (M < nt) M <<= 1;
    if (nt > VT_D)   // fewer replicas than list slots: no node can overflow
        k_vc_slow<<<(unsigned)std::min<int64_t>(N, 4096), 64, 0, c.stream>>>(N, nt, M, mapped, in, slow, top, tv, own,
                                                                              flag + N, hist, ctr);
    k_vc_flags<<<std::min<unsigned>(nblk(N), 1024u), TB, 0, c.stream>>>(N, flag, ctr + VT_K);
    k_vc_flags<<<std::min<unsigned>(nblk(N), 1024u), TB, 0, c.stream>>>(N, flag + N, ctr + VT_KVOTED);
    ph.mark(3);   // count
}
// Synchronises, checks and writes the caller's outputs (nothing on error).  counted: vote_count_run ran.
static void vote_finish(Ctx& c, bool counted, int nt, int64_t k_map, int64_t slow_members, int32_t* dev_top,
                        int32_t* dev_tv, int32_t* dev_own, int64_t* own_hist, fc_vote_info* info, VoteMarks& ph) {
    const int64_t N = c.N;
    unsigned long long h[VT_CTRS] = {};
    FC_HIP(hipMemcpyAsync(h, c.vt_ctr.p, sizeof(h), hipMemcpyDeviceToHost, c.stream));
    sync(c);
    ph.collect();
    fc_vote_info out{};
    out.n_total = nt;
    if (k_map >= 0) { out.k = k_map; out.mapped_communities = (int64_t)h[VT_NCOMM]; out.slow_members = slow_members; }
    if (counted) {
        FC_REQUIRE(h[VT_BAD] == 0, FC_EINVAL,
                   "dev_mapped holds " + std::to_string(h[VT_BAD]) + " node(s) with a value that is no cluster id of labels");
        out.k = (int64_t)h[VT_K]; out.k_voted = (int64_t)h[VT_KVOTED]; out.moved = (int64_t)h[VT_MOVED];
        out.unanimous = (int64_t)h[VT_UNANIMOUS]; out.tied = (int64_t)h[VT_TIED]; out.slow_nodes = (int64_t)h[VT_SLOW];
        const size_t nb = sizeof(int32_t) * (size_t)N;
        if (dev_top) FC_HIP(hipMemcpyAsync(dev_top, c.vt_top.p, nb, hipMemcpyDeviceToDevice, c.stream));
        if (dev_tv) FC_HIP(hipMemcpyAsync(dev_tv, c.vt_tv.p, nb, hipMemcpyDeviceToDevice, c.stream));
        if (dev_own) FC_HIP(hipMemcpyAsync(dev_own, c.vt_own.p, nb, hipMemcpyDeviceToDevice, c.stream));
        if (own_hist)
            FC_HIP(hipMemcpyAsync(own_hist, c.vt_hist.p, sizeof(int64_t) * (size_t)(nt + 1), hipMemcpyDeviceToHost, c.stream));
        sync(c);
    }
    if (info) *info = out;
}

// labels: host int32[N] in node order, ids in [0, N), validated by the caller.  All synchronise.
void vote_map(Ctx& c, const int32_t* labels, int32_t* dev_mapped, fc_vote_info* info) {
    score_require(c);
    VoteMarks ph(c);
    ScLabT lt(c);
    int64_t k = 0;
    const int64_t slow = vote_map_run(c, partition_upload(c, labels), dev_mapped, &k, ph);
    vote_finish(c, false, c.n_r, k, slow, nullptr, nullptr, nullptr, nullptr, info, ph);
}
void vote_count(Ctx& c, const int32_t* labels, const int32_t* dev_mapped, int n_total, int32_t* dev_top, int32_t* dev_tv,
                int32_t* dev_own, int64_t* own_hist, fc_vote_info* info) {
    VoteMarks ph(c);
    vote_count_run(c, partition_upload(c, labels), dev_mapped, n_total, ph);
    vote_finish(c, true, n_total, -1, 0, dev_top, dev_tv, dev_own, own_hist, info, ph);
}
void vote(Ctx& c, const int32_t* labels, int32_t* dev_top, int32_t* dev_tv, int32_t* dev_own, int64_t* own_hist,
          fc_vote_info* info) {
    score_require(c);
    VoteMarks ph(c);
    ScLabT lt(c);
    int32_t* mapped = ensure<int32_t>(c.vt_mapped, (size_t)c.n_r * c.N);
    const int32_t* in = partition_upload(c, labels);
    int64_t k = 0;
    const int64_t slow = vote_map_run(c, in, mapped, &k, ph);
    vote_count_run(c, in, mapped, c.n_r, ph);
    vote_finish(c, true, c.n_r, k, slow, dev_top, dev_tv, dev_own, own_hist, info, ph);
}

}  // namespace fc
