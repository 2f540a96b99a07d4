// cluster.h -- cluster and item consensus of a given partition P over the local labelings
// (fc_cluster_consensus): per cluster k of P the sum of the consensus-matrix entries over its
// ordered member pairs, per node v the sum over the members of v's own cluster, both with the
// diagonal and both without the matrix.  With C_r[k][d] = the members of cluster k that replica r
// labels d,
//     pairs[k] = sum_r sum_d C_r[k][d]^2        item[v] = sum_r C_r[P(v)][lab_r(v)]
// exact integers, sums over replicas (ranks add theirs), O(N n_r) work.
// Included at the end of consensus.hip after coassoc.h (score.h's segments, cell-kernel pieces,
// fallback plan and ScLabT, analysis.h's PhaseMarks and the hipcub wrappers are in scope).
//
// The count kernel keeps the per-cluster structure: one wave per cluster of P, LANES ARE REPLICAS,
// each lane building the (label, count) list of its replica in SC_D registers (sc_list_walk).  At
// the segment's end the lists are the rows C_r[k][.]: the wave adds their squares to pairs[k], then
// streams the members a second time and adds each lane's count of its own label for that member
// (sc_gather4, sc_list_count) to item[v].  A lane with a ninth label, and every lane of a cluster
// longer than the length cap, is left to the exact fallback: score.h's entries, here emitted one
// thread per key and sorted, run-length encoded and handed to the caller's kernel chunk by chunk
// (cell_chunks, which vote.h, affinity.h, merge.h and match.h run as well), each key of this call
// carrying its member's vertex through the sort.  Every contribution is an int64 atomicAdd of an
// integer, so neither the order nor the split over banks and paths shows in the result.
#pragma once
#include <algorithm>
#include <vector>

namespace fc {

// out[t] = item[sigma[t]]: sums by internal vertex -> node order
__global__ void k_cc_item_out(int64_t N, const unsigned long long* __restrict__ item, const int32_t* __restrict__ sigma,
                              int64_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N) out[t] = (int64_t)item[sigma[t]];
}
// *total += sum of x[0 .. n)
__global__ __launch_bounds__(256) void k_cc_total(int64_t n, const unsigned long long* __restrict__ x,
                                                  unsigned long long* __restrict__ total) {
    unsigned long long s = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) s += x[i];
    s = sc_wave_sum(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
}

// ------------------------------------------------------------------ count kernel (lanes are replicas)
// lcap: longest cluster one wave streams (score_list_cap with sum32).  ovf[bank * k + cluster]: the
// lanes left to the fallback.  pairs[cluster] and item[internal vertex] are zeroed by the caller.
__global__ __launch_bounds__(256) void k_cc_count(int64_t k, const int32_t* __restrict__ seg,
                                                  const int32_t* __restrict__ sval,
                                                  const int32_t* __restrict__ labT, int ldT, int n_r, int lcap,
                                                  unsigned long long* __restrict__ ovf,
                                                  unsigned long long* __restrict__ pairs,
                                                  unsigned long long* __restrict__ item) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int bank = blockIdx.y;
    const int r = bank * 64 + lane;
    const bool act = r < n_r;
    const int32_t* col = labT + (act ? r : 0);
    for (int64_t cc = (int64_t)blockIdx.x * 4 + w; cc < k; cc += (int64_t)gridDim.x * 4) {
        const int32_t s0 = seg[cc], s1 = seg[cc + 1], len = s1 - s0;
        bool ov = act && len > lcap;
        if (len <= lcap) {   // wave-uniform
            int32_t key[SC_D];
            int32_t cnt[SC_D];
            // pass 1: the list of (label, count) of this lane's replica over the cluster's members
            sc_list_walk(key, cnt, s0, s1, sval, col, ldT, act, ov, lane);
            const bool live = act && !ov;
            unsigned long long sq = 0;
            if (live) {
#pragma unroll
                for (int d = 0; d < SC_D; ++d) sq += (unsigned long long)cnt[d] * (unsigned long long)cnt[d];
            }
            sq = sc_wave_sum(sq);
            if (lane == 0 && sq) atomicAdd(&pairs[cc], sq);
            // pass 2: the same members against the lists still in registers
            if (sq) {   // wave-uniform: some lane is live
                for (int32_t b0 = s0; b0 < s1; b0 += 64) {
                    const int nb = s1 - b0 < 64 ? s1 - b0 : 64;
                    const int32_t myv = b0 + lane < s1 ? sval[b0 + lane] : 0;
                    for (int t = 0; t < nb; t += 4) {
                        int32_t l[4];
                        sc_gather4(l, myv, t, nb, col, ldT, live);
                        unsigned n[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int32_t x = sc_list_count(key, cnt, l[j]);
                            n[j] = live && t + j < nb ? (unsigned)x : 0u;
                        }
                        const unsigned tot = sc_sum4(n, lane);
                        const int tj = t + (lane >> 4);   // the member this lane's group of 16 summed
                        const int32_t v = __shfl(myv, tj < nb ? tj : nb - 1);
                        if ((lane & 15) == 0 && tj < nb && tot) atomicAdd(&item[v], (unsigned long long)tot);
                    }
                }
            }
        }
        const unsigned long long mask = __ballot(ov);
        if (lane == 0) ovf[(int64_t)bank * k + cc] = mask;
    }
}

// ------------------------------------------------------------------ exact fallback, with member identity
// score.h's entries, prefix sums E and chunk windows (score_fallback_plan); a key
// (entry * 64 + lane) << 32 | label now travels with its member's vertex as the sort value.
// One thread per key position p of the chunk [lo, lo + n): the key lo + p lies in entry i
// (E[i] <= lo + p < E[i + 1]), item q of it (its q-th set lane) and is member t of the cluster.  The
// chunk owns the items that start in [lo, hi); a position whose item starts before lo (the
// previous chunk emitted it) or at or past hi (the next one will) keeps its sentinel.  k_sc_emit's
// one wave per entry would walk a cluster of a million members alone; here every key is its own
// thread, whatever the shape of the partition.
__global__ __launch_bounds__(256) void k_cc_emit(int64_t nbk, int64_t k, const int64_t* __restrict__ E,
                                                 const unsigned long long* __restrict__ ovf,
                                                 const int32_t* __restrict__ seg, const int32_t* __restrict__ sval,
                                                 const int32_t* __restrict__ labT, int ldT, int64_t lo, int64_t hi,
                                                 int64_t n, unsigned long long* __restrict__ keys,
                                                 int32_t* __restrict__ vals) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = lo + p;   // < E[nbk]: n <= T - lo
        int64_t a = 0, b = nbk - 1;   // the last entry with E[i] <= g (empty entries repeat E: the last is the nonempty one)
        while (a < b) {
            const int64_t mid = (a + b + 1) >> 1;
            if (E[mid] <= g) a = mid;
            else b = mid - 1;
        }
        const int64_t i = a, bank = i / k, cc = i % k;
        const int32_t s0 = seg[cc], len = seg[cc + 1] - s0;
        const int64_t off = g - E[i];
        const int q = (int)(off / len);
        const int32_t t = (int32_t)(off - (int64_t)q * len);
        const int64_t start = g - t;
        if (start < lo || start >= hi) continue;
        unsigned long long m = ovf[i];
        for (int z = 0; z < q; ++z) m &= m - 1ull;   // drop the q lowest set lanes
        const int lane = __ffsll((long long)m) - 1;   // a set bit is a lane below n_r
        const int32_t v = sval[s0 + t];
        keys[p] = (((unsigned long long)i * 64ull + (unsigned long long)lane) << 32) |
                  (unsigned long long)(uint32_t)labT[(int64_t)v * ldT + bank * 64 + lane];
        vals[p] = v;
    }
}
// One run = one contingency cell of c members; S = the exclusive prefix sums of the run lengths
// (S[*nruns] = n).  Sorted element j finds its run q (S[q] <= j < S[q + 1]) and adds c to its
// member's item sum; the run's first element adds c^2 to the cluster's pair sum.
__global__ __launch_bounds__(256) void k_cc_fold(int64_t n, const int32_t* __restrict__ nruns,
                                                 const unsigned long long* __restrict__ ukeys,
                                                 const int32_t* __restrict__ counts, const int32_t* __restrict__ S,
                                                 const int32_t* __restrict__ svals, int64_t k,
                                                 unsigned long long* __restrict__ pairs,
                                                 unsigned long long* __restrict__ item) {
    const int32_t nr = *nruns;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        int32_t a = 0, b = nr - 1;   // the last q with S[q] <= j
        while (a < b) {
            const int32_t mid = (a + b + 1) >> 1;
            if ((int64_t)S[mid] <= j) a = mid;
            else b = mid - 1;
        }
        const unsigned long long key = ukeys[a];
        if (key == ~0ull) continue;   // the chunk's padding
        const unsigned long long c = (unsigned long long)counts[a];
        atomicAdd(&item[svals[j]], c);
        if ((int64_t)S[a] == j) atomicAdd(&pairs[(int64_t)(((key >> 32) >> 6) % (unsigned long long)k)], c * c);
    }
}
namespace {
// one chunk of the fallback, sorted and run-length encoded: the n keys of the chunk make *nruns runs,
// run j = one contingency cell (ukeys[j], its counts[j] members), the padding's run last.  With the
// members kept: svals[p] = the vertex of sorted key p, S = the exclusive prefix sums of counts.
struct CellChunk {
    int64_t n;
    const unsigned long long* ukeys;
    const int32_t *counts, *nruns, *svals, *S;
};
}  // namespace
// The chunk loop of every cell call's fallback after score_fallback_plan: k_cc_emit's keys of the
// replica columns labT / ldT, the sort and the run lengths, then fold(chunk) launches the call's own
// fold or lookup kernel on the stream.  MEMBERS: each key takes its member's vertex through the
// sort and the run lengths are scanned (cluster consensus alone adds per member).
template <bool MEMBERS, class Fold>
static void cell_chunks(Ctx& c, const ScSeg& s, const ScPlan& p, const unsigned long long* ovf, const int32_t* labT, int ldT,
                        Fold fold) {
    const ScChunkBufs b = score_chunk_buffers(c);
    int32_t* v1 = ensure<int32_t>(c.cc_fv1, b.cap);   // k_cc_emit writes them either way
    int32_t* v2 = MEMBERS ? ensure<int32_t>(c.cc_fv2, b.cap) : nullptr;
    int32_t* S = MEMBERS ? ensure<int32_t>(c.cc_fscan, b.cap + 1) : nullptr;
    for (int64_t lo = 0; lo < p.T; lo += b.step) {
        const int64_t hi = lo + b.step, n = std::min<int64_t>(b.cap, p.T - lo);
        FC_HIP(hipMemsetAsync(b.k1, 0xff, sizeof(uint64_t) * (size_t)n, c.stream));
        if (MEMBERS) {
            FC_HIP(hipMemsetAsync(v1, 0, sizeof(int32_t) * (size_t)n, c.stream));
            FC_HIP(hipMemsetAsync(b.rc, 0, sizeof(int32_t) * (size_t)(n + 1), c.stream));   // run lengths past the last run: 0
        }
        k_cc_emit<<<std::min<unsigned>(nblk(n), 8192u), TB, 0, c.stream>>>(p.nbk, s.k, p.E, ovf, s.seg, s.sval, labT, ldT, lo,
                                                                          hi, n, b.k1, v1);
        if (MEMBERS) sort_pairs_public(c, (const uint64_t*)b.k1, (uint64_t*)b.k2, (const int32_t*)v1, v2, n, 64);
        else sort_keys_public(c, (const uint64_t*)b.k1, (uint64_t*)b.k2, n, 64);
        run_length(c, (const unsigned long long*)b.k2, b.k1, b.rc, b.nr, n);
        if (MEMBERS) exclusive_scan(c, (const int32_t*)b.rc, S, n + 1);
        fold(CellChunk{n, b.k1, b.rc, b.nr, v2, S});
    }
}
// returns the (member, replica) pairs handled here
static int64_t cluster_fallback(Ctx& c, const ScSeg& s, int banks, const unsigned long long* ovf,
                                unsigned long long* pairs, unsigned long long* item) {
    const ScPlan p = score_fallback_plan(c, s, (int64_t)banks * s.k, ovf,
                                         "too many (cluster, replica) slots for the cluster-consensus fallback");
    if (p.T == 0) return 0;
    cell_chunks<true>(c, s, p, ovf, c.labT.as<int32_t>(), c.ldT, [&](const CellChunk& ch) {
        k_cc_fold<<<std::min<unsigned>(nblk(ch.n), 4096u), TB, 0, c.stream>>>(ch.n, ch.nruns, ch.ukeys, ch.counts, ch.S,
                                                                             ch.svals, s.k, pairs, item);
    });
    return p.T;
}

// labels: host int32[N] in node order, ids in [0, N), validated by the caller.  Synchronises.
void cluster_consensus(Ctx& c, const int32_t* labels, int32_t* ids_out, int64_t* size_out, int64_t* dev_cluster,
                       int64_t* dev_item, fc_cluster_info* info) {
    score_require(c);
    const int64_t N = c.N;
    const int banks = (c.n_r + 63) / 64;
    PhaseMarks ph(c, c.cc_ms);
    ph.clear();
    ScLabT lt(c);
    ph.mark();
    const ScSeg s = partition_segments(c, partition_upload(c, labels));
    ph.mark();   // segments
    unsigned long long* pairs = (unsigned long long*)ensure<uint64_t>(c.cc_pairs, N);
    unsigned long long* item = (unsigned long long*)ensure<uint64_t>(c.cc_item, N);
    unsigned long long* tot = (unsigned long long*)ensure<uint64_t>(c.cc_tot, 1);
    unsigned long long* ovf = (unsigned long long*)ensure<uint64_t>(c.sc_ovf, (size_t)banks * s.k + 1);
    FC_HIP(hipMemsetAsync(pairs, 0, sizeof(uint64_t) * (size_t)N, c.stream));
    FC_HIP(hipMemsetAsync(item, 0, sizeof(uint64_t) * (size_t)N, c.stream));
    FC_HIP(hipMemsetAsync(tot, 0, sizeof(uint64_t), c.stream));
    k_cc_count<<<dim3(score_count_grid(s.k), banks), TB, 0, c.stream>>>(s.k, s.seg, s.sval, c.labT.as<int32_t>(), c.ldT, c.n_r,
                                                                       score_list_cap(c, true), ovf, pairs, item);
    ph.mark();   // count
    const int64_t slow = cluster_fallback(c, s, banks, ovf, pairs, item);
    ph.mark();   // fallback
    k_cc_total<<<std::min<unsigned>(nblk(s.k), 1024u), TB, 0, c.stream>>>(s.k, pairs, tot);
    PartSummary sum;
    sum.fetch(c, s.k);
    const int64_t total = read_i64(c, (const int64_t*)tot);   // synchronises
    ph.collect();
    if (dev_cluster) FC_HIP(hipMemcpyAsync(dev_cluster, pairs, sizeof(int64_t) * (size_t)N, hipMemcpyDeviceToDevice, c.stream));
    if (dev_item) k_cc_item_out<<<nblk(N), TB, 0, c.stream>>>(N, item, c.sigma.as<int32_t>(), dev_item);
    sync(c);
    sum.finish(ids_out, size_out);
    if (info) {
        *info = fc_cluster_info{};
        info->k = s.k; info->max_size = sum.max_size; info->singletons = sum.singletons;
        info->pairs_total = total; info->slow_members = slow; info->n_r = c.n_r;
    }
}

}  // namespace fc
