// match.h -- cluster-wise Jaccard best match of a given partition P against every local labeling,
// or against one labeling handed in (fc_cluster_match): per cluster k of P and replica r the
// community d of r with the largest Jaccard index
//     J_r(k, d) = C / (s_k + t_r(d) - C),   C = C_r[k][d] = the members of k that r labels d,
//     s_k = the size of k, t_r(d) = the nodes (of all N) that r labels d,
// reported as the two integers inter = C and csize = t of that community.  Hennig's cluster-wise
// stability, recovered / dissolved counts and best-match F1 are functions of them (core.py).
// Included at the end of consensus.hip after merge.h (score.h's segments, cell-kernel pieces,
// fallback plan and ScLabT, cluster.h's cell_chunks, analysis.h's PhaseMarks are in scope).
//
// The choice is made on integers alone: two fractions C1 / U1 and C2 / U2 (U = s + t - C) are
// compared as C1 * U2 against C2 * U1 (C <= N < 2^31 and U < 2^32: the products fit 64 bits), and
// among equal fractions the larger C wins -- equal J and equal C force equal U, hence equal t, so the
// pair (inter, csize) is unique whatever the order the candidates are met in.  cm_better is the one
// place that compares; the register path, the fallback and the fallback's combine all call it.
//
// The sizes t_r(d) are one table per call in labT's layout, csz[d * ldT + r], so that a wave whose
// lanes are replicas gathers them as it gathers labels.  The match kernel is score.h's
// sc_list_walk: one wave per cluster, LANES ARE REPLICAS, each lane building the (label, count) list
// of its replica in SC_D registers; at the segment's end the lane looks up t for its labels, keeps
// the best pair and writes its own entry of the two tables (one writer per entry, no atomics).  A
// lane with a ninth label, and every lane of a cluster longer than the length cap, goes to the exact
// fallback: score.h's entries in cluster.h's cell_chunks, sorted and run-length folded; a run is one
// cell (its length is C, its label gives t) and is folded into its group's 64-bit slot
// (C << 32 | t) by a compare-and-swap loop on cm_better.  The order is a total one on the pairs, so
// the slot ends at the same maximum however the runs arrive and however the chunks cut the key stream.
#pragma once
#include <algorithm>
#include <optional>
#include <vector>

namespace fc {

// (C1, t1) beats (C2, t2) as the match of a cluster of s members; (0, 0) loses to every real cell
__device__ __forceinline__ bool cm_better(uint32_t s, uint32_t C1, uint32_t t1, uint32_t C2, uint32_t t2) {
    const unsigned long long a = (unsigned long long)C1 * (unsigned long long)(s + t2 - C2);
    const unsigned long long b = (unsigned long long)C2 * (unsigned long long)(s + t1 - C1);
    return a > b || (a == b && C1 > C2);
}

// col[sigma[t]] = in[t]: one labeling in node order as a one-column labT (ldT = 1)
__global__ void k_cm_column(int64_t N, const int32_t* __restrict__ in, const int32_t* __restrict__ sigma,
                            int32_t* __restrict__ col) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N) col[sigma[t]] = in[t];
}
// csz[d * ldT + r] = the vertices replica r labels d (csz zeroed by the caller): one pass over labT,
// a wave's adds spread over the replicas of a few rows
__global__ __launch_bounds__(256) void k_cm_sizes(int64_t N, int n_r, int ldT, const int32_t* __restrict__ labT,
                                                  int32_t* __restrict__ csz) {
    const int64_t total = N * ldT;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i % ldT);
        if (r >= n_r) continue;   // labT's padding columns are never written
        const int32_t d = labT[i];
        if ((uint32_t)d < (uint32_t)N) atomicAdd(&csz[(int64_t)d * ldT + r], 1);
    }
}

// ------------------------------------------------------------------ match kernel (lanes are replicas)
// lcap: longest cluster one wave streams (0: everything to the fallback).  ovf[bank * k + cluster]:
// the lanes left to the fallback.  Lane r writes inter[r * ldi + cluster] and csize[r * ldc + cluster].
__global__ __launch_bounds__(256) void k_cm_match(int64_t k, const int32_t* __restrict__ seg,
                                                  const int32_t* __restrict__ sval,
                                                  const int32_t* __restrict__ labT, int ldT, int n_r, int lcap,
                                                  const int32_t* __restrict__ csz,
                                                  unsigned long long* __restrict__ ovf, int32_t* __restrict__ inter,
                                                  int64_t ldi, int32_t* __restrict__ csize, int64_t ldc) {
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
            sc_list_walk(key, cnt, s0, s1, sval, col, ldT, act, ov, lane);
            if (act && !ov) {
                uint32_t t[SC_D];
#pragma unroll
                for (int d = 0; d < SC_D; ++d)   // the gathers go out together; an empty slot reads nothing
                    t[d] = key[d] >= 0 ? (uint32_t)csz[(int64_t)key[d] * ldT + r] : 0u;
                uint32_t bc = 0, bt = 0;
#pragma unroll
                for (int d = 0; d < SC_D; ++d)
                    if (key[d] >= 0 && cm_better((uint32_t)len, (uint32_t)cnt[d], t[d], bc, bt)) {
                        bc = (uint32_t)cnt[d];
                        bt = t[d];
                    }
                inter[(int64_t)r * ldi + cc] = (int32_t)bc;
                csize[(int64_t)r * ldc + cc] = (int32_t)bt;
            }
        }
        const unsigned long long mask = __ballot(ov);
        if (lane == 0) ovf[(int64_t)bank * k + cc] = mask;
    }
}

// ------------------------------------------------------------------ exact fallback
// One run of the sorted keys = one cell of c members of group g = entry * 64 + lane (the key's high
// word); best[g] = C << 32 | t of the group's best cell so far, zeroed by the caller.  An item
// (all keys of one group) lies inside one chunk, so a run is a whole cell; the groups of different
// chunks, and the runs of one group, meet in best[g] through the same compare.
__global__ __launch_bounds__(256) void k_cm_fold(const int32_t* __restrict__ nruns,
                                                 const unsigned long long* __restrict__ ukeys,
                                                 const int32_t* __restrict__ counts, int64_t k,
                                                 const int32_t* __restrict__ seg, const int32_t* __restrict__ csz,
                                                 int ldT, unsigned long long* __restrict__ best) {
    const int64_t n = *nruns;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = ukeys[j];
        if (key == ~0ull) continue;   // the chunk's padding
        const unsigned long long g = key >> 32, entry = g >> 6;
        const int64_t bank = (int64_t)(entry / (unsigned long long)k), cc = (int64_t)(entry % (unsigned long long)k);
        const uint32_t s = (uint32_t)(seg[cc + 1] - seg[cc]), C = (uint32_t)counts[j];
        const uint32_t t = (uint32_t)csz[(int64_t)(uint32_t)key * ldT + bank * 64 + (int64_t)(g & 63ull)];
        const unsigned long long mine = ((unsigned long long)C << 32) | t;
        unsigned long long cur = best[g];
        while (cm_better(s, C, t, (uint32_t)(cur >> 32), (uint32_t)cur)) {
            const unsigned long long old = atomicCAS(&best[g], cur, mine);
            if (old == cur) break;
            cur = old;
        }
    }
}
// the fallback's groups into the two tables: one thread per (entry, lane), the set lanes write
__global__ __launch_bounds__(256) void k_cm_scatter(int64_t nbk, int64_t k, const unsigned long long* __restrict__ ovf,
                                                    const unsigned long long* __restrict__ best,
                                                    int32_t* __restrict__ inter, int64_t ldi,
                                                    int32_t* __restrict__ csize, int64_t ldc) {
    const int64_t total = nbk * 64;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = g >> 6;
        const int lane = (int)(g & 63);
        if (!((ovf[i] >> lane) & 1ull)) continue;   // a set bit is a lane below n_r
        const int64_t r = (i / k) * 64 + lane, cc = i % k;
        const unsigned long long b = best[g];
        inter[r * ldi + cc] = (int32_t)(b >> 32);
        csize[r * ldc + cc] = (int32_t)(uint32_t)b;
    }
}
// tot[0] += the entries with inter == s_k == csize, tot[1] += inter, over rows x k
__global__ __launch_bounds__(256) void k_cm_total(int64_t rows, int64_t k, const int32_t* __restrict__ seg,
                                                  const int32_t* __restrict__ inter, int64_t ldi,
                                                  const int32_t* __restrict__ csize, int64_t ldc,
                                                  unsigned long long* __restrict__ tot) {
    unsigned long long perfect = 0, sum = 0;
    const int64_t total = rows * k;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / k, cc = i - r * k;
        const int32_t s = seg[cc + 1] - seg[cc], c = inter[r * ldi + cc];
        perfect += c == s && csize[r * ldc + cc] == s;
        sum += (unsigned long long)c;
    }
    perfect = sc_wave_sum(perfect);
    sum = sc_wave_sum(sum);
    if ((threadIdx.x & 63) == 0 && sum) {
        if (perfect) atomicAdd(&tot[0], perfect);
        atomicAdd(&tot[1], sum);
    }
}

namespace {
struct CmTables {
    const int32_t* labT;   // [N][ldT] by internal vertex
    int ldT, n_r;
    const int32_t* csz;    // [N][ldT] by label
    int32_t* inter;
    int64_t ldi;
    int32_t* csize;
    int64_t ldc;
};
}  // namespace

// returns the (member, replica) pairs handled here
static int64_t match_fallback(Ctx& c, const ScSeg& s, int banks, const unsigned long long* ovf, const CmTables& m) {
    const ScPlan p = score_fallback_plan(c, s, (int64_t)banks * s.k, ovf,
                                         "too many (cluster, replica) slots for the cluster-match fallback");
    if (p.T == 0) return 0;
    unsigned long long* best = (unsigned long long*)ensure<uint64_t>(c.cm_best, (size_t)p.nbk * 64);
    FC_HIP(hipMemsetAsync(best, 0, sizeof(uint64_t) * (size_t)p.nbk * 64, c.stream));
    cell_chunks<false>(c, s, p, ovf, m.labT, m.ldT, [&](const CellChunk& ch) {
        k_cm_fold<<<std::min<unsigned>(nblk(ch.n), 4096u), TB, 0, c.stream>>>(ch.nruns, ch.ukeys, ch.counts, s.k, s.seg, m.csz,
                                                                             m.ldT, best);
    });
    k_cm_scatter<<<std::min<unsigned>(nblk(p.nbk * 64), 4096u), TB, 0, c.stream>>>(p.nbk, s.k, ovf, best, m.inter, m.ldi,
                                                                                  m.csize, m.ldc);
    return p.T;
}

// labels, other: host int32[N] in node order, ids in [0, N), validated by the caller; other null:
// the local labelings (the caller checked that there are some).  Synchronises.
void cluster_match(Ctx& c, const int32_t* labels, const int32_t* other, int64_t ld, int32_t* ids_out, int64_t* size_out,
                   int32_t* dev_inter, int32_t* dev_csize, fc_match_info* info) {
    const int64_t N = c.N;
    PhaseMarks ph(c, c.cm_ms);
    ph.clear();
    std::optional<ScLabT> lt;   // the labelings' labT; with `other` the labelings are not looked at
    if (!other) lt.emplace(c);
    ph.mark();
    const ScSeg s = partition_segments(c, partition_upload(c, labels));   // synchronises: st_lab is free again
    ph.mark();   // segments
    if ((dev_inter || dev_csize) && ld < s.k) {
        if (info) info->k = s.k;
        FC_REQUIRE(false, FC_EINVAL,
                   "ld = " + std::to_string(ld) + " is below the number of clusters, " + std::to_string(s.k));
    }
    CmTables m{};
    if (other) {
        const int32_t* in = partition_upload(c, other);
        int32_t* col = ensure<int32_t>(c.cm_col, N);
        k_cm_column<<<nblk(N), TB, 0, c.stream>>>(N, in, c.sigma.as<int32_t>(), col);
        m.labT = col; m.ldT = 1; m.n_r = 1;
    } else {
        m.labT = c.labT.as<int32_t>(); m.ldT = c.ldT; m.n_r = c.n_r;
    }
    const int rows = m.n_r, banks = (rows + 63) / 64;
    int32_t* csz = ensure<int32_t>(c.cm_csz, (size_t)N * m.ldT);
    FC_HIP(hipMemsetAsync(csz, 0, sizeof(int32_t) * (size_t)N * m.ldT, c.stream));
    k_cm_sizes<<<std::min<unsigned>(nblk(N * m.ldT), 8192u), TB, 0, c.stream>>>(N, m.n_r, m.ldT, m.labT, csz);
    m.csz = csz;
    ph.mark();   // sizes
    m.inter = dev_inter ? dev_inter : ensure<int32_t>(c.cm_inter, (size_t)rows * s.k);
    m.csize = dev_csize ? dev_csize : ensure<int32_t>(c.cm_csize, (size_t)rows * s.k);
    m.ldi = dev_inter ? ld : s.k;
    m.ldc = dev_csize ? ld : s.k;
    unsigned long long* tot = (unsigned long long*)ensure<uint64_t>(c.cm_tot, 2);
    unsigned long long* ovf = (unsigned long long*)ensure<uint64_t>(c.sc_ovf, (size_t)banks * s.k + 1);
    FC_HIP(hipMemsetAsync(tot, 0, 2 * sizeof(uint64_t), c.stream));
    k_cm_match<<<dim3(score_count_grid(s.k), banks), TB, 0, c.stream>>>(s.k, s.seg, s.sval, m.labT, m.ldT, m.n_r,
                                                                       score_list_cap(c, false), m.csz, ovf, m.inter,
                                                                       m.ldi, m.csize, m.ldc);
    ph.mark();   // match
    const int64_t slow = match_fallback(c, s, banks, ovf, m);
    ph.mark();   // fallback
    k_cm_total<<<std::min<unsigned>(nblk((int64_t)rows * s.k), 2048u), TB, 0, c.stream>>>(rows, s.k, s.seg, m.inter, m.ldi,
                                                                                         m.csize, m.ldc, tot);
    PartSummary sum;
    unsigned long long htot[2];
    sum.fetch(c, s.k);
    FC_HIP(hipMemcpyAsync(htot, tot, sizeof(htot), hipMemcpyDeviceToHost, c.stream));
    sync(c);
    ph.collect();
    sum.finish(ids_out, size_out);
    if (info) {
        *info = fc_match_info{};
        info->k = s.k; info->max_size = sum.max_size; info->singletons = sum.singletons;
        info->perfect = (int64_t)htot[0]; info->inter_total = (int64_t)htot[1];
        info->slow_members = slow; info->n_r = rows;
    }
}

}  // namespace fc
