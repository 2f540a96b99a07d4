// score.h -- partition scoring over the local labelings (fc_score_partitions / fc_score_pairs):
// community sizes, entropy and modularity per replica, contingency sums (NMI / ARI) per pair.
// Included at the end of consensus.hip (its hipcub wrappers and launch helpers are in scope).
//
// One "row" a at a time (a local replica or the reference labeling): its vertices sorted by
// label give the communities of a as segments.  The pair kernel then takes one community per
// wave and streams its members; LANES ARE REPLICAS: for each member the wave reads that
// vertex's labT row (one coalesced 256-byte load for 64 replicas), and lane b keeps the distinct
// b-labels of this community with their counts in SC_D registers.  At the segment's end lane b
// adds sum n^2, sum n ln n and the cell count to pair (a, b): every pair of row a from one pass
// over labT.  A lane that meets more than SC_D labels in a community, and every lane of a
// community longer than the length cap, is left to the exact fallback: its (community, lane)
// members become 64-bit keys (slot << 32 | b-label), radix-sorted and run-length folded in
// chunks of a fixed key budget.  Both paths give the same integers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace fc {

static constexpr int SC_D = 8;            // register-resident distinct labels per lane and community
static constexpr int SC_GRID = 2048;      // pair / edge kernels: blocks of 4 waves (8 waves per SIMD on 256 CUs)
static constexpr int SC_MAX_REPLICAS = 2048;   // the fold kernel keeps 24 bytes of LDS per lane

template <class K>
static void run_length(Ctx& c, const K* in, K* uniq, int32_t* counts, int32_t* nruns, int64_t n) {
    size_t tmp = 0;
    FC_HIP(hipcub::DeviceRunLengthEncode::Encode(nullptr, tmp, in, uniq, counts, nruns, (int)n, c.stream));
    c.sort_tmp.ensure(tmp);
    FC_HIP(hipcub::DeviceRunLengthEncode::Encode(c.sort_tmp.p, tmp, in, uniq, counts, nruns, (int)n, c.stream));
}

// ------------------------------------------------------------------ a labeling handed in
// row[tpos[t]] = in[t]: a labeling in node order as a label row in slot order
__global__ void k_cc_row_slots(int64_t N, const int32_t* __restrict__ in, const int32_t* __restrict__ tpos,
                               int32_t* __restrict__ row) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N) row[tpos[t]] = in[t];
}
// labels: host int32[N] in node order -> the context's staging row on the device
static const int32_t* partition_upload(Ctx& c, const int32_t* labels) {
    int32_t* in = ensure<int32_t>(c.st_lab, c.N + 1);
    FC_HIP(hipMemcpyAsync(in, labels, 4 * (size_t)c.N, hipMemcpyHostToDevice, c.stream));
    return in;
}
void score_set_reference(Ctx& c, const int32_t* labels) {
    c.sc_ref_set = false;
    if (!labels) return;
    const int64_t N = c.N;
    const int32_t* in = partition_upload(c, labels);
    int32_t* ref = ensure<int32_t>(c.sc_ref, N);
    k_cc_row_slots<<<nblk(N), TB, 0, c.stream>>>(N, in, c.tpos.as<int32_t>(), ref);
    sync(c);
    c.sc_ref_set = true;
}

// ------------------------------------------------------------------ segments of one row
namespace {
struct ScSeg {
    int64_t k;             // communities
    const int32_t* seg;    // [k + 1] first sorted position of each community
    const int32_t* sval;   // [N] internal vertices sorted by label
};
struct ScStats {
    int64_t k = 0, max_size = 0, sum_sq = 0;
    double s_log = 0.0;
    unsigned __int128 tot_sq = 0;
};
}  // namespace

// row: a label row in slot order, labels in [0, N) (a local replica, the reference, or cluster.h's
// partition).  sinv gives each slot's vertex, so the sort reads both in place; one row's buffers
// serve the next row.
static ScSeg score_segments(Ctx& c, const int32_t* row) {
    const int64_t N = c.N;
    uint32_t* k2 = ensure<uint32_t>(c.sc_key, N);
    int32_t* v2 = ensure<int32_t>(c.sc_val, N);
    sort_pairs_public(c, (const uint32_t*)row, k2, (const int32_t*)c.sinv.as<int32_t>(), v2, N, c.key_bits);
    uint32_t* ul = ensure<uint32_t>(c.sc_ulab, N);
    int32_t* cnt = ensure<int32_t>(c.sc_cnt, N + 1);
    int32_t* nr = ensure<int32_t>(c.sc_nruns, 4);
    run_length(c, (const uint32_t*)k2, ul, cnt, nr, N);
    FC_HIP(hipMemcpyAsync(c.hpin, nr, sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
    sync(c);
    const int64_t k = *(const int32_t*)c.hpin.p;
    int32_t* seg = ensure<int32_t>(c.sc_seg, N + 2);
    exclusive_scan(c, (const int32_t*)cnt, seg, k + 1);   // seg[k] = N whatever cnt[k] holds
    return ScSeg{k, seg, v2};
}
// idx: a local replica, or FC_SCORE_REF
static ScSeg score_segments(Ctx& c, int idx) {
    return score_segments(c, idx < 0 ? c.sc_ref.as<int32_t>() : c.lab.as<int32_t>() + (int64_t)idx * c.N);
}
// in: a partition P on the device in node order (partition_upload's, or the caller's own).
// Synchronises; sc_ulab / sc_cnt hold P's ascending ids and their sizes until the next row.
static ScSeg partition_segments(Ctx& c, const int32_t* in) {
    int32_t* row = ensure<int32_t>(c.cc_row, c.N);
    k_cc_row_slots<<<nblk(c.N), TB, 0, c.stream>>>(c.N, in, c.tpos.as<int32_t>(), row);
    return score_segments(c, (const int32_t*)row);
}
namespace {
// ids, sizes, largest size and singletons of partition_segments' clusters, for the calls that report them
struct PartSummary {
    std::vector<int32_t> cnt, id;
    int64_t max_size = 0, singletons = 0;
    // queues the two copies; the caller synchronises before finish()
    void fetch(Ctx& c, int64_t k) {
        cnt.resize((size_t)k);
        id.resize((size_t)k);
        FC_HIP(hipMemcpyAsync(cnt.data(), c.sc_cnt.as<int32_t>(), 4 * (size_t)k, hipMemcpyDeviceToHost, c.stream));
        FC_HIP(hipMemcpyAsync(id.data(), c.sc_ulab.as<int32_t>(), 4 * (size_t)k, hipMemcpyDeviceToHost, c.stream));
    }
    void finish(int32_t* ids_out, int64_t* size_out) {
        for (size_t i = 0; i < cnt.size(); ++i) {
            max_size = std::max<int64_t>(max_size, cnt[i]);
            singletons += cnt[i] == 1;
            if (ids_out) ids_out[i] = id[i];
            if (size_out) size_out[i] = cnt[i];
        }
    }
};
}  // namespace

// Per block: sum size^2, max size, sum size ln size and (TOT) the 128-bit sum of (community
// degree)^2, the community degree from the prefix sums P of kdeg in sorted order.
// partial[block] = {sum_sq, max, s_log bits, tot lo, tot hi}; the host adds the blocks in order.
template <bool TOT>
__global__ __launch_bounds__(256) void k_sc_part_stats(int64_t k, const int32_t* __restrict__ seg,
                                                       const int64_t* __restrict__ P,
                                                       unsigned long long* __restrict__ partial) {
    __shared__ unsigned long long s_sq[256], s_mx[256], s_lo[256], s_hi[256];
    __shared__ double s_lg[256];
    const int64_t cc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int t = threadIdx.x;
    unsigned long long sq = 0, mx = 0, lo = 0, hi = 0;
    double lg = 0.0;
    if (cc < k) {
        const int32_t a = seg[cc], b = seg[cc + 1];
        const unsigned long long n = (unsigned long long)(b - a);
        sq = n * n;
        mx = n;
        if (n > 1) lg = (double)n * log((double)n);
        if (TOT) {
            const unsigned long long d = (unsigned long long)(P[b] - P[a]);
            lo = d * d;
            hi = __umul64hi(d, d);
        }
    }
    s_sq[t] = sq; s_mx[t] = mx; s_lg[t] = lg; s_lo[t] = lo; s_hi[t] = hi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            s_sq[t] += s_sq[t + o];
            s_mx[t] = s_mx[t] > s_mx[t + o] ? s_mx[t] : s_mx[t + o];
            s_lg[t] += s_lg[t + o];
            const unsigned long long l = s_lo[t] + s_lo[t + o];
            s_hi[t] += s_hi[t + o] + (l < s_lo[t] ? 1ull : 0ull);
            s_lo[t] = l;
        }
        __syncthreads();
    }
    if (t == 0) {
        unsigned long long* p = partial + (size_t)blockIdx.x * 5;
        p[0] = s_sq[0]; p[1] = s_mx[0]; p[2] = (unsigned long long)__double_as_longlong(s_lg[0]);
        p[3] = s_lo[0]; p[4] = s_hi[0];
    }
}
__global__ void k_sc_gather_kdeg(int64_t N, const int32_t* sval, const int64_t* kdeg, int64_t* kd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) kd[i] = kdeg[sval[i]];
    else if (i == N) kd[i] = 0;
}
static ScStats score_stats(Ctx& c, const ScSeg& s, const Graph* g) {
    const int64_t N = c.N;
    const int64_t* P = nullptr;
    if (g) {
        int64_t* kd = ensure<int64_t>(c.sc_kd, N + 1);
        int64_t* kp = ensure<int64_t>(c.sc_kp, N + 1);
        k_sc_gather_kdeg<<<nblk(N + 1), TB, 0, c.stream>>>(N, s.sval, g->kdeg.as<int64_t>(), kd);
        exclusive_scan(c, (const int64_t*)kd, kp, N + 1);
        P = kp;
    }
    const unsigned nb = nblk(s.k);
    unsigned long long* part = (unsigned long long*)ensure<int64_t>(c.sc_part, (size_t)nb * 5);
    if (g) k_sc_part_stats<true><<<nb, TB, 0, c.stream>>>(s.k, s.seg, P, part);
    else k_sc_part_stats<false><<<nb, TB, 0, c.stream>>>(s.k, s.seg, P, part);
    std::vector<unsigned long long> h((size_t)nb * 5);
    FC_HIP(hipMemcpyAsync(h.data(), part, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, c.stream));
    sync(c);
    ScStats st;
    st.k = s.k;
    for (unsigned b = 0; b < nb; ++b) {
        const unsigned long long* p = &h[(size_t)b * 5];
        st.sum_sq += (int64_t)p[0];
        st.max_size = std::max<int64_t>(st.max_size, (int64_t)p[1]);
        double lg;
        memcpy(&lg, &p[2], sizeof(double));
        st.s_log += lg;
        st.tot_sq += ((unsigned __int128)p[4] << 64) | p[3];
    }
    return st;
}

// ------------------------------------------------------------------ the cell kernels' shared pieces
// Six kernels build the contingency cells C_r[k][d] (the members of segment k that replica r labels
// d) the same way: one wave per segment, LANES ARE REPLICAS, lane r keeping the distinct labels of its
// replica with their counts in SC_D registers (k_sc_pairs, k_cc_count, k_vm_count, k_ia_count,
// k_mc_count, k_cm_match).  What they share is here; what each does with the finished list is its own.

// l[j] = the label this lane's replica (column col of labT) gives member t + j of a batch of nb
// members, lane i of the wave holding the batch's i-th vertex in myv; the members past the batch
// repeat its last one, a lane that is not `live` reads nothing.  Four rows in flight.
__device__ __forceinline__ void sc_gather4(int32_t (&l)[4], int32_t myv, int t, int nb, const int32_t* __restrict__ col,
                                           int ldT, bool live) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int tt = t + j < nb ? t + j : nb - 1;
        const int32_t v = __shfl(myv, tt);
        l[j] = live ? col[(int64_t)v * ldT] : 0;
    }
}
// Builds the lane's (label, count) list over the members sval[s0 .. s1) of one segment.
// Contract: every lane of the wave calls it with the same s0, s1, sval and ldT (it shuffles).  act:
// the lane has a replica (col is its column of labT; a lane without one passes any valid column and
// reads nothing).  ov on entry: the lane is already left to the fallback and only keeps the wave
// company; on exit it is set as well when the lane met a label with all SC_D slots taken.
// A lane with act && !ov on exit holds the segment's whole row C_r[k][.]: key[d] >= 0 are its labels,
// cnt[d] their counts, an unused slot is (-1, 0).  A lane with ov set holds garbage in its list: the
// walk stops updating it, and stops altogether once no lane of the wave is still building.
// The scalars come by reference on purpose: by value (noundef) k_cc_count's count phase ran 19 to 33 %
// longer on the MI355X, by reference it runs as the text written out did (profiles/cell_refactor_ab.txt).
__device__ __forceinline__ void sc_list_walk(int32_t (&key)[SC_D], int32_t (&cnt)[SC_D], const int32_t& s0,
                                             const int32_t& s1,
                                             const int32_t* __restrict__ sval, const int32_t* __restrict__ col, const int& ldT,
                                             const bool& act, bool& ov, const int& lane) {
#pragma unroll
    for (int d = 0; d < SC_D; ++d) { key[d] = -1; cnt[d] = 0; }
    for (int32_t b0 = s0; b0 < s1; b0 += 64) {
        if (!__any(act && !ov)) break;
        const int nb = s1 - b0 < 64 ? s1 - b0 : 64;
        const int32_t myv = b0 + lane < s1 ? sval[b0 + lane] : 0;
        for (int t = 0; t < nb; t += 4) {
            int32_t l[4];
            sc_gather4(l, myv, t, nb, col, ldT, act);   // before the list updates
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (t + j < nb && act && !ov) {
                    const int32_t lab = l[j];
                    bool f = false;
#pragma unroll
                    for (int d = 0; d < SC_D; ++d) {
                        const bool h = key[d] == lab;
                        cnt[d] += h ? 1 : 0;
                        f |= h;
                    }
                    if (!f) {
                        bool placed = false;
#pragma unroll
                        for (int d = 0; d < SC_D; ++d)
                            if (!placed && key[d] < 0) { key[d] = lab; cnt[d] = 1; placed = true; }
                        if (!placed) ov = true;
                    }
                }
            }
        }
    }
}
// the count of label l in a finished list (0 when the segment has no member of that label)
__device__ __forceinline__ int32_t sc_list_count(const int32_t (&key)[SC_D], const int32_t (&cnt)[SC_D], int32_t l) {
    int32_t x = 0;
#pragma unroll
    for (int d = 0; d < SC_D; ++d) x += key[d] == l ? cnt[d] : 0;
    return x;
}
__device__ __forceinline__ unsigned long long sc_wave_sum(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
// Four per-lane values -> their four wave sums in 7 shuffles: the halves of the wave trade two
// values, the quarters one, and four steps finish inside each group of 16 lanes.  The lanes with
// (lane & 15) == 0 return the sum of value lane >> 4; the others return partial sums.
__device__ __forceinline__ unsigned sc_sum4(const unsigned (&c)[4], int lane) {
    const bool hi = lane & 32, h2 = lane & 16;
    unsigned a0 = hi ? c[2] : c[0], a1 = hi ? c[3] : c[1];
    a0 += __shfl_xor(hi ? c[0] : c[2], 32);
    a1 += __shfl_xor(hi ? c[1] : c[3], 32);
    unsigned b = h2 ? a1 : a0;
    b += __shfl_xor(h2 ? a0 : a1, 16);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) b += __shfl_xor(b, o);
    return b;
}
// lcap of a cell kernel: the longest segment one wave streams, 0 (FC_SCORE_SLOW) sending everything to
// the fallback.  sum32: the kernel adds a member's counts over the wave in 32 bits (sc_sum4); a count
// is at most the segment's length, so 64 lanes of a segment of up to 2^24 members stay below 2^32.
static int score_list_cap(const Ctx& c, bool sum32) {
    return c.score_slow ? 0 : (sum32 ? std::min(c.score_lcap, 1 << 24) : c.score_lcap);
}
// grid x of a cell kernel: blocks of 4 waves over `waves` segments, grid-stride past SC_GRID
static int score_count_grid(int64_t waves) { return (int)std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, SC_GRID)); }

// ------------------------------------------------------------------ pair kernel (lanes are replicas)
// want[bank]: the lanes whose pair with this row was asked for.  lcap: longest community one
// wave streams (0: everything to the fallback).  ovf[bank * k + community]: the lanes left to
// the fallback.  Per-block partials [bank][block][lane] of sum n^2, cells, fallback members and
// sum n ln n; k_sc_pair_reduce adds the blocks in order (the sums are run-to-run identical).
__global__ __launch_bounds__(256) void k_sc_pairs(int64_t k, const int32_t* __restrict__ seg,
                                                  const int32_t* __restrict__ sval,
                                                  const int32_t* __restrict__ labT, int ldT, int n_r,
                                                  const unsigned long long* __restrict__ want, int lcap,
                                                  unsigned long long* __restrict__ ovf,
                                                  unsigned long long* __restrict__ part) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int bank = blockIdx.y;
    const int r = bank * 64 + lane;
    const bool act = r < n_r && ((want[bank] >> lane) & 1ull);
    const int32_t* col = labT + (act ? r : 0);
    unsigned long long a_sq = 0, a_cells = 0, a_slow = 0;
    double a_log = 0.0;
    for (int64_t cc = (int64_t)blockIdx.x * 4 + w; cc < k; cc += (int64_t)gridDim.x * 4) {
        const int32_t s0 = seg[cc], s1 = seg[cc + 1], len = s1 - s0;
        bool ov = act && len > lcap;
        if (len <= lcap) {   // wave-uniform
            int32_t key[SC_D];
            int32_t cnt[SC_D];
            sc_list_walk(key, cnt, s0, s1, sval, col, ldT, act, ov, lane);
            if (act && !ov) {
#pragma unroll
                for (int d = 0; d < SC_D; ++d)
                    if (key[d] >= 0) {
                        const unsigned long long n = (unsigned long long)cnt[d];
                        a_sq += n * n;
                        a_cells += 1;
                        if (n > 1) a_log += (double)n * log((double)n);
                    }
            }
        }
        if (ov) a_slow += (unsigned long long)len;
        const unsigned long long mask = __ballot(ov);
        if (lane == 0) ovf[(int64_t)bank * k + cc] = mask;
    }
    __shared__ unsigned long long s_u[3][4][64];
    __shared__ double s_d[4][64];
    s_u[0][w][lane] = a_sq; s_u[1][w][lane] = a_cells; s_u[2][w][lane] = a_slow; s_d[w][lane] = a_log;
    __syncthreads();
    if (w == 0) {
        unsigned long long* p = part + ((size_t)bank * gridDim.x + blockIdx.x) * 256 + lane;
#pragma unroll
        for (int f = 0; f < 3; ++f) p[f * 64] = s_u[f][0][lane] + s_u[f][1][lane] + s_u[f][2][lane] + s_u[f][3][lane];
        p[192] = (unsigned long long)__double_as_longlong(s_d[0][lane] + s_d[1][lane] + s_d[2][lane] + s_d[3][lane]);
    }
}
// out[f * LP + bank * 64 + lane], f = 0..3 (sum n^2, cells, fallback members, sum n ln n bits).
// One block of 16 waves per bank: wave j adds the blocks j, j + 16, ..., then the 16 sums are added
// in order (a single wave walking all blocks paid one memory latency per block: 0.7 ms a row).
__global__ __launch_bounds__(1024) void k_sc_pair_reduce(int gx, int LP, const unsigned long long* __restrict__ part,
                                                         unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_u[3][16][64];
    __shared__ double s_d[16][64];
    const int lane = threadIdx.x & 63, j = threadIdx.x >> 6, bank = blockIdx.x;
    unsigned long long u[3] = {0, 0, 0};
    double lg = 0.0;
#pragma unroll 4
    for (int b = j; b < gx; b += 16) {
        const unsigned long long* p = part + ((size_t)bank * gx + b) * 256 + lane;
        u[0] += p[0]; u[1] += p[64]; u[2] += p[128];
        lg += __longlong_as_double((long long)p[192]);
    }
    s_u[0][j][lane] = u[0]; s_u[1][j][lane] = u[1]; s_u[2][j][lane] = u[2]; s_d[j][lane] = lg;
    __syncthreads();
    if (j != 0) return;
    for (int q = 1; q < 16; ++q) {
        u[0] += s_u[0][q][lane]; u[1] += s_u[1][q][lane]; u[2] += s_u[2][q][lane];
        lg += s_d[q][lane];
    }
    const int t = bank * 64 + lane;
    out[t] = u[0]; out[LP + t] = u[1]; out[2 * LP + t] = u[2];
    out[3 * LP + t] = (unsigned long long)__double_as_longlong(lg);
}

// ------------------------------------------------------------------ exact fallback
// Entry i = bank * k + community holds popc(ovf[i]) items of `size` keys each; E = the exclusive
// prefix sums of the entries' key counts.  Item q of entry i (its q-th set lane) starts at
// E[i] + q * size.  A chunk takes the items that start in [lo, hi): their keys land at
// (start - lo + member) of a buffer pre-filled with all-ones sentinels, so no chunk needs its
// bounds on the host; an item is at most N keys, so a chunk is at most (hi - lo) + N keys.
__global__ void k_sc_ovf_keys(int64_t nbk, int64_t k, const unsigned long long* ovf, const int32_t* seg, int64_t* cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nbk) return;
    if (i == nbk) { cnt[i] = 0; return; }
    const int64_t cc = i % k;
    cnt[i] = (int64_t)__popcll(ovf[i]) * (int64_t)(seg[cc + 1] - seg[cc]);
}
// rng = {first entry ending past lo, first entry starting at or past hi}
__global__ void k_sc_chunk_range(int64_t nbk, const int64_t* E, int64_t lo, int64_t hi, int64_t* rng) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t a = 0, b = nbk;
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (E[mid + 1] > lo) b = mid;
        else a = mid + 1;
    }
    rng[0] = a;
    a = 0; b = nbk;
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (E[mid] >= hi) b = mid;
        else a = mid + 1;
    }
    rng[1] = a;
}
__global__ __launch_bounds__(256) void k_sc_emit(int64_t k, const int64_t* __restrict__ rng,
                                                 const int64_t* __restrict__ E,
                                                 const unsigned long long* __restrict__ ovf,
                                                 const int32_t* __restrict__ seg, const int32_t* __restrict__ sval,
                                                 const int32_t* __restrict__ labT, int ldT, int64_t lo, int64_t hi,
                                                 unsigned long long* __restrict__ keys) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
    const int64_t i1 = rng[1];
    for (int64_t i = rng[0] + wave; i < i1; i += nw) {
        const unsigned long long mask = ovf[i];
        if (!mask) continue;
        const int64_t bank = i / k, cc = i % k;
        const int32_t s0 = seg[cc], s1 = seg[cc + 1], len = s1 - s0;
        const bool bit = (mask >> lane) & 1ull;
        const int q = __popcll(mask & ((1ull << lane) - 1ull));
        const int64_t start = E[i] + (int64_t)q * len;
        const bool mine = bit && start >= lo && start < hi;
        if (!__any(mine)) continue;
        const int32_t* col = labT + (mine ? bank * 64 + lane : 0);   // a set bit is a lane below n_r
        const unsigned long long slot = ((unsigned long long)i * 64ull + (unsigned long long)lane) << 32;
        for (int32_t b0 = s0; b0 < s1; b0 += 64) {
            const int nb = s1 - b0 < 64 ? s1 - b0 : 64;
            const int32_t myv = b0 + lane < s1 ? sval[b0 + lane] : 0;
            for (int t = 0; t < nb; ++t) {
                const int32_t v = __shfl(myv, t);
                if (mine) keys[start - lo + (b0 - s0) + t] = slot | (unsigned long long)(uint32_t)col[(int64_t)v * ldT];
            }
        }
    }
}
// One run = one contingency cell of n members.  acc[f * LP + lane], f = 0..3 (sum n^2, cells, and
// sum n ln n in fixed point: floor(x * 2^26) and the next 26 bits): LDS per block, then one global
// atomic per touched lane and field.  A term x = n ln n >= 2 ln 2 is a whole multiple of 2^-52, so
// the two integers hold it exactly, and integer sums do not depend on the order the atomics land
// in: the same labelings give the same s_log in every run.  Up to 2^31 terms of sum < 2^36 fit.
__global__ __launch_bounds__(256) void k_sc_fold(const int32_t* __restrict__ nruns,
                                                 const unsigned long long* __restrict__ ukeys,
                                                 const int32_t* __restrict__ counts, int64_t k, int LP,
                                                 unsigned long long* __restrict__ acc) {
    extern __shared__ unsigned long long s_fold[];
    unsigned long long* s_sq = s_fold;
    unsigned long long* s_ce = s_fold + LP;
    unsigned long long* s_l1 = s_fold + 2 * LP;
    unsigned long long* s_l2 = s_fold + 3 * LP;
    for (int t = threadIdx.x; t < LP; t += blockDim.x) { s_sq[t] = 0; s_ce[t] = 0; s_l1[t] = 0; s_l2[t] = 0; }
    __syncthreads();
    const int64_t n = *nruns;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = ukeys[j];
        if (key == ~0ull) continue;   // the chunk's padding
        const unsigned long long slot = key >> 32;
        const int t = (int)((slot >> 6) / (unsigned long long)k) * 64 + (int)(slot & 63ull);
        const unsigned long long c = (unsigned long long)counts[j];
        atomicAdd(&s_sq[t], c * c);
        atomicAdd(&s_ce[t], 1ull);
        if (c > 1) {
            const double x26 = (double)c * log((double)c) * 67108864.0, f = floor(x26);
            atomicAdd(&s_l1[t], (unsigned long long)f);
            atomicAdd(&s_l2[t], (unsigned long long)((x26 - f) * 67108864.0));
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < LP; t += blockDim.x) {
        if (!s_ce[t]) continue;
        atomicAdd(&acc[t], s_sq[t]);
        atomicAdd(&acc[LP + t], s_ce[t]);
        atomicAdd(&acc[2 * LP + t], s_l1[t]);
        atomicAdd(&acc[3 * LP + t], s_l2[t]);
    }
}
namespace {
// the fallback's plan: nbk entries, E their prefix sums, T = E[nbk] keys in all
struct ScPlan {
    int64_t nbk = 0, T = 0;
    const int64_t* E = nullptr;
};
// a chunk's buffers: up to cap keys a chunk, one chunk every `step` keys of the stream; k1 takes the
// emitted keys and then the unique ones, k2 the sorted ones, rc the run lengths, *nr their number
struct ScChunkBufs {
    int64_t cap, step;
    unsigned long long *k1, *k2;
    int32_t *rc, *nr;
};
}  // namespace
// Counts the entries' keys and scans them; synchronises.  Nothing flagged: T = 0 and the caller is
// done.  too_many: the caller's message for a partition whose slots do not fit a key's high word.
static ScPlan score_fallback_plan(Ctx& c, const ScSeg& s, int64_t nbk, const unsigned long long* ovf, const char* too_many) {
    int64_t* cnt = ensure<int64_t>(c.sc_e1, nbk + 1);
    int64_t* E = ensure<int64_t>(c.sc_e2, nbk + 1);
    k_sc_ovf_keys<<<nblk(nbk + 1), TB, 0, c.stream>>>(nbk, s.k, ovf, s.seg, cnt);
    exclusive_scan(c, (const int64_t*)cnt, E, nbk + 1);
    const int64_t T = read_i64(c, E + nbk);
    FC_REQUIRE(T == 0 || nbk * 64 < ((int64_t)1 << 32), FC_ELIMIT, too_many);
    return ScPlan{nbk, T, E};
}
static ScChunkBufs score_chunk_buffers(Ctx& c) {
    ScChunkBufs b;
    b.cap = std::max<int64_t>(2 * c.N, c.score_chunk);
    b.step = b.cap - c.N;
    b.k1 = (unsigned long long*)ensure<uint64_t>(c.sc_fk1, b.cap);
    b.k2 = (unsigned long long*)ensure<uint64_t>(c.sc_fk2, b.cap);
    b.rc = ensure<int32_t>(c.sc_fcnt, b.cap + 1);
    b.nr = ensure<int32_t>(c.sc_nruns, 4);
    return b;
}
static void score_fallback(Ctx& c, const ScSeg& s, int banks, const unsigned long long* ovf, unsigned long long* acc) {
    const int LP = banks * 64;
    const ScPlan p = score_fallback_plan(c, s, (int64_t)banks * s.k, ovf,
                                         "too many (community, replica) slots for the scoring fallback");
    if (p.T == 0) return;
    FC_REQUIRE((size_t)LP * 32 <= 65536, FC_ELIMIT, "too many replicas for the scoring fallback's LDS table");
    const ScChunkBufs b = score_chunk_buffers(c);
    int64_t* rng = ensure<int64_t>(c.sc_rng, 2);
    for (int64_t lo = 0; lo < p.T; lo += b.step) {
        const int64_t hi = lo + b.step, n = std::min<int64_t>(b.cap, p.T - lo);
        FC_HIP(hipMemsetAsync(b.k1, 0xff, sizeof(uint64_t) * (size_t)n, c.stream));
        k_sc_chunk_range<<<1, 64, 0, c.stream>>>(p.nbk, p.E, lo, hi, rng);
        k_sc_emit<<<SC_GRID, TB, 0, c.stream>>>(s.k, rng, p.E, ovf, s.seg, s.sval, c.labT.as<int32_t>(), c.ldT, lo, hi, b.k1);
        sort_keys_public(c, (const uint64_t*)b.k1, (uint64_t*)b.k2, n, 64);
        run_length(c, (const unsigned long long*)b.k2, b.k1, b.rc, b.nr, n);
        k_sc_fold<<<std::min<unsigned>(nblk(n), 1024u), TB, (size_t)LP * 32, c.stream>>>(b.nr, b.k1, b.rc, s.k, LP, acc);
    }
}

namespace {
struct ScLane {
    int64_t cells = 0, sum_sq = 0, slow = 0;
    double s_log = 0.0;
};
// labT for the scoring kernels; the context's view of it (labT_valid, ldT) is put back after
struct ScLabT {
    Ctx& c;
    bool valid;
    int ldT;
    explicit ScLabT(Ctx& x) : c(x), valid(x.labT_valid), ldT(x.ldT) {
        if (!c.labT_valid) labels_transpose(c);
    }
    ~ScLabT() {
        if (!valid) { c.labT_valid = false; c.ldT = ldT; }
    }
};
}  // namespace

// every wanted lane of row s against it: out[lane] for lane < n_r
static void score_row_pairs(Ctx& c, const ScSeg& s, const std::vector<unsigned long long>& want, std::vector<ScLane>& out) {
    const int banks = (c.n_r + 63) / 64, LP = banks * 64;
    const int gx = score_count_grid(s.k);
    unsigned long long* dwant = (unsigned long long*)ensure<uint64_t>(c.sc_want, banks);
    unsigned long long* hw = (unsigned long long*)(c.hpin + 1024);
    for (int b = 0; b < banks; ++b) hw[b] = want[b];
    FC_HIP(hipMemcpyAsync(dwant, hw, sizeof(uint64_t) * banks, hipMemcpyHostToDevice, c.stream));
    unsigned long long* ovf = (unsigned long long*)ensure<uint64_t>(c.sc_ovf, (size_t)banks * s.k + 1);
    unsigned long long* part = (unsigned long long*)ensure<uint64_t>(c.sc_part2, (size_t)banks * gx * 256);
    unsigned long long* res = (unsigned long long*)ensure<uint64_t>(c.sc_res, (size_t)8 * LP);
    FC_HIP(hipMemsetAsync(res + 4 * LP, 0, sizeof(uint64_t) * 4 * LP, c.stream));
    const int lcap = score_list_cap(c, false);
    k_sc_pairs<<<dim3(gx, banks), TB, 0, c.stream>>>(s.k, s.seg, s.sval, c.labT.as<int32_t>(), c.ldT, c.n_r, dwant, lcap,
                                                     ovf, part);
    k_sc_pair_reduce<<<banks, 1024, 0, c.stream>>>(gx, LP, part, res);
    score_fallback(c, s, banks, ovf, res + 4 * LP);
    std::vector<unsigned long long> h((size_t)8 * LP);
    FC_HIP(hipMemcpyAsync(h.data(), res, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost, c.stream));
    sync(c);
    out.assign(c.n_r, ScLane{});
    for (int r = 0; r < c.n_r; ++r) {
        double l0;
        memcpy(&l0, &h[3 * LP + r], 8);
        const double l1 = (double)(ldexpl((long double)h[6 * LP + r], -26) + ldexpl((long double)h[7 * LP + r], -52));
        out[r].sum_sq = (int64_t)(h[r] + h[4 * LP + r]);
        out[r].cells = (int64_t)(h[LP + r] + h[5 * LP + r]);
        out[r].slow = (int64_t)h[2 * LP + r];
        out[r].s_log = l0 + l1;
    }
}

// ------------------------------------------------------------------ modularity edge pass
// Lanes are replicas: a wave walks edges, lane r compares its labels at u and v and keeps the
// weight sum in a register; one atomicAdd per lane and block.  UNIT: no weight loads.
template <bool UNIT>
__global__ __launch_bounds__(256) void k_sc_edges(int64_t m, const int32_t* __restrict__ eu,
                                                  const int32_t* __restrict__ ev, const int32_t* __restrict__ ew,
                                                  const int32_t* __restrict__ labT, int ldT, int n_r,
                                                  unsigned long long* __restrict__ inw) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = blockIdx.y * 64 + lane;
    const bool act = r < n_r;
    const int32_t* col = labT + (act ? r : 0);
    unsigned long long sum = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t b0 = ((int64_t)blockIdx.x * 4 + w) * 64; b0 < m; b0 += stride) {
        const int nb = m - b0 < 64 ? (int)(m - b0) : 64;
        const bool in = b0 + lane < m;
        const int32_t mu = in ? eu[b0 + lane] : 0, mv = in ? ev[b0 + lane] : 0;
        const int32_t mw = UNIT ? 1 : (in ? ew[b0 + lane] : 0);
        for (int t = 0; t < nb; t += 4) {
            int32_t a[4], b[4], wt[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {   // eight rows in flight
                const int tt = t + j < nb ? t + j : nb - 1;
                const int32_t u = __shfl(mu, tt), v = __shfl(mv, tt);
                wt[j] = t + j < nb ? (UNIT ? 1 : __shfl(mw, tt)) : 0;
                a[j] = act ? col[(int64_t)u * ldT] : 0;
                b[j] = act ? col[(int64_t)v * ldT] : 1;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) sum += a[j] == b[j] ? (unsigned long long)wt[j] : 0ull;
        }
    }
    __shared__ unsigned long long s_w[4][64];
    s_w[w][lane] = sum;
    __syncthreads();
    if (w == 0 && act) {
        const unsigned long long t = s_w[0][lane] + s_w[1][lane] + s_w[2][lane] + s_w[3][lane];
        if (t) atomicAdd(&inw[r], t);
    }
}

// ------------------------------------------------------------------ host entry points
static void score_require(Ctx& c) {
    FC_REQUIRE(c.N > 0, FC_ESTATE, "no graph loaded");
    FC_REQUIRE(c.n_r > 0, FC_ESTATE, "no labelings: run fc_run, fc_cd or fc_set_labels first");
    FC_REQUIRE(c.n_r <= SC_MAX_REPLICAS, FC_ELIMIT, "scoring handles at most 2048 local replicas");
}
static double sc_entropy(int64_t n, double s_log) { return std::log((double)n) - s_log / (double)n; }

void score_partitions(Ctx& c, int graph, fc_part_score* out) {
    score_require(c);
    const Graph& g = graph == FC_SCORE_GRAPH_INPUT ? c.g0 : c.g;
    const int64_t N = c.N;
    const int n_r = c.n_r;
    ScLabT lt(c);
    unsigned long long* inw = (unsigned long long*)ensure<uint64_t>(c.sc_res, (size_t)7 * ((n_r + 63) / 64) * 64);
    FC_HIP(hipMemsetAsync(inw, 0, sizeof(uint64_t) * n_r, c.stream));
    if (g.m > 0) {
        const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((g.m + 255) / 256, SC_GRID)), (n_r + 63) / 64);
        if (unit_weights(g))
            k_sc_edges<true><<<grid, TB, 0, c.stream>>>(g.m, g.eu.as<int32_t>(), g.ev.as<int32_t>(), nullptr,
                                                         c.labT.as<int32_t>(), c.ldT, n_r, inw);
        else
            k_sc_edges<false><<<grid, TB, 0, c.stream>>>(g.m, g.eu.as<int32_t>(), g.ev.as<int32_t>(), g.ew.as<int32_t>(),
                                                          c.labT.as<int32_t>(), c.ldT, n_r, inw);
    }
    std::vector<unsigned long long> hin(n_r);
    FC_HIP(hipMemcpyAsync(hin.data(), inw, sizeof(uint64_t) * n_r, hipMemcpyDeviceToHost, c.stream));
    sync(c);
    const unsigned __int128 W2 = (unsigned __int128)(uint64_t)g.M2;
    for (int r = 0; r < n_r; ++r) {
        const ScSeg s = score_segments(c, r);
        const ScStats st = score_stats(c, s, &g);
        fc_part_score& o = out[r];
        o.k = st.k; o.max_size = st.max_size; o.sum_sq = st.sum_sq; o.in_weight = (int64_t)hin[r];
        o.tot_sq_lo = (uint64_t)st.tot_sq; o.tot_sq_hi = (uint64_t)(st.tot_sq >> 64);
        o.s_log = st.s_log;
        o.entropy = sc_entropy(N, st.s_log);
        // (2 in W2 - tot_sq) / W2^2 from exact integers, rounded at the division
        if (g.M2 == 0) o.modularity = 0.0;
        else {
            const __int128 num = (__int128)(2 * (unsigned __int128)hin[r] * W2) - (__int128)st.tot_sq;
            o.modularity = (double)((long double)num / (long double)(W2 * W2));
        }
    }
}

// pairs [np][2], validated by the caller (local replica indices or FC_SCORE_REF)
void score_pairs(Ctx& c, const int32_t* pairs, int64_t np, fc_pair_score* out) {
    score_require(c);
    const int64_t N = c.N;
    const int n_r = c.n_r, banks = (n_r + 63) / 64;
    ScLabT lt(c);
    // index n_r stands for the reference; a pair (a, REF) is scored as row REF, lane a
    std::vector<char> need(n_r + 1, 0);
    std::vector<std::vector<unsigned long long>> want(n_r + 1);
    auto ix = [&](int32_t i) { return i < 0 ? n_r : (int)i; };
    for (int64_t p = 0; p < np; ++p) {
        int a = ix(pairs[2 * p]), b = ix(pairs[2 * p + 1]);
        need[a] = need[b] = 1;
        if (b == n_r) std::swap(a, b);
        if (b == n_r) continue;   // (REF, REF): from the reference's own sizes
        if (want[a].empty()) want[a].assign(banks, 0ull);
        want[a][b >> 6] |= 1ull << (b & 63);
    }
    std::vector<ScStats> st(n_r + 1);
    std::vector<std::vector<ScLane>> acc(n_r + 1);
    for (int i = 0; i <= n_r; ++i) {
        if (!need[i]) continue;
        const ScSeg s = score_segments(c, i == n_r ? FC_SCORE_REF : i);
        st[i] = score_stats(c, s, nullptr);
        if (!want[i].empty()) score_row_pairs(c, s, want[i], acc[i]);
    }
    const double ln_n = std::log((double)N);
    const __int128 n128 = (__int128)N, T = n128 * (n128 - 1) / 2;
    for (int64_t p = 0; p < np; ++p) {
        int a = ix(pairs[2 * p]), b = ix(pairs[2 * p + 1]);
        fc_pair_score& o = out[p];
        o.a = pairs[2 * p]; o.b = pairs[2 * p + 1];
        int row = a, lane = b;
        if (lane == n_r) std::swap(row, lane);
        if (lane == n_r) { o.cells = st[n_r].k; o.sum_sq = st[n_r].sum_sq; o.s_log = st[n_r].s_log; o.slow_members = 0; }
        else {
            const ScLane& l = acc[row][lane];
            o.cells = l.cells; o.sum_sq = l.sum_sq; o.s_log = l.s_log; o.slow_members = l.slow;
        }
        const ScStats &sa = st[a], &sb = st[b];
        double mi = ln_n + (o.s_log - sa.s_log - sb.s_log) / (double)N;
        if (!(mi > 0.0)) mi = 0.0;
        o.mi = mi;
        const double h = (sc_entropy(N, sa.s_log) + sc_entropy(N, sb.s_log)) / 2;
        o.nmi = (sa.k == 1 && sb.k == 1) ? 1.0 : (mi > 0.0 ? mi / h : 0.0);
        // ari from exact integers: numerator and denominator times 2 T
        const __int128 Sij = ((__int128)o.sum_sq - n128) / 2, Sa = ((__int128)sa.sum_sq - n128) / 2,
                       Sb = ((__int128)sb.sum_sq - n128) / 2;
        const __int128 num = 2 * (Sij * T - Sa * Sb), den = (Sa + Sb) * T - 2 * Sa * Sb;
        o.ari = den == 0 ? 1.0 : (double)((long double)num / (long double)den);
    }
}

}  // namespace fc
