// analysis.h -- what the analysis headers (components.h, levels.h, coassoc.h) share: the bin of a
// support value, the wave-aggregated add into LDS bins, and the phase timer of one call.
// Included by consensus.hip before score.h (Ctx, timer_begin and FC_HIP are in scope).
#pragma once

namespace fc {

// bin of a support value: s inside [0, nt], nt + 1 for anything else (a caller's buffer is not trusted)
__device__ __forceinline__ int support_bin(int32_t s, int nt) { return (uint32_t)s <= (uint32_t)nt ? s : nt + 1; }

// bins[bin] += 1 for every lane with `in` set: the lanes that agree with the wave's first active lane
// add once (supports and counts pile up at 0 and at the replica count), the stragglers one by one.
// Every lane of the wave calls this (wave-uniform control flow) with act = __ballot(in) != 0.
// `bin` travels by reference on purpose: a by-value argument is marked noundef, the compiler then
// drops the freeze it keeps on k_ca_hist's 16 accumulators and vectorises that kernel's tile loop
// differently (135 VGPRs and 39 SGPR spills instead of 131 and 19).
__device__ __forceinline__ void wave_bin_add(unsigned int* bins, bool in, const int& bin, unsigned long long act,
                                             int lane) {
    const int src = __ffsll((long long)act) - 1;
    const int lead = __shfl(bin, src);
    const unsigned long long same = __ballot(in && bin == lead);
    if (lane == src) atomicAdd(&bins[lead], (unsigned int)__popcll(same));
    if (in && bin != lead) atomicAdd(&bins[bin], 1u);
}
// the same add from the same ballot and shuffle, returning the lane's rank inside its bin (the
// bin's value before the lane's own 1; undefined for a lane without `in`)
__device__ __forceinline__ unsigned int wave_bin_rank(unsigned int* bins, bool in, const int& bin,
                                                      unsigned long long act, int lane) {
    const int src = __ffsll((long long)act) - 1;
    const int lead = __shfl(bin, src);
    const bool mine = in && bin == lead;
    const unsigned long long same = __ballot(mine);
    unsigned int r = 0;
    if (lane == src) r = atomicAdd(&bins[lead], (unsigned int)__popcll(same));
    r = __shfl(r, src) + (unsigned int)__popcll(same & ((1ull << lane) - 1ull));
    if (in && !mine) r = atomicAdd(&bins[bin], 1u);
    return r;
}

// Phase boundaries of one call as events of the timing pool (timing enabled only); the device
// time of each phase goes to the array given (Ctx::cp_ms / lv_ms / ca_ms).
struct PhaseMarks {
    static constexpr int MAX = 5;
    Ctx& c;
    double* ms;
    const int phases;
    int ev[MAX + 1];
    int n = 0;
    template <int N> PhaseMarks(Ctx& x, double (&out)[N]) : c(x), ms(out), phases(N) {
        static_assert(N <= MAX, "PhaseMarks::ev is too short");
    }
    void clear() {
        for (int i = 0; i < phases; ++i) ms[i] = 0.0;
    }
    void mark() {
        if (c.timer.on && n <= phases) ev[n++] = timer_begin(c);
    }
    void collect() {   // after a stream synchronise
        clear();
        for (int i = 0; i + 1 < n; ++i) {
            float x = 0.f;
            FC_HIP(hipEventElapsedTime(&x, c.timer.pool[ev[i]], c.timer.pool[ev[i + 1]]));
            ms[i] = x;
        }
    }
};

}  // namespace fc
