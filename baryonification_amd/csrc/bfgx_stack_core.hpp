// bfgx_stack_core.hpp -- the part of a halo-centred profile kernel that is not geometry, shared by the shell, box and grid measurements
// (bfgx_stack.hpp, bfgx_snapshot_stack.hpp, bfgx_grid_stack.hpp).
//
// Each kernel enumerates its own pairs (disc pixels, cell columns, grid chords), forms its own abscissa x and applies its own value rule.
// What happens to an (x, value) lives here: the edges in LDS, the bin rule, the bins of a halo in LDS and their one store per cell; and,
// for the two workgroup-per-halo kernels, how a round of ragged runs (cell columns, chords) is flattened over the threads.
#pragma once
#include "bfgx_kernels.hpp"

namespace bfgx {

constexpr int kStackMaxBins = 64;
constexpr int kStackEdgeLds = 128;            // the edges padded with +inf to a power of two: a branch-free search

// the [nhalo][nb] outputs of a measurement (the shear members are unused without a shear pair; the box measurement has npix = npart)
struct StackOut { int64_t *npix, *npix_shear; double *sum, *sum_t, *sum_x; };

// s_edges[kStackEdgeLds] = the nb + 1 edges, then +inf (the caller's barrier makes them visible)
__device__ inline void stack_load_edges(double *s_edges, const double *edges, int nb, int tid, int nthreads)
{
    for (int i = tid; i < kStackEdgeLds; i += nthreads) s_edges[i] = i <= nb ? edges[i] : __builtin_inf();
}

// THE bin rule: b with edges[b] <= x < edges[b + 1], or -1 where x is outside [edges[0], edges[nb]) or NaN.  e0 = s_edges[0], read once
// per halo by the caller: it stays in registers over the pair loop
__device__ inline int stack_find_bin(const double *s_edges, double e0, double x, int nb)
{
    int b = 0;                                  // largest b with edges[b] <= x (the padding is +inf)
#pragma unroll
    for (int st = kStackEdgeLds >> 1; st > 0; st >>= 1)
        if (s_edges[b + st] <= x) b += st;
    return (!(x >= e0) || b >= nb) ? -1 : b;
}

// The (at most) 64 bins of one halo in LDS: fp64 LDS adds (ds_add_f64, -munsafe-fp-atomics) for the sums, 32-bit LDS adds for the counts
// (every kernel states why its counts stay below 2^32).  SECOND adds the bins of the shear pair.  Thread / lane i calls clear(i) and
// store(i, ...): bin i to cell o, every cell of every output written exactly once, no zero-fill; the caller's barriers separate them from the adds.
template <bool SECOND>
struct StackBins {
    double sum[kStackMaxBins];
    unsigned int n[kStackMaxBins];
    __device__ void clear(int i) { sum[i] = 0.0; n[i] = 0u; }
    __device__ void count(int b) { atomicAdd(&n[b], 1u); }
    __device__ void add_sum(int b, double v) { atomicAdd(&sum[b], v); }
    __device__ void add(int b, double v) { count(b); add_sum(b, v); }
    __device__ void store(int i, int64_t o, const StackOut &out, bool with_sum = true) const
    {
        out.npix[o] = (int64_t)n[i];
        if (with_sum) out.sum[o] = sum[i];
    }
};

template <>
struct StackBins<true> : StackBins<false> {
    double sum_t[kStackMaxBins], sum_x[kStackMaxBins];
    unsigned int ns[kStackMaxBins];
    __device__ void clear(int i) { StackBins<false>::clear(i); sum_t[i] = 0.0; sum_x[i] = 0.0; ns[i] = 0u; }
    __device__ void add_shear(int b, double t, double x)
    {
        atomicAdd(&ns[b], 1u);
        atomicAdd(&sum_t[b], t);
        atomicAdd(&sum_x[b], x);
    }
    __device__ void store(int i, int64_t o, const StackOut &out) const
    {
        StackBins<false>::store(i, o, out);
        out.npix_shear[o] = (int64_t)ns[i];
        out.sum_t[o] = sum_t[i];
        out.sum_x[o] = sum_x[i];
    }
};

// One round of a workgroup of THREADS threads over ragged runs: thread t brings the length cnt of its run(s) and gets their exclusive prefix
// over the workgroup and the total.  wtot: THREADS / kWave words of LDS.  Holds one barrier; a second, after the caller has stored its prefix
// slots, comes before ragged_find.
template <int THREADS>
__device__ inline void block_ragged_prefix(uint32_t cnt, int lane, int wid, uint32_t *wtot, uint32_t &excl, uint32_t &total)
{
    const uint32_t incl = wave_scan_incl_u32(cnt, lane);
    if (lane == kWave - 1) wtot[wid] = incl;
    __syncthreads();
    uint32_t woff = 0;
    total = 0;
#pragma unroll
    for (int q = 0; q < THREADS / kWave; ++q) {
        const uint32_t t = wtot[q];
        woff += (q < wid) ? t : 0u;
        total += t;
    }
    excl = woff + incl - cnt;
}

// the run of element t of the concatenation: the largest slot with prefix[slot] <= t (an empty run shares its prefix with the next: skipped)
template <int SLOTS>
__device__ inline int ragged_find(const uint32_t *prefix, uint32_t t)
{
    int slot = 0;
#pragma unroll
    for (int st = SLOTS >> 1; st > 0; st >>= 1)
        if (prefix[slot + st] <= t) slot += st;
    return slot;
}

}  // namespace bfgx
