// The integer selection machinery, each building block once: wave scan, ballot rank, wave-aggregated histogram add, the bin of a 256-bin
// histogram that holds a rank, the 4-pass radix select of one workgroup.  The counting sorts (lk_knn.hip), the stable compactions
// (lk_optim.hip), the inside mask and the tracker's median (lk_mask_dev.h), the batch partition of k_pregather (lk_loop.hip) and the
// high-gradient pixel pool (lk_map.hip) call these.
// What is shared is the arithmetic on lanes and bins.  Where the values come from (registers, scratch, an image), which of them take part
// (absent rays, NaN), which passes aggregate and in which order a kernel sums its wave counts is its own.
// As in lk_relpos_dev.h the pieces with branches in them are MACROS that expand in the caller and the straight-line ones are functions: behind a
// __forceinline__ function (the select with its fill as a force-inlined lambda included) k_pregather and k_inside_mask, which run once per
// frame inside the timed step, came out with other instruction streams and more scalar registers; as macros every kernel of the timed
// path is the instruction stream it was when each site had its own copy (profiles/select_forms.md, section 2).
// A wave is 64 lanes; `lane` is lk_lane() of the caller (every site has it in a register already).
#pragma once
#include "lk_common.h"

// ------------------------------------------------------------------ 1. wave inclusive scan
// v of lanes 0 .. lane summed, log-step.  All 64 lanes take part.
#define LK_WAVE_INCL_SCAN(v, lane)                                                                                  \
    _Pragma("unroll") for (int o_ = 1; o_ < 64; o_ <<= 1) {                                                         \
        const auto nb_ = __shfl_up(v, o_);                                                                          \
        if ((lane) >= o_) v += nb_;                                                                                 \
    }
template <class T>
__device__ __forceinline__ T lk_wave_incl_scan(T v, int lane) {
    LK_WAVE_INCL_SCAN(v, lane)
    return v;
}

// ------------------------------------------------------------------ 2. ballot rank
// before = lanes below this one whose pred holds; returns the ballot, whose __popcll is the wave's total (left to the caller: the
// compactions want it in two places, and written once it costs them two scalar registers).  All 64 lanes call it, so where it stands in a
// loop the trip count has to be wave-uniform: the callers give the lanes past the end a false pred instead of leaving.
__device__ __forceinline__ unsigned long long lk_ballot_rank(bool pred, int lane, int& before) {
    const unsigned long long b = __ballot(pred);
    before = __popcll(b & ((1ull << lane) - 1ull));
    return b;
}
// off + the counts of the waves before wave w (wc: per-wave totals in LDS, written by lane 0 of every wave, a barrier in between)
__device__ __forceinline__ int lk_waves_before(const int* wc, int w, int off) {
    for (int q = 0; q < w; ++q) off += wc[q];
    return off;
}

// ------------------------------------------------------------------ 3. wave-aggregated histogram add
// hist[digit] += 1 for every lane with `on`, as one LDS add per (wave, distinct digit): depths and residuals share their top bytes, and
// 1024 adds to the same address serialise (microseconds).  All 64 lanes walk the loop together.  on, digit: variables of the caller.
#define LK_HIST_ADD_WAVE(hist, on, digit, lane)                                                                     \
    {                                                                                                               \
        unsigned long long pending_ = __ballot(on);                                                                 \
        while (pending_) {                                                                                          \
            const int leader_ = __ffsll((long long)pending_) - 1;                                                   \
            const unsigned dl_ = __shfl(digit, leader_);                                                            \
            const unsigned long long same_ = __ballot(on && digit == dl_);                                          \
            if ((lane) == leader_) atomicAdd(&(hist)[dl_], (unsigned)__popcll(same_));                              \
            pending_ &= ~same_;                                                                                     \
        }                                                                                                           \
    }

// ------------------------------------------------------------------ 4. the bin that holds a rank
// hist: 256 counts, rank < their sum.  All 64 lanes of ONE wave, 4 bins per lane.  Exactly one lane owns the bin: it alone runs the
// statements of the last argument, with bin and rank_in_bin declared for them.
#define LK_RADIX_LOCATE(hist, rank, lane, bin, rank_in_bin, ...)                                                    \
    const unsigned h0_ = (hist)[4 * (lane)], h1_ = (hist)[4 * (lane) + 1], h2_ = (hist)[4 * (lane) + 2], h3_ = (hist)[4 * (lane) + 3]; \
    const unsigned tot_ = h0_ + h1_ + h2_ + h3_;                                                                    \
    unsigned incl_ = tot_;                                                                                          \
    LK_WAVE_INCL_SCAN(incl_, lane)                                                                                  \
    const unsigned excl_ = incl_ - tot_;                                                                            \
    if ((rank) >= excl_ && (rank) < incl_) {                                                                        \
        unsigned rank_in_bin = (rank) - excl_, bin = 4 * (lane);                                                    \
        if (rank_in_bin >= h0_) { rank_in_bin -= h0_; ++bin; if (rank_in_bin >= h1_) { rank_in_bin -= h1_; ++bin;   \
            if (rank_in_bin >= h2_) { rank_in_bin -= h2_; ++bin; } } }                                              \
        __VA_ARGS__                                                                                                 \
    }

// ------------------------------------------------------------------ 5. 4-pass radix select of one workgroup
// Leaves in S.s_prefix the 32-bit pattern of ascending rank `rank` among the candidates, most significant byte first; t: threadIdx.x.
// clear: the statement that zeroes S.hist (`if (t < 256) S.hist[t] = 0` where the workgroup has that many threads).  The last argument is
// the fill: statements that add to S.hist the byte (v >> shift) & 255 of every candidate v with (v & himask) == prefix (shift, prefix,
// himask: declared here); every thread of the workgroup runs them, so they may hold ballots.  run == false (workgroup-uniform): no pass
// runs, S.s_prefix = 0.
// Every lane of wave 0 reads s_rank before the one lane that owns the bin writes the next one: the read stands in front of the scan's
// shuffles and the write behind them, and a wave runs them in program order.
struct LkSelectShared { unsigned hist[256]; unsigned s_prefix, s_rank, s_cnt, s_aux; };
#define LK_RADIX_SELECT(S, t, rank, run, clear, ...)                                                                \
    if ((t) == 0) { S.s_prefix = 0; S.s_rank = (rank); }                                                            \
    __syncthreads();                                                                                                \
    for (int shift = 24; (run) && shift >= 0; shift -= 8) {                                                         \
        clear;                                                                                                      \
        __syncthreads();                                                                                            \
        const unsigned prefix = S.s_prefix;                                                                         \
        const unsigned himask = (shift == 24) ? 0u : (0xffffffffu << (shift + 8));                                  \
        __VA_ARGS__                                                                                                 \
        __syncthreads();                                                                                            \
        if ((t) < 64) {                                                                                             \
            const unsigned rank_ = S.s_rank;                                                                        \
            LK_RADIX_LOCATE(S.hist, rank_, (t), bin_, rib_, S.s_rank = rib_; S.s_prefix = prefix | (bin_ << shift);) \
        }                                                                                                           \
        __syncthreads();                                                                                            \
    }
