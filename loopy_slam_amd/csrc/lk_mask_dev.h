// Inside-mask threshold thr = min(10 * median(d > 0), 1.2 * max(d)) of a ray batch (Tracker.py:153-155, Mapper.py:674-676)
// as a device function of ONE 1024-thread workgroup, shared by k_inside_mask (lk_optim.hip) and the fused batch-assembly
// kernel of the tracking loop (lk_loop.hip).  Median = 4-pass radix select over the bit patterns of the positive depths.
// REG = true (n <= LK_MASK_REG_MAX): the values stay in registers between the passes; otherwise they are re-read from
// `scratch`.  The top byte of a depth takes a handful of values, so in the first pass the histogram is built with
// one LDS add per (wave, distinct byte) instead of one same-address add per ray.
// (the select itself, its histogram add and the shared-memory block: lk_scan_dev.h)
#pragma once
#include "lk_common.h"
#include "lk_scan_dev.h"

#define LK_MASK_REG_MAX 8192
#define LK_MASK_VPT (LK_MASK_REG_MAX / 1024)
// the batch-assembly kernel of the per-frame loops also comes in a 16-values-per-thread form (k_pregather<16>: the 10 000-ray mapping
// batches of the TUM / ScanNet configs)
#define LK_LOOP_MAX_R 16384

// u[q] = bit pattern of depth (t + 1024 q) if positive else 0 (REG) / scratch[i] likewise (!REG); mycnt / mymax = this
// thread's count of positive depths and their largest bit pattern.  Returns thr; *any = false if no depth is positive.
template <bool REG, int VPT = LK_MASK_VPT>
__device__ __forceinline__ float lk_inside_thr(const unsigned (&u)[VPT], const uint32_t* __restrict__ scratch, int n,
                                               unsigned mycnt, unsigned mymax, LkSelectShared& S, bool* any) {       // S.s_aux: the largest bit pattern
    const int t = threadIdx.x, lane = t & 63;
    if (t == 0) { S.s_cnt = 0; S.s_aux = 0; }
    __syncthreads();
    // one LDS atomic per WAVE (1024 same-address atomics cost microseconds)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mycnt += __shfl_xor(mycnt, o); mymax = max(mymax, (unsigned)__shfl_xor((int)mymax, o)); }
    if (lane == 0) { atomicAdd(&S.s_cnt, mycnt); atomicMax(&S.s_aux, mymax); }
    __syncthreads();
    const unsigned m = S.s_cnt;
    *any = m != 0;
    if (m == 0) return 0.0f;
    // Shortcut: thr = min(10*median, 1.2*max) is 1.2*max unless the median itself satisfies fl(10 v) < fl(1.2 max); that
    // predicate is monotone in v, so the (lower) median at rank (m-1)/2 satisfies it iff MORE than (m-1)/2 values do -
    // one counting pass instead of the 4-pass radix select (depth images: median ~ max/2, the select almost never runs).
    const float mx12 = __fmul_rn(1.2f, __uint_as_float(S.s_aux));
    {
        unsigned below = 0;
        if (REG) {
#pragma unroll
            for (int q = 0; q < VPT; ++q) below += (u[q] && __fmul_rn(10.0f, __uint_as_float(u[q])) < mx12) ? 1u : 0u;
        } else {
            for (int i = t; i < n; i += 1024) { const unsigned v = scratch[i]; below += (v && __fmul_rn(10.0f, __uint_as_float(v)) < mx12) ? 1u : 0u; }
        }
        if (t == 0) S.s_rank = 0;
        __syncthreads();
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o);
        if (lane == 0) atomicAdd(&S.s_rank, below);
        __syncthreads();
    }
    const bool need_median = S.s_rank > (m - 1) / 2;                    // block-uniform
    __syncthreads();
    // torch.median: the lower of the two middle values
    LK_RADIX_SELECT(S, t, (m - 1) / 2, need_median, if (t < 256) S.hist[t] = 0,
        if (REG) {
            _Pragma("unroll") for (int q = 0; q < VPT; ++q) {
                const bool on = u[q] && (u[q] & himask) == prefix;
                const unsigned digit = (u[q] >> shift) & 255u;
                if (shift == 24) LK_HIST_ADD_WAVE(S.hist, on, digit, lane)       // all lanes: the loop over q is wave-uniform
                else if (on) atomicAdd(&S.hist[digit], 1u);
            }
        } else {
            for (int i = t; i < n; i += 1024) {
                const unsigned v = scratch[i];
                if (v && (v & himask) == prefix) atomicAdd(&S.hist[(v >> shift) & 255u], 1u);
            }
        })
    const float med = __uint_as_float(S.s_prefix);
    return need_median ? fminf(__fmul_rn(10.0f, med), mx12) : mx12;
}

// ------------------------------------------------------------------------------------------------------------------------
// tracking.handle_dynamic: False (Tracker.py:177-179): the outlier mask of the tracker loss is |gt - depth| < 10 * median(|gt - depth|)
// instead of the uncertainty-normalised residual against 10 x its mean.  resid[i] >= 0 (or NaN) for a present ray, sign bit set for
// an absent one (gt_depth <= 0: the reference filters those before it renders).  ONE 1024-thread workgroup: 4-pass radix select
// over the bit patterns (non-negative floats order as unsigned integers), values re-read from memory in every pass.
// torch.median: the LOWER of the two middle values (rank (m - 1) / 2), NaN if any element is NaN (the mask is then empty).
// No present ray: 0 (empty mask).
__device__ __forceinline__ float lk_block_median10(const float* __restrict__ resid, int n, LkSelectShared& S) {      // S.s_aux: NaN count
    const int t = threadIdx.x, lane = t & 63, nt = blockDim.x;
    if (t == 0) { S.s_cnt = 0; S.s_aux = 0; }
    __syncthreads();
    unsigned cnt = 0, nan = 0;
    for (int i = t; i < n; i += nt) {
        const unsigned v = __float_as_uint(resid[i]);
        if (!(v & 0x80000000u)) { ++cnt; nan += (v > 0x7f800000u) ? 1u : 0u; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o); nan += __shfl_xor(nan, o); }
    if (lane == 0) { atomicAdd(&S.s_cnt, cnt); atomicAdd(&S.s_aux, nan); }
    __syncthreads();
    const unsigned m = S.s_cnt;
    if (m == 0) return 0.0f;
    if (S.s_aux != 0) return __uint_as_float(0x7fc00000u);
    __syncthreads();
    // every pass aggregates: residuals share their top bytes, same-address adds would serialise
    LK_RADIX_SELECT(S, t, (m - 1) / 2, true, for (int b = t; b < 256; b += nt) S.hist[b] = 0,
        for (int i0 = 0; i0 < n; i0 += nt) {         // workgroup-uniform trip count: every lane takes part in the ballots
            const unsigned v = (i0 + t < n) ? __float_as_uint(resid[i0 + t]) : 0x80000000u;
            const bool on = !(v & 0x80000000u) && (v & himask) == prefix;
            const unsigned digit = (v >> shift) & 255u;
            LK_HIST_ADD_WAVE(S.hist, on, digit, lane)
        })
    return __fmul_rn(10.0f, __uint_as_float(S.s_prefix));
}
