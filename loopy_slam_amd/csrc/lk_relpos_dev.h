// The wave tile of the relative-position neighbour MLP (color_decoder.mlp_col_neighbor, decoder.py:477-490), defined ONCE for its three
// kernel bodies: relpos_fwd_wave (lk_decode.hip), relpos_bwd_wave and relpos_bwd_wave_fused (lk_bwd2.hip).
//   tile   64 lanes = 32 neighbour rows x 2 half-waves; row j = lane & 31 is neighbour j & 7 of sample sample0 + (j >> 3)
//   chain  x_j = [sin(2 pi D_j B_r), cos(2 pi D_j B_r), F[I_j]] (KR = 52 units) -> 128 softplus100 -> 32,  D_j = x_I - p,  p = o + z d
//   units  CT tiles (lk_common.h): register 4 g + t of half-wave h holds unit 32 tile + 8 g + 4 h + t of this lane's row.  Units 0..ER-1
//          (20) are the embedding [sin 10 | cos 10], ER..KR-1 feature channels 0..31, KR..KRP-1 (52..55) and the rest of tile 1 zero;
//          group 2 of tile 0 is mixed: embedding units 16..19 in half-wave 0, channels 0..3 in half-wave 1
//   rows   a padded slot (idx < 0) reads the finite dummy row 0 with weight 0; a lane past the last sample recomputes the last one, stores nothing
// The pieces with branches in them are MACROS that expand in the caller, the straight-line ones are functions: a __forceinline__ function
// is optimised on its own before it is inlined, and where it has branches that changed the register allocation of these kernels, which
// run at their register limit (profiles/relpos_forms.md, section 5).
#pragma once
#include "lk_common.h"
#include "lk_kernels.h"

#define RPF_SC 1024.0f                  // pre-scale of the fp16-piece backward chains (d out * 2^10) and its inverse where d x leaves
#define RPF_ISC (1.0f / 1024.0f)

// [sin(x_0..n-1), cos(x_0..n-1)] embedding unit u of a [3][n] matrix (colour: n = 20, rel-pos: n = 10); PADDED: units u >= 2 n are 0
template <bool PADDED>
__device__ __forceinline__ float sincos_embed_unit(const float* __restrict__ B, int n, int u, float a0, float a1, float a2) {
    if (PADDED && u >= 2 * n) return 0.0f;
    const int xi = (u < n) ? u : u - n;
    const float x = lk_fourier_arg(a0, a1, a2, B[xi], B[n + xi], B[2 * n + xi]);
    return (u < n) ? lk_sinf(x) : lk_cosf(x);
}

// 1. Row set-up from the pointer set LkRelposArgs / LkRelposBwdArgs share; P: samples of this launch (its live prefix).  Declares
//    h, sample, live, sp (clamped sample), nb_i, idx (clamped: padded slot -> 0), has, wgt, a0..a2 = fl(2 pi (x_I - p)), frow.
//    The one real difference: the FORWARD's weight counts whenever the slot is filled, `has` (nbr_count >= min_nn) is applied where it
//    stores c (rp_has there: the load stays late); the BACKWARD kernels' weight counts in a live row of a kept sample only.
template <class Args>
__device__ __forceinline__ bool rp_has(const Args& a, int sp) { return a.nbr_count[sp] >= a.min_nn; }
#define RP_ROW_SETUP(a, sample0, P, lane, BWD)                                                                      \
    const int h = (lane) >> 5;                                                                                      \
    const int j = (lane) & 31;                                                                                      \
    const int sample = (sample0) + (j >> 3);                                                                        \
    const bool live = sample < (P);                                                                                 \
    const int sp = live ? sample : (P) - 1;                                                                         \
    const int nb_i = j & 7;                                                                                         \
    const int r = sp / a.S;                                                                                         \
    const float z = a.z[sp];                                                                                        \
    const float px = lk_madd_rn(a.rays_o[3 * r], a.rays_d[3 * r], z);                                               \
    const float py = lk_madd_rn(a.rays_o[3 * r + 1], a.rays_d[3 * r + 1], z);                                       \
    const float pz = lk_madd_rn(a.rays_o[3 * r + 2], a.rays_d[3 * r + 2], z);                                       \
    int idx = a.nbr_idx[(size_t)sp * LK_K + nb_i];                                                                  \
    const bool has = (BWD) ? rp_has(a, sp) : true;                                                                  \
    const float wgt = (idx >= 0 && has && (!(BWD) || live)) ? a.nbr_w[(size_t)sp * LK_K + nb_i] : 0.0f;             \
    if (idx < 0) idx = 0;                                                                                           \
    const float a0 = __fmul_rn(LK_TWO_PI, __fsub_rn(a.pos[3 * (size_t)idx], px));       /* D = x_I - p */           \
    const float a1 = __fmul_rn(LK_TWO_PI, __fsub_rn(a.pos[3 * (size_t)idx + 1], py));                               \
    const float a2 = __fmul_rn(LK_TWO_PI, __fsub_rn(a.pos[3 * (size_t)idx + 2], pz));                               \
    const size_t frow = (size_t)idx * LK_C;

// 2. Input tiles x0, x1 of the row (declared here).  f16: half feature tables - a run-time value in the forward, a template parameter in
//    the backward bodies.  PAD: the embedding unit's u >= 2 n test, dead here (u0 < ER) - the forward keeps it, as it always had it
#define RP_INPUT_TILES(x0, x1, W, col_feats, f16, PAD)                                                              \
    f32x16 x0, x1;                                                                                                  \
    _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                                 \
        const int u0 = 8 * g + 4 * h;                                                                               \
        if (u0 < ER) {                                                                                              \
            _Pragma("unroll") for (int t = 0; t < 4; ++t) x0[4 * g + t] = sincos_embed_unit<PAD>(W + R_EB, 10, u0 + t, a0, a1, a2); \
        } else {                                                                                                    \
            const float4 v = lk_feat4(col_feats, f16, frow + (u0 - ER));                                            \
            x0[4 * g] = v.x; x0[4 * g + 1] = v.y; x0[4 * g + 2] = v.z; x0[4 * g + 3] = v.w;                         \
        }                                                                                                           \
    }                                                                                                               \
    x1 = lk_zero16();                                                                                               \
    _Pragma("unroll") for (int g = 0; g < 3; ++g) {                                                                 \
        const int u0 = 32 + 8 * g + 4 * h;                                                                          \
        if (u0 < KR) {                                                                                              \
            const float4 v = lk_feat4(col_feats, f16, frow + (u0 - ER));                                            \
            x1[4 * g] = v.x; x1[4 * g + 1] = v.y; x1[4 * g + 2] = v.z; x1[4 * g + 3] = v.w;                         \
        }                                                                                                           \
    }

// 3. Hidden layer hid[4] (declared here), unpipelined form (forward and plain backward): bias tiles, linear1 on fp16x3 pieces, softplus.
//    FH: the fp16 forward fragments.  (The fused body keeps its fragment-ahead loop: another schedule, not a copy.)
//    FMA: the form of the fp16 cut's remainder (lk_common.h: lk_cut2h), SA: the addressing form of the loads (lk_sbase) - the same bits either way
#define RP_HIDDEN(hid, W, FH, x0, x1, lane, FMA, SA)                                                                      \
    f32x16 hid[4];                                                                                                  \
    _Pragma("unroll") for (int nb = 0; nb < 4; ++nb) hid[nb] = lk_rowvec_tile<SA>(W + R_B1, nb * 32, lane);   /* accumulators start from the bias */ \
    lk_gemm_h3<4, 2, FMA, SA>(hid, FH + FM20_FWDH, 4, 0, 0, x0, 0, lane);                                              \
    lk_gemm_h3<4, 2, FMA, SA>(hid, FH + FM20_FWDH, 4, 2, 0, x1, 0, lane);     /* units 32..55; registers 12..15 of x1 are zero */ \
    _Pragma("unroll") for (int nb = 0; nb < 4; ++nb) {                                                              \
        _Pragma("unroll") for (int q = 0; q < 16; ++q) hid[nb][q] = lk_softplus100(hid[nb][q]);                     \
    }

// 4. d sin = cos, d cos = -sin: the derivative of embedding unit u is (+/-) the FORWARD value of its partner unit u +/- 10, which x0 holds - in
//    this lane for 12 of the 20 units, in the other half-wave's lane for units 2, 3, 6, 7 / 12, 13, 16, 17 (four exchanges).  v[4 g + t]: register 4 g + t
struct RpFder { float v[12]; };
__device__ __forceinline__ RpFder rp_fder(const f32x16& x0, int h) {
    RpFder f;
    const float r0 = __shfl_xor(h ? x0[4] : x0[8], 32), r1 = __shfl_xor(h ? x0[5] : x0[9], 32);
    const float r2 = __shfl_xor(x0[2], 32), r3 = __shfl_xor(x0[3], 32);
    f.v[0] = x0[6]; f.v[1] = x0[7]; f.v[2] = r0; f.v[3] = r1;                                        // units 0-3 | 4-7
    f.v[4] = h ? -r2 : x0[10]; f.v[5] = h ? -r3 : x0[11]; f.v[6] = -x0[0]; f.v[7] = -x0[1];          // units 8-11 | 12-15
    f.v[8] = -r2; f.v[9] = -r3; f.v[10] = -x0[4]; f.v[11] = -x0[5];                                  // units 16-19 (low half)
    return f;
}

// 5. linear2's operands: dW2 = sum_rows (w d c) hid^T = sum_samples d c (sum_j w_j hid_j)^T -> only the per-SAMPLE weight sum and weighted
//    hidden vector Hbar [P][128] are needed (8x fewer rows, no hid rows)
#define RP_STORE_WSUM(a) { const float wsum = lk_sum8<true>(wgt); if (live && h == 0 && nb_i == 0) a.w_sum[sp] = wsum; }
#define RP_STORE_HBAR(a, hid, nb)                                                                                   \
    _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                                 \
        float v[4];                                                                                                 \
        _Pragma("unroll") for (int tt = 0; tt < 4; ++tt) v[tt] = lk_sum8<true>(wgt * hid[nb][4 * g + tt]);          \
        if (live && nb_i == 0)                                                                                      \
            *reinterpret_cast<float4*>(a.hbar + (size_t)sp * 128 + nb * 32 + 8 * g + 4 * h) = make_float4(v[0], v[1], v[2], v[3]); \
    }

// 6. Tail: d B_r partials (half-wave sums, then LDS adds into part [3][10]: two units - sin, cos - and both half-waves meet in one slot)
//    and the d feature rows of the neighbours (summed per point by k_feat_gather), from dx[2] and fd = rp_fder(x0).  SCALED: d x still
//    carries RPF_SC and is scaled back inside the expressions, (d x * ISC) * fder - the plain fp16-piece body scales d x beforehand, the same
//    product.  DP (plain body) with want_p: dax / day / daz += this lane's share of d loss / d (x_I - p).  want_w: the d B partials are wanted
#define RP_UNSCALE(SCALED, v) ((SCALED) ? (v) * RPF_ISC : (v))
#define RP_TAIL(a, dx, fd, SCALED, DP, want_p, want_w, part, dax, day, daz)                                         \
    _Pragma("unroll") for (int tile = 0; tile < 2; ++tile)                                                          \
    _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                                 \
        const int u0 = 32 * tile + 8 * g + 4 * h;                                                                   \
        const bool is_emb = u0 < ER;                 /* uniform per half-wave (group 2 of tile 0 is mixed) */        \
        if (tile == 0 && g < 3) {                    /* groups that hold embedding units in at least one half */     \
            _Pragma("unroll") for (int t = 0; t < 4; ++t) {                                                         \
                const int u = u0 + t;                                                                               \
                const int xi = is_emb ? ((u < 10) ? u : u - 10) : 0;                                                \
                float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;                                                              \
                if (DP) { const float* B = a.W + R_EB; b0 = B[xi]; b1 = B[10 + xi]; b2 = B[20 + xi]; }              \
                float gx = 0.0f;                                                                                    \
                if (is_emb) gx = RP_UNSCALE(SCALED, dx[tile][4 * g + t]) * fd.v[4 * g + t];                          \
                if ((DP) && (want_p)) {                                                                             \
                    dax = fmaf(gx * LK_TWO_PI, b0, dax); day = fmaf(gx * LK_TWO_PI, b1, day); daz = fmaf(gx * LK_TWO_PI, b2, daz); \
                }                                                                                                   \
                if (want_w) {                        /* every lane takes part in the reductions: convergent shuffles */ \
                    const float s0 = lk_half_wave_sum(gx * a0), s1 = lk_half_wave_sum(gx * a1), s2 = lk_half_wave_sum(gx * a2); \
                    if ((lane & 31) == LK_HWS_LANE && is_emb) {                                                     \
                        atomicAdd(part + xi, s0);                                                                   \
                        atomicAdd(part + 10 + xi, s1);                                                              \
                        atomicAdd(part + 20 + xi, s2);                                                              \
                    }                                                                                               \
                }                                                                                                   \
            }                                                                                                       \
        }                                                                                                           \
        if (!is_emb && u0 < KR) {                    /* d feature row of this neighbour */                          \
            if ((a.flags & LK_FLAG_GRAD_FEATS) && live)                                                             \
                *reinterpret_cast<float4*>(a.dfeat + ((size_t)sp * 8 + nb_i) * LK_C + (u0 - ER)) =                  \
                    make_float4(RP_UNSCALE(SCALED, dx[tile][4 * g]), RP_UNSCALE(SCALED, dx[tile][4 * g + 1]),       \
                                RP_UNSCALE(SCALED, dx[tile][4 * g + 2]), RP_UNSCALE(SCALED, dx[tile][4 * g + 3]));  \
        }                                                                                                           \
    }
