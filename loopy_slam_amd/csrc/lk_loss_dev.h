// The per-ray arithmetic of the two losses and the pose <-> rays map, each formula once: the mapper's loss (Mapper.py:691-720), the two
// passes of the tracker's (Tracker.py:169-191), quaternion -> rotation (common.py:301-324) and the pose gradient from the ray moments
// (common.py:104-120 backwards).  The standalone loss kernels (lk_optim.hip), the composite kernels (lk_sample.hip, lk_loop.hip), the
// epilogue of the fused forward (lk_decode.hip) and the tracker's prologue of k_decode_bwd (lk_track_dev.h) call these; the mapper's prologue of
// k_decode_bwd (lk_map_draw, lk_composite_dev.h) keeps a written-out copy of lk_map_ray_loss, for the reason given there.
// What a kernel does with the terms - the order of its reduction, atomics or none - is its own.
#pragma once
#include "lk_common.h"

__device__ __forceinline__ float lk_sgn(float x) { return (x > 0.0f) ? 1.0f : ((x < 0.0f) ? -1.0f : 0.0f); }

// ------------------------------------------------------------------ mapper
// gd: the reading of ray r (<= 0: absent), d: its rendered depth, valid: enough of its samples have neighbours, c*: its rendered colour;
// gt_color [R][3]: the observed colours, read only for a masked ray with use_color.  dd, dc*: d loss / d depth, d colour; geo, col, cnt: the
// ray's terms of the loss row.
struct LkMapRayLoss { float dd, dc0, dc1, dc2, geo, col, cnt; };
__device__ __forceinline__ LkMapRayLoss lk_map_ray_loss(float gd, float d, bool valid, float c0, float c1, float c2, const float* __restrict__ gt_color, int r,
                                                        float w_color, int use_color) {
    LkMapRayLoss o;
    o.dd = 0.0f; o.dc0 = 0.0f; o.dc1 = 0.0f; o.dc2 = 0.0f; o.geo = 0.0f; o.col = 0.0f; o.cnt = 0.0f;
    if ((gd > 0.0f) && valid && !(d != d)) {
        o.geo = fabsf(gd - d);
        // two compares, not lk_sgn(d - gd): the spelling of the timed path (lk_map_draw).  The same value for every non-NaN pair while fp32
        // denormals are on (d - gd == 0 only if d == gd)
        o.dd = (d > gd) ? 1.0f : ((d < gd) ? -1.0f : 0.0f);
        o.cnt = 1.0f;
        if (use_color) {
            const float e0 = c0 - gt_color[3 * r], e1 = c1 - gt_color[3 * r + 1], e2 = c2 - gt_color[3 * r + 2];
            o.col = fabsf(e0) + fabsf(e1) + fabsf(e2);
            o.dc0 = w_color * lk_sgn(e0); o.dc1 = w_color * lk_sgn(e1); o.dc2 = w_color * lk_sgn(e2);
        }
    }
    return o;
}

// ------------------------------------------------------------------ tracker, pass 1
// Rays with gt_depth <= 0 are "absent": the reference filters them out BEFORE rendering (get_samples depth_filter + inside mask,
// Tracker.py:142-160), so they take no part in the mean.  tv: the uncertainty-normalised residual, cv: 1 for a present ray (the two terms of
// the batch mean); resid: what pass 2's mask compares with its threshold - tv, or with median (tracking.handle_dynamic: False,
// Tracker.py:177-179) |gt - depth| with the sign bit set for an absent ray
struct LkTrackResid { float tv, cv, resid; };
__device__ __forceinline__ LkTrackResid lk_track_resid(float gd, float depth, float var, int median) {
    LkTrackResid o;
    const bool present = gd > 0.0f;
    o.tv = present ? fabsf(gd - depth) / sqrtf(var + 1e-10f) : 0.0f;
    o.cv = present ? 1.0f : 0.0f;
    o.resid = median ? (present ? fabsf(gd - depth) : -1.0f) : o.tv;
    return o;
}

// ------------------------------------------------------------------ tracker, pass 2
// in: the ray's rendered depth / variance / colour (d, v, c*), its readings (g, g*) and pass 1's resid (tm); thr: 10 x the batch mean of tv,
// or 10 x the median of |gt - depth|
struct LkTrackRayIn { float d, v, g, tm, c0, c1, c2, g0, g1, g2; };
struct LkTrackRayLoss { float dd, dc0, dc1, dc2, geo, col, cnt, gt; };
__device__ __forceinline__ LkTrackRayLoss lk_track_ray_loss(const LkTrackRayIn& in, float thr, int median, int use_color, float w_color) {
    LkTrackRayLoss o;
    const float d = in.d, v = in.v, g = in.g, tm = in.tm;
    const float tt = median ? fabsf(g - d) / sqrtf(v + 1e-10f) : tm;          // the loss term stays uncertainty-normalised
    const bool m = (tm < thr) && (g > 0.0f) && !(d != d) && !(v != v);
    o.dd = 0.0f; o.dc0 = 0.0f; o.dc1 = 0.0f; o.dc2 = 0.0f; o.geo = 0.0f; o.col = 0.0f; o.cnt = 0.0f; o.gt = g;
    if (m) {
        o.geo = fminf(fmaxf(tt, 0.0f), 1e3f);
        if (tt <= 1e3f) o.dd = lk_sgn(d - g) / sqrtf(v + 1e-10f);
        o.cnt = 1.0f;
        const float e0 = in.c0 - in.g0, e1 = in.c1 - in.g1, e2 = in.c2 - in.g2;
        o.col = fabsf(e0) + fabsf(e1) + fabsf(e2);
        if (use_color) { o.dc0 = w_color * lk_sgn(e0); o.dc1 = w_color * lk_sgn(e1); o.dc2 = w_color * lk_sgn(e2); }
    }
    return o;
}

// ------------------------------------------------------------------ pose <-> rays
// cam = (q_r, q_i, q_j, q_k | T): rays_d = Rm dir, rays_o = T
__device__ __forceinline__ void lk_quat_rot(const float* __restrict__ cam, float (&Rm)[9]) {
    const float qr = cam[0], qi = cam[1], qj = cam[2], qk = cam[3];
    const float s = 2.0f / (qr * qr + qi * qi + qj * qj + qk * qk);
    Rm[0] = 1.0f - s * (qj * qj + qk * qk); Rm[1] = s * (qi * qj - qk * qr); Rm[2] = s * (qi * qk + qj * qr);
    Rm[3] = s * (qi * qj + qk * qr); Rm[4] = 1.0f - s * (qi * qi + qk * qk); Rm[5] = s * (qj * qk - qi * qr);
    Rm[6] = s * (qi * qk - qj * qr); Rm[7] = s * (qj * qk + qi * qr); Rm[8] = 1.0f - s * (qi * qi + qj * qj);
}
// d loss / d cam[7] from the twelve ray moments acc = [sum_r g_rd (x) dir  (3 x 3, row = ray axis) | sum_r g_ro]: Rm = I + s P(q), s = 2 / |q|^2
__device__ __forceinline__ void lk_pose_grad(const float* cam, const float* acc, float (&gc)[7]) {
    const float qr = cam[0], qi = cam[1], qj = cam[2], qk = cam[3];
    const float N = qr * qr + qi * qi + qj * qj + qk * qk, s = 2.0f / N;
    const float P[9] = {-(qj * qj + qk * qk), qi * qj - qk * qr, qi * qk + qj * qr,
                        qi * qj + qk * qr, -(qi * qi + qk * qk), qj * qk - qi * qr,
                        qi * qk - qj * qr, qj * qk + qi * qr, -(qi * qi + qj * qj)};
    float gp = 0.0f;
#pragma unroll
    for (int q = 0; q < 9; ++q) gp += acc[q] * P[q];
    const float* g = acc;
    const float dPr = g[1] * (-qk) + g[2] * qj + g[3] * qk + g[5] * (-qi) + g[6] * (-qj) + g[7] * qi;
    const float dPi = g[1] * qj + g[2] * qk + g[3] * qj + g[4] * (-2.0f * qi) + g[5] * (-qr) + g[6] * qk + g[7] * qr + g[8] * (-2.0f * qi);
    const float dPj = g[0] * (-2.0f * qj) + g[1] * qi + g[2] * qr + g[3] * qi + g[5] * qk + g[6] * (-qr) + g[7] * qk + g[8] * (-2.0f * qj);
    const float dPk = g[0] * (-2.0f * qk) + g[1] * (-qr) + g[2] * qi + g[3] * qr + g[4] * (-2.0f * qk) + g[5] * qj + g[6] * qi + g[7] * qj;
    const float ds = -s * s;            // d s / d q_x = -s^2 q_x
    gc[0] = ds * qr * gp + s * dPr; gc[1] = ds * qi * gp + s * dPi; gc[2] = ds * qj * gp + s * dPj; gc[3] = ds * qk * gp + s * dPk;
    gc[4] = acc[9]; gc[5] = acc[10]; gc[6] = acc[11];
}
