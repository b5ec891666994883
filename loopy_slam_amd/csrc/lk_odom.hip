// Visual odometry (include/loopy_hip.h, "visual odometry"): the multi-scale hybrid RGB-D odometry that gives the tracker its starting pose
// (the reference's tracking.visual_odometer, src/utils/visual_odometer.py around o3d.t.pipelines.odometry, Hybrid).  tests/odometry_referee.py
// states the same contract in NumPy.
//
//   k_odom_level0   colour, depth -> intensity and depth of level 0 (NaN = no reading)
//   k_odom_down     level l -> level l + 1: binomial intensity, depth-aware binomial depth
//   k_odom_derive   per level: vertex map x and y, Sobel / 8 of intensity and depth
//   k_odom_pixels   one Gauss-Newton iteration over the source pixels: 29 fp32 sums per lane, DPP half-wave sums, one partial row per workgroup
//   k_odom_solve    one workgroup: partial rows added in workgroup order in fp64, 6 x 6 Cholesky, T <- exp(x) T, the iteration's record
// No floating-point atomic and a fixed grid per level: equal inputs give equal bits.  A whole estimate is enqueued without a host
// synchronisation; T lives on the device between the two kernels of an iteration.
//
// k_odom_pixels keeps 29 accumulators and about as many temporaries per lane, well under the 128 registers at which a 256-thread workgroup
// still shares a SIMD with three others; the sums leave the lanes by five DPP adds each (plain VALU: lk_half_wave_sum), not by 6 x 29 LDS
// permutes, the eight half-wave rows of a workgroup meet in 1 KB of LDS and are added in a fixed order.
#include "lk_common.h"

#include <math.h>

#define OD_PLANES 8
#define OD_I 0
#define OD_VX 1
#define OD_VY 2
#define OD_D 3                                // depth = z of the vertex map
#define OD_IX 4
#define OD_IY 5
#define OD_DX 6
#define OD_DY 7
#define OD_NSUM 29                            // 21 of A, 6 of b, the loss, the count
#define OD_ROW 32                             // floats of a partial row
#define OD_MAX_WG 512                         // partial rows of an iteration at the most (grid-stride above that)

struct OdLevels {
    int n;
    int h[LK_ODOM_MAX_LEVELS], w[LK_ODOM_MAX_LEVELS];
    int64_t off[LK_ODOM_MAX_LEVELS + 1];      // first float of each level; off[n] = total
};

static OdLevels od_levels(int H, int W, int n_levels) {
    OdLevels L;
    L.n = n_levels;
    int h = H, w = W;
    int64_t off = 0;
    for (int l = 0; l < LK_ODOM_MAX_LEVELS; ++l) {
        L.h[l] = l < n_levels ? h : 0;
        L.w[l] = l < n_levels ? w : 0;
        L.off[l] = off;
        if (l < n_levels) off += (int64_t)OD_PLANES * h * w;
        h /= 2;
        w /= 2;
    }
    L.off[LK_ODOM_MAX_LEVELS] = off;
    return L;
}

static int od_check(int H, int W, int n_levels, const char* who) {
    if (!(n_levels >= 1 && n_levels <= LK_ODOM_MAX_LEVELS && H > 0 && W > 0 && (int64_t)H * W <= (int64_t)LK_ODOM_MAX_PIXELS &&
          (H >> (n_levels - 1)) >= 8 && (W >> (n_levels - 1)) >= 8)) {
        lk_set_error("%s: 1 <= n_levels <= %d, H W <= %d and a coarsest level of 8 x 8 at least are required", who, LK_ODOM_MAX_LEVELS,
                     LK_ODOM_MAX_PIXELS);
        return LK_ERR_ARG;
    }
    return LK_OK;
}

__device__ __forceinline__ float od_nan() { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ bool od_finite(float v) { return fabsf(v) <= LK_FLT_MAX; }      // false for NaN and the infinities

// ------------------------------------------------------------------ pyramid
__global__ __launch_bounds__(256) void k_odom_level0(const float* __restrict__ color, const float* __restrict__ depth, int n, float max_depth,
                                                     float* __restrict__ I, float* __restrict__ D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float r = color[3 * (size_t)i], g = color[3 * (size_t)i + 1], b = color[3 * (size_t)i + 2];
    I[i] = (0.299f * r + 0.587f * g) + 0.114f * b;
    const float d = depth[i];
    D[i] = (d > 0.0f && d <= max_depth) ? d : od_nan();
}

__global__ __launch_bounds__(256) void k_odom_down(const float* __restrict__ sI, const float* __restrict__ sD, int sh, int sw,
                                                   float* __restrict__ dI, float* __restrict__ dD, int dh, int dw, float depth_diff) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= dh * dw) return;
    const int y = i / dw, x = i - y * dw;
    const float K[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float out = 0.0f;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int yy = min(max(2 * y + r - 2, 0), sh - 1);
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < 5; ++k) t += K[k] * sI[(size_t)yy * sw + min(max(2 * x + k - 2, 0), sw - 1)];
        out += K[r] * t;
    }
    dI[i] = out;
    const float c = sD[(size_t)(2 * y) * sw + 2 * x];
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int yy = 2 * y + r - 2, xx = 2 * x + k - 2;
            if (yy < 0 || yy >= sh || xx < 0 || xx >= sw) continue;
            const float v = sD[(size_t)yy * sw + xx];
            if (fabsf(v - c) <= depth_diff) {            // false where either is NaN
                const float wgt = K[r] * K[k];           // exact
                num += wgt * v;
                den += wgt;
            }
        }
    dD[i] = c == c ? num / den : od_nan();               // a valid centre counts itself: den >= 9/64
}

// Sobel / 8 at (y, x) with the border replicated; any_nan: one of the nine taps is NaN
__device__ __forceinline__ void od_sobel(const float* __restrict__ p, int h, int w, int y, int x, float& dx, float& dy, bool& any_nan) {
    const int y0 = max(y - 1, 0), y2 = min(y + 1, h - 1), x0 = max(x - 1, 0), x2 = min(x + 1, w - 1);
    const float a = p[(size_t)y0 * w + x0], b = p[(size_t)y0 * w + x], c = p[(size_t)y0 * w + x2];
    const float d = p[(size_t)y * w + x0], e = p[(size_t)y * w + x], f = p[(size_t)y * w + x2];
    const float g = p[(size_t)y2 * w + x0], k = p[(size_t)y2 * w + x], m = p[(size_t)y2 * w + x2];
    dx = (((c + 2.0f * f) + m) - ((a + 2.0f * d) + g)) * 0.125f;
    dy = (((g + 2.0f * k) + m) - ((a + 2.0f * b) + c)) * 0.125f;
    const float s = (((a + b) + (c + d)) + ((e + f) + (g + k))) + m;
    any_nan = !(s == s);
}

__global__ __launch_bounds__(256) void k_odom_derive(float* __restrict__ lev, int h, int w, float fx, float fy, float cx, float cy) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = h * w;
    if (i >= n) return;
    const int y = i / w, x = i - y * w;
    const float d = lev[(size_t)OD_D * n + i];
    lev[(size_t)OD_VX * n + i] = (((float)x - cx) / fx) * d;
    lev[(size_t)OD_VY * n + i] = (((float)y - cy) / fy) * d;
    float dx, dy;
    bool bad;
    od_sobel(lev + (size_t)OD_I * n, h, w, y, x, dx, dy, bad);
    lev[(size_t)OD_IX * n + i] = dx;
    lev[(size_t)OD_IY * n + i] = dy;
    od_sobel(lev + (size_t)OD_D * n, h, w, y, x, dx, dy, bad);
    lev[(size_t)OD_DX * n + i] = bad ? od_nan() : dx;
    lev[(size_t)OD_DY * n + i] = bad ? od_nan() : dy;
}

// ------------------------------------------------------------------ one iteration: the sums
struct OdTaps { int i00; float a, b; int w; };
__device__ __forceinline__ float od_bil(const float* __restrict__ m, const OdTaps& t) {
    const float m00 = m[t.i00], m01 = m[t.i00 + 1], m10 = m[t.i00 + t.w], m11 = m[t.i00 + t.w + 1];
    return (1.0f - t.b) * ((1.0f - t.a) * m00 + t.a * m01) + t.b * ((1.0f - t.a) * m10 + t.a * m11);
}

__global__ __launch_bounds__(256) void k_odom_pixels(const float* __restrict__ src, const float* __restrict__ tgt, int h, int w, float fx, float fy,
                                                     float cx, float cy, const double* __restrict__ T, float trunc, float huber_i, float huber_d,
                                                     float* __restrict__ part) {
    __shared__ float s_half[8][OD_ROW];
    const int n = h * w;
    float R[9], tr[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (float)T[4 * i + j];
        tr[i] = (float)T[4 * i + 3];
    }
    float acc[OD_NSUM];
#pragma unroll
    for (int k = 0; k < OD_NSUM; ++k) acc[k] = 0.0f;

#pragma unroll 1
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const float pz = src[(size_t)OD_D * n + p];
        if (!(pz == pz)) continue;
        const float px = src[(size_t)OD_VX * n + p], py = src[(size_t)OD_VY * n + p];
        const float X = ((R[0] * px + R[1] * py) + R[2] * pz) + tr[0];
        const float Y = ((R[3] * px + R[4] * py) + R[5] * pz) + tr[1];
        const float Z = ((R[6] * px + R[7] * py) + R[8] * pz) + tr[2];
        if (!(Z > 0.0f)) continue;
        const float uf = (fx * X) / Z + cx, vf = (fy * Y) / Z + cy;
        const float u0 = floorf(uf + 0.0009765625f), v0 = floorf(vf + 0.0009765625f);
        if (!(u0 >= 0.0f && u0 < (float)(w - 1) && v0 >= 0.0f && v0 < (float)(h - 1))) continue;      // NaN fails
        OdTaps t;
        t.i00 = (int)v0 * w + (int)u0;
        t.w = w;
        t.a = fminf(fmaxf(uf - u0, 0.0f), 1.0f);
        t.b = fminf(fmaxf(vf - v0, 0.0f), 1.0f);
        const float rD = od_bil(tgt + (size_t)OD_D * n, t) - Z;
        const float hx = od_bil(tgt + (size_t)OD_DX * n, t), hy = od_bil(tgt + (size_t)OD_DY * n, t);
        // a bilinear value is finite exactly when its four taps are: a zero weight does not hide a NaN
        if (!(od_finite(rD) && od_finite(hx) && od_finite(hy) && fabsf(rD) <= trunc)) continue;
        const float rI = od_bil(tgt + (size_t)OD_I * n, t) - src[(size_t)OD_I * n + p];
        const float gx = od_bil(tgt + (size_t)OD_IX * n, t), gy = od_bil(tgt + (size_t)OD_IY * n, t);
        const float iz = 1.0f / Z;
        float JI[6], JD[6];
        {
            const float c0 = (gx * fx) * iz, c1 = (gy * fy) * iz, c2 = -((c0 * X + c1 * Y) * iz);
            JI[0] = -(Z * c1) + Y * c2; JI[1] = Z * c0 - X * c2; JI[2] = -(Y * c0) + X * c1; JI[3] = c0; JI[4] = c1; JI[5] = c2;
        }
        {
            const float c0 = (hx * fx) * iz, c1 = (hy * fy) * iz, c2 = -((c0 * X + c1 * Y) * iz);
            JD[0] = (-(Z * c1) + Y * c2) - Y; JD[1] = (Z * c0 - X * c2) + X; JD[2] = -(Y * c0) + X * c1; JD[3] = c0; JD[4] = c1; JD[5] = c2 - 1.0f;
        }
        const float aI = fabsf(rI), aD = fabsf(rD);
        const float wI = aI <= huber_i ? 1.0f : huber_i / aI, wD = aD <= huber_d ? 1.0f : huber_d / aD;
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const float wi = wI * JI[i], wd = wD * JD[i];
#pragma unroll
            for (int j = i; j < 6; ++j) acc[k++] += wi * JI[j] + wd * JD[j];
            acc[21 + i] += wi * rI + wd * rD;
        }
        acc[27] += (aI <= huber_i ? 0.5f * rI * rI : huber_i * (aI - 0.5f * huber_i)) +
                   (aD <= huber_d ? 0.5f * rD * rD : huber_d * (aD - 0.5f * huber_d));
        acc[28] += 1.0f;
    }

    // lanes -> half-waves by DPP adds (valid in the lanes with bit 4 set), the eight half-wave rows through LDS, added in a fixed order
    const int lane = lk_lane();
#pragma unroll
    for (int k = 0; k < OD_NSUM; ++k) {
        const float s = lk_half_wave_sum(acc[k]);
        if ((lane & 31) == LK_HWS_LANE) s_half[(threadIdx.x >> 6) * 2 + (lane >> 5)][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < OD_ROW) {
        float s = 0.0f;
        if (threadIdx.x < OD_NSUM) {
            s = s_half[0][threadIdx.x];
#pragma unroll
            for (int q = 1; q < 8; ++q) s += s_half[q][threadIdx.x];
        }
        part[(size_t)blockIdx.x * OD_ROW + threadIdx.x] = s;
    }
}

// ------------------------------------------------------------------ one iteration: reduce, solve, update
__global__ __launch_bounds__(64) void k_odom_solve(const float* __restrict__ part, int n_rows, int level, int iter, double* __restrict__ T,
                                                   double* __restrict__ rec) {
    __shared__ double s_sum[OD_ROW];
    const int t = threadIdx.x;
    if (t < OD_ROW) {
        double s = 0.0;
        if (t < OD_NSUM) {
#pragma unroll 4
            for (int g = 0; g < n_rows; ++g) s += (double)part[(size_t)g * OD_ROW + t];
        }
        s_sum[t] = s;
    }
    __syncthreads();
    if (t != 0) return;
    double A[6][6], L[6][6], b[6], x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { A[i][j] = s_sum[k]; A[j][i] = s_sum[k]; ++k; }
    for (int i = 0; i < 6; ++i) b[i] = s_sum[21 + i];
    const double count = s_sum[28];
    bool bad = count < 6.0;
    for (int j = 0; j < 6 && !bad; ++j) {                  // A = L L^T
        double d = A[j][j];
        for (int q = 0; q < j; ++q) d -= L[j][q] * L[j][q];
        if (!(d > 0.0)) { bad = true; break; }             // a NaN pivot too
        const double r = sqrt(d);
        L[j][j] = r;
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            for (int q = 0; q < j; ++q) v -= L[i][q] * L[j][q];
            L[i][j] = v / r;
        }
    }
    double norm = 0.0;
    if (!bad) {
        double yv[6];
        for (int i = 0; i < 6; ++i) {
            double v = -b[i];
            for (int q = 0; q < i; ++q) v -= L[i][q] * yv[q];
            yv[i] = v / L[i][i];
        }
        for (int i = 5; i >= 0; --i) {
            double v = yv[i];
            for (int q = i + 1; q < 6; ++q) v -= L[q][i] * x[q];
            x[i] = v / L[i][i];
        }
        for (int i = 0; i < 6; ++i) norm += x[i] * x[i];
        norm = sqrt(norm);
        bad = !(norm <= DBL_MAX);                            // an overflowed or NaN step is no step
    }
    if (!bad) {
        const double th = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        double ca = 1.0, cb = 0.5;                           // sin(th) / th and (1 - cos(th)) / th^2
        if (th >= 1e-12) { ca = sin(th) / th; cb = (1.0 - cos(th)) / (th * th); }
        const double Kx[3][3] = {{0.0, -x[2], x[1]}, {x[2], 0.0, -x[0]}, {-x[1], x[0], 0.0}};
        double Rm[3][3], Tn[12];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double k2 = 0.0;
                for (int q = 0; q < 3; ++q) k2 += Kx[i][q] * Kx[q][j];
                Rm[i][j] = (i == j ? 1.0 : 0.0) + ca * Kx[i][j] + cb * k2;
            }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) {
                double v = 0.0;
                for (int q = 0; q < 3; ++q) v += Rm[i][q] * T[4 * q + j];
                Tn[4 * i + j] = j == 3 ? v + x[3 + i] : v;
            }
        for (int i = 0; i < 12; ++i) T[i] = Tn[i];
    } else {
        norm = 0.0;
    }
    if (rec != nullptr) {
        rec[0] = (double)level; rec[1] = (double)iter; rec[2] = count; rec[3] = s_sum[27];
        for (int i = 0; i < 27; ++i) rec[4 + i] = s_sum[i];
        rec[31] = norm; rec[32] = bad ? 1.0 : 0.0;
    }
}

// ------------------------------------------------------------------ C ABI
extern "C" int lk_odom_ws_bytes(int32_t H, int32_t W, int32_t n_levels, int64_t* out_layout) {
    LK_REQUIRE(out_layout != nullptr, "lk_odom_ws_bytes: NULL output");
    if (int rc = od_check(H, W, n_levels, "lk_odom_ws_bytes")) return rc;
    const OdLevels L = od_levels(H, W, n_levels);
    out_layout[0] = L.off[LK_ODOM_MAX_LEVELS] * (int64_t)sizeof(float);
    out_layout[1] = (int64_t)OD_MAX_WG * OD_ROW * (int64_t)sizeof(float);
    out_layout[2] = OD_PLANES;
    out_layout[3] = n_levels;
    for (int l = 0; l < LK_ODOM_MAX_LEVELS; ++l) {
        out_layout[4 + l] = L.off[l];
        out_layout[4 + LK_ODOM_MAX_LEVELS + l] = (int64_t)L.h[l] * L.w[l];
    }
    return LK_OK;
}

extern "C" int lk_odom_prepare(const float* color, const float* depth, int32_t H, int32_t W, int32_t n_levels, float fx, float fy, float cx, float cy,
                               float max_depth, float depth_diff, float* pyr, void* stream_) {
    if (int rc = od_check(H, W, n_levels, "lk_odom_prepare")) return rc;
    LK_REQUIRE(color && depth && pyr, "lk_odom_prepare: NULL buffer");
    LK_REQUIRE(fx > 0.0f && fy > 0.0f, "lk_odom_prepare: fx, fy > 0 are required");
    hipStream_t st = (hipStream_t)stream_;
    const OdLevels L = od_levels(H, W, n_levels);
    for (int l = 0; l < n_levels; ++l) {
        const int h = L.h[l], w = L.w[l], n = h * w;
        float* lev = pyr + L.off[l];
        if (l == 0) {
            hipLaunchKernelGGL(k_odom_level0, dim3(lk_cdiv(n, 256)), dim3(256), 0, st, color, depth, n, max_depth, lev + (size_t)OD_I * n,
                               lev + (size_t)OD_D * n);
        } else {
            const int sn = L.h[l - 1] * L.w[l - 1];
            const float* up = pyr + L.off[l - 1];
            hipLaunchKernelGGL(k_odom_down, dim3(lk_cdiv(n, 256)), dim3(256), 0, st, up + (size_t)OD_I * sn, up + (size_t)OD_D * sn, L.h[l - 1],
                               L.w[l - 1], lev + (size_t)OD_I * n, lev + (size_t)OD_D * n, h, w, depth_diff);
        }
        hipLaunchKernelGGL(k_odom_derive, dim3(lk_cdiv(n, 256)), dim3(256), 0, st, lev, h, w, fx, fy, cx, cy);
        fx *= 0.5f; fy *= 0.5f; cx *= 0.5f; cy *= 0.5f;
    }
    LK_LAUNCH_CHECK();
    return LK_OK;
}

extern "C" int lk_odom_estimate(const float* pyr_src, const float* pyr_tgt, int32_t H, int32_t W, int32_t n_levels, float fx, float fy, float cx,
                                float cy, const int32_t* iters, float outlier_trunc, float huber_intensity, float huber_depth, double* T,
                                double* out_log, void* ws, void* stream_) {
    if (int rc = od_check(H, W, n_levels, "lk_odom_estimate")) return rc;
    LK_REQUIRE(pyr_src && pyr_tgt && iters && T && ws, "lk_odom_estimate: NULL buffer");
    LK_REQUIRE(((uintptr_t)ws & 7u) == 0 && ((uintptr_t)T & 7u) == 0 && ((uintptr_t)out_log & 7u) == 0, "lk_odom_estimate: ws, T and out_log must be 8-byte aligned");
    LK_REQUIRE(outlier_trunc > 0.0f && huber_intensity > 0.0f && huber_depth > 0.0f, "lk_odom_estimate: the truncation and the Huber widths must be positive");
    int64_t total = 0;
    for (int i = 0; i < n_levels; ++i) {
        LK_REQUIRE(iters[i] >= 0, "lk_odom_estimate: iters < 0");
        total += iters[i];
    }
    LK_REQUIRE(total <= LK_ODOM_MAX_ITERS, "lk_odom_estimate: too many iterations");
    hipStream_t st = (hipStream_t)stream_;
    const OdLevels L = od_levels(H, W, n_levels);
    float* part = (float*)ws;
    int64_t r = 0;
    for (int li = 0; li < n_levels; ++li) {
        const int l = n_levels - 1 - li;
        const int h = L.h[l], w = L.w[l];
        const float s = ldexpf(1.0f, -l);
        const int rows = min(lk_cdiv((int64_t)h * w, 256), OD_MAX_WG);
        for (int it = 0; it < iters[li]; ++it, ++r) {
            hipLaunchKernelGGL(k_odom_pixels, dim3(rows), dim3(256), 0, st, pyr_src + L.off[l], pyr_tgt + L.off[l], h, w, fx * s, fy * s, cx * s,
                               cy * s, (const double*)T, outlier_trunc, huber_intensity, huber_depth, part);
            hipLaunchKernelGGL(k_odom_solve, dim3(1), dim3(64), 0, st, (const float*)part, rows, l, it, T,
                               out_log ? out_log + r * LK_ODOM_REC : (double*)nullptr);
        }
    }
    LK_LAUNCH_CHECK();
    return LK_OK;
}
