// Rendering evaluation of one frame pair (include/loopy_hip.h "rendering evaluation"): the masked depth-L1 and colour sums behind the
// reference's depth L1 and PSNR, and the per-level, per-channel means of the SSIM and contrast-structure maps behind its MS-SSIM
// (src/Mapper.py:1120-1160 around pytorch_msssim) -
//   k_img_level   one launch per pyramid level: a workgroup owns a 32 x 32 region of the level's image in one channel, stages it with a
//                 10-pixel halo behind it, filters (columns, then rows, as the package does), forms both maps, reduces them to one partial
//                 per workgroup and writes its share of the 2 x 2-pooled next level; the first level also takes the masked sums
//   k_img_reduce  one workgroup per record entry sums that entry's partials in a fixed order
// No floating-point atomic: equal inputs give equal bits.  The workspace is written before it is read, every call.
//
// LDS: two staged tiles [42][42] (X and Y) and five filtered planes [32][42] (G applied down the columns of X, Y, XX, YY, XY), 41 152 bytes
// with the reduction scratch: three workgroups per compute unit of 160 KB.  Every pass walks its elements with consecutive lanes on consecutive floats
// (a wave covers 64 consecutive elements of a row-major plane, or two 32-float row pieces in the last pass), so each 32-lane group of a
// ds_read_b32 / ds_write_b32 meets 32 different banks whatever the row pitch is: the pitch is the tile width, 42, with no padding.
#include "lk_common.h"

#include <math.h>

#define LK_IMG_TX 32
#define LK_IMG_TY 32
#define LK_IMG_WIN 11
#define LK_IMG_HALO (LK_IMG_WIN - 1)
#define LK_IMG_TW (LK_IMG_TX + LK_IMG_HALO)
#define LK_IMG_TH (LK_IMG_TY + LK_IMG_HALO)
#define LK_IMG_LEVELS 5
#define LK_IMG_KINDS 5                               // partials per workgroup: n_valid, depth sum, colour sum, SSIM sum, cs sum
#define LK_IMG_MASKED 1
#define LK_IMG_SSIM 2

struct LkImgWin { float g[LK_IMG_WIN]; float c1, c2; };

struct LkImgLevel {
    const float* x; const float* y;                  // element (c, i, j) at c * chan + i * row + j * pix
    int64_t chan; int32_t row, pix;
    int32_t h, w;
    float* nx; float* ny;                            // next level, planar [3][h2][w2]; NULL at the last level
    int32_t h2, w2;
    double* part;                                    // [LK_IMG_KINDS][workgroups], workgroup (c, by, bx) at (c * gy + by) * gx + bx
    int32_t mode;
};

struct LkImgEntries {                                // the partials behind every record entry: part[off .. off + n), divided by div
    int64_t off[LK_IMG_REC]; int32_t n[LK_IMG_REC]; double div[LK_IMG_REC];
};

__device__ __forceinline__ double lk_img_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(256) void k_img_level(LkImgLevel L, LkImgWin Wn, const float* __restrict__ gt_depth, const float* __restrict__ depth) {
    __shared__ float s_x[LK_IMG_TH * LK_IMG_TW], s_y[LK_IMG_TH * LK_IMG_TW];
    __shared__ float s_pl[5][LK_IMG_TY * LK_IMG_TW];
    __shared__ double s_red[4][LK_IMG_KINDS];
    const int t = (int)threadIdx.x, c = (int)blockIdx.z;
    const int i0 = (int)blockIdx.y * LK_IMG_TY, j0 = (int)blockIdx.x * LK_IMG_TX;
    const int h = L.h, w = L.w;
    double acc[LK_IMG_KINDS] = {0.0, 0.0, 0.0, 0.0, 0.0};

    if (L.mode & LK_IMG_MASKED) {
        // the difference is one fp32 subtraction (torch's); widened, it is squared or made absolute and added in fp64
#pragma unroll 1
        for (int p = t; p < LK_IMG_TY * LK_IMG_TX; p += 256) {
            const int i = i0 + p / LK_IMG_TX, j = j0 + p % LK_IMG_TX;
            if (i < h && j < w) {
                const size_t q = (size_t)i * w + j;
                const float gd = gt_depth[q];
                if (gd > 0.0f) {
                    const double dc = (double)__fsub_rn(L.x[3 * q + c], L.y[3 * q + c]);
                    acc[2] += dc * dc;
                    if (c == 0) {
                        acc[0] += 1.0;
                        acc[1] += fabs((double)__fsub_rn(gd, depth[q]));
                    }
                }
            }
        }
    }

    if (L.mode & LK_IMG_SSIM) {
        // the tile: rows i0 .. i0 + 41, columns j0 .. j0 + 41 of channel c, zero beyond the image
#pragma unroll 1
        for (int p = t; p < LK_IMG_TH * LK_IMG_TW; p += 256) {
            const int i = i0 + p / LK_IMG_TW, j = j0 + p % LK_IMG_TW;
            float a = 0.0f, b = 0.0f;
            if (i < h && j < w) {
                const size_t q = (size_t)c * L.chan + (size_t)i * L.row + (size_t)j * L.pix;
                a = L.x[q]; b = L.y[q];
            }
            s_x[p] = a; s_y[p] = b;
        }
        __syncthreads();

        // the next level: pixel (i2, j2) = a quarter of the 2 x 2 block that starts at row 2 i2 - (h & 1), column 2 j2 - (w & 1); row or
        // column -1 is the padding (zeros that count).  The workgroup whose region holds the block's first row and column writes it (the
        // one at the image's edge also those that start at -1); the block's second row and column lie in the halo at the latest.
        if (L.nx != nullptr) {
            const int ph = h & 1, pw = w & 1;
#pragma unroll 1
            for (int p = t; p < (LK_IMG_TY / 2 + 1) * (LK_IMG_TX / 2 + 1); p += 256) {
                const int i2 = i0 / 2 + p / (LK_IMG_TX / 2 + 1), j2 = j0 / 2 + p % (LK_IMG_TX / 2 + 1);
                const int r0 = 2 * i2 - ph, c0 = 2 * j2 - pw;
                const bool mine = (r0 >= i0 || r0 < 0) && r0 < i0 + LK_IMG_TY && (c0 >= j0 || c0 < 0) && c0 < j0 + LK_IMG_TX && i2 < L.h2 && j2 < L.w2;
                if (mine) {
                    float sx = 0.0f, sy = 0.0f;
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const int r = r0 + (d >> 1), cc = c0 + (d & 1);
                        const bool in = r >= 0 && cc >= 0;
                        const int at = in ? (r - i0) * LK_IMG_TW + (cc - j0) : 0;
                        sx = __fadd_rn(sx, in ? s_x[at] : 0.0f);
                        sy = __fadd_rn(sy, in ? s_y[at] : 0.0f);
                    }
                    const size_t q = ((size_t)c * L.h2 + i2) * L.w2 + j2;
                    L.nx[q] = __fmul_rn(sx, 0.25f); L.ny[q] = __fmul_rn(sy, 0.25f);
                }
            }
        }

        // G down the columns: plane[i][s] = sum_k g[k] tile[i + k][s], i < 32, s < 42
#pragma unroll 1
        for (int p = t; p < LK_IMG_TY * LK_IMG_TW; p += 256) {
            float mx = 0.0f, my = 0.0f, mxx = 0.0f, myy = 0.0f, mxy = 0.0f;
#pragma unroll
            for (int k = 0; k < LK_IMG_WIN; ++k) {
                const float g = Wn.g[k], a = s_x[p + k * LK_IMG_TW], b = s_y[p + k * LK_IMG_TW];
                mx = __fadd_rn(mx, __fmul_rn(g, a));
                my = __fadd_rn(my, __fmul_rn(g, b));
                mxx = __fadd_rn(mxx, __fmul_rn(g, __fmul_rn(a, a)));
                myy = __fadd_rn(myy, __fmul_rn(g, __fmul_rn(b, b)));
                mxy = __fadd_rn(mxy, __fmul_rn(g, __fmul_rn(a, b)));
            }
            s_pl[0][p] = mx; s_pl[1][p] = my; s_pl[2][p] = mxx; s_pl[3][p] = myy; s_pl[4][p] = mxy;
        }
        __syncthreads();

        // G along the rows, the two maps, their sums over the map pixels of this region
        const int mh = h - LK_IMG_HALO, mw = w - LK_IMG_HALO;
#pragma unroll 1
        for (int p = t; p < LK_IMG_TY * LK_IMG_TX; p += 256) {
            const int i = p / LK_IMG_TX, j = p % LK_IMG_TX;
            if (i0 + i < mh && j0 + j < mw) {
                float f[5];
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    float s = 0.0f;
#pragma unroll
                    for (int k = 0; k < LK_IMG_WIN; ++k) s = __fadd_rn(s, __fmul_rn(Wn.g[k], s_pl[q][i * LK_IMG_TW + j + k]));
                    f[q] = s;
                }
                const float mu11 = __fmul_rn(f[0], f[0]), mu22 = __fmul_rn(f[1], f[1]), mu12 = __fmul_rn(f[0], f[1]);
                const float s1 = __fsub_rn(f[2], mu11), s2 = __fsub_rn(f[3], mu22), s12 = __fsub_rn(f[4], mu12);
                const float cs = __fadd_rn(__fmul_rn(2.0f, s12), Wn.c2) / __fadd_rn(__fadd_rn(s1, s2), Wn.c2);
                const float ss = __fmul_rn(__fadd_rn(__fmul_rn(2.0f, mu12), Wn.c1) / __fadd_rn(__fadd_rn(mu11, mu22), Wn.c1), cs);
                acc[3] += (double)ss;
                acc[4] += (double)cs;
            }
        }
    }

    // one partial per kind and workgroup: lanes, then waves, in a fixed order
#pragma unroll
    for (int k = 0; k < LK_IMG_KINDS; ++k) {
        const double s = lk_img_wave_sum(acc[k]);
        if (lk_lane() == 0) s_red[t >> 6][k] = s;
    }
    __syncthreads();
    if (t < LK_IMG_KINDS) {
        const size_t nb = (size_t)gridDim.x * gridDim.y * gridDim.z;
        const size_t b = ((size_t)c * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        L.part[(size_t)t * nb + b] = ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t];
    }
}

__global__ __launch_bounds__(256) void k_img_reduce(const double* __restrict__ part, LkImgEntries E, int first, double* __restrict__ out) {
    __shared__ double s_sum[256];
    const int t = (int)threadIdx.x, e = first + (int)blockIdx.x;
    const double* p = part + E.off[e];
    const int n = E.n[e];
    double s = 0.0;
#pragma unroll 1
    for (int k = t; k < n; k += 256) s += p[k];
    s_sum[t] = s;
    __syncthreads();
#pragma unroll 1
    for (int m = 128; m >= 1; m >>= 1) {
        if (t < m) s_sum[t] += s_sum[t + m];
        __syncthreads();
    }
    if (t == 0) out[e] = s_sum[0] / E.div[e];
}

// ------------------------------------------------------------------ host
struct LkImgPlan {
    int h[LK_IMG_LEVELS], w[LK_IMG_LEVELS], gx[LK_IMG_LEVELS], gy[LK_IMG_LEVELS];
    int64_t part_off[LK_IMG_LEVELS];                 // in doubles
    int64_t plane_off[LK_IMG_LEVELS];                // in bytes; X of level l (l >= 1), Y follows it
    int64_t bytes;
};

static void lk_img_plan(int H, int W, LkImgPlan* P) {
    int64_t doubles = 0;
    for (int l = 0; l < LK_IMG_LEVELS; ++l) {
        P->h[l] = l ? (P->h[l - 1] + 1) / 2 : H;
        P->w[l] = l ? (P->w[l - 1] + 1) / 2 : W;
        P->gx[l] = lk_cdiv(P->w[l], LK_IMG_TX);
        P->gy[l] = lk_cdiv(P->h[l], LK_IMG_TY);
        P->part_off[l] = doubles;
        doubles += (int64_t)LK_IMG_KINDS * 3 * P->gx[l] * P->gy[l];
    }
    int64_t bytes = doubles * (int64_t)sizeof(double);
    P->plane_off[0] = 0;
    for (int l = 1; l < LK_IMG_LEVELS; ++l) {
        P->plane_off[l] = bytes;
        bytes += 2 * 3 * (int64_t)P->h[l] * P->w[l] * (int64_t)sizeof(float);
    }
    P->bytes = bytes;
}

extern "C" int lk_img_eval_ws_bytes(int32_t H, int32_t W, int64_t* out_bytes) {
    LK_REQUIRE(H > 0 && W > 0 && 3 * (int64_t)H * W < (1ll << 31) && out_bytes != nullptr, "lk_img_eval_ws_bytes: bad image size");
    LkImgPlan P;
    lk_img_plan(H, W, &P);
    *out_bytes = P.bytes;
    return LK_OK;
}

extern "C" int lk_img_eval(const float* gt_color, const float* color, const float* gt_depth, const float* depth, int32_t H, int32_t W,
                           int32_t with_msssim, void* ws, double* out_rec, void* stream_) {
    LK_REQUIRE(H > 0 && W > 0 && 3 * (int64_t)H * W < (1ll << 31), "lk_img_eval: bad image size");
    LK_REQUIRE(gt_color && color && gt_depth && depth && ws && out_rec, "lk_img_eval: NULL buffer");
    LK_REQUIRE(((uintptr_t)ws & 7) == 0, "lk_img_eval: the workspace must be 8-byte aligned");
    LK_REQUIRE(!with_msssim || (H > 160 && W > 160), "lk_img_eval: MS-SSIM is defined for min(H, W) > 160 only");
    hipStream_t st = (hipStream_t)stream_;
    LkImgPlan P;
    lk_img_plan(H, W, &P);
    LkImgWin Wn;
    double g[LK_IMG_WIN], sum = 0.0;
    for (int k = 0; k < LK_IMG_WIN; ++k) { g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5)); sum += g[k]; }
    for (int k = 0; k < LK_IMG_WIN; ++k) Wn.g[k] = (float)(g[k] / sum);
    Wn.c1 = (float)(0.01 * 0.01); Wn.c2 = (float)(0.03 * 0.03);

    double* part = reinterpret_cast<double*>(ws);
    LkImgEntries E;
    for (int e = 0; e < LK_IMG_REC; ++e) { E.off[e] = 0; E.n[e] = 0; E.div[e] = 1.0; }
    const int nb0 = P.gx[0] * P.gy[0];               // workgroups of one channel of level 0; channel 0 comes first
    E.off[0] = 0;                       E.n[0] = nb0;
    E.off[1] = (int64_t)3 * nb0;        E.n[1] = nb0;
    E.off[2] = (int64_t)2 * 3 * nb0;    E.n[2] = 3 * nb0;
    const int levels = with_msssim ? LK_IMG_LEVELS : 1;
    for (int l = 0; l < levels; ++l) {
        LkImgLevel L;
        const int nb = P.gx[l] * P.gy[l];
        if (l == 0) {
            L.x = gt_color; L.y = color; L.chan = 1; L.row = 3 * W; L.pix = 3;
        } else {
            L.x = reinterpret_cast<const float*>((char*)ws + P.plane_off[l]);
            L.y = L.x + 3 * (size_t)P.h[l] * P.w[l];
            L.chan = (int64_t)P.h[l] * P.w[l]; L.row = P.w[l]; L.pix = 1;
        }
        L.h = P.h[l]; L.w = P.w[l];
        L.nx = nullptr; L.ny = nullptr; L.h2 = 0; L.w2 = 0;
        if (l + 1 < levels) {
            L.nx = reinterpret_cast<float*>((char*)ws + P.plane_off[l + 1]);
            L.ny = L.nx + 3 * (size_t)P.h[l + 1] * P.w[l + 1];
            L.h2 = P.h[l + 1]; L.w2 = P.w[l + 1];
        }
        L.part = part + P.part_off[l];
        L.mode = (l == 0 ? LK_IMG_MASKED : 0) | (with_msssim ? LK_IMG_SSIM : 0);
        hipLaunchKernelGGL(k_img_level, dim3(P.gx[l], P.gy[l], 3), dim3(256), 0, st, L, Wn, gt_depth, depth);
        if (with_msssim) {
            const double pixels = (double)(P.h[l] - LK_IMG_HALO) * (double)(P.w[l] - LK_IMG_HALO);
            for (int c = 0; c < 3; ++c)
                for (int cs = 0; cs < 2; ++cs) {
                    const int e = 3 + 6 * l + 3 * cs + c;
                    E.off[e] = P.part_off[l] + (int64_t)(3 + cs) * 3 * nb + (int64_t)c * nb;
                    E.n[e] = nb; E.div[e] = pixels;
                }
        }
    }
    hipLaunchKernelGGL(k_img_reduce, dim3(with_msssim ? LK_IMG_REC : 3), dim3(256), 0, st, (const double*)part, E, 0, out_rec);
    LK_LAUNCH_CHECK();
    return LK_OK;
}
