// Frame preparation (include/loopy_hip.h, "frame preparation"): the decoded bytes of an RGB-D frame -> the float colour and depth images the
// trackers and mappers consume - what the reference's reader does on the CPU behind cv2.imread (src/utils/datasets.py:95-119).
// tests/datasets_referee.py states the same contract in NumPy float64.
//
//   k_frame_undistort   uint8 -> uint8 colour, cv2's fixed-point remap restated (1/32-pixel coordinates, integer weights that sum to 2^15)
//   k_frame_stream      no resampling (Replica, TUM as configured): four consecutive output pixels per lane, 12 bytes of colour and 8 of depth in,
//                       three 16-byte colour stores and one depth store out; the tail of a row and unaligned rows go pixel by pixel
//   k_frame_resample    colour resize to the depth size and / or crop_size: one output pixel per lane, taps composed on the fly through L2
// At most two launches per frame, on the caller's stream; nothing is allocated and nothing synchronises.  6.5 MB move at 640 x 480: the
// kernels are launch-bound and use no LDS; the stream kernel needs a dozen registers, so occupancy is not a question.
#include "lk_common.h"

#include <math.h>

struct FrameArgs {
    const uint8_t* color;          // [Hc][Wc][3], after the undistortion if there was one
    const void* depth;             // [Hd][Wd] uint16 or float
    float* out_color;              // [Ho][Wo][3]
    float* out_depth;              // [Ho][Wo]
    int Hc, Wc, Hd, Wd;
    int Hb, Wb;                    // the image crop_edge cuts: crop_size, else the depth size
    int Ho, Wo, e;
    int bgr, depth_f32, resize, crop, vec_ok;
    float depth_scale;
    float near_y, near_x;          // fp32(in / out) of the nearest-neighbour depth
};

// two taps of one axis and the weight of the second
struct FrameLin { int i0, i1; float f; };

// align_corners: source = dst (in - 1) / (out - 1); cell and remainder in integers, one rounding in the fraction
__device__ __forceinline__ FrameLin fr_corners(int dst, int in, int out) {
    const int n = dst * (in - 1), d = out - 1;
    const int i0 = n / d, r = n - i0 * d;
    FrameLin L;
    L.i0 = i0;
    L.i1 = min(i0 + 1, in - 1);
    L.f = (float)r / (float)d;
    return L;
}

// pixel centres (cv2 INTER_LINEAR): source = (dst + 0.5) in / out - 0.5 = ((2 dst + 1) in - out) / (2 out), clamped to [0, in - 1]
__device__ __forceinline__ FrameLin fr_centres(int dst, int in, int out) {
    const int n = (2 * dst + 1) * in - out, d = 2 * out;
    FrameLin L;
    if (n <= 0) { L.i0 = 0; L.i1 = 0; L.f = 0.0f; return L; }
    const int i0 = n / d;
    if (i0 >= in - 1) { L.i0 = in - 1; L.i1 = in - 1; L.f = 0.0f; return L; }
    L.i0 = i0;
    L.i1 = i0 + 1;
    L.f = (float)(n - i0 * d) / (float)d;
    return L;
}

__device__ __forceinline__ float fr_bilinear(float p00, float p01, float p10, float p11, float fx, float fy) {
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    return gy * (gx * p00 + fx * p01) + fy * (gx * p10 + fx * p11);
}

__device__ __forceinline__ float fr_unit(uint8_t c) { return (float)c / 255.0f; }

__device__ __forceinline__ float fr_depth(const FrameArgs& a, int y, int x) {
    const size_t i = (size_t)y * a.Wd + x;
    const float d = a.depth_f32 ? reinterpret_cast<const float*>(a.depth)[i] : (float)reinterpret_cast<const uint16_t*>(a.depth)[i];
    return d / a.depth_scale;
}

// ------------------------------------------------------------------ undistortion (uint8 -> uint8)
__global__ __launch_bounds__(256) void k_frame_undistort(const uint8_t* __restrict__ src, int H, int W, double fx, double fy, double cx, double cy,
                                                         double k1, double k2, double p1, double p2, double k3, uint8_t* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    const int v = i / W, u = i - v * W;
    const double x = ((double)u - cx) / fx, y = ((double)v - cy) / fy;
    const double r2 = x * x + y * y, r4 = r2 * r2;
    const double rad = ((1.0 + k1 * r2) + k2 * r4) + k3 * (r4 * r2);
    const double xd = (x * rad + ((2.0 * p1) * x) * y) + p2 * (r2 + (2.0 * x) * x);
    const double yd = (y * rad + p1 * (r2 + (2.0 * y) * y)) + ((2.0 * p2) * x) * y;
    const double lim = 1073741824.0;           // 2^30 / 32 pixels: far outside any image, keeps the conversion defined
    const int qx = (int)fmin(fmax(rint((fx * xd + cx) * 32.0), -lim), lim);
    const int qy = (int)fmin(fmax(rint((fy * yd + cy) * 32.0), -lim), lim);
    const int ix = qx >> 5, iy = qy >> 5, ax = qx & 31, ay = qy & 31;
    const int w00 = 32 * (32 - ay) * (32 - ax), w01 = 32 * (32 - ay) * ax, w10 = 32 * ay * (32 - ax), w11 = 32 * ay * ax;
    const bool y0 = iy >= 0 && iy < H, y1 = iy + 1 >= 0 && iy + 1 < H, x0 = ix >= 0 && ix < W, x1 = ix + 1 >= 0 && ix + 1 < W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int s = 1 << 14;
        if (y0 && x0) s += w00 * src[((size_t)iy * W + ix) * 3 + c];
        if (y0 && x1) s += w01 * src[((size_t)iy * W + ix + 1) * 3 + c];
        if (y1 && x0) s += w10 * src[((size_t)(iy + 1) * W + ix) * 3 + c];
        if (y1 && x1) s += w11 * src[((size_t)(iy + 1) * W + ix + 1) * 3 + c];
        dst[(size_t)i * 3 + c] = (uint8_t)(s >> 15);
    }
}

// ------------------------------------------------------------------ the streaming conversion
__global__ __launch_bounds__(256) void k_frame_stream(const FrameArgs a) {
    const int quads = (a.Wo + 3) >> 2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.Ho * quads) return;
    const int oy = i / quads, ox = (i - oy * quads) * 4;
    const size_t src = (size_t)(oy + a.e) * a.Wd + (ox + a.e), dst = (size_t)oy * a.Wo + ox;      // pixel indices
    const int n = min(4, a.Wo - ox);
    const int r = a.bgr ? 2 : 0, b = 2 - r;
    if (n == 4 && a.vec_ok && ((src | dst) & 3) == 0) {
        const uint32_t* cw = reinterpret_cast<const uint32_t*>(a.color + src * 3);
        const uint32_t w0 = cw[0], w1 = cw[1], w2 = cw[2];
        uint8_t c[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c[k] = (uint8_t)(w0 >> (8 * k));
            c[4 + k] = (uint8_t)(w1 >> (8 * k));
            c[8 + k] = (uint8_t)(w2 >> (8 * k));
        }
        float f[12];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            f[3 * p + 0] = fr_unit(c[3 * p + r]);
            f[3 * p + 1] = fr_unit(c[3 * p + 1]);
            f[3 * p + 2] = fr_unit(c[3 * p + b]);
        }
        float4* oc = reinterpret_cast<float4*>(a.out_color + dst * 3);
        oc[0] = make_float4(f[0], f[1], f[2], f[3]);
        oc[1] = make_float4(f[4], f[5], f[6], f[7]);
        oc[2] = make_float4(f[8], f[9], f[10], f[11]);
        float4 d;
        if (a.depth_f32) {
            d = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(a.depth) + src);
        } else {
            const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(a.depth) + src);
            d = make_float4((float)(h.x & 0xffffu), (float)(h.x >> 16), (float)(h.y & 0xffffu), (float)(h.y >> 16));
        }
        *reinterpret_cast<float4*>(a.out_depth + dst) = make_float4(d.x / a.depth_scale, d.y / a.depth_scale, d.z / a.depth_scale, d.w / a.depth_scale);
        return;
    }
    // the tail of a row (n < 4) and rows whose bytes are not aligned for the wide accesses
    for (int p = 0; p < n; ++p) {
        const uint8_t* c = a.color + (src + p) * 3;
        float* o = a.out_color + (dst + p) * 3;
        o[0] = fr_unit(c[r]);
        o[1] = fr_unit(c[1]);
        o[2] = fr_unit(c[b]);
        a.out_depth[dst + p] = fr_depth(a, oy + a.e, ox + a.e + p);
    }
}

// ------------------------------------------------------------------ resize and / or crop_size
// colour of pixel (y, x) of the depth-size image, channel offset ch into the stored bytes
__device__ __forceinline__ float fr_sized(const FrameArgs& a, const FrameLin& Y, const FrameLin& X, int ch) {
    const uint8_t* c = a.color + ch;
    const float p00 = fr_unit(c[((size_t)Y.i0 * a.Wc + X.i0) * 3]);
    if (!a.resize) return p00;
    return fr_bilinear(p00, fr_unit(c[((size_t)Y.i0 * a.Wc + X.i1) * 3]), fr_unit(c[((size_t)Y.i1 * a.Wc + X.i0) * 3]),
                       fr_unit(c[((size_t)Y.i1 * a.Wc + X.i1) * 3]), X.f, Y.f);
}

__device__ __forceinline__ FrameLin fr_axis(const FrameArgs& a, int i, int in, int out) {
    if (a.resize) return fr_centres(i, in, out);
    FrameLin L;
    L.i0 = L.i1 = i;
    L.f = 0.0f;
    return L;
}

__global__ __launch_bounds__(256) void k_frame_resample(const FrameArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.Ho * a.Wo) return;
    const int oy = i / a.Wo, ox = i - oy * a.Wo;
    const int by = oy + a.e, bx = ox + a.e;                  // in the image crop_edge cuts
    float* o = a.out_color + (size_t)i * 3;
    if (a.crop) {
        const FrameLin CY = fr_corners(by, a.Hd, a.Hb), CX = fr_corners(bx, a.Wd, a.Wb);
        const FrameLin Y0 = fr_axis(a, CY.i0, a.Hc, a.Hd), Y1 = fr_axis(a, CY.i1, a.Hc, a.Hd);
        const FrameLin X0 = fr_axis(a, CX.i0, a.Wc, a.Wd), X1 = fr_axis(a, CX.i1, a.Wc, a.Wd);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int ch = a.bgr ? 2 - c : c;
            o[c] = fr_bilinear(fr_sized(a, Y0, X0, ch), fr_sized(a, Y0, X1, ch), fr_sized(a, Y1, X0, ch), fr_sized(a, Y1, X1, ch), CX.f, CY.f);
        }
        const int sy = min((int)floorf((float)by * a.near_y), a.Hd - 1), sx = min((int)floorf((float)bx * a.near_x), a.Wd - 1);
        a.out_depth[i] = fr_depth(a, sy, sx);
    } else {
        const FrameLin Y = fr_axis(a, by, a.Hc, a.Hd), X = fr_axis(a, bx, a.Wc, a.Wd);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = fr_sized(a, Y, X, a.bgr ? 2 - c : c);
        a.out_depth[i] = fr_depth(a, by, bx);
    }
}

// ------------------------------------------------------------------ entry
extern "C" int lk_frame_prepare(const uint8_t* color, int32_t Hc, int32_t Wc, const void* depth, int32_t Hd, int32_t Wd, uint32_t flags,
                                float png_depth_scale, double fx, double fy, double cx, double cy, const double* distortion, int32_t crop_h,
                                int32_t crop_w, int32_t crop_edge, uint8_t* undist, float* out_color, float* out_depth, void* stream_) {
    LK_REQUIRE(color && depth, "lk_frame_prepare: NULL input buffer");
    LK_REQUIRE(Hc >= 1 && Wc >= 1 && Hd >= 1 && Wd >= 1 && Hc <= LK_FRAME_MAX_DIM && Wc <= LK_FRAME_MAX_DIM && Hd <= LK_FRAME_MAX_DIM &&
                   Wd <= LK_FRAME_MAX_DIM, "lk_frame_prepare: image sizes of 1 .. LK_FRAME_MAX_DIM are required");
    LK_REQUIRE((flags & ~(LK_FRAME_BGR | LK_FRAME_DEPTH_F32)) == 0, "lk_frame_prepare: unknown flag bits");
    LK_REQUIRE(png_depth_scale > 0.0f && png_depth_scale <= LK_FLT_MAX, "lk_frame_prepare: png_depth_scale must be finite and > 0");
    LK_REQUIRE(crop_h >= 0 && crop_w >= 0 && crop_h <= LK_FRAME_MAX_DIM && crop_w <= LK_FRAME_MAX_DIM && (crop_h == 0) == (crop_w == 0),
               "lk_frame_prepare: crop_size is two sizes of 1 .. LK_FRAME_MAX_DIM, or 0, 0 for none");
    LK_REQUIRE(crop_h != 1 && crop_w != 1, "lk_frame_prepare: crop_size with a dimension of 1 has no align_corners scale");
    const bool crop = crop_h > 0;
    const int Hb = crop ? crop_h : Hd, Wb = crop ? crop_w : Wd;
    LK_REQUIRE(crop_edge >= 0 && 2 * (int64_t)crop_edge < Hb && 2 * (int64_t)crop_edge < Wb, "lk_frame_prepare: crop_edge leaves no pixels");
    LK_REQUIRE(out_color && out_depth, "lk_frame_prepare: NULL output buffer");
    hipStream_t st = (hipStream_t)stream_;

    bool distorted = false;
    if (distortion)
        for (int k = 0; k < 5; ++k) distorted |= distortion[k] != 0.0;
    if (distorted) {
        LK_REQUIRE(undist != nullptr, "lk_frame_prepare: a distortion needs the undist buffer");
        LK_REQUIRE(fx != 0.0 && fy != 0.0, "lk_frame_prepare: fx and fy must not be 0 with a distortion");
        hipLaunchKernelGGL(k_frame_undistort, dim3(lk_cdiv((int64_t)Hc * Wc, 256)), dim3(256), 0, st, color, Hc, Wc, fx, fy, cx, cy, distortion[0],
                           distortion[1], distortion[2], distortion[3], distortion[4], undist);
        color = undist;
    }

    FrameArgs a;
    a.color = color; a.depth = depth; a.out_color = out_color; a.out_depth = out_depth;
    a.Hc = Hc; a.Wc = Wc; a.Hd = Hd; a.Wd = Wd; a.Hb = Hb; a.Wb = Wb;
    a.e = crop_edge; a.Ho = Hb - 2 * crop_edge; a.Wo = Wb - 2 * crop_edge;
    a.bgr = (flags & LK_FRAME_BGR) != 0; a.depth_f32 = (flags & LK_FRAME_DEPTH_F32) != 0;
    a.resize = Hc != Hd || Wc != Wd;
    a.crop = crop && (crop_h != Hd || crop_w != Wd);         // crop_size equal to the depth size: every fraction is 0, the stage is the identity
    a.depth_scale = png_depth_scale;
    a.near_y = (float)Hd / (float)Hb; a.near_x = (float)Wd / (float)Wb;
    a.vec_ok = ((uintptr_t)color % 4 == 0) && ((uintptr_t)depth % 16 == 0) && ((uintptr_t)out_color % 16 == 0) && ((uintptr_t)out_depth % 16 == 0);
    if (!a.resize && !a.crop)
        hipLaunchKernelGGL(k_frame_stream, dim3(lk_cdiv((int64_t)a.Ho * ((a.Wo + 3) / 4), 256)), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(k_frame_resample, dim3(lk_cdiv((int64_t)a.Ho * a.Wo, 256)), dim3(256), 0, st, a);
    LK_LAUNCH_CHECK();
    return LK_OK;
}
