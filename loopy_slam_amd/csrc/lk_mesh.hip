// Reconstruction evaluation of a finished mesh: what the reference does on the host with trimesh, Open3D and scipy at the end of every
// experiment (src/tools/cull_mesh.py, src/tools/eval_recon.py) -
//   lk_nearest                 exact nearest target point of every query over the uniform grid, bounded or unbounded (cKDTree.query)
//   lk_mesh_areas              triangle areas, the weights of the surface sampler
//   lk_mesh_sample             area-weighted surface samples from a counter-based generator (trimesh.sample.sample_surface)
//   lk_mesh_cull               which points project into at least one camera of a trajectory (cull_mesh.py, eval_recon.py check_proj)
//   lk_mesh_depth_setup / lk_mesh_depth_raster
//                              z-depth image of a triangle mesh (Open3D's off-screen depth capture)
// The buffers are the caller's (loopy_slam_amd/mesh_eval.py).  fp32 throughout except the sampler's cumulative area table (fp64).  The only
// atomic is the z-buffer's 32-bit unsigned minimum on the bit pattern of a positive depth, which does not depend on the arrival order:
// equal inputs (and an equal seed) give equal bits everywhere.
#include "lk_common.h"
#include "lk_knn_dev.h"
#include "lk_reg_dev.h"
#include "lk_philox_dev.h"
#include "lk_kernels.h"

#include <math.h>

struct LkMeshMat12 { float m[12]; };                // row-major 3 x 4, passed by value

// ------------------------------------------------------------------ exact nearest neighbour
// The growing-box form of lk_nearest_coop (lk_reg.hip): eight lanes per query, one (d2, index) key per lane, a min-butterfly per round.  Round
// r walks the box of half-width h_r (h_0 just under one cell edge, h_{r+1} = 2 h_r, never beyond the caller's bound); a box holds every
// point within h of the query, so a hit with d2 <= h^2 (1 - 1e-6) is nearer than anything outside it and ends the search, as does a box
// that covers the whole grid or has reached the bound.  Every round walks its whole box again - the minimum does not mind meeting a
// candidate twice, and with doubling half-widths the earlier boxes add a seventh to the last one.  The butterfly and the vote that ends the
// loop are executed by every lane of the wave in every round (groups that are done idle through them), so no collective sits under
// divergent control flow.
#define LK_NEAREST_ROUNDS 160                       // 2^160 overflows fp32: an infinite half-width covers every grid

__device__ __forceinline__ uint64_t lk_mesh_min8(uint64_t k) {
    uint64_t o = lk_dpp_u64<0xB1>(k); k = o < k ? o : k;
    o = lk_dpp_u64<0x4E>(k); k = o < k ? o : k;
    o = lk_dpp_u64<0x141>(k); k = o < k ? o : k;
    return k;
}

__global__ __launch_bounds__(256) void k_nearest(const LkGrid* __restrict__ G, const float4* __restrict__ sorted,
                                                 const int32_t* __restrict__ cell_start, const float* __restrict__ q, int P, float r2,
                                                 float* __restrict__ out_d2, int32_t* __restrict__ out_idx) {
    const int qi_raw = blockIdx.x * LK_REG_GROUPS + (int)threadIdx.x / LK_REG_T;
    const int sub = (int)threadIdx.x % LK_REG_T;
    const bool live = qi_raw < P;
    const int i = live ? qi_raw : P - 1;                 // dead groups shadow the last query
    const float qx = q[3 * (size_t)i], qy = q[3 * (size_t)i + 1], qz = q[3 * (size_t)i + 2];
    const bool bounded = r2 < INFINITY;
    const float rfull = bounded ? lk_box_halfwidth(r2) : INFINITY;
    float h = fminf(G->cell * 0.9999f - 1e-6f, rfull);
    if (!(h > 0.0f)) h = rfull;                          // a cell edge below 1e-6 (never built by lk_knn_build's callers)
    uint64_t best = LK_KEY_EMPTY;
    bool done = G->n <= 0;
#pragma unroll 1
    for (int round = 0; round < LK_NEAREST_ROUNDS; ++round) {
        bool last = false;
        if (!done) {
            const LkGridBox b = lk_grid_box(G, qx, qy, qz, h);
            lk_box_rows(G, cell_start, b, [&](int s, int e) {
#pragma unroll 1
                for (int t = s + sub; t < e; t += LK_REG_T) {
                    const float4 p = sorted[t];
                    const float d2 = lk_dist2(qx, qy, qz, p.x, p.y, p.z);
                    const uint64_t key = lk_key(d2, __float_as_int(p.w));
                    if (d2 <= r2 && key < best) best = key;
                }
            });
            last = h >= rfull || (b.any && b.ix0 == 0 && b.iy0 == 0 && b.iz0 == 0 && b.ix1 == G->dx - 1 && b.iy1 == G->dy - 1 && b.iz1 == G->dz - 1);
        }
        best = lk_mesh_min8(best);
        // (every lane of the group holds the same key, query and half-width: the decision is group-uniform)
        if (!done) {
            done = last || (best != LK_KEY_EMPTY && __uint_as_float((uint32_t)(best >> 32)) <= h * h * (1.0f - 1e-6f));
            h = fminf(h * 2.0f, rfull);
        }
        if (!__any(!done)) break;
    }
    if (live && sub == 0) {
        const bool hit = best != LK_KEY_EMPTY;
        out_idx[i] = hit ? (int)(uint32_t)best : -1;
        out_d2[i] = hit ? __uint_as_float((uint32_t)(best >> 32)) : INFINITY;
    }
}

extern "C" int lk_nearest(lk_knn_t knn, const float* queries, int64_t P, float max_dist, float* out_d2, int32_t* out_idx, void* stream_) {
    LK_REQUIRE(knn != nullptr, "lk_nearest: NULL index");
    LK_REQUIRE(P >= 0 && P < (1ll << 31), "lk_nearest: P out of range");
    LK_REQUIRE(max_dist > 0.0f, "lk_nearest: max_dist must be > 0 (infinity: unbounded)");
    if (P == 0) return LK_OK;
    LK_REQUIRE(queries && out_d2 && out_idx, "lk_nearest: NULL buffer");
    const float r2 = isinf(max_dist) ? INFINITY : max_dist * max_dist;
    hipLaunchKernelGGL(k_nearest, dim3(lk_cdiv(P, LK_REG_GROUPS)), dim3(256), 0, (hipStream_t)stream_, (const LkGrid*)knn->grid,
                       (const float4*)knn->sorted, (const int32_t*)knn->cell_start, queries, (int)P, r2, out_d2, out_idx);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

// ------------------------------------------------------------------ surface sampling
// the three corners of face f, or false if an index lies outside [0, V)
__device__ __forceinline__ bool lk_mesh_corners(const float* __restrict__ verts, int V, const int32_t* __restrict__ faces, int f, float (&p)[3][3]) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = faces[3 * (size_t)f + c];
        const bool in = v >= 0 && v < V;
        ok = ok && in;
#pragma unroll
        for (int a = 0; a < 3; ++a) p[c][a] = in ? verts[3 * (size_t)v + a] : 0.0f;
    }
    return ok;
}

__global__ __launch_bounds__(256) void k_mesh_areas(const float* __restrict__ verts, int V, const int32_t* __restrict__ faces, int F,
                                                    float* __restrict__ out_area) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    float p[3][3];
    float area = 0.0f;
    if (lk_mesh_corners(verts, V, faces, f, p)) {
        const float ax = __fsub_rn(p[1][0], p[0][0]), ay = __fsub_rn(p[1][1], p[0][1]), az = __fsub_rn(p[1][2], p[0][2]);
        const float bx = __fsub_rn(p[2][0], p[0][0]), by = __fsub_rn(p[2][1], p[0][1]), bz = __fsub_rn(p[2][2], p[0][2]);
        const float cx = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by)), cy = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz)),
                    cz = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
        area = __fmul_rn(0.5f, sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(cx, cx), __fmul_rn(cy, cy)), __fmul_rn(cz, cz))));
        if (!(area >= 0.0f) || isinf(area)) area = 0.0f;                 // a NaN or overflowing face is never sampled
    }
    out_area[f] = area;
}

extern "C" int lk_mesh_areas(const float* verts, int64_t V, const int32_t* faces, int64_t F, float* out_area, void* stream_) {
    LK_REQUIRE(V >= 0 && V < (1ll << 31) && F >= 0 && 3 * F < (1ll << 31), "lk_mesh_areas: bad sizes");
    if (F == 0) return LK_OK;
    LK_REQUIRE(faces && out_area && (V == 0 || verts), "lk_mesh_areas: NULL buffer");
    hipLaunchKernelGGL(k_mesh_areas, dim3(lk_cdiv(F, 256)), dim3(256), 0, (hipStream_t)stream_, verts, (int)V, faces, (int)F, out_area);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

// u = (r + 0.5) / 2^32 in fp32: the conversion, the add and the multiply each rounded once; in (0, 1]
__device__ __forceinline__ float lk_mesh_unit(uint32_t r) { return __fmul_rn(__fadd_rn((float)r, 0.5f), 2.3283064365386963e-10f); }

__global__ __launch_bounds__(256) void k_mesh_sample(const float* __restrict__ verts, int V, const int32_t* __restrict__ faces, int F,
                                                     const double* __restrict__ cum, uint32_t seed_lo, uint32_t seed_hi, int S,
                                                     float* __restrict__ out_pos, int32_t* __restrict__ out_face, float* __restrict__ out_bary) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= S) return;
    uint32_t r[4];
    lk_philox(seed_lo, seed_hi, (uint32_t)k, 0u, r);
    const double target = (((double)r[0] + 0.5) * 2.3283064365386963e-10) * cum[F - 1];
    int lo = 0, hi = F - 1;                              // the first f with cum[f] > target
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > target) hi = mid; else lo = mid + 1;
    }
    const float a = sqrtf(lk_mesh_unit(r[1])), b = lk_mesh_unit(r[2]);
    const float w0 = __fsub_rn(1.0f, a), w1 = __fmul_rn(a, __fsub_rn(1.0f, b)), w2 = __fmul_rn(a, b);
    float p[3][3];
    lk_mesh_corners(verts, V, faces, lo, p);
    out_face[k] = lo;
    out_bary[3 * (size_t)k] = w0; out_bary[3 * (size_t)k + 1] = w1; out_bary[3 * (size_t)k + 2] = w2;
#pragma unroll
    for (int c = 0; c < 3; ++c) out_pos[3 * (size_t)k + c] = __fmaf_rn(w0, p[0][c], __fmaf_rn(w1, p[1][c], __fmul_rn(w2, p[2][c])));
}

extern "C" int lk_mesh_sample(const float* verts, int64_t V, const int32_t* faces, int64_t F, const double* cum_area, uint64_t seed,
                              int64_t S, float* out_pos, int32_t* out_face, float* out_bary, void* stream_) {
    LK_REQUIRE(V > 0 && V < (1ll << 31) && F > 0 && 3 * F < (1ll << 31), "lk_mesh_sample: an empty mesh has no surface to sample");
    LK_REQUIRE(S >= 0 && 3 * S < (1ll << 31), "lk_mesh_sample: S out of range");
    if (S == 0) return LK_OK;
    LK_REQUIRE(verts && faces && cum_area && out_pos && out_face && out_bary, "lk_mesh_sample: NULL buffer");
    hipLaunchKernelGGL(k_mesh_sample, dim3(lk_cdiv(S, 256)), dim3(256), 0, (hipStream_t)stream_, verts, (int)V, faces, (int)F, cum_area,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (int)S, out_pos, out_face, out_bary);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

// ------------------------------------------------------------------ frustum culling
// Workgroup (x, y): 256 points against the slice of LK_CULL_POSES poses y; a point seen by a pose of the slice stores a 1 (idempotent, the
// caller zeroes the bytes).  The slice's matrices are read through the scalar cache (the pose index is uniform).
#define LK_CULL_POSES 64

__global__ __launch_bounds__(256) void k_mesh_cull(const float* __restrict__ pts, int N, const float* __restrict__ w2c, int n_poses, float fW,
                                                   float fH, float fx, float fy, float cx, float cy, uint8_t* __restrict__ seen) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
    const int k0 = blockIdx.y * LK_CULL_POSES, k1 = min(k0 + LK_CULL_POSES, n_poses);
    bool any = false;
#pragma unroll 1
    for (int k = k0; k < k1 && !any; ++k) {
        float x, y, z;
        lk_rigid_apply(w2c + 12 * (size_t)k, px, py, pz, x, y, z);
        const float zz = __fadd_rn(z, 1e-5f);
        const float u = __fadd_rn(__fmul_rn(fx, -x), __fmul_rn(cx, z)) / zz, v = __fadd_rn(__fmul_rn(fy, y), __fmul_rn(cy, z)) / zz;
        any = 0.0f <= -zz && u < fW && u > 0.0f && v < fH && v > 0.0f;
    }
    if (any) seen[i] = 1;
}

extern "C" int lk_mesh_cull(const float* points, int64_t N, const float* w2c, int32_t n_poses, int32_t H, int32_t W, float fx, float fy,
                            float cx, float cy, uint8_t* seen, void* stream_) {
    LK_REQUIRE(N >= 0 && N < (1ll << 31) / 3 && n_poses >= 0 && n_poses <= 65535 * LK_CULL_POSES && H > 0 && W > 0, "lk_mesh_cull: bad sizes");
    if (N == 0 || n_poses == 0) return LK_OK;
    LK_REQUIRE(points && w2c && seen, "lk_mesh_cull: NULL buffer");
    hipLaunchKernelGGL(k_mesh_cull, dim3(lk_cdiv(N, 256), lk_cdiv(n_poses, LK_CULL_POSES)), dim3(256), 0, (hipStream_t)stream_, points, (int)N,
                       w2c, (int)n_poses, (float)W, (float)H, fx, fy, cx, cy, seen);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

// ------------------------------------------------------------------ depth rasteriser
// Camera space: x right, y down, z forward (the host turns the project's camera into it as lk_tsdf_integrate does).  The ray of pixel (row i,
// column j) is the line through the origin with direction d = ((j - cx) / fx, (i - cy) / fy, 1), so its parameter IS the z-depth.
//
// Set-up, one thread per triangle: the corners a, b, c in camera space; the normals of the three planes through the origin and one edge,
// e.g. (b - c) x c = b x c for the edge opposite a - the pixel is inside the triangle's cone iff d has the same sign against all three -
// each formed from the edge's corners in ascending vertex order and negated if that reverses the edge, so that two triangles sharing an
// edge test it with the same bits (no crack, no gap); and the triangle's own plane n = (b - a) x (c - a), k = n . a.  Nothing is projected
// there, so a triangle that crosses the camera plane needs no clipping for the test itself; only its screen box does: the box is taken over
// the projections of the corners with z >= near and of the points where an edge crosses z = near, half a pixel added on every side, and cut
// to the image.  The box is counted in 8 x 8-pixel tiles of the image's tile grid.
// Raster, one wave per tile of the work list (the inclusive prefix sum of the tile counts locates the triangle by bisection): lane = pixel.
#define LK_TILE 8
#define LK_DEPTH_REC 16                             // floats per triangle record: na, nb, nc, n (3 each), k, 3 unused
#define LK_DEPTH_EMPTY 0xffffffffu

struct LkDepthCam { float fx, fy, cx, cy, near, far; int H, W; };

__device__ __forceinline__ void lk_cross(const float* u, const float* v, float* o) {
    o[0] = __fsub_rn(__fmul_rn(u[1], v[2]), __fmul_rn(u[2], v[1]));
    o[1] = __fsub_rn(__fmul_rn(u[2], v[0]), __fmul_rn(u[0], v[2]));
    o[2] = __fsub_rn(__fmul_rn(u[0], v[1]), __fmul_rn(u[1], v[0]));
}
// p x q for the cone plane of the edge p -> q, canonical in the vertex order: (p - q) x q if ip < iq, else -((q - p) x p)
__device__ __forceinline__ void lk_edge_plane(const float* p, int ip, const float* q, int iq, float* o) {
    const bool fwd = ip < iq;
    const float* lo = fwd ? p : q;
    const float* hi = fwd ? q : p;
    const float e[3] = {__fsub_rn(lo[0], hi[0]), __fsub_rn(lo[1], hi[1]), __fsub_rn(lo[2], hi[2])};
    lk_cross(e, hi, o);
    if (!fwd) { o[0] = -o[0]; o[1] = -o[1]; o[2] = -o[2]; }
}

__global__ __launch_bounds__(256) void k_mesh_depth_setup(const float* __restrict__ verts, int V, const int32_t* __restrict__ faces, int F,
                                                          LkMeshMat12 M, LkDepthCam cam, float* __restrict__ rec, int32_t* __restrict__ box,
                                                          int32_t* __restrict__ ntiles) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    float w[3][3], p[3][3];
    bool ok = lk_mesh_corners(verts, V, faces, f, w);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lk_rigid_apply(M.m, w[c][0], w[c][1], w[c][2], p[c][0], p[c][1], p[c][2]);
        ok = ok && fabsf(p[c][0]) < LK_FLT_MAX && fabsf(p[c][1]) < LK_FLT_MAX && fabsf(p[c][2]) < LK_FLT_MAX;      // finite
    }
    const float zmin = fminf(p[0][2], fminf(p[1][2], p[2][2])), zmax = fmaxf(p[0][2], fmaxf(p[1][2], p[2][2]));
    ok = ok && zmax >= cam.near && zmin <= cam.far;
    int tx0 = 0, ty0 = 0, ntx = 0, nty = 0;
    if (ok) {
        float umin = LK_FLT_MAX, umax = -LK_FLT_MAX, vmin = LK_FLT_MAX, vmax = -LK_FLT_MAX;
        auto take = [&](float x, float y, float z) {
            const float u = __fadd_rn(__fmul_rn(cam.fx, x) / z, cam.cx), v = __fadd_rn(__fmul_rn(cam.fy, y) / z, cam.cy);
            umin = fminf(umin, u); umax = fmaxf(umax, u); vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
        };
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int n = (c + 1) % 3;
            if (p[c][2] >= cam.near) take(p[c][0], p[c][1], p[c][2]);
            if ((p[c][2] >= cam.near) != (p[n][2] >= cam.near)) {
                const float s = __fsub_rn(cam.near, p[c][2]) / __fsub_rn(p[n][2], p[c][2]);
                take(__fadd_rn(p[c][0], __fmul_rn(s, __fsub_rn(p[n][0], p[c][0]))), __fadd_rn(p[c][1], __fmul_rn(s, __fsub_rn(p[n][1], p[c][1]))),
                     cam.near);
            }
        }
        // half a pixel of margin, then cut to the image (the clamps come first: the float -> int conversions stay in range; a NaN
        // projection fails the comparison and leaves the box empty)
        const float fW = (float)cam.W, fH = (float)cam.H;
        umin = fmaxf(__fsub_rn(umin, 0.5f), 0.0f); umax = fminf(__fadd_rn(umax, 0.5f), fW - 1.0f);
        vmin = fmaxf(__fsub_rn(vmin, 0.5f), 0.0f); vmax = fminf(__fadd_rn(vmax, 0.5f), fH - 1.0f);
        if (umin <= umax && vmin <= vmax) {
            tx0 = (int)floorf(umin) / LK_TILE; ty0 = (int)floorf(vmin) / LK_TILE;
            ntx = (int)ceilf(umax) / LK_TILE - tx0 + 1; nty = (int)ceilf(vmax) / LK_TILE - ty0 + 1;
        }
    }
    float* r = rec + (size_t)f * LK_DEPTH_REC;
    const int ia = ok ? faces[3 * (size_t)f] : 0, ib = ok ? faces[3 * (size_t)f + 1] : 0, ic = ok ? faces[3 * (size_t)f + 2] : 0;
    lk_edge_plane(p[1], ib, p[2], ic, r);                // b x c
    lk_edge_plane(p[2], ic, p[0], ia, r + 3);            // c x a
    lk_edge_plane(p[0], ia, p[1], ib, r + 6);            // a x b
    const float e1[3] = {__fsub_rn(p[1][0], p[0][0]), __fsub_rn(p[1][1], p[0][1]), __fsub_rn(p[1][2], p[0][2])};
    const float e2[3] = {__fsub_rn(p[2][0], p[0][0]), __fsub_rn(p[2][1], p[0][1]), __fsub_rn(p[2][2], p[0][2])};
    lk_cross(e1, e2, r + 9);
    r[12] = __fadd_rn(__fadd_rn(__fmul_rn(r[9], p[0][0]), __fmul_rn(r[10], p[0][1])), __fmul_rn(r[11], p[0][2]));
    r[13] = 0.0f; r[14] = 0.0f; r[15] = 0.0f;
    box[4 * (size_t)f] = tx0; box[4 * (size_t)f + 1] = ty0; box[4 * (size_t)f + 2] = ntx; box[4 * (size_t)f + 3] = nty;
    ntiles[f] = ntx * nty;
}

__global__ __launch_bounds__(256) void k_mesh_depth_fill(uint32_t* __restrict__ zbuf, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) zbuf[i] = LK_DEPTH_EMPTY;
}

__global__ __launch_bounds__(256) void k_mesh_depth_raster(const float* __restrict__ rec, const int32_t* __restrict__ box,
                                                           const int32_t* __restrict__ tile_end, int F, int T, LkDepthCam cam,
                                                           uint32_t* __restrict__ zbuf) {
    const int g = blockIdx.x * 4 + ((int)threadIdx.x >> 6);          // tile of the work list: one per wave
    if (g >= T) return;
    int lo = 0, hi = F - 1;                              // the first triangle with tile_end > g (wave-uniform)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tile_end[mid] > g) hi = mid; else lo = mid + 1;
    }
    const int f = lo;
    const int tx0 = box[4 * (size_t)f], ty0 = box[4 * (size_t)f + 1], ntx = box[4 * (size_t)f + 2], nty = box[4 * (size_t)f + 3];
    const int local = g - (tile_end[f] - ntx * nty);
    if (local < 0 || local >= ntx * nty) return;          // a prefix that is not the one of these boxes
    const int lane = lk_lane();
    const int j = (tx0 + local % ntx) * LK_TILE + (lane & (LK_TILE - 1)), i = (ty0 + local / ntx) * LK_TILE + lane / LK_TILE;
    if (i >= cam.H || j >= cam.W) return;
    const float4* r4 = reinterpret_cast<const float4*>(rec + (size_t)f * LK_DEPTH_REC);
    const float4 r0 = r4[0], r1 = r4[1], r2 = r4[2], r3 = r4[3];
    const float dx = __fsub_rn((float)j, cam.cx) / cam.fx, dy = __fsub_rn((float)i, cam.cy) / cam.fy;
    const float wa = __fadd_rn(__fadd_rn(__fmul_rn(r0.x, dx), __fmul_rn(r0.y, dy)), r0.z);
    const float wb = __fadd_rn(__fadd_rn(__fmul_rn(r0.w, dx), __fmul_rn(r1.x, dy)), r1.y);
    const float wc = __fadd_rn(__fadd_rn(__fmul_rn(r1.z, dx), __fmul_rn(r1.w, dy)), r2.x);
    const bool inside = (wa >= 0.0f && wb >= 0.0f && wc >= 0.0f) || (wa <= 0.0f && wb <= 0.0f && wc <= 0.0f);
    if (!inside) return;
    const float nd = __fadd_rn(__fadd_rn(__fmul_rn(r2.y, dx), __fmul_rn(r2.z, dy)), r2.w);
    const float z = r3.x / nd;
    if (!(z >= cam.near && z <= cam.far)) return;        // also false for nd = 0 (a triangle seen edge-on) and for a NaN
    atomicMin(zbuf + (size_t)i * cam.W + j, __float_as_uint(z));
}

// in place: the bit pattern of the nearest depth, or 0 where no triangle was met
__global__ __launch_bounds__(256) void k_mesh_depth_resolve(uint32_t* __restrict__ zbuf, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && zbuf[i] == LK_DEPTH_EMPTY) zbuf[i] = 0u;
}

static int lk_depth_cam(int32_t H, int32_t W, float fx, float fy, float cx, float cy, float near, float far, LkDepthCam* cam) {
    LK_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) && fx != 0.0f && fy != 0.0f && near > 0.0f && far >= near && far < INFINITY,
               "lk_mesh_depth: bad image size, focal length or depth range");
    cam->fx = fx; cam->fy = fy; cam->cx = cx; cam->cy = cy; cam->near = near; cam->far = far; cam->H = H; cam->W = W;
    return LK_OK;
}

extern "C" int lk_mesh_depth_setup(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* host_w2c12, int32_t H, int32_t W,
                                   float fx, float fy, float cx, float cy, float near, float far, float* out_rec, int32_t* out_box,
                                   int32_t* out_ntiles, float* out_depth, void* stream_) {
    LkDepthCam cam;
    const int rc = lk_depth_cam(H, W, fx, fy, cx, cy, near, far, &cam);
    if (rc != LK_OK) return rc;
    LK_REQUIRE(V >= 0 && V < (1ll << 31) && F >= 0 && LK_DEPTH_REC * F < (1ll << 31) && host_w2c12 != nullptr, "lk_mesh_depth_setup: bad arguments");
    LK_REQUIRE(out_depth != nullptr, "lk_mesh_depth_setup: NULL depth image");
    hipStream_t st = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_mesh_depth_fill, dim3(lk_cdiv((int64_t)H * W, 256)), dim3(256), 0, st, reinterpret_cast<uint32_t*>(out_depth), H * W);
    if (F > 0) {
        LK_REQUIRE(faces && out_rec && out_box && out_ntiles && (V == 0 || verts), "lk_mesh_depth_setup: NULL buffer");
        LkMeshMat12 M;
        for (int k = 0; k < 12; ++k) M.m[k] = host_w2c12[k];
        hipLaunchKernelGGL(k_mesh_depth_setup, dim3(lk_cdiv(F, 256)), dim3(256), 0, st, verts, (int)V, faces, (int)F, M, cam, out_rec, out_box,
                           out_ntiles);
    }
    LK_LAUNCH_CHECK();
    return LK_OK;
}

extern "C" int lk_mesh_depth_raster(const float* rec, const int32_t* box, const int32_t* tile_end, int64_t F, int64_t T, int32_t H, int32_t W,
                                    float fx, float fy, float cx, float cy, float near, float far, float* depth, void* stream_) {
    LkDepthCam cam;
    const int rc = lk_depth_cam(H, W, fx, fy, cx, cy, near, far, &cam);
    if (rc != LK_OK) return rc;
    LK_REQUIRE(F >= 0 && LK_DEPTH_REC * F < (1ll << 31) && T >= 0 && T < (1ll << 31), "lk_mesh_depth_raster: bad sizes");
    LK_REQUIRE(depth != nullptr, "lk_mesh_depth_raster: NULL depth image");
    hipStream_t st = (hipStream_t)stream_;
    if (F > 0 && T > 0) {
        LK_REQUIRE(rec && box && tile_end, "lk_mesh_depth_raster: NULL buffer");
        hipLaunchKernelGGL(k_mesh_depth_raster, dim3(lk_cdiv(T, 4)), dim3(256), 0, st, rec, box, tile_end, (int)F, (int)T, cam,
                           reinterpret_cast<uint32_t*>(depth));
    }
    hipLaunchKernelGGL(k_mesh_depth_resolve, dim3(lk_cdiv((int64_t)H * W, 256)), dim3(256), 0, st, reinterpret_cast<uint32_t*>(depth), H * W);
    LK_LAUNCH_CHECK();
    return LK_OK;
}
