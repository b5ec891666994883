// Loop closure, geometric back end: the per-point work of registering two map segments and of moving the map afterwards.
// Replaces what the reference does per loop trigger with Open3D on the host (src/common.py: pairwise_registration,
// register_point_cloud_pair, estimate_normals; src/neural_point.py: apply_transformation):
//   lk_normals           radius-neighbourhood covariance -> smallest eigenvector, oriented to a camera centre
//   lk_icp_accumulate    one Gauss-Newton step's sums of point-to-plane ICP (optionally Tukey-weighted), or the sums of the
//                        correspondence information matrix
//   lk_apply_correction  p <- R[seg] p + t[seg] over the whole cloud
// Every search goes through the exact uniform-grid index (lk_knn.hip, under the contract of lk_knn_dev.h), so the correspondence of a source point is THE nearest target
// point under the index's total order (d2, index) and does not depend on the grid's cell order.
//
// Reductions are repeatable: a lane adds the terms of its queries in query order, the wave combines lanes with a fixed xor butterfly, the
// workgroup adds its four waves in wave order and stores ONE row of LK_REG_OUT partials; a second one-workgroup launch adds the rows in
// row order in fp64.  No floating-point atomics anywhere.
//
// Shared with lk_greg.hip: the radius box and its row walk (lk_knn_dev.h: lk_grid_box, lk_box_rows), the 8-lane group, the rigid map and
// the Jacobi rotation (lk_reg_dev.h).
#include "lk_common.h"
#include "lk_knn_dev.h"
#include "lk_reg_dev.h"
#include "lk_kernels.h"

#define LK_REG_QPW 128                              // queries per workgroup: the grid follows the point count

struct LkMat12 { float m[12]; };                    // row-major 3 x 4, passed by value

// ------------------------------------------------------------------ normals
// unit eigenvector of the smallest eigenvalue of the symmetric matrix (xx xy xz; . yy yz; . . zz): cyclic Jacobi, fp32
__device__ __forceinline__ void lk_smallest_eigvec(float xx, float xy, float xz, float yy, float yz, float zz, float& nx, float& ny, float& nz) {
    const float tr = xx + yy + zz;
    const float sc = tr > 0.0f ? 1.0f / tr : 0.0f;
    float a[3][3] = {{xx * sc, xy * sc, xz * sc}, {xy * sc, yy * sc, yz * sc}, {xz * sc, yz * sc, zz * sc}};
    float v[3][3] = {{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}};
#pragma unroll 1
    for (int sweep = 0; sweep < 8; ++sweep) {
        lk_jacobi_rot<3, 0, 1>(a, v);
        lk_jacobi_rot<3, 0, 2>(a, v);
        lk_jacobi_rot<3, 1, 2>(a, v);
    }
    const float l0 = a[0][0], l1 = a[1][1], l2 = a[2][2];
    const bool p0 = l0 <= l1 && l0 <= l2, p1 = !p0 && l1 <= l2;
    nx = p0 ? v[0][0] : (p1 ? v[0][1] : v[0][2]);
    ny = p0 ? v[1][0] : (p1 ? v[1][1] : v[1][2]);
    nz = p0 ? v[2][0] : (p1 ? v[2][1] : v[2][2]);
    const float inv = rsqrtf(nx * nx + ny * ny + nz * nz);
    nx *= inv; ny *= inv; nz *= inv;
}

// one 8-lane group per point: every point of the index with d2 <= r2 (the point itself included) enters the sums, taken relative
// to the point so that the covariance does not cancel against the room's coordinates
__global__ __launch_bounds__(256) void k_normals(const LkGrid* __restrict__ G, const float4* __restrict__ sorted,
                                                 const int32_t* __restrict__ cell_start, const float* __restrict__ pos, int N, float r2,
                                                 float cx, float cy, float cz, float* __restrict__ out_n, uint8_t* __restrict__ out_valid) {
    const int qi_raw = blockIdx.x * LK_REG_GROUPS + (int)threadIdx.x / LK_REG_T;
    const int sub = (int)threadIdx.x % LK_REG_T;
    const bool live = qi_raw < N;
    const int i = live ? qi_raw : N - 1;
    const float qx = pos[3 * (size_t)i], qy = pos[3 * (size_t)i + 1], qz = pos[3 * (size_t)i + 2];
    float cnt = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sxx = 0.0f, sxy = 0.0f, sxz = 0.0f, syy = 0.0f, syz = 0.0f, szz = 0.0f;
    lk_box_rows(G, cell_start, lk_grid_box(G, qx, qy, qz, lk_box_halfwidth(r2)), [&](int s, int e) {
#pragma unroll 1
        for (int t = s + sub; t < e; t += LK_REG_T) {
            const float4 p = sorted[t];
            if (lk_dist2(qx, qy, qz, p.x, p.y, p.z) <= r2) {
                const float ax = p.x - qx, ay = p.y - qy, az = p.z - qz;
                cnt += 1.0f;
                sx += ax; sy += ay; sz += az;
                sxx += ax * ax; sxy += ax * ay; sxz += ax * az;
                syy += ay * ay; syz += ay * az; szz += az * az;
            }
        }
    });
    cnt = lk_sum8(cnt);
    sx = lk_sum8(sx); sy = lk_sum8(sy); sz = lk_sum8(sz);
    sxx = lk_sum8(sxx); sxy = lk_sum8(sxy); sxz = lk_sum8(sxz);
    syy = lk_sum8(syy); syz = lk_sum8(syz); szz = lk_sum8(szz);
    if (!live || sub != 0) return;
    const bool valid = cnt >= 3.0f;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (valid) {
        const float in = 1.0f / cnt;
        const float mx = sx * in, my = sy * in, mz = sz * in;
        lk_smallest_eigvec(sxx * in - mx * mx, sxy * in - mx * my, sxz * in - mx * mz, syy * in - my * my, syz * in - my * mz,
                           szz * in - mz * mz, nx, ny, nz);
        if (nx * (cx - qx) + ny * (cy - qy) + nz * (cz - qz) < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    }
    out_n[3 * (size_t)i] = nx; out_n[3 * (size_t)i + 1] = ny; out_n[3 * (size_t)i + 2] = nz;
    out_valid[i] = valid ? 1 : 0;
}

extern "C" int lk_normals(lk_knn_t knn, const float* pos, int64_t N, float radius, const float* host_camera3, float* out_normals,
                          uint8_t* out_valid, void* stream_) {
    LK_REQUIRE(knn != nullptr, "lk_normals: NULL index");
    LK_REQUIRE(N == knn->n, "lk_normals: N is not the size of the index (build it over pos first)");
    LK_REQUIRE(radius > 0.0f && host_camera3 != nullptr, "lk_normals: bad radius or NULL camera centre");
    if (N == 0) return LK_OK;
    LK_REQUIRE(pos && out_normals && out_valid, "lk_normals: NULL buffer");
    hipLaunchKernelGGL(k_normals, dim3(lk_cdiv(N, LK_REG_GROUPS)), dim3(256), 0, (hipStream_t)stream_, (const LkGrid*)knn->grid,
                       (const float4*)knn->sorted, (const int32_t*)knn->cell_start, pos, (int)N, radius * radius, host_camera3[0],
                       host_camera3[1], host_camera3[2], out_normals, out_valid);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

// ------------------------------------------------------------------ nearest-1 search
// The nearest-1 specialisation of lk_knn_scan_coop (same contract: candidates d2 <= r2, order (d2, index) as one 64-bit key): a lane keeps
// ONE key instead of a sorted list of eight, and the group meets in exactly two min-butterflies that every lane of the wave executes - the
// walks between them hold no collective, so groups of one wave may leave them at different times.  Two phases as there: the box of just
// under one cell edge first; a point found inside it is nearer than anything outside it, and only a query without one walks the full box.
__device__ __forceinline__ uint64_t lk_group_min8(uint64_t k) {
    uint64_t o = lk_dpp_u64<0xB1>(k); k = o < k ? o : k;
    o = lk_dpp_u64<0x4E>(k); k = o < k ? o : k;
    o = lk_dpp_u64<0x141>(k); k = o < k ? o : k;
    return k;
}

__device__ __forceinline__ uint64_t lk_nearest_coop(const LkGrid* __restrict__ G, const float4* __restrict__ sorted,
                                                    const int32_t* __restrict__ cell_start, float qx, float qy, float qz, float r2, int sub) {
    uint64_t best = LK_KEY_EMPTY;
    const float rfull = lk_box_halfwidth(r2);
    const float cellf = G->cell;
    const bool big = rfull > cellf * 1.05f;
    const float r = big ? cellf * 0.9999f - 1e-6f : rfull;
    auto walk = [&](int s, int e) {
#pragma unroll 1
        for (int t = s + sub; t < e; t += LK_REG_T) {
            const float4 p = sorted[t];
            const float d2 = lk_dist2(qx, qy, qz, p.x, p.y, p.z);
            const uint64_t key = lk_key(d2, __float_as_int(p.w));
            if (d2 <= r2 && key < best) best = key;
        }
    };
    const LkGridBox b1 = lk_grid_box(G, qx, qy, qz, r);
    lk_box_rows(G, cell_start, b1, walk);
    best = lk_group_min8(best);
    // (every lane of the group holds the same key here, so the decision is group-uniform)
    const bool done = !big || (best != LK_KEY_EMPTY && __uint_as_float((uint32_t)(best >> 32)) <= r * r * (1.0f - 1e-6f));
    if (!done) {
        // the full box minus what phase 1 has seen: [ix0, ix1] of the rows of its box (an empty phase-1 box has no rows)
        const LkGridBox bf = lk_grid_box(G, qx, qy, qz, rfull);
        const int dx = G->dx, dy = G->dy;
        auto part = [&](int row, int xa, int xb) {
            if (xa <= xb) walk(cell_start[row + xa], cell_start[row + xb + 1]);
        };
#pragma unroll 1
        for (int iz = bf.iz0; iz <= bf.iz1; ++iz) {
#pragma unroll 1
            for (int iy = bf.iy0; iy <= bf.iy1; ++iy) {
                const int row = (iz * dy + iy) * dx;
                const bool seen = iz >= b1.iz0 && iz <= b1.iz1 && iy >= b1.iy0 && iy <= b1.iy1;
                if (!seen) part(row, bf.ix0, bf.ix1);
                else { part(row, bf.ix0, b1.ix0 - 1); part(row, b1.ix1 + 1, bf.ix1); }
            }
        }
    }
    return lk_group_min8(best);
}

// ------------------------------------------------------------------ ICP sums
// Slot s of a row of partials: 0..20 the upper triangle of the 6 x 6 matrix, row by row; 21..26 J^T r; 27 count; 28 sum d2; 29 sum w r^2;
// 30, 31 unused (zero).  Lane `sub` of a query's group owns slots 4 sub .. 4 sub + 3.
__global__ __launch_bounds__(256) void k_icp_accumulate(const LkGrid* __restrict__ G, const float4* __restrict__ sorted,
                                                        const int32_t* __restrict__ cell_start, const float* __restrict__ tgt_pos,
                                                        const float* __restrict__ tgt_nrm, const uint8_t* __restrict__ tgt_valid,
                                                        const float* __restrict__ src, int P, LkMat12 M, float r2, float tukey_k, int mode,
                                                        int32_t* __restrict__ out_corr, float* __restrict__ partials) {
    __shared__ float red[4][LK_REG_OUT];
    const int sub = (int)threadIdx.x % LK_REG_T, group = (int)threadIdx.x / LK_REG_T;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int pass = 0; pass < LK_REG_QPW / LK_REG_GROUPS; ++pass) {
        const int qi_raw = blockIdx.x * LK_REG_QPW + pass * LK_REG_GROUPS + group;
        const bool live = qi_raw < P;
        const int i = live ? qi_raw : P - 1;             // dead groups shadow the last query (the search's collectives stay convergent)
        const float px = src[3 * (size_t)i], py = src[3 * (size_t)i + 1], pz = src[3 * (size_t)i + 2];
        float sx, sy, sz;
        lk_rigid_apply(M.m, px, py, pz, sx, sy, sz);
        const uint64_t key = lk_nearest_coop(G, sorted, cell_start, sx, sy, sz, r2, sub);
        const int j = (int)(uint32_t)key;                // -1 when the key is the empty one
        const float d2 = __uint_as_float((uint32_t)(key >> 32));
        if (live && out_corr && sub == 0) out_corr[i] = j;
        float v[LK_REG_OUT];
#pragma unroll
        for (int s = 0; s < LK_REG_OUT; ++s) v[s] = 0.0f;
        if (live && j >= 0) {
            const float qx = tgt_pos[3 * (size_t)j], qy = tgt_pos[3 * (size_t)j + 1], qz = tgt_pos[3 * (size_t)j + 2];
            if (mode == LK_ICP_INFORMATION) {
                // G = [-[q]x | I]: rows (0, qz, -qy, 1, 0, 0), (-qz, 0, qx, 0, 1, 0), (qy, -qx, 0, 0, 0, 1)
                const float g[3][6] = {{0.0f, qz, -qy, 1.0f, 0.0f, 0.0f}, {-qz, 0.0f, qx, 0.0f, 1.0f, 0.0f}, {qy, -qx, 0.0f, 0.0f, 0.0f, 1.0f}};
                int s = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = a; b < 6; ++b, ++s) v[s] = g[0][a] * g[0][b] + g[1][a] * g[1][b] + g[2][a] * g[2][b];
                v[27] = 1.0f;
                v[28] = d2;
            } else if (tgt_valid[j]) {
                const float nx = tgt_nrm[3 * (size_t)j], ny = tgt_nrm[3 * (size_t)j + 1], nz = tgt_nrm[3 * (size_t)j + 2];
                const float r = nx * (sx - qx) + ny * (sy - qy) + nz * (sz - qz);
                const float J[6] = {sy * nz - sz * ny, sz * nx - sx * nz, sx * ny - sy * nx, nx, ny, nz};
                float w = 1.0f;
                if (tukey_k > 0.0f) {
                    const float u = r / tukey_k, h = 1.0f - u * u;
                    w = fabsf(r) <= tukey_k ? h * h : 0.0f;
                }
                int s = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = a; b < 6; ++b, ++s) v[s] = w * J[a] * J[b];
#pragma unroll
                for (int a = 0; a < 6; ++a) v[21 + a] = w * J[a] * r;
                v[27] = 1.0f;
                v[28] = d2;
                v[29] = w * r * r;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float x = 0.0f;
#pragma unroll
            for (int s = 0; s < LK_REG_T; ++s) x = sub == s ? v[4 * s + q] : x;
            acc[q] += x;
        }
    }
    // lanes with the same `sub` hold partials of the same four slots: xor butterfly over the wave's eight groups
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[q] += __shfl_xor(acc[q], 8);
        acc[q] += __shfl_xor(acc[q], 16);
        acc[q] += __shfl_xor(acc[q], 32);
    }
    const int lane = lk_lane(), wave = (int)threadIdx.x >> 6;
    if (lane < LK_REG_T) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave][4 * lane + q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < LK_REG_OUT) {
        const int t = (int)threadIdx.x;
        partials[(size_t)blockIdx.x * LK_REG_OUT + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    }
}

// rows of partials -> LK_REG_OUT doubles, in a fixed order: thread (slot c, strand s) adds rows s, s + 8, ... ascending, then thread c adds
// the eight strands ascending
__global__ __launch_bounds__(256) void k_icp_final(const float* __restrict__ partials, int n_rows, double* __restrict__ out) {
    __shared__ double strand[8][LK_REG_OUT];
    const int c = (int)threadIdx.x & (LK_REG_OUT - 1), s = (int)threadIdx.x >> 5;
    double a = 0.0;
    for (int r = s; r < n_rows; r += 8) a += (double)partials[(size_t)r * LK_REG_OUT + c];
    strand[s][c] = a;
    __syncthreads();
    if (threadIdx.x < LK_REG_OUT) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += strand[k][c];
        out[c] = t;
    }
}

extern "C" int64_t lk_icp_scratch_floats(int64_t P) { return P <= 0 ? 0 : (int64_t)lk_cdiv(P, LK_REG_QPW) * LK_REG_OUT; }

extern "C" int lk_icp_accumulate(lk_knn_t tgt, const float* tgt_pos, const float* tgt_normals, const uint8_t* tgt_valid, const float* src,
                                 int64_t P, const float* host_T12, float max_dist, float tukey_k, int32_t mode, int32_t* out_corr,
                                 float* scratch, int64_t scratch_floats, double* out_sums, void* stream_) {
    LK_REQUIRE(tgt != nullptr, "lk_icp_accumulate: NULL target index");
    LK_REQUIRE(P >= 0 && P < (1ll << 31), "lk_icp_accumulate: P out of range");
    LK_REQUIRE(mode == LK_ICP_POINT_TO_PLANE || mode == LK_ICP_INFORMATION, "lk_icp_accumulate: unknown mode");
    LK_REQUIRE(host_T12 != nullptr && out_sums != nullptr, "lk_icp_accumulate: NULL transform or output");
    LK_REQUIRE(max_dist > 0.0f, "lk_icp_accumulate: max_dist must be > 0");
    hipStream_t st = (hipStream_t)stream_;
    const int n_rows = lk_cdiv(P, LK_REG_QPW);
    if (P > 0) {
        LK_REQUIRE(src != nullptr, "lk_icp_accumulate: NULL source");
        LK_REQUIRE(tgt->n == 0 || tgt_pos != nullptr, "lk_icp_accumulate: NULL target positions");
        LK_REQUIRE(tgt->n == 0 || mode == LK_ICP_INFORMATION || (tgt_normals && tgt_valid), "lk_icp_accumulate: point-to-plane needs the target normals");
        LK_REQUIRE(scratch != nullptr && scratch_floats >= lk_icp_scratch_floats(P), "lk_icp_accumulate: scratch smaller than lk_icp_scratch_floats(P)");
        LkMat12 M;
        for (int k = 0; k < 12; ++k) M.m[k] = host_T12[k];
        hipLaunchKernelGGL(k_icp_accumulate, dim3(n_rows), dim3(256), 0, st, (const LkGrid*)tgt->grid, (const float4*)tgt->sorted,
                           (const int32_t*)tgt->cell_start, tgt_pos, tgt_normals, tgt_valid, src, (int)P, M, max_dist * max_dist, tukey_k,
                           (int)mode, out_corr, scratch);
    }
    hipLaunchKernelGGL(k_icp_final, dim3(1), dim3(256), 0, st, (const float*)scratch, n_rows, out_sums);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

// ------------------------------------------------------------------ map correction
__global__ __launch_bounds__(256) void k_apply_correction(float* __restrict__ pos, long long N, const int32_t* __restrict__ seg_id,
                                                          const float* __restrict__ mats, int n_seg) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int s = seg_id[i];
    if (s < 0 || s >= n_seg) return;                      // a row without a segment stays where it is
    const float* m = mats + 12 * (size_t)s;
    const bool ident = m[0] == 1.0f && m[1] == 0.0f && m[2] == 0.0f && m[3] == 0.0f && m[4] == 0.0f && m[5] == 1.0f && m[6] == 0.0f &&
                       m[7] == 0.0f && m[8] == 0.0f && m[9] == 0.0f && m[10] == 1.0f && m[11] == 0.0f;
    if (ident) return;                                    // bit-identical, signed zeros included
    const float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
    lk_rigid_apply(m, x, y, z, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
}

extern "C" int lk_apply_correction(float* pos, int64_t N, const int32_t* seg_id, const float* mats, int32_t n_seg, void* stream_) {
    LK_REQUIRE(N >= 0 && n_seg >= 0, "lk_apply_correction: bad sizes");
    if (N == 0 || n_seg == 0) return LK_OK;
    LK_REQUIRE(pos && seg_id && mats, "lk_apply_correction: NULL buffer");
    hipLaunchKernelGGL(k_apply_correction, dim3(lk_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream_, pos, (long long)N, seg_id, mats, (int)n_seg);
    LK_LAUNCH_CHECK();
    return LK_OK;
}
