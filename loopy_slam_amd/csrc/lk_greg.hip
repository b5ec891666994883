// Loop closure, global start: what the reference does with Open3D before its ICP (src/common.py: preprocess_point_cloud,
// execute_global_registration) -
//   lk_voxel_keys / lk_voxel_heads / lk_voxel_downsample   one centroid per occupied voxel, ascending key order
//   lk_knn_canonicalize                                    the points of every grid cell in ascending point order
//   lk_fpfh                                                Rusu's SPFH and FPFH over all neighbours inside the radius
//   lk_feature_match                                       nearest row of B for every row of A under (d2, index)
//   lk_ransac_gather / lk_ransac_hypotheses / lk_ransac_score / lk_ransac_best
//                                                          counter-based 3-point RANSAC over a correspondence set
// All arithmetic is fp32.  Nothing here adds floating-point numbers through atomics: histograms are integer counts (LDS integer atomics,
// order-free), every floating-point sum is walked in an order the inputs fix (the canonical cell order, the row order of a table, a fixed
// butterfly), so equal inputs and an equal seed give equal bits.
//
// Shared with lk_reg.hip: the radius box and its row walk (lk_knn_dev.h: lk_grid_box, lk_box_rows), the 8-lane group, the rigid map and
// the Jacobi rotation (lk_reg_dev.h).
#include "lk_common.h"
#include "lk_knn_dev.h"
#include "lk_reg_dev.h"
#include "lk_philox_dev.h"
#include "lk_kernels.h"

#define LK_PI_F 3.14159265358979323846f

// ------------------------------------------------------------------ voxel downsample
__device__ __forceinline__ int lk_voxel_coord(float x, float o, float v) {
    const float f = floorf(__fsub_rn(x, o) / v);
    return (int)fminf(fmaxf(f, 0.0f), (float)LK_VOXEL_AXIS_MAX);
}

__global__ __launch_bounds__(256) void k_voxel_keys(const float* __restrict__ pos, long long N, float ox, float oy, float oz, float v,
                                                    int64_t* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int64_t kx = lk_voxel_coord(pos[3 * i], ox, v), ky = lk_voxel_coord(pos[3 * i + 1], oy, v), kz = lk_voxel_coord(pos[3 * i + 2], oz, v);
    keys[i] = (kx << 42) | (ky << 21) | kz;
}

__global__ __launch_bounds__(256) void k_voxel_heads(const int64_t* __restrict__ sorted_keys, long long N, uint8_t* __restrict__ head) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    head[i] = (i == 0 || sorted_keys[i] != sorted_keys[i - 1]) ? 1 : 0;
}

// one thread per voxel: its points in sorted order, summed relative to the first of them (the sum does not cancel against the room's coordinates)
__global__ __launch_bounds__(256) void k_voxel_centroids(const float* __restrict__ pos, long long N, const int64_t* __restrict__ order,
                                                         const int32_t* __restrict__ starts, int n_vox, float* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_vox) return;
    const int s = starts[j], e = j + 1 < n_vox ? starts[j + 1] : (int)N;
    const long long i0 = order[s];
    const float x0 = pos[3 * i0], y0 = pos[3 * i0 + 1], z0 = pos[3 * i0 + 2];
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int t = s + 1; t < e; ++t) {
        const long long i = order[t];
        sx += pos[3 * i] - x0; sy += pos[3 * i + 1] - y0; sz += pos[3 * i + 2] - z0;
    }
    const float inv = 1.0f / (float)(e - s);
    out[3 * (size_t)j] = x0 + sx * inv; out[3 * (size_t)j + 1] = y0 + sy * inv; out[3 * (size_t)j + 2] = z0 + sz * inv;
}

extern "C" int lk_voxel_keys(const float* pos, int64_t N, const float* host_origin3, float voxel, int64_t* out_keys, void* stream_) {
    LK_REQUIRE(N >= 0 && N < (1ll << 31) && voxel > 0.0f && host_origin3 != nullptr, "lk_voxel_keys: bad arguments");
    if (N == 0) return LK_OK;
    LK_REQUIRE(pos && out_keys, "lk_voxel_keys: NULL buffer");
    hipLaunchKernelGGL(k_voxel_keys, dim3(lk_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream_, pos, (long long)N, host_origin3[0],
                       host_origin3[1], host_origin3[2], voxel, out_keys);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

extern "C" int lk_voxel_heads(const int64_t* sorted_keys, int64_t N, uint8_t* out_head, void* stream_) {
    LK_REQUIRE(N >= 0 && N < (1ll << 31), "lk_voxel_heads: bad size");
    if (N == 0) return LK_OK;
    LK_REQUIRE(sorted_keys && out_head, "lk_voxel_heads: NULL buffer");
    hipLaunchKernelGGL(k_voxel_heads, dim3(lk_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream_, sorted_keys, (long long)N, out_head);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

extern "C" int lk_voxel_downsample(const float* pos, int64_t N, const int64_t* order, const int32_t* starts, int32_t n_vox, float* out_centroids,
                                   void* stream_) {
    LK_REQUIRE(N >= 0 && N < (1ll << 31) && n_vox >= 0 && n_vox <= N, "lk_voxel_downsample: bad sizes");
    if (n_vox == 0) return LK_OK;
    LK_REQUIRE(pos && order && starts && out_centroids, "lk_voxel_downsample: NULL buffer");
    hipLaunchKernelGGL(k_voxel_centroids, dim3(lk_cdiv(n_vox, 256)), dim3(256), 0, (hipStream_t)stream_, pos, (long long)N, order, starts,
                       (int)n_vox, out_centroids);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

// ------------------------------------------------------------------ canonical cell order
// lk_knn_build places the points of a cell in the order their counting atomics landed.  The thread of a cell's rank-0 point sorts the cell's
// run by point index (insertion sort: cells hold tens of points); every cell has exactly one such thread and the runs are disjoint.
__global__ __launch_bounds__(256) void k_knn_canon(int n, const int32_t* __restrict__ cell_start, const int32_t* __restrict__ cell_of,
                                                   const int32_t* __restrict__ rank_of, float4* __restrict__ sorted) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || rank_of[i] != 0) return;
    const int c = cell_of[i];
    const int s = cell_start[c], e = cell_start[c + 1];
    for (int a = s + 1; a < e; ++a) {
        const float4 x = sorted[a];
        const int kx = __float_as_int(x.w);
        int b = a - 1;
        while (b >= s && __float_as_int(sorted[b].w) > kx) { sorted[b + 1] = sorted[b]; --b; }
        sorted[b + 1] = x;
    }
}

extern "C" int lk_knn_canonicalize(lk_knn_t h, void* stream_) {
    LK_REQUIRE(h != nullptr, "lk_knn_canonicalize: NULL index");
    if (h->n == 0) return LK_OK;
    hipLaunchKernelGGL(k_knn_canon, dim3(lk_cdiv(h->n, 256)), dim3(256), 0, (hipStream_t)stream_, (int)h->n, (const int32_t*)h->cell_start,
                       (const int32_t*)h->cell_of, (const int32_t*)h->rank_of, h->sorted);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

// ------------------------------------------------------------------ FPFH
__device__ __forceinline__ int lk_bin11(float x) { return (int)fminf(fmaxf(floorf(x), 0.0f), 10.0f); }

// Pass 1.  One 8-lane group per point; the three 11-bin histograms are integer counts in LDS, scaled by 100 / count at the end.
__global__ __launch_bounds__(256) void k_spfh(const LkGrid* __restrict__ G, const float4* __restrict__ sorted, const int32_t* __restrict__ cell_start,
                                              const float* __restrict__ pos, const float* __restrict__ nrm, const uint8_t* __restrict__ valid, int N,
                                              float r2, float* __restrict__ spfh) {
    __shared__ unsigned hist[LK_REG_GROUPS][LK_FPFH_DIM + 3];
    const int group = (int)threadIdx.x / LK_REG_T, sub = (int)threadIdx.x % LK_REG_T;
    const int qi_raw = blockIdx.x * LK_REG_GROUPS + group;
    const bool live = qi_raw < N;
    const int i = live ? qi_raw : N - 1;
    for (int b = sub; b < LK_FPFH_DIM; b += LK_REG_T) hist[group][b] = 0u;
    __syncthreads();
    const float qx = pos[3 * (size_t)i], qy = pos[3 * (size_t)i + 1], qz = pos[3 * (size_t)i + 2];
    const float n1x = nrm[3 * (size_t)i], n1y = nrm[3 * (size_t)i + 1], n1z = nrm[3 * (size_t)i + 2];
    const bool own = valid[i] != 0;
    float cnt = 0.0f;
    if (own) {
        lk_box_rows(G, cell_start, lk_grid_box(G, qx, qy, qz, lk_box_halfwidth(r2)), [&](int s, int e) {
#pragma unroll 1
            for (int t = s + sub; t < e; t += LK_REG_T) {
                const float4 p = sorted[t];
                const int k = __float_as_int(p.w);
                const float d2 = lk_dist2(qx, qy, qz, p.x, p.y, p.z);
                if (d2 > r2 || k == i || !valid[k]) continue;
                cnt += 1.0f;
                const float n2x = nrm[3 * (size_t)k], n2y = nrm[3 * (size_t)k + 1], n2z = nrm[3 * (size_t)k + 2];
                float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
                const float d = sqrtf(d2);
                if (d > 0.0f) {
                    float ex = __fsub_rn(p.x, qx), ey = __fsub_rn(p.y, qy), ez = __fsub_rn(p.z, qz);
                    const float a1 = (n1x * ex + n1y * ey + n1z * ez) / d, a2 = (n2x * ex + n2y * ey + n2z * ez) / d;
                    // acos|a1| > acos|a2|.  The one decision taken in fp64 (exact differences, products of fp32 values): a neighbour along the
                    // normal - the three points of one ray - has a1 = a2 up to rounding, and the swap turns f2 from -1 to +1
                    const double gx = (double)p.x - (double)qx, gy = (double)p.y - (double)qy, gz = (double)p.z - (double)qz;
                    const bool swap = fabs((double)n1x * gx + (double)n1y * gy + (double)n1z * gz) <
                                      fabs((double)n2x * gx + (double)n2y * gy + (double)n2z * gz);
                    const float ux = swap ? n2x : n1x, uy = swap ? n2y : n1y, uz = swap ? n2z : n1z;
                    const float mx = swap ? n1x : n2x, my = swap ? n1y : n2y, mz = swap ? n1z : n2z;
                    if (swap) { ex = -ex; ey = -ey; ez = -ez; }
                    float vx = ey * uz - ez * uy, vy = ez * ux - ex * uz, vz = ex * uy - ey * ux;
                    const float vn = sqrtf(vx * vx + vy * vy + vz * vz);
                    if (vn > 0.0f) {
                        vx /= vn; vy /= vn; vz /= vn;
                        const float wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
                        f2 = swap ? -a2 : a1;
                        f1 = vx * mx + vy * my + vz * mz;
                        f0 = atan2f(wx * mx + wy * my + wz * mz, ux * mx + uy * my + uz * mz);
                    }
                }
                atomicAdd(&hist[group][lk_bin11(11.0f * (f0 + LK_PI_F) / (2.0f * LK_PI_F))], 1u);
                atomicAdd(&hist[group][11 + lk_bin11(11.0f * (f1 + 1.0f) * 0.5f)], 1u);
                atomicAdd(&hist[group][22 + lk_bin11(11.0f * (f2 + 1.0f) * 0.5f)], 1u);
            }
        });
    }
    cnt = lk_sum8(cnt);
    __syncthreads();
    if (!live) return;
    const float incr = cnt > 0.0f ? 100.0f / cnt : 0.0f;
    for (int b = sub; b < LK_FPFH_DIM; b += LK_REG_T) spfh[(size_t)i * LK_FPFH_DIM + b] = (float)hist[group][b] * incr;
}

// Pass 2.  Lane `sub` of a point's group owns bins sub, sub + 8, ..; all eight lanes walk ALL neighbours in the canonical cell order, so a bin
// is one sequential sum.  The block sums are taken over the bins in ascending order.
__global__ __launch_bounds__(256) void k_fpfh(const LkGrid* __restrict__ G, const float4* __restrict__ sorted, const int32_t* __restrict__ cell_start,
                                              const float* __restrict__ pos, const uint8_t* __restrict__ valid, int N, float r2,
                                              const float* __restrict__ spfh, float* __restrict__ fpfh) {
    __shared__ float row[LK_REG_GROUPS][LK_FPFH_DIM + 3];
    constexpr int NB = (LK_FPFH_DIM + LK_REG_T - 1) / LK_REG_T;
    const int group = (int)threadIdx.x / LK_REG_T, sub = (int)threadIdx.x % LK_REG_T;
    const int qi_raw = blockIdx.x * LK_REG_GROUPS + group;
    const bool live = qi_raw < N;
    const int i = live ? qi_raw : N - 1;
    const float qx = pos[3 * (size_t)i], qy = pos[3 * (size_t)i + 1], qz = pos[3 * (size_t)i + 2];
    const bool own = valid[i] != 0;
    float acc[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) acc[q] = 0.0f;
    if (own) {
        lk_box_rows(G, cell_start, lk_grid_box(G, qx, qy, qz, lk_box_halfwidth(r2)), [&](int s, int e) {
#pragma unroll 1
            for (int t = s; t < e; ++t) {
                const float4 p = sorted[t];
                const int k = __float_as_int(p.w);
                const float d2 = lk_dist2(qx, qy, qz, p.x, p.y, p.z);
                if (d2 > r2 || k == i || !valid[k] || d2 == 0.0f) continue;
#pragma unroll
                for (int q = 0; q < NB; ++q) {
                    const int b = sub + LK_REG_T * q;
                    if (b < LK_FPFH_DIM) acc[q] += spfh[(size_t)k * LK_FPFH_DIM + b] / d2;
                }
            }
        });
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        const int b = sub + LK_REG_T * q;
        if (b < LK_FPFH_DIM) row[group][b] = acc[q];
    }
    __syncthreads();
    if (!live) return;
    float scale[3];
#pragma unroll
    for (int blk = 0; blk < 3; ++blk) {
        float sum = 0.0f;
        for (int b = 0; b < 11; ++b) sum += row[group][11 * blk + b];
        scale[blk] = sum != 0.0f ? 100.0f / sum : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        const int b = sub + LK_REG_T * q;
        if (b < LK_FPFH_DIM) {
            const float sc = b < 11 ? scale[0] : (b < 22 ? scale[1] : scale[2]);
            fpfh[(size_t)i * LK_FPFH_DIM + b] = own ? acc[q] * sc + spfh[(size_t)i * LK_FPFH_DIM + b] : 0.0f;
        }
    }
}

extern "C" int lk_fpfh(lk_knn_t knn, const float* pos, const float* normals, const uint8_t* valid, int64_t N, float radius, float* out_spfh,
                       float* out_fpfh, void* stream_) {
    LK_REQUIRE(knn != nullptr, "lk_fpfh: NULL index");
    LK_REQUIRE(N == knn->n, "lk_fpfh: N is not the size of the index (build it over pos first)");
    LK_REQUIRE(radius > 0.0f, "lk_fpfh: bad radius");
    if (N == 0) return LK_OK;
    LK_REQUIRE(pos && normals && valid && out_spfh && out_fpfh, "lk_fpfh: NULL buffer");
    hipStream_t st = (hipStream_t)stream_;
    const dim3 grid(lk_cdiv(N, LK_REG_GROUPS));
    hipLaunchKernelGGL(k_spfh, grid, dim3(256), 0, st, (const LkGrid*)knn->grid, (const float4*)knn->sorted, (const int32_t*)knn->cell_start, pos,
                       normals, valid, (int)N, radius * radius, out_spfh);
    hipLaunchKernelGGL(k_fpfh, grid, dim3(256), 0, st, (const LkGrid*)knn->grid, (const float4*)knn->sorted, (const int32_t*)knn->cell_start, pos,
                       valid, (int)N, radius * radius, (const float*)out_spfh, out_fpfh);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

// ------------------------------------------------------------------ feature match
// One thread per row of A (its 33 values in registers); B goes through LDS in tiles of 64 rows padded to 36 floats, every lane reads the
// same address (broadcast).  d2 = sum over the 33 columns ascending of (a - b)^2; the smallest (d2, index) wins: rows are met in ascending
// order and only a strictly smaller d2 replaces the holder.
#define LK_FM_TILE 64
#define LK_FM_LD 36
__global__ __launch_bounds__(256) void k_feature_match(const float* __restrict__ A, const uint8_t* __restrict__ validA, int Na,
                                                       const float* __restrict__ B, const uint8_t* __restrict__ validB, int Nb,
                                                       int32_t* __restrict__ out_idx, float* __restrict__ out_d2) {
    __shared__ __attribute__((aligned(16))) float tile[LK_FM_TILE * LK_FM_LD];
    __shared__ int tile_ok[LK_FM_TILE];
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    const bool live = i < Na;
    const int ia = live ? i : Na - 1;
    float a[LK_FPFH_DIM];
#pragma unroll
    for (int c = 0; c < LK_FPFH_DIM; ++c) a[c] = A[(size_t)ia * LK_FPFH_DIM + c];
    float best = LK_FLT_MAX;
    int best_j = -1;
#pragma unroll 1
    for (int j0 = 0; j0 < Nb; j0 += LK_FM_TILE) {
        const int nj = Nb - j0 < LK_FM_TILE ? Nb - j0 : LK_FM_TILE;
        __syncthreads();
        for (int e = (int)threadIdx.x; e < nj * LK_FPFH_DIM; e += 256) {
            const int r = e / LK_FPFH_DIM, c = e - r * LK_FPFH_DIM;
            tile[r * LK_FM_LD + c] = B[(size_t)j0 * LK_FPFH_DIM + e];
        }
        if ((int)threadIdx.x < nj) tile_ok[threadIdx.x] = validB ? (int)validB[j0 + threadIdx.x] : 1;
        __syncthreads();
#pragma unroll 1
        for (int r = 0; r < nj; ++r) {
            if (!tile_ok[r]) continue;
            const float4* __restrict__ b4 = reinterpret_cast<const float4*>(tile + r * LK_FM_LD);
            float d2 = 0.0f;
#pragma unroll
            for (int c4 = 0; c4 < 8; ++c4) {
                const float4 b = b4[c4];
                const float e0 = a[4 * c4] - b.x, e1 = a[4 * c4 + 1] - b.y, e2 = a[4 * c4 + 2] - b.z, e3 = a[4 * c4 + 3] - b.w;
                d2 += e0 * e0; d2 += e1 * e1; d2 += e2 * e2; d2 += e3 * e3;
            }
            const float el = a[32] - tile[r * LK_FM_LD + 32];
            d2 += el * el;
            if (d2 < best) { best = d2; best_j = j0 + r; }
        }
    }
    if (!live) return;
    const bool ok = (validA ? validA[i] != 0 : true) && best_j >= 0;
    out_idx[i] = ok ? best_j : -1;
    out_d2[i] = ok ? best : 0.0f;
}

extern "C" int lk_feature_match(const float* A, const uint8_t* validA, int64_t Na, const float* B, const uint8_t* validB, int64_t Nb,
                                int32_t* out_idx, float* out_d2, void* stream_) {
    LK_REQUIRE(Na >= 0 && Nb >= 0 && Na < (1ll << 31) && Nb < (1ll << 31), "lk_feature_match: bad sizes");
    if (Na == 0) return LK_OK;
    LK_REQUIRE(A && out_idx && out_d2 && (Nb == 0 || B), "lk_feature_match: NULL buffer");
    hipLaunchKernelGGL(k_feature_match, dim3(lk_cdiv(Na, 256)), dim3(256), 0, (hipStream_t)stream_, A, validA, (int)Na, B, validB, (int)Nb,
                       out_idx, out_d2);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

// ------------------------------------------------------------------ RANSAC
__global__ __launch_bounds__(256) void k_ransac_gather(const float* __restrict__ src, const float* __restrict__ tgt, const int32_t* __restrict__ corr,
                                                       int M, float* __restrict__ cs, float* __restrict__ ct) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const int a = corr[2 * j], b = corr[2 * j + 1];
#pragma unroll
    for (int c = 0; c < 3; ++c) { cs[3 * (size_t)j + c] = src[3 * (size_t)a + c]; ct[3 * (size_t)j + c] = tgt[3 * (size_t)b + c]; }
}

// One thread per trial: draw, check, fit (Horn 1987: the rotation is the unit eigenvector of the largest eigenvalue of a symmetric 4 x 4 matrix
// of the centred cross-covariance; cyclic Jacobi), check again.  ok[t] = 1 and T[t] (row-major 3 x 4) for a survivor.
__global__ __launch_bounds__(256) void k_ransac_hyp(const float* __restrict__ cs, const float* __restrict__ ct, int M, uint32_t seed_lo,
                                                    uint32_t seed_hi, uint64_t trial0, int n_trials, float edge_ratio, float dist_thr,
                                                    int32_t* __restrict__ out_triples, uint8_t* __restrict__ out_ok, float* __restrict__ out_T) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_trials) return;
    const uint64_t trial = trial0 + (uint64_t)t;
    uint32_t r[4];
    lk_philox(seed_lo, seed_hi, (uint32_t)trial, (uint32_t)(trial >> 32), r);
    int id[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) id[k] = (int)(((uint64_t)r[k] * (uint32_t)M) >> 32);
    if (out_triples) { out_triples[3 * (size_t)t] = id[0]; out_triples[3 * (size_t)t + 1] = id[1]; out_triples[3 * (size_t)t + 2] = id[2]; }
    bool ok = id[0] != id[1] && id[1] != id[2] && id[0] != id[2];
    float s[3][3], q[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) { s[k][c] = cs[3 * (size_t)id[k] + c]; q[k][c] = ct[3 * (size_t)id[k] + c]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int l = (k + 1) % 3;
        const float ds = sqrtf(lk_dist2(s[k][0], s[k][1], s[k][2], s[l][0], s[l][1], s[l][2]));
        const float dt = sqrtf(lk_dist2(q[k][0], q[k][1], q[k][2], q[l][0], q[l][1], q[l][2]));
        ok = ok && !(ds < dt * edge_ratio || dt < ds * edge_ratio);
    }
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = 0.0f;
    if (ok) {
        // The fit alone runs in fp64 (the trials the edge checker lets through: a few per cent).  A thin triangle of length L and width w fixes
        // the rotation about its long side through terms of size w^2 beside terms of size L^2: fp32 leaves 1e-7 L^2 / w^2 rad of it.
        double ms[3], mq[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ms[c] = (((double)s[0][c] + (double)s[1][c]) + (double)s[2][c]) / 3.0;
            mq[c] = (((double)q[0][c] + (double)q[1][c]) + (double)q[2][c]) / 3.0;
        }
        double S[3][3];                               // S[a][b] = sum_k (s_k - ms)_a (q_k - mq)_b
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b)
                S[a][b] = ((s[0][a] - ms[a]) * (q[0][b] - mq[b]) + (s[1][a] - ms[a]) * (q[1][b] - mq[b])) + (s[2][a] - ms[a]) * (q[2][b] - mq[b]);
        double nrm = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) nrm += fabs(S[a][b]);
        const double sc = nrm > 0.0 ? 1.0 / nrm : 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) S[a][b] *= sc;
        double Nm[4][4] = {{S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
                           {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
                           {S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
                           {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]}};
        double V[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
#pragma unroll 1
        for (int sweep = 0; sweep < 12; ++sweep) {
            lk_jacobi_rot<4, 0, 1>(Nm, V); lk_jacobi_rot<4, 0, 2>(Nm, V); lk_jacobi_rot<4, 0, 3>(Nm, V);
            lk_jacobi_rot<4, 1, 2>(Nm, V); lk_jacobi_rot<4, 1, 3>(Nm, V); lk_jacobi_rot<4, 2, 3>(Nm, V);
        }
        double lmax = Nm[0][0];
        int col = 0;
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (Nm[k][k] > lmax) { lmax = Nm[k][k]; col = k; }
        double qw = 0.0, qx = 0.0, qy = 0.0, qz = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (col == k) { qw = V[0][k]; qx = V[1][k]; qy = V[2][k]; qz = V[3][k]; }
        const double qi = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
        qw *= qi; qx *= qi; qy *= qi; qz *= qi;
        const double R[3][3] = {{1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)},
                                {2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)},
                                {2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)}};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            T[4 * a] = (float)R[a][0]; T[4 * a + 1] = (float)R[a][1]; T[4 * a + 2] = (float)R[a][2];
            T[4 * a + 3] = (float)(mq[a] - (R[a][0] * ms[0] + R[a][1] * ms[1] + R[a][2] * ms[2]));
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float px, py, pz;
            lk_rigid_apply(T, s[k][0], s[k][1], s[k][2], px, py, pz);
            ok = ok && !(sqrtf(lk_dist2(px, py, pz, q[k][0], q[k][1], q[k][2])) > dist_thr);
        }
    }
    out_ok[t] = ok ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) out_T[12 * (size_t)t + k] = ok ? T[k] : 0.0f;
}

// One wave per surviving hypothesis, four per workgroup; the correspondences go through LDS in tiles that the four waves share.  A lane
// counts and sums its pairs j = lane, lane + 64, .. in ascending order; the wave meets in a fixed xor butterfly.
#define LK_RS_TILE 1024
__global__ __launch_bounds__(256) void k_ransac_score(const float* __restrict__ cs, const float* __restrict__ ct, int M, const float* __restrict__ T_all,
                                                      const int32_t* __restrict__ surv, const int32_t* __restrict__ n_surv, float thr2,
                                                      int32_t* __restrict__ out_count, float* __restrict__ out_sum) {
    __shared__ float ls[LK_RS_TILE * 3];
    __shared__ float lt[LK_RS_TILE * 3];
    const int ns = *n_surv;
    if ((int)blockIdx.x * 4 >= ns) return;               // uniform over the workgroup
    const int wave = (int)threadIdx.x >> 6, lane = lk_lane();
    const int h = blockIdx.x * 4 + wave;
    const bool live = h < ns;
    const int trial = surv[live ? h : ns - 1];
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = T_all[12 * (size_t)trial + k];
    int cnt = 0;
    float sum = 0.0f;
#pragma unroll 1
    for (int j0 = 0; j0 < M; j0 += LK_RS_TILE) {
        const int nj = M - j0 < LK_RS_TILE ? M - j0 : LK_RS_TILE;
        __syncthreads();
        for (int e = (int)threadIdx.x; e < 3 * nj; e += 256) { ls[e] = cs[3 * (size_t)j0 + e]; lt[e] = ct[3 * (size_t)j0 + e]; }
        __syncthreads();
#pragma unroll 1
        for (int j = lane; j < nj; j += 64) {
            float px, py, pz;
            lk_rigid_apply(T, ls[3 * j], ls[3 * j + 1], ls[3 * j + 2], px, py, pz);
            const float d2 = lk_dist2(px, py, pz, lt[3 * j], lt[3 * j + 1], lt[3 * j + 2]);
            if (d2 <= thr2) { cnt += 1; sum += d2; }
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        cnt += __shfl_xor(cnt, m);
        sum += __shfl_xor(sum, m);
    }
    if (live && lane == 0) { out_count[h] = cnt; out_sum[h] = sum; }
}

// (count descending, sum ascending, trial ascending): a total order, so the winner does not depend on who meets whom
__device__ __forceinline__ bool lk_rs_better(int c, float s, long long t, int bc, float bs, long long bt) {
    return c > bc || (c == bc && (s < bs || (s == bs && t < bt)));
}

// One workgroup: the best of this batch's survivors against the record of the batches before.
// best (int32 [LK_RANSAC_BEST]): 0 count (-1: none yet), 1 bits of sum d2, 2 / 3 trial low / high, 4..15 bits of T, 16 survivors so far
__global__ __launch_bounds__(256) void k_ransac_best(const int32_t* __restrict__ count, const float* __restrict__ sum, const int32_t* __restrict__ surv,
                                                     const int32_t* __restrict__ n_surv, const float* __restrict__ T_all, uint64_t trial0,
                                                     int32_t* __restrict__ best) {
    __shared__ int sc[256];
    __shared__ float ss[256];
    __shared__ long long st[256];
    const int ns = *n_surv, tid = (int)threadIdx.x;
    int bc = -1;
    float bs = 0.0f;
    long long bt = -1;
    for (int h = tid; h < ns; h += 256) {
        const long long t = (long long)trial0 + surv[h];
        if (bc < 0 || lk_rs_better(count[h], sum[h], t, bc, bs, bt)) { bc = count[h]; bs = sum[h]; bt = t; }
    }
    sc[tid] = bc; ss[tid] = bs; st[tid] = bt;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w && sc[tid + w] >= 0 && (sc[tid] < 0 || lk_rs_better(sc[tid + w], ss[tid + w], st[tid + w], sc[tid], ss[tid], st[tid]))) {
            sc[tid] = sc[tid + w]; ss[tid] = ss[tid + w]; st[tid] = st[tid + w];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    best[16] += ns;
    if (sc[0] < 0) return;
    const long long old_t = (long long)(((uint64_t)(uint32_t)best[3] << 32) | (uint32_t)best[2]);
    if (best[0] >= 0 && !lk_rs_better(sc[0], ss[0], st[0], best[0], __int_as_float(best[1]), old_t)) return;
    best[0] = sc[0]; best[1] = __float_as_int(ss[0]);
    best[2] = (int32_t)(uint32_t)(uint64_t)st[0]; best[3] = (int32_t)(uint32_t)((uint64_t)st[0] >> 32);
    const size_t local = (size_t)(st[0] - (long long)trial0);
    for (int k = 0; k < 12; ++k) best[4 + k] = __float_as_int(T_all[12 * local + k]);
}

extern "C" int lk_ransac_gather(const float* src, const float* tgt, const int32_t* corr, int32_t M, float* out_cs, float* out_ct, void* stream_) {
    LK_REQUIRE(M >= 0, "lk_ransac_gather: bad size");
    if (M == 0) return LK_OK;
    LK_REQUIRE(src && tgt && corr && out_cs && out_ct, "lk_ransac_gather: NULL buffer");
    hipLaunchKernelGGL(k_ransac_gather, dim3(lk_cdiv(M, 256)), dim3(256), 0, (hipStream_t)stream_, src, tgt, corr, (int)M, out_cs, out_ct);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

extern "C" int lk_ransac_hypotheses(const float* cs, const float* ct, int32_t M, uint64_t seed, uint64_t trial0, int32_t n_trials,
                                    float edge_ratio, float dist_thr, int32_t* out_triples, uint8_t* out_ok, float* out_T, void* stream_) {
    LK_REQUIRE(M >= 3 && n_trials >= 0, "lk_ransac_hypotheses: needs at least 3 correspondences");
    if (n_trials == 0) return LK_OK;
    LK_REQUIRE(cs && ct && out_ok && out_T, "lk_ransac_hypotheses: NULL buffer");
    hipLaunchKernelGGL(k_ransac_hyp, dim3(lk_cdiv(n_trials, 256)), dim3(256), 0, (hipStream_t)stream_, cs, ct, (int)M, (uint32_t)seed,
                       (uint32_t)(seed >> 32), trial0, (int)n_trials, edge_ratio, dist_thr, out_triples, out_ok, out_T);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

extern "C" int lk_ransac_score(const float* cs, const float* ct, int32_t M, const float* T_all, const int32_t* survivors, const int32_t* n_survivors,
                               int32_t max_survivors, float dist_thr, int32_t* out_count, float* out_sum_d2, void* stream_) {
    LK_REQUIRE(M >= 0 && max_survivors >= 0, "lk_ransac_score: bad sizes");
    if (max_survivors == 0) return LK_OK;
    LK_REQUIRE(T_all && survivors && n_survivors && out_count && out_sum_d2 && (M == 0 || (cs && ct)), "lk_ransac_score: NULL buffer");
    hipLaunchKernelGGL(k_ransac_score, dim3(lk_cdiv(max_survivors, 4)), dim3(256), 0, (hipStream_t)stream_, cs, ct, (int)M, T_all, survivors,
                       n_survivors, dist_thr * dist_thr, out_count, out_sum_d2);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

extern "C" int lk_ransac_best(const int32_t* count, const float* sum_d2, const int32_t* survivors, const int32_t* n_survivors, const float* T_all,
                              uint64_t trial0, int32_t* best, void* stream_) {
    LK_REQUIRE(count && sum_d2 && survivors && n_survivors && T_all && best, "lk_ransac_best: NULL buffer");
    hipLaunchKernelGGL(k_ransac_best, dim3(1), dim3(256), 0, (hipStream_t)stream_, count, sum_d2, survivors, n_survivors, T_all, trial0, best);
    LK_LAUNCH_CHECK();
    return LK_OK;
}
