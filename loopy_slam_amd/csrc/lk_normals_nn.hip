// Loop closure on fused sensor surfaces: what a segment's SURFACE cloud (the vertices of its TSDF volume, tsdf.py / loop_closure.py
// `cloud: 'tsdf'`) needs beside the calls of lk_reg.hip:
//   lk_normals_nn   normals over the max_nn NEAREST neighbours within a radius (Open3D's hybrid search, src/common.py:545-549, 606-617):
//                   an exact selection per point under the index's total order (d2, index), then the covariance summed in that order
//   lk_rigid_map    p <- R p + t over one whole cloud with ONE matrix (lk_apply_correction wants a label per row)
// A file of its own: lk_reg.hip and lk_knn_dev.h keep the instruction streams they have (DESIGN.md §8 on k_sample_interp).
//
// k_normals_nn: ONE WAVE PER POINT.  The best list so far is one 64-bit key (lk_key: d2 bits << 32 | index) per lane, ascending over the
// lanes, a copy of it in LDS.  The candidates of the box's rows of cells come 64 at a time, one per lane; a ballot against the current
// max_nn-th key says whether any of them belongs to the selection at all - next to a dense surface most batches end there.  Otherwise list
// and batch are merged by RANK: a list key moves up by the number of passing candidates below it (one LDS broadcast read per passing
// candidate, the loop runs over the ballot's set bits), a passing candidate lands at (list keys below it: a 6-step binary search in the
// LDS copy) + (passing candidates below it); ranks below 64 are scattered into the other of two LDS list buffers and read back.  Keys are
// distinct (the index holds every point once), so the ranks are a permutation and the result is THE max_nn smallest keys whatever order
// the cells, rows and lanes present them in.  No shuffles: the only collectives are the ballot and the wave's own LDS ordering.
// The sums then run over the list in lane order = ascending (d2, index), every lane adding the same terms (LDS broadcast), so the
// result depends on the cloud alone - equal bits after a rebuild of the index, which lk_normals cannot promise.  No atomics.
//
// Work per point: ceil(row length / 64) batches over at most 3 x 3 rows (cell >= radius), each one load + distance + ballot; a merge costs
// (passing candidates) + 6 dependent LDS reads.  With n candidates met in an order unrelated to distance the expected number of passing
// candidates is about max_nn (1 + ln(n / max_nn)), not n.  LDS: 2 304 bytes per wave.
#include "lk_common.h"
#include "lk_knn_dev.h"
#include "lk_reg_dev.h"

#define LK_NN_WAVES 4                               // points per workgroup of 256
#define LK_NN_LIST LK_NORMALS_MAX_NN                // = the wave: one key per lane

struct LkNnMat12 { float m[12]; };                  // row-major 3 x 4, passed by value

// the wave's LDS writes so far are visible to its reads behind this point (on the chip one wave's LDS operations execute in order; the host
// emulation runs lanes as fibers and needs the meeting point)
__device__ __forceinline__ void lk_nn_wave_sync() {
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
}

// unit eigenvector of the smallest eigenvalue of the symmetric matrix (xx xy xz; . yy yz; . . zz): k_normals' steps (lk_reg.hip), on the
// shared rotation lk_jacobi_rot
__device__ __forceinline__ void lk_nn_smallest_eigvec(float xx, float xy, float xz, float yy, float yz, float zz, float& nx, float& ny, float& nz) {
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

__global__ __launch_bounds__(256) void k_normals_nn(const LkGrid* __restrict__ G, const float4* __restrict__ sorted,
                                                    const int32_t* __restrict__ cell_start, const float* __restrict__ pos, int N, float r2,
                                                    int max_nn, float cx, float cy, float cz, float* __restrict__ out_n,
                                                    uint8_t* __restrict__ out_valid, int32_t* __restrict__ out_count,
                                                    int32_t* __restrict__ out_nbr) {
    __shared__ uint64_t sh_key[LK_NN_WAVES][3][LK_NN_LIST];        // per wave: two list buffers (the merge writes the other one), the batch
    __shared__ float sh_rel[LK_NN_WAVES][3 * LK_NN_LIST];          // the selection relative to the point
    const int lane = lk_lane(), wave = lk_uniform((int)threadIdx.x >> 6);
    const int i = (int)blockIdx.x * LK_NN_WAVES + wave;
    if (i >= N) return;                                            // the whole wave: nothing below meets another wave
    const float qx = pos[3 * (size_t)i], qy = pos[3 * (size_t)i + 1], qz = pos[3 * (size_t)i + 2];
    uint64_t* const cand = sh_key[wave][2];
    int cur = 0;
    uint64_t K = LK_KEY_EMPTY, thr = LK_KEY_EMPTY;                 // my list entry; the max_nn-th (every lane holds the same)
    sh_key[wave][0][lane] = K;
    lk_box_rows(G, cell_start, lk_grid_box(G, qx, qy, qz, lk_box_halfwidth(r2)), [&](int s, int e) {
#pragma unroll 1
        for (int t0 = s; t0 < e; t0 += LK_NN_LIST) {
            const int t = t0 + lane;
            uint64_t c = LK_KEY_EMPTY;
            if (t < e) {
                const float4 p = sorted[t];
                const float d2 = lk_dist2(qx, qy, qz, p.x, p.y, p.z);
                if (d2 <= r2) c = lk_key(d2, __float_as_int(p.w));
            }
            const bool pass = c < thr;                             // the order is total: exactly "among the max_nn smallest so far"
            const unsigned long long mask = __ballot(pass);
            if (mask == 0ull) continue;
            const uint64_t* const lst = sh_key[wave][cur];
            uint64_t* const nl = sh_key[wave][cur ^ 1];
            cand[lane] = c;
            lk_nn_wave_sync();
            int below_k = 0, below_c = 0;                          // passing candidates below my list entry / below my candidate
#pragma unroll 1
            for (unsigned long long m = mask; m != 0ull; m &= m - 1ull) {
                const uint64_t x = cand[__ffsll(m) - 1];
                below_k += x < K ? 1 : 0;
                below_c += x < c ? 1 : 0;
            }
            int lb = 0;                                            // list entries below my candidate (at most 63 for a passing one)
#pragma unroll
            for (int step = LK_NN_LIST / 2; step > 0; step >>= 1) lb += lst[lb + step - 1] < c ? step : 0;
            const int rank_k = lane + below_k, rank_c = lb + below_c;
            if (rank_k < LK_NN_LIST) nl[rank_k] = K;
            if (pass && rank_c < LK_NN_LIST) nl[rank_c] = c;
            lk_nn_wave_sync();
            K = nl[lane];
            thr = nl[max_nn - 1];
            cur ^= 1;
        }
    });
    const bool sel = lane < max_nn && K != LK_KEY_EMPTY;
    const int count = __popcll(__ballot(sel));
    if (out_nbr && lane < max_nn) out_nbr[(size_t)i * max_nn + lane] = (int)(uint32_t)K;      // the empty key's index is -1
    if (out_count && lane == 0) out_count[i] = count;
    float* const rel = sh_rel[wave];
    if (sel) {
        const size_t j = (size_t)(uint32_t)K;
        rel[3 * lane] = pos[3 * j] - qx; rel[3 * lane + 1] = pos[3 * j + 1] - qy; rel[3 * lane + 2] = pos[3 * j + 2] - qz;
    }
    lk_nn_wave_sync();
    // ascending (d2, index): every lane adds the same terms in the same order
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sxx = 0.0f, sxy = 0.0f, sxz = 0.0f, syy = 0.0f, syz = 0.0f, szz = 0.0f;
#pragma unroll 1
    for (int k = 0; k < count; ++k) {
        const float ax = rel[3 * k], ay = rel[3 * k + 1], az = rel[3 * k + 2];
        sx += ax; sy += ay; sz += az;
        sxx += ax * ax; sxy += ax * ay; sxz += ax * az;
        syy += ay * ay; syz += ay * az; szz += az * az;
    }
    if (lane != 0) return;
    const bool valid = count >= 3;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (valid) {
        const float in = 1.0f / (float)count;
        const float mx = sx * in, my = sy * in, mz = sz * in;
        lk_nn_smallest_eigvec(sxx * in - mx * mx, sxy * in - mx * my, sxz * in - mx * mz, syy * in - my * my, syz * in - my * mz,
                              szz * in - mz * mz, nx, ny, nz);
        if (nx * (cx - qx) + ny * (cy - qy) + nz * (cz - qz) < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    }
    out_n[3 * (size_t)i] = nx; out_n[3 * (size_t)i + 1] = ny; out_n[3 * (size_t)i + 2] = nz;
    out_valid[i] = valid ? 1 : 0;
}

extern "C" int lk_normals_nn(lk_knn_t knn, const float* pos, int64_t N, float radius, int32_t max_nn, const float* host_camera3,
                             float* out_normals, uint8_t* out_valid, int32_t* out_count, int32_t* out_nbr, void* stream_) {
    LK_REQUIRE(knn != nullptr, "lk_normals_nn: NULL index");
    LK_REQUIRE(N == knn->n, "lk_normals_nn: N is not the size of the index (build it over pos first)");
    LK_REQUIRE(radius > 0.0f && host_camera3 != nullptr, "lk_normals_nn: bad radius or NULL camera centre");
    LK_REQUIRE(max_nn >= 1 && max_nn <= LK_NORMALS_MAX_NN, "lk_normals_nn: max_nn outside 1 .. LK_NORMALS_MAX_NN");
    if (N == 0) return LK_OK;
    LK_REQUIRE(pos && out_normals && out_valid, "lk_normals_nn: NULL buffer");
    hipLaunchKernelGGL(k_normals_nn, dim3(lk_cdiv(N, LK_NN_WAVES)), dim3(256), 0, (hipStream_t)stream_, (const LkGrid*)knn->grid,
                       (const float4*)knn->sorted, (const int32_t*)knn->cell_start, pos, (int)N, radius * radius, (int)max_nn,
                       host_camera3[0], host_camera3[1], host_camera3[2], out_normals, out_valid, out_count, out_nbr);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

// ------------------------------------------------------------------ one matrix over one cloud
__global__ __launch_bounds__(256) void k_rigid_map(float* __restrict__ pos, long long N, LkNnMat12 M) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
    lk_rigid_apply(M.m, x, y, z, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
}

extern "C" int lk_rigid_map(float* pos, int64_t N, const float* host_M12, void* stream_) {
    LK_REQUIRE(N >= 0 && N < (1ll << 31) && host_M12 != nullptr, "lk_rigid_map: bad size or NULL matrix");
    if (N == 0) return LK_OK;
    LK_REQUIRE(pos != nullptr, "lk_rigid_map: NULL buffer");
    LkNnMat12 M;
    bool ident = true;
    for (int k = 0; k < 12; ++k) {
        M.m[k] = host_M12[k];
        ident = ident && M.m[k] == ((k == 0 || k == 5 || k == 10) ? 1.0f : 0.0f);
    }
    if (ident) return LK_OK;                              // bit-identical, signed zeros included: nothing is launched
    hipLaunchKernelGGL(k_rigid_map, dim3(lk_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream_, pos, (long long)N, M);
    LK_LAUNCH_CHECK();
    return LK_OK;
}
