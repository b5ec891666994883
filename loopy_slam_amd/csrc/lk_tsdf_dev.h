// Device helpers of lk_tsdf.hip: the sparse 16^3 block volume (keys, voxel centres, the five planes of a slot) and the corner / edge
// addressing of marching cubes across block borders.
#pragma once
#include "lk_common.h"
#include "lk_reg_dev.h"

#define LK_TSDF_B 16                                 // voxels per block edge
#define LK_TSDF_BV 4096                              // voxels per block (one plane of a slot)
#define LK_TSDF_PLANES 5                             // tsdf, weight, r, g, b
#define LK_TSDF_BIAS (1 << 20)                       // block coordinate + bias is what a key packs, 21 bits per axis
#define LK_TSDF_NO_KEY ((int64_t)-1)

struct LkTsdfCam {                                   // passed by value
    float m[12];                                     // row-major 3 x 4: camera -> world (touch) or world -> camera (integrate), OpenCV axes
    float fx, fy, cx, cy;
    int H, W;
};

__device__ __forceinline__ int64_t lk_tsdf_key(int bx, int by, int bz) {
    return ((int64_t)(bx + LK_TSDF_BIAS) << 42) | ((int64_t)(by + LK_TSDF_BIAS) << 21) | (int64_t)(bz + LK_TSDF_BIAS);
}
__device__ __forceinline__ void lk_tsdf_unkey(int64_t key, int& bx, int& by, int& bz) {
    bx = (int)((key >> 42) & 0x1fffff) - LK_TSDF_BIAS;
    by = (int)((key >> 21) & 0x1fffff) - LK_TSDF_BIAS;
    bz = (int)(key & 0x1fffff) - LK_TSDF_BIAS;
}
__device__ __forceinline__ bool lk_tsdf_coord_ok(int b) { return b >= -LK_TSDF_BIAS && b < LK_TSDF_BIAS; }

// centre of voxel i of block b along one axis
__device__ __forceinline__ float lk_tsdf_centre(int b, int i, float voxel) {
    return __fmul_rn(__fadd_rn((float)(LK_TSDF_B * b + i), 0.5f), voxel);
}

__device__ __forceinline__ int lk_tsdf_voxel(int i, int j, int k) { return (k * LK_TSDF_B + j) * LK_TSDF_B + i; }
__device__ __forceinline__ size_t lk_tsdf_plane(int slot, int plane) { return ((size_t)slot * LK_TSDF_PLANES + plane) * LK_TSDF_BV; }

// Marching cubes: voxel (i, j, k) with coordinates in [0, 16] seen from block `pos` (position among the sorted keys).  nbr[pos][o],
// o = (i >> 4) | (j >> 4) << 1 | (k >> 4) << 2, is the position of the block the voxel lies in, -1 if that block does not exist.
struct LkMcRef { int pos; int voxel; };
__device__ __forceinline__ LkMcRef lk_mc_ref(const int32_t* __restrict__ nbr, int pos, int i, int j, int k) {
    const int o = (i >> 4) | ((j >> 4) << 1) | ((k >> 4) << 2);
    LkMcRef r;
    r.pos = o == 0 ? pos : nbr[(size_t)pos * 8 + o];
    r.voxel = lk_tsdf_voxel(i & 15, j & 15, k & 15);
    return r;
}

// edge e = 4 * axis + b1 + 2 * b2 of the cube at (i, j, k): its lower corner and its axis (lk_mc_table.h)
__device__ __forceinline__ void lk_mc_edge(int e, int i, int j, int k, int& ei, int& ej, int& ek, int& axis) {
    axis = e >> 2;
    const int b1 = e & 1, b2 = (e >> 1) & 1;
    ei = i + (axis == 0 ? 0 : b1);
    ej = j + (axis == 0 ? b1 : (axis == 1 ? 0 : b2));
    ek = k + (axis == 2 ? 0 : b2);
}
