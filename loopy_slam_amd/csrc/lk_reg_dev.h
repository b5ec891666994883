// What the two loop-closure files (lk_reg.hip, lk_greg.hip) share on the device: the lanes-per-point group, the 3 x 4 rigid map and the
// cyclic Jacobi rotation.  The radius box over the uniform grid is in lk_knn_dev.h (lk_grid_box / lk_box_rows), beside the index's search.
#pragma once
#include "lk_common.h"

#define LK_REG_T 8                                  // lanes per point (as the standalone search at size)
#define LK_REG_GROUPS (256 / LK_REG_T)              // points a workgroup of 256 works on at a time

// p <- M p, M row-major 3 x 4 (LkMat12::m, a row of `mats` in global memory, a local T[12]).  The fma nesting is the contract: per coordinate
// fma(m0, x, fma(m1, y, fma(m2, z, m3))).
__device__ __forceinline__ void lk_rigid_apply(const float* m, float x, float y, float z, float& ox, float& oy, float& oz) {
    ox = __fmaf_rn(m[0], x, __fmaf_rn(m[1], y, __fmaf_rn(m[2], z, m[3])));
    oy = __fmaf_rn(m[4], x, __fmaf_rn(m[5], y, __fmaf_rn(m[6], z, m[7])));
    oz = __fmaf_rn(m[8], x, __fmaf_rn(m[9], y, __fmaf_rn(m[10], z, m[11])));
}

// One rotation of the cyclic Jacobi method on the symmetric N x N matrix a: zeroes a[P][Q], accumulates the eigenvectors in the columns
// of v, in the scalar type S (std:: overloads: fp32 stays fp32).  Sweep counts, the choice of the eigenvector and its normalisation are
// the caller's.
template <int N, int P, int Q, class S>
__device__ __forceinline__ void lk_jacobi_rot(S (&a)[N][N], S (&v)[N][N]) {
    const S apq = a[P][Q];
    if (apq == S(0)) return;
    const S theta = (a[Q][Q] - a[P][P]) / (S(2) * apq);
    const S t = (theta >= S(0) ? S(1) : S(-1)) / (std::fabs(theta) + std::sqrt(theta * theta + S(1)));
    const S c = S(1) / std::sqrt(t * t + S(1)), s = t * c;
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = S(0); a[Q][P] = S(0);
#pragma unroll
    for (int r = 0; r < N; ++r) {
        if (r != P && r != Q) {
            const S arp = a[r][P], arq = a[r][Q];
            a[r][P] = c * arp - s * arq; a[P][r] = a[r][P];
            a[r][Q] = s * arp + c * arq; a[Q][r] = a[r][Q];
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const S vp = v[k][P], vq = v[k][Q];
        v[k][P] = c * vp - s * vq;
        v[k][Q] = s * vp + c * vq;
    }
}
