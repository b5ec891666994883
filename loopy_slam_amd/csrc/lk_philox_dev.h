// The counter-based generator of the library's random draws (lk_ransac_hypotheses, lk_mesh_sample): one copy for every translation unit.
// tests/greg_referee.py::philox is its referee.
#pragma once
#include "lk_common.h"

// Philox4x32-10 (Salmon et al. 2011), key = (seed low, seed high), counter = (trial low, trial high, 0, 0); loopy_hip.h writes the rule out.
__device__ __forceinline__ void lk_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t (&r)[4]) {
    uint32_t c2 = 0u, c3 = 0u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}
