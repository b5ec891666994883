// Place recognition (include/loopy_hip.h, "place recognition"): an ORB-like binary descriptor of a keyframe and the brute-force
// descriptor match that scores a query frame against every database segment.  Integer arithmetic from the grey image onward: no
// floating point after the one fused multiply-add per channel, no floating-point atomic, every thread owns what it writes - equal
// inputs give equal bits, and tests/place_referee.py states the same contract in NumPy.
//
//   k_place_grey       colour [H][W][3] fp32 -> grey level 0 (uint8)
//   k_place_pyr        level l -> level l + 1 (ratio 6/5, bilinear in integer tenths)
//   k_place_corners    FAST-9 + integer Harris from a 24 x 24 LDS tile (16 x 16 pixels, 4-pixel halo) -> int64 score per pixel
//   k_place_nms        3 x 3 non-maximum suppression among corners -> key mask (compacted by lk_compact_large)
//   k_place_level_counts  candidates per level from the compacted (ascending) index list
//   k_place_smooth     separable binomial [1 6 15 20 15 6 1], undivided uint32 sums, from a 22 x 22 LDS tile
//   k_place_describe   one wave per keypoint: moments over the radius-15 disc, orientation bin, 256 tests packed by ballots
//   k_place_match      best / second-best Hamming distance and best index per row, both directions, the other set through LDS
//   k_place_score      per segment: query rows whose best match is mutual, near enough and distinctive
#include "lk_common.h"

#define PL_TILE 16
#define PL_HALO 4
#define PL_TW (PL_TILE + 2 * PL_HALO)        // 24
#define PL_SH 3                              // halo of the smoothing tile
#define PL_SW (PL_TILE + 2 * PL_SH)          // 22
#define PL_NONE INT64_MIN                    // score of a pixel that is no corner

struct PlLevels {
    int n;
    int h[LK_PLACE_MAX_LEVELS], w[LK_PLACE_MAX_LEVELS];
    int off[LK_PLACE_MAX_LEVELS + 1];        // first pixel of each level in the concatenated arrays; off[n] = total
};

static PlLevels pl_levels(int H, int W, int n_levels) {
    PlLevels L;
    L.n = n_levels;
    int h = H, w = W, off = 0;
    for (int l = 0; l < LK_PLACE_MAX_LEVELS; ++l) {
        L.h[l] = l < n_levels ? h : 0;
        L.w[l] = l < n_levels ? w : 0;
        L.off[l] = off;
        if (l < n_levels) off += h * w;
        h = 5 * h / 6;
        w = 5 * w / 6;
    }
    L.off[LK_PLACE_MAX_LEVELS] = off;
    for (int l = n_levels; l <= LK_PLACE_MAX_LEVELS; ++l) L.off[l] = off;
    return L;
}

static inline int64_t pl_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

struct PlLayout { int64_t P, grey, smooth, score, mask, index, count, scratch, bytes; };
static PlLayout pl_layout(const PlLevels& L) {
    PlLayout o;
    o.P = L.off[L.n];
    const int64_t P = o.P > 0 ? o.P : 1;
    int64_t at = 0;
    o.grey = at;    at = pl_align(at + P);
    o.smooth = at;  at = pl_align(at + 4 * P);
    o.score = at;   at = pl_align(at + 8 * P);
    o.mask = at;    at = pl_align(at + P);
    o.index = at;   at = pl_align(at + 4 * P);
    o.count = at;   at = pl_align(at + 4);
    o.scratch = at; at = pl_align(at + 4 * (int64_t)lk_cdiv(P, 256) + 4);
    o.bytes = at;
    return o;
}

// ------------------------------------------------------------------ grey image and pyramid
__device__ __forceinline__ int pl_quant(float c) {
    const float v = fmaf(c, 255.0f, 0.5f);
    if (!(v > 0.0f)) return 0;               // negative, zero and NaN
    return v >= 255.0f ? 255 : (int)v;
}

__global__ __launch_bounds__(256) void k_place_grey(const float* __restrict__ color, int n, uint8_t* __restrict__ grey) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int q0 = pl_quant(color[3 * (size_t)i]), q1 = pl_quant(color[3 * (size_t)i + 1]), q2 = pl_quant(color[3 * (size_t)i + 2]);
    grey[i] = (uint8_t)((1868 * q0 + 9617 * q1 + 4899 * q2 + 8192) >> 14);
}

__global__ __launch_bounds__(256) void k_place_pyr(const uint8_t* __restrict__ src, int sh, int sw, uint8_t* __restrict__ dst, int dh, int dw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= dh * dw) return;
    const int y = i / dw, x = i - y * dw;
    const int ty = 12 * y + 1, tx = 12 * x + 1;
    const int y0 = min(ty / 10, sh - 1), x0 = min(tx / 10, sw - 1), fy = ty % 10, fx = tx % 10;
    const int y1 = min(y0 + 1, sh - 1), x1 = min(x0 + 1, sw - 1);
    const int a = src[(size_t)y0 * sw + x0], b = src[(size_t)y0 * sw + x1], c = src[(size_t)y1 * sw + x0], d = src[(size_t)y1 * sw + x1];
    const int sum = (10 - fy) * ((10 - fx) * a + fx * b) + fy * ((10 - fx) * c + fx * d);
    dst[i] = (uint8_t)((sum + 50) / 100);
}

// ------------------------------------------------------------------ corners: FAST-9, Harris score
// `m` has bit k set for circle pixel k: is there a run of 9 consecutive set bits on the 16-pixel circle?
__device__ __forceinline__ bool pl_run9(unsigned m) {
    unsigned d = m | (m << 16);
    d &= d >> 1;
    d &= d >> 2;
    d &= d >> 4;
    d &= d >> 1;
    return (d & 0xffffu) != 0u;
}

__global__ __launch_bounds__(256) void k_place_corners(const uint8_t* __restrict__ img, int h, int w, int64_t* __restrict__ score) {
    __shared__ uint8_t tile[PL_TW][PL_TW + 8];
    const int bx = blockIdx.x * PL_TILE, by = blockIdx.y * PL_TILE;
    for (int t = threadIdx.x; t < PL_TW * PL_TW; t += 256) {
        const int ty = t / PL_TW, tx = t - ty * PL_TW;
        const int gy = min(max(by + ty - PL_HALO, 0), h - 1), gx = min(max(bx + tx - PL_HALO, 0), w - 1);
        tile[ty][tx] = img[(size_t)gy * w + gx];
    }
    __syncthreads();
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const int x = bx + lx, y = by + ly;
    if (x >= w || y >= h) return;
    int64_t out = PL_NONE;
    if (x >= LK_PLACE_BORDER && y >= LK_PLACE_BORDER && x < w - LK_PLACE_BORDER && y < h - LK_PLACE_BORDER) {
        const int cx = lx + PL_HALO, cy = ly + PL_HALO;
        const int p = tile[cy][cx];
        const int ox[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
        const int oy[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
        unsigned bright = 0u, dark = 0u;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int v = tile[cy + oy[k]][cx + ox[k]];
            bright |= (unsigned)(v > p + LK_PLACE_FAST_T) << k;
            dark |= (unsigned)(v < p - LK_PLACE_FAST_T) << k;
        }
        if (pl_run9(bright) || pl_run9(dark)) {
            int a = 0, b = 0, c = 0;
            for (int dy = -3; dy <= 3; ++dy)
                for (int dx = -3; dx <= 3; ++dx) {
                    const int yy = cy + dy, xx = cx + dx;
                    const int ix = (tile[yy - 1][xx + 1] + 2 * tile[yy][xx + 1] + tile[yy + 1][xx + 1]) -
                                   (tile[yy - 1][xx - 1] + 2 * tile[yy][xx - 1] + tile[yy + 1][xx - 1]);
                    const int iy = (tile[yy + 1][xx - 1] + 2 * tile[yy + 1][xx] + tile[yy + 1][xx + 1]) -
                                   (tile[yy - 1][xx - 1] + 2 * tile[yy - 1][xx] + tile[yy - 1][xx + 1]);
                    a += ix * ix;
                    b += ix * iy;
                    c += iy * iy;
                }
            const int64_t A = a, B = b, Cc = c;
            out = 25 * (A * Cc - B * B) - (A + Cc) * (A + Cc);
        }
    }
    score[(size_t)y * w + x] = out;
}

// key[i] = 1 for a corner that no corner among its 8 neighbours beats under (score descending, flat index ascending)
__global__ __launch_bounds__(256) void k_place_nms(const int64_t* __restrict__ score, int h, int w, uint8_t* __restrict__ key) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, x = i - y * w;
    const int64_t r = score[i];
    bool keep = r != PL_NONE;
    if (keep) {
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int yy = y + dy, xx = x + dx;
                if ((dy == 0 && dx == 0) || yy < 0 || xx < 0 || yy >= h || xx >= w) continue;
                const int j = yy * w + xx;
                const int64_t q = score[j];
                if (q != PL_NONE && (q > r || (q == r && j < i))) keep = false;
            }
    }
    key[i] = keep ? 1 : 0;
}

// index[0 .. *count) ascending: out[l] = entries in [off[l], off[l + 1])
__global__ void k_place_level_counts(const int32_t* __restrict__ index, const int32_t* __restrict__ count, PlLevels L, int32_t* __restrict__ out) {
    const int l = threadIdx.x;
    if (l >= L.n) return;
    const int n = *count;
    int pos[2];
    for (int e = 0; e < 2; ++e) {
        const int bound = L.off[l + e];
        int lo = 0, hi = n;                  // first position with index >= bound
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (index[mid] < bound) lo = mid + 1; else hi = mid;
        }
        pos[e] = lo;
    }
    out[l] = pos[1] - pos[0];
}

// ------------------------------------------------------------------ binomial smoothing
__global__ __launch_bounds__(256) void k_place_smooth(const uint8_t* __restrict__ img, int h, int w, uint32_t* __restrict__ out) {
    __shared__ uint8_t tile[PL_SW][PL_SW + 2];
    __shared__ uint32_t rows[PL_SW][PL_TILE];
    const int bx = blockIdx.x * PL_TILE, by = blockIdx.y * PL_TILE;
    for (int t = threadIdx.x; t < PL_SW * PL_SW; t += 256) {
        const int ty = t / PL_SW, tx = t - ty * PL_SW;
        const int gy = min(max(by + ty - PL_SH, 0), h - 1), gx = min(max(bx + tx - PL_SH, 0), w - 1);
        tile[ty][tx] = img[(size_t)gy * w + gx];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < PL_SW * PL_TILE; t += 256) {
        const int ty = t / PL_TILE, tx = t - ty * PL_TILE;
        const uint8_t* r = &tile[ty][tx];
        rows[ty][tx] = (uint32_t)(r[0] + r[6]) + 6u * (uint32_t)(r[1] + r[5]) + 15u * (uint32_t)(r[2] + r[4]) + 20u * (uint32_t)r[3];
    }
    __syncthreads();
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const int x = bx + lx, y = by + ly;
    if (x >= w || y >= h) return;
    out[(size_t)y * w + x] = (rows[ly][lx] + rows[ly + 6][lx]) + 6u * (rows[ly + 1][lx] + rows[ly + 5][lx]) +
                             15u * (rows[ly + 2][lx] + rows[ly + 4][lx]) + 20u * rows[ly + 3][lx];
}

// ------------------------------------------------------------------ descriptor
// One wave per keypoint.  sel[k]: the keypoint's pixel in the concatenated level arrays.
__global__ __launch_bounds__(256) void k_place_describe(const uint8_t* __restrict__ grey, const uint32_t* __restrict__ smooth, PlLevels L,
                                                        const int32_t* __restrict__ sel, int N, const int32_t* __restrict__ cs /*[2][30]*/,
                                                        const int8_t* __restrict__ pattern /*[30][256][4]*/, int32_t* __restrict__ kp,
                                                        uint32_t* __restrict__ desc) {
    const int k = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = lk_lane();
    if (k >= N) return;                                      // whole waves leave together
    const int g = sel[k];
    int lev = 0;
    for (int l = 1; l < L.n; ++l) lev += (g >= L.off[l]) ? 1 : 0;
    const int w = L.w[lev], h = L.h[lev];
    const int i = g - L.off[lev];
    const int y = i / w, x = i - y * w;
    // what a keypoint of this library never is: too close to the edge for the disc and the pattern (checked, not assumed)
    const bool inside = g >= 0 && g < L.off[L.n] && x >= LK_PLACE_BORDER && y >= LK_PLACE_BORDER && x < w - LK_PLACE_BORDER && y < h - LK_PLACE_BORDER;
    int bin = 0;
    uint32_t word_lo[4] = {0u, 0u, 0u, 0u}, word_hi[4] = {0u, 0u, 0u, 0u};
    if (inside) {
        const uint8_t* __restrict__ img = grey + L.off[lev];
        const uint32_t* __restrict__ sm = smooth + L.off[lev];
        int m10 = 0, m01 = 0;
        for (int t = lane; t < 31 * 31; t += 64) {
            const int dy = t / 31 - 15, dx = t % 31 - 15;
            if (dx * dx + dy * dy <= 225) {
                const int v = img[(size_t)(y + dy) * w + (x + dx)];
                m10 += dx * v;
                m01 += dy * v;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            m10 += __shfl_xor(m10, o);
            m01 += __shfl_xor(m01, o);
        }
        long long best = 0;
        for (int b = 0; b < LK_PLACE_BINS; ++b) {
            const long long v = (long long)m10 * cs[b] + (long long)m01 * cs[LK_PLACE_BINS + b];
            if (b == 0 || v > best) { best = v; bin = b; }
        }
        const int8_t* __restrict__ pat = pattern + (size_t)bin * 1024;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int8_t* q = pat + 4 * (64 * r + lane);
            // (the contract's tables stay within 17 pixels; a caller's table that does not is held inside the image)
            const int ax = min(max(x + q[0], 0), w - 1), ay = min(max(y + q[1], 0), h - 1);
            const int bx = min(max(x + q[2], 0), w - 1), by = min(max(y + q[3], 0), h - 1);
            const uint32_t sa = sm[(size_t)ay * w + ax], sb = sm[(size_t)by * w + bx];
            const unsigned long long bits = __ballot(sa < sb);
            word_lo[r] = (uint32_t)bits;
            word_hi[r] = (uint32_t)(bits >> 32);
        }
    }
    if (lane == 0) {
        kp[4 * (size_t)k + 0] = x; kp[4 * (size_t)k + 1] = y; kp[4 * (size_t)k + 2] = lev; kp[4 * (size_t)k + 3] = bin;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            desc[8 * (size_t)k + 2 * r] = word_lo[r];
            desc[8 * (size_t)k + 2 * r + 1] = word_hi[r];
        }
    }
}

// ------------------------------------------------------------------ match and score
// grid (row tiles, segments, 2): direction 0 = every query row against the segment's rows, 1 = every row of the segment against the query.
// rows [S][2][F][3] = (best, second, index of the best).
__global__ __launch_bounds__(256) void k_place_match(const uint32_t* __restrict__ query, int nq, const uint32_t* __restrict__ db,
                                                     const int32_t* __restrict__ counts, int F, int32_t* __restrict__ rows) {
    __shared__ uint32_t other[8][256];              // word-major: the tile's store is conflict-free, its reads are broadcasts
    const int s = blockIdx.y, dir = blockIdx.z;
    const int nt = min(max(counts[s], 0), F);
    const uint32_t* __restrict__ seg = db + (size_t)s * F * 8;
    const uint32_t* __restrict__ A = dir == 0 ? query : seg;
    const uint32_t* __restrict__ B = dir == 0 ? seg : query;
    const int na = dir == 0 ? nq : nt, nb = dir == 0 ? nt : nq;
    if ((int)blockIdx.x * 256 >= na) return;                 // uniform over the workgroup
    const int i = blockIdx.x * 256 + threadIdx.x;
    uint32_t a[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (i < na) {
#pragma unroll
        for (int c = 0; c < 8; ++c) a[c] = A[8 * (size_t)i + c];
    }
    int best = LK_PLACE_NO_MATCH, second = LK_PLACE_NO_MATCH, idx = -1;
    for (int j0 = 0; j0 < nb; j0 += 256) {
        __syncthreads();
        const int jn = min(256, nb - j0);
        if ((int)threadIdx.x < jn) {
#pragma unroll
            for (int c = 0; c < 8; ++c) other[c][threadIdx.x] = B[8 * (size_t)(j0 + threadIdx.x) + c];
        }
        __syncthreads();
        for (int j = 0; j < jn; ++j) {
            int d = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) d += __popc(a[c] ^ other[c][j]);
            if (d < best) { second = best; best = d; idx = j0 + j; }
            else if (d < second) second = d;
        }
    }
    if (i < na) {
        int32_t* o = rows + (((size_t)s * 2 + dir) * F + i) * 3;
        o[0] = best; o[1] = second; o[2] = idx;
    }
}

__global__ __launch_bounds__(256) void k_place_score(const int32_t* __restrict__ rows, int nq, const int32_t* __restrict__ counts, int F,
                                                     int max_hamming, int32_t* __restrict__ out) {
    __shared__ int part[4];
    const int s = blockIdx.x;
    const int nt = min(max(counts[s], 0), F);
    const int32_t* __restrict__ fw = rows + (size_t)s * 2 * F * 3;
    const int32_t* __restrict__ bw = fw + (size_t)F * 3;
    int n = 0;
    for (int i0 = 0; i0 < nq; i0 += 256) {
        const int i = i0 + threadIdx.x;
        bool ok = false;
        if (i < nq) {
            const int best = fw[3 * i], second = fw[3 * i + 1], j = fw[3 * i + 2];
            ok = j >= 0 && j < nt && bw[3 * j + 2] == i && best <= max_hamming && 5 * best <= 4 * second;
        }
        n += __popcll(__ballot(ok));
    }
    if (lk_lane() == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) out[s] = part[0] + part[1] + part[2] + part[3];
}

// ------------------------------------------------------------------ C ABI
static int pl_check_image(int H, int W, int n_levels, const char* who) {
    if (!(H > 0 && W > 0 && n_levels >= 1 && n_levels <= LK_PLACE_MAX_LEVELS && (int64_t)H * W <= (int64_t)LK_PLACE_MAX_PIXELS)) {
        lk_set_error("%s: 0 < H, W, H W <= %d and 1 <= n_levels <= %d are required", who, LK_PLACE_MAX_PIXELS, LK_PLACE_MAX_LEVELS);
        return LK_ERR_ARG;
    }
    return LK_OK;
}

extern "C" int lk_place_ws_bytes(int32_t H, int32_t W, int32_t n_levels, int64_t* out_layout) {
    LK_REQUIRE(out_layout != nullptr, "lk_place_ws_bytes: NULL output");
    if (int rc = pl_check_image(H, W, n_levels, "lk_place_ws_bytes")) return rc;
    const PlLayout o = pl_layout(pl_levels(H, W, n_levels));
    out_layout[0] = o.bytes; out_layout[1] = o.P; out_layout[2] = o.grey; out_layout[3] = o.smooth;
    out_layout[4] = o.score; out_layout[5] = o.index; out_layout[6] = o.count; out_layout[7] = o.mask;
    return LK_OK;
}

extern "C" int lk_place_detect(const float* color, int32_t H, int32_t W, int32_t n_levels, void* ws, int32_t* out_level_counts, void* stream_) {
    if (int rc = pl_check_image(H, W, n_levels, "lk_place_detect")) return rc;
    LK_REQUIRE(color && ws && out_level_counts, "lk_place_detect: NULL buffer");
    LK_REQUIRE(((uintptr_t)ws & 7u) == 0, "lk_place_detect: the workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream_;
    const PlLevels L = pl_levels(H, W, n_levels);
    const PlLayout o = pl_layout(L);
    char* base = (char*)ws;
    uint8_t* grey = (uint8_t*)(base + o.grey);
    uint32_t* smooth = (uint32_t*)(base + o.smooth);
    int64_t* score = (int64_t*)(base + o.score);
    uint8_t* mask = (uint8_t*)(base + o.mask);
    int32_t* index = (int32_t*)(base + o.index);
    int32_t* count = (int32_t*)(base + o.count);
    int32_t* scratch = (int32_t*)(base + o.scratch);
    hipLaunchKernelGGL(k_place_grey, dim3(lk_cdiv((int64_t)H * W, 256)), dim3(256), 0, st, color, H * W, grey);
    for (int l = 0; l < n_levels; ++l) {
        const int h = L.h[l], w = L.w[l];
        if (h * w == 0) continue;
        if (l > 0)
            hipLaunchKernelGGL(k_place_pyr, dim3(lk_cdiv((int64_t)h * w, 256)), dim3(256), 0, st, (const uint8_t*)(grey + L.off[l - 1]), L.h[l - 1],
                               L.w[l - 1], grey + L.off[l], h, w);
        const dim3 tiles(lk_cdiv(w, PL_TILE), lk_cdiv(h, PL_TILE));
        hipLaunchKernelGGL(k_place_corners, tiles, dim3(256), 0, st, (const uint8_t*)(grey + L.off[l]), h, w, score + L.off[l]);
        hipLaunchKernelGGL(k_place_nms, dim3(lk_cdiv((int64_t)h * w, 256)), dim3(256), 0, st, (const int64_t*)(score + L.off[l]), h, w, mask + L.off[l]);
        hipLaunchKernelGGL(k_place_smooth, tiles, dim3(256), 0, st, (const uint8_t*)(grey + L.off[l]), h, w, smooth + L.off[l]);
    }
    LK_LAUNCH_CHECK();
    if (int rc = lk_compact_large(mask, (int32_t)o.P, index, count, scratch, stream_)) return rc;
    hipLaunchKernelGGL(k_place_level_counts, dim3(1), dim3(64), 0, st, (const int32_t*)index, (const int32_t*)count, L, out_level_counts);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

extern "C" int lk_place_describe(const void* ws, int32_t H, int32_t W, int32_t n_levels, const int32_t* sel, int32_t N, const int32_t* cos_sin,
                                 const int8_t* pattern, int32_t* out_kp, uint32_t* out_desc, void* stream_) {
    if (int rc = pl_check_image(H, W, n_levels, "lk_place_describe")) return rc;
    LK_REQUIRE(N >= 0, "lk_place_describe: N < 0");
    if (N == 0) return LK_OK;
    LK_REQUIRE(ws && sel && cos_sin && pattern && out_kp && out_desc, "lk_place_describe: NULL buffer");
    const PlLevels L = pl_levels(H, W, n_levels);
    const PlLayout o = pl_layout(L);
    const char* base = (const char*)ws;
    hipLaunchKernelGGL(k_place_describe, dim3(lk_cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream_, (const uint8_t*)(base + o.grey),
                       (const uint32_t*)(base + o.smooth), L, sel, (int)N, cos_sin, pattern, out_kp, out_desc);
    LK_LAUNCH_CHECK();
    return LK_OK;
}

extern "C" int lk_place_match_score(const uint32_t* query, int32_t n_query, const uint32_t* db, const int32_t* counts, int32_t S, int32_t F,
                                    int32_t max_hamming, int32_t* rows, int32_t* out_count, void* stream_) {
    LK_REQUIRE(n_query >= 0 && S >= 0 && F >= 1 && n_query <= F && S <= 65535, "lk_place_match_score: 0 <= n_query <= F, 0 <= S <= 65535 are required");
    if (S == 0) return LK_OK;
    LK_REQUIRE(db && counts && rows && out_count && (n_query == 0 || query), "lk_place_match_score: NULL buffer");
    hipStream_t st = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_place_match, dim3(lk_cdiv(F, 256), S, 2), dim3(256), 0, st, query, (int)n_query, db, counts, (int)F, rows);
    hipLaunchKernelGGL(k_place_score, dim3(S), dim3(256), 0, st, (const int32_t*)rows, (int)n_query, counts, (int)F, (int)max_hamming, out_count);
    LK_LAUNCH_CHECK();
    return LK_OK;
}
