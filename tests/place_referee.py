"""NumPy referee of the place-recognition contract (include/loopy_hip.h, "place recognition"), integers throughout, written from the contract's
text: whole-image array operations where the kernels walk tiles and waves, its own Philox and its own pattern tables."""
import numpy as np

BORDER, FAST_T, BINS, SEED, NO_MATCH = 20, 20, 30, 0x4F524221, 257
CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
BINOMIAL = (1, 6, 15, 20, 15, 6, 1)


# ------------------------------------------------------------------------------------------------ tables
def philox_words(key, counter0, counter1):
    """Ten rounds on one counter (python integers): the four output words."""
    c = [counter0 & 0xFFFFFFFF, counter1 & 0xFFFFFFFF, 0, 0]
    k0, k1 = key & 0xFFFFFFFF, 0
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


_TABLES = []


def tables():
    """(cos_sin int32 [2,30], pattern int8 [30,256,4])."""
    if not _TABLES:
        base = np.array([[sum(u % 7 for u in philox_words(SEED, i, c)) - 12 for c in range(4)] for i in range(256)], dtype=np.int64)
        cos_sin = np.zeros((2, BINS), dtype=np.int32)
        pattern = np.zeros((BINS, 256, 4), dtype=np.int8)
        theta = np.arange(BINS, dtype=np.float64) * (np.pi / 15.0)            # 12 degrees a bin
        cos_all, sin_all = np.cos(theta), np.sin(theta)
        for k in range(BINS):
            c, s = cos_all[k], sin_all[k]
            cos_sin[0, k], cos_sin[1, k] = np.rint(16384.0 * c), np.rint(16384.0 * s)
            for p in (0, 2):
                x, y = base[:, p].astype(np.float64), base[:, p + 1].astype(np.float64)
                pattern[k, :, p], pattern[k, :, p + 1] = np.rint(c * x - s * y), np.rint(s * x + c * y)
        _TABLES.extend([cos_sin, pattern])
    return _TABLES[0], _TABLES[1]


def quotas(n_features, n_levels):
    f = 5.0 / 6.0
    d = n_features * (1.0 - f) / (1.0 - f ** n_levels)
    out = []
    for _ in range(n_levels - 1):
        out.append(int(np.floor(d + 0.5)))
        d = d * f
    out.append(max(n_features - sum(out), 0))
    return out


# ------------------------------------------------------------------------------------------------ image
def grey_image(color):
    """color [H,W,3] float32 -> int64 [H,W] in 0 .. 255."""
    v = (color.astype(np.float64) * 255.0 + 0.5).astype(np.float32)        # exact product and sum in fp64, one rounding: the fused multiply-add
    v = np.where(np.isnan(v), np.float32(0.0), v)
    q = np.clip(np.trunc(np.clip(v, -1.0, 256.0)).astype(np.int64), 0, 255)
    return (1868 * q[..., 0] + 9617 * q[..., 1] + 4899 * q[..., 2] + 8192) >> 14


def next_level(img):
    def taps(n):
        m = 5 * n // 6
        t = 12 * np.arange(m, dtype=np.int64) + 1
        i0 = np.minimum(t // 10, n - 1)
        return i0, np.minimum(i0 + 1, n - 1), t % 10
    y0, y1, fy = taps(img.shape[0])
    x0, x1, fx = taps(img.shape[1])
    wy0, wy1, wx0, wx1 = (10 - fy)[:, None], fy[:, None], (10 - fx)[None, :], fx[None, :]
    s = wy0 * (wx0 * img[np.ix_(y0, x0)] + wx1 * img[np.ix_(y0, x1)]) + wy1 * (wx0 * img[np.ix_(y1, x0)] + wx1 * img[np.ix_(y1, x1)])
    return (s + 50) // 100


def pyramid(color, n_levels):
    out = [grey_image(color)]
    for _ in range(n_levels - 1):
        out.append(next_level(out[-1]))
    return out


def shifted(img, dx, dy):
    """img(x + dx, y + dy) for every pixel, edge-clamped."""
    h, w = img.shape
    ys, xs = np.clip(np.arange(h) + dy, 0, h - 1), np.clip(np.arange(w) + dx, 0, w - 1)
    return img[np.ix_(ys, xs)]


def corners(img):
    """(is corner [h,w] bool, Harris R [h,w] as python-exact int64)."""
    h, w = img.shape
    ring = np.stack([shifted(img, dx, dy) for dx, dy in CIRCLE])          # [16,h,w]
    hit = np.zeros((h, w), dtype=bool)
    for sign in (1, -1):
        far = (sign * (ring - img[None]) > FAST_T)
        for start in range(16):
            run = np.ones((h, w), dtype=bool)
            for k in range(9):
                run &= far[(start + k) % 16]
            hit |= run
    inside = np.zeros((h, w), dtype=bool)
    if h > 2 * BORDER and w > 2 * BORDER:
        inside[BORDER:h - BORDER, BORDER:w - BORDER] = True
    hit &= inside
    ix = (shifted(img, 1, -1) + 2 * shifted(img, 1, 0) + shifted(img, 1, 1)) - (shifted(img, -1, -1) + 2 * shifted(img, -1, 0) + shifted(img, -1, 1))
    iy = (shifted(img, -1, 1) + 2 * shifted(img, 0, 1) + shifted(img, 1, 1)) - (shifted(img, -1, -1) + 2 * shifted(img, 0, -1) + shifted(img, 1, -1))

    def block(v):
        return sum(shifted(v, dx, dy) for dy in range(-3, 4) for dx in range(-3, 4))
    a, b, c = block(ix * ix), block(ix * iy), block(iy * iy)
    return hit, 25 * (a * c - b * b) - (a + c) ** 2


def keys_of_level(img):
    """Flat pixels of the level's keys in the order (R descending, pixel ascending), and their R."""
    hit, R = corners(img)
    h, w = img.shape
    flat = np.arange(h * w).reshape(h, w)
    keep = hit.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            ys, xs = np.arange(h) + dy, np.arange(w) + dx
            ok = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
            nh, nr, nf = shifted(hit, dx, dy) & ok, shifted(R, dx, dy), shifted(flat, dx, dy)
            keep &= ~(nh & ((nr > R) | ((nr == R) & (nf < flat))))
    idx = flat[keep]
    order = np.lexsort((idx, -R[keep]))
    return idx[order], R[keep][order]


def smoothed(img):
    along_x = sum(wt * shifted(img, k - 3, 0) for k, wt in enumerate(BINOMIAL))
    return sum(wt * shifted(along_x, 0, k - 3) for k, wt in enumerate(BINOMIAL))


_DISC = [(dx, dy) for dy in range(-15, 16) for dx in range(-15, 16) if dx * dx + dy * dy <= 225]


def describe(color, n_features=500, n_levels=8):
    """(kp int32 [N,4], desc uint32 [N,8])."""
    cos_sin, pattern = tables()
    dx, dy = np.array([d[0] for d in _DISC]), np.array([d[1] for d in _DISC])
    kps, descs = [], []
    for lev, (img, quota) in enumerate(zip(pyramid(color, n_levels), quotas(n_features, n_levels))):
        h, w = img.shape
        if h <= 2 * BORDER or w <= 2 * BORDER:
            continue
        idx, _ = keys_of_level(img)
        idx = idx[:quota]
        if len(idx) == 0:
            continue
        S = smoothed(img)
        y, x = idx // w, idx % w
        v = img[y[:, None] + dy[None], x[:, None] + dx[None]]
        m10, m01 = (v * dx[None]).sum(1), (v * dy[None]).sum(1)
        proj = m10[:, None] * cos_sin[0].astype(np.int64)[None] + m01[:, None] * cos_sin[1].astype(np.int64)[None]
        bins = np.argmax(proj, axis=1)                                    # the first maximum: the lowest k
        pat = pattern[bins].astype(np.int64)                              # [n,256,4]
        bit = S[y[:, None] + pat[:, :, 1], x[:, None] + pat[:, :, 0]] < S[y[:, None] + pat[:, :, 3], x[:, None] + pat[:, :, 2]]
        words = (bit.reshape(-1, 8, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)[None, None]).sum(2).astype(np.uint32)
        kps.append(np.stack([x, y, np.full_like(x, lev), bins], 1).astype(np.int32))
        descs.append(words)
    if not kps:
        return np.zeros((0, 4), dtype=np.int32), np.zeros((0, 8), dtype=np.uint32)
    return np.concatenate(kps), np.concatenate(descs)


# ------------------------------------------------------------------------------------------------ match and score
_POP8 = np.array([bin(i).count('1') for i in range(256)], dtype=np.int64)


def hamming(A, B):
    """[Na,Nb] distances of uint32 [.,8] descriptor sets."""
    x = A[:, None, :] ^ B[None, :, :]
    if hasattr(np, 'bitwise_count'):
        return np.bitwise_count(x).sum(-1, dtype=np.int64)
    return _POP8[x.view(np.uint8)].sum(-1)


def best_of_rows(d):
    """(best, second, index) int64 [n] of every row of the distance table d [n,m]."""
    n, m = d.shape
    best, second, index = np.full(n, NO_MATCH, dtype=np.int64), np.full(n, NO_MATCH, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    if n and m:
        d = d.copy()
        index = np.argmin(d, axis=1)                    # the first minimum: the lowest row
        best = d[np.arange(n), index]
        if m > 1:
            d[np.arange(n), index] = NO_MATCH + 1
            second = d.min(1)
    return best, second, index


def match(A, B):
    """(best, second, index) int64 [Na] of every row of A over the rows of B."""
    return best_of_rows(hamming(A, B))


def good_count(A, B, max_hamming):
    """The integer of lk_place_match_score and the row records of both directions."""
    d = hamming(A, B)
    fw, bw = best_of_rows(d), best_of_rows(d.T)
    i = np.arange(len(A))
    j = fw[2]
    mutual = (j >= 0) & (bw[2][np.maximum(j, 0)] == i) if len(B) else np.zeros(len(A), dtype=bool)
    good = mutual & (fw[0] <= max_hamming) & (5 * fw[0] <= 4 * fw[1])
    return int(good.sum()), fw, bw


def score(A, B, max_hamming):
    if len(A) == 0 or len(B) == 0:
        return 0.0
    return good_count(A, B, max_hamming)[0] / min(len(A), len(B))
