"""NumPy referee of the global start of loop closure (tests/test_global_registration*.py): the voxel rule, FPFH with Open3D's conventions,
the mutual nearest feature match, the Philox draw of include/loopy_hip.h, the checkers, the 3-point fit and the scoring - the arithmetic in
fp64, the decisions the ABI states in fp32 (voxel keys, neighbourhoods) in fp32.  Nothing here is loaded by the product.

Input: two 30 000-point clouds of the FURNISHED synthetic room, the source sampled from loop poses 0, 3, 6, 9 of 200, the target from poses
5, 8, 11, 14 (three points per ray at 0.98 / 1.0 / 1.02 x depth, as synthetic.build_cloud makes them), the source moved by the inverse of
the planted transform.  The plain room of lc_referee.clouds is no input for a global registration: a near-symmetric box seen in full is
ambiguous by construction.

The planted transform is (40, -25, 70) degrees, (1.2, -0.8, 0.4) m.  With the (25, -15, 40) degrees, (0.8, -0.5, 0.3) m first proposed
for this input the 0.3-m coarse ICP still converges FROM THE IDENTITY (lc_referee.icp, fp64: max |T - T_planted| = 1.45e-3, the same
basin as from the RANSAC start, 1.40e-3), so that pair cannot show what the global start is for; at the enlarged transform the
referee's ICP from the identity finds fewer than six correspondences within 0.3 m and stays at the identity (PLANTED_SMALL keeps the
first proposal)."""
import numpy as np

import lc_referee as R

VOXEL, EDGE_RATIO = 0.04, 0.9
SRC_POSES, TGT_POSES = (0, 3, 6, 9), (5, 8, 11, 14)
SRC_SEED, TGT_SEED = 101, 202
PLANTED = ((40.0, -25.0, 70.0), (1.2, -0.8, 0.4))
PLANTED_SMALL = ((25.0, -15.0, 40.0), (0.8, -0.5, 0.3))
EDGE_SLACK = 1e-4            # a pair feature this close to a bin edge may fall on either side in fp32
REL_SLACK = 1e-5             # a checker or inlier decision this close (relative) to its threshold is a rounding matter
_CACHE = {}


def furnished_cloud(poses, n_points, seed):
    """[n_points,3] fp32 and the first pose's camera centre: n_points / 3 rays spread over the poses, three points per ray."""
    from loopy_slam_amd import synthetic
    return synthetic.furnished_cloud(poses, n_points, seed)


def segment_pair(n=30000, planted=PLANTED):
    """dict(src [n,3] moved by the inverse of the planted transform, tgt [n,3], T the planted 4 x 4, cam_s, cam_t)."""
    key = ('pair', n, planted)
    if key not in _CACHE:
        src0, cam_s = furnished_cloud(SRC_POSES, n, SRC_SEED)
        tgt, cam_t = furnished_cloud(TGT_POSES, n, TGT_SEED)
        T = R.planted(*planted)
        Ti = R.inv4(T)
        _CACHE[key] = {'src': R.move(src0, Ti), 'src0': src0, 'tgt': tgt, 'T': T, 'cam_s': Ti[:3, :3] @ cam_s + Ti[:3, 3], 'cam_t': cam_t}
    return _CACHE[key]


def rot_angle_deg(Ra):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra) - 1.0) / 2.0, -1.0, 1.0))))


def pose_error(T, T_ref):
    """(degrees, metres) between two 4 x 4 transforms."""
    D = R.inv4(T_ref) @ T
    return rot_angle_deg(D[:3, :3]), float(np.linalg.norm(T[:3, 3] - T_ref[:3, 3]))


# ------------------------------------------------------------------------------------------------ voxel downsample
def voxel_downsample(pos, voxel=VOXEL):
    """(centroids [n,3] fp64 in ascending key order, keys [n] int64): key = (kx << 42) | (ky << 21) | kz, k = floor((p - (min - 0.5 v)) / v)
    per axis with the subtraction and the division in fp32, as the ABI states them."""
    p32 = np.ascontiguousarray(pos, dtype=np.float32)
    v = np.float32(voxel)
    origin = p32.min(0) - np.float32(0.5) * v
    k = np.clip(np.floor((p32 - origin) / v), 0, 2097151).astype(np.int64)
    key = (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]
    uk, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    out = np.zeros((len(uk), 3))
    for c in range(3):
        out[:, c] = np.bincount(inv, weights=p32[:, c].astype(np.float64), minlength=len(uk)) / cnt
    return out, uk


# ------------------------------------------------------------------------------------------------ FPFH
def neighbour_pairs(pos32, valid, radius):
    """(i, k, d2 fp32) of every ordered pair k != i with contract d2 <= fl32(radius)^2, both normals valid; sorted by i."""
    p32 = np.ascontiguousarray(pos32, dtype=np.float32)
    r2 = np.float32(radius) * np.float32(radius)
    g = R.Grid(p32, radius * 1.01)
    I, K, D = [], [], []
    for a in range(0, len(p32), 4000):
        qq = p32[a:a + 4000]
        rep, cand, _, _ = g.candidates(qq)
        d2 = R.dist2(qq[rep], p32[cand])
        keep = (d2 <= r2) & (cand != rep + a) & (valid[cand] != 0) & (valid[rep + a] != 0)
        I.append(rep[keep] + a); K.append(cand[keep]); D.append(d2[keep])
    return np.concatenate(I), np.concatenate(K), np.concatenate(D)


def pair_features(p1, n1, p2, n2):
    """Open3D's ComputePairFeatures, vectorised, fp64: [n,3] = (f0, f1, f2)."""
    e = p2 - p1
    d = np.linalg.norm(e, axis=1)
    ok = d > 0
    ds = np.where(ok, d, 1.0)
    a1, a2 = (n1 * e).sum(1) / ds, (n2 * e).sum(1) / ds
    swap = np.abs((n1 * e).sum(1)) < np.abs((n2 * e).sum(1))          # acos|a1| > acos|a2|, without the common division (as the library decides it)
    u = np.where(swap[:, None], n2, n1)
    m = np.where(swap[:, None], n1, n2)
    e = np.where(swap[:, None], -e, e)
    f2 = np.where(swap, -a2, a1)
    v = np.cross(e, u)
    vn = np.linalg.norm(v, axis=1)
    ok &= vn > 0
    v = v / np.where(vn > 0, vn, 1.0)[:, None]
    w = np.cross(u, v)
    f1 = (v * m).sum(1)
    f0 = np.arctan2((w * m).sum(1), (u * m).sum(1))
    return np.where(ok[:, None], np.stack([f0, f1, f2], 1), 0.0)


def spfh(pos32, normals, valid, radius):
    """(spfh [N,33] fp64, neighbours [N], near_edge [N] = pair features of the point within EDGE_SLACK of an inner bin edge)."""
    p64, n64 = np.asarray(pos32, dtype=np.float64), np.asarray(normals, dtype=np.float64)
    N = len(p64)
    I, K, _ = neighbour_pairs(pos32, valid, radius)
    f = pair_features(p64[I], n64[I], p64[K], n64[K])
    cnt = np.bincount(I, minlength=N)
    out = np.zeros((N, 33))
    near = np.zeros(N, dtype=np.int64)
    for c, (lo, width) in enumerate(((-np.pi, 2 * np.pi / 11), (-1.0, 2.0 / 11), (-1.0, 2.0 / 11))):
        x = (f[:, c] - lo) / width
        b = np.clip(np.floor(x), 0, 10).astype(np.int64)
        np.add.at(out, (I, 11 * c + b), 1.0)
        e = np.round(x)
        close = (np.abs(x - e) * width < EDGE_SLACK) & (e >= 1) & (e <= 10)
        near += np.bincount(I[close], minlength=N)
    out *= np.where(cnt > 0, 100.0 / np.maximum(cnt, 1), 0.0)[:, None]
    return out, cnt, near


def fpfh_pass2(spfh_tab, pos32, valid, radius):
    """Pass 2 in fp64 from a given SPFH table, the neighbour distances being the fp32 contract distances."""
    s = np.asarray(spfh_tab, dtype=np.float64)
    N = len(s)
    I, K, d2 = neighbour_pairs(pos32, valid, radius)
    use = d2 > 0
    I, K, d2 = I[use], K[use], d2[use].astype(np.float64)
    acc = np.zeros((N, 33))
    np.add.at(acc, I, s[K] / d2[:, None])
    out = np.zeros((N, 33))
    for blk in range(3):
        sl = slice(11 * blk, 11 * blk + 11)
        tot = acc[:, sl].sum(1)
        out[:, sl] = acc[:, sl] * np.where(tot != 0, 100.0 / np.where(tot != 0, tot, 1.0), 0.0)[:, None]
    out += s
    out[np.asarray(valid) == 0] = 0.0
    return out


def features(pos, camera, voxel=VOXEL):
    """The referee's own preprocess_point_cloud, fp64: dict(pos, normals, valid, fpfh)."""
    down, _ = voxel_downsample(pos, voxel)
    d32 = down.astype(np.float32)
    nrm, cnt, _ = R.normals(d32, 2.0 * voxel, camera)
    valid = (cnt >= 3).astype(np.uint8)
    s, _, _ = spfh(d32, nrm, valid, 5.0 * voxel)
    return {'pos': d32, 'normals': nrm, 'valid': valid, 'fpfh': fpfh_pass2(s, d32, valid, 5.0 * voxel)}


# ------------------------------------------------------------------------------------------------ match
def match(A, valid_a, B, valid_b):
    """Per row of A: (index of the nearest valid row of B under (d2, index) or -1, its d2, the runner-up's d2), fp64."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    Na = len(A)
    idx, d1, d2 = np.full(Na, -1, dtype=np.int64), np.full(Na, np.inf), np.full(Na, np.inf)
    cols = np.nonzero(np.asarray(valid_b) != 0)[0]
    if len(cols) == 0:
        return idx, d1, d2
    Bv = B[cols]
    for a in range(0, Na, 1024):
        blk = A[a:a + 1024]
        g = (blk * blk).sum(1)[:, None] + (Bv * Bv).sum(1)[None] - 2.0 * blk @ Bv.T
        near = np.argsort(g, axis=1, kind='stable')[:, :4]                       # refine the few nearest with direct differences
        dd = ((blk[:, None, :] - Bv[near]) ** 2).sum(2)
        near = np.sort(near, axis=1)                                             # ascending index: the stable sort below keeps (d2, index)
        dd = ((blk[:, None, :] - Bv[near]) ** 2).sum(2)
        o = np.argsort(dd, axis=1, kind='stable')
        r = np.arange(len(blk))
        idx[a:a + 1024], d1[a:a + 1024] = cols[near[r, o[:, 0]]], dd[r, o[:, 0]]
        if near.shape[1] > 1:
            d2[a:a + 1024] = dd[r, o[:, 1]]
    bad = np.asarray(valid_a) == 0
    idx[bad], d1[bad], d2[bad] = -1, np.inf, np.inf
    return idx, d1, d2


def mutual(m_st, m_ts):
    """[M,2] (source, target) in source order: the pairs that choose each other; fewer than three: every source's own choice."""
    m_st, m_ts = np.asarray(m_st, dtype=np.int64), np.asarray(m_ts, dtype=np.int64)
    has = m_st >= 0
    mut = has & (m_ts[np.maximum(m_st, 0)] == np.arange(len(m_st)))
    rows = np.nonzero(mut)[0]
    if len(rows) < 3:
        rows = np.nonzero(has)[0]
    return np.stack([rows, m_st[rows]], 1)


# ------------------------------------------------------------------------------------------------ RANSAC
def philox(seed, trials):
    """Philox4x32-10, key (seed low, seed high), counter (trial low, trial high, 0, 0): [n,4] uint32 as uint64 values."""
    M32 = np.uint64(0xFFFFFFFF)
    t = np.asarray(trials, dtype=np.uint64)
    c = [t & M32, t >> np.uint64(32), np.zeros_like(t), np.zeros_like(t)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, 1)


def draw(seed, trial0, n, M):
    """Triples [n,3] int64: i_k = (r_k x M) >> 32."""
    r = philox(seed, np.arange(trial0, trial0 + n, dtype=np.uint64))
    return ((r[:, :3] * np.uint64(M)) >> np.uint64(32)).astype(np.int64)


def rigid_fit_batch(a, b):
    """Kabsch per row: a, b [n,k,3] -> [n,4,4] taking a onto b (fp64, det = +1)."""
    ma, mb = a.mean(1, keepdims=True), b.mean(1, keepdims=True)
    H = np.einsum('nki,nkj->nij', b - mb, a - ma)
    U, _, Vt = np.linalg.svd(H)
    det = np.linalg.det(U @ Vt)
    D = np.tile(np.eye(3), (len(a), 1, 1))
    D[:, 2, 2] = np.where(det < 0, -1.0, 1.0)
    Rm = U @ D @ Vt
    T = np.tile(np.eye(4), (len(a), 1, 1))
    T[:, :3, :3] = Rm
    T[:, :3, 3] = mb[:, 0] - np.einsum('nij,nj->ni', Rm, ma[:, 0])
    return T


def hypotheses(cs, ct, seed, trial0, n, dist_thr, edge_ratio=EDGE_RATIO):
    """dict(triples [n,3], ok [n] bool, T [n,4,4], near [n] bool = a checker decision within REL_SLACK of its threshold)."""
    cs, ct = np.asarray(cs, dtype=np.float64), np.asarray(ct, dtype=np.float64)
    tri = draw(seed, trial0, n, len(cs))
    ok = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    near = np.zeros(n, dtype=bool)
    s, q = cs[tri], ct[tri]
    for k in range(3):
        l = (k + 1) % 3
        ds, dt = np.linalg.norm(s[:, k] - s[:, l], axis=1), np.linalg.norm(q[:, k] - q[:, l], axis=1)
        ok &= ~((ds < dt * edge_ratio) | (dt < ds * edge_ratio))
        near |= (np.abs(ds - dt * edge_ratio) <= REL_SLACK * ds) | (np.abs(dt - ds * edge_ratio) <= REL_SLACK * dt)
    T = np.tile(np.eye(4), (n, 1, 1))
    rows = np.nonzero(ok | near)[0]
    if len(rows):
        T[rows] = rigid_fit_batch(s[rows], q[rows])
        res = np.linalg.norm(np.einsum('nij,nkj->nki', T[rows, :3, :3], s[rows]) + T[rows, None, :3, 3] - q[rows], axis=2)
        ok[rows] &= ~(res > dist_thr).any(1)
        near[rows] |= (np.abs(res - dist_thr) <= REL_SLACK * dist_thr).any(1)
    return {'triples': tri, 'ok': ok, 'T': T, 'near': near}


def score(cs, ct, T, dist_thr):
    """(inlier count, sum d2, correspondences within REL_SLACK of the threshold) of one 4 x 4 hypothesis over the correspondence set."""
    cs, ct = np.asarray(cs, dtype=np.float64), np.asarray(ct, dtype=np.float64)
    d = np.linalg.norm(cs @ T[:3, :3].T + T[:3, 3] - ct, axis=1)
    inl = d <= dist_thr
    return int(inl.sum()), float((d[inl] ** 2).sum()), int((np.abs(d - dist_thr) <= REL_SLACK * dist_thr).sum())


def ransac(cs, ct, dist_thr, seed=0, conf=0.99999, max_iter=10_000_000, batch=65536):
    """The product's loop in fp64: dict(T refitted over the best hypothesis' inliers, T_best, inliers, trials) or None."""
    cs, ct = np.asarray(cs, dtype=np.float64), np.asarray(ct, dtype=np.float64)
    M = len(cs)
    best, trials, k_stop = None, 0, float(max_iter)
    while M >= 3 and trials < min(k_stop, max_iter):
        n = int(min(batch, max_iter - trials))
        h = hypotheses(cs, ct, seed, trials, n, dist_thr)
        for t in np.nonzero(h['ok'])[0]:
            c, s2, _ = score(cs, ct, h['T'][t], dist_thr)
            cand = (-c, s2, trials + int(t))
            if best is None or cand < best[0]:
                best = (cand, h['T'][t])
        trials += n
        if best is not None and best[0][0] < 0:
            ratio3 = min(-best[0][0] / M, 1.0) ** 3
            k_stop = 0.0 if ratio3 >= 1.0 else np.log(1.0 - conf) / np.log(1.0 - ratio3)
    if best is None:
        return None
    T = best[1]
    inl = np.linalg.norm(cs @ T[:3, :3].T + T[:3, 3] - ct, axis=1) <= dist_thr
    Tr = rigid_fit_batch(cs[inl][None], ct[inl][None])[0] if inl.sum() >= 3 else T
    return {'T': Tr, 'T_best': T, 'inliers': -best[0][0], 'trials': trials}


def global_registration(pair, seed=0, voxel=VOXEL):
    """The referee's own chain on a segment_pair, with its preconditions asserted: dict(fs, ft, corr, inlier_ratio, ransac result)."""
    key = ('greg', id(pair), seed, voxel)
    if key not in _CACHE:
        fkey = ('feat', id(pair), voxel)
        if fkey not in _CACHE:
            fs, ft = features(pair['src'], pair['cam_s'], voxel), features(pair['tgt'], pair['cam_t'], voxel)
            m_st, _, _ = match(fs['fpfh'], fs['valid'], ft['fpfh'], ft['valid'])
            m_ts, _, _ = match(ft['fpfh'], ft['valid'], fs['fpfh'], fs['valid'])
            corr = mutual(m_st, m_ts)
            cs, ct = fs['pos'][corr[:, 0]].astype(np.float64), ft['pos'][corr[:, 1]].astype(np.float64)
            T = pair['T']
            ratio = float((np.linalg.norm(cs @ T[:3, :3].T + T[:3, 3] - ct, axis=1) <= 1.5 * voxel).mean())
            assert ratio >= 0.03, f'referee precondition: mutual inlier ratio {ratio:.4f} < 3 %'
            _CACHE[fkey] = (fs, ft, corr, cs, ct, ratio)
        fs, ft, corr, cs, ct, ratio = _CACHE[fkey]
        r = ransac(cs, ct, 1.5 * voxel, seed)
        assert r is not None, 'referee precondition: no surviving hypothesis'
        deg, m = pose_error(r['T_best'], pair['T'])
        assert deg <= 3.0 and m <= 0.1, f'referee precondition: best hypothesis {deg:.2f} degrees, {m:.3f} m from the planted transform'
        _CACHE[key] = {'fs': fs, 'ft': ft, 'corr': corr, 'inlier_ratio': ratio, 'ransac': r, 'best_error': (deg, m)}
    return _CACHE[key]


def refine(pair, init):
    """The referee's coarse 0.3 m plain and fine 0.03 m Tukey point-to-plane ICP (lc_referee.icp, fp64) of the pair from `init`."""
    from loopy_slam_amd import loop_closure as LC
    key = ('tnrm', id(pair))
    if key not in _CACHE:
        nrm, cnt, _ = R.normals(pair['tgt'], LC.NORMAL_RADIUS, pair['cam_t'])
        _CACHE[key] = (nrm, (cnt >= 3).astype(np.uint8))
    nrm, valid = _CACHE[key]
    coarse = R.icp(pair['tgt'], nrm, valid, pair['src'], init, LC.COARSE_DIST)
    return R.icp(pair['tgt'], nrm, valid, pair['src'], coarse, LC.FINE_DIST, LC.TUKEY_K)
