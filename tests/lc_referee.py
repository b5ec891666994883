"""NumPy referee of the loop-closure back end (tests/test_loop_closure*.py): nearest neighbours under the index's contract,
normals, point-to-plane ICP with the Tukey loss, the information matrix - the arithmetic in fp64, neighbourhoods in the precision asked for.
Nothing here is loaded by the product."""
import numpy as np

BIG = np.iinfo(np.int64).max


def so3_exp(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def planted(rot_deg, trans_m):
    T = np.eye(4)
    T[:3, :3] = so3_exp(np.deg2rad(np.asarray(rot_deg, dtype=np.float64)))
    T[:3, 3] = trans_m
    return T


def inv4(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def dist2(q, p):
    """(dx*dx + dy*dy) + dz*dz in the dtype of the operands (fp32: one rounding per operation, the contract)."""
    d = p - q
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


class Grid:
    """Uniform grid over a target cloud; candidates(q) lists, per query, every target point of the 27 cells around it."""

    def __init__(self, tgt, h):
        self.tgt = np.asarray(tgt)
        self.h = float(h)
        t64 = self.tgt.astype(np.float64)
        if len(t64) == 0:
            self.lo, self.dims = np.zeros(3), np.ones(3, dtype=np.int64)
        else:
            self.lo = t64.min(0)
            self.dims = np.floor((t64.max(0) - self.lo) / self.h).astype(np.int64) + 1
        c = np.clip(np.floor((t64 - self.lo) / self.h).astype(np.int64), 0, self.dims - 1) if len(t64) else np.zeros((0, 3), dtype=np.int64)
        key = (c[:, 2] * self.dims[1] + c[:, 1]) * self.dims[0] + c[:, 0]
        self.order = np.argsort(key, kind='stable')
        self.starts = np.searchsorted(key[self.order], np.arange(int(np.prod(self.dims)) + 1))

    def candidates(self, q):
        """(rep [M] query of each candidate, ascending; cand [M] target index; qstart [P]; qcnt [P])."""
        q64 = np.asarray(q, dtype=np.float64)
        P = len(q64)
        c = np.floor((q64 - self.lo) / self.h).astype(np.int64)
        off = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing='ij'), -1).reshape(27, 3)
        cc = c[:, None, :] + off[None]
        ok = ((cc >= 0) & (cc < self.dims)).all(-1)
        cid = np.where(ok, (cc[..., 2] * self.dims[1] + cc[..., 1]) * self.dims[0] + cc[..., 0], 0)
        s = self.starts[cid]
        cnt = np.where(ok, self.starts[cid + 1] - s, 0).ravel()
        seg = np.cumsum(cnt) - cnt
        rep27 = np.repeat(np.arange(P * 27), cnt)
        cand = self.order[s.ravel()[rep27] + (np.arange(int(cnt.sum())) - seg[rep27])]
        qcnt = cnt.reshape(P, 27).sum(1)
        return rep27 // 27, cand, np.cumsum(qcnt) - qcnt, qcnt


def _seg_two_smallest(d, idx, qstart, qcnt, P):
    """Per query segment: (index of the smallest by (d, index), its d, the second smallest d)."""
    best_i = np.full(P, -1, dtype=np.int64)
    best_d = np.full(P, np.inf, dtype=d.dtype)
    second = np.full(P, np.inf, dtype=d.dtype)
    nz = qcnt > 0
    if not nz.any() or len(d) == 0:
        return best_i, best_d, second
    st = qstart[nz]
    rep = np.repeat(np.arange(P)[nz], qcnt[nz])
    m = np.minimum.reduceat(d, st)
    best_d[nz] = m
    at_min = d == best_d[rep]
    bi = np.minimum.reduceat(np.where(at_min, idx, BIG), st)
    best_i[nz] = bi
    rest = np.where(idx == best_i[rep], np.inf, d).astype(d.dtype)
    second[nz] = np.minimum.reduceat(rest, st)
    none = ~np.isfinite(best_d)
    best_i[none] = -1
    return best_i, best_d, second


def nearest(tgt, q, max_dist, dtype=np.float32, r2=None, need_second=True):
    """Nearest target point per query with d2 <= r2 under the order (d2, index): (index or -1, d2, second-nearest d2 or inf), distances in
    `dtype`.  r2 defaults to fl32(max_dist) * fl32(max_dist), as the library squares it.  Exact: a grid pass over the 27 cells around the query
    settles every query whose nearest point is closer than one cell edge; the others go through brute force."""
    tgt = np.ascontiguousarray(tgt, dtype=dtype)
    q = np.ascontiguousarray(q, dtype=dtype)
    P = len(q)
    if r2 is None:
        r2 = np.float32(max_dist) * np.float32(max_dist)
    r2 = dtype(r2)
    out_i, out_d, out_2 = np.full(P, -1, dtype=np.int64), np.full(P, np.inf, dtype=dtype), np.full(P, np.inf, dtype=dtype)
    if len(tgt) == 0 or P == 0:
        return out_i, out_d, out_2
    h = 0.1 if max_dist > 0.0999 else max(max_dist * 1.01, 0.05)
    g = Grid(tgt, h)
    for a in range(0, P, 20000):
        qq = q[a:a + 20000]
        rep, cand, qstart, qcnt = g.candidates(qq)
        d = dist2(qq[rep], tgt[cand])
        d = np.where(d <= r2, d, dtype(np.inf)).astype(dtype)
        bi, bd, b2 = _seg_two_smallest(d, cand, qstart, qcnt, len(qq))
        # settled: the radius lies inside the 27 cells, or the two nearest both do
        lim = dtype((0.999 * h) ** 2)
        settled = np.full(len(qq), max_dist <= 0.999 * h) | ((bd < lim) & ((b2 < lim) | (not need_second)))
        todo = np.nonzero(~settled)[0]
        for b in range(0, len(todo), 512):
            rows = todo[b:b + 512]
            qb = qq[rows]
            dx = qb[:, None, 0] - tgt[None, :, 0]
            dy = qb[:, None, 1] - tgt[None, :, 1]
            dz = qb[:, None, 2] - tgt[None, :, 2]
            dd = (dx * dx + dy * dy) + dz * dz
            dd = np.where(dd <= r2, dd, dtype(np.inf)).astype(dtype)
            i1 = np.argmin(dd, axis=1)                       # first index among equal distances: the (d2, index) order
            d1 = dd[np.arange(len(rows)), i1]
            dd[np.arange(len(rows)), i1] = np.inf
            bi[rows], bd[rows], b2[rows] = np.where(np.isfinite(d1), i1, -1), d1, dd.min(axis=1)
        out_i[a:a + 20000], out_d[a:a + 20000], out_2[a:a + 20000] = bi, bd, b2
    return out_i, out_d, out_2


def normals(pos, radius, camera):
    """Per point: neighbours with contract d2 <= fl32(radius)^2 in fp32 (the point itself included), covariance and eigenvectors in fp64.
    Returns (normal [N,3] oriented to the camera, count [N], gap [N] = (l1 - l0) / l2)."""
    p32 = np.ascontiguousarray(pos, dtype=np.float32)
    p64 = p32.astype(np.float64)
    N = len(p32)
    r2 = np.float32(radius) * np.float32(radius)
    g = Grid(p32, radius * 1.01)
    nrm, cnt, gap = np.zeros((N, 3)), np.zeros(N, dtype=np.int64), np.zeros(N)
    for a in range(0, N, 10000):
        qq = p32[a:a + 10000]
        rep, cand, _, _ = g.candidates(qq)
        keep = dist2(qq[rep], p32[cand]) <= r2
        rep, cand = rep[keep], cand[keep]
        n = np.bincount(rep, minlength=len(qq)).astype(np.float64)
        d = p64[cand] - p64[a:a + 10000][rep]
        nn = np.maximum(n, 1.0)
        m = np.stack([np.bincount(rep, weights=d[:, k], minlength=len(qq)) for k in range(3)], 1) / nn[:, None]
        Cm = np.zeros((len(qq), 3, 3))
        for i in range(3):
            for j in range(i, 3):
                Cm[:, i, j] = Cm[:, j, i] = np.bincount(rep, weights=d[:, i] * d[:, j], minlength=len(qq)) / nn - m[:, i] * m[:, j]
        w, v = np.linalg.eigh(Cm)
        nv = v[:, :, 0]
        flip = (nv * (np.asarray(camera, dtype=np.float64)[None] - p64[a:a + 10000])).sum(1) < 0
        nv[flip] *= -1
        nrm[a:a + 10000], cnt[a:a + 10000] = nv, n.astype(np.int64)
        gap[a:a + 10000] = (w[:, 1] - w[:, 0]) / np.maximum(w[:, 2], 1e-300)
    return nrm, cnt, gap


def upper(A):
    return A[np.triu_indices(6)]


def p2p_sums(tgt, nrm, valid, src, T, corr, d2, tukey_k):
    """The 32 outputs of the point-to-plane mode in fp64 for given correspondences (corr [P], -1 = none; d2 their squared distances)."""
    s = np.asarray(src, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]
    use = corr >= 0
    use[use] &= np.asarray(valid)[corr[use]] != 0
    s, q, n = s[use], np.asarray(tgt, dtype=np.float64)[corr[use]], np.asarray(nrm, dtype=np.float64)[corr[use]]
    r = (n * (s - q)).sum(1)
    J = np.concatenate([np.cross(s, n), n], 1)
    w = np.ones_like(r)
    if tukey_k > 0:
        w = np.where(np.abs(r) <= tukey_k, (1 - (r / tukey_k) ** 2) ** 2, 0.0)
    out = np.zeros(32)
    out[:21] = upper((J * w[:, None]).T @ J)
    out[21:27] = (J * w[:, None]).T @ r
    out[27], out[28], out[29] = use.sum(), np.asarray(d2, dtype=np.float64)[use].sum(), (w * r * r).sum()
    return out


def info_sums(tgt, corr, d2):
    use = corr >= 0
    q = np.asarray(tgt, dtype=np.float64)[corr[use]]
    out = np.zeros(32)
    A = np.zeros((6, 6))
    z = np.zeros(len(q))
    o = np.ones(len(q))
    for row in ((z, q[:, 2], -q[:, 1], o, z, z), (-q[:, 2], z, q[:, 0], z, o, z), (q[:, 1], -q[:, 0], z, z, z, o)):
        G = np.stack(row, 1)
        A += G.T @ G
    out[:21] = upper(A)
    out[27], out[28] = use.sum(), np.asarray(d2, dtype=np.float64)[use].sum()
    return out


def icp(tgt, nrm, valid, src, init, max_dist, tukey_k=0.0, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
    """Point-to-plane ICP in fp64 (correspondences: nearest under the fp64 distance with d2 <= max_dist^2), Open3D's loop."""
    from loopy_slam_amd.loop_closure import se3_exp
    tgt64, src64 = np.asarray(tgt, dtype=np.float64), np.asarray(src, dtype=np.float64)
    T = np.array(init, dtype=np.float64)

    def evaluate(T):
        s = src64 @ T[:3, :3].T + T[:3, 3]
        ci, d2, _ = nearest(tgt64, s, max_dist, dtype=np.float64, r2=float(max_dist) ** 2, need_second=False)
        d2 = np.where(ci >= 0, d2, 0.0)
        S = p2p_sums(tgt64, nrm, valid, src64, T, ci, d2, tukey_k)
        A = np.zeros((6, 6))
        A[np.triu_indices(6)] = S[:21]
        A = A + np.triu(A, 1).T
        cnt = S[27]
        return A, S[21:27], cnt / len(src64), (np.sqrt(S[28] / cnt) if cnt else 0.0), cnt

    A, b, fit, rmse, cnt = evaluate(T)
    for _ in range(max_iter):
        if cnt < 6:
            break
        T = se3_exp(np.linalg.solve(A, -b)) @ T
        A, b, fn, rn, cnt = evaluate(T)
        done = abs(fn - fit) < rel_fitness and abs(rn - rmse) < rel_rmse
        fit, rmse = fn, rn
        if done:
            break
    return T


def clouds(n_each=30000, seed=5):
    """(source [n,3], target [n,3]) fp32: rows [0, n) and [2n/3, 5n/3) of a fixed permutation of synthetic.build_cloud(2n, seed):
    one third shared points, the rest different samples of the same surfaces."""
    from loopy_slam_amd import synthetic
    return synthetic.overlapping_pair(n_each, seed)


def move(pts, T):
    """fp32 points moved by the 4 x 4 T (in fp64, rounded once)."""
    return np.ascontiguousarray((np.asarray(pts, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32))


DRIFTS = (((0.6, -0.5, 0.7), (0.02, -0.015, 0.01)), ((1.5, -1.0, 2.0), (0.05, -0.04, 0.03)))
CAMERA = (0.0, 0.0, 0.0)
