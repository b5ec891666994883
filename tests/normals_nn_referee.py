"""NumPy referee of lk_normals_nn (tests/test_normals_nn.py, tests/test_segment_tsdf.py): the selection - the max_nn smallest of the
candidates with contract distance d2 <= fl32(radius)^2 under the order (d2, index), the distance in fp32 with one rounding per operation -
and, over that selection, covariance and eigenvectors in fp64.  Extends tests/lc_referee.py; nothing here is loaded by the product."""
import numpy as np

import lc_referee as R


def _keys(d2, idx):
    """(d2, index) as one uint64: d2 >= +0, so the unsigned order of its bits is its order."""
    return (np.ascontiguousarray(d2, dtype=np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)


def select_brute(pos, radius, max_nn, queries=None):
    """(count [Q], nbr [Q,max_nn] padded with -1) against EVERY point of the cloud: no grid, for small inputs."""
    p = np.ascontiguousarray(pos, dtype=np.float32)
    q_idx = np.arange(len(p)) if queries is None else np.asarray(queries)
    r2 = np.float32(radius) * np.float32(radius)
    count, nbr = np.zeros(len(q_idx), dtype=np.int64), np.full((len(q_idx), max_nn), -1, dtype=np.int64)
    all_idx = np.arange(len(p))
    for a, i in enumerate(q_idx):
        d = p - p[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inside = d2 <= r2
        order = np.argsort(_keys(d2[inside], all_idx[inside]), kind='stable')[:max_nn]
        count[a] = len(order)
        nbr[a, :len(order)] = all_idx[inside][order]
    return count, nbr


def select(pos, radius, max_nn, queries=None, chunk=4000):
    """The same through lc_referee.Grid (cells of 1.01 radius: the 27 cells around a query hold every point within the radius), with
    n_in_radius [Q] besides: (count, nbr, n_in_radius)."""
    p = np.ascontiguousarray(pos, dtype=np.float32)
    q_idx = np.arange(len(p)) if queries is None else np.asarray(queries)
    r2 = np.float32(radius) * np.float32(radius)
    g = R.Grid(p, radius * 1.01)
    Q = len(q_idx)
    count, nbr, n_in = np.zeros(Q, dtype=np.int64), np.full((Q, max_nn), -1, dtype=np.int64), np.zeros(Q, dtype=np.int64)
    for a in range(0, Q, chunk):
        qi = q_idx[a:a + chunk]
        rep, cand, _, _ = g.candidates(p[qi])
        d2 = R.dist2(p[qi][rep], p[cand])
        keep = d2 <= r2
        rep, cand, d2 = rep[keep], cand[keep], d2[keep]
        order = np.lexsort((_keys(d2, cand), rep))
        rep, cand = rep[order], cand[order]
        n = np.bincount(rep, minlength=len(qi))
        rank = np.arange(len(rep)) - (np.cumsum(n) - n)[rep]
        take = rank < max_nn
        nbr[a + rep[take], rank[take]] = cand[take]
        n_in[a:a + chunk] = n
        count[a:a + chunk] = np.minimum(n, max_nn)
    return count, nbr, n_in


def normals(pos, nbr, count, camera, queries=None):
    """fp64 normals over a given selection: (normal [Q,3] oriented to the camera - zero where count < 1 -, gap [Q] = (l1 - l0) / l2)."""
    p64 = np.ascontiguousarray(pos, dtype=np.float32).astype(np.float64)
    q_idx = np.arange(len(p64)) if queries is None else np.asarray(queries)
    Q, k = nbr.shape
    nrm, gap = np.zeros((Q, 3)), np.zeros(Q)
    for a in range(0, Q, 20000):
        nb, q = nbr[a:a + 20000], p64[q_idx[a:a + 20000]]
        w = (nb >= 0).astype(np.float64)
        d = (p64[np.maximum(nb, 0)] - q[:, None, :]) * w[:, :, None]
        n = np.maximum(count[a:a + 20000].astype(np.float64), 1.0)
        m = d.sum(1) / n[:, None]
        Cm = np.einsum('qki,qkj->qij', d, d) / n[:, None, None] - m[:, :, None] * m[:, None, :]
        ev, v = np.linalg.eigh(Cm)
        nv = v[:, :, 0].copy()
        flip = (nv * (np.asarray(camera, dtype=np.float64)[None] - q)).sum(1) < 0
        nv[flip] *= -1
        nrm[a:a + 20000] = nv
        gap[a:a + 20000] = (ev[:, 1] - ev[:, 0]) / np.maximum(ev[:, 2], 1e-300)
    return nrm, gap


def angle(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.clip((a * b).sum(1), -1.0, 1.0))
