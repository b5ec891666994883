"""fp64 NumPy / scipy referee of loopy_slam_amd/mesh_eval.py and csrc/lk_mesh.hip (tests/test_mesh_eval.py, tests/test_eval_recon_slam.py).
It states the rules of include/loopy_hip.h "reconstruction evaluation" a second time, in fp64, and says where a comparison in fp32 may
legitimately fall on the other side (the `undecidable` masks)."""
import numpy as np
from scipy.spatial import cKDTree

from greg_referee import philox


# ---------------------------------------------------------------------------------------------------- nearest
def nearest(target, queries):
    """(distance [P] f64, index [P]) by a k-d tree; an empty target gives (inf, -1)."""
    t, q = np.asarray(target, np.float64).reshape(-1, 3), np.asarray(queries, np.float64).reshape(-1, 3)
    if len(t) == 0:
        return np.full(len(q), np.inf), np.full(len(q), -1)
    d, i = cKDTree(t).query(q)
    return d, i


# ---------------------------------------------------------------------------------------------------- sampling
def areas(v, t):
    v = np.asarray(v, np.float64)
    return 0.5 * np.linalg.norm(np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]), axis=1)


def unit32(r):
    """u = fl(fl((float)r + 0.5) 2^-32) in fp32, one rounding per step."""
    f = r.astype(np.int64).astype(np.float32)
    return (f + np.float32(0.5)) * np.float32(2.0 ** -32)


def sample(cum, seed, S):
    """(face [S], bary [S,3] f32) of the sampler's rule on the cumulative table `cum` (fp64) and the Philox words of samples 0 .. S."""
    r = philox(seed, np.arange(S, dtype=np.uint64))
    target = ((r[:, 0].astype(np.float64) + 0.5) * 2.0 ** -32) * cum[-1]
    face = np.searchsorted(cum, target, side='right')                  # the first f with cum[f] > target
    a, b = np.sqrt(unit32(r[:, 1])), unit32(r[:, 2])
    one = np.float32(1.0)
    return face, np.stack([one - a, a * (one - b), a * b], 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- culling
def seen(points, poses, H, W, fx, fy, cx, cy, px_tol=1e-3, z_tol=1e-6):
    """(seen [N] bool, undecidable [N] bool) of the reference's projection test over all poses (camera-to-world, project convention)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    yes, maybe = np.zeros(len(p), bool), np.zeros(len(p), bool)
    for c2w in np.asarray(poses, np.float64).reshape(-1, 4, 4):
        w2c = np.linalg.inv(c2w)
        cam = p @ w2c[:3, :3].T + w2c[:3, 3]
        x, y, z = cam[:, 0], cam[:, 1], cam[:, 2]
        zz = z + 1e-5
        with np.errstate(divide='ignore', invalid='ignore'):
            u, v = (fx * -x + cx * z) / zz, (fy * y + cy * z) / zz
        inside = (0 <= -zz) & (u < W) & (u > 0) & (v < H) & (v > 0)
        clear_in = (-zz > z_tol) & (u < W - px_tol) & (u > px_tol) & (v < H - px_tol) & (v > px_tol)
        clear_out = (-zz < -z_tol) | ((np.abs(zz) > z_tol) & ((u > W + px_tol) | (u < -px_tol) | (v > H + px_tol) | (v < -px_tol)))
        yes |= inside & clear_in
        maybe |= ~(clear_in | clear_out)
    return yes, maybe & ~yes                                          # one clear sighting decides the vertex


# ---------------------------------------------------------------------------------------------------- depth
def to_camera(c2w):
    """world -> camera (x right, y down, z forward) of a project camera-to-world matrix, fp64."""
    m = np.array(c2w, np.float64).reshape(4, 4)
    m[:3, 1] *= -1.0
    m[:3, 2] *= -1.0
    return np.linalg.inv(m)


def depth(v, t, c2w, H, W, fx, fy, cx, cy, near=0.01, far=20.0, px_tol=1e-3, cos_tol=0.05, z_band=5e-4):
    """(depth [H,W] f64 with 0 = empty, undecidable [H,W] bool): one ray per pixel centre against every triangle.  A pixel is undecidable if
    its centre lies within px_tol pixels of a projected edge of a triangle that is (or, were the pixel inside it, would be) the nearest
    there, or if the plane of the nearest hit makes less than cos_tol with the ray."""
    w2c = to_camera(c2w)
    p = np.asarray(v, np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]                      # [F,3]
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(jj - cx) / fx, (ii - cy) / fy, np.ones_like(jj)], -1).reshape(-1, 3)      # [P,3]
    cones = [np.cross(b, c), np.cross(c, a), np.cross(a, b)]
    w = [d @ m.T for m in cones]                                      # [P,F]
    inside = ((w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)) | ((w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0))
    n = np.cross(b - a, c - a)
    nd = d @ n.T
    with np.errstate(divide='ignore', invalid='ignore'):
        z = np.einsum('fk,fk->f', n, a)[None, :] / nd
    ok = inside & np.isfinite(z) & (z >= near) & (z <= far)
    zhit = np.where(ok, z, np.inf)
    best = zhit.min(1)
    first = zhit.argmin(1)
    out = np.where(np.isfinite(best), best, 0.0)
    # signed distance in pixels from the pixel centre to the image line of every cone plane, positive on the triangle's side
    det = np.einsum('fk,fk->f', a, cones[0])
    sgn = np.where(det >= 0, 1.0, -1.0)
    dist = []
    for m in cones:
        A, B = m[:, 0] / fx, m[:, 1] / fy
        Cc = m[:, 2] - A * cx - B * cy
        with np.errstate(divide='ignore', invalid='ignore'):
            s = (jj.reshape(-1, 1) * A[None] + ii.reshape(-1, 1) * B[None] + Cc[None]) / np.sqrt(A * A + B * B)[None]
        dist.append(np.where(np.isfinite(s), s * sgn[None], np.inf))
    dist = np.stack(dist, -1)                                          # [P,F,3]
    nearly_in = (dist >= -px_tol).all(-1)
    on_edge = (np.abs(dist) < px_tol).any(-1)
    in_range = np.isfinite(z) & (z >= near - z_band) & (z <= far + z_band)
    would_win = z <= (best[:, None] + z_band)                          # also true where the pixel is empty (best = inf)
    und = (nearly_in & on_edge & in_range & would_win).any(1)
    cosv = np.abs(nd) / (np.linalg.norm(n, axis=1)[None] * np.linalg.norm(d, axis=1)[:, None] + 1e-300)
    hit = np.isfinite(best)
    und |= hit & (cosv[np.arange(len(d)), first] < cos_tol)
    return out.reshape(H, W), und.reshape(H, W)


# ---------------------------------------------------------------------------------------------------- metrics, alignment
def metrics(rec_points, gt_points, dist_th=0.05, f_th=0.01):
    d_rg, _ = nearest(gt_points, rec_points)
    d_gr, _ = nearest(rec_points, gt_points)
    p, r = np.mean(d_rg < f_th), np.mean(d_gr < f_th)
    return {'accuracy': d_rg.mean() * 100, 'completion': d_gr.mean() * 100, 'completion ratio': np.mean(d_gr < dist_th) * 100,
            'precision': p * 100, 'recall': r * 100, 'f-score': 2 * p * r / (p + r) * 100 if p + r > 0 else 0.0}


def kabsch(p, q):
    """4 x 4 rigid T (det = +1) taking the points p onto q in the least-squares sense (fp64)."""
    mp, mq = p.mean(0), q.mean(0)
    U, _, Vt = np.linalg.svd((p - mp).T @ (q - mq))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    T = np.eye(4)
    T[:3, :3] = Vt.T @ D @ U.T
    T[:3, 3] = mq - T[:3, :3] @ mp
    return T


def icp_point_to_point(src, tgt, threshold=0.1, max_iter=30, tol=1e-6):
    """Open3D's registration_icp with TransformationEstimationPointToPoint from the identity, replayed in fp64."""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    tree = cKDTree(tgt)
    T = np.eye(4)

    def evaluate(T):
        moved = src @ T[:3, :3].T + T[:3, 3]
        d, i = tree.query(moved, distance_upper_bound=threshold)
        hit = np.isfinite(d)
        n = int(hit.sum())
        return moved[hit], tgt[i[hit]], n / len(src), (np.sqrt(np.mean(d[hit] ** 2)) if n else 0.0)

    p, q, fit, rmse = evaluate(T)
    for _ in range(max_iter):
        if len(p) < 3:
            break
        T = kabsch(p, q) @ T
        p, q, fit_new, rmse_new = evaluate(T)
        done = abs(fit_new - fit) < tol and abs(rmse_new - rmse) < tol
        fit, rmse = fit_new, rmse_new
        if done:
            break
    return T


def motion_error(A, B):
    """(translation difference in m, rotation angle in rad) between two 4 x 4 rigid transforms."""
    R = A[:3, :3].T @ B[:3, :3]
    return float(np.linalg.norm(A[:3, 3] - B[:3, 3])), float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
