"""Loop closure, geometric back end: register map segments, optimise the segment pose graph, move the map.

Reference                                                  here
  src/common.py  pairwise_registration (Open3D ICP)        register_pair -> icp -> lk_icp_accumulate (device sums, 6 x 6 solve on the host)
  src/common.py  estimate_normals / orient_normals         estimate_normals -> lk_normals, or lk_normals_nn (the max_nn nearest: Open3D's hybrid search)
  get_information_matrix_from_point_clouds                 information_matrix -> lk_icp_accumulate (LK_ICP_INFORMATION)
  src/common.py  register_point_cloud_pair                 register_pair's success rule
  o3d global_optimization (Levenberg-Marquardt)            optimize_pose_graph (host, fp64)
  src/neural_point.py  apply_correction / apply_transformation   LoopCloser.apply -> lk_apply_correction + lk_knn_build

  src/common.py  preprocess_point_cloud (voxel, FPFH)       fpfh_features -> lk_voxel_downsample, lk_normals, lk_fpfh
  src/common.py  execute_global_registration (RANSAC)      global_registration -> lk_feature_match, lk_ransac_hypotheses, lk_ransac_score

  src/neural_point.py  ORB + DBoW query, compute_dbow_score  LoopCloser.appearance_candidates / on_mapped_frame -> place.PlaceRecognizer

  src/neural_point.py  compute_tsdf (per-segment clouds)     LoopCloser.fuse_closed_segments -> tsdf.fuse_segment, extract_point_cloud; lk_rigid_map

Which pairs are registered is `loop_closure.candidates`: 'pose' (the tracked keyframe poses), 'appearance' (place recognition: the
library's own binary descriptor and matching score, place.py - not OpenCV's ORB, not a DBoW vocabulary) or a callable.  The
methods 'icp' and 'robust_icp' start from the tracked poses (the identity between two segments of one world frame: the reference's
method == "icp" branch, plus the Tukey fine stage of its "robust_icp" branch); 'fpfh_robust_icp' puts the reference's global start in
front of them - voxel downsample, FPFH, mutual feature matches, 3-point RANSAC, all on the device - and survives a loop that has really
drifted.  The error plots are out.  What is registered is `loop_closure.cloud`: 'neural' (default) = the segments' NEURAL points (on the
device, thinned by the insertion radius), normals over every point within 0.1 m; 'tsdf' = what the reference registers - the sensor frames of
every closed segment fused into a TSDF volume at the tracked poses, the mesh vertices kept per segment and moved with the map, normals over the
50 nearest within 0.1 m; the pose graph then has one node per CLOSED segment.  Of the reference's edge filters only the
`old_trans_mag_filter` branch (its default) is built.  Feature rows are not touched (rotation-agnostic in the reference too).
"""
import ctypes as C

import numpy as np
import torch

from . import _ffi, core, place
from ._ffi import ptr

COARSE_DIST, FINE_DIST, TUKEY_K, NORMAL_RADIUS = 0.3, 0.03, 0.01, 0.1      # src/common.py:594-595, 607, 647
METHODS = ('identity', 'icp', 'robust_icp', 'fpfh_robust_icp')
# the global start (src/common.py preprocess_point_cloud / execute_global_registration): voxel, normals over 2 voxels, features over 5,
# checkers at 0.9 and 1.5 voxels, confidence and trial cap of the reference
VOXEL, EDGE_RATIO, GLOBAL_CONF, GLOBAL_ITER, RANSAC_BATCH = 0.04, 0.9, 0.99999, 10_000_000, 65536
MIN_SCORE = 0.223


# ------------------------------------------------------------------------------------------------ SE(3), fp64, vectors (omega, v)
def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(x):
    x = np.asarray(x, dtype=np.float64)
    w, v = x[:3], x[3:]
    th = float(np.linalg.norm(w))
    K = _hat(w)
    if th < 1e-6:
        a, b, c = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        a, b, c = np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * K + b * K @ K
    T[:3, 3] = (np.eye(3) + b * K + c * K @ K) @ v
    return T


def se3_log(T):
    T = np.asarray(T, dtype=np.float64)
    R, t = T[:3, :3], T[:3, 3]
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])       # sin(th) * axis
    s, c = float(np.linalg.norm(a)), 0.5 * (np.trace(R) - 1.0)
    th = float(np.arctan2(s, c))
    w = a * (th / s) if s > 1e-9 else a
    K = _hat(w)
    if th < 1e-6:
        k = 1.0 / 12.0
    else:
        k = (1.0 - th * np.sin(th) / (2.0 * (1.0 - np.cos(th)))) / th ** 2
    v = (np.eye(3) - 0.5 * K + k * K @ K) @ t
    return np.concatenate([w, v])


def _adjoint(T):
    R, t = T[:3, :3], T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = _hat(t) @ R
    return A


def _inv(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


# ------------------------------------------------------------------------------------------------ device layer
def _sync(eng):
    if eng.device.type == 'cuda':
        torch.cuda.current_stream(eng.device).synchronize()


class SegmentCloud:
    """The points of one segment on the device with what a registration needs of them: one grid index and the normals.

    One index with NORMAL_RADIUS cells serves all three searches: the normals' radius equals the cell edge (3 x 3 rows of cells), the
    0.3-m coarse search is the index's two-phase search (the box of one cell edge first, the full box only for a point with no
    neighbour that near), the 0.03-m fine search touches at most 2 x 2 rows."""

    def __init__(self, eng, pos, camera, cell=NORMAL_RADIUS, max_nn=None, fpfh_max_nn=None):
        """max_nn: the normals take the max_nn nearest neighbours within NORMAL_RADIUS (lk_normals_nn; the reference's 50 on a fused
        surface cloud) instead of all of them (lk_normals); fpfh_max_nn: the same for the normals of the FPFH preprocessing (its 30)."""
        self.eng = eng
        self.pos = pos.detach().to(eng.device, torch.float32).contiguous()
        self.camera = np.asarray(torch.as_tensor(camera).detach().cpu().numpy(), dtype=np.float64).reshape(-1)[:3]
        self.cell = float(cell)
        self.max_nn, self.fpfh_max_nn = max_nn, fpfh_max_nn
        self._knn = self._normals = None
        self._features = {}

    def features(self, voxel=VOXEL):
        """fpfh_features of this cloud, computed once per voxel size."""
        if voxel not in self._features:
            self._features[voxel] = fpfh_features(self.eng, self.pos, self.camera, voxel, max_nn=self.fpfh_max_nn)
        return self._features[voxel]

    def __len__(self):
        return int(self.pos.shape[0])

    @property
    def knn(self):
        if self._knn is None:
            self._knn = core.KnnIndex(self.eng, capacity=max(len(self), 1), cell_size=self.cell)
            self._knn.build(self.pos)
        return self._knn

    @property
    def normals(self):
        if self._normals is None:
            self._normals = estimate_normals(self.eng, self.pos, NORMAL_RADIUS, self.camera, knn=self.knn, max_nn=self.max_nn)
        return self._normals

    def close(self):
        if self._knn is not None:
            self._knn.close()
            self._knn = None


def estimate_normals(eng, pos, radius=NORMAL_RADIUS, camera=(0.0, 0.0, 0.0), knn=None, max_nn=None):
    """(normals [N,3] f32, valid [N] uint8) of the cloud pos; knn: an index already built over pos.  max_nn None: every point within the
    radius (lk_normals); a number: the max_nn nearest of them under (d2, index) (lk_normals_nn, Open3D's hybrid search)."""
    pos = pos.contiguous()
    N = int(pos.shape[0])
    own = knn is None
    if own:
        knn = core.KnnIndex(eng, capacity=max(N, 1), cell_size=radius)
        knn.build(pos)
    normals, valid = eng.zeros(N, 3), eng.zeros(N, dtype=torch.uint8)
    cam = (C.c_float * 3)(*[float(c) for c in np.asarray(camera, dtype=np.float64).reshape(-1)[:3]])
    if max_nn is None:
        eng.lib.check(eng.lib.dll.lk_normals(knn.h, ptr(pos), N, C.c_float(radius), cam, ptr(normals), ptr(valid), eng.stream), 'lk_normals')
    else:
        eng.lib.check(eng.lib.dll.lk_normals_nn(knn.h, ptr(pos), N, C.c_float(radius), int(max_nn), cam, ptr(normals), ptr(valid), None, None,
                                                eng.stream), 'lk_normals_nn')
    if own:
        _sync(eng)
        knn.close()
    return normals, valid


def normals_nn(eng, pos, knn, radius=NORMAL_RADIUS, max_nn=50, camera=(0.0, 0.0, 0.0), want_selection=True):
    """lk_normals_nn with its selection: (normals [N,3] f32, valid [N] uint8, count [N] int32, nbr [N,max_nn] int32) - the last two None
    without want_selection.  knn: the index built over pos."""
    pos = pos.contiguous()
    N = int(pos.shape[0])
    normals, valid = eng.zeros(N, 3), eng.zeros(N, dtype=torch.uint8)
    count = eng.empty(N, dtype=torch.int32) if want_selection else None
    nbr = eng.empty(N, max(int(max_nn), 1), dtype=torch.int32) if want_selection else None
    cam = (C.c_float * 3)(*[float(c) for c in np.asarray(camera, dtype=np.float64).reshape(-1)[:3]])
    eng.lib.check(eng.lib.dll.lk_normals_nn(knn.h, ptr(pos), N, C.c_float(radius), int(max_nn), cam, ptr(normals), ptr(valid), ptr(count),
                                            ptr(nbr), eng.stream), 'lk_normals_nn')
    return normals, valid, count, nbr


def rigid_map(eng, pos, T):
    """pos [n,3] (contiguous, on the device) <- R pos + t in place, T 4 x 4 rounded to fp32 (lk_rigid_map; the identity keeps the bits)."""
    M12 = (C.c_float * 12)(*np.asarray(T, dtype=np.float64)[:3, :4].astype(np.float32).ravel().tolist())
    eng.lib.check(eng.lib.dll.lk_rigid_map(ptr(pos), int(pos.shape[0]), M12, eng.stream), 'lk_rigid_map')


def icp_sums(eng, tgt, src_pos, T, max_dist, tukey_k=0.0, mode=_ffi.ICP_POINT_TO_PLANE, want_corr=False):
    """One lk_icp_accumulate call: (sums float64 [32] on the host, correspondence index [P] int32 on the device or None).
    tgt: SegmentCloud; T: 4 x 4 (rounded to fp32 for the device)."""
    src_pos = src_pos.contiguous()
    P = int(src_pos.shape[0])
    T12 = (C.c_float * 12)(*np.asarray(T, dtype=np.float64)[:3, :4].astype(np.float32).ravel().tolist())
    n_scr = int(eng.lib.dll.lk_icp_scratch_floats(P))
    scratch = eng.empty(max(n_scr, 1))
    out = eng.zeros(_ffi.ICP_SUMS, dtype=torch.float64)
    corr = eng.empty(P, dtype=torch.int32) if want_corr else None
    p2p = mode == _ffi.ICP_POINT_TO_PLANE
    nrm, val = tgt.normals if p2p else (None, None)
    eng.lib.check(eng.lib.dll.lk_icp_accumulate(tgt.knn.h, ptr(tgt.pos), ptr(nrm), ptr(val), ptr(src_pos), P, T12, C.c_float(max_dist),
                                                C.c_float(tukey_k), int(mode), ptr(corr), ptr(scratch), n_scr, ptr(out), eng.stream),
                  'lk_icp_accumulate')
    return out.cpu().numpy(), corr           # the copy is the one synchronisation of an iteration


def unpack_sums(s):
    """(A 6 x 6 symmetric, b [6], count, sum_d2, sum_w_r2) of a row of lk_icp_accumulate sums."""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[:21]
    A = A + np.triu(A, 1).T
    return A, np.array(s[21:27]), float(s[27]), float(s[28]), float(s[29])


def icp(eng, src, tgt, init=None, max_dist=FINE_DIST, tukey_k=0.0, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
    """Point-to-plane ICP of src onto tgt (SegmentClouds) from the 4 x 4 `init`: Gauss-Newton, sums on the device, the 6 x 6 solve
    in fp64 here, T <- exp(x) T; Open3D's default convergence criteria (the change of fitness and of inlier rmse both below 1e-6, or 30
    iterations).  Returns dict(T, fitness = count / P, inlier_rmse = sqrt(sum d2 / count), iterations).  count is the number of
    correspondences that enter the sums: those within max_dist whose target normal is valid."""
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    P = max(len(src), 1)

    def evaluate(T):
        s, _ = icp_sums(eng, tgt, src.pos, T, max_dist, tukey_k)
        A, b, cnt, sd2, _ = unpack_sums(s)
        return A, b, cnt / P, (np.sqrt(sd2 / cnt) if cnt > 0 else 0.0), cnt

    A, b, fit, rmse, cnt = evaluate(T)
    it = 0
    for it in range(1, max_iter + 1):
        if cnt < 6:
            break
        try:
            x = np.linalg.solve(A, -b)
        except np.linalg.LinAlgError:
            break
        T = se3_exp(x) @ T
        A, b, fit_new, rmse_new, cnt = evaluate(T)
        done = abs(fit_new - fit) < rel_fitness and abs(rmse_new - rmse) < rel_rmse
        fit, rmse = fit_new, rmse_new
        if done:
            break
    return {'T': T, 'fitness': fit, 'inlier_rmse': rmse, 'iterations': it}


def information_matrix(eng, src, tgt, T, max_dist=FINE_DIST):
    """sum G^T G over the correspondences within max_dist at T, G = [-[q]x | I] (Open3D's get_information_matrix_from_point_clouds):
    (6 x 6, count, sum d2)."""
    s, _ = icp_sums(eng, tgt, src.pos, T, max_dist, mode=_ffi.ICP_INFORMATION)
    A, _, cnt, sd2, _ = unpack_sums(s)
    return A, cnt, sd2


# ------------------------------------------------------------------------------------------------ global start: FPFH + RANSAC
def _compact(eng, mask):
    """Indices of the non-zero entries of a uint8 mask, ascending (lk_compact_large): (index [n] int32 with the first `count` filled,
    count [1] int32, both on the device)."""
    n = int(mask.shape[0])
    index, count = eng.empty(max(n, 1), dtype=torch.int32), eng.zeros(1, dtype=torch.int32)
    scratch = eng.empty(max((n + 255) // 256, 1), dtype=torch.int32)
    eng.lib.check(eng.lib.dll.lk_compact_large(ptr(mask), n, ptr(index), ptr(count), ptr(scratch), eng.stream), 'lk_compact_large')
    return index, count


def voxel_downsample(eng, pos, voxel=VOXEL):
    """One centroid per occupied voxel of edge `voxel`, in ascending voxel-key order (lk_voxel_keys -> sort -> lk_voxel_downsample); the
    voxel grid starts half a voxel below the cloud's minimum, as Open3D's does."""
    pos = pos.contiguous()
    N = int(pos.shape[0])
    if N == 0:
        return eng.zeros(0, 3)
    dll = eng.lib.dll
    origin = pos.min(0).values.cpu().numpy().astype(np.float32) - np.float32(0.5) * np.float32(voxel)
    keys = eng.empty(N, dtype=torch.int64)
    eng.lib.check(dll.lk_voxel_keys(ptr(pos), N, (C.c_float * 3)(*origin.tolist()), C.c_float(voxel), ptr(keys), eng.stream), 'lk_voxel_keys')
    skeys, order = torch.sort(keys, stable=True)
    head = eng.empty(N, dtype=torch.uint8)
    eng.lib.check(dll.lk_voxel_heads(ptr(skeys), N, ptr(head), eng.stream), 'lk_voxel_heads')
    starts, count = _compact(eng, head)
    n_vox = int(count.cpu()[0])
    out = eng.empty(n_vox, 3)
    order = order.contiguous()
    eng.lib.check(dll.lk_voxel_downsample(ptr(pos), N, ptr(order), ptr(starts), n_vox, ptr(out), eng.stream), 'lk_voxel_downsample')
    _sync(eng)
    return out


def _canonical_index(eng, pos, cell):
    knn = core.KnnIndex(eng, capacity=max(int(pos.shape[0]), 1), cell_size=cell)
    knn.build(pos)
    eng.lib.check(eng.lib.dll.lk_knn_canonicalize(knn.h, eng.stream), 'lk_knn_canonicalize')
    return knn


def fpfh(eng, pos, normals, valid, radius):
    """(spfh [N,33], fpfh [N,33]) of a cloud with normals (lk_fpfh) over an index of `radius` cells in canonical order."""
    pos = pos.contiguous()
    N = int(pos.shape[0])
    spfh, out = eng.zeros(N, _ffi.FPFH_DIM), eng.zeros(N, _ffi.FPFH_DIM)
    knn = _canonical_index(eng, pos, radius)
    try:
        eng.lib.check(eng.lib.dll.lk_fpfh(knn.h, ptr(pos), ptr(normals), ptr(valid), N, C.c_float(radius), ptr(spfh), ptr(out), eng.stream),
                      'lk_fpfh')
        _sync(eng)
    finally:
        knn.close()
    return spfh, out


def fpfh_features(eng, pos, camera, voxel=VOXEL, max_nn=None):
    """preprocess_point_cloud: downsample to `voxel`, normals over 2 voxels (towards `camera`; max_nn: over the nearest max_nn of them, the
    reference's 30), FPFH over 5 voxels.  Returns dict(pos, normals, valid, spfh, fpfh) on the device."""
    down = voxel_downsample(eng, pos, voxel)
    knn = _canonical_index(eng, down, 2.0 * voxel)
    try:
        normals, valid = estimate_normals(eng, down, 2.0 * voxel, camera, knn=knn, max_nn=max_nn)
        _sync(eng)
    finally:
        knn.close()
    spfh, feat = fpfh(eng, down, normals, valid, 5.0 * voxel)
    return {'pos': down, 'normals': normals, 'valid': valid, 'spfh': spfh, 'fpfh': feat}


def feature_match(eng, A, valid_a, B, valid_b):
    """(index [Na] int32, d2 [Na]) of the nearest row of B for every row of A under (d2, index); -1 where there is none (lk_feature_match)."""
    Na, Nb = int(A.shape[0]), int(B.shape[0])
    idx, d2 = eng.empty(Na, dtype=torch.int32), eng.empty(Na)
    eng.lib.check(eng.lib.dll.lk_feature_match(ptr(A), ptr(valid_a), Na, ptr(B), ptr(valid_b), Nb, ptr(idx), ptr(d2), eng.stream),
                  'lk_feature_match')
    return idx, d2


def mutual_matches(eng, fs, ft):
    """Correspondences [M,2] int32 (source row, target row) in source order: the pairs that choose each other, or - fewer than three of
    those - every source row's own choice."""
    m_st, _ = feature_match(eng, fs['fpfh'], fs['valid'], ft['fpfh'], ft['valid'])
    m_ts, _ = feature_match(eng, ft['fpfh'], ft['valid'], fs['fpfh'], fs['valid'])
    Ns = int(m_st.shape[0])
    if Ns == 0 or int(m_ts.shape[0]) == 0:
        return torch.zeros(0, 2, dtype=torch.int32, device=eng.device)
    has = m_st >= 0
    back = m_ts[m_st.clamp(min=0).long()]
    mutual = (has & (back == torch.arange(Ns, dtype=torch.int32, device=eng.device))).to(torch.uint8)
    rows, count = _compact(eng, mutual)
    n = int(count.cpu()[0])
    if n < 3:
        rows, count = _compact(eng, has.to(torch.uint8))
        n = int(count.cpu()[0])
    rows = rows[:n]
    return torch.stack([rows, m_st[rows.long()]], 1).contiguous()


def ransac_batch(eng, cs, ct, seed, trial0, n_trials, dist_thr, edge_ratio=EDGE_RATIO, want_triples=False):
    """One batch of trials (lk_ransac_hypotheses -> lk_compact_large -> lk_ransac_score): dict(triples or None, ok [n] uint8, T [n,12],
    survivors [n] int32, n_survivors [1] int32, count [n] int32, sum_d2 [n]) on the device; the last two hold one entry per survivor."""
    dll, M = eng.lib.dll, int(cs.shape[0])
    triples = eng.empty(n_trials, 3, dtype=torch.int32) if want_triples else None
    ok, T = eng.empty(n_trials, dtype=torch.uint8), eng.empty(n_trials, 12)
    eng.lib.check(dll.lk_ransac_hypotheses(ptr(cs), ptr(ct), M, int(seed), int(trial0), n_trials, C.c_float(edge_ratio), C.c_float(dist_thr),
                                           ptr(triples), ptr(ok), ptr(T), eng.stream), 'lk_ransac_hypotheses')
    surv, n_surv = _compact(eng, ok)
    count, sum_d2 = eng.zeros(n_trials, dtype=torch.int32), eng.zeros(n_trials)
    eng.lib.check(dll.lk_ransac_score(ptr(cs), ptr(ct), M, ptr(T), ptr(surv), ptr(n_surv), n_trials, C.c_float(dist_thr), ptr(count),
                                      ptr(sum_d2), eng.stream), 'lk_ransac_score')
    return {'triples': triples, 'ok': ok, 'T': T, 'survivors': surv, 'n_survivors': n_surv, 'count': count, 'sum_d2': sum_d2}


def ransac_gather(eng, src_pos, tgt_pos, corr):
    """(cs [M,3], ct [M,3]): the source and target points of the correspondences corr [M,2] (lk_ransac_gather)."""
    M = int(corr.shape[0])
    cs, ct = eng.empty(M, 3), eng.empty(M, 3)
    eng.lib.check(eng.lib.dll.lk_ransac_gather(ptr(src_pos), ptr(tgt_pos), ptr(corr), M, ptr(cs), ptr(ct), eng.stream), 'lk_ransac_gather')
    return cs, ct


def ransac_best_init(eng):
    """The device record lk_ransac_best folds into, before the first batch: best[0] = -1 (none yet), the rest 0."""
    best = eng.zeros(_ffi.RANSAC_BEST, dtype=torch.int32)
    best[0] = -1
    return best


def ransac_fold(eng, r, trial0, best):
    """Fold the ransac_batch result r, whose first trial is trial0, into the record `best` (lk_ransac_best)."""
    eng.lib.check(eng.lib.dll.lk_ransac_best(ptr(r['count']), ptr(r['sum_d2']), ptr(r['survivors']), ptr(r['n_survivors']), ptr(r['T']),
                                             int(trial0), ptr(best), eng.stream), 'lk_ransac_best')


def rigid_fit(a, b):
    """Least-squares rotation and translation (no scale, det = +1) taking the points a [n,3] onto b [n,3], fp64: 4 x 4."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ma, mb = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((b - mb).T @ (a - ma))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    T = np.eye(4)
    T[:3, :3] = U @ D @ Vt
    T[:3, 3] = mb - T[:3, :3] @ ma
    return T


def ransac(eng, src_pos, tgt_pos, corr, dist_thr, conf=GLOBAL_CONF, max_iter=GLOBAL_ITER, seed=0, batch=RANSAC_BATCH):
    """RANSAC over the correspondences corr [M,2] in batches of `batch` trials, the best hypothesis (inlier count over the correspondence
    set, then sum d2, then trial) read back after each; stops after k = log(1 - conf) / log(1 - ratio^3) trials, ratio = best count / M
    (Open3D's rule), or max_iter.  The best hypothesis is then re-fitted over all its inlier correspondences here in fp64.
    Returns dict(T, T_best, inliers, n_corr, trials, survivors, global_ok)."""
    M = int(corr.shape[0])
    out = {'T': np.eye(4), 'T_best': np.eye(4), 'inliers': 0, 'n_corr': M, 'trials': 0, 'survivors': 0, 'global_ok': False}
    if M < 3:
        return out
    cs, ct = ransac_gather(eng, src_pos, tgt_pos, corr)
    best = ransac_best_init(eng)
    trials, k_stop, b = 0, float(max_iter), None
    while trials < min(k_stop, max_iter):
        n = int(min(batch, max_iter - trials))
        r = ransac_batch(eng, cs, ct, seed, trials, n, dist_thr)
        ransac_fold(eng, r, trials, best)
        trials += n
        b = best.cpu().numpy()               # the one synchronisation of a batch
        if b[0] > 0:
            ratio3 = min(float(b[0]) / M, 1.0) ** 3
            k_stop = 0.0 if ratio3 >= 1.0 else np.log(1.0 - conf) / np.log(1.0 - ratio3)
    out.update(trials=trials, survivors=int(b[16]))
    if b[0] < 0:
        return out
    T = np.eye(4)
    T[:3, :4] = b[4:16].view(np.float32).astype(np.float64).reshape(3, 4)
    s64, t64 = cs.cpu().numpy().astype(np.float64), ct.cpu().numpy().astype(np.float64)
    inl = (((s64 @ T[:3, :3].T + T[:3, 3]) - t64) ** 2).sum(1) <= float(dist_thr) ** 2
    out.update(T_best=T, T=rigid_fit(s64[inl], t64[inl]) if inl.sum() >= 3 else T, inliers=int(b[0]), global_ok=True)
    return out


def global_registration(eng, seg_s, seg_t, voxel=VOXEL, conf=GLOBAL_CONF, max_iter=GLOBAL_ITER, seed=0):
    """execute_global_registration for two SegmentClouds: FPFH features of both (cached on the clouds), mutual nearest feature matches,
    RANSAC with the edge-length checker at 0.9 and the distance checker at 1.5 voxels.  Returns ransac()'s dict: T moves seg_s onto seg_t;
    fewer than 3 correspondences or no surviving hypothesis: the identity and global_ok = False."""
    fs, ft = seg_s.features(voxel), seg_t.features(voxel)
    corr = mutual_matches(eng, fs, ft)
    return ransac(eng, fs['pos'], ft['pos'], corr, 1.5 * voxel, conf, max_iter, seed)


def register_pair(seg_s, seg_t, method='robust_icp', adjacent=False, eng=None, global_cfg=None):
    """src/common.py pairwise_registration + register_point_cloud_pair for two SegmentClouds, starting from the identity.
    'identity': the odometry edge of adjacent segments; 'icp': coarse 0.3 m then fine 0.03 m; 'robust_icp': coarse 0.3 m plain, then
    fine 0.03 m with the Tukey loss k = 0.01; 'fpfh_robust_icp': the same two stages started from global_registration's transform
    (global_cfg: its conf / max_iter / seed; without a global result exactly 'robust_icp').  A non-adjacent pair whose transform stays the identity or whose overlap
    information[5,5] / n_points is below 0.3 fails: identity transform, identity information."""
    if method not in METHODS:
        raise NotImplementedError(f'loop_closure.method {method!r}: one of {METHODS}')
    eng = eng if eng is not None else seg_s.eng
    out = {'fitness': 0.0, 'inlier_rmse': 0.0, 'iterations': 0}
    if method == 'identity':
        T = np.eye(4)
    else:
        init = np.eye(4)
        if method == 'fpfh_robust_icp':
            g = global_registration(eng, seg_s, seg_t, **(global_cfg or {}))
            init = g['T'] if g['global_ok'] else init
            out.update(T_global=init, global_inliers=g['inliers'], global_trials=g['trials'], global_ok=g['global_ok'])
        coarse = icp(eng, seg_s, seg_t, init, COARSE_DIST)
        fine = icp(eng, seg_s, seg_t, coarse['T'], FINE_DIST, TUKEY_K if method != 'icp' else 0.0)
        T = fine['T']
        out.update(fitness=fine['fitness'], inlier_rmse=fine['inlier_rmse'], iterations=coarse['iterations'] + fine['iterations'],
                   T_coarse=coarse['T'])
    info, cnt, sd2 = information_matrix(eng, seg_s, seg_t, T, FINE_DIST)
    n_points = max(min(len(seg_s), len(seg_t)), 1)
    out.update(T=T, information=info, n_points=n_points, overlap=info[5, 5] / n_points, success=True,
               transl_mag=float(np.abs(T[:3, 3]).mean()))
    if method == 'identity':
        out.update(fitness=cnt / max(len(seg_s), 1), inlier_rmse=float(np.sqrt(sd2 / cnt)) if cnt > 0 else 0.0)
    if not adjacent and (np.trace(T) == 4.0 or out['overlap'] < 0.3):
        out.update(success=False, T=np.eye(4), information=np.eye(6))
    return out


# ------------------------------------------------------------------------------------------------ pose graph (host, fp64)
def line_process_mu(edges, lc_pref, max_dist):
    """The line-process scale of Open3D's global_optimization: lc_pref x max_dist^2 x (mean over the edges of information[5,5],
    the number of correspondences) - the energy e^T Lambda e of an edge all of whose correspondences are sqrt(lc_pref) x max_dist off."""
    if not edges:
        return 0.0
    return float(lc_pref) * float(max_dist) ** 2 * float(np.mean([np.asarray(e[3])[5, 5] for e in edges]))


def _lm(n_nodes, edges, X, mu, max_iter=100):
    """Levenberg-Marquardt over X_1 .. X_{n-1} (left perturbations X <- exp(d) X, node 0 fixed) of
    sum_certain x + sum_uncertain mu x / (mu + x), x = e^T Lambda e, e = log(T_st^-1 X_t^-1 X_s): the Geman-McClure form that
    Choi et al.'s line process l = (mu / (mu + x))^2 minimises to; l is also the weight of the edge's Gauss-Newton terms."""
    def residuals(X):
        out = []
        for s, t, T, L, unc in edges:
            A = _inv(T) @ _inv(X[t])
            e = se3_log(A @ X[s])
            out.append((A, e, float(e @ L @ e)))
        return out

    def cost(res):
        return sum((mu * x / (mu + x) if (unc and mu > 0) else x) for (_, _, x), (_, _, _, _, unc) in zip(res, edges))

    def weights(res):
        return [((mu / (mu + x)) ** 2 if (unc and mu > 0) else 1.0) for (_, _, x), (_, _, _, _, unc) in zip(res, edges)]

    res = residuals(X)
    c, lam = cost(res), 1e-6
    nv = 6 * (n_nodes - 1)
    for _ in range(max_iter):
        if nv == 0:
            break
        H, g = np.zeros((nv, nv)), np.zeros(nv)
        for (A, e, x), (s, t, T, L, unc), l in zip(res, edges, weights(res)):
            w, v = e[:3], e[3:]
            ad = np.zeros((6, 6))
            ad[:3, :3] = _hat(w); ad[3:, 3:] = _hat(w); ad[3:, :3] = _hat(v)
            J = (np.eye(6) - 0.5 * ad + ad @ ad / 12.0) @ _adjoint(A)        # d e / d (delta_s - delta_t), left Jacobian inverse to 2nd order
            for (a, sa) in ((s, 1.0), (t, -1.0)):
                if a == 0:
                    continue
                ia = slice(6 * (a - 1), 6 * a)
                g[ia] += l * sa * (J.T @ L @ e)
                for (b, sb) in ((s, 1.0), (t, -1.0)):
                    if b == 0:
                        continue
                    H[ia, slice(6 * (b - 1), 6 * b)] += l * sa * sb * (J.T @ L @ J)
        step_ok = False
        for _try in range(30):
            try:
                d = np.linalg.solve(H + lam * (np.diag(np.diag(H)) + 1e-12 * np.eye(nv)), -g)
            except np.linalg.LinAlgError:
                lam *= 10.0
                continue
            Xn = [X[0]] + [se3_exp(d[6 * (i - 1):6 * i]) @ X[i] for i in range(1, n_nodes)]
            rn = residuals(Xn)
            cn = cost(rn)
            if cn <= c:
                step_ok = True
                break
            lam *= 10.0
        if not step_ok:
            break
        X, res, lam = Xn, rn, max(lam / 10.0, 1e-12)
        small = np.abs(d).max() < 1e-13 or cn < 1e-26
        c = cn
        if small:
            break
    return X, weights(res), c


def optimize_pose_graph(n_nodes, edges, prune=0.25, lc_pref=5.0, max_dist=FINE_DIST, max_iter=100):
    """Open3D's global_optimization for the segment graph.  edges: (s, t, T_st 4 x 4, Lambda_st 6 x 6, uncertain); T_st moves the
    points of segment s onto segment t, so the corrections X_i (node 0 fixed to the identity) are sought with T_st = X_t^-1 X_s.
    Uncertain (loop) edges carry a line-process weight; those ending below `prune` are dropped and the graph is optimised again.
    Returns dict(nodes [n,4,4], weights (per input edge, at the end of the first pass), kept (mask), mu, cost)."""
    edges = [(int(s), int(t), np.asarray(T, dtype=np.float64), np.asarray(L, dtype=np.float64), bool(u)) for s, t, T, L, u in edges]
    mu = line_process_mu(edges, lc_pref, max_dist)
    X = [np.eye(4) for _ in range(n_nodes)]
    X, w, c = _lm(n_nodes, edges, X, mu, max_iter)
    kept = [(not e[4]) or wi >= prune for e, wi in zip(edges, w)]
    if not all(kept):
        # the second pass keeps the surviving edges' line process on, as Open3D's second global_optimization pass does
        X, _, c = _lm(n_nodes, [e for e, k in zip(edges, kept) if k], X, mu, max_iter)
    return {'nodes': np.stack(X), 'weights': np.array(w), 'kept': np.array(kept), 'mu': mu, 'cost': c}


# ------------------------------------------------------------------------------------------------ the closer
DEFAULTS = {'enabled': False, 'method': 'robust_icp', 'candidates': 'pose', 'max_center_dist': 1.5, 'min_axis_cos': 0.5,
            'global_conf': GLOBAL_CONF, 'global_iter': GLOBAL_ITER, 'global_seed': 0,      # these three: 'fpfh_robust_icp' only
            # candidates 'appearance' only.  min_score: midway between the two figures of profiles/place_recognition.md (the highest score
            # of two views 50 or more poses apart, the lowest of two within 5)
            'min_score': MIN_SCORE, 'n_features': 500, 'n_levels': 8, 'max_hamming': 64,
            # what is registered.  'neural': the segments' neural points, normals over every point within NORMAL_RADIUS.  'tsdf': the
            # reference's clouds - every sensor frame of a closed segment fused into a TSDF volume at the tracked poses, the mesh vertices
            # kept (src/neural_point.py:960-1017); normals over the 50 nearest within the radius, the FPFH preprocessing's over 30
            # (src/common.py:606-617, 545-549).  normals_max_nn: None = those defaults (no cap for 'neural'), a number overrides the 50.
            # tsdf_every: frame stride inside a segment (1 = the reference)
            'cloud': 'neural', 'normals_max_nn': None, 'tsdf_voxel_length': 5.0 / 512.0, 'tsdf_sdf_trunc': 0.04, 'tsdf_every': 1}
CANDIDATES = ('pose', 'appearance')
CLOUDS = ('neural', 'tsdf')
SURFACE_MAX_NN, SURFACE_FPFH_MAX_NN = 50, 30               # src/common.py:606-617, 545-549


def settings(cfg):
    """cfg['loop_closure'] over the defaults (absent key: disabled)."""
    out = dict(DEFAULTS)
    out.update(cfg.get('loop_closure') or {})
    return out


class LoopCloser:
    """Owns the per-point segment id of a NeuralPointCloud and runs a closure when a segment opens (slam.Mapper calls on_new_segment)."""

    def __init__(self, cfg, npc, slam=None):
        lc = settings(cfg)
        dist = getattr(slam, 'dist', None)
        if dist is not None and getattr(dist, 'world', 1) > 1:
            raise NotImplementedError('loop_closure.enabled with world > 1: rank 0 would decide and broadcast the corrections '
                                      '(SURVEY.md 8(e)); that exchange is not built - run loop closure on one rank')
        if lc['method'] not in METHODS:
            raise NotImplementedError(f"loop_closure.method {lc['method']!r}: one of {METHODS}")
        if not callable(lc['candidates']) and lc['candidates'] not in CANDIDATES:
            raise NotImplementedError(f"loop_closure.candidates {lc['candidates']!r}: one of {CANDIDATES} or a callable")
        if lc['cloud'] not in CLOUDS:
            raise NotImplementedError(f"loop_closure.cloud {lc['cloud']!r}: one of {CLOUDS}")
        tr = cfg.get('tracking', {})
        self.cfg, self.npc, self.slam, self.eng = lc, npc, slam, npc.eng
        self.method, self.candidates = lc['method'], lc['candidates']
        # cloud 'tsdf': surface[i] = {'pos' [V,3], 'color' [V,3]} on the device, the fused sensor surface of every CLOSED segment i, moved with
        # the map at every closure; the pose graph then has one node per closed segment (the reference's use_old_segments_only).  Empty otherwise.
        self.tsdf = lc['cloud'] == 'tsdf'
        self.surface = {}
        self.max_nn = lc['normals_max_nn'] if lc['normals_max_nn'] is not None else (SURFACE_MAX_NN if self.tsdf else None)
        self.fpfh_max_nn = SURFACE_FPFH_MAX_NN if self.tsdf else None
        # place recognition (the reference's values: configs/point_slam.yaml): owned in the 'appearance' mode only
        self.kval, self.dbow_filter, self.mult_dbow = int(tr.get('kval', 2)), bool(tr.get('dbow_filter', True)), float(tr.get('mult_dbow', 1.0))
        self.min_score = float(lc['min_score'])
        self.place = None
        if lc['candidates'] == 'appearance':
            self.place = place.PlaceRecognizer(self.eng, int(lc['n_features']), int(lc['n_levels']), int(lc['max_hamming']))
        self.seg_desc, self.self_score, self.last_scores = [], [], None      # per segment: the keyframe's descriptors, compute_dbow_score's minimum
        self.global_cfg = {'conf': float(lc['global_conf']), 'max_iter': int(lc['global_iter']), 'seed': int(lc['global_seed'])}
        self.min_dist = tr.get('min_dist', 1)
        self.prune_pgo, self.lc_pref = tr.get('prune_pgo', 0.25), tr.get('lc_pref', 5.0)
        self.fitness_thresh, self.std_threshold = tr.get('fitness_thresh', 0.1), tr.get('std_threshold', 0.04)
        self.trans_mag_percentile = tr.get('trans_mag_percentile', 90)
        self.current_segment = 0
        self.loop_edges = []             # accepted loop edges of earlier closures, kept in the corrected frames
        self.odometry_info = {}          # (s, s + 1) -> information at the identity
        self.corrections = []            # per segment: the accumulated 4 x 4 correction (checkpoint 'fragments')
        self.last_edges, self.last_result, self.last_registrations = None, None, []
        npc.closer = self
        npc._seg = torch.zeros(npc.capacity, dtype=torch.int32, device=self.eng.device)

    # ---- bookkeeping
    def segment_rows(self, i):
        return torch.nonzero(self.npc._seg[:self.npc.n] == i).reshape(-1)

    def segment_cloud(self, i, segments):
        """What is registered of segment i: its stored surface cloud (cloud 'tsdf') or its neural points."""
        pos = self.surface[i]['pos'] if self.tsdf else self.npc._pos[:self.npc.n][self.segment_rows(i)]
        return SegmentCloud(self.eng, pos, segments[i]['est_c2w'][:3, 3], max_nn=self.max_nn, fpfh_max_nn=self.fpfh_max_nn)

    def fuse_closed_segments(self, segments):
        """cloud 'tsdf': every closed segment without a surface cloud yet - in a run the one that has just closed, segment len(segments) - 2
        - gets one: its frames [start, next start) stepped by tsdf_every, sensor depth and colour of slam.frame_reader at
        slam.estimate_c2w_list (tsdf.fuse_segment), the vertices and colours of the volume kept, the volume dropped."""
        from . import tsdf
        slam, lc = self.slam, self.cfg
        if slam is None:
            raise ValueError("loop_closure.cloud 'tsdf' fuses the sensor frames of a segment: the closer needs the slam object (frame_reader, estimate_c2w_list)")
        for i in range(len(segments) - 1):
            if i in self.surface:
                continue
            idxs = [f for f in range(int(segments[i]['idx']), int(segments[i + 1]['idx']), max(int(lc['tsdf_every']), 1))
                    if tsdf.pose_usable(slam.estimate_c2w_list[f])]

            def frames():
                for f in idxs:
                    _, color, depth, _ = slam.frame_reader[f]
                    yield depth, color
            vol = tsdf.fuse_segment(self.eng, frames(), [slam.estimate_c2w_list[f] for f in idxs], slam.fx, slam.fy, slam.cx, slam.cy,
                                    voxel_length=lc['tsdf_voxel_length'], sdf_trunc=lc['tsdf_sdf_trunc'])
            cloud = vol.extract_point_cloud()
            self.surface[i] = {'pos': cloud['vertices'].contiguous(), 'color': cloud['colors'].contiguous()}

    def pose_candidates(self, segments):
        """Pairs (newest, t): non-adjacent by more than tracking.min_dist, keyframe centres within max_center_dist metres and
        optical axes within min_axis_cos."""
        s = len(segments) - 1
        ks = segments[s]['est_c2w'].detach().cpu().double()
        out = []
        for t in range(s):
            if abs(s - t) <= self.min_dist:
                continue
            kt = segments[t]['est_c2w'].detach().cpu().double()
            if float((ks[:3, 3] - kt[:3, 3]).norm()) <= self.cfg['max_center_dist'] and \
                    float(torch.dot(ks[:3, 2], kt[:3, 2])) >= self.cfg['min_axis_cos']:
                out.append((s, t))
        return out

    # ---- place recognition
    def describe_segments(self, segments):
        """Every segment's keyframe is described once and joins the database, in segment order."""
        for i in range(len(self.seg_desc), len(segments)):
            _, desc = self.place.describe(segments[i]['color'])
            self.place.add(desc)
            self.seg_desc.append(desc)
            self.self_score.append(-1.0)

    def on_mapped_frame(self, color, segments):
        """slam.Mapper: a mapped frame that opens no segment.  self_score[t] of the running segment t is the lowest score between its
        keyframe and its other mapped frames (the reference's compute_dbow_score), -1 while it has none."""
        if self.place is None or not segments:
            return
        self.describe_segments(segments)
        t = len(segments) - 1
        _, desc = self.place.describe(color)
        sc = float(self.place.scores(desc)[t])
        self.self_score[t] = sc if self.self_score[t] < 0 else min(self.self_score[t], sc)

    def appearance_candidates(self, segments):
        """Pairs (newest, t) by appearance: of the earlier segments with |s - t| > tracking.min_dist, score > loop_closure.min_score and -
        tracking.dbow_filter - score > tracking.mult_dbow x self_score[t], the tracking.kval best (score descending, t ascending).
        The reference thresholds with the QUERY segment's own score; the newest segment has no frames of its own yet, so the candidate's is
        used (the score is symmetric up to the ratio test, which looks at the query's second-best match)."""
        self.describe_segments(segments)
        s = len(segments) - 1
        scores = self.place.scores(self.seg_desc[s])
        self.last_scores = scores
        ok = [t for t in range(s) if abs(s - t) > self.min_dist and scores[t] > self.min_score and
              (not self.dbow_filter or scores[t] > self.mult_dbow * self.self_score[t])]
        ok.sort(key=lambda t: (-scores[t], t))
        return [(s, t) for t in ok[:max(self.kval, 0)]]

    def filter_edges(self, regs):
        """The reference's old_trans_mag_filter branch: if the translation magnitudes of the successful loop registrations spread by no
        more than tracking.std_threshold all of them are kept; otherwise those below their trans_mag_percentile-th percentile with a
        fitness of at least tracking.fitness_thresh."""
        ok = [r for r in regs if r['success']]
        if not ok:
            return []
        mags = np.array([r['transl_mag'] for r in ok])
        if mags.std() <= self.std_threshold:
            return ok
        thr = np.percentile(mags, self.trans_mag_percentile)
        return [r for r in ok if r['transl_mag'] < thr and r['fitness'] >= self.fitness_thresh]

    # ---- one closure
    def compute_correction(self, segments):
        """Register the candidate pairs of the newest segment and optimise the pose graph.  Returns the optimize_pose_graph result,
        or None when the newest segment got no loop edge (nothing is optimised then, as in the reference).  cloud 'tsdf': the graph is
        over the CLOSED segments, segments[:-1] - candidates, the "newest" node and the n < 3 rule included."""
        if self.tsdf:
            segments = segments[:-1]
        n = len(segments)
        self.last_edges, self.last_result, self.last_registrations = None, None, []
        if n < 3:
            return None
        if callable(self.candidates):
            pairs = self.candidates(segments)
        else:
            pairs = self.appearance_candidates(segments) if self.candidates == 'appearance' else self.pose_candidates(segments)
        pairs = [(int(s), int(t)) for s, t in pairs]
        if not pairs:
            return None
        clouds = {}

        def cloud(i):
            if i not in clouds:
                clouds[i] = self.segment_cloud(i, segments)
            return clouds[i]

        try:
            regs = []
            for s, t in pairs:
                r = register_pair(cloud(s), cloud(t), self.method, adjacent=False, eng=self.eng, global_cfg=self.global_cfg)
                r.update(s=s, t=t)
                regs.append(r)
            self.last_registrations = regs
            new_loops = [(r['s'], r['t'], r['T'], r['information'], True) for r in self.filter_edges(regs)]
            if not any(n - 1 in (e[0], e[1]) for e in new_loops):
                return None
            for i in range(n - 1):
                if (i, i + 1) not in self.odometry_info:
                    self.odometry_info[(i, i + 1)] = register_pair(cloud(i), cloud(i + 1), 'identity', adjacent=True, eng=self.eng)['information']
        finally:
            _sync(self.eng)
            for c in clouds.values():
                c.close()
        edges = [(i, i + 1, np.eye(4), self.odometry_info[(i, i + 1)], False) for i in range(n - 1)] + self.loop_edges + new_loops
        self.last_edges = edges
        self.last_result = optimize_pose_graph(n, edges, prune=self.prune_pgo, lc_pref=self.lc_pref, max_dist=FINE_DIST)
        return self.last_result

    def apply(self, pose_graph, segments, estimate_c2w_list=None, keyframe_dict=None, n_frames=None):
        """Move the map by the node matrices: positions (lk_apply_correction), the frame poses of every segment, the segments' and the
        keyframes' poses, then rebuild the neighbour index."""
        nodes = np.asarray(pose_graph['nodes'] if isinstance(pose_graph, dict) else pose_graph, dtype=np.float64)
        n, npc, eng = len(segments), self.npc, self.eng
        if self.tsdf and nodes.shape[0] == n - 1:
            # one node per closed segment: the segment that has just opened (one frame so far) takes the matrix of the last closed one
            # (src/neural_point.py:164-170)
            nodes = np.concatenate([nodes, nodes[-1:]], 0)
        assert nodes.shape[0] == n
        for i, sc in self.surface.items():
            rigid_map(eng, sc['pos'], nodes[i])
        mats = torch.from_numpy(nodes[:, :3, :4].astype(np.float32).reshape(n, 12)).to(eng.device).contiguous()
        eng.lib.check(eng.lib.dll.lk_apply_correction(ptr(npc._pos), npc.n, ptr(npc._seg), ptr(mats), n, eng.stream), 'lk_apply_correction')
        if npc.n:
            npc.knn.build(npc._pos[:npc.n])
        starts = [int(sg['idx']) for sg in segments]

        def moved(X, c2w):
            # 4 x 4 algebra on the host in fp64, rounded once: the same bits wherever the pose lives
            out = torch.from_numpy(X) @ c2w.detach().cpu().double()
            out[3, :] = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)
            return out.to(c2w.dtype).to(c2w.device)

        def seg_of(frame):
            return max(int(np.searchsorted(starts, int(frame), side='right')) - 1, 0)

        if estimate_c2w_list is not None:
            end_all = len(estimate_c2w_list) if n_frames is None else n_frames
            for i in range(n):
                a, b = starts[i], (starts[i + 1] if i + 1 < n else end_all)
                if i == 0:
                    a = 0
                for f in range(a, b):
                    estimate_c2w_list[f] = moved(nodes[i], estimate_c2w_list[f])
        for i, sg in enumerate(segments):
            sg['est_c2w'] = moved(nodes[i], sg['est_c2w'])
        for kf in (keyframe_dict or []):
            kf['est_c2w'] = moved(nodes[seg_of(kf['idx'])], kf['est_c2w'])
        # remembered loop edges follow their segments: T' = X_t T X_s^-1
        kept = pose_graph['kept'] if isinstance(pose_graph, dict) and self.last_edges is not None else None
        if kept is not None:
            self.loop_edges = [(s, t, nodes[t] @ T @ _inv(nodes[s]), L, True)
                               for (s, t, T, L, u), k in zip(self.last_edges, kept) if u and k]
        while len(self.corrections) < n:
            self.corrections.append(np.eye(4))
        self.corrections = [nodes[i] @ self.corrections[i] for i in range(n)]

    def on_new_segment(self, mapper, first_new_row):
        """slam.Mapper: segment len(segments) - 1 has just opened; the rows the opening frame inserted belong to it."""
        segments = mapper.segments
        self.current_segment = len(segments) - 1
        self.npc._seg[first_new_row:self.npc.n] = self.current_segment
        if self.place is not None:
            self.describe_segments(segments)
        if self.tsdf:
            self.fuse_closed_segments(segments)
        pg = self.compute_correction(segments)
        if pg is None:
            return None
        slam = self.slam
        self.apply(pg, segments, slam.estimate_c2w_list if slam is not None else None, mapper.keyframe_dict,
                   n_frames=int(segments[-1]['idx']) + 1)
        return pg

    def fragments(self, segments):
        """The checkpoint's per-segment records."""
        out = []
        for i, sg in enumerate(segments):
            out.append({'start_idx': int(sg['idx']), 'keyframe': sg['est_c2w'].detach().cpu(),
                        'n_points': int((self.npc._seg[:self.npc.n] == i).sum()),
                        'correction': torch.from_numpy(self.corrections[i] if i < len(self.corrections) else np.eye(4))})
            if self.tsdf:
                out[-1]['n_surface_points'] = int(self.surface[i]['pos'].shape[0]) if i in self.surface else 0
        return out
