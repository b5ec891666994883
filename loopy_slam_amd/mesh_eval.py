"""Reconstruction evaluation of a finished mesh (csrc/lk_mesh.hip; include/loopy_hip.h "reconstruction evaluation").

Reference                                                       here
  src/tools/cull_mesh.py                                          cull -> lk_mesh_cull + lk_compact_large
  src/tools/eval_recon.py  get_align_transformation (o3d ICP)     align -> lk_nearest (bounded), Kabsch in fp64 on the host
  trimesh.sample.sample_surface                                   sample_surface -> lk_mesh_areas, lk_mesh_sample
  scipy cKDTree.query / evaluate_3d_reconstruction                metrics_3d -> lk_nearest (unbounded)
  calc_2d_metric (o3d off-screen depth capture)                   metric_2d -> lk_mesh_depth_setup + lk_mesh_depth_raster
  get_cam_position / viewmatrix / check_proj                      sample_views (-> lk_mesh_cull on the unseen points)
  trimesh.load / o3d.io.read_triangle_mesh                        read_ply

A mesh is a dict {'vertices' [V,3] f32, 'triangles' [F,3] int32, optionally 'colors' [V,3] f32 in [0, 1]} of torch tensors or arrays, as
tsdf.TSDFVolume.extract_triangle_mesh returns it.  Camera poses are 4 x 4 camera-to-world matrices in the project's convention (x right, y
up, looking down -z: tsdf._c2w16).  Every function takes `eng` (core.Engine); None: the product engine on the current device.  Bookkeeping
(cumulative sums, masks, means) is torch on the engine's device; everything that touches a point, a face or a pixel is a kernel.

Deviations from the reference, all deliberate: the view positions of sample_views come from the axis-aligned bounding box instead of
trimesh's oriented one; the principal point of metric_2d is (W / 2 - 0.5, H / 2 - 0.5) (the reference swaps H and W, equal at its 500 x 500);
the samples come from our counter-based generator, so figures agree with the reference's statistically, not sample by sample; the
rasteriser reports the nearest intersection of the pixel-centre ray (OpenGL rasterises with its own fill rule and a 24-bit depth buffer).
One process only: with torch.distributed initialised at world > 1 every entry point raises.
"""
import ctypes as C

import numpy as np
import torch

from . import core
from ._ffi import ptr

INF = float('inf')
NEAR, FAR = 0.01, 20.0                                # Open3D's near plane is dynamic; 20 m is the reference's set_constant_z_far
CULL_POSE_CHUNK = 4096
_ENGINE = None


def _engine(eng=None):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError('mesh_eval runs in one process: evaluate the written mesh outside the world > 1 job')
    global _ENGINE
    if eng is None:
        if _ENGINE is None:
            _ENGINE = core.Engine()
        eng = _ENGINE
    return eng


def _sync(eng):
    if eng.device.type == 'cuda':
        torch.cuda.current_stream(eng.device).synchronize()


def _compact(eng, mask):
    from .loop_closure import _compact as compact
    return compact(eng, mask)


def _mesh(eng, mesh):
    """(vertices [V,3] f32, triangles [F,3] int32, colours or None) on the device, indices checked."""
    v = eng.f32(mesh['vertices']).reshape(-1, 3)
    t = torch.as_tensor(mesh['triangles']).to(eng.device).reshape(-1, 3)
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= v.shape[0]):
        raise ValueError(f'mesh: a triangle index lies outside [0, {v.shape[0]})')
    c = mesh.get('colors')
    return v, t.to(torch.int32).contiguous(), (None if c is None else eng.f32(c).reshape(-1, 3))


def transform(mesh, T, eng=None):
    """The mesh with its vertices moved by the 4 x 4 T (fp64 on the device, rounded once)."""
    eng = _engine(eng)
    v, t, c = _mesh(eng, mesh)
    T = torch.as_tensor(np.asarray(T, dtype=np.float64), device=eng.device)
    out = {'vertices': (v.double() @ T[:3, :3].T + T[:3, 3]).float().contiguous(), 'triangles': t}
    if c is not None:
        out['colors'] = c
    return out


# ------------------------------------------------------------------------------------------------ PLY
_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def read_ply(path):
    """{'vertices' [V,3] f32, 'triangles' [F,3] int32, and 'colors' [V,3] f32 = uchar / 255 if the file has red, green, blue} on the host,
    from an ascii or binary PLY with triangular faces: what tsdf.write_ply writes, and the ground-truth meshes of Replica and ScanNet
    (int or uint indices, with or without colours).  A face with another number of indices raises."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.find(b'end_header')
    if not data.startswith(b'ply') or end < 0:
        raise ValueError(f'{path}: not a PLY file')
    body = data.find(b'\n', end) + 1
    fmt, elements = None, []
    for line in data[:end].decode('ascii', 'replace').splitlines():
        w = line.split()
        if not w or w[0] in ('ply', 'comment', 'obj_info'):
            continue
        if w[0] == 'format':
            fmt = w[1]
        elif w[0] == 'element':
            elements.append({'name': w[1], 'count': int(w[2]), 'props': []})
        elif w[0] == 'property':
            if w[1] == 'list':
                elements[-1]['props'].append((w[4], 'list', _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]))
            else:
                elements[-1]['props'].append((w[2], _PLY_TYPES[w[1]]))
    if fmt not in ('ascii', 'binary_little_endian'):
        raise ValueError(f'{path}: PLY format {fmt!r} is not read (ascii and binary_little_endian are)')
    tokens = data[body:].split() if fmt == 'ascii' else None
    at = 0 if fmt == 'ascii' else body
    out = {}
    for el in elements:
        n, props = el['count'], el['props']
        lists = [p for p in props if p[1] == 'list']
        if len(lists) > 1 or (lists and el['name'] != 'face') or (lists and lists[0][0] not in ('vertex_indices', 'vertex_index')):
            raise ValueError(f"{path}: element {el['name']!r} has a list property this reader does not know")
        # a face row is (count, 3 indices): any other count changes the row length, which the size check below catches
        width = sum(4 if p[1] == 'list' else 1 for p in props)
        if fmt == 'ascii':
            rows = np.array(tokens[at:at + n * width], dtype=np.float64)
            if rows.size != n * width:
                raise ValueError(f"{path}: element {el['name']!r} is short, or has faces that are not triangles")
            at += n * width
            rows = rows.reshape(n, width)
            cols, k = {}, 0
            for p in props:
                if p[1] == 'list':
                    cols['#'], cols[p[0]] = rows[:, k], rows[:, k + 1:k + 4]
                    k += 4
                else:
                    cols[p[0]] = rows[:, k]
                    k += 1
        else:
            dt = []
            for p in props:
                dt += [('#', '<' + p[2]), (p[0], '<' + p[3], 3)] if p[1] == 'list' else [(p[0], '<' + p[1])]
            dt = np.dtype(dt)
            if at + n * dt.itemsize > len(data):
                raise ValueError(f"{path}: element {el['name']!r} is short, or has faces that are not triangles")
            rec = np.frombuffer(data, dtype=dt, count=n, offset=at)
            at += n * dt.itemsize
            cols = {name: rec[name] for name in dt.names}
        if el['name'] == 'vertex':
            out['vertices'] = torch.from_numpy(np.stack([np.asarray(cols[a]).astype(np.float32) for a in 'xyz'], 1))
            if all(a in cols for a in ('red', 'green', 'blue')):
                rgb = np.stack([np.asarray(cols[a]).astype(np.float32) for a in ('red', 'green', 'blue')], 1)
                out['colors'] = torch.from_numpy(rgb / np.float32(255.0))
        elif el['name'] == 'face':
            if n and not np.all(np.asarray(cols['#']) == 3):
                raise ValueError(f'{path}: faces with other than 3 indices (triangulate the mesh first)')
            key = 'vertex_indices' if 'vertex_indices' in cols else 'vertex_index'
            idx = np.asarray(cols[key]).astype(np.int64).reshape(n, 3)
            if n and (idx.min() < 0 or idx.max() >= (1 << 31)):
                raise ValueError(f'{path}: face index out of range')
            out['triangles'] = torch.from_numpy(idx.astype(np.int32))
    if fmt != 'ascii' and at != len(data):
        raise ValueError(f'{path}: {len(data) - at} bytes left over: faces that are not triangles, or a damaged file')
    if 'vertices' not in out:
        raise ValueError(f'{path}: no vertex element')
    out.setdefault('triangles', torch.zeros(0, 3, dtype=torch.int32))
    return out


# ------------------------------------------------------------------------------------------------ nearest neighbour
class NearestIndex:
    """Uniform-grid index over target points for lk_nearest.  The cell edge is chosen for a handful of points per cell of a SURFACE-like
    cloud (N points over the bounding box's faces); lk_knn_build grows it if the box needs more than 2^22 cells."""

    def __init__(self, eng, pos, cell=None):
        self.eng = eng
        self.pos = eng.f32(pos).reshape(-1, 3)
        N = int(self.pos.shape[0])
        if cell is None:
            cell = 1.0
            if N > 1:
                e = (self.pos.max(0).values - self.pos.min(0).values).double().cpu().numpy()
                area = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0])
                cell = float(np.sqrt(4.0 * area / N)) if area > 0 else float(e.max() / N)
                cell = cell if np.isfinite(cell) and cell > 1e-4 else 1e-4
        self.cell = float(cell)
        self.knn = core.KnnIndex(eng, capacity=max(N, 1), cell_size=self.cell, max_cells=1 << 22)
        self.knn.build(self.pos)

    def query(self, q, max_dist=INF):
        """(d2 [P] f32, index [P] int32) of the nearest target of every query; beyond a finite max_dist (or with no target): (inf, -1)."""
        eng = self.eng
        q = eng.f32(q).reshape(-1, 3)
        P = int(q.shape[0])
        d2, idx = eng.empty(P), eng.empty(P, dtype=torch.int32)
        eng.lib.check(eng.lib.dll.lk_nearest(self.knn.h, ptr(q), P, C.c_float(max_dist), ptr(d2), ptr(idx), eng.stream), 'lk_nearest')
        return d2, idx

    def close(self):
        _sync(self.eng)
        self.knn.close()


def nearest(target, queries, max_dist=INF, eng=None):
    """One-shot NearestIndex(target).query(queries, max_dist)."""
    eng = _engine(eng)
    index = NearestIndex(eng, target)
    try:
        return index.query(queries, max_dist)
    finally:
        index.close()


def _distances(eng, index, q):
    """fp64 distances [P] from every query to its nearest target (the index chosen by lk_nearest, the norm retaken in fp64)."""
    q = eng.f32(q).reshape(-1, 3)
    _, idx = index.query(q)
    if int(index.pos.shape[0]) == 0:
        return torch.full((q.shape[0],), INF, dtype=torch.float64, device=eng.device)
    return (q.double() - index.pos[idx.long()].double()).norm(dim=1)


# ------------------------------------------------------------------------------------------------ surface sampling
def face_areas(mesh, eng=None):
    """fp32 areas [F] (lk_mesh_areas)."""
    eng = _engine(eng)
    v, t, _ = _mesh(eng, mesh)
    area = eng.empty(int(t.shape[0]))
    eng.lib.check(eng.lib.dll.lk_mesh_areas(ptr(v), int(v.shape[0]), ptr(t), int(t.shape[0]), ptr(area), eng.stream), 'lk_mesh_areas')
    return area


def sample_surface(mesh, n, seed=0, eng=None):
    """n area-weighted surface samples: {'points' [n,3] f32, 'faces' [n] int32, 'bary' [n,3] f32, 'areas' [F] f32, 'cum' [F] f64}.
    Sample s of a seed is a pure function of (mesh, seed, s): equal arguments give equal bits."""
    eng = _engine(eng)
    v, t, _ = _mesh(eng, mesh)
    F = int(t.shape[0])
    if F == 0:
        raise ValueError('sample_surface: the mesh has no faces')
    area = face_areas({'vertices': v, 'triangles': t}, eng)
    cum = torch.cumsum(area.double(), 0).contiguous()
    if not float(cum[-1]) > 0.0:
        raise ValueError('sample_surface: the mesh has no area')
    pts, face, bary = eng.empty(n, 3), eng.empty(n, dtype=torch.int32), eng.empty(n, 3)
    eng.lib.check(eng.lib.dll.lk_mesh_sample(ptr(v), int(v.shape[0]), ptr(t), F, ptr(cum), int(seed) & ((1 << 64) - 1), int(n),
                                             ptr(pts), ptr(face), ptr(bary), eng.stream), 'lk_mesh_sample')
    return {'points': pts, 'faces': face, 'bary': bary, 'areas': area, 'cum': cum}


# ------------------------------------------------------------------------------------------------ culling
def _poses64(poses):
    """[K,4,4] f64 on the host of a tensor, an array or a list of either; poses with a non-finite entry are dropped."""
    if torch.is_tensor(poses):
        poses = poses.detach().cpu().numpy()
    else:
        poses = [q.detach().cpu().numpy() if torch.is_tensor(q) else q for q in poses]
    p = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    return p[np.isfinite(p).all((1, 2))]


def seen_mask(points, poses, H, W, fx, fy, cx, cy, eng=None):
    """uint8 [N]: 1 where a point projects strictly inside (0, W) x (0, H) of at least one pose (lk_mesh_cull; the reference's cull_mesh.py and
    check_proj).  poses: [K,4,4] camera-to-world; they are inverted here in fp64 and staged on the device in chunks."""
    eng = _engine(eng)
    pts = eng.f32(points).reshape(-1, 3)
    N = int(pts.shape[0])
    seen = eng.zeros(N, dtype=torch.uint8)
    p = _poses64(poses)
    for k in range(0, len(p), CULL_POSE_CHUNK):
        w2c = torch.from_numpy(np.linalg.inv(p[k:k + CULL_POSE_CHUNK])[:, :3, :].astype(np.float32)).to(eng.device).contiguous()
        eng.lib.check(eng.lib.dll.lk_mesh_cull(ptr(pts), N, ptr(w2c), int(w2c.shape[0]), int(H), int(W), C.c_float(fx), C.c_float(fy),
                                               C.c_float(cx), C.c_float(cy), ptr(seen), eng.stream), 'lk_mesh_cull')
    return seen


def cull(mesh, poses, H, W, fx, fy, cx, cy, compact=True, eng=None):
    """The mesh without the faces no camera sees: a face stays if at least one of its vertices is seen; the kept faces keep their order.
    compact: vertices (and colours) no kept face refers to are removed and the indices remapped.  Also returns 'seen' [V] uint8 and
    'face_index' [F'] int32 (the kept faces' positions in the input)."""
    eng = _engine(eng)
    v, t, c = _mesh(eng, mesh)
    seen = seen_mask(v, poses, H, W, fx, fy, cx, cy, eng)
    keep = seen[t.long()].amax(1) if t.shape[0] else eng.zeros(0, dtype=torch.uint8)
    index, count = _compact(eng, keep.contiguous())
    face_index = index[:int(count.cpu()[0])].contiguous()
    faces = t[face_index.long()]
    out = {'seen': seen, 'face_index': face_index}
    if compact:
        used = eng.zeros(int(v.shape[0]), dtype=torch.uint8)
        used[faces.reshape(-1).long()] = 1
        vindex, vcount = _compact(eng, used)
        vindex = vindex[:int(vcount.cpu()[0])].long()
        remap = torch.cumsum(used, 0, dtype=torch.int32) - 1
        faces = remap[faces.long()]
        v = v[vindex]
        c = None if c is None else c[vindex]
    out.update({'vertices': v.contiguous(), 'triangles': faces.to(torch.int32).contiguous()})
    if c is not None:
        out['colors'] = c.contiguous()
    return out


# ------------------------------------------------------------------------------------------------ depth
def _w2c_cv(c2w):
    """Row-major 3 x 4 world -> camera (x right, y down, z forward) of a project camera-to-world matrix: columns 1 and 2 negated (tsdf.py's
    flip), inverted in fp64, rounded once."""
    m = np.array(torch.as_tensor(c2w).detach().cpu().numpy(), dtype=np.float64).reshape(4, 4)
    m[:3, 1] *= -1.0
    m[:3, 2] *= -1.0
    return (C.c_float * 12)(*np.linalg.inv(m)[:3, :].astype(np.float32).ravel().tolist())


class DepthRasteriser:
    """Depth images of one mesh from many views (the per-triangle buffers are allocated once)."""

    def __init__(self, mesh, H, W, fx, fy, cx, cy, near=NEAR, far=FAR, eng=None):
        self.eng = eng = _engine(eng)
        self.v, self.t, _ = _mesh(eng, mesh)
        self.cam = (int(H), int(W)) + tuple(C.c_float(x) for x in (fx, fy, cx, cy, near, far))
        F = int(self.t.shape[0])
        self.rec, self.box, self.ntiles = eng.empty(max(F, 1), 16), eng.empty(max(F, 1), 4, dtype=torch.int32), eng.empty(max(F, 1), dtype=torch.int32)

    def render(self, c2w):
        """[H,W] f32: the nearest z-depth in [near, far] along each pixel-centre ray, 0 where the mesh is not met."""
        eng, dll = self.eng, self.eng.lib.dll
        V, F = int(self.v.shape[0]), int(self.t.shape[0])
        depth = eng.empty(self.cam[0], self.cam[1])
        eng.lib.check(dll.lk_mesh_depth_setup(ptr(self.v), V, ptr(self.t), F, _w2c_cv(c2w), *self.cam, ptr(self.rec), ptr(self.box),
                                              ptr(self.ntiles), ptr(depth), eng.stream), 'lk_mesh_depth_setup')
        tile_end = torch.cumsum(self.ntiles[:F], 0, dtype=torch.int64)
        T = int(tile_end[-1]) if F else 0
        if T >= (1 << 31):
            raise ValueError('DepthRasteriser: more than 2^31 tiles in the work list')
        tile_end = tile_end.to(torch.int32).contiguous()
        eng.lib.check(dll.lk_mesh_depth_raster(ptr(self.rec), ptr(self.box), ptr(tile_end), F, T, *self.cam, ptr(depth), eng.stream),
                      'lk_mesh_depth_raster')
        return depth


def render_depth(mesh, c2w, H, W, fx, fy, cx, cy, near=NEAR, far=FAR, eng=None):
    return DepthRasteriser(mesh, H, W, fx, fy, cx, cy, near, far, eng).render(c2w)


# ------------------------------------------------------------------------------------------------ alignment
def kabsch(n, sp, sq, spq):
    """4 x 4 rigid T (det = +1) minimising sum |T p - q|^2 from the sums n, sum p [3], sum q [3], sum p q^T [3,3] (fp64)."""
    mp, mq = sp / n, sq / n
    Hm = spq / n - np.outer(mp, mq)
    U, _, Vt = np.linalg.svd(Hm)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    T = np.eye(4)
    T[:3, :3] = Vt.T @ D @ U.T
    T[:3, 3] = mq - T[:3, :3] @ mp
    return T


def align(rec, gt, threshold=0.1, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, eng=None):
    """The reference's get_align_transformation: point-to-point ICP of the rec vertices onto the gt vertices from the identity, Open3D's
    loop and stopping rule (fitness and inlier rmse both change by less than 1e-6, or max_iter updates).  Correspondences: lk_nearest with
    max_dist = threshold on the moved points rounded to fp32; the sums are formed in fp64 on the device, the fit (Kabsch) in fp64 here.
    Returns dict(T, fitness, inlier_rmse, iterations)."""
    eng = _engine(eng)
    src = eng.f32(rec['vertices']).reshape(-1, 3).double()
    index = NearestIndex(eng, gt['vertices'])
    tgt = index.pos.double()
    P = max(int(src.shape[0]), 1)
    T = np.eye(4)

    def evaluate(T):
        Td = torch.as_tensor(T, device=eng.device)
        moved = src @ Td[:3, :3].T + Td[:3, 3]
        d2, idx = index.query(moved.float().contiguous(), threshold)
        hit = idx >= 0
        p, q = moved[hit], tgt[idx[hit].long()]
        n = int(p.shape[0])
        sums = torch.cat([p.sum(0), q.sum(0), (p.T @ q).reshape(-1), d2[hit].double().sum().reshape(1)]).cpu().numpy()
        return n, sums, n / P, (float(np.sqrt(sums[15] / n)) if n else 0.0)

    try:
        n, sums, fit, rmse = evaluate(T)
        it = 0
        for it in range(1, max_iter + 1):
            if n < 3:
                break
            T = kabsch(n, sums[0:3], sums[3:6], sums[6:15].reshape(3, 3)) @ T
            n, sums, fit_new, rmse_new = evaluate(T)
            done = abs(fit_new - fit) < rel_fitness and abs(rmse_new - rmse) < rel_rmse
            fit, rmse = fit_new, rmse_new
            if done:
                break
    finally:
        index.close()
    return {'T': T, 'fitness': fit, 'inlier_rmse': rmse, 'iterations': it}


_align = align                                        # metrics_3d has a flag of that name


# ------------------------------------------------------------------------------------------------ metrics
def metrics_3d(rec, gt, n_samples=200_000, seed=0, align=True, dist_th=0.05, f_th=0.01, eng=None, return_samples=False):
    """The reference's 3D figures: 'accuracy' / 'completion' = mean distance rec -> gt / gt -> rec in cm, 'completion ratio' = share of
    gt -> rec distances below dist_th in %, 'precision' / 'recall' = share of rec -> gt / gt -> rec distances below f_th in %, 'f-score' their
    harmonic mean.  n_samples surface samples per mesh (rec: `seed`, gt: `seed + 1`), exact nearest neighbours, means in fp64.
    align: rec is first moved by align(rec, gt)."""
    eng = _engine(eng)
    if align:
        rec = transform(rec, _align(rec, gt, eng=eng)['T'], eng)
    rp = sample_surface(rec, n_samples, seed, eng)['points']
    gp = sample_surface(gt, n_samples, seed + 1, eng)['points']
    gi, ri = NearestIndex(eng, gp), NearestIndex(eng, rp)
    try:
        d_rg, d_gr = _distances(eng, gi, rp), _distances(eng, ri, gp)
    finally:
        gi.close()
        ri.close()
    prec, rec_ = float((d_rg < f_th).double().mean()), float((d_gr < f_th).double().mean())
    out = {'accuracy': float(d_rg.mean()) * 100.0, 'completion': float(d_gr.mean()) * 100.0,
           'completion ratio': float((d_gr < dist_th).double().mean()) * 100.0,
           'precision': prec * 100.0, 'recall': rec_ * 100.0,
           'f-score': (2.0 * prec * rec_ / (prec + rec_) * 100.0) if prec + rec_ > 0 else 0.0}
    if return_samples:
        out['rec_points'], out['gt_points'] = rp, gp
    return out


def _unit(x):
    return x / np.linalg.norm(x)


def viewmatrix(z, up, pos):
    """The reference's viewmatrix: columns (x, y, z, position) of a camera whose z column is `z` normalised."""
    v2 = _unit(z)
    v0 = _unit(np.cross(up, v2))
    v1 = _unit(np.cross(v2, v0))
    return np.stack([v0, v1, v2, pos], 1)


def sample_views(gt, n, seed=0, unseen=None, H=500, W=500, focal=300.0, max_tries=1000, eng=None):
    """[n,4,4] f64 camera-to-world matrices (project convention) of the reference's random evaluation views: a position drawn in the gt
    bounding box shrunk to (0.3, 0.7, 0.7) of its extents and raised by 0.4 m in z, a look-at target drawn in [-10 000, 10 000]^3 rounded to
    0.01, up = (0, 0, -1).  unseen [M,3]: a view that sees any of these points (check_proj, through lk_mesh_cull) is drawn again."""
    eng = _engine(eng)
    v = np.asarray(torch.as_tensor(gt['vertices']).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    centre, ext = 0.5 * (lo + hi) + np.array([0.0, 0.0, 0.4]), (hi - lo) * np.array([0.3, 0.7, 0.7])
    rng = np.random.RandomState(seed)
    pts = None if unseen is None or len(unseen) == 0 else eng.f32(unseen).reshape(-1, 3)
    views = []
    for _ in range(n):
        for _try in range(max_tries):
            origin = centre + (rng.rand(3) - 0.5) * ext
            target = np.round(rng.uniform(-10000.0, 10000.0, 3), 2)
            c2w = np.eye(4)
            c2w[:3, :] = viewmatrix(target - origin, np.array([0.0, 0.0, -1.0]), origin)
            c2w[:3, 1] *= -1.0                            # the reference hands this matrix to Open3D (y down, z forward); ours look down -z
            c2w[:3, 2] *= -1.0
            if pts is None or not bool(seen_mask(pts, c2w[None], H, W, focal, focal, W / 2.0 - 0.5, H / 2.0 - 0.5, eng).any()):
                break
        else:
            raise RuntimeError(f'sample_views: no view without an unseen point in {max_tries} draws')
        views.append(c2w)
    return np.stack(views) if views else np.zeros((0, 4, 4))


def metric_2d(rec, gt, views, H=500, W=500, focal=300.0, eng=None):
    """{'depth l1': cm}: per view the mean of |gt depth - rec depth| over the pixels where the rec depth is > 0, both meshes rendered with
    lk_mesh_depth; views without such a pixel are skipped; the mean over the views (nan without one)."""
    eng = _engine(eng)
    cam = (H, W, focal, focal, W / 2.0 - 0.5, H / 2.0 - 0.5)
    r_rec, r_gt = DepthRasteriser(rec, *cam, eng=eng), DepthRasteriser(gt, *cam, eng=eng)
    errors = []
    for c2w in np.asarray(views, dtype=np.float64).reshape(-1, 4, 4):
        d_rec, d_gt = r_rec.render(c2w), r_gt.render(c2w)
        on = d_rec > 0
        if bool(on.any()):
            errors.append(float((d_gt[on].double() - d_rec[on].double()).abs().mean()))
    return {'depth l1': float(np.mean(errors)) * 100.0 if errors else float('nan')}
