"""fp64 NumPy restatement of the TSDF fusion and marching-cubes contracts (include/loopy_hip.h "TSDF fusion and meshing"), written from the
contract and from Open3D's documented behaviour (ScalableTSDFVolume: integrate, extract_triangle_mesh).  Test-only."""
import os
import sys

import numpy as np

B, BV = 16, 4096
BIAS = 1 << 20
MASK = (1 << 21) - 1

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import gen_mc_table  # noqa: E402

_TABLE = gen_mc_table.table()


def pack(b):
    b = np.asarray(b, dtype=np.int64)
    return ((b[..., 0] + BIAS) << 42) | ((b[..., 1] + BIAS) << 21) | (b[..., 2] + BIAS)


def unpack(keys):
    keys = np.asarray(keys, dtype=np.int64)
    return np.stack([((keys >> 42) & MASK) - BIAS, ((keys >> 21) & MASK) - BIAS, (keys & MASK) - BIAS], -1)


def cv_c2w(c2w):
    """The project's camera (y up, looks down -z) as Open3D's (y down, looks down +z): columns 1 and 2 negated."""
    m = np.array(c2w, dtype=np.float64)
    m[:3, 1] *= -1.0
    m[:3, 2] *= -1.0
    return m


# ------------------------------------------------------------------------------------------------ touch
def touch(depth, c2w, intr, voxel, trunc, margin, stride=4, depth_trunc=30.0):
    """Keys of the blocks overlapped by the boxes p +- (trunc + margin) of the sampled pixels (a set)."""
    d = np.asarray(depth, dtype=np.float64)[::stride, ::stride]
    H, W = np.asarray(depth).shape
    jj, ii = np.meshgrid(np.arange(0, H, stride, dtype=np.float64), np.arange(0, W, stride, dtype=np.float64), indexing='ij')
    ok = (d > 0) & (d < depth_trunc)
    d, ii, jj = d[ok], ii[ok], jj[ok]
    pc = np.stack([(ii - intr['cx']) * d / intr['fx'], (jj - intr['cy']) * d / intr['fy'], d, np.ones_like(d)], -1)
    p = (pc @ cv_c2w(c2w).T)[:, :3]
    bs = B * float(np.float32(voxel))
    lo, hi = np.floor((p - (trunc + margin)) / bs).astype(np.int64), np.floor((p + (trunc + margin)) / bs).astype(np.int64)
    out = set()
    for o in range(8):
        off = np.array([o & 1, (o >> 1) & 1, o >> 2])
        b = lo + off
        keep = (b <= hi).all(-1)
        out.update(pack(b[keep]).tolist())
    return out


# ------------------------------------------------------------------------------------------------ integrate
def _local():
    v = np.arange(BV)
    return np.stack([v & 15, (v >> 4) & 15, v >> 8], -1)                   # [4096,3] (i, j, k) of a voxel index


class Volume:
    """Planes [n,5,4096] in fp64 in the device's slot order, plus what the comparison needs: `undecidable` [n,4096] marks voxels with a visit
    whose branch fp32 may legitimately take the other way."""

    def __init__(self, voxel, trunc, depth_trunc=30.0):
        self.voxel, self.trunc, self.depth_trunc = float(np.float32(voxel)), float(np.float32(trunc)), float(np.float32(depth_trunc))
        self.keys = np.zeros(0, dtype=np.int64)
        self.planes = np.zeros((0, 5, BV))
        self.undecidable = np.zeros((0, BV), dtype=bool)
        self.touched = np.zeros((0, BV), dtype=bool)                       # voxels some visit updated
        self.visits_inside, self.visits_undecidable = 0, 0

    def sync_slots(self, keys):
        """Adopt the device's slot order: `keys` extends self.keys."""
        keys = np.asarray(keys, dtype=np.int64)
        assert np.array_equal(keys[:len(self.keys)], self.keys)
        k = len(keys) - len(self.keys)
        self.keys = keys.copy()
        self.planes = np.concatenate([self.planes, np.zeros((k, 5, BV))])
        self.undecidable = np.concatenate([self.undecidable, np.zeros((k, BV), dtype=bool)])
        self.touched = np.concatenate([self.touched, np.zeros((k, BV), dtype=bool)])

    def integrate(self, touched_keys, depth, color, c2w, intr):
        slot_of = {int(k): s for s, k in enumerate(self.keys)}
        slots = np.array([slot_of[int(k)] for k in touched_keys], dtype=np.int64)
        depth = np.asarray(depth, dtype=np.float64)
        H, W = depth.shape
        q = np.floor(np.clip(np.asarray(color, dtype=np.float32), np.float32(0), np.float32(1)) * np.float32(255)).astype(np.float64)
        centre = ((B * unpack(self.keys[slots])[:, None, :] + _local()[None]) + 0.5) * self.voxel            # [m,4096,3]
        w2c = np.linalg.inv(cv_c2w(c2w))
        pc = centre @ w2c[:3, :3].T + w2c[:3, 3]
        x, y, z = pc[..., 0], pc[..., 1], pc[..., 2]
        und = np.abs(z) < 1e-6
        front = z > 0
        zs = np.where(front, z, 1.0)
        u, v = x * intr['fx'] / zs + intr['cx'] + 0.5, y * intr['fy'] / zs + intr['cy'] + 0.5
        near_edge = (np.abs(u - np.rint(u)) < 1e-3) | (np.abs(v - np.rint(v)) < 1e-3)
        inside = front & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        und |= front & near_edge & (u > -1e-3) & (u < W + 1e-3) & (v > -1e-3) & (v < H + 1e-3)
        iu, iv = np.where(inside, u, 0).astype(np.int64), np.where(inside, v, 0).astype(np.int64)
        d = depth[iv, iu]
        valid = inside & (d > 0) & (d < self.depth_trunc)
        xx, yy = (iu - intr['cx']) / intr['fx'], (iv - intr['cy']) / intr['fy']
        sdf = (d - z) * np.sqrt(xx * xx + yy * yy + 1.0)
        und |= valid & (np.abs(sdf + self.trunc) < 1e-5)
        upd = valid & (sdf > -self.trunc)
        t = np.minimum(1.0, sdf / self.trunc)
        self.visits_inside += int(inside.sum())
        self.visits_undecidable += int(und.sum())
        P = self.planes[slots]
        w = P[:, 1]
        new = P.copy()
        new[:, 0] = (P[:, 0] * w + t) / (w + 1)
        for c in range(3):
            new[:, 2 + c] = (P[:, 2 + c] * w + q[iv, iu, c]) / (w + 1)
        new[:, 1] = w + 1
        self.planes[slots] = np.where(upd[:, None, :], new, P)
        self.undecidable[slots] |= und
        self.touched[slots] |= upd
        return slots, upd, und


# ------------------------------------------------------------------------------------------------ marching cubes
def _edge(e):
    """(offset of the lower corner [3], axis) of edge e = 4 axis + b1 + 2 b2."""
    a, b1, b2 = e // 4, e & 1, (e >> 1) & 1
    off = [0, 0, 0]
    o = [k for k in range(3) if k != a]
    off[o[0]], off[o[1]] = b1, b2
    return np.array(off), a


def mesh(sorted_keys, planes, voxel, triangles=True):
    """Marching cubes over blocks given in ascending key order (planes [n,5,4096], any float type, used as they are).  Returns owners [V]
    (ascending ids (position * 4096 + voxel) * 3 + axis of the cut edges of active cubes), vertices [V,3], colors [V,3], triangles [F,3],
    tri_cube [F,3] (global voxel coordinates of the cube each triangle comes from)."""
    sorted_keys = np.asarray(sorted_keys, dtype=np.int64)
    planes = np.asarray(planes, dtype=np.float64)
    voxel = float(np.float32(voxel))
    n = len(sorted_keys)
    blocks = unpack(sorted_keys)
    loc = _local()

    def find(b):
        pos = np.clip(np.searchsorted(sorted_keys, pack(b)), 0, max(n - 1, 0))
        return np.where(sorted_keys[pos] == pack(b), pos, -1)

    def locate(g):
        """(position of the block, voxel index) of global voxel coordinates g[..., 3]; position -1 where the block is absent"""
        l = np.mod(g, B)
        return find(np.floor_divide(g, B)), (l[..., 2] * B + l[..., 1]) * B + l[..., 0]

    def sample(g, plane):
        pos, vox = locate(g)
        return planes[np.maximum(pos, 0), plane, vox], pos >= 0

    g0 = (B * blocks[:, None, :] + loc[None]).reshape(-1, 3)                # global coordinates of every cube's corner 0
    active = np.ones(len(g0), dtype=bool)
    code = np.zeros(len(g0), dtype=np.int64)
    for c in range(8):
        off = np.array([c & 1, (c >> 1) & 1, c >> 2])
        pos, vox = locate(g0 + off)
        ex = pos >= 0
        w, f = planes[np.maximum(pos, 0), 1, vox], planes[np.maximum(pos, 0), 0, vox]
        active &= ex & (w > 0)
        code |= (f < 0).astype(np.int64) << c
    code = np.where(active, code, 0)
    edges = []
    for e in range(12):
        off, a = _edge(e)
        lo = off[0] | off[1] << 1 | off[2] << 2
        cut = ((code >> lo) ^ (code >> (lo | 1 << a))) & 1
        g = g0[cut == 1] + off
        edges.append(np.concatenate([g, np.full((len(g), 1), a)], 1))
    edges = np.concatenate(edges)

    def owner_id(g, a):
        pos = find(np.floor_divide(g, B))
        assert (pos >= 0).all()
        l = np.mod(g, B)
        return (pos * BV + (l[..., 2] * B + l[..., 1]) * B + l[..., 0]) * 3 + a

    ids = owner_id(edges[:, :3], edges[:, 3])
    owners, first = np.unique(ids, return_index=True)
    eg, ea = edges[first, :3], edges[first, 3]
    g1 = eg.copy()
    g1[np.arange(len(g1)), ea] += 1
    f0, f1 = sample(eg, 0)[0], sample(g1, 0)[0]
    t = f0 / (f0 - f1)
    p0, p1 = (eg + 0.5) * voxel, (g1 + 0.5) * voxel
    vertices = p0 + t[:, None] * (p1 - p0)
    colors = np.stack([sample(eg, 2 + c)[0] + t * (sample(g1, 2 + c)[0] - sample(eg, 2 + c)[0]) for c in range(3)], -1) / 255.0
    tris, cubes = [], []
    ntri = np.array([len(x) for x in _TABLE])
    for cube in (np.nonzero(ntri[code] > 0)[0] if triangles else ()):
        for tri in _TABLE[code[cube]]:
            row = []
            for e in tri:
                off, a = _edge(e)
                row.append(np.searchsorted(owners, owner_id(g0[cube] + off, a)))
            tris.append(row)
            cubes.append(g0[cube])
    triangles = np.array(tris, dtype=np.int64).reshape(-1, 3)
    return dict(owners=owners, vertices=vertices, colors=colors, triangles=triangles, tri_cube=np.array(cubes, dtype=np.int64).reshape(-1, 3),
                edge_voxel=eg, edge_axis=ea)


def directed_edge_counts(tri, V):
    """(unique directed edges a * V + b, their counts)"""
    tri = np.asarray(tri, dtype=np.int64)
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    return np.unique(e[:, 0] * V + e[:, 1], return_counts=True)


def common_cubes(edge_voxels, edge_axes):
    """Global coordinates of the cubes that contain all of the given lattice edges (lower voxel [m,3], axis [m])."""
    g = np.asarray(edge_voxels, dtype=np.int64)
    top = g.copy()
    top[np.arange(len(g)), np.asarray(edge_axes)] += 1
    lo, hi = top.max(0) - 1, g.min(0)
    out = []
    for x in range(lo[0], hi[0] + 1):
        for y in range(lo[1], hi[1] + 1):
            for z in range(lo[2], hi[2] + 1):
                out.append((x, y, z))
    return out


def cube_touches_block(q, block):
    """Does the cube at global voxel q have a corner in block `block`?"""
    q, lo = np.asarray(q), B * np.asarray(block)
    return bool(np.all((q + 1 >= lo) & (q <= lo + B - 1)))
