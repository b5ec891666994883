"""TSDF fusion and marching-cubes meshing (csrc/lk_tsdf.hip, loopy_slam_amd/tsdf.py) against the fp64 referee tests/tsdf_referee.py, on the
host emulator and on the GPU."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tsdf_referee as R
from util import backends, make_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTR = dict(H=60, W=80, fx=60.0, fy=60.0, cx=39.5, cy=29.5)
CAM = (INTR['fx'], INTR['fy'], INTR['cx'], INTR['cy'])
VOXEL, TRUNC = 0.02, 0.08
FRAMES = (0, 40, 80)


@functools.lru_cache(maxsize=None)
def frames():
    from loopy_slam_amd import synthetic
    return [synthetic.render_frame(k, intr=INTR, holes=0.01, scene='furnished') for k in FRAMES]


def new_volume(eng):
    from loopy_slam_amd.tsdf import TSDFVolume
    return TSDFVolume(eng, voxel_length=VOXEL, sdf_trunc=TRUNC)


def np_of(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def fused(backend):
    """The three frames integrated in order on `backend`, the referee fed the same per-frame block lists, and what test_integrate asserts
    about bits that must not move (collected while the frames go in)."""
    eng = make_engine(backend)
    vol, ref = new_volume(eng), R.Volume(VOXEL, TRUNC)
    moved = 0
    for depth, color, c2w in frames():
        before = np_of(vol.planes[:vol.n]).copy()
        touched = np_of(vol.integrate(depth, color, c2w, *CAM))
        ref.sync_slots(np_of(vol.keys))
        slots, upd, und = ref.integrate(touched, depth.numpy(), color.numpy(), c2w.numpy(), INTR)
        after = np_of(vol.planes[:vol.n])
        keep = np.ones((vol.n, R.BV), dtype=bool)                 # voxels this frame must leave alone: all but the updated / undecidable ones
        keep[slots] = ~(upd | und)
        old = np.zeros_like(after)                                # a new slot starts as zeros
        old[:len(before)] = before
        moved += int((after.view(np.uint32) != old.view(np.uint32))[np.broadcast_to(keep[:, None, :], after.shape)].sum())
    return dict(eng=eng, vol=vol, ref=ref, moved=moved)


# ---------------------------------------------------------------------------------------------------- touch
@pytest.mark.parametrize('backend', backends())
def test_touch(backend):
    eng = make_engine(backend)
    vol = new_volume(eng)
    for depth, color, c2w in frames():
        got = set(np_of(vol.touch(depth, c2w, *CAM)).tolist())
        small = R.touch(depth.numpy(), c2w.numpy(), INTR, VOXEL, TRUNC, -1e-5)
        large = R.touch(depth.numpy(), c2w.numpy(), INTR, VOXEL, TRUNC, +1e-5)
        assert len(small) > 100
        assert small <= got, len(small - got)
        assert got <= large, len(got - large)
    # a stride that divides neither side of the image: rows 0, 7, .., 56 and columns 0, 7, .., 77
    from loopy_slam_amd.tsdf import TSDFVolume
    odd = TSDFVolume(eng, voxel_length=VOXEL, sdf_trunc=TRUNC, depth_stride=7)
    depth, color, c2w = frames()[1]
    got = set(np_of(odd.touch(depth, c2w, *CAM)).tolist())
    assert R.touch(depth.numpy(), c2w.numpy(), INTR, VOXEL, TRUNC, -1e-5, stride=7) <= got <= R.touch(depth.numpy(), c2w.numpy(), INTR, VOXEL, TRUNC, +1e-5, stride=7)


# ---------------------------------------------------------------------------------------------------- integrate
@pytest.mark.parametrize('backend', backends())
def test_integrate(backend):
    f = fused(backend)
    vol, ref = f['vol'], f['ref']
    assert vol.n > 300
    frac = ref.visits_undecidable / ref.visits_inside
    print(f'blocks {vol.n}, visits inside {ref.visits_inside}, undecidable {ref.visits_undecidable} ({100 * frac:.3f} %)')
    assert frac <= 0.01
    got = np_of(vol.planes[:vol.n]).astype(np.float64)
    ok = ~ref.undecidable
    assert ok.mean() > 0.98
    assert (ref.touched & ok).sum() > 100_000
    assert np.array_equal(got[:, 1][ok], ref.planes[:, 1][ok])
    err_t = np.abs(got[:, 0] - ref.planes[:, 0])[ok].max()
    err_c = np.abs(got[:, 2:] - ref.planes[:, 2:])[np.broadcast_to(ok[:, None, :], got[:, 2:].shape)].max()
    print(f'tsdf error {err_t:.3e}, colour error {err_c:.3e} (of 255)')
    assert err_t <= 1e-4
    assert err_c <= 1e-3
    assert f['moved'] == 0
    # slots beyond the allocated ones stay zero
    assert not np_of(vol.planes[vol.n:]).any()


# ---------------------------------------------------------------------------------------------------- the generated table
def test_mc_table():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_mc_table as G
    t = G.table()
    assert G.render(t) == open(G.HEADER).read()
    assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_mc_table.py'), '--check']).returncode == 0

    def face_edges(case, axis, side):
        """directed polygon edges of the case whose two cut edges both lie on the face"""
        on = {e for e in range(12) if all(((c >> axis) & 1) == side for c in G.edge_corners(e))}
        out = set()
        for loop in G.case_loops(case):
            for a, b in zip(loop, loop[1:] + loop[:1]):
                if a in on and b in on:
                    out.add((a, b))
        return out

    def mirror_edge(e, axis):
        lo, hi = G.edge_corners(e)
        return G.EDGE_OF[frozenset((lo ^ (1 << axis), hi ^ (1 << axis)))]

    for case in range(256):
        used = {e for tri in t[case] for e in tri}
        cut = {e for e in range(12) if ((case >> G.edge_corners(e)[0]) ^ (case >> G.edge_corners(e)[1])) & 1}
        assert used == cut, case
        assert len(t[case]) <= 5
        assert len(t[case]) == sum(len(l) - 2 for l in G.case_loops(case))
        for axis in range(3):
            mirrored = sum((((case >> c) & 1) << (c ^ (1 << axis))) for c in range(8))
            for side in (0, 1):
                mine = face_edges(case, axis, side)
                theirs = {(mirror_edge(b, axis), mirror_edge(a, axis)) for a, b in face_edges(mirrored, axis, 1 - side)}
                assert mine == theirs, (case, axis, side)


# ---------------------------------------------------------------------------------------------------- sphere
CENTRE = np.array([0.013, -0.007, 0.021])
RADIUS = 0.3
ORIGIN = (-1, -1, -1)


def sphere_volume(eng, drop_block=None):
    from loopy_slam_amd.tsdf import TSDFVolume
    n = 3 * 16
    ax = [(16 * ORIGIN[a] + np.arange(n) + 0.5) * float(np.float32(VOXEL)) for a in range(3)]
    p = np.stack(np.meshgrid(*ax, indexing='ij'), -1)
    tsdf = np.clip((np.linalg.norm(p - CENTRE, axis=-1) - RADIUS) / TRUNC, -1.0, 1.0).astype(np.float32)
    weight = np.ones_like(tsdf)
    color = (255.0 * (0.5 + 0.5 * np.sin(5.0 * p))).astype(np.float32)
    if drop_block is not None:
        s = [slice(16 * (drop_block[a] - ORIGIN[a]), 16 * (drop_block[a] - ORIGIN[a]) + 16) for a in range(3)]
        weight[s[0], s[1], s[2]] = 0.0
    return TSDFVolume.from_dense(eng, tsdf, weight, color, ORIGIN, voxel_length=VOXEL, sdf_trunc=TRUNC)


def check_against_referee(vol, mesh, triangles=True, tol_color=1e-5):
    ref = R.mesh(np_of(vol.sorted_keys), np_of(vol.planes[vol.sorted_slots.long()]), VOXEL, triangles=triangles)
    assert np.array_equal(np_of(mesh['owners']), ref['owners'])
    assert len(ref['owners']) > 1000
    err_p = np.abs(np_of(mesh['vertices']).astype(np.float64) - ref['vertices']).max()
    err_c = np.abs(np_of(mesh['colors']).astype(np.float64) - ref['colors']).max()
    print(f'V {len(ref["owners"])}, F {len(mesh["triangles"])}: position error {err_p:.3e} m, colour error {err_c:.3e}')
    assert err_p <= 1e-6
    assert err_c <= tol_color
    if triangles:
        assert np.array_equal(np_of(mesh['triangles']), ref['triangles'])
    return ref


@pytest.mark.parametrize('backend', backends())
def test_mesh_sphere(backend):
    eng = make_engine(backend)
    vol = sphere_volume(eng)
    assert vol.n == 27
    mesh = vol.extract_triangle_mesh()
    check_against_referee(vol, mesh)
    v, tri = np_of(mesh['vertices']).astype(np.float64), np_of(mesh['triangles']).astype(np.int64)
    V, F = len(v), len(tri)
    assert mesh['vertices'].dtype == torch.float32 and mesh['colors'].dtype == torch.float32 and mesh['triangles'].dtype == torch.int32
    assert tri.min() >= 0 and tri.max() < V
    assert ((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 2] != tri[:, 0])).all()
    edges, counts = R.directed_edge_counts(tri, V)
    assert (counts == 1).all()                                           # every directed edge once ...
    rev = (edges % V) * V + edges // V
    assert np.array_equal(np.sort(rev), edges)                           # ... and its reverse once
    assert V - len(edges) // 2 + F == 2
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    nrm = np.cross(b - a, c - a)
    big = np.linalg.norm(nrm, axis=1) / 2 > 1e-12
    assert big.sum() > 0.9 * F
    assert (np.einsum('ij,ij->i', nrm, (a + b + c) / 3 - CENTRE)[big] > 0).all()
    h = float(np.float32(VOXEL))
    assert np.abs(np.linalg.norm(v - CENTRE, axis=1) - RADIUS).max() <= h * h / (8 * (RADIUS - h)) + 1e-6
    cloud = vol.extract_point_cloud()
    assert torch.equal(cloud['vertices'], mesh['vertices']) and torch.equal(cloud['colors'], mesh['colors'])


@pytest.mark.parametrize('backend', backends())
def test_mesh_missing_block(backend):
    eng = make_engine(backend)
    gone = (0, 0, 0)
    vol = sphere_volume(eng, drop_block=gone)
    assert vol.n == 26
    mesh = vol.extract_triangle_mesh()
    ref = check_against_referee(vol, mesh)
    tri = np_of(mesh['triangles']).astype(np.int64)
    V = len(ref['owners'])
    ev, ea = ref['edge_voxel'], ref['edge_axis']
    for t in tri:                                                        # no triangle from a cube with a corner in the missing block
        cubes = R.common_cubes(ev[t], ea[t])
        assert cubes and not all(R.cube_touches_block(q, gone) for q in cubes), t
    assert not any(R.cube_touches_block(q, gone) for q in ref['tri_cube'])
    edges, counts = R.directed_edge_counts(tri, V)
    assert (counts == 1).all()
    have = set(edges.tolist())
    open_edges = [(e // V, e % V) for e in edges.tolist() if (e % V) * V + e // V not in have]
    assert len(open_edges) > 20                                          # the hole has a rim
    for a, b in open_edges:
        cubes = R.common_cubes(ev[[a, b]], ea[[a, b]])
        assert any(R.cube_touches_block(q, gone) for q in cubes), (a, b)


@pytest.mark.parametrize('backend', backends())
def test_mesh_of_fused_volume(backend):
    vol = fused(backend)['vol']
    mesh = vol.extract_triangle_mesh()
    check_against_referee(vol, mesh, triangles=False)
    tri = np_of(mesh['triangles']).astype(np.int64)
    assert len(tri) > 1000 and tri.min() >= 0 and tri.max() < len(mesh['vertices'])
    _, counts = R.directed_edge_counts(tri, len(mesh['vertices']))
    assert (counts == 1).all()


# ---------------------------------------------------------------------------------------------------- repeatability, edge cases
@pytest.mark.parametrize('backend', backends())
def test_repeatable(backend):
    first = fused(backend)['vol']
    eng = make_engine(backend)
    again = new_volume(eng)
    for depth, color, c2w in frames():
        again.integrate(depth, color, c2w, *CAM)
    assert torch.equal(first.keys, again.keys)
    assert torch.equal(first.planes[:first.n].view(torch.int32), again.planes[:again.n].view(torch.int32))
    m0, m1 = first.extract_triangle_mesh(), again.extract_triangle_mesh()
    for k in ('vertices', 'colors'):
        assert torch.equal(m0[k].view(torch.int32), m1[k].view(torch.int32)), k
    assert torch.equal(m0['triangles'], m1['triangles']) and torch.equal(m0['owners'], m1['owners'])


@pytest.mark.parametrize('backend', backends())
def test_degenerate(backend):
    from loopy_slam_amd.tsdf import TSDFVolume
    eng = make_engine(backend)
    vol = new_volume(eng)
    depth, color, c2w = frames()[0]
    vol.integrate(torch.zeros_like(depth), color, c2w, *CAM)
    assert vol.n == 0
    mesh = vol.extract_triangle_mesh()
    assert tuple(mesh['vertices'].shape) == (0, 3) and tuple(mesh['colors'].shape) == (0, 3) and tuple(mesh['triangles'].shape) == (0, 3)
    assert tuple(vol.extract_point_cloud()['vertices'].shape) == (0, 3)
    with pytest.raises(ValueError):
        TSDFVolume(eng, voxel_length=0.01, sdf_trunc=0.0801)
    from loopy_slam_amd import _ffi
    bad = new_volume(eng)
    bad.sdf_trunc = 0.17                                                 # past the constructor: the call itself refuses
    with pytest.raises(_ffi.LoopyError):
        bad.touch(depth, c2w, *CAM)
