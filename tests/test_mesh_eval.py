"""Reconstruction evaluation (csrc/lk_mesh.hip, loopy_slam_amd/mesh_eval.py) against the fp64 referee tests/mesh_eval_referee.py, on the host
emulator and on the GPU.  Every test prints the worst figure behind each of its bounds (profiles/mesh_eval.md records them)."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_eval_referee as R
from util import backends, make_engine

INTR = dict(H=60, W=80, fx=60.0, fy=60.0, cx=39.5, cy=29.5)
CAM = (INTR['fx'], INTR['fy'], INTR['cx'], INTR['cy'])
VOXEL, TRUNC = 0.02, 0.08
FRAMES = (0, 40, 80)


def np_of(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def frames():
    from loopy_slam_amd import synthetic
    return [synthetic.render_frame(k, intr=INTR, holes=0.01, scene='furnished') for k in FRAMES]


@functools.lru_cache(maxsize=None)
def fused_mesh(backend):
    """The furnished room's three 80 x 60 frames fused and meshed on `backend` (the fixture of tests/test_tsdf.py), as host arrays."""
    from loopy_slam_amd.tsdf import TSDFVolume
    eng = make_engine(backend)
    vol = TSDFVolume(eng, voxel_length=VOXEL, sdf_trunc=TRUNC)
    for depth, color, c2w in frames():
        vol.integrate(depth, color, c2w, *CAM)
    m = vol.extract_triangle_mesh()
    return {k: np_of(m[k]) for k in ('vertices', 'colors', 'triangles')}


# ---------------------------------------------------------------------------------------------------- nearest
NEAREST_SEED = 11


@functools.lru_cache(maxsize=None)
def nearest_case():
    """3 000 targets in a 4 m box - two clusters with empty cells between them, 50 exact duplicates, 50 strays - and 1 003 queries: 20 of
    them 3 m outside the box, 100 that are targets themselves; with the referee's answers."""
    rng = np.random.RandomState(NEAREST_SEED)
    a = rng.uniform(0.0, 1.2, (1400, 3))
    b = rng.uniform(2.8, 4.0, (1500, 3))
    stray = rng.uniform(0.0, 4.0, (50, 3))
    tgt = np.concatenate([a, b, stray]).astype(np.float32)
    tgt = np.concatenate([tgt, tgt[100:150]])                          # exact duplicates of lower-numbered points
    assert tgt.shape == (3000, 3)
    out = rng.uniform(0.0, 4.0, (20, 3))
    out[:10, 0] = 7.0 + rng.uniform(0.0, 0.2, 10)                      # 3 m beyond the box in +x
    out[10:, 1] = -3.0 - rng.uniform(0.0, 0.2, 10)                     # ... and in -y
    own = tgt[rng.choice(3000, 100, replace=False)]
    own[:10] = tgt[100:110]                                            # ten of them on duplicated targets
    near = tgt[rng.choice(3000, 300)] + rng.normal(0.0, 0.03, (300, 3))
    free = rng.uniform(-0.2, 4.2, (583, 3))                            # the gap between the clusters included
    q = np.concatenate([out, own, near, free]).astype(np.float32)
    assert q.shape == (1003, 3)
    d, i = R.nearest(tgt, q)
    return tgt, q, d, i


@pytest.mark.parametrize('backend', backends())
def test_nearest(backend):
    from loopy_slam_amd import mesh_eval as E
    eng = make_engine(backend)
    tgt, q, d_ref, _ = nearest_case()
    t64, q64 = tgt.astype(np.float64), q.astype(np.float64)
    worst_d = worst_own = 0.0
    for cell in (None, 0.1, 0.7):                                      # the module's own choice, a fine grid (many doublings), a coarse one
        index = E.NearestIndex(eng, tgt, cell=cell)
        d2, idx = index.query(q)
        d2b, idxb = index.query(q)
        assert torch.equal(d2.view(torch.int32), d2b.view(torch.int32)) and torch.equal(idx, idxb)
        d, idx = np.sqrt(np_of(d2).astype(np.float64)), np_of(idx)
        assert idx.min() >= 0 and idx.max() < 3000
        worst_d = max(worst_d, np.abs(d - d_ref).max())
        worst_own = max(worst_own, np.abs(np.linalg.norm(q64 - t64[idx], axis=1) - d_ref).max())
        # ties go to the lower index: a query on a duplicated target gets the original, not the copy
        assert np.array_equal(idx[20:30], np.arange(100, 110))
        assert (np_of(d2)[20:120] == 0).all()
        # bounded
        cut = 0.05
        d2c, idxc = index.query(q, cut)
        d2c2, idxc2 = index.query(q, cut)
        assert torch.equal(d2c.view(torch.int32), d2c2.view(torch.int32)) and torch.equal(idxc, idxc2)
        hit, hit_ref, close = np_of(idxc) >= 0, d_ref <= cut, np.abs(d_ref - cut) < 1e-6
        assert close.sum() < 0.01 * len(q)                             # the seed leaves the referee itself below the cap
        assert 100 < hit_ref.sum() < 900
        assert np.array_equal(hit[~close], hit_ref[~close])
        assert np.isinf(np_of(d2c)[~hit]).all() and (np_of(idxc)[~hit] == -1).all()
        assert np.array_equal(np_of(idxc)[hit & ~close], idx[hit & ~close])
        assert np.array_equal(np_of(d2c)[hit & ~close], np_of(d2)[hit & ~close])
        index.close()
    print(f'nearest: |d - d_ref| max {worst_d:.3e} m, own fp64 distance of the returned index vs the minimum {worst_own:.3e} m (bound 2e-6)')
    assert worst_d <= 2e-6 and worst_own <= 2e-6


@pytest.mark.parametrize('backend', backends())
def test_nearest_small_indexes(backend):
    from loopy_slam_amd import mesh_eval as E
    eng = make_engine(backend)
    _, q, _, _ = nearest_case()
    one = np.array([[1.0, 2.0, 3.0]], np.float32)
    d2, idx = E.nearest(one, q, eng=eng)
    assert (np_of(idx) == 0).all()
    assert np.abs(np.sqrt(np_of(d2).astype(np.float64)) - np.linalg.norm(q.astype(np.float64) - one, axis=1)).max() <= 2e-6
    d2, idx = E.nearest(one, q, 0.5, eng=eng)
    ref = np.linalg.norm(q.astype(np.float64) - one, axis=1) <= 0.5
    assert np.array_equal(np_of(idx) >= 0, ref)
    for cut in (E.INF, 0.05):
        d2, idx = E.nearest(np.zeros((0, 3), np.float32), q, cut, eng=eng)
        assert (np_of(idx) == -1).all() and np.isinf(np_of(d2)).all()
    d2, idx = E.nearest(one, np.zeros((0, 3), np.float32), eng=eng)
    assert tuple(d2.shape) == (0,) and tuple(idx.shape) == (0,)


# ---------------------------------------------------------------------------------------------------- sampling
ZERO_FACES = (7, 50, 123, 200, 298)
S = 20_011


@functools.lru_cache(maxsize=None)
def sample_mesh():
    """300 separate triangles inside +-2 m with areas spanning 1 : 1 000, five of them without area."""
    rng = np.random.RandomState(5)
    v = np.zeros((900, 3))
    for k in range(300):
        L = 0.01 * np.sqrt(10.0 ** (3.0 * k / 299.0))
        u1 = rng.normal(size=3)
        u1 /= np.linalg.norm(u1)
        u2 = np.cross(u1, rng.normal(size=3))
        u2 /= np.linalg.norm(u2)                                       # a right angle at vertex 0: area L^2 / 2
        p0 = rng.uniform(-1.5, 1.5, 3)
        v[3 * k:3 * k + 3] = p0, p0 + L * u1, p0 + L * u2
    v = v.astype(np.float32)
    for k in ZERO_FACES:
        v[3 * k + 2] = v[3 * k + 1]
    return v, np.arange(900, dtype=np.int32).reshape(300, 3)


@pytest.mark.parametrize('backend', backends())
def test_sample_surface(backend):
    from loopy_slam_amd import mesh_eval as E
    eng = make_engine(backend)
    v, t = sample_mesh()
    mesh = {'vertices': v, 'triangles': t}
    s = E.sample_surface(mesh, S, seed=3, eng=eng)
    area, cum = np_of(s['areas']).astype(np.float64), np_of(s['cum'])
    ref_area = R.areas(v, t)
    pos_area = ref_area > 0
    assert (~pos_area).sum() == 5 and (area[~pos_area] == 0).all()
    assert 999 < ref_area[pos_area].max() / ref_area[pos_area].min() < 1001 * 1.01
    err_a = np.abs(area / np.where(pos_area, ref_area, 1.0) - 1.0)[pos_area].max()
    assert np.abs(cum - np.cumsum(area)).max() <= 1e-12 * cum[-1]
    face, bary, pts = np_of(s['faces']), np_of(s['bary']), np_of(s['points']).astype(np.float64)
    face_ref, bary_ref = R.sample(cum, 3, S)
    assert np.array_equal(face, face_ref)
    assert not np.isin(face, ZERO_FACES).any()
    b64 = bary.astype(np.float64)
    err_sum = np.abs(b64.sum(1) - 1.0).max()
    err_b = np.abs(b64 - bary_ref.astype(np.float64)).max()
    v64 = v.astype(np.float64)
    comb = sum(b64[:, c:c + 1] * v64[t[face, c]] for c in range(3))
    err_p = np.linalg.norm(pts - comb, axis=1).max()
    print(f'sampling: area rel. error {err_a:.3e} (1e-5), |sum bary - 1| {err_sum:.3e} (2e-7), bary vs referee {err_b:.3e} (2e-7), '
          f'position {err_p:.3e} m (1e-6)')
    assert err_a <= 1e-5
    assert (bary >= 0).all() and err_sum <= 2e-7 and err_b <= 2e-7
    assert err_p <= 1e-6
    # counts: binomial, faces with an expectation below 5 pooled into one bin
    p = area / area.sum()
    counts = np.bincount(face, minlength=300).astype(np.float64)
    small = S * p < 5
    pc = np.append(p[~small], p[small].sum())
    cc = np.append(counts[~small], counts[small].sum())
    dev = np.abs(cc - S * pc) / np.sqrt(S * pc * (1 - pc))
    print(f'sampling: {int((~small).sum())} faces + 1 pooled bin, worst deviation {dev.max():.2f} sigma (5)')
    assert (~small).sum() > 100 and dev.max() <= 5.0
    # repeatable, seeded
    again = E.sample_surface(mesh, S, seed=3, eng=eng)
    for k in ('points', 'bary'):
        assert torch.equal(s[k].view(torch.int32), again[k].view(torch.int32)), k
    assert torch.equal(s['faces'], again['faces'])
    other = E.sample_surface(mesh, S, seed=4, eng=eng)
    assert (np_of(other['faces']) != face).mean() > 0.5
    with pytest.raises(ValueError):
        E.sample_surface({'vertices': v, 'triangles': t[list(ZERO_FACES)]}, 10, eng=eng)
    with pytest.raises(ValueError):
        E.sample_surface({'vertices': v, 'triangles': np.array([[0, 1, 900]])}, 10, eng=eng)


# ---------------------------------------------------------------------------------------------------- culling
def cull_poses():
    from loopy_slam_amd import synthetic
    return np.stack([synthetic.loop_pose(k).numpy().astype(np.float64) for k in (0, 20, 40, 60, 80, 120, 160)])


@pytest.mark.parametrize('backend', backends())
def test_cull(backend):
    from loopy_slam_amd import mesh_eval as E
    eng = make_engine(backend)
    mesh = fused_mesh(backend)
    v, t = mesh['vertices'], mesh['triangles']
    poses = cull_poses()
    H, W = 40, 56                                                     # narrower than the frames were: part of the mesh is out of every view
    cam = (H, W, 60.0, 60.0, 27.5, 19.5)
    seen_ref, und = R.seen(v, poses, *cam)
    out = E.cull(mesh, poses, *cam, compact=False, eng=eng)
    seen = np_of(out['seen']).astype(bool)
    print(f'cull: V {len(v)}, F {len(t)}, seen {seen_ref.mean():.3f}, undecidable {und.mean():.5f} (0.01)')
    assert und.mean() <= 0.01
    assert 0.05 < seen_ref.mean() < 0.95
    assert np.array_equal(seen[~und], seen_ref[~und])
    # faces: kept iff a vertex is seen; judged where the referee can decide
    keep_sure = (seen_ref & ~und)[t].any(1)
    drop_sure = (~seen_ref & ~und)[t].all(1)
    kept = np.zeros(len(t), bool)
    kept[np_of(out['face_index'])] = True
    assert np.array_equal(kept[keep_sure | drop_sure], keep_sure[keep_sure | drop_sure])
    assert np.array_equal(kept, seen[t].any(1))
    assert np.array_equal(np_of(out['triangles']), t[kept])           # original order, original indices
    assert np.array_equal(np_of(out['vertices']), v)
    # compact: the same corner positions and colours, in order; no vertex left unreferenced
    c = E.cull(mesh, poses, *cam, compact=True, eng=eng)
    cv, ct, cc = np_of(c['vertices']), np_of(c['triangles']), np_of(c['colors'])
    assert len(cv) < len(v) and np.array_equal(np.unique(ct), np.arange(len(cv)))
    assert np.array_equal(cv[ct], v[t[kept]]) and np.array_equal(cc[ct], mesh['colors'][t[kept]])
    # one pose that sees nothing
    away = np.eye(4)
    away[:3, 3] = (0.0, 0.0, -500.0)                                # looks down -z, the room behind it
    e = E.cull(mesh, away[None], *cam, compact=True, eng=eng)
    assert tuple(e['vertices'].shape) == (0, 3) and tuple(e['triangles'].shape) == (0, 3) and tuple(e['colors'].shape) == (0, 3)
    e = E.cull(mesh, np.zeros((0, 4, 4)), *cam, compact=False, eng=eng)
    assert tuple(e['triangles'].shape) == (0, 3) and len(e['vertices']) == len(v)


# ---------------------------------------------------------------------------------------------------- depth
DEPTH_CAM = dict(H=30, W=40, fx=30.0, fy=30.0, cx=19.5, cy=14.5)


@functools.lru_cache(maxsize=None)
def depth_scene():
    """About 200 triangles given in camera axes (x right, y down, z forward) and moved into the world by a camera pose: one covers the
    whole image, one crosses the camera plane, slivers thinner than a pixel, a wall seen from behind, one beyond `far`, and small ones."""
    from loopy_slam_amd import synthetic
    rng = np.random.RandomState(2)
    tri = [[(-8.0, -2.5, 4.0), (8.0, -2.5, 4.0), (0.0, 7.5, 4.0)],                              # the whole image (a pixel is 0.13 m there)
           [(-0.3, 0.4, -0.5), (0.4, 0.5, -0.5), (0.1, -0.2, 2.5)],                             # through the camera plane
           [(-1.0, -1.0, 3.0), (-1.0, 0.5, 3.0), (0.8, 0.5, 3.2)], [(-1.0, -1.0, 3.0), (0.8, 0.5, 3.2), (0.8, -1.0, 3.2)],   # a wall ...
           [(-30.0, -30.0, 25.0), (30.0, -30.0, 25.0), (0.0, 40.0, 25.0)]]                      # beyond far
    tri[2], tri[3] = [tri[2][k] for k in (0, 2, 1)], [tri[3][k] for k in (0, 2, 1)]             # ... wound to face away
    for _ in range(20):                                                # slivers: 1 m long, 0.3 pixel wide at 2 m
        c, ang = np.array([rng.uniform(-1, 1), rng.uniform(-0.8, 0.8), 2.0 + rng.uniform(-0.2, 0.2)]), rng.uniform(0, np.pi)
        along, across = np.array([np.cos(ang), np.sin(ang), 0.1]), np.array([-np.sin(ang), np.cos(ang), 0.0])
        tri.append([c - 0.5 * along, c + 0.5 * along, c + 0.02 * across])
    while len(tri) < 200:
        c = np.array([rng.uniform(-2.5, 2.5), rng.uniform(-2.0, 2.0), rng.uniform(1.0, 5.0)])
        tri.append([c + rng.uniform(-0.4, 0.4, 3) for _ in range(3)])
    cam = np.array(tri, np.float64).reshape(-1, 3)
    c2w = synthetic.loop_pose(7).numpy().astype(np.float64)
    cv = c2w.copy()
    cv[:3, 1] *= -1.0
    cv[:3, 2] *= -1.0                                                  # camera (y down, z forward) -> world
    world = (cam @ cv[:3, :3].T + cv[:3, 3]).astype(np.float32)
    # weld a few: the wall's two triangles share their diagonal through shared vertex ids
    t = np.arange(len(world), dtype=np.int32).reshape(-1, 3)
    t[3, 0], t[3, 2] = t[2, 0], t[2, 1]
    return world, t, c2w


@pytest.mark.parametrize('backend', backends())
def test_depth(backend):
    from loopy_slam_amd import mesh_eval as E
    eng = make_engine(backend)
    v, t, c2w = depth_scene()
    K = DEPTH_CAM
    cam = (K['H'], K['W'], K['fx'], K['fy'], K['cx'], K['cy'])
    ref, und = R.depth(v, t, c2w, *cam)
    mesh = {'vertices': v, 'triangles': t}
    got_t = E.render_depth(mesh, c2w, *cam, eng=eng)
    got = np_of(got_t).astype(np.float64)
    ok = ~und
    err = np.abs(got - ref)[ok & (ref > 0)].max()
    print(f'depth: undecidable {und.mean():.4f} (0.03), covered {np.mean(ref > 0):.3f}, |z - z_ref| max {err:.3e} m (5e-4), '
          f'range {ref[ref > 0].min():.3f} .. {ref.max():.3f} m')
    assert und.mean() <= 0.03
    assert (ref > 0).all()                                            # the big triangle is behind every pixel
    assert ref.max() < 4.01 and ref[ref > 0].min() < 1.0       # nothing from beyond far; the crossing triangle is seen close up
    assert np.array_equal((got > 0)[ok], (ref > 0)[ok])
    assert err <= 5e-4
    again = E.render_depth(mesh, c2w, *cam, eng=eng)
    assert torch.equal(got_t.view(torch.int32), again.view(torch.int32))
    # without the big triangle there are empty pixels, and they read 0; the triangle beyond far alone gives an empty image
    ref2, und2 = R.depth(v, t[1:], c2w, *cam)
    got2 = np_of(E.render_depth({'vertices': v, 'triangles': t[1:]}, c2w, *cam, eng=eng)).astype(np.float64)
    ok2 = ~und2
    assert und2.mean() <= 0.03 and 0.05 < np.mean(ref2 == 0) < 0.95
    assert np.array_equal((got2 > 0)[ok2], (ref2 > 0)[ok2]) and np.abs(got2 - ref2)[ok2].max() <= 5e-4
    assert not np_of(E.render_depth({'vertices': v, 'triangles': t[4:5]}, c2w, *cam, eng=eng)).any()
    assert not np_of(E.render_depth({'vertices': v, 'triangles': t[:0]}, c2w, *cam, eng=eng)).any()


# ---------------------------------------------------------------------------------------------------- metrics
def square(z, side=1.0):
    v = np.array([[0, 0, z], [side, 0, z], [side, side, z], [0, side, z]], np.float32)
    return {'vertices': v, 'triangles': np.array([[0, 1, 2], [0, 2, 3]], np.int32)}


@pytest.mark.parametrize('backend', backends())
def test_metrics_3d(backend):
    from loopy_slam_amd import mesh_eval as E
    eng = make_engine(backend)
    m = E.metrics_3d(square(0.03), square(0.0), n_samples=20_000, seed=1, align=False, eng=eng, return_samples=True)
    ref = R.metrics(np_of(m['rec_points']), np_of(m['gt_points']))
    keys = ('accuracy', 'completion', 'completion ratio', 'precision', 'recall', 'f-score')
    rel = max(abs(m[k] - ref[k]) / max(abs(ref[k]), 1e-300) for k in keys if ref[k] != 0)
    print('metrics: ' + ', '.join(f'{k} {m[k]:.6f}' for k in keys) + f'; worst relative difference to the referee {rel:.3e} (1e-6)')
    assert 3.0 <= m['accuracy'] <= 3.1 and 3.0 <= m['completion'] <= 3.1
    assert m['completion ratio'] == 100.0
    assert m['precision'] == 0.0 and m['recall'] == 0.0 and m['f-score'] == 0.0
    assert rel <= 1e-6 and all(m[k] == ref[k] for k in keys if ref[k] == 0)
    # a mesh against itself: 20 000 independent samples on a 0.25-m square are 320 000 per m^2, so a sample without a partner within 1 cm
    # has probability exp(-320 000 pi 1e-4) per sample
    s = E.metrics_3d(square(0.0, 0.25), square(0.0, 0.25), n_samples=20_000, seed=1, align=False, eng=eng)
    assert s['precision'] == 100.0 and s['recall'] == 100.0 and s['f-score'] == 100.0 and s['completion ratio'] == 100.0
    assert s['accuracy'] < 0.2


# ---------------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize('backend', backends())
def test_align(backend):
    from loopy_slam_amd import mesh_eval as E
    from loopy_slam_amd.loop_closure import se3_exp
    eng = make_engine(backend)
    mesh = fused_mesh(backend)
    v = mesh['vertices'].astype(np.float64)
    c = v.mean(0)
    axis = np.array([0.3, -0.5, 0.8])
    M = se3_exp(np.concatenate([np.deg2rad(0.2) * axis / np.linalg.norm(axis), np.zeros(3)]))
    M[:3, 3] = c - M[:3, :3] @ c + 0.005 * np.array([0.6, 0.0, 0.8])   # 0.2 degrees about the centroid, then 5 mm
    gt = {'vertices': (v @ M[:3, :3].T + M[:3, 3]).astype(np.float32), 'triangles': mesh['triangles']}
    T_ref = R.icp_point_to_point(mesh['vertices'], gt['vertices'])
    ref_err = R.motion_error(T_ref, M)
    out = E.align(mesh, gt, eng=eng)
    err = R.motion_error(out['T'], T_ref)
    print(f'align: {out["iterations"]} iterations, fitness {out["fitness"]:.4f}, rmse {out["inlier_rmse"]:.3e}; to the referee '
          f'{err[0]:.3e} m {err[1]:.3e} rad (1e-4, 1e-4); referee to the planted motion {ref_err[0]:.3e} m {ref_err[1]:.3e} rad')
    assert ref_err[0] <= 1e-4 and ref_err[1] <= 1e-4
    assert err[0] <= 1e-4 and err[1] <= 1e-4
    assert out['fitness'] > 0.99 and abs(np.linalg.det(out['T'][:3, :3]) - 1.0) < 1e-12


# ---------------------------------------------------------------------------------------------------- PLY
def test_read_ply(tmp_path):
    from loopy_slam_amd import mesh_eval as E
    from loopy_slam_amd.tsdf import write_ply
    rng = np.random.RandomState(0)
    mesh = {'vertices': torch.from_numpy(rng.normal(size=(50, 3)).astype(np.float32)), 'colors': torch.from_numpy(rng.rand(50, 3).astype(np.float32)),
            'triangles': torch.from_numpy(rng.randint(0, 50, (80, 3)).astype(np.int32))}
    path = str(tmp_path / 'a.ply')
    write_ply(path, mesh)
    back = E.read_ply(path)
    assert torch.equal(back['vertices'].view(torch.int32), mesh['vertices'].view(torch.int32))
    assert torch.equal(back['triangles'], mesh['triangles']) and back['triangles'].dtype == torch.int32
    as_u8 = lambda c: np.clip(np.rint(c.numpy().astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    assert np.array_equal(as_u8(back['colors']), as_u8(mesh['colors']))
    # ascii, with a normal the reader must skip and a comment
    with open(tmp_path / 'b.ply', 'w') as f:
        f.write('ply\nformat ascii 1.0\ncomment hand-written\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n'
                'property float nx\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n'
                '0 0 0 1\n1 0 0.5 1\n1 1 0 1\n0 1 -2.25 1\n3 0 1 2\n3 0 2 3\n')
    b = E.read_ply(str(tmp_path / 'b.ply'))
    assert np.array_equal(b['vertices'].numpy(), np.array([[0, 0, 0], [1, 0, 0.5], [1, 1, 0], [0, 1, -2.25]], np.float32))
    assert np.array_equal(b['triangles'].numpy(), [[0, 1, 2], [0, 2, 3]]) and 'colors' not in b
    # binary, double positions, uint indices, no colours
    vert = np.zeros(4, dtype=[('p', '<f8', 3)])
    vert['p'] = b['vertices'].numpy()
    face = np.zeros(2, dtype=[('n', 'u1'), ('i', '<u4', 3)])
    face['n'], face['i'] = 3, [[0, 1, 2], [0, 2, 3]]
    head = ('ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty double x\nproperty double y\nproperty double z\n'
            'element face 2\nproperty list uchar uint vertex_indices\nend_header\n')
    with open(tmp_path / 'c.ply', 'wb') as f:
        f.write(head.encode() + vert.tobytes() + face.tobytes())
    c = E.read_ply(str(tmp_path / 'c.ply'))
    assert torch.equal(c['vertices'], b['vertices']) and torch.equal(c['triangles'], b['triangles']) and 'colors' not in c
    # a quad raises, in both encodings
    quad = np.zeros(1, dtype=[('n', 'u1'), ('i', '<u4', 4)])
    quad['n'], quad['i'] = 4, [[0, 1, 2, 3]]
    with open(tmp_path / 'd.ply', 'wb') as f:
        f.write(head.replace('face 2', 'face 1').encode() + vert.tobytes() + quad.tobytes())
    with pytest.raises(ValueError):
        E.read_ply(str(tmp_path / 'd.ply'))
    with open(tmp_path / 'e.ply', 'w') as f:
        f.write('ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n'
                'element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n')
    with pytest.raises(ValueError):
        E.read_ply(str(tmp_path / 'e.ply'))
    with pytest.raises(ValueError):
        E.read_ply(os.path.abspath(__file__))


def test_one_process_only(monkeypatch):
    import torch.distributed as dist
    from loopy_slam_amd import mesh_eval as E
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda *a, **k: 2)
    with pytest.raises(NotImplementedError):
        E.metrics_3d(square(0.0), square(0.0), n_samples=10)
