"""Loop closure above the kernels (loopy_slam_amd/loop_closure.py and its hooks in slam.py): the registration loop against the fp64
NumPy referee of tests/lc_referee.py, the pose graph on planted problems, and the plumbing through NeuralPointCloud / Mapper / Logger.

Registration: max |T - T_planted| of register_pair('robust_icp') is held against the SAME figure of the referee's coarse + Tukey-fine
ICP, computed here on the same clouds with its own fp64 correspondences and normals: at most 2 x it (fp32 sums; correspondences that
fall either side of max_dist between the two precisions)."""
import copy

import numpy as np
import pytest
import torch

import lc_referee as R
import util
from loopy_slam_amd import config, slam, synthetic
from loopy_slam_amd import loop_closure as LC

torch.set_num_threads(1)
_REF = {}


def referee_registration(n, drift):
    """max |T - T_planted| of the fp64 referee (coarse 0.3 m plain, fine 0.03 m Tukey 0.01) and the moved source cloud."""
    key = (n, drift)
    if key not in _REF:
        src0, tgt = R.clouds(n)
        if ('normals', n) not in _REF:
            nrm, cnt, _ = R.normals(tgt, LC.NORMAL_RADIUS, R.CAMERA)
            _REF[('normals', n)] = (nrm, cnt >= 3)
        nrm, valid = _REF[('normals', n)]
        T = R.planted(*R.DRIFTS[drift])
        moved = R.move(src0, R.inv4(T))
        Tc = R.icp(tgt, nrm, valid, moved, np.eye(4), LC.COARSE_DIST)
        Tf = R.icp(tgt, nrm, valid, moved, Tc, LC.FINE_DIST, LC.TUKEY_K)
        _REF[key] = (T, moved, tgt, float(np.abs(Tf - T).max()), float(np.abs(Tc - T).max()))
    return _REF[key]


def check_registration(eng, n):
    figures = []
    for drift in range(len(R.DRIFTS)):
        T, moved, tgt, ref_err, ref_coarse = referee_registration(n, drift)
        sc, tc = LC.SegmentCloud(eng, torch.from_numpy(moved), R.CAMERA), LC.SegmentCloud(eng, torch.from_numpy(tgt), R.CAMERA)
        out = LC.register_pair(sc, tc, 'robust_icp')
        err = float(np.abs(out['T'] - T).max())
        print(f'registration, {n} x {n}, drift {drift}: product {err:.3e} (coarse {np.abs(out["T_coarse"] - T).max():.3e}), '
              f'referee {ref_err:.3e} (coarse {ref_coarse:.3e}), ratio {err / ref_err:.3f}, overlap {out["overlap"]:.3f}, '
              f'fitness {out["fitness"]:.3f}, {out["iterations"]} iterations')
        assert out['success'] and out['overlap'] >= 0.3
        assert err <= 2.0 * ref_err, (err, ref_err)
        assert np.array_equal(out['T'][3], [0, 0, 0, 1])
        plain = LC.register_pair(sc, tc, 'icp')
        assert plain['success'] and np.abs(plain['T'] - T).max() <= 2.0 * ref_coarse        # the plain fine stage only improves on the coarse one
        ident = LC.register_pair(sc, tc, 'identity', adjacent=True)
        assert ident['success'] and np.array_equal(ident['T'], np.eye(4)) and ident['information'][5, 5] > 0
        figures.append((err, ref_err))
        sc.close()
        tc.close()
    return figures


@pytest.mark.parametrize('backend', util.backends())
def test_registration(backend):
    check_registration(util.make_engine(backend), 30000)


@pytest.mark.gpu
def test_registration_at_size_100k():
    check_registration(util.make_engine('hip'), 100000)


@pytest.mark.parametrize('backend', util.backends())
def test_registration_failure_rule(backend):
    eng = util.make_engine(backend)
    src0, tgt = R.clouds(30000)
    far = LC.SegmentCloud(eng, torch.from_numpy(src0[:5000] + np.float32(50.0)), R.CAMERA)
    tc = LC.SegmentCloud(eng, torch.from_numpy(tgt), R.CAMERA)
    for method in ('icp', 'robust_icp', 'identity'):
        out = LC.register_pair(far, tc, method)
        assert not out['success'] and np.array_equal(out['T'], np.eye(4)) and np.array_equal(out['information'], np.eye(6))
    with pytest.raises(NotImplementedError):
        LC.register_pair(far, tc, 'colored_icp')


# ------------------------------------------------------------------------------------------------ pose graph (host only)
def _planted_graph(seed=0, n=6):
    rng = np.random.RandomState(seed)
    X = [np.eye(4)] + [R.planted(rng.uniform(-2, 2, 3), rng.uniform(-0.05, 0.05, 3)) for _ in range(n - 1)]
    pts = rng.uniform(-3, 3, (1000, 3))
    L = R.info_sums(pts, np.arange(1000), np.zeros(1000))
    Lm = np.zeros((6, 6))
    Lm[np.triu_indices(6)] = L[:21]
    Lm = Lm + np.triu(Lm, 1).T

    def edge(s, t, unc):
        return (s, t, R.inv4(X[t]) @ X[s], Lm, unc)
    edges = [edge(i, i + 1, False) for i in range(n - 1)] + [edge(5, 0, True), edge(4, 1, True), edge(3, 0, True)]
    return X, edges, Lm


def test_se3_exp_log():
    rng = np.random.RandomState(1)
    for _ in range(20):
        x = np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-2, 2, 3)])
        assert np.abs(LC.se3_log(LC.se3_exp(x)) - x).max() < 1e-12
    assert np.abs(LC.se3_exp(np.zeros(6)) - np.eye(4)).max() == 0


def test_pose_graph_recovers_planted_corrections():
    X, edges, _ = _planted_graph()
    out = LC.optimize_pose_graph(6, edges, prune=0.25, lc_pref=5.0, max_dist=0.03)
    err = max(np.abs(out['nodes'][i] - X[i]).max() for i in range(6))
    print('pose graph: worst |X - X_planted|', err, 'mu', out['mu'])
    assert err <= 1e-6 and out['kept'].all()
    assert np.array_equal(out['nodes'][0], np.eye(4))


def test_pose_graph_prunes_a_wrong_loop_edge():
    X, edges, Lm = _planted_graph()
    wrong = R.inv4(X[0]) @ X[2]
    wrong[:3, 3] += [0.5, 0.0, 0.0]
    edges = edges + [(2, 0, wrong, Lm, True)]
    out = LC.optimize_pose_graph(6, edges, prune=0.25, lc_pref=5.0, max_dist=0.03)
    assert out['weights'][-1] < 0.25 and not out['kept'][-1] and out['kept'][:-1].all()
    err = max(np.abs(out['nodes'][i] - X[i]).max() for i in range(6))
    print('pose graph with a wrong edge: its weight', out['weights'][-1], 'worst |X - X_planted|', err)
    assert err <= 1e-6


# ------------------------------------------------------------------------------------------------ through the classes
def small_cfg():
    """configs/Synthetic/room.yaml at the reduced image and work budget of tests/test_slam_api.py."""
    cfg = copy.deepcopy(config.load_config('configs/Synthetic/room.yaml', 'configs/point_slam.yaml'))
    cfg['cam'].update(H=24, W=32, fx=26.0, fy=26.0, cx=15.5, cy=11.5)
    cfg['tracking'].update(ignore_edge_W=2, ignore_edge_H=2, pixels=48, iters=3)
    cfg['mapping'].update(pixels=64, pixels_adding=400, iters=3, iters_first=6, geo_iter_first=2, every_frame=2, keyframe_every=2,
                          mapping_window_size=4)
    cfg['pointcloud'].update(radius_add=0.12, radius_query=0.24, radius_min=0.06)
    cfg['data']['n_frames'] = 40
    return cfg


SEG_POSES, SEG_STARTS, RAYS = (0, 100, 25, 3), (0, 10, 20, 30), 20000
# the points of a segment are laid down through a wide virtual camera (116 x 100 degrees): a segment then holds two or three walls with
# floor and ceiling - one wall alone leaves point-to-plane ICP free to slide along it
WIDE = dict(H=24, W=32, fx=10.0, fy=10.0, cx=15.5, cy=11.5)


def four_segment_map(eng, candidates):
    """A map of four segments laid down from true poses (segment 3 looks at what segment 0 saw), then segments 2 and 3 - points and
    cameras - displaced by one planted drift.  Returns (slam object, drift 4 x 4, undisplaced positions)."""
    cfg = small_cfg()
    cfg['loop_closure'] = {'enabled': True, 'method': 'robust_icp', 'candidates': candidates}
    ps = slam.Point_SLAM(cfg, None, eng=eng)
    npc, mapper = ps.npc, ps.mapper
    assert mapper.closer is not None and npc._seg is not None
    intr = dict(H=24, W=32, fx=26.0, fy=26.0, cx=15.5, cy=11.5)
    D = R.planted(*R.DRIFTS[0])
    g = torch.Generator().manual_seed(11)
    true_pos, seg_ids = [], []
    for s, k in enumerate(SEG_POSES):
        c2w = synthetic.loop_pose(k)
        i, j = torch.rand(RAYS, generator=g) * 31, torch.rand(RAYS, generator=g) * 23
        ro, rd = synthetic.pixel_rays(c2w, i, j, WIDE)
        d = synthetic.room_depth(ro, rd)
        pts = (ro + rd * d[:, None]).float()              # on the surface: one point per ray
        true_pos.append(pts)
        seg_ids.append(torch.full((pts.shape[0],), s, dtype=torch.int32))
    true_pos, seg_ids = torch.cat(true_pos).numpy(), torch.cat(seg_ids)
    moved = np.where((seg_ids.numpy() >= 2)[:, None], R.move(true_pos, D), true_pos).astype(np.float32)
    n = len(moved)
    npc._grow(n)
    npc._pos[:n] = eng.f32(moved)
    npc._seg[:n] = seg_ids.to(eng.device)
    npc._geo[:n] = 0.1 * torch.randn(n, 32, generator=g).to(eng.device)
    npc._col[:n] = 0.1 * torch.randn(n, 32, generator=g).to(eng.device)
    npc.n = n
    npc.knn.build(npc._pos[:n])
    Dt = torch.from_numpy(D).float()
    for s, k in enumerate(SEG_POSES):
        c2w = synthetic.loop_pose(k)
        est = (Dt @ c2w) if s >= 2 else c2w.clone()
        depth, color, _ = synthetic.render_frame(k, intr=intr, holes=0.0)
        rec = {'idx': SEG_STARTS[s], 'color': color.to(eng.device), 'depth': depth.to(eng.device), 'est_c2w': est.to(eng.device),
               'gt_c2w': c2w.to(eng.device), 'r2_query': None, 'exposure_feat': None}
        mapper.segments.append(rec)
        for f in (SEG_STARTS[s], SEG_STARTS[s] + 4):
            mapper.keyframe_list.append(f)
            mapper.keyframe_dict.append({'idx': f, 'est_c2w': est.to(eng.device).clone(), 'gt_c2w': c2w.to(eng.device), 'color': rec['color'],
                                         'depth': rec['depth'], 'r2_query': None, 'exposure_feat': None})
        end = SEG_STARTS[s + 1] if s + 1 < 4 else SEG_STARTS[s] + 1
        ps.estimate_c2w_list[SEG_STARTS[s]:end] = est
    return ps, D, true_pos


@pytest.mark.parametrize('backend', util.backends())
def test_closure_through_the_classes(backend):
    eng = util.make_engine(backend)
    ps, D, true_pos = four_segment_map(eng, lambda segments: [(3, 0)])
    npc, mapper, closer = ps.npc, ps.mapper, ps.mapper.closer
    n = npc.n
    seg = npc._seg[:n].cpu().numpy()
    old_pos = npc._pos[:n].cpu().numpy().copy()
    old_list = ps.estimate_c2w_list.clone()
    old_seg = [s['est_c2w'].cpu().clone() for s in mapper.segments]
    old_kf = [k['est_c2w'].cpu().clone() for k in mapper.keyframe_dict]
    pg = closer.on_new_segment(mapper, n)
    assert pg is not None and closer.last_registrations[0]['success']
    # the node matrices are what optimize_pose_graph returns for the edges the closer reports
    again = LC.optimize_pose_graph(4, closer.last_edges, prune=closer.prune_pgo, lc_pref=closer.lc_pref, max_dist=LC.FINE_DIST)
    X = pg['nodes']
    assert np.array_equal(X, again['nodes'])
    assert [(e[0], e[1], e[4]) for e in closer.last_edges] == [(0, 1, False), (1, 2, False), (2, 3, False), (3, 0, True)]
    assert all(np.array_equal(e[2], np.eye(4)) for e in closer.last_edges[:3])
    new_pos = npc._pos[:n].cpu().numpy()
    X32 = X[:, :3, :4].astype(np.float32).astype(np.float64)
    for s in range(4):
        rows = seg == s
        ref = old_pos[rows].astype(np.float64) @ X32[s][:, :3].T + X32[s][:, 3]
        assert np.abs(new_pos[rows] - ref).max() <= 5e-6, s
    assert new_pos[seg == 0].tobytes() == old_pos[seg == 0].tobytes() and np.array_equal(X[0], np.eye(4))

    def moved(Xs, c2w):
        out = torch.from_numpy(Xs) @ c2w.double()
        out[3] = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)
        return out.to(c2w.dtype)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0])
    for s in range(4):
        assert torch.equal(mapper.segments[s]['est_c2w'].cpu(), moved(X[s], old_seg[s]))
        assert torch.equal(mapper.segments[s]['est_c2w'].cpu()[3], bottom)
        a, b = SEG_STARTS[s], (SEG_STARTS[s + 1] if s + 1 < 4 else SEG_STARTS[s] + 1)
        for f in range(a, b):
            assert torch.equal(ps.estimate_c2w_list[f], moved(X[s], old_list[f])), f
    assert torch.equal(ps.estimate_c2w_list[SEG_STARTS[3] + 1:], old_list[SEG_STARTS[3] + 1:])         # frames not tracked yet
    for kf, old in zip(mapper.keyframe_dict, old_kf):
        s = max(i for i in range(4) if SEG_STARTS[i] <= kf['idx'])
        assert torch.equal(kf['est_c2w'].cpu(), moved(X[s], old))
    rows3 = seg == 3
    before = np.linalg.norm(old_pos[rows3] - true_pos[rows3], axis=1).mean()
    after = np.linalg.norm(new_pos[rows3] - true_pos[rows3], axis=1).mean()
    print(f'segment 3, mean distance to the undisplaced positions: {before:.4e} m before, {after:.4e} m after the closure')
    assert after < before
    # the live index is the corrected cloud's: a render of segment 3's keyframe runs on it
    depth, _, _ = ps.renderer_map.render_img(npc, ps.shared_decoders, mapper.segments[3]['est_c2w'], eng.device, 'color',
                                             gt_depth=mapper.segments[3]['depth'])
    assert torch.isfinite(depth).all()
    fresh = LC.core.KnnIndex(eng, capacity=n, cell_size=npc._cell)
    fresh.build(npc._pos[:n].clone())
    q = npc._pos[:2000] + 0.01
    for x, y in zip(npc.knn.query(q, 0.08 ** 2), fresh.query(q, 0.08 ** 2)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    # the checkpoint's fragments
    frags = closer.fragments(mapper.segments)
    assert [f['start_idx'] for f in frags] == list(SEG_STARTS) and all(f['n_points'] == RAYS for f in frags)
    assert np.array_equal(frags[3]['correction'].numpy(), X[3])
    # the forwarding names of NeuralPointCloud
    assert npc.compute_correction.__self__ is npc and npc.apply_correction.__self__ is npc


@pytest.mark.parametrize('backend', util.backends())
def test_failed_pair_changes_nothing(backend):
    eng = util.make_engine(backend)
    ps, _, _ = four_segment_map(eng, lambda segments: [(3, 1)])          # segment 1 looks at another wall
    npc, mapper = ps.npc, ps.mapper
    pos, lst = npc._pos[:npc.n].clone(), ps.estimate_c2w_list.clone()
    segs = [s['est_c2w'].clone() for s in mapper.segments]
    kfs = [k['est_c2w'].clone() for k in mapper.keyframe_dict]
    assert mapper.closer.on_new_segment(mapper, npc.n) is None
    assert not mapper.closer.last_registrations[0]['success']
    assert torch.equal(pos, npc._pos[:npc.n]) and torch.equal(lst, ps.estimate_c2w_list)
    assert all(torch.equal(a, s['est_c2w']) for a, s in zip(segs, mapper.segments))
    assert all(torch.equal(a, k['est_c2w']) for a, k in zip(kfs, mapper.keyframe_dict))
    assert mapper.closer.fragments(mapper.segments)[3]['correction'].equal(torch.eye(4, dtype=torch.float64))


@pytest.mark.parametrize('backend', util.backends())
def test_off_switch(backend):
    """Key absent and enabled: False give the same bits after ten frames, and neither allocates the id buffer.  On the chip this is
    configs/Synthetic/room.yaml as it stands; on the host emulator the same config at the reduced budget of small_cfg()."""
    eng = util.make_engine(backend)
    states = []
    for lc in (None, {'enabled': False}):
        cfg = copy.deepcopy(config.load_config('configs/Synthetic/room.yaml', 'configs/point_slam.yaml')) if backend == 'hip' else small_cfg()
        cfg['data']['n_frames'] = 10
        cfg.pop('loop_closure', None)
        if lc is not None:
            cfg['loop_closure'] = lc
        ps = slam.Point_SLAM(cfg, None, eng=eng)
        ps.run()
        assert ps.mapper.closer is None and ps.npc.closer is None and ps.npc._seg is None
        states.append((ps.npc._pos[:ps.npc.n].clone(), ps.npc._geo[:ps.npc.n].clone(), ps.npc._col[:ps.npc.n].clone(),
                       ps.estimate_c2w_list.clone(), torch.stack([s['est_c2w'].cpu() for s in ps.mapper.segments]),
                       list(ps.mapper.keyframe_list)))
    for a, b in zip(*states):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b


@pytest.mark.parametrize('backend', util.backends())
def test_mapper_runs_with_closure_on(backend):
    """A short run with the feature on: every row carries a segment id, the checkpoint lists the fragments."""
    import tempfile
    eng = util.make_engine(backend)
    cfg = small_cfg()
    cfg['data']['n_frames'] = 6
    cfg['mapping'].update(segment_strategy='fixed', fixed_segment_size=2)
    cfg['loop_closure'] = {'enabled': True}
    ps = slam.Point_SLAM(cfg, None, eng=eng)
    ps.run()
    npc, mapper = ps.npc, ps.mapper
    assert len(mapper.segments) == 3
    seg = npc._seg[:npc.n].cpu().numpy()
    # (a frame that opens a segment may insert nothing: the last segment can be empty)
    assert seg.min() == 0 and 1 <= seg.max() <= 2 and (np.diff(seg) >= 0).all()
    with tempfile.TemporaryDirectory() as d:
        ck = torch.load(slam.Logger(cfg, None, mapper, ckptsdir=d).log(5, mapper.keyframe_dict, mapper.keyframe_list, npc=npc, last_log=True),
                        map_location='cpu', weights_only=False)
    assert [f['start_idx'] for f in ck['fragments']] == [0, 2, 4]
    assert sum(f['n_points'] for f in ck['fragments']) == npc.n
    assert all(set(f) == {'start_idx', 'keyframe', 'n_points', 'correction'} for f in ck['fragments'])


def test_refuses_several_ranks():
    class Dist:
        rank, world = 0, 2

    class Npc:
        pass
    with pytest.raises(NotImplementedError, match='world > 1'):
        LC.LoopCloser({'loop_closure': {'enabled': True}}, Npc(), slam=type('S', (), {'dist': Dist()})())
