"""'fpfh_robust_icp' above its kernels: register_pair end to end against the fp64 referee, the untouched 'robust_icp', and a closure through
LoopCloser on a map whose drift is far outside the ICP basin.

End to end: the furnished-room pair of tests/greg_referee.py, planted (40, -25, 70) degrees, (1.2, -0.8, 0.4) m (its docstring says why not
the smaller transform).  max |T - T_planted| of register_pair(.., 'fpfh_robust_icp') is at most 2 x the same figure of the referee's
coarse + Tukey-fine ICP started from the referee's own RANSAC result - the margin of tests/test_loop_closure.py and its reason (fp32 sums;
correspondences that fall either side of max_dist between the two precisions).  Measured on the emulator: product 1.483e-03, referee
1.484e-03, ratio 0.999.  On the same pair 'robust_icp' from the identity fails its success rule (no correspondence within 0.3 m enters
the sums: it stays at the identity, 1.2 m from the planted transform), as the referee's ICP from the identity does.
Small drift: 'robust_icp' on lc_referee.clouds returns the bits the parent commit returned (tests/golden/lc_robust_icp_parent_emu.npz,
recorded by running the parent's library and package on the emulator).  On the chip the parent's own bits are not reproducible from one
index build to the next (lk_normals sums in the cell order that lk_knn_build's counting atomics leave: loopy_hip.h), so the hip case is
held against the same record within 1e-5 per entry of T - a sixth of the registration's own error of 6e-5, and what one Gauss-Newton
iteration more or less moves at the stopping rule (fitness and rmse changing by less than 1e-6) - and 1e-3 relative on the information.
Through the classes: four segments of the furnished room, segments 2 and 3 displaced by the large transform; with 'fpfh_robust_icp' the
closure brings segment 3 back to within 1 cm (mean distance to the undisplaced positions), with 'robust_icp' it does not.
At size (-m gpu): the same pair at 100 000 points per segment; a denser sample of the same surfaces does not raise the ICP's bias, so the
bound is 2 x the referee's figure at 30 000 points."""
import os

import numpy as np
import pytest
import torch

import greg_referee as G
import lc_referee as R
import test_loop_closure as TLC
import util
from loopy_slam_amd import loop_closure as LC
from loopy_slam_amd import slam, synthetic

torch.set_num_threads(1)


def referee_error(pair):
    ref = G.global_registration(pair, 0)
    return float(np.abs(G.refine(pair, ref['ransac']['T']) - pair['T']).max()), ref


def segments(eng, pair):
    return (LC.SegmentCloud(eng, torch.from_numpy(pair['src']), pair['cam_s']), LC.SegmentCloud(eng, torch.from_numpy(pair['tgt']), pair['cam_t']))


@pytest.mark.parametrize('backend', util.backends())
def test_end_to_end(backend):
    eng = util.make_engine(backend)
    pair = G.segment_pair()
    ref_err, ref = referee_error(pair)
    ss, st = segments(eng, pair)
    out = LC.register_pair(ss, st, 'fpfh_robust_icp', eng=eng)
    err = float(np.abs(out['T'] - pair['T']).max())
    deg, m = G.pose_error(out['T_global'], pair['T'])
    print(f'end to end: product {err:.3e}, referee {ref_err:.3e}, ratio {err / ref_err:.3f}; global start {deg:.2f} degrees, {m:.3f} m off with '
          f'{out["global_inliers"]} inliers after {out["global_trials"]} trials (referee: {ref["best_error"][0]:.2f} degrees, '
          f'{ref["best_error"][1]:.3f} m, {ref["ransac"]["inliers"]} inliers, mutual inlier ratio {ref["inlier_ratio"]:.3f}); '
          f'overlap {out["overlap"]:.3f}')
    assert out['success'] and out['global_ok'] and out['overlap'] >= 0.3
    assert err <= 2.0 * ref_err, (err, ref_err)
    assert np.array_equal(out['T'][3], [0, 0, 0, 1])
    plain = LC.register_pair(ss, st, 'robust_icp', eng=eng)
    print(f'   robust_icp from the identity: success {plain["success"]}, max |T - T_planted| = {np.abs(plain["T"] - pair["T"]).max():.3f}')
    assert (not plain['success']) or np.abs(plain['T'] - pair['T']).max() > 0.1
    assert 'T_global' not in plain


@pytest.mark.parametrize('backend', util.backends())
def test_small_drift_keeps_the_parents_bits(backend):
    eng = util.make_engine(backend)
    gold = util.load('lc_robust_icp_parent_emu')
    src0, tgt = R.clouds(30000)
    for i, drift in enumerate(R.DRIFTS):
        moved = R.move(src0, R.inv4(R.planted(*drift)))
        sc, tc = LC.SegmentCloud(eng, torch.from_numpy(moved), R.CAMERA), LC.SegmentCloud(eng, torch.from_numpy(tgt), R.CAMERA)
        out = LC.register_pair(sc, tc, 'robust_icp')
        if backend == 'emu':
            assert out['T'].tobytes() == gold[f'T{i}'].tobytes() and out['information'].tobytes() == gold[f'information{i}'].tobytes()
            assert out['iterations'] == int(gold[f'iterations{i}'])
        else:
            dT = float(np.abs(out['T'] - gold[f'T{i}']).max())
            dI = float(np.abs(out['information'] - gold[f'information{i}']).max() / np.abs(gold[f'information{i}']).max())
            print(f'small drift {i}: max |T - T_parent| = {dT:.2e}, information {dI:.2e} relative, {out["iterations"]} iterations '
                  f'(parent on the emulator: {int(gold[f"iterations{i}"])})')
            assert dT <= 1e-5 and dI <= 1e-3
        sc.close()
        tc.close()
    assert LC.DEFAULTS['method'] == 'robust_icp' and LC.METHODS[:3] == ('identity', 'icp', 'robust_icp')


# ------------------------------------------------------------------------------------------------ through the classes
RAYS = 30000


def furnished_four_segment_map(eng, method):
    """tests/test_loop_closure.py's four_segment_map in the furnished room: four segments laid down from true poses through the wide virtual
    camera (segment 3 looks at what segment 0 saw), segments 2 and 3 - points and cameras - displaced by the large planted transform."""
    cfg = TLC.small_cfg()
    cfg['loop_closure'] = {'enabled': True, 'method': method, 'candidates': lambda segments: [(3, 0)], 'global_seed': 0}
    ps = slam.Point_SLAM(cfg, None, eng=eng)
    npc, mapper = ps.npc, ps.mapper
    intr = dict(H=24, W=32, fx=26.0, fy=26.0, cx=15.5, cy=11.5)
    D = R.planted(*G.PLANTED)
    g = torch.Generator().manual_seed(11)
    true_pos, seg_ids = [], []
    for s, k in enumerate(TLC.SEG_POSES):
        c2w = synthetic.loop_pose(k)
        i, j = torch.rand(RAYS, generator=g) * 31, torch.rand(RAYS, generator=g) * 23
        ro, rd = synthetic.pixel_rays(c2w, i, j, TLC.WIDE)
        d, _ = synthetic.furnished_hit(ro, rd)
        true_pos.append((ro + rd * d[:, None]).float())
        seg_ids.append(torch.full((RAYS,), s, dtype=torch.int32))
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
    for s, k in enumerate(TLC.SEG_POSES):
        c2w = synthetic.loop_pose(k)
        est = (Dt @ c2w) if s >= 2 else c2w.clone()
        depth, color, _ = synthetic.render_frame(k, intr=intr, holes=0.0, scene='furnished')
        rec = {'idx': TLC.SEG_STARTS[s], 'color': color.to(eng.device), 'depth': depth.to(eng.device), 'est_c2w': est.to(eng.device),
               'gt_c2w': c2w.to(eng.device), 'r2_query': None, 'exposure_feat': None}
        mapper.segments.append(rec)
        mapper.keyframe_list.append(TLC.SEG_STARTS[s])
        mapper.keyframe_dict.append({'idx': TLC.SEG_STARTS[s], 'est_c2w': est.to(eng.device).clone(), 'gt_c2w': c2w.to(eng.device),
                                     'color': rec['color'], 'depth': rec['depth'], 'r2_query': None, 'exposure_feat': None})
        end = TLC.SEG_STARTS[s + 1] if s + 1 < 4 else TLC.SEG_STARTS[s] + 1
        ps.estimate_c2w_list[TLC.SEG_STARTS[s]:end] = est
    return ps, true_pos


@pytest.mark.parametrize('backend', util.backends())
def test_closure_through_the_classes(backend):
    eng = util.make_engine(backend)
    after = {}
    for method in ('fpfh_robust_icp', 'robust_icp'):
        ps, true_pos = furnished_four_segment_map(eng, method)
        npc, mapper, closer = ps.npc, ps.mapper, ps.mapper.closer
        assert closer.method == method and closer.global_cfg == {'conf': LC.GLOBAL_CONF, 'max_iter': LC.GLOBAL_ITER, 'seed': 0}
        n = npc.n
        rows3 = npc._seg[:n].cpu().numpy() == 3
        before = np.linalg.norm(npc._pos[:n].cpu().numpy()[rows3] - true_pos[rows3], axis=1).mean()
        pg = closer.on_new_segment(mapper, n)
        after[method] = np.linalg.norm(npc._pos[:n].cpu().numpy()[rows3] - true_pos[rows3], axis=1).mean()
        reg = closer.last_registrations[0]
        print(f'{method}: registration success {reg["success"]}, segment 3 mean distance to the undisplaced positions {before:.3f} m before, '
              f'{after[method]:.4e} m after')
        if method == 'fpfh_robust_icp':
            assert pg is not None and reg['success'] and reg['global_ok'] and reg['global_trials'] > 0
        else:
            assert pg is None and not reg['success']
    assert after['fpfh_robust_icp'] < 0.01
    assert not after['robust_icp'] < 0.01


def test_config_rejects_an_unknown_method():
    class Npc:
        eng, capacity, closer, _seg = type('E', (), {'device': torch.device('cpu')})(), 4, None, None
    with pytest.raises(NotImplementedError):
        LC.LoopCloser({'loop_closure': {'enabled': True, 'method': 'fpfh_icp'}}, Npc())
    assert LC.LoopCloser({'loop_closure': {'enabled': True, 'method': 'fpfh_robust_icp', 'global_iter': 1000, 'global_seed': 7}}, Npc()).global_cfg == \
        {'conf': LC.GLOBAL_CONF, 'max_iter': 1000, 'seed': 7}


@pytest.mark.gpu
def test_at_size_100k():
    eng = util.make_engine('hip')
    ref_err, _ = referee_error(G.segment_pair())
    pair = G.segment_pair(100000)
    ss, st = segments(eng, pair)
    out = LC.register_pair(ss, st, 'fpfh_robust_icp', eng=eng)
    err = float(np.abs(out['T'] - pair['T']).max())
    f = ss.features()
    print(f'at size: 100 000 points per segment -> {len(f["pos"])} voxels, {out["global_inliers"]} inliers after {out["global_trials"]} trials, '
          f'product {err:.3e} (bound {2.0 * ref_err:.3e}), overlap {out["overlap"]:.3f}')
    assert out['success'] and out['global_ok'] and out['overlap'] >= 0.3
    assert err <= 2.0 * ref_err
