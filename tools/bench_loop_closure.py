#!/usr/bin/env python3
"""Timing of the loop-closure back end on one MI355X (loopy_slam_amd/loop_closure.py, csrc/lk_reg.hip): normals, one coarse + fine
registration, the information matrix, correction + index rebuild, at 30 k / 100 k / 1 M points per cloud; with --global also the stages of
the global start (csrc/lk_greg.hip) on a furnished-room pair under a large planted transform: voxel downsample, FPFH (normals included),
the two-way feature match, RANSAC per 65 536 trials and register_pair 'fpfh_robust_icp' end to end.

Every figure is the wall time of the whole call including its host synchronisations (an ICP iteration ends in one small copy), warm, the
median of `--repeats` runs.  --referee also times the fp64 NumPy referee of tests/lc_referee.py on the host for the two smaller sizes: the
reference's own stage needs Open3D and cannot run here, so this is the only context there is.

    python tools/bench_loop_closure.py [--sizes 30000 100000 1000000] [--repeats 5] [--referee] [--global [--global-sizes 30000 100000]]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from loopy_slam_amd import core, synthetic
from loopy_slam_amd import loop_closure as LC
from loopy_slam_amd._ffi import ptr


def planted():
    T = np.eye(4)
    T[:3, :3] = LC.se3_exp(np.concatenate([np.deg2rad([0.6, -0.5, 0.7]), np.zeros(3)]))[:3, :3]
    T[:3, 3] = (0.02, -0.015, 0.01)
    return T


def clouds(n):
    src, tgt = synthetic.overlapping_pair(n, seed=5)
    T = planted()
    src = (src.astype(np.float64) - T[:3, 3]) @ T[:3, :3]              # moved by the inverse of the planted transform
    return np.ascontiguousarray(src.astype(np.float32)), tgt, T


GLOBAL_PLANTED = ((40.0, -25.0, 70.0), (1.2, -0.8, 0.4))       # degrees, metres: outside the 0.3-m ICP basin


def furnished_pair(n):
    """Two n-point clouds of the furnished room from loop poses 0, 3, 6, 9 and 5, 8, 11, 14 (three points per ray), the first moved by the
    inverse of GLOBAL_PLANTED: (source, target, planted 4 x 4, source camera, target camera)."""
    src, cam_s = synthetic.furnished_cloud((0, 3, 6, 9), n, 101)
    tgt, cam_t = synthetic.furnished_cloud((5, 8, 11, 14), n, 202)
    T = LC.se3_exp(np.concatenate([np.deg2rad(GLOBAL_PLANTED[0]), np.zeros(3)]))
    T[:3, 3] = GLOBAL_PLANTED[1]
    src = ((src.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    return np.ascontiguousarray(src), tgt, T, (cam_s - T[:3, 3]) @ T[:3, :3], cam_t


def global_rows(eng, n, repeats, sync):
    src, tgt, T, cam_s, cam_t = furnished_pair(n)
    ps, pt = eng.f32(src), eng.f32(tgt)
    fs, ft = LC.fpfh_features(eng, ps, cam_s), LC.fpfh_features(eng, pt, cam_t)
    corr = LC.mutual_matches(eng, fs, ft)
    M = int(corr.shape[0])
    cs, ct = LC.ransac_gather(eng, fs['pos'], ft['pos'], corr)
    best = LC.ransac_best_init(eng)

    def batch():
        LC.ransac_fold(eng, LC.ransac_batch(eng, cs, ct, 0, 0, LC.RANSAC_BATCH, 1.5 * LC.VOXEL), 0, best)
        best.cpu()
    res = {}

    def end_to_end():
        sc, tc = LC.SegmentCloud(eng, ps, cam_s), LC.SegmentCloud(eng, pt, cam_t)         # fresh clouds: nothing cached
        res.update(LC.register_pair(sc, tc, 'fpfh_robust_icp'))
        sc.close(); tc.close()
    ns, nt = len(fs['pos']), len(ft['pos'])
    return [
        (n, f'voxel downsample 0.04 m (-> {ns:,} voxels)', timed(lambda: LC.voxel_downsample(eng, ps), repeats, sync), ''),
        (n, 'fpfh_features: downsample + index + lk_normals 0.08 m + lk_fpfh 0.2 m', timed(lambda: LC.fpfh_features(eng, ps, cam_s), repeats, sync), ''),
        (n, f'lk_fpfh alone incl. its index ({ns:,} points)', timed(lambda: LC.fpfh(eng, fs['pos'], fs['normals'], fs['valid'], 5 * LC.VOXEL), repeats, sync), ''),
        (n, f'mutual_matches: lk_feature_match both ways ({ns:,} x {nt:,})', timed(lambda: LC.mutual_matches(eng, fs, ft), repeats, sync), f'{M} mutual pairs'),
        (n, 'RANSAC, one batch of 65 536 trials (hypotheses + compact + score + best + read-back)', timed(batch, repeats, sync), ''),
        (n, "register_pair 'fpfh_robust_icp' end to end, fresh clouds", timed(end_to_end, repeats, sync),
         f"{res['global_trials']} trials, {res['global_inliers']} inliers, {res['iterations']} ICP iterations, max abs (T - planted) {np.abs(res['T'] - T).max():.1e}"),
    ]


def timed(fn, repeats, sync):
    fn()
    sync()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[30000, 100000, 1000000])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--referee', action='store_true')
    ap.add_argument('--global', dest='glob', action='store_true', help="time the stages of 'fpfh_robust_icp' instead")
    ap.add_argument('--global-sizes', type=int, nargs='+', default=[30000, 100000])
    args = ap.parse_args()
    eng = core.Engine()
    sync = torch.cuda.synchronize
    rows = []
    if args.glob:
        args.sizes = []
        for n in args.global_sizes:
            rows += global_rows(eng, n, args.repeats, sync)
    for n in args.sizes:
        src, tgt, T = clouds(n)
        sc, tc = LC.SegmentCloud(eng, torch.from_numpy(src), (0, 0, 0)), LC.SegmentCloud(eng, torch.from_numpy(tgt), (0, 0, 0))
        tc.knn, sc.knn
        rows.append((n, 'index build (0.1-m cells)', timed(lambda: tc.knn.build(tc.pos), args.repeats, sync), ''))
        rows.append((n, 'lk_normals (radius 0.1 m)', timed(lambda: LC.estimate_normals(eng, tc.pos, knn=tc.knn), args.repeats, sync), ''))
        tc.normals
        rows.append((n, 'lk_icp_accumulate, one step, 0.3 m', timed(lambda: LC.icp_sums(eng, tc, sc.pos, np.eye(4), 0.3), args.repeats, sync), ''))
        rows.append((n, 'lk_icp_accumulate, one step, 0.03 m Tukey', timed(lambda: LC.icp_sums(eng, tc, sc.pos, T, 0.03, 0.01), args.repeats, sync), ''))
        res = {}
        rows.append((n, "register_pair 'robust_icp' (coarse + fine + information)",
                     timed(lambda: res.update(LC.register_pair(sc, tc, 'robust_icp')), args.repeats, sync), ''))
        rows[-1] = rows[-1][:3] + (f"{res['iterations']} iterations, max abs (T - planted) {np.abs(res['T'] - T).max():.1e}",)
        rows.append((n, 'information matrix (0.03 m)', timed(lambda: LC.information_matrix(eng, sc, tc, T), args.repeats, sync), ''))
        # correction + rebuild over a map of the two clouds (2 n points, two segments, one of them moved)
        pos = torch.cat([sc.pos, tc.pos]).contiguous()
        seg = torch.cat([torch.zeros(n, dtype=torch.int32), torch.ones(n, dtype=torch.int32)]).to(eng.device)
        mats = torch.from_numpy(np.stack([np.eye(4), T])[:, :3, :4].astype(np.float32).reshape(2, 12)).to(eng.device)
        live = core.KnnIndex(eng, capacity=2 * n)
        live.build(pos)

        def correct():
            eng.lib.check(eng.lib.dll.lk_apply_correction(ptr(pos), 2 * n, ptr(seg), ptr(mats), 2, eng.stream), 'lk_apply_correction')
            live.build(pos)
        rows.append((n, f'lk_apply_correction + lk_knn_build ({2 * n:,} points)', timed(correct, args.repeats, sync), ''))
        live.close(); sc.close(); tc.close()
        if args.referee and n <= 100000:
            sys.path.insert(0, os.path.join(ROOT, 'tests'))
            import lc_referee as R
            t0 = time.perf_counter(); nrm, cnt, _ = R.normals(tgt, 0.1, (0, 0, 0)); t_n = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            Tc = R.icp(tgt, nrm, cnt >= 3, src, np.eye(4), 0.3)
            R.icp(tgt, nrm, cnt >= 3, src, Tc, 0.03, 0.01)
            t_r = (time.perf_counter() - t0) * 1e3
            rows.append((n, 'fp64 NumPy referee on the host: normals', (t_n, t_n, t_n), 'one run'))
            rows.append((n, 'fp64 NumPy referee on the host: coarse + fine ICP', (t_r, t_r, t_r), 'one run'))
    print('| points per cloud | stage | median ms | min .. max ms | note |')
    print('|---|---|---|---|---|')
    for n, name, (med, lo, hi), note in rows:
        print(f'| {n:,} | {name} | {med:.2f} | {lo:.2f} .. {hi:.2f} | {note} |')


if __name__ == '__main__':
    main()
