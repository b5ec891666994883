#!/usr/bin/env python3
"""Timing of the loop-closure back end on one MI355X (loopy_slam_amd/loop_closure.py, csrc/lk_reg.hip): normals, one coarse + fine
registration, the information matrix, correction + index rebuild, at 30 k / 100 k / 1 M points per cloud.

Every figure is the wall time of the whole call including its host synchronisations (an ICP iteration ends in one small copy), warm, the
median of `--repeats` runs.  --referee also times the fp64 NumPy referee of tests/lc_referee.py on the host for the two smaller sizes: the
reference's own stage needs Open3D and cannot run here, so this is the only context there is.

    python tools/bench_loop_closure.py [--sizes 30000 100000 1000000] [--repeats 5] [--referee]
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
    pos = synthetic.build_cloud(2 * n, seed=5)[0].numpy()
    pos = pos[np.random.RandomState(0).permutation(len(pos))]
    a = (2 * n) // 3
    T = planted()
    src = (pos[:n].astype(np.float64) - T[:3, 3]) @ T[:3, :3]          # moved by the inverse of the planted transform
    return np.ascontiguousarray(src.astype(np.float32)), np.ascontiguousarray(pos[a:a + n]), T


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
    args = ap.parse_args()
    eng = core.Engine()
    sync = torch.cuda.synchronize
    rows = []
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
