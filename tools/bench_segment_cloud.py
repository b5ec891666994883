#!/usr/bin/env python3
"""Timing of loop closure's per-segment surface clouds on one MI355X (loop_closure.cloud = 'tsdf': tsdf.fuse_segment, TSDFVolume.
extract_point_cloud, csrc/lk_normals_nn.hip): two segments of `--frames` frames each of the furnished synthetic room's loop at 640 x 480, fused
at the reference's resolution (voxel 5/512 m, truncation 4 cm); the second segment starts `--offset` poses after the first and its poses are
displaced by a planted drift (0.6 / -0.5 / 0.7 degrees, 2 / -1.5 / 1 cm), so that registering it onto the first has something to find.

  fusion        wall time per frame of TSDFVolume.integrate (touch, allocation, integration) with a synchronisation, first segment
  extraction    wall time of extract_point_cloud of the first segment, synchronised
  candidates    points of the cloud with contract distance <= 0.1 m of a query (the query itself included), over a random sample of
                `--sample` queries (torch.cdist in fp32 against the whole cloud): mean and maximum, and vertices per square metre estimated
                from the mean as mean / (pi 0.1^2)
  normals       lk_normals_nn at max_nn = 50 and lk_normals (every point within 0.1 m) on the first cloud over one index with 0.1-m cells:
                device events around the call, median of `--reps` after a warm-up call
  registration  wall time of register_pair('robust_icp') on the two clouds as SegmentCloud(max_nn=50), indices and normals included, and
                max |T - T_planted|

    python tools/bench_segment_cloud.py [--frames 10] [--offset 5] [--reps 7] [--out profiles/segment_clouds.md]
"""
import argparse
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from loopy_slam_amd import core, synthetic, tsdf
from loopy_slam_amd import loop_closure as LC

DRIFT = (np.deg2rad([0.6, -0.5, 0.7]).tolist() + [0.02, -0.015, 0.01])


def commit():
    try:
        return subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip() or 'unknown'
    except OSError:
        return 'unknown'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=10)
    ap.add_argument('--offset', type=int, default=5)
    ap.add_argument('--step', type=int, default=2, help='loop poses between two frames of a segment')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sample', type=int, default=4000)
    ap.add_argument('--commit', type=str, default=None, help='the commit to name in the output (default: git rev-parse)')
    ap.add_argument('--out', type=str, default=None, help='also append the lines to this file')
    args = ap.parse_args()
    eng = core.Engine()
    sync = torch.cuda.synchronize
    intr = synthetic.TUM_INTR
    cam = (intr['fx'], intr['fy'], intr['cx'], intr['cy'])
    D = LC.se3_exp(DRIFT)
    Dt = torch.from_numpy(D).float().to(eng.device)

    def segment(first, displaced):
        fr = [synthetic.render_frame(first + k * args.step, intr=intr, holes=0.01, device=eng.device, scene='furnished') for k in range(args.frames)]
        return [(d, c) for d, c, _ in fr], [(Dt @ p) if displaced else p for _, _, p in fr]

    fa, pa = segment(0, False)
    fb, pb = segment(args.offset, True)
    warm = tsdf.fuse_segment(eng, fa[:1], pa[:1], *cam)             # first-call costs (allocator, torch kernels) stay out of the figures
    warm.extract_point_cloud()
    del warm
    sync()

    vol = tsdf.TSDFVolume(eng)
    t_fuse = []
    for (depth, color), c2w in zip(fa, pa):
        sync()
        t0 = time.perf_counter()
        vol.integrate(depth, color, c2w.float(), *cam)
        sync()
        t_fuse.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    cloud_a = vol.extract_point_cloud()['vertices'].contiguous()
    sync()
    t_extract = (time.perf_counter() - t0) * 1e3
    n_blocks = vol.n
    del vol
    cloud_b = tsdf.fuse_segment(eng, fb, pb, *cam).extract_point_cloud()['vertices'].contiguous()
    N = int(cloud_a.shape[0])

    # candidates per 0.1-m ball over a sample of the queries
    g = torch.Generator(device='cpu').manual_seed(3)
    q = cloud_a[torch.randperm(N, generator=g)[:args.sample].to(eng.device)]
    r = float(np.float32(LC.NORMAL_RADIUS))
    n_in = torch.cat([(torch.cdist(q[a:a + 250], cloud_a) <= r).sum(1) for a in range(0, int(q.shape[0]), 250)]).double()
    mean_in, max_in = float(n_in.mean()), int(n_in.max())

    camera = pa[0][:3, 3].cpu().numpy()
    knn = core.KnnIndex(eng, capacity=N, cell_size=LC.NORMAL_RADIUS)
    knn.build(cloud_a)

    def timed(fn):
        fn()
        sync()
        out = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            sync()
            out.append(e0.elapsed_time(e1))
        return statistics.median(out), min(out), max(out)
    t_nn = timed(lambda: LC.estimate_normals(eng, cloud_a, LC.NORMAL_RADIUS, camera, knn=knn, max_nn=50))
    t_all = timed(lambda: LC.estimate_normals(eng, cloud_a, LC.NORMAL_RADIUS, camera, knn=knn))
    n_nn, v_nn = LC.estimate_normals(eng, cloud_a, LC.NORMAL_RADIUS, camera, knn=knn, max_nn=50)
    n_all, v_all = LC.estimate_normals(eng, cloud_a, LC.NORMAL_RADIUS, camera, knn=knn)
    both = (v_nn != 0) & (v_all != 0)
    cosang = (n_nn[both] * n_all[both]).sum(1).abs().clamp(max=1)          # the angle between the two LINES: the flip is a separate matter
    ang = torch.rad2deg(torch.acos(cosang))
    knn.close()

    sync()
    t0 = time.perf_counter()
    sc, tc = LC.SegmentCloud(eng, cloud_b, pb[0][:3, 3], max_nn=50), LC.SegmentCloud(eng, cloud_a, pa[0][:3, 3], max_nn=50)
    reg = LC.register_pair(sc, tc, 'robust_icp')
    sync()
    t_reg = (time.perf_counter() - t0) * 1e3
    sc.close()
    tc.close()
    err = float(np.abs(reg['T'] - LC._inv(D)).max())

    lines = [f'commit {args.commit or commit()}; {args.frames} frames 640 x 480 per segment, voxel {5.0 / 512.0:.6f} m, truncation 0.04 m', '',
             '| figure | value |', '|---|---|',
             f'| cloud sizes (segment A, segment B) | {N:,}, {int(cloud_b.shape[0]):,} vertices ({n_blocks:,} blocks in A\'s volume) |',
             f'| candidates per 0.1-m ball ({int(q.shape[0]):,} sampled queries of A) | mean {mean_in:.0f}, max {max_in:,} |',
             f'| vertices per square metre (mean / (pi 0.1^2)) | {mean_in / (math.pi * r * r):,.0f} |',
             f'| fusion per frame (touch + allocation + integration, synchronised) | median {statistics.median(t_fuse):.2f} ms, '
             f'first {t_fuse[0]:.2f} ms, max {max(t_fuse):.2f} ms |',
             f'| extraction (extract_point_cloud of A) | {t_extract:.1f} ms |',
             f'| lk_normals_nn, max_nn = 50, on A | median {t_nn[0]:.3f} ms (min {t_nn[1]:.3f}, max {t_nn[2]:.3f}; {args.reps} calls) |',
             f'| lk_normals, every point within 0.1 m, on A | median {t_all[0]:.3f} ms (min {t_all[1]:.3f}, max {t_all[2]:.3f}) |',
             f'| angle between the two normals | median {float(ang.median()):.2f} degrees, 99th percentile {float(ang.quantile(0.99)):.2f} degrees |',
             f'| register_pair(robust_icp) B -> A, indices and normals included | {t_reg:.1f} ms, {reg["iterations"]} iterations, '
             f'overlap {reg["overlap"]:.3f}, fitness {reg["fitness"]:.3f}, max abs(T - T_planted) {err:.2e} |']
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text)


if __name__ == '__main__':
    main()
