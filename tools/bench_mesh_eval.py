#!/usr/bin/env python3
"""Timing of the reconstruction evaluation on one MI355X (loopy_slam_amd/mesh_eval.py, csrc/lk_mesh.hip): `--frames` frames of the furnished
synthetic room's loop at 640 x 480 are fused at the reference's resolution and meshed; that mesh is the reconstruction, a copy moved by
5 mm the ground truth.

Kernel rows: ms per call, the median over `--reps` windows of `--inner` back-to-back calls between two events on the stream, after a warm-up
call (so the inputs are cache-warm and launch gaps are part of the figure).  Wall rows: host time around the whole function with a
synchronisation (index builds, torch bookkeeping and read-backs included).

    python tools/bench_mesh_eval.py [--frames 20] [--samples 200000] [--reps 5] [--inner 50] [--out profiles/mesh_eval.md]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from loopy_slam_amd import core, mesh_eval as E, synthetic
from loopy_slam_amd._ffi import ptr
from loopy_slam_amd.tsdf import TSDFVolume


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--samples', type=int, default=200_000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=50, help='calls per timed window of a kernel row')
    ap.add_argument('--out', type=str, default=None, help='also append the table to this file')
    args = ap.parse_args()
    eng = core.Engine()
    dll, sync = eng.lib.dll, torch.cuda.synchronize
    intr = synthetic.TUM_INTR
    cam = (intr['fx'], intr['fy'], intr['cx'], intr['cy'])
    step = max(1, 200 // args.frames)
    vol = TSDFVolume(eng)
    poses = []
    for k in range(args.frames):
        depth, color, c2w = synthetic.render_frame(k * step, intr=intr, holes=0.01, device=eng.device, scene='furnished')
        vol.integrate(depth, color, c2w, *cam)
        poses.append(c2w.cpu().numpy().astype(np.float64))
    rec = vol.extract_triangle_mesh()
    del vol
    shift = np.eye(4)
    shift[:3, 3] = (0.003, 0.0, 0.004)
    gt = E.transform(rec, shift, eng)
    v, t, _ = E._mesh(eng, rec)
    V, F, S = int(v.shape[0]), int(t.shape[0]), args.samples

    def kernel_ms(fn):
        """ms per call: `--inner` calls between two events (one call is tens of microseconds, too short a window by itself)"""
        fn()
        sync()
        out = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _k in range(args.inner):
                fn()
            e1.record()
            sync()
            out.append(e0.elapsed_time(e1) / args.inner)
        return statistics.median(out)

    def wall_ms(fn):
        fn()
        sync()
        out = []
        for _ in range(max(1, args.reps // 2)):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    rows = []
    area = eng.empty(F)
    rows.append(('k_mesh_areas', f'{F:,} faces', kernel_ms(lambda: eng.lib.check(dll.lk_mesh_areas(ptr(v), V, ptr(t), F, ptr(area), eng.stream)))))
    cum = torch.cumsum(area.double(), 0).contiguous()
    pts, face, bary = eng.empty(S, 3), eng.empty(S, dtype=torch.int32), eng.empty(S, 3)
    rows.append(('k_mesh_sample', f'{S:,} samples of {F:,} faces',
                 kernel_ms(lambda: eng.lib.check(dll.lk_mesh_sample(ptr(v), V, ptr(t), F, ptr(cum), 0, S, ptr(pts), ptr(face), ptr(bary), eng.stream)))))
    gp = E.sample_surface(gt, S, 1, eng)['points']
    index = E.NearestIndex(eng, gp)
    rows.append(('k_nearest, unbounded', f'{S:,} queries, {S:,} targets, cell {index.cell:.4f} m', kernel_ms(lambda: index.query(pts))))
    vindex = E.NearestIndex(eng, gt['vertices'])
    rows.append(('k_nearest, max_dist 0.1', f'{V:,} queries, {V:,} targets, cell {vindex.cell:.4f} m', kernel_ms(lambda: vindex.query(v, 0.1))))
    index.close()
    vindex.close()
    w2c = torch.from_numpy(np.linalg.inv(np.stack(poses))[:, :3, :].astype(np.float32)).to(eng.device).contiguous()
    seen = eng.zeros(V, dtype=torch.uint8)
    rows.append(('k_mesh_cull', f'{V:,} vertices x {len(poses)} poses',
                 kernel_ms(lambda: eng.lib.check(dll.lk_mesh_cull(ptr(v), V, ptr(w2c), len(poses), intr['H'], intr['W'], *[C.c_float(x) for x in cam],
                                                                  ptr(seen), eng.stream)))))
    view = poses[len(poses) // 2]
    ras = E.DepthRasteriser(rec, 500, 500, 300.0, 300.0, 249.5, 249.5, eng=eng)
    depth = eng.empty(500, 500)
    m12 = E._w2c_cv(view)
    rows.append(('k_mesh_depth_setup (+ fill)', f'{F:,} faces, 500 x 500',
                 kernel_ms(lambda: eng.lib.check(dll.lk_mesh_depth_setup(ptr(ras.v), V, ptr(ras.t), F, m12, *ras.cam, ptr(ras.rec), ptr(ras.box),
                                                                         ptr(ras.ntiles), ptr(depth), eng.stream)))))
    tile_end = torch.cumsum(ras.ntiles[:F], 0, dtype=torch.int64)
    T = int(tile_end[-1])
    tile_end = tile_end.to(torch.int32).contiguous()

    def raster():
        eng.lib.check(dll.lk_mesh_depth_setup(ptr(ras.v), V, ptr(ras.t), F, m12, *ras.cam, ptr(ras.rec), ptr(ras.box), ptr(ras.ntiles), ptr(depth),
                                              eng.stream))
        eng.lib.check(dll.lk_mesh_depth_raster(ptr(ras.rec), ptr(ras.box), ptr(tile_end), F, T, *ras.cam, ptr(depth), eng.stream))
    t_both = kernel_ms(raster)
    rows.append(('k_mesh_depth_raster (+ resolve)', f'{T:,} tiles of 8 x 8, {float((depth > 0).float().mean()) * 100:.1f} % of the pixels covered',
                 t_both - rows[-1][2]))
    walls = [('DepthRasteriser.render, one view', wall_ms(lambda: ras.render(view))),
             ('sample_surface', wall_ms(lambda: E.sample_surface(rec, S, 0, eng))),
             ('NearestIndex build', wall_ms(lambda: E.NearestIndex(eng, gp).close())),
             ('align (ICP over the vertices)', wall_ms(lambda: E.align(rec, gt, eng=eng))),
             (f'metrics_3d, {S:,} samples, align=False', wall_ms(lambda: E.metrics_3d(rec, gt, n_samples=S, align=False, eng=eng))),
             (f'metrics_3d, {S:,} samples, align=True', wall_ms(lambda: E.metrics_3d(rec, gt, n_samples=S, align=True, eng=eng)))]
    views = E.sample_views(gt, 10, seed=0, eng=eng)
    walls.append(('metric_2d, 10 views 500 x 500', wall_ms(lambda: E.metric_2d(rec, gt, views, eng=eng))))
    m = E.metrics_3d(rec, gt, n_samples=S, align=True, eng=eng)

    lines = [f'{args.frames} frames 640 x 480 fused at voxel 5/512 m: V = {V:,}, F = {F:,}; ground truth = the same mesh moved by 5 mm', '',
             '| kernel | size | ms per call (median of %d windows of %d calls) |' % (args.reps, args.inner), '|---|---|---|']
    lines += [f'| `{n}` | {s} | {ms:.3f} |' for n, s, ms in rows]
    lines += ['', '| host function (wall, synchronised) | ms |', '|---|---|']
    lines += [f'| {n} | {ms:.1f} |' for n, ms in walls]
    lines += ['', 'metrics_3d of that pair after alignment: ' + ', '.join(f'{k} {x:.4f}' for k, x in m.items())]
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text)


if __name__ == '__main__':
    main()
