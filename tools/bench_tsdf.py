#!/usr/bin/env python3
"""Timing of TSDF fusion and meshing on one MI355X (loopy_slam_amd/tsdf.py, csrc/lk_tsdf.hip): `--frames` frames of the furnished synthetic
room's loop at 640 x 480 fused at the reference's resolution (voxel 5/512 m, truncation 4 cm), then one mesh extraction.

Per frame: touch + allocation (lk_tsdf_touch, torch.unique, the key sort, growing the planes; wall time with a synchronisation) and the
integration (lk_tsdf_integrate alone between two events on the stream).  The integration is HBM-bound; its traffic is reported under two models:
  moved = 40 B per updated voxel (five planes read and written; voxels that fail a test load nothing from the volume)
  model = 40 B per updated voxel + 20 B per visited voxel (a kernel that reads a voxel before it decides)
both divided by the integration time, next to the ~6.3 TB/s a streaming copy reaches on this chip.  Updated voxels are counted as the growth
of the weight plane's sum, visited voxels are 4 096 per touched block.

    python tools/bench_tsdf.py [--frames 40] [--voxel 0.009765625] [--trunc 0.04] [--out profiles/tsdf.md]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from loopy_slam_amd import core, synthetic
from loopy_slam_amd.tsdf import BLOCK_VOXELS, TSDFVolume

COPY_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=40)
    ap.add_argument('--voxel', type=float, default=5.0 / 512.0)
    ap.add_argument('--trunc', type=float, default=0.04)
    ap.add_argument('--out', type=str, default=None, help='also append the tables to this file')
    args = ap.parse_args()
    eng = core.Engine()
    sync = torch.cuda.synchronize
    intr = synthetic.TUM_INTR
    cam = (intr['fx'], intr['fy'], intr['cx'], intr['cy'])
    step = max(1, 200 // args.frames)
    frames = [synthetic.render_frame(k * step, intr=intr, holes=0.01, device=eng.device, scene='furnished') for k in range(args.frames)]
    warm = TSDFVolume(eng, args.voxel, args.trunc)                 # first-call costs (allocator, torch kernels) stay out of the figures
    warm.integrate(*frames[0], *cam)
    warm.extract_triangle_mesh()
    del warm
    sync()

    vol = TSDFVolume(eng, args.voxel, args.trunc)
    rows = []
    for depth, color, c2w in frames:
        sync()
        t0 = time.perf_counter()
        touched = vol.touch(depth, c2w, *cam)
        slots = vol.allocate(touched)
        sync()
        t_touch = (time.perf_counter() - t0) * 1e3
        w0 = float(vol.planes[:vol.n, 1].sum(dtype=torch.float64))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        vol.integrate_blocks(touched, depth, color, c2w, *cam, slots=slots)        # only the kernel is between the events
        e1.record()
        sync()
        t_int = e0.elapsed_time(e1)
        updated = int(round(float(vol.planes[:vol.n, 1].sum(dtype=torch.float64)) - w0))
        visited = int(touched.shape[0]) * BLOCK_VOXELS
        rows.append((int(touched.shape[0]), vol.n, t_touch, t_int, updated, visited))
    sync()
    t0 = time.perf_counter()
    mesh = vol.extract_triangle_mesh()
    sync()
    t_mesh = (time.perf_counter() - t0) * 1e3

    lines = [f'{args.frames} frames 640 x 480, voxel {args.voxel:.6f} m, truncation {args.trunc} m, {vol.n:,} blocks '
             f'({vol.n * 5 * BLOCK_VOXELS * 4 / 2 ** 20:.0f} MiB of planes)', '',
             '| frame | blocks touched | blocks total | touch + allocation ms | integrate ms | updated voxels | moved GB/s | model GB/s |',
             '|---|---|---|---|---|---|---|---|']
    for k, (nt, n, tt, ti, up, vis) in enumerate(rows):
        if k < 3 or k % 8 == 0 or k == len(rows) - 1:
            lines.append(f'| {k} | {nt:,} | {n:,} | {tt:.2f} | {ti:.3f} | {up:,} | {40 * up / ti / 1e6:.0f} | {(40 * up + 20 * vis) / ti / 1e6:.0f} |')
    ti_all, up_all, vis_all = sum(r[3] for r in rows), sum(r[4] for r in rows), sum(r[5] for r in rows)
    lines += ['',
              f'- touch + allocation: median {statistics.median(r[2] for r in rows):.2f} ms per frame, total {sum(r[2] for r in rows):.1f} ms',
              f'- integration: median {statistics.median(r[3] for r in rows):.3f} ms per frame, total {ti_all:.1f} ms; '
              f'{40 * up_all / ti_all / 1e9:.2f} TB/s moved, {(40 * up_all + 20 * vis_all) / ti_all / 1e9:.2f} TB/s by the model '
              f'(streaming copy: ~{COPY_TBS} TB/s); {100.0 * up_all / vis_all:.1f} % of the visited voxels are updated',
              f'- extraction (neighbour table, lk_mc_mark, compaction, lk_mc_vertices, lk_mc_triangles): {t_mesh:.1f} ms, '
              f'V = {mesh["vertices"].shape[0]:,}, F = {mesh["triangles"].shape[0]:,}']
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text)


if __name__ == '__main__':
    main()
