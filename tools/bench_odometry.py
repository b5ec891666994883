#!/usr/bin/env python3
"""Timing of the visual odometry on one MI355X (loopy_slam_amd/odometry.py, csrc/lk_odom.hip) on frames of the textured synthetic room on the
hand-held walk:

  prepare       lk_odom_prepare of one 480 x 640 and one 680 x 1200 frame (3 levels, 6 launches) - events on the stream
  estimate      lk_odom_estimate with the default iterations 100 / 50 / 30 (360 launches) - events on the stream
  per frame     VisualOdometer.estimate_pose: prepare + estimate + the one read-back - wall clock, the synchronisation included
  for scale     the tracker's share of the benchmark workload: `--track-iters` iterations of FrameWorkload's tracking loop (bench.py's step)

Every GPU step runs in a child process of its own under its own time limit; a step that fails or runs out of time ends the run.

    python tools/bench_odometry.py [--reps 5] [--inner 5] [--no-frame] [--out profiles/odometry.md]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 240


def step(args):
    import torch
    from loopy_slam_amd import core, odometry, synthetic
    eng = core.Engine()

    def wall_ms(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for _k in range(args.inner):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3 / args.inner)
        return statistics.median(out)

    def event_ms(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _k in range(args.inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / args.inner)
        return statistics.median(out)

    if args.step == 'frame':
        from loopy_slam_amd import workload
        wl = workload.FrameWorkload(eng)
        ms = wall_ms(lambda: wl.step())
        print(f'| one frame-equivalent of the benchmark workload (`FrameWorkload.step`) | 640 x 480, {wl.n} points | {ms:.2f} | tracking and the '
              f'mapping share together |')
        return
    H, W = (int(v) for v in args.step.split('x'))
    intr = dict(H=H, W=W, fx=0.8 * W, fy=0.8 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    frames = [synthetic.render_frame(k, intr=intr, holes=0.02, device=eng.device, motion='handheld', scene='textured') for k in (11, 12)]
    vo = odometry.VisualOdometer(eng, intr, True)
    d0, c0, _ = frames[0]
    d1, c1, p1 = frames[1]
    ms = event_ms(lambda: vo.prepare(c1, d1, vo.pyr[1]))
    print(f'| `lk_odom_prepare` | {H} x {W} | {ms:.3f} | 3 levels, 6 launches, {vo.layout[0] / 2 ** 20:.1f} MiB per pyramid |')
    vo.prepare(c0, d0, vo.pyr[0])
    ms = event_ms(lambda: vo.estimate(vo.pyr[1], vo.pyr[0]))
    rec = vo.state[16 + (vo.n_iters - 1) * 33:16 + vo.n_iters * 33].cpu()
    print(f'| `lk_odom_estimate` | {H} x {W} | {ms:.3f} | iterations {vo.opt["iters"]}, {2 * vo.n_iters} launches; last step {float(rec[31]):.1e}, '
          f'{int(rec[2])} valid pixels |')

    def per_frame():
        vo.set_init_state(c0, d0, frames[0][2])
        return vo.estimate_pose(c1, d1)
    ms = wall_ms(per_frame)
    c2w = per_frame()
    err = 100 * float((c2w[:3, 3] - p1.cpu().double()[:3, 3]).norm())
    copied = 100 * float((frames[0][2].cpu().double()[:3, 3] - p1.cpu().double()[:3, 3]).norm())
    print(f'| `set_init_state` + `estimate_pose` (two prepares, one estimate, one read-back) | {H} x {W} | {ms:.3f} | start {err:.2f} cm from the '
          f'truth, the copied pose {copied:.2f} cm |')
    for iters in ((20, 10, 5), (10, 5, 3)):
        vs = odometry.VisualOdometer(eng, intr, {'iters': list(iters)})

        def short():
            vs.set_init_state(c0, d0, frames[0][2])
            return vs.estimate_pose(c1, d1)
        ms = wall_ms(short)
        c2w = short()
        err = 100 * float((c2w[:3, 3] - p1.cpu().double()[:3, 3]).norm())
        print(f'| the same with iterations {list(iters)} | {H} x {W} | {ms:.3f} | start {err:.2f} cm from the truth |')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--no-frame', action='store_true', help='skip the frame-equivalent of the benchmark workload')
    ap.add_argument('--out', type=str, default=None, help='also append the table to this file')
    ap.add_argument('--step', type=str, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    lines = [f'ms per call, median of {args.reps} windows of {args.inner} calls', '', '| call | size | ms | note |', '|---|---|---|---|']
    for name in ['480x640', '680x1200'] + ([] if args.no_frame else ['frame']):
        cmd = [sys.executable, os.path.abspath(__file__), '--step', name, '--reps', str(args.reps), '--inner', str(args.inner)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f'step {name}: no result within {STEP_LIMIT_S} s; stopping', file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f'step {name} failed (exit {r.returncode}); stopping\n{r.stdout}{r.stderr}', file=sys.stderr)
            return 1
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith('|')]
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
