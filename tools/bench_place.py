#!/usr/bin/env python3
"""Timing of place recognition on one MI355X (loopy_slam_amd/place.py, csrc/lk_place.hip) on frames of the textured synthetic room:

  describe      PlaceRecognizer.describe of one 480 x 640 and one 680 x 1200 frame: lk_place_detect, the read-back of the level counts, the
                per-level sorts, lk_place_describe (500 features, 8 levels) - wall-clock per call, the host synchronisation included
  match + score lk_place_match_score of one frame's descriptors against databases of 10, 100 and 1 000 segments of 500 descriptors
                (the descriptors of a few frames repeated) - events on the stream around back-to-back calls
  for scale     one frame-equivalent of the benchmark workload (bench.py: track one frame + its 60-iteration share of a mapped frame's 300)

    python tools/bench_place.py [--reps 5] [--inner 10] [--no-frame] [--out profiles/place_recognition.md]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from loopy_slam_amd import core, place, synthetic


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--no-frame', action='store_true', help='skip the frame-equivalent of the benchmark workload')
    ap.add_argument('--out', type=str, default=None, help='also append the tables to this file')
    args = ap.parse_args()
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

    lines = [f'ms per call, median of {args.reps} windows of {args.inner} calls', '', '| call | size | ms | note |', '|---|---|---|---|']
    descs = []
    for H, W in ((480, 640), (680, 1200)):
        intr = dict(H=H, W=W, fx=0.8 * W, fy=0.8 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
        pr = place.PlaceRecognizer(eng)
        frames = [synthetic.render_frame(k, intr=intr, holes=0.0, device=eng.device, scene='textured')[1].contiguous() for k in (0, 30, 60)]
        kp, desc = pr.describe(frames[0])
        ms = wall_ms(lambda: pr.describe(frames[0]))
        ws = pr.workspace(H, W)
        counts = eng.empty(pr.n_levels, dtype=torch.int32)
        det = event_ms(lambda: eng.lib.check(eng.lib.dll.lk_place_detect(frames[0].data_ptr(), H, W, pr.n_levels, ws.data_ptr(), counts.data_ptr(), eng.stream)))
        lines.append(f'| `PlaceRecognizer.describe` | {H} x {W} | {ms:.3f} | {int(kp.shape[0])} keypoints, {pr.layout[0] / 2 ** 20:.1f} MiB of workspace |')
        lines.append(f'| of which `lk_place_detect` (device time) | {H} x {W} | {det:.3f} | {4 * pr.n_levels + 3} launches |')
        if (H, W) == (480, 640):
            descs = [pr.describe(f)[1] for f in frames]
    for S in (10, 100, 1000):
        pr = place.PlaceRecognizer(eng, capacity=S)
        for s in range(S):
            pr.add(descs[s % len(descs)])
        q = descs[0]
        ms = event_ms(lambda: pr.match_counts(q))
        sc = pr.scores(q)
        lines.append(f'| `lk_place_match_score` | {int(q.shape[0])} rows against {S} segments | {ms:.3f} | best score {sc.max():.3f}, '
                     f'{int((sc > 0.223).sum())} segments above 0.223 |')
    if not args.no_frame:
        from loopy_slam_amd import workload
        wl = workload.FrameWorkload(eng)
        ms = wall_ms(lambda: wl.step())
        lines.append(f'| one frame-equivalent of the benchmark workload (`FrameWorkload.step`) | 640 x 480, {wl.n} points | {ms:.1f} | a mapped frame '
                     f'is five of these mapping shares |')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text)


if __name__ == '__main__':
    main()
