#!/usr/bin/env python3
"""What a frame costs before the tracker sees it (loopy_slam_amd/datasets.py, csrc/lk_frame.hip), per 640 x 480 frame of the textured room:

  host      Pillow's JPEG and 16-bit PNG decode; the host pipeline the device path replaces (the float64 referee of tests/datasets_referee.py:
            what the reference's reader does in NumPy / cv2 after decoding) - wall clock, no GPU
  upload    the raw bytes (uint8 colour + uint16 depth, 1.5 MB) against the float images the host pipeline would upload (4.9 MB), pinned memory
  prepare   lk_frame_prepare: the identity path (Replica, TUM), the ScanNet path (968 x 1296 colour resized to the 480 x 640 depth) and a
            distorted frame with crop_size - events on the stream
  slam      tools/slam_run.py frames/s on an exported Replica-layout sequence read during the run, data.prefetch 0 and 2

Every step runs in a child process of its own under its own time limit; a step that fails or runs out of time ends the run.

    python tools/bench_frames.py [--reps 5] [--inner 20] [--no-slam] [--slam-frames 16] [--out profiles/frames.md]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
STEP_LIMIT_S = 400
H, W = 480, 640
DISTORTION = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)
CROP_SIZE = (384, 512)


def wall_ms(fn, reps, inner=1):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _k in range(inner):
            fn()
        out.append((time.perf_counter() - t0) * 1e3 / inner)
    return statistics.median(out)


def frame(h=H, w=W):
    import export_sequence as ex
    return ex.synthetic_frames(1, h, w)[0][:2]


def host_step(args):
    import numpy as np
    import datasets_referee as ref
    import export_sequence as ex
    from loopy_slam_amd import datasets
    c8, d16 = frame()
    tmp = tempfile.mkdtemp()
    ex._save(c8, os.path.join(tmp, 'c.jpg'), quality=95)
    ex._save(d16, os.path.join(tmp, 'd.png'))
    buf_c, buf_d = np.empty_like(c8), np.empty_like(d16)
    print(f'| Pillow JPEG decode into a reused buffer | {H} x {W} | {wall_ms(lambda: datasets.decode_color(os.path.join(tmp, "c.jpg"), buf_c), args.reps, 5):.2f} | '
          f'{os.path.getsize(os.path.join(tmp, "c.jpg")) / 1024:.0f} KB file |')
    print(f'| Pillow 16-bit PNG decode into a reused buffer | {H} x {W} | {wall_ms(lambda: datasets.decode_depth(os.path.join(tmp, "d.png"), buf_d), args.reps, 5):.2f} | '
          f'{os.path.getsize(os.path.join(tmp, "d.png")) / 1024:.0f} KB file |')
    K = ex.intrinsics(H, W)
    k4 = {k: K[k] for k in ('fx', 'fy', 'cx', 'cy')}
    print(f'| host pipeline, identity path (c / 255. in float64, depth / scale, float32 copies for the upload) | {H} x {W} | '
          f'{wall_ms(lambda: [a.astype(np.float32) for a in ref.prepare(c8, d16, 6553.5)[:2]], args.reps):.2f} | NumPy, one thread |')
    big = frame(968, 1296)[0]
    print(f'| host pipeline, ScanNet path (resize 968 x 1296 -> 480 x 640 in float64) | {H} x {W} | '
          f'{wall_ms(lambda: ref.prepare(big, d16, 1000.0, edge=10), max(1, args.reps // 2)):.2f} | NumPy referee, not cv2 |')
    print(f'| host pipeline, undistortion + crop_size {CROP_SIZE} | {H} x {W} | '
          f'{wall_ms(lambda: ref.prepare(c8, d16, 5000.0, distortion=DISTORTION, crop_size=CROP_SIZE, edge=8, **k4), max(1, args.reps // 2)):.2f} | '
          f'NumPy referee, not cv2 |')


def device_step(args):
    import torch
    import export_sequence as ex
    from loopy_slam_amd import core, datasets
    eng = core.Engine()

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

    c8, d16 = frame()
    big = frame(968, 1296)[0]
    hc, hd = torch.from_numpy(c8).pin_memory(), torch.from_numpy(d16.view('int16')).pin_memory()
    fc, fd = torch.empty(H, W, 3).pin_memory(), torch.empty(H, W).pin_memory()
    dc, dd = eng.empty(H, W, 3, dtype=torch.uint8), eng.empty(H, W, dtype=torch.int16)
    dfc, dfd = eng.empty(H, W, 3), eng.empty(H, W)
    dbig = torch.from_numpy(big).to(eng.device)
    undist = eng.empty(H, W, 3, dtype=torch.uint8)
    K = ex.intrinsics(H, W)
    k4 = {k: K[k] for k in ('fx', 'fy', 'cx', 'cy')}
    raw = event_ms(lambda: (dc.copy_(hc, non_blocking=True), dd.copy_(hd, non_blocking=True)))
    flt = event_ms(lambda: (dfc.copy_(fc, non_blocking=True), dfd.copy_(fd, non_blocking=True)))
    print(f'| upload of the raw bytes (uint8 colour + uint16 depth, pinned) | {H} x {W} | {raw:.3f} | {(hc.numel() + 2 * hd.numel()) / 1e6:.2f} MB |')
    print(f'| upload of float colour + depth, what the host pipeline would send (pinned) | {H} x {W} | {flt:.3f} | {4 * (fc.numel() + fd.numel()) / 1e6:.2f} MB |')
    out = (eng.empty(H, W, 3), eng.empty(H, W))
    ms = event_ms(lambda: datasets.prepare_frame(eng, dc, dd, 6553.5, out=out))
    print(f'| `lk_frame_prepare`, identity path | {H} x {W} | {ms:.4f} | 1 launch, {(dc.numel() + 2 * dd.numel() + 16 * dd.numel()) / 1e6:.1f} MB of traffic |')
    out10 = (eng.empty(H - 20, W - 20, 3), eng.empty(H - 20, W - 20))
    ms = event_ms(lambda: datasets.prepare_frame(eng, dbig, dd, 1000.0, crop_edge=10, out=out10))
    print(f'| `lk_frame_prepare`, ScanNet path (colour 968 x 1296 -> 480 x 640, crop_edge 10) | {H} x {W} | {ms:.4f} | 1 launch, 4 taps per pixel |')
    Ho, Wo = datasets.output_size(H, W, CROP_SIZE, 8)
    outc = (eng.empty(Ho, Wo, 3), eng.empty(Ho, Wo))
    ms = event_ms(lambda: datasets.prepare_frame(eng, dc, dd, 5000.0, distortion=DISTORTION, crop_size=CROP_SIZE, crop_edge=8, undist=undist, out=outc,
                                                 **k4))
    print(f'| `lk_frame_prepare`, undistortion + crop_size {CROP_SIZE} + crop_edge 8 | {H} x {W} | {ms:.4f} | 2 launches |')


def slam_step(args):
    """tools/slam_run.py on an exported Replica-layout sequence, frames read during the run."""
    prefetch, folder = args.step.split(':', 2)[1:]
    import export_sequence as ex
    K = ex.intrinsics(H, W)
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'slam_run.py'), '--config', 'configs/Replica/room0.yaml', '--input_folder', folder,
           '--prefetch', prefetch, '--stream', '--cam', ','.join(str(K[k]) for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=STEP_LIMIT_S - 40)     # ends before this step's own limit does
    except subprocess.TimeoutExpired:
        sys.stderr.write(f'slam_run.py: no result within {STEP_LIMIT_S - 40} s\n')
        return 1
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return r.returncode
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    print(f'| `tools/slam_run.py --stream`, Replica layout, data.prefetch {prefetch} | {H} x {W} | {out["ms_tracked_frame"]} per tracked frame, '
          f'{out["ms_mapped_frame"]} per mapped frame | {out["frames_per_s"]} frames/s over {out["frames"]} frames, {out["points"]} points |')
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--no-slam', action='store_true')
    ap.add_argument('--no-device', action='store_true', help='host figures only (no GPU needed)')
    ap.add_argument('--slam-frames', type=int, default=16)
    ap.add_argument('--out', type=str, default=None, help='also append the table to this file')
    ap.add_argument('--step', type=str, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == 'host':
        return host_step(args)
    if args.step == 'device':
        return device_step(args)
    if args.step:
        return slam_step(args)
    steps = ['host'] + ([] if args.no_device else ['device'])
    if not (args.no_slam or args.no_device):
        import export_sequence as ex
        folder = tempfile.mkdtemp(prefix='replica_export_')
        ex.write_sequence(folder, 'replica', ex.synthetic_frames(args.slam_frames, H, W, png_depth_scale=6553.5))
        steps += [f'slam:0:{folder}', f'slam:2:{folder}']
    lines = [f'ms per call, median of {args.reps} windows', '', '| call | size | ms | note |', '|---|---|---|---|']
    for name in steps:
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
        print('\n'.join(ln for ln in r.stdout.splitlines() if ln.startswith('|')), flush=True)
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
