#!/usr/bin/env python3
"""Write frames of the synthetic room (loopy_slam_amd.synthetic) to disk in the layout of one of the datasets the readers of
loopy_slam_amd.datasets open - the way to exercise a reader without owning a dataset:

    python tools/export_sequence.py OUT --layout tumrgbd [--scene textured] [--motion handheld] [--frames 12] [--size 120x160]
                                        [--png_depth_scale 5000]

Colour is quantised to uint8 (PNG for tumrgbd: a lossless round trip; JPEG for replica, scannet, azure, as those datasets ship), depth to
uint16 at png_depth_scale; a pose goes into the dataset's own file convention with columns 1 and 2 of its rotation negated, so that the reader's
negation restores it.  A TUM reader reports poses relative to its first frame.  The camera of a W x H export: fx = fy = 26 W / 32,
cx = W / 2 - 0.5, cy = H / 2 - 0.5 (intrinsics(H, W) below; put them into the run's cam section).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAYOUTS = ('replica', 'scannet', 'azure', 'tumrgbd')


def intrinsics(H, W):
    return dict(H=H, W=W, fx=26.0 * W / 32, fy=26.0 * W / 32, cx=W / 2 - 0.5, cy=H / 2 - 0.5)


def quantise(color, depth, png_depth_scale):
    """float colour [H,W,3] in [0,1] and depth [H,W] in metres (arrays or tensors) -> (uint8, uint16) arrays."""
    color, depth = np.asarray(color, dtype=np.float64), np.asarray(depth, dtype=np.float64)
    return (np.clip(np.rint(color * 255.0), 0, 255).astype(np.uint8),
            np.clip(np.rint(depth * float(png_depth_scale)), 0, 65535).astype(np.uint16))


def synthetic_frames(n, H, W, scene='textured', motion='handheld', png_depth_scale=5000.0):
    """[(uint8 colour, uint16 depth, c2w float64 [4,4])] of the synthetic room at intrinsics(H, W)."""
    from loopy_slam_amd import synthetic
    out = []
    for k in range(n):
        d, c, p = synthetic.render_frame(k, intr=intrinsics(H, W), holes=0.01, n_poses=2000, motion=motion, scene=scene)
        out.append(quantise(c.numpy(), d.numpy(), png_depth_scale) + (p.double().numpy(),))
    return out


def file_pose(c2w):
    """The pose as a dataset file holds it: columns 1 and 2 of the rotation negated."""
    out = np.array(c2w, dtype=np.float64)
    out[:3, 1] *= -1
    out[:3, 2] *= -1
    return out


def matrix_quaternion(R):
    """(x, y, z, w) of a rotation matrix, w >= 0: the branch with the largest diagonal term, for a well-conditioned square root."""
    R = np.asarray(R, dtype=np.float64)
    t = np.trace(R)
    if t > 0:
        s = 2.0 * np.sqrt(1.0 + t)
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0, 0.0, 0.0, (R[k, j] - R[j, k]) / s]
        q[i], q[j], q[k] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    q = np.array(q)
    return q if q[3] >= 0 else -q


def _num(v):
    return repr(float(v))


def _save(arr, path, **kw):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path, **kw)


def write_sequence(folder, layout, frames, names=None, poses=True, jpeg_quality=95):
    """frames: [(uint8 colour, uint16 depth, c2w)].  names: the integer of each ScanNet file name (default 0, 1, ...).  poses=False leaves the
    trajectory file of an Azure export out.  -> the 4 x 4 float64 matrices written (TUM: the matrix whose translation and quaternion were)."""
    if layout not in LAYOUTS:
        raise ValueError(f'layout {layout!r}; supported: {", ".join(LAYOUTS)}')
    os.makedirs(folder, exist_ok=True)
    written = [file_pose(p) for _, _, p in frames]
    rows = lambda T: [' '.join(_num(v) for v in r) for r in T]              # noqa: E731
    if layout == 'replica':
        for k, (c, d, _) in enumerate(frames):
            _save(c, os.path.join(folder, 'results', f'frame{k:06d}.jpg'), quality=jpeg_quality)
            _save(d, os.path.join(folder, 'results', f'depth{k:06d}.png'))
        with open(os.path.join(folder, 'traj.txt'), 'w') as f:
            f.writelines(' '.join(rows(T)) + '\n' for T in written)
    elif layout == 'scannet':
        names = list(range(len(frames))) if names is None else list(names)
        os.makedirs(os.path.join(folder, 'frames', 'pose'), exist_ok=True)
        for n, (c, d, _), T in zip(names, frames, written):
            _save(c, os.path.join(folder, 'frames', 'color', f'{n}.jpg'), quality=jpeg_quality)
            _save(d, os.path.join(folder, 'frames', 'depth', f'{n}.png'))
            with open(os.path.join(folder, 'frames', 'pose', f'{n}.txt'), 'w') as f:
                f.write('\n'.join(rows(T)) + '\n')
    elif layout == 'azure':
        for k, (c, d, _) in enumerate(frames):
            _save(c, os.path.join(folder, 'color', f'{k:05d}.jpg'), quality=jpeg_quality)
            _save(d, os.path.join(folder, 'depth', f'{k:05d}.png'))
        if poses:
            os.makedirs(os.path.join(folder, 'scene'), exist_ok=True)
            with open(os.path.join(folder, 'scene', 'trajectory.log'), 'w') as f:
                for k, T in enumerate(written):
                    f.write(f'{k} {k} 1.0\n' + '\n'.join(rows(T)) + '\n')
    else:
        lists = {n: [f'# {n} of a synthetic sequence', '# file: export_sequence', '# timestamp ...'] for n in ('rgb', 'depth', 'groundtruth')}
        for k, ((c, d, _), T) in enumerate(zip(frames, written)):
            stamp = f'{1000.0 + 0.04 * k:.6f}'
            _save(c, os.path.join(folder, 'rgb', stamp + '.png'))
            _save(d, os.path.join(folder, 'depth', stamp + '.png'))
            lists['rgb'].append(f'{stamp} rgb/{stamp}.png')
            lists['depth'].append(f'{stamp} depth/{stamp}.png')
            lists['groundtruth'].append(' '.join([stamp] + [_num(v) for v in T[:3, 3]] + [_num(v) for v in matrix_quaternion(T[:3, :3])]))
        for n, lines in lists.items():
            with open(os.path.join(folder, n + '.txt'), 'w') as f:
                f.write('\n'.join(lines) + '\n')
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description='Export frames of the synthetic room in a dataset layout.')
    ap.add_argument('out')
    ap.add_argument('--layout', choices=LAYOUTS, default='tumrgbd')
    ap.add_argument('--scene', default='textured')
    ap.add_argument('--motion', default='handheld')
    ap.add_argument('--frames', type=int, default=12)
    ap.add_argument('--size', default='120x160', help='HxW')
    ap.add_argument('--png_depth_scale', type=float, default=5000.0)
    args = ap.parse_args(argv)
    H, W = (int(v) for v in args.size.lower().split('x'))
    write_sequence(args.out, args.layout, synthetic_frames(args.frames, H, W, args.scene, args.motion, args.png_depth_scale))
    print(f'{args.frames} frames of {H} x {W} in the {args.layout} layout -> {args.out}; cam: {intrinsics(H, W)}, '
          f'png_depth_scale {args.png_depth_scale}')


if __name__ == '__main__':
    main()
