#!/usr/bin/env python3
"""Timing of the rendering evaluation of one frame pair on one MI355X (loopy_slam_amd/render_eval.py, csrc/lk_imgeval.hip): a 680 x 1200
frame of the furnished synthetic room (the Replica size) against itself plus noise, its depth against itself plus noise.

Two paths over the same formulas on the same device:
  lk_img_eval     the six launches of render_eval.frame_metrics (workspace and record allocated outside the timed window for the ABI row)
  torch ops       what a user would write without it: grouped conv2d and avg_pool2d for the five levels, boolean-mask gathers and means
                  for depth L1 and PSNR (each gather synchronises), the combination on the device
ms per frame pair: the median over `--reps` windows of `--inner` back-to-back calls between two events on the stream, after a warm-up call
(inputs cache-warm, launch gaps part of the figure).  The last line compares the figures the two paths produce.

    python tools/bench_render_eval.py [--H 680] [--W 1200] [--reps 5] [--inner 20] [--out profiles/render_eval.md]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
from loopy_slam_amd import core, render_eval, synthetic
from loopy_slam_amd._ffi import IMG_REC, ptr


def torch_path(gt_color, color, gt_depth, depth):
    """(depth_l1, psnr, ms_ssim) as device scalars from torch ops alone."""
    on = gt_depth > 0
    l1 = (gt_depth[on] - depth[on]).abs().mean()
    psnr = -10.0 * torch.log10(((gt_color[on] - color[on]) ** 2).mean())
    k = torch.arange(11, dtype=torch.float32, device=gt_color.device) - 5
    g = torch.exp(-(k * k) / (2 * 1.5 ** 2))
    g = g / g.sum()
    gv, gh = g.reshape(1, 1, 11, 1).repeat(3, 1, 1, 1), g.reshape(1, 1, 1, 11).repeat(3, 1, 1, 1)
    G = lambda x: F.conv2d(F.conv2d(x, gv, groups=3), gh, groups=3)
    X, Y = gt_color.permute(2, 0, 1)[None], color.permute(2, 0, 1)[None]
    vals = []
    for l in range(5):
        mu1, mu2 = G(X), G(Y)
        s1, s2, s12 = G(X * X) - mu1 * mu1, G(Y * Y) - mu2 * mu2, G(X * Y) - mu1 * mu2
        cs = (2 * s12 + 0.03 ** 2) / (s1 + s2 + 0.03 ** 2)
        if l < 4:
            vals.append(torch.relu(cs.flatten(2).mean(-1)))
            pad = [s % 2 for s in X.shape[2:]]
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
        else:
            vals.append(torch.relu((((2 * mu1 * mu2 + 0.01 ** 2) / (mu1 * mu1 + mu2 * mu2 + 0.01 ** 2)) * cs).flatten(2).mean(-1)))
    w = torch.tensor(render_eval.MS_WEIGHTS, device=gt_color.device)
    return l1, psnr, torch.prod(torch.stack(vals, 0) ** w.view(-1, 1, 1), 0).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--H', type=int, default=680)
    ap.add_argument('--W', type=int, default=1200)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', type=str, default=None, help='also append the table to this file')
    args = ap.parse_args()
    eng = core.Engine()
    H, W = args.H, args.W
    intr = dict(H=H, W=W, fx=0.5 * W, fy=0.5 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    gt_depth, gt_color, _ = synthetic.render_frame(7, intr=intr, holes=0.02, device=eng.device, scene='furnished')
    g = torch.Generator(device=eng.device).manual_seed(3)
    color = (gt_color + 0.05 * torch.randn(gt_color.shape, generator=g, device=eng.device)).clamp(0, 1).contiguous()
    depth = (gt_depth + 0.01 * torch.randn(gt_depth.shape, generator=g, device=eng.device)).contiguous()
    gt_depth, gt_color = gt_depth.contiguous(), gt_color.contiguous()
    n = C.c_int64(0)
    eng.lib.check(eng.lib.dll.lk_img_eval_ws_bytes(H, W, C.byref(n)), 'lk_img_eval_ws_bytes')
    ws, rec = eng.empty((n.value + 7) // 8, dtype=torch.float64), eng.empty(IMG_REC, dtype=torch.float64)

    def abi(msssim=1):
        eng.lib.check(eng.lib.dll.lk_img_eval(ptr(gt_color), ptr(color), ptr(gt_depth), ptr(depth), H, W, msssim, ptr(ws), ptr(rec), eng.stream))

    def window_ms(fn):
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

    rows = [('`lk_img_eval`, MS-SSIM and masked sums', '6 launches', window_ms(abi)),
            ('`lk_img_eval`, masked sums alone (`with_msssim = 0`)', '2 launches', window_ms(lambda: abi(0))),
            ('`render_eval.frame_metrics` (allocates workspace and record)', '6 launches + 2 allocations',
             window_ms(lambda: render_eval.frame_metrics(eng, gt_color, color, gt_depth, depth))),
            ('torch ops (grouped `conv2d`, `avg_pool2d`, masked means)', 'about 130 launches, 2 host synchronisations',
             window_ms(lambda: torch_path(gt_color, color, gt_depth, depth)))]
    s = render_eval.summarise([render_eval.frame_metrics(eng, gt_color, color, gt_depth, depth)])
    l1, psnr, ms = (float(x) for x in torch_path(gt_color, color, gt_depth, depth))
    lines = [f'One {H} x {W} frame pair ({n.value / 2 ** 20:.1f} MiB of workspace), ms per pair, median of {args.reps} windows of {args.inner} calls', '',
             '| path | launches | ms |', '|---|---|---|']
    lines += [f'| {name} | {what} | {ms_:.3f} |' for name, what, ms_ in rows]
    lines += ['', f'kernel / torch ops: depth L1 {s["depth_l1"][0]:.6f} / {l1:.6f} m, PSNR {s["psnr"][0]:.4f} / {psnr:.4f} dB, '
                  f'MS-SSIM {s["ms_ssim"][0]:.6f} / {ms:.6f}; the kernel path takes {rows[0][2] / rows[3][2] * 100:.1f} % of the torch-op time']
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text)


if __name__ == '__main__':
    main()
