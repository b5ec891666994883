#!/usr/bin/env python3
"""The rendering evaluation of a finished run from its files: the frames {output}/rendered_every_frame/depth_XXXXX.npy and color_XXXXX.npy
(kept by a run with meshing.source 'rendered') measured against the input frames of the config's reader - depth L1, PSNR, MS-SSIM - and
the ATE of the last checkpoint's poses, into {output}/eval/rendering.json: the file a run with rendering_eval.enabled writes itself
(loopy_slam_amd/render_eval.py; needs the GPU).

    python tools/eval_rendering.py configs/Synthetic/room.yaml [--output DIR] [--input_folder DIR]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from loopy_slam_amd import config, core, datasets, render_eval, slam
from get_mesh_tsdf_fusion import last_checkpoint, rendered_frames


def evaluate(eng, cfg, output, reader=None, write=True):
    """The result dict of the run in `output`; reader: the frames ([i] -> (idx, color, depth, c2w)), default the config's."""
    if reader is None:               # as Point_SLAM picks it: the config's reader on a sequence on disk, else the synthetic room
        reader = datasets.open_sequence(cfg, None, eng=eng) or slam.SyntheticRoomDataset(cfg, eng.device)
    ck = last_checkpoint(output)
    n = int(ck['idx']) + 1
    est, gt = ck['estimate_c2w_list'][:n], ck['gt_c2w_list'][:n]
    es = render_eval.settings(cfg)
    frames, records, msssim, reason = [], [], False, 'no frame to evaluate'
    for idx, depth_file, color_file in rendered_frames(os.path.join(output, 'rendered_every_frame')):
        if idx >= n or not bool(torch.isfinite(est[idx]).all()):
            continue
        _, gt_color, gt_depth, _ = reader[idx]
        if not records:
            msssim, reason = render_eval.wants_msssim(es, int(gt_depth.shape[0]), int(gt_depth.shape[1]))
        frames.append(idx)
        records.append(render_eval.frame_metrics(eng, gt_color, torch.from_numpy(np.load(color_file).astype(np.float32)), gt_depth,
                                                 torch.from_numpy(np.load(depth_file).astype(np.float32)), msssim))
    if not records:
        raise ValueError(f'no depth_*.npy of an evaluated frame in {os.path.join(output, "rendered_every_frame")}')
    return render_eval.report(frames, records, est, gt, msssim, reason, output if write else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('config', type=str)
    ap.add_argument('--output', type=str)
    ap.add_argument('--input_folder', type=str, help='the sequence the run read; overrides data.input_folder')
    args = ap.parse_args()
    cfg = config.load_config(args.config, os.path.join(ROOT, 'configs', 'point_slam.yaml'))
    if args.input_folder:
        cfg['data']['input_folder'] = args.input_folder
    output = args.output or cfg['data'].get('output', 'output')
    out = evaluate(core.Engine(), cfg, output)
    ms = 'none' if out['avg_ms_ssim'] is None else f"{out['avg_ms_ssim']:.4f}"
    print(f"{len(out['frames'])} frames -> {os.path.join(output, 'eval', 'rendering.json')}: depth L1 {out['avg_depth_l1']:.5f} m, "
          f"PSNR {out['avg_psnr']:.3f} dB, MS-SSIM {ms}, ATE rmse {(out['ate'] or {}).get('absolute_translational_error.rmse')}")


if __name__ == '__main__':
    main()
