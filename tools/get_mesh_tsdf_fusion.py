#!/usr/bin/env python3
"""The mesh of a finished run from its files, as the reference's src/tools/get_mesh_tsdf_fusion.py --no_render makes it: the frames
{output}/rendered_every_frame/depth_XXXXX.npy and color_XXXXX.npy are fused at the poses of the last checkpoint in {output}/ckpts
(estimate_c2w_list) and the mesh goes to {output}/mesh/{scene}_pred_mesh.ply (loopy_slam_amd/tsdf.py; needs the GPU).

    python tools/get_mesh_tsdf_fusion.py configs/Synthetic/room.yaml [--output DIR] [--input_folder DIR] [--name FILE.ply]
                                         [--voxel_length 0.009765625] [--sdf_trunc 0.04]
"""
import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from loopy_slam_amd import config, core, tsdf


def last_checkpoint(output):
    ckpts = sorted(glob.glob(os.path.join(output, 'ckpts', '*.tar')))
    if not ckpts:
        raise ValueError(f'no checkpoint in {os.path.join(output, "ckpts")}')
    return torch.load(ckpts[-1], map_location='cpu', weights_only=False)


def rendered_frames(folder):
    """[(frame index, depth file, colour file)] of a rendered_every_frame folder, ascending."""
    out = []
    for d in sorted(glob.glob(os.path.join(folder, 'depth_*.npy'))):
        idx = int(os.path.splitext(d)[0][-5:])
        out.append((idx, d, os.path.join(folder, f'color_{idx:05d}.npy')))
    return out


def fuse_files(eng, frames, poses, cam, voxel_length, sdf_trunc):
    """cam = (fx, fy, cx, cy) of the (cropped) images."""
    vol = tsdf.TSDFVolume(eng, voxel_length=voxel_length, sdf_trunc=sdf_trunc)
    for idx, depth_file, color_file in frames:
        c2w = poses[idx].float()
        if not bool(torch.isfinite(c2w).all()):
            continue
        vol.integrate(torch.from_numpy(np.load(depth_file).astype(np.float32)), torch.from_numpy(np.load(color_file).astype(np.float32)),
                      c2w, *cam)
    return vol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('config', type=str)
    ap.add_argument('--input_folder', type=str)
    ap.add_argument('--output', type=str)
    ap.add_argument('--name', type=str, help='file name of the mesh (default {scene}_pred_mesh.ply)')
    ap.add_argument('--voxel_length', type=float)
    ap.add_argument('--sdf_trunc', type=float)
    args = ap.parse_args()
    cfg = config.load_config(args.config, os.path.join(ROOT, 'configs', 'point_slam.yaml'))
    if args.input_folder:
        cfg['data']['input_folder'] = args.input_folder
    output = args.output or cfg['data'].get('output', 'output')
    ms = tsdf.settings(cfg)
    c = cfg['cam']
    e = c.get('crop_edge', 0) or 0
    cam = (c['fx'], c['fy'], c['cx'] - e, c['cy'] - e)
    frames = rendered_frames(os.path.join(output, 'rendered_every_frame'))
    if not frames:
        raise ValueError(f'no depth_*.npy in {os.path.join(output, "rendered_every_frame")}')
    vol = fuse_files(core.Engine(), frames, last_checkpoint(output)['estimate_c2w_list'], cam, args.voxel_length or ms['voxel_length'],
                     args.sdf_trunc or ms['sdf_trunc'])
    mesh = vol.extract_triangle_mesh()
    path = os.path.join(output, 'mesh', args.name) if args.name else tsdf.mesh_path(cfg, output)
    tsdf.write_ply(path, mesh)
    print(f'{len(frames)} frames, {vol.n} blocks -> {path}: {mesh["vertices"].shape[0]} vertices, {mesh["triangles"].shape[0]} triangles')


if __name__ == '__main__':
    main()
