#!/usr/bin/env python3
"""The reference's src/tools/cull_mesh.py: removes the faces of a mesh that no camera of a trajectory sees (a face stays if one of its
vertices projects into an image).  The trajectory file holds one camera-to-world matrix per line as 16 numbers, row-major, in the datasets'
axes (y down, z forward: the Replica traj.txt); the intrinsics default to Replica's.  loopy_slam_amd/mesh_eval.py; needs the GPU.

    python tools/cull_mesh.py --input_mesh IN.ply --traj traj.txt --output_mesh OUT.ply [--H 680 --W 1200 --fx 600 --fy 600 --cx 599.5 --cy 339.5]
                              [--keep_vertices]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from loopy_slam_amd import mesh_eval, tsdf


def load_poses(path):
    """[K,4,4] f64 in the project's camera convention: columns 1 and 2 of every matrix negated, as the reference's load_poses does."""
    poses = []
    with open(path) as f:
        for line in f:
            w = line.split()
            if not w:
                continue
            c2w = np.array(list(map(float, w)), dtype=np.float64).reshape(4, 4)
            c2w[:3, 1] *= -1.0
            c2w[:3, 2] *= -1.0
            poses.append(c2w)
    return np.stack(poses) if poses else np.zeros((0, 4, 4))


def main(argv=None):
    ap = argparse.ArgumentParser(description='Arguments to cull the mesh.')
    ap.add_argument('--input_mesh', type=str, required=True, help='path to the mesh to be culled')
    ap.add_argument('--traj', type=str, required=True, help='path to the trajectory')
    ap.add_argument('--output_mesh', type=str, required=True, help='path to the output mesh')
    ap.add_argument('--H', type=int, default=680)
    ap.add_argument('--W', type=int, default=1200)
    ap.add_argument('--fx', type=float, default=600.0)
    ap.add_argument('--fy', type=float, default=600.0)
    ap.add_argument('--cx', type=float, default=599.5)
    ap.add_argument('--cy', type=float, default=339.5)
    ap.add_argument('--keep_vertices', action='store_true', help='keep unreferenced vertices, as the reference does')
    args = ap.parse_args(argv)
    mesh = mesh_eval.read_ply(args.input_mesh)
    poses = load_poses(args.traj)
    out = mesh_eval.cull(mesh, poses, args.H, args.W, args.fx, args.fy, args.cx, args.cy, compact=not args.keep_vertices)
    if 'colors' not in out:
        out['colors'] = torch.full_like(out['vertices'], 0.7)
    tsdf.write_ply(args.output_mesh, out)
    print({'poses': int(len(poses)), 'vertices in': int(mesh['vertices'].shape[0]), 'faces in': int(mesh['triangles'].shape[0]),
           'vertices out': int(out['vertices'].shape[0]), 'faces out': int(out['triangles'].shape[0])})


if __name__ == '__main__':
    main()
