#!/usr/bin/env python3
"""The reference's src/tools/eval_recon.py: accuracy, completion, completion ratio, precision / recall / F-score at 1 cm (-3d) and the depth
L1 of the two meshes rendered from random views inside the ground truth's bounding box (-2d), printed as one dict.  The reconstruction is
first aligned to the ground truth by point-to-point ICP over the vertices unless --no_align.  With -2d, views that see a point of
{gt_mesh minus .ply}_pc_unseen.npy are drawn again, if that file exists (the reference requires it).  loopy_slam_amd/mesh_eval.py; needs the
GPU.

    python tools/eval_recon.py --rec_mesh REC.ply --gt_mesh GT.ply [-2d] [-3d] [--no_align] [--n_samples 200000] [--n_views 1000] [--seed 0]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from loopy_slam_amd import mesh_eval


def main(argv=None):
    ap = argparse.ArgumentParser(description='Arguments to evaluate the reconstruction.')
    ap.add_argument('--rec_mesh', type=str, required=True, help='reconstructed mesh file path')
    ap.add_argument('--gt_mesh', type=str, required=True, help='ground truth mesh file path')
    ap.add_argument('-2d', '--metric_2d', action='store_true', help='enable 2D metric')
    ap.add_argument('-3d', '--metric_3d', action='store_true', help='enable 3D metric')
    ap.add_argument('--no_align', default=False, action='store_true', help='do not align the two meshes first')
    ap.add_argument('--n_samples', type=int, default=200_000)
    ap.add_argument('--n_views', type=int, default=1000)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args(argv)
    rec, gt = mesh_eval.read_ply(args.rec_mesh), mesh_eval.read_ply(args.gt_mesh)
    if not args.no_align:
        rec = mesh_eval.transform(rec, mesh_eval.align(rec, gt)['T'])
    result = {}
    if args.metric_3d:
        result.update(mesh_eval.metrics_3d(rec, gt, n_samples=args.n_samples, seed=args.seed, align=False))
    if args.metric_2d:
        unseen_file = args.gt_mesh.replace('.ply', '_pc_unseen.npy')
        unseen = np.load(unseen_file) if os.path.exists(unseen_file) else None
        views = mesh_eval.sample_views(gt, args.n_views, seed=args.seed, unseen=unseen)
        result.update(mesh_eval.metric_2d(rec, gt, views))
    print(result)


if __name__ == '__main__':
    main()
