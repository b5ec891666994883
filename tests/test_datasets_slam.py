"""A sequence on disk through Point_SLAM: a 12-frame 120 x 160 TUM-layout export of the textured room (tools/export_sequence.py) read by
datasets.TUM_RGBD, against an in-memory reader that holds the same quantised frames; run.py on that export; update_cam with crop_size."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from loopy_slam_amd import config, datasets, slam
from util import make_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import export_sequence as ex  # noqa: E402

torch.set_num_threads(1)
H, W, N = 120, 160, 12
SCALE = 5000.0
# the miniature run of tests/test_slam_api.py at five times its image: more pixels and iterations, the coarse cloud kept
OVERRIDES = dict(
    tracking=dict(ignore_edge_W=4, ignore_edge_H=4, pixels=200, iters=8, lr=0.0005, sample_with_color_grad=False),
    mapping=dict(pixels=300, pixels_adding=1500, pixels_based_on_color_grad=0, iters=8, iters_first=40, geo_iter_first=16, every_frame=2,
                 keyframe_every=4, mapping_window_size=4, color_refine=False),
    pointcloud=dict(radius_add=0.06, radius_query=0.12, radius_min=0.03, radius_add_max=0.08, radius_add_min=0.04),
)


@pytest.fixture(scope='module')
def export(tmp_path_factory):
    folder = str(tmp_path_factory.mktemp('tum_export'))
    # the slow loop of the synthetic end-to-end runs whose band is used below (tests/test_slam_api.py), not the hand-held walk
    frames = ex.synthetic_frames(N, H, W, scene='textured', motion='loop', png_depth_scale=SCALE)
    ex.write_sequence(folder, 'tumrgbd', frames)
    return folder, frames


def run_cfg(folder):
    cfg = copy.deepcopy(config.load_config('configs/TUM_RGBD/freiburg1_desk.yaml', 'configs/point_slam.yaml'))
    cfg['cam'].update(ex.intrinsics(H, W), crop_edge=0, png_depth_scale=SCALE)
    for k, v in OVERRIDES.items():
        cfg[k].update(v)
    cfg['data'].update(input_folder=folder)
    return cfg


class InMemory:
    """The same quantised frames without a file or a kernel in between: c / 255 and d / 5000 in torch, the poses of the reader."""

    def __init__(self, frames, poses, device):
        self.items = [((torch.from_numpy(c.astype(np.float64)) / 255.0).float().to(device),
                       (torch.from_numpy(d.astype(np.float32)) / SCALE).to(device), p.to(device)) for (c, d, _), p in zip(frames, poses)]
        self.n_img = len(self.items)

    def __len__(self):
        return self.n_img

    def __getitem__(self, i):
        c, d, p = self.items[i]
        return i, c, d, p.clone()


class Recording:
    def __init__(self, inner):
        self.inner, self.n_img, self.seen = inner, len(inner), []

    def __len__(self):
        return self.n_img

    def __getitem__(self, i):
        out = self.inner[i]
        self.seen.append(out)
        return out


@pytest.mark.gpu
def test_point_slam_reads_the_sequence(export):
    folder, frames = export
    eng = make_engine('hip')
    cfg = run_cfg(folder)
    ps = slam.Point_SLAM(copy.deepcopy(cfg), None, eng=eng)                      # no dataset handed in: the folder is found and read
    assert isinstance(ps.frame_reader, datasets.TUM_RGBD) and ps.n_img == N
    disk = ps.frame_reader = Recording(ps.frame_reader)
    est_a, gt_a = ps.run()
    memory = Recording(InMemory(frames, disk.inner.poses, eng.device))
    est_b, gt_b = slam.Point_SLAM(copy.deepcopy(cfg), None, eng=eng, dataset=memory).run()
    disk.inner.close()
    # the frames handed to the tracker are the same bits
    assert len(disk.seen) == len(memory.seen) == N
    for a, b in zip(disk.seen, memory.seen):
        assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert torch.equal(gt_a, gt_b)
    # both runs track: finite poses within the band of the synthetic end-to-end runs (tests/test_slam_api.py: 0.1 m of the truth)
    for est, gt in ((est_a, gt_a), (est_b, gt_b)):
        err = (est[:, :3, 3] - gt[:, :3, 3]).norm(dim=1)
        print(f'max |t - t_gt| = {100 * float(err.max()):.2f} cm over {est.shape[0]} frames')
        assert est.shape[0] == N and torch.isfinite(est).all() and float(err.max()) < 0.1


@pytest.mark.gpu
def test_run_py_reads_the_folder(export, tmp_path):
    folder, _ = export
    cfg_file = str(tmp_path / 'export.yaml')
    with open(cfg_file, 'w') as f:
        yaml.safe_dump(dict(inherit_from='configs/TUM_RGBD/freiburg1_desk.yaml', cam=dict(ex.intrinsics(H, W), crop_edge=0, png_depth_scale=SCALE),
                            **OVERRIDES), f)
    r = subprocess.run([sys.executable, 'run.py', cfg_file, '--input_folder', folder, '--stop', '10', '--output', str(tmp_path / 'out')],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'run.py: reading the tumrgbd sequence' in r.stdout and 'TUM_RGBD' in r.stdout and 'NO FRAME READER' not in r.stdout, r.stdout[-2000:]
    assert 'run.py: 11 frames' in r.stdout, r.stdout[-2000:]
    assert os.path.exists(os.path.join(str(tmp_path / 'out'), 'ckpts', '00010.tar'))


def test_a_folder_that_is_no_sequence_gets_the_synthetic_room(tmp_path):
    from test_slam_api import mini_cfg
    cfg = mini_cfg()
    cfg['dataset'] = 'replica'
    cfg['data']['input_folder'] = str(tmp_path)                                  # exists, holds no Replica layout
    ps = slam.Point_SLAM(cfg, None, eng=make_engine('emu'))
    assert isinstance(ps.frame_reader, slam.SyntheticRoomDataset)


def test_update_cam_with_crop_size():
    """Point_SLAM.py:160-175 by hand: 480 x 640 -> crop_size (384, 512) scales by 0.8 in both axes, crop_edge 8 then shifts the centre."""
    from test_slam_api import mini_cfg
    cfg = mini_cfg()
    cfg['cam'].update(H=480, W=640, fx=500.0, fy=520.0, cx=320.0, cy=240.0, crop_size=[384, 512], crop_edge=8)
    ps = slam.Point_SLAM.__new__(slam.Point_SLAM)
    ps.cfg = cfg
    ps.H, ps.W, ps.fx, ps.fy, ps.cx, ps.cy = 480, 640, 500.0, 520.0, 320.0, 240.0
    ps.update_cam()
    assert (ps.H, ps.W) == (384 - 16, 512 - 16)
    assert (ps.fx, ps.fy, ps.cx, ps.cy) == pytest.approx((400.0, 416.0, 256.0 - 8, 192.0 - 8), abs=1e-9)
    assert datasets.output_size(480, 640, [384, 512], 8) == (ps.H, ps.W)
    cfg['cam'].pop('crop_size')
    ps.H, ps.W, ps.fx, ps.fy, ps.cx, ps.cy = 480, 640, 500.0, 520.0, 320.0, 240.0
    ps.update_cam()
    assert (ps.H, ps.W, ps.fx, ps.fy, ps.cx, ps.cy) == (464, 624, 500.0, 520.0, 312.0, 232.0)
