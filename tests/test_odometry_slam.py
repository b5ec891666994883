"""cfg['tracking']['visual_odometer'] through the classes (slam.Tracker.track_frame -> odometry.VisualOdometer): the starting pose the track
optimiser is handed, the reference's precedence (constant speed first), the fallback to the copied pose, and the off switch - on the
miniature synthetic room of tests/test_slam_api.py with the hand-held walk in the textured scene."""
import copy

import pytest
import torch

from loopy_slam_amd import config, odometry, slam, steps
from loopy_slam_amd.common import get_camera_from_tensor
from util import backends, make_engine

torch.set_num_threads(1)
H, W = 48, 64                                        # twice the miniature room's 24 x 32: at 2 degrees per pixel an odometry has nothing to gain
VO = {'levels': 2, 'iters': [20, 10]}                # 48 x 64 -> 24 x 32; converged (last step 1e-6): the start is a fixed point, not a count
# At a degree per pixel the estimate is worth 0.05 cm on frame 2 (copied pose 0.51 cm) but only 1.00 against 1.08 cm on frame 3; the accuracy
# that the odometry is FOR is held at 120 x 160 in tests/test_odometry_kernels.py::test_estimate.


def mini_cfg(visual_odometer, const_speed, n_frames=4):
    cfg = copy.deepcopy(config.load_config('configs/Synthetic/room.yaml', 'configs/point_slam.yaml'))
    cfg['cam'].update(H=H, W=W, fx=26.0 * W / 32, fy=26.0 * W / 32, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    cfg['tracking'].update(ignore_edge_W=2, ignore_edge_H=2, pixels=48, iters=3, const_speed_assumption=const_speed,
                           lr=0.0002)       # three iterations on 48 rays of an untrained map: a small step keeps the tracked pose near its start
    if visual_odometer is None:
        cfg['tracking'].pop('visual_odometer', None)
    else:
        cfg['tracking']['visual_odometer'] = visual_odometer
    cfg['mapping'].update(pixels=64, pixels_adding=400, iters=3, iters_first=6, geo_iter_first=2, every_frame=2, keyframe_every=2,
                          mapping_window_size=4)
    cfg['pointcloud'].update(radius_add=0.12, radius_query=0.24, radius_min=0.06)
    cfg['data'].update(n_frames=n_frames, motion='handheld', scene='textured')
    return cfg


class Spy:
    """Records the starting pose of every TrackOptimizer.track call and counts VisualOdometer.estimate_pose calls."""

    def __init__(self, monkeypatch):
        self.starts, self.estimates = [], 0
        track, estimate_pose = steps.TrackOptimizer.track, odometry.VisualOdometer.estimate_pose

        def spy_track(to, cam, *a, **k):
            c2w = torch.eye(4)
            c2w[:3] = get_camera_from_tensor(cam.detach().cpu())
            self.starts.append(c2w)
            return track(to, cam, *a, **k)

        def spy_estimate(vo, *a, **k):
            self.estimates += 1
            return estimate_pose(vo, *a, **k)
        monkeypatch.setattr(steps.TrackOptimizer, 'track', spy_track)
        monkeypatch.setattr(odometry.VisualOdometer, 'estimate_pose', spy_estimate)


def t_err(a, b):
    return float((a[:3, 3].double() - b[:3, 3].double()).norm())


@pytest.mark.parametrize('backend', backends())
def test_starting_pose_is_the_odometry_estimate(backend, monkeypatch):
    eng = make_engine(backend)
    spy = Spy(monkeypatch)
    ps = slam.Point_SLAM(mini_cfg(VO, False), None, eng=eng)
    est, gt = ps.run()
    assert len(spy.starts) == 2 and spy.estimates == 2 and ps.tracker.odometry_fallbacks == 0          # frames 2 and 3
    c = ps.cfg['cam']
    direct = odometry.VisualOdometer(eng, dict(H=c['H'], W=c['W'], fx=c['fx'], fy=c['fy'], cx=c['cx'], cy=c['cy']), VO)
    for idx in (0, 1):
        _, color, depth, c2w = ps.frame_reader[idx]
        direct.set_init_state(color, depth, c2w)
    for n, idx in enumerate((2, 3)):
        _, color, depth, c2w = ps.frame_reader[idx]
        direct.update_est_abs_pose(est[idx - 1])
        want = direct.estimate_pose(color, depth)
        assert direct.last_ok and direct.last_record[32] == 0
        got = spy.starts[n]
        print(f'frame {idx}: start {100 * t_err(got, gt[idx]):.3f} cm from the truth, copied pose {100 * t_err(est[idx - 1], gt[idx]):.3f} cm')
        assert torch.allclose(got.double(), want, atol=2e-6, rtol=0)
        assert t_err(got, gt[idx]) < t_err(est[idx - 1], gt[idx])
    assert ps.tracker.odometer.get_last_frame()[1].shape == (c['H'], c['W'])


@pytest.mark.parametrize('backend', backends())
def test_constant_speed_comes_first(backend, monkeypatch):
    eng = make_engine(backend)
    spy = Spy(monkeypatch)
    ps = slam.Point_SLAM(mini_cfg(VO, True), None, eng=eng)
    est, gt = ps.run()
    assert ps.tracker.odometer is not None and spy.estimates == 0 and len(spy.starts) == 2
    for n, idx in enumerate((2, 3)):
        pre, pre2 = est[idx - 1].float(), est[idx - 2].float()
        assert torch.allclose(spy.starts[n], pre @ torch.linalg.inv(pre2) @ pre, atol=2e-6, rtol=0)


class NoDepthAt:
    """The run's frames with the depth of one of them gone."""

    def __init__(self, inner, idx):
        self.inner, self.idx, self.n_img = inner, idx, inner.n_img

    def __len__(self):
        return len(self.inner)

    def __getitem__(self, idx):
        i, color, depth, c2w = self.inner[idx]
        return i, color, (torch.zeros_like(depth) if idx == self.idx else depth), c2w


@pytest.mark.parametrize('backend', backends())
def test_a_frame_without_depth_falls_back(backend, monkeypatch):
    eng = make_engine(backend)
    spy = Spy(monkeypatch)
    cfg = mini_cfg(VO, False)
    frames = NoDepthAt(slam.SyntheticRoomDataset(cfg, eng.device), 3)
    ps = slam.Point_SLAM(cfg, None, eng=eng, dataset=frames)
    est, gt = ps.run()
    vo = ps.tracker.odometer
    assert spy.estimates == 2 and ps.tracker.odometry_fallbacks == 1 and not vo.last_ok
    assert vo.last_record[32] == 1 and vo.last_record[2] == 0
    assert torch.allclose(spy.starts[1], est[2].float(), atol=2e-6, rtol=0)                 # the copied pose (through the quaternion form)
    assert not torch.allclose(spy.starts[0], est[1].float(), atol=1e-4, rtol=0)


def test_off_means_no_odometer():
    eng = make_engine('emu')
    for value in (None, False):
        tr = slam.Point_SLAM(mini_cfg(value, False), None, eng=eng).tracker
        assert tr.odometer is None and tr.odometry_fallbacks == 0
    assert config.load_config('configs/Synthetic/room.yaml', 'configs/point_slam.yaml')['tracking']['visual_odometer'] is False
