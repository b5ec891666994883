"""cfg['rendering_eval'] through the classes (slam.Mapper.run -> render_eval.eval_run): eval/rendering.json of a three-frame synthetic run,
the off switch, the shared render with cfg['meshing'], and tools/eval_rendering.py on the run's files."""
import atexit
import copy
import functools
import importlib.util
import json
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import render_eval_referee as referee
from loopy_slam_amd import config, render_eval, slam, tsdf
from util import backends, make_engine

torch.set_num_threads(1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHING = {'enabled': True, 'source': 'rendered', 'voxel_length': 0.04}


def mini_cfg(out, rendering_eval=None, meshing=None, H=24, W=32):
    """A miniature synthetic room: three frames, frames 0 and 2 mapped, a handful of iterations (what is tested starts when the run ends)."""
    cfg = copy.deepcopy(config.load_config('configs/Synthetic/room.yaml', 'configs/point_slam.yaml'))
    f = 26.0 * W / 32.0
    cfg['cam'].update(H=H, W=W, fx=f, fy=f, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    cfg['tracking'].update(ignore_edge_W=2, ignore_edge_H=2, pixels=48, iters=2)
    cfg['mapping'].update(pixels=64, pixels_adding=400, iters=2, iters_first=3, geo_iter_first=1, every_frame=2, keyframe_every=2,
                          mapping_window_size=4)
    cfg['pointcloud'].update(radius_add=0.12, radius_query=0.24, radius_min=0.06)
    cfg['data']['n_frames'] = 3
    cfg['data']['output'] = out
    for key, val in (('rendering_eval', rendering_eval), ('meshing', meshing)):
        cfg.pop(key, None)
        if val is not None:
            cfg[key] = val
    return cfg


class Run:
    def __init__(self, backend, rendering_eval, meshing, logger=False, H=24, W=32):
        self.out = tempfile.mkdtemp(prefix='loopy_eval_')
        atexit.register(shutil.rmtree, self.out, ignore_errors=True)
        self.ps = ps = slam.Point_SLAM(mini_cfg(self.out, rendering_eval, meshing, H, W), None, eng=make_engine(backend))
        if logger:
            ps.mapper.logger = slam.Logger(ps.cfg, None, ps.mapper)
        self.renders = []
        inner = ps.mapper.renderer.render_img

        def counted(*a, **k):
            self.renders.append(1)
            return inner(*a, **k)
        ps.mapper.renderer.render_img = counted
        est, gt = ps.run()
        ps.mapper.renderer.render_img = inner
        self.est, self.gt = est.clone(), gt.clone()


@functools.lru_cache(maxsize=None)
def run(backend, kind):
    if kind == 'eval':
        return Run(backend, {'enabled': True}, None)
    if kind == 'eval+mesh':
        return Run(backend, {'enabled': True}, MESHING, logger=True)
    if kind == 'mesh':                                    # (and the evaluation switched off by its flag)
        return Run(backend, {'enabled': False}, MESHING)
    return Run(backend, None, None)                       # both keys absent


def rerendered(r, idx):
    ps = r.ps
    _, gt_color, gt_depth, _ = ps.frame_reader[idx]
    depth, color = tsdf.rendered_frame(ps.mapper, idx, gt_color, gt_depth, ps.estimate_c2w_list[idx].float().to(ps.eng.device))
    return gt_color, color, gt_depth, depth


@pytest.mark.parametrize('backend', backends())
def test_rendering_json(backend):
    r = run(backend, 'eval')
    path = os.path.join(r.out, 'eval', 'rendering.json')
    assert os.path.exists(path)
    res = r.ps.mapper.eval_result
    with open(path) as f:
        assert json.load(f) == res
    assert res['frames'] == [0, 2] and len(r.renders) == 2 and res['skipped'] == []
    assert res['ms_ssim'] is None and res['avg_ms_ssim'] is None and '160' in res['ms_ssim_reason'] and '24 x 32' in res['ms_ssim_reason']
    for k, idx in enumerate(res['frames']):
        l1, psnr = referee.figures(referee.record(*rerendered(r, idx), msssim=False))
        assert abs(res['depth_l1'][k] - l1) <= 1e-12 * l1 and abs(res['psnr'][k] - psnr) <= 1e-12 * abs(psnr)
        assert 0.0 < l1 < 3.0 and 0.0 < psnr < 60.0
    assert abs(res['avg_depth_l1'] - np.mean(res['depth_l1'])) <= 1e-15 and abs(res['avg_psnr'] - np.mean(res['psnr'])) <= 1e-13
    for key, align in (('ate', True), ('ate_no_align', False)):
        want = referee.ate(r.ps.estimate_c2w_list.numpy(), r.ps.gt_c2w_list.numpy(), align=align)
        assert tuple(res[key].keys()) == referee.ATE_KEYS and res[key]['compared_pose_pairs'] == 3
        for name in referee.ATE_KEYS:
            assert abs(res[key][name] - want[name]) <= 1e-12


@pytest.mark.parametrize('backend', backends())
def test_off_switch(backend):
    on = run(backend, 'eval')
    for kind in ('off', 'mesh'):                          # the key absent; enabled: False
        off = run(backend, kind)
        assert not os.path.exists(os.path.join(off.out, 'eval'))
        assert off.ps.mapper.eval_result is None and not off.ps.mapper.rendering_eval
        assert torch.equal(off.est, on.est) and torch.equal(off.gt, on.gt)
        assert off.ps.npc.n == on.ps.npc.n
        for a, b in ((off.ps.npc._pos, on.ps.npc._pos), (off.ps.npc._geo, on.ps.npc._geo), (off.ps.npc._col, on.ps.npc._col)):
            assert torch.equal(a[:off.ps.npc.n], b[:on.ps.npc.n])
    assert run(backend, 'off').renders == []


@pytest.mark.parametrize('backend', backends())
def test_one_render_serves_mesh_and_evaluation(backend):
    both, mesh, alone = run(backend, 'eval+mesh'), run(backend, 'mesh'), run(backend, 'eval')
    assert both.ps.mapper.eval_result['frames'] == [0, 2] and len(both.renders) == 2 and len(mesh.renders) == 2
    name = os.path.join('mesh', 'synthetic_room_pred_mesh.ply')
    with open(os.path.join(both.out, name), 'rb') as f, open(os.path.join(mesh.out, name), 'rb') as g:
        data = f.read()
        assert len(data) > 1000 and data == g.read()
    for key in ('depth_l1', 'psnr', 'ate', 'ate_no_align'):
        assert both.ps.mapper.eval_result[key] == alone.ps.mapper.eval_result[key]


@pytest.mark.parametrize('backend', backends())
def test_tool_on_the_run_s_files(backend):
    spec = importlib.util.spec_from_file_location('eval_rendering', os.path.join(ROOT, 'tools', 'eval_rendering.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    r = run(backend, 'eval+mesh')
    assert os.path.exists(os.path.join(r.out, 'ckpts', '00002.tar'))
    with open(os.path.join(r.out, 'eval', 'rendering.json')) as f:
        own = json.load(f)
    os.remove(os.path.join(r.out, 'eval', 'rendering.json'))
    got = tool.evaluate(r.ps.eng, r.ps.cfg, r.out)
    with open(os.path.join(r.out, 'eval', 'rendering.json')) as f:
        assert json.load(f) == got == own == r.ps.mapper.eval_result


def test_refuses_several_ranks():
    class Dist:
        rank, world = 0, 2
    ps = slam.Point_SLAM(mini_cfg('unused'), None, eng=make_engine('emu'))
    ps.dist = Dist()
    with pytest.raises(NotImplementedError, match='world > 1'):
        slam.Mapper(mini_cfg('unused', {'enabled': True}), None, ps)
    slam.Mapper(mini_cfg('unused', {'enabled': False}), None, ps)


@pytest.mark.gpu
def test_msssim_of_a_run():
    """164 x 172: the smallest run whose frames have an MS-SSIM (a 28 000-ray render, too slow for the emulator)."""
    from test_render_eval import bounds
    r = Run('hip', {'enabled': True}, None, H=164, W=172)
    res = r.ps.mapper.eval_result
    assert res['frames'] == [0, 2] and 'ms_ssim_reason' not in res
    for k, idx in enumerate(res['frames']):
        want = referee.combine(referee.record(*rerendered(r, idx)))
        print(f'frame {idx}: ms_ssim {res["ms_ssim"][k]:.6f}, referee {want:.6f}, difference {abs(res["ms_ssim"][k] - want):.3e}')
        assert abs(res['ms_ssim'][k] - want) <= bounds()[1]
    assert abs(res['avg_ms_ssim'] - np.mean(res['ms_ssim'])) <= 1e-15
