"""cfg['meshing'] through the classes (slam.Mapper.run -> tsdf.mesh_run): the mesh file of a short synthetic run, and the off switch."""
import copy
import functools
import atexit
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

from loopy_slam_amd import config, slam
from util import backends, make_engine

torch.set_num_threads(1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mini_cfg(out, meshing):
    """The miniature room of tests/test_slam_api.py at three frames and fewer iterations: what is tested here starts when the run ends."""
    cfg = copy.deepcopy(config.load_config('configs/Synthetic/room.yaml', 'configs/point_slam.yaml'))
    cfg['cam'].update(H=24, W=32, fx=26.0, fy=26.0, cx=15.5, cy=11.5)
    cfg['tracking'].update(ignore_edge_W=2, ignore_edge_H=2, pixels=48, iters=2)
    cfg['mapping'].update(pixels=64, pixels_adding=400, iters=2, iters_first=3, geo_iter_first=1, every_frame=2, keyframe_every=2,
                          mapping_window_size=4)
    cfg['pointcloud'].update(radius_add=0.12, radius_query=0.24, radius_min=0.06)
    cfg['data']['n_frames'] = 3
    cfg['data']['output'] = out
    cfg.pop('meshing', None)
    if meshing is not None:
        cfg['meshing'] = meshing
    return cfg


@functools.lru_cache(maxsize=None)
def run(backend, source):
    """One run per (backend, meshing source); source None = the key absent."""
    out = tempfile.mkdtemp(prefix='loopy_mesh_')
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    meshing = None if source is None else {'enabled': True, 'source': source, 'voxel_length': 0.04}
    ps = slam.Point_SLAM(mini_cfg(out, meshing), None, eng=make_engine(backend))
    est, _ = ps.run()
    return ps, est.clone(), out


def read_ply(path):
    """(vertices [V,3] f32, colours [V,3] u8, triangles [F,3] i32) of a binary little-endian PLY with the properties write_ply writes."""
    with open(path, 'rb') as f:
        assert f.readline() == b'ply\n' and f.readline() == b'format binary_little_endian 1.0\n'
        count, props, cur = {}, {}, None
        for line in iter(f.readline, b'end_header\n'):
            w = line.decode().split()
            if w[0] == 'element':
                cur = w[1]
                count[cur], props[cur] = int(w[2]), []
            elif w[0] == 'property':
                props[cur].append(w[1:])
        assert props['vertex'] == [['float', 'x'], ['float', 'y'], ['float', 'z'], ['uchar', 'red'], ['uchar', 'green'], ['uchar', 'blue']]
        assert props['face'] == [['list', 'uchar', 'int', 'vertex_indices']]
        vert = np.frombuffer(f.read(15 * count['vertex']), dtype=[('p', '<f4', 3), ('c', 'u1', 3)])
        face = np.frombuffer(f.read(13 * count['face']), dtype=[('n', 'u1'), ('i', '<i4', 3)])
        assert f.read() == b'' and (face['n'] == 3).all()
    return vert['p'], vert['c'], face['i']


@pytest.mark.parametrize('backend', backends())
def test_sensor_mesh_file(backend):
    from loopy_slam_amd import tsdf
    ps, _, out = run(backend, 'sensor')
    path = os.path.join(out, 'mesh', 'synthetic_room_pred_mesh.ply')
    assert ps.mapper.mesh_file == path == tsdf.mesh_path(ps.cfg) and os.path.exists(path)
    v, c, t = read_ply(path)
    mesh = tsdf.fuse_run(ps.mapper, 3).extract_triangle_mesh()
    assert len(v) > 500 and len(t) > 500
    assert np.array_equal(v.view(np.uint32), mesh['vertices'].cpu().numpy().view(np.uint32))
    assert np.array_equal(t, mesh['triangles'].cpu().numpy())
    assert np.abs(c.astype(np.float64) / 255.0 - mesh['colors'].cpu().numpy()).max() <= 1.0 / 255.0
    # the surface is the room's: every vertex inside the 6 x 4 x 3 m box grown by its relief (3 cm), one voxel (4 cm) and the pose error a run
    # this short may have (10 cm, the bound of tests/test_slam_api.py)
    assert (np.abs(v) <= np.array([3.0, 2.0, 1.5]) + 0.03 + 0.04 + 0.1).all()


@pytest.mark.parametrize('backend', backends())
def test_rendered_mesh_file(backend):
    ps, _, out = run(backend, 'rendered')
    path = os.path.join(out, 'mesh', 'synthetic_room_pred_mesh.ply')
    assert os.path.exists(path)
    v, c, t = read_ply(path)
    assert np.isfinite(v).all()
    assert t.size == 0 or (t.min() >= 0 and t.max() < len(v))


@pytest.mark.parametrize('backend', backends())
def test_tool_fuses_the_saved_frames(backend):
    """tools/get_mesh_tsdf_fusion.py: the frames the run kept in rendered_every_frame, fused at the run's poses, give the run's mesh."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('get_mesh_tsdf_fusion', os.path.join(ROOT, 'tools', 'get_mesh_tsdf_fusion.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ps, _, out = run(backend, 'rendered')
    frames = tool.rendered_frames(os.path.join(out, 'rendered_every_frame'))
    assert [f[0] for f in frames] == [0, 2]
    vol = tool.fuse_files(ps.eng, frames, ps.estimate_c2w_list, (ps.fx, ps.fy, ps.cx, ps.cy), 0.04, 0.04)
    mesh = vol.extract_triangle_mesh()
    v, c, t = read_ply(os.path.join(out, 'mesh', 'synthetic_room_pred_mesh.ply'))
    assert np.array_equal(v.view(np.uint32), mesh['vertices'].cpu().numpy().view(np.uint32))
    assert np.array_equal(t, mesh['triangles'].cpu().numpy())


@pytest.mark.parametrize('backend', backends())
def test_off_switch(backend):
    off, est_off, out_off = run(backend, None)
    on, est_on, _ = run(backend, 'sensor')
    assert not os.path.exists(os.path.join(out_off, 'mesh')) and not os.path.exists(os.path.join(out_off, 'rendered_every_frame'))
    assert off.mapper.mesh_file is None and not off.mapper.meshing
    assert torch.equal(est_off, est_on)
    for a, b in ((off.npc._pos, on.npc._pos), (off.npc._geo, on.npc._geo), (off.npc._col, on.npc._col)):
        assert off.npc.n == on.npc.n and torch.equal(a[:off.npc.n], b[:on.npc.n])
    disabled = slam.Point_SLAM(mini_cfg(out_off, {'enabled': False}), None, eng=make_engine(backend))
    assert not disabled.mapper.meshing


def test_refuses_several_ranks():
    class Dist:
        rank, world = 0, 2
    cfg = mini_cfg('unused', {'enabled': True})
    ps = slam.Point_SLAM(mini_cfg('unused', None), None, eng=make_engine('emu'))
    ps.dist = Dist()
    with pytest.raises(NotImplementedError, match='world > 1'):
        slam.Mapper(cfg, None, ps)
