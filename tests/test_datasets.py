"""The sequence readers (loopy_slam_amd/datasets.py) on sequences that tools/export_sequence.py writes: layouts, file order, pose conventions,
frames against the referee applied to a Pillow decode of the same files, TUM association, and the decode-ahead thread."""
import copy
import os
import sys
import threading
import types

import numpy as np
import pytest
import torch
from PIL import Image

import datasets_referee as ref
from loopy_slam_amd import config, datasets
from util import backends, make_engine

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import export_sequence as ex  # noqa: E402

torch.set_num_threads(1)
H, W, N = 24, 32, 6
CONFIGS = {'replica': 'configs/Replica/room0.yaml', 'scannet': 'configs/ScanNet/scene0000.yaml', 'azure': 'configs/Replica/room0.yaml',
           'tumrgbd': 'configs/TUM_RGBD/freiburg1_desk.yaml'}
SCANNET_NAMES = [0, 1, 2, 10, 11, 100]              # '10' sorts before '2' as text


@pytest.fixture(scope='module')
def frames():
    out = {}
    for scale in (6553.5, 1000.0, 5000.0):
        out[scale] = ex.synthetic_frames(N, H, W, png_depth_scale=scale)
    return out


def cfg_for(layout, folder, edge=0, prefetch=2):
    cfg = copy.deepcopy(config.load_config(CONFIGS[layout], 'configs/point_slam.yaml'))
    cfg['dataset'] = layout
    cfg['cam'].update(ex.intrinsics(H, W), crop_edge=edge)
    cfg['data'].update(input_folder=str(folder), prefetch=prefetch)
    return cfg


def write(layout, folder, frames, **kw):
    cfg = cfg_for(layout, folder)
    fr = frames[cfg['cam']['png_depth_scale']]
    if layout == 'scannet':
        kw.setdefault('names', SCANNET_NAMES)
    return fr, ex.write_sequence(str(folder), layout, fr, **kw)


def decoded(reader, i):
    return np.array(Image.open(reader.color_paths[i]).convert('RGB')), np.array(Image.open(reader.depth_paths[i]))


def check_frame(reader, i, edge):
    idx, color, depth, c2w = reader[i]
    c8, d16 = decoded(reader, i)
    assert d16.dtype == np.uint16
    want_c, want_d, _ = ref.prepare(c8, d16, reader.png_depth_scale, edge=edge)
    assert idx == i and color.dtype == depth.dtype == c2w.dtype == torch.float32
    assert color.device.type == depth.device.type == c2w.device.type == reader.device.type
    assert np.array_equal(color.cpu().numpy(), want_c.astype(np.float32)) and np.array_equal(depth.cpu().numpy(), want_d)
    return color, depth, c2w


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('layout', list(CONFIGS))
def test_layout_round_trip(backend, layout, frames, tmp_path):
    eng = make_engine(backend)
    edge = 2 if layout == 'scannet' else 0
    fr, written = write(layout, tmp_path, frames)
    reader = datasets.get_dataset(cfg_for(layout, tmp_path, edge), types.SimpleNamespace(input_folder=None), eng=eng)
    assert isinstance(reader, datasets.dataset_dict[layout]) and len(reader) == N == reader.n_img
    if layout == 'scannet':
        assert [int(os.path.basename(p)[:-4]) for p in reader.color_paths] == SCANNET_NAMES
        assert [int(os.path.basename(p)[:-4]) for p in reader.depth_paths] == SCANNET_NAMES
    else:
        assert reader.color_paths == sorted(reader.color_paths) and reader.depth_paths == sorted(reader.depth_paths)
    # poses: the un-negated matrices written come back negated, i.e. as the exporter's c2w; TUM relative to its first frame
    first_inv = np.linalg.inv(written[0])
    for i in range(N):
        want = ref.flip_yz(first_inv @ written[i]) if layout == 'tumrgbd' else fr[i][2]
        assert np.abs(reader.poses[i].double().numpy() - want).max() < 1e-6
        assert reader.poses[i].dtype == torch.float32
    independent = {'replica': lambda: ref.replica_poses(os.path.join(tmp_path, 'traj.txt'), N),
                   'scannet': lambda: ref.scannet_poses(os.path.join(tmp_path, 'frames', 'pose')),
                   'azure': lambda: ref.azure_poses(os.path.join(tmp_path, 'scene', 'trajectory.log'), N),
                   'tumrgbd': lambda: [p for _, _, p in ref.tum_sequence(str(tmp_path))]}[layout]()
    assert len(independent) == N
    for a, b in zip(reader.poses, independent):
        assert np.abs(a.numpy().astype(np.float64) - b.astype(np.float64)).max() < 1e-6
    for i in range(N):
        color, depth, c2w = check_frame(reader, i, edge)
        assert tuple(depth.shape) == (H - 2 * edge, W - 2 * edge) and torch.equal(c2w.cpu(), reader.poses[i])
    if layout == 'tumrgbd':                               # PNG colour: the quantised frame comes back exactly
        _, color, depth, _ = reader[3]
        assert np.array_equal(color.cpu().numpy(), (fr[3][0].astype(np.float64) / 255.0).astype(np.float32))
        assert torch.equal(reader.poses[0], torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0])))        # the identity, columns negated
    reader.close()


def test_azure_without_trajectory_gives_identity_poses(frames, tmp_path):
    write('azure', tmp_path, frames, poses=False)
    reader = datasets.get_dataset(cfg_for('azure', tmp_path), None, eng=make_engine('emu'))
    assert len(reader) == N and all(torch.equal(p, torch.eye(4)) for p in reader.poses)
    assert torch.equal(reader[1][3].cpu(), torch.eye(4))
    reader.close()


def test_args_input_folder_overrides_the_config(frames, tmp_path):
    write('replica', tmp_path, frames)
    cfg = cfg_for('replica', tmp_path / 'nowhere')
    assert datasets.open_sequence(cfg, None, eng=make_engine('emu')) is None
    reader = datasets.open_sequence(cfg, types.SimpleNamespace(input_folder=str(tmp_path)), eng=make_engine('emu'))
    assert isinstance(reader, datasets.Replica) and len(reader) == N
    reader.close()


def test_unknown_dataset_key_lists_the_supported_ones(tmp_path):
    cfg = cfg_for('replica', tmp_path)
    cfg['dataset'] = 'cofusion'
    with pytest.raises(ValueError) as e:
        datasets.get_dataset(cfg, None, eng=make_engine('emu'))
    for name in ('replica', 'scannet', 'azure', 'tumrgbd'):
        assert name in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- TUM lists
def tum_tree(folder, rgb, depth, pose, pose_name='groundtruth.txt'):
    for name, lines in (('rgb.txt', rgb), ('depth.txt', depth), (pose_name, pose)):
        with open(os.path.join(folder, name), 'w') as f:
            f.write('\n'.join(lines) + '\n')


def test_tum_association_on_hand_written_lists(tmp_path):
    q = '0 0 0 1'
    rgb = ['# color images', '# file: hand written', '# timestamp filename',
           '10.000 rgb/a.png',          # depth 10.079 (just inside 0.08), pose 10.01        -> kept, frame 0
           '10.020 rgb/b.png',          # 0.020 s after a kept frame: under 1/32 s           -> thinned
           '10.170 rgb/c.png',          # nearest depth 10.251 is 0.081 away (just outside)  -> no association
           '10.300 rgb/d.png',          # depth 10.30; nearest pose 10.20 is 0.1 away: a gap -> no association
           '10.500 rgb/e.png']          # depth 10.52, pose 10.50                            -> kept, frame 1
    depth = ['# depth maps', '10.079 depth/a.png', '10.251 depth/c.png', '10.300 depth/d.png', '10.520 depth/e.png']
    pose = ['# ground truth trajectory', '# timestamp tx ty tz qx qy qz qw',
            f'10.010 1 2 3 {q}', f'10.200 1 2 3.5 {q}', '10.500 2 2 3 0 0 0.7071067811865476 0.7071067811865476']
    tum_tree(tmp_path, rgb, depth, pose)
    colors, depths, poses = datasets.TUM_RGBD.loadtum(str(tmp_path), frame_rate=32)
    assert [os.path.basename(p) for p in colors] == ['a.png', 'e.png'] and [os.path.basename(p) for p in depths] == ['a.png', 'e.png']
    assert torch.equal(poses[0], torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0])))      # the first pose becomes the identity (columns negated)
    want = np.eye(4)
    want[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]                        # 90 degrees about z
    want[:3, 3] = [1, 0, 0]
    assert np.abs(poses[1].double().numpy() - ref.flip_yz(want)).max() < 1e-6
    mine = ref.tum_sequence(str(tmp_path))
    assert [os.path.basename(c) for c, _, _ in mine] == ['a.png', 'e.png']
    # without thinning the second image is kept too; its nearest depth is a.png again
    colors, depths, _ = datasets.TUM_RGBD.loadtum(str(tmp_path), frame_rate=1000)
    assert [os.path.basename(p) for p in colors] == ['a.png', 'b.png', 'e.png'] and os.path.basename(depths[1]) == 'a.png'
    # pose.txt is read when groundtruth.txt is absent
    os.rename(os.path.join(tmp_path, 'groundtruth.txt'), os.path.join(tmp_path, 'pose.txt'))
    assert len(datasets.TUM_RGBD.loadtum(str(tmp_path), frame_rate=32)[0]) == 2


def test_quaternion_matrix():
    g = np.random.RandomState(0)
    for q in list(g.randn(20, 4)) + [np.array([0, 0, 0, 1.0]), np.array([1.0, 0, 0, 0]), np.array([0, 2.0, 0, 0])]:
        R = datasets.quaternion_matrix(q)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
        assert np.abs(R - ref.quat_matrix(q)).max() < 1e-12
        back = ex.matrix_quaternion(R)
        assert np.abs(datasets.quaternion_matrix(back) - R).max() < 1e-12
        try:
            from scipy.spatial.transform import Rotation
        except ImportError:
            continue
        assert np.abs(R - Rotation.from_quat(q).as_matrix()).max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------- decode-ahead
def decode_threads():
    return [t for t in threading.enumerate() if t.name == 'loopy-frame-decode']


@pytest.mark.parametrize('backend', backends())
def test_prefetch_on_and_off_deliver_identical_tensors(backend, frames, tmp_path):
    eng = make_engine(backend)
    write('replica', tmp_path, frames)
    on = datasets.get_dataset(cfg_for('replica', tmp_path, prefetch=2), None, eng=eng)
    off = datasets.get_dataset(cfg_for('replica', tmp_path, prefetch=0), None, eng=eng)
    assert not decode_threads()                                   # nothing runs before the first frame is asked for
    kept = []
    for i in range(N):
        a, b = on[i], off[i]
        kept.append(a)
        for x, y in zip(a[1:], b[1:]):
            assert torch.equal(x, y)
    assert len(decode_threads()) == 1 and off._fetcher is None
    assert on._fetcher.hits == N - 1 and on._fetcher.misses == 1  # frame 0 opens the sequence, the others were decoded ahead
    for i, a in enumerate(kept):                                  # a frame handed out is not overwritten by later ones
        assert torch.equal(a[1], off[i][1]) and torch.equal(a[2], off[i][2])
    # out of order: decoded on the spot, then the ring follows the new position
    for i in (4, 1, 2, 3, 0, 5, 5):
        a, b = on[i], off[i]
        assert a[0] == i and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    with pytest.raises(IndexError):
        on[N]
    thread = on._fetcher.thread
    on.close()
    assert not thread.is_alive() and not decode_threads()
    assert torch.equal(on[2][1], off[2][1])                       # a closed reader opens again on demand
    on.close()
    off.close()
    assert not decode_threads()


def test_a_corrupt_file_raises_and_the_thread_goes_on(frames, tmp_path):
    write('replica', tmp_path, frames)
    bad = os.path.join(tmp_path, 'results', 'depth000002.png')
    with open(bad, 'r+b') as f:
        f.truncate(20)
    for prefetch in (2, 0):
        reader = datasets.get_dataset(cfg_for('replica', tmp_path, prefetch=prefetch), None, eng=make_engine('emu'))
        reader[0], reader[1]
        with pytest.raises(Exception) as e:
            reader[2]
        assert not isinstance(e.value, (IndexError, AssertionError))
        check_frame(reader, 3, 0)                                 # the reader, and its thread, still serve the next frame
        check_frame(reader, 4, 0)
        if prefetch:
            assert reader._fetcher.thread.is_alive()
        reader.close()
    assert not decode_threads()
