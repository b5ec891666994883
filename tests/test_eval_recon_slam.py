"""End to end: the furnished room's three frames fused twice - at their true poses, and with one pose 2 cm off - and judged by
loopy_slam_amd/mesh_eval.py against the first mesh; and the two command-line tools on the written PLY files (they load the product library,
so that part needs the GPU)."""
import ast
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from util import backends, make_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTR = dict(H=60, W=80, fx=60.0, fy=60.0, cx=39.5, cy=29.5)
CAM = (INTR['fx'], INTR['fy'], INTR['cx'], INTR['cy'])
VOXEL, TRUNC = 0.04, 0.08
FRAMES = (0, 40, 80)
N_SAMPLES = 20_000
VIEW = dict(H=48, W=48, focal=30.0)


@functools.lru_cache(maxsize=None)
def frames():
    from loopy_slam_amd import synthetic
    return [synthetic.render_frame(k, intr=INTR, holes=0.01, scene='furnished') for k in FRAMES]


@functools.lru_cache(maxsize=None)
def meshes(backend):
    """(mesh at the true poses, mesh with the middle frame's pose moved by 2 cm), device tensors of `backend`."""
    from loopy_slam_amd.tsdf import TSDFVolume
    eng = make_engine(backend)
    out = []
    for shift in (0.0, 0.02):
        vol = TSDFVolume(eng, voxel_length=VOXEL, sdf_trunc=TRUNC)
        for k, (depth, color, c2w) in enumerate(frames()):
            c2w = c2w.clone()
            if k == 1:
                c2w[:3, 3] += shift * torch.tensor([0.6, 0.0, 0.8])
            vol.integrate(depth, color, c2w, *CAM)
        out.append(vol.extract_triangle_mesh())
    return eng, out[0], out[1]


@pytest.mark.parametrize('backend', backends())
def test_metrics_tell_the_two_fusions_apart(backend):
    from loopy_slam_amd import mesh_eval as E
    eng, good, bad = meshes(backend)
    assert len(good['triangles']) > 5000 and len(bad['triangles']) > 5000
    m_good = E.metrics_3d(good, good, n_samples=N_SAMPLES, seed=0, align=False, eng=eng)
    m_bad = E.metrics_3d(bad, good, n_samples=N_SAMPLES, seed=0, align=False, eng=eng)
    print('self:', {k: round(v, 4) for k, v in m_good.items()})
    print('2 cm:', {k: round(v, 4) for k, v in m_bad.items()})
    assert all(np.isfinite(v) for v in list(m_good.values()) + list(m_bad.values()))
    assert m_good['accuracy'] < m_bad['accuracy'] and m_good['f-score'] > m_bad['f-score']
    assert m_good['completion'] < m_bad['completion']
    views = E.sample_views(good, 5, seed=0, eng=eng, **VIEW)
    assert views.shape == (5, 4, 4)
    l_good, l_bad = E.metric_2d(good, good, views, eng=eng, **VIEW)['depth l1'], E.metric_2d(bad, good, views, eng=eng, **VIEW)['depth l1']
    print(f'depth l1: self {l_good:.5f} cm, 2 cm {l_bad:.5f} cm')
    assert np.isfinite(l_good) and np.isfinite(l_bad) and l_good == 0.0 and l_bad > l_good
    # the alignment undoes most of a rigid offset of the whole mesh
    moved = E.transform(good, np.array([[1, 0, 0, 0.01], [0, 1, 0, -0.01], [0, 0, 1, 0.005], [0, 0, 0, 1.0]]), eng)
    m_raw = E.metrics_3d(moved, good, n_samples=N_SAMPLES, seed=0, align=False, eng=eng)
    m_al = E.metrics_3d(moved, good, n_samples=N_SAMPLES, seed=0, align=True, eng=eng)
    print(f"accuracy of a 1.5 cm offset: raw {m_raw['accuracy']:.4f} cm, aligned {m_al['accuracy']:.4f} cm, self {m_good['accuracy']:.4f} cm")
    # (the moved mesh has the same vertices, so the fit has an exact answer; what remains is the sampling distance of 20 000 samples)
    assert m_al['accuracy'] < m_raw['accuracy'] and m_al['f-score'] > m_raw['f-score']
    assert abs(m_al['accuracy'] - m_good['accuracy']) < 0.01


def _dict_of(stdout):
    line = [l for l in stdout.strip().splitlines() if l.startswith('{')][-1]
    return ast.literal_eval(line.replace('nan', 'None'))


@pytest.mark.gpu
def test_tools_on_written_files(tmp_path):
    from loopy_slam_amd import mesh_eval as E
    from loopy_slam_amd.tsdf import write_ply
    eng, good, bad = meshes('hip')
    rec, gt = str(tmp_path / 'rec.ply'), str(tmp_path / 'gt.ply')
    write_ply(rec, bad)
    write_ply(gt, good)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'eval_recon.py'), '--rec_mesh', rec, '--gt_mesh', gt, '-2d', '-3d',
                        '--no_align', '--n_samples', str(N_SAMPLES), '--n_views', '5'], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _dict_of(r.stdout)
    assert set(d) == {'accuracy', 'completion', 'completion ratio', 'precision', 'recall', 'f-score', 'depth l1'}
    here = E.metrics_3d(E.read_ply(rec), E.read_ply(gt), n_samples=N_SAMPLES, seed=0, align=False, eng=eng)
    assert all(d[k] == here[k] for k in here), (d, here)              # the same kernels on the same files: the same bits
    assert d['depth l1'] is not None and d['depth l1'] > 0
    # cull: the three poses in the datasets' axes (y down, z forward), the frames' intrinsics
    traj, out = str(tmp_path / 'traj.txt'), str(tmp_path / 'culled.ply')
    poses = np.stack([c2w.numpy().astype(np.float64) for _, _, c2w in frames()])
    with open(traj, 'w') as f:
        for p in poses:
            q = p.copy()
            q[:3, 1] *= -1.0
            q[:3, 2] *= -1.0
            f.write(' '.join(repr(float(x)) for x in q.ravel()) + '\n')
    cam = ['--H', '40', '--W', '56', '--fx', '60', '--fy', '60', '--cx', '27.5', '--cy', '19.5']
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'cull_mesh.py'), '--input_mesh', gt, '--traj', traj, '--output_mesh', out]
                       + cam, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _dict_of(r.stdout)
    culled = E.read_ply(out)
    here = E.cull(E.read_ply(gt), poses, 40, 56, 60.0, 60.0, 27.5, 19.5, compact=True, eng=eng)
    assert d['poses'] == 3 and 0 < d['faces out'] < d['faces in'] == len(good['triangles'])
    assert torch.equal(culled['vertices'], here['vertices'].cpu()) and torch.equal(culled['triangles'], here['triangles'].cpu())
