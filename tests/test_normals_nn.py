"""lk_normals_nn (csrc/lk_normals_nn.hip): normals over the max_nn nearest neighbours within a radius, against the NumPy referee
tests/normals_nn_referee.py, on the host emulator and, under -m gpu, on the chip.

  selection      out_count and out_nbr equal the referee's element for element - the contract distance is fp32 with one rounding per
                 operation and the order (d2, index) is total, so there is nothing to tolerate.  Inputs: (a) a lattice slab
                 {0..23} x {0..23} x {0,1} x 0.01 m, ties at every rank (what the vertices of a TSDF volume look like), (b) the target of
                 lc_referee.clouds(30000), (c) eight isolated points and one pair
  normals        valid == (referee count >= 3); angle to the fp64 normal over the SAME selection <= 1e-3 rad where the referee's eigen-gap
                 (l1 - l0) / l2 >= 0.05, at most 10 % of the cloud under the gap rule (the bound and the rule of
                 tests/test_loop_closure_kernels.py::test_normals).  Input (b) at max_nn 16 and 50: 3.1 % and 2.7 % fall under the rule
  never binding  max_nn = 64 on a cloud thinned until no ball holds more than 64 points: valid equals lk_normals', normals within 1e-3 rad
  repeatability  equal bits from two calls, and after the index is built again over the same array
  arguments      max_nn 0 and 65 and radius 0 are LK_ERR_ARG, N = 0 is a no-op, NULL out_count / out_nbr are accepted
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lc_referee as R
import normals_nn_referee as NR
import util
from loopy_slam_amd import _ffi, core
from loopy_slam_amd import loop_closure as LC

RADIUS = LC.NORMAL_RADIUS
ANGLE, GAP, LEFT_OUT = 1e-3, 0.05, 0.10


def lattice():
    g = np.stack(np.meshgrid(np.arange(24), np.arange(24), np.arange(2), indexing='ij'), -1).reshape(-1, 3)
    return np.ascontiguousarray(g.astype(np.float32) * np.float32(0.01))


def isolated():
    """Eight points 0.5 m apart and a ninth 0.03 m from the first: counts 2, 1 x 7, 2 - nobody has a normal."""
    p = np.array([[0.5 * (k & 1), 0.5 * ((k >> 1) & 1), 0.5 * (k >> 2)] for k in range(8)] + [[0.03, 0.0, 0.0]], dtype=np.float32)
    return np.ascontiguousarray(p + np.float32(0.123))


@functools.lru_cache(maxsize=None)
def cloud_b():
    return R.clouds(30000)[1]


@functools.lru_cache(maxsize=None)
def referee_b(max_nn):
    """(count, nbr, n_in_radius, normals, gap) of input (b): computed once per max_nn, shared, never written to."""
    count, nbr, n_in = NR.select(cloud_b(), RADIUS, max_nn)
    nrm, gap = NR.normals(cloud_b(), nbr, count, R.CAMERA)
    return count, nbr, n_in, nrm, gap


def run(eng, p, max_nn, radius=RADIUS, camera=R.CAMERA):
    pos = eng.f32(p)
    knn = core.KnnIndex(eng, capacity=max(len(p), 1), cell_size=radius)
    knn.build(pos)
    try:
        out = [x.cpu().numpy() for x in LC.normals_nn(eng, pos, knn, radius, max_nn, camera)]
    finally:
        knn.close()
    return out


def check_selection(got_count, got_nbr, ref_count, ref_nbr):
    assert np.array_equal(got_count.astype(np.int64), ref_count)
    assert np.array_equal(got_nbr.astype(np.int64), ref_nbr)


def check_normals(nrm, valid, pos, ref_count, ref_nrm, gap, camera, label):
    nrm = nrm.astype(np.float64)
    assert np.array_equal(valid != 0, ref_count >= 3)
    assert not nrm[valid == 0].any()
    judged = (ref_count >= 3) & (gap >= GAP)
    left_out = 1.0 - judged.mean()
    assert np.abs(np.linalg.norm(nrm[valid != 0], axis=1) - 1.0).max() < 1e-5
    ang = NR.angle(nrm[judged], ref_nrm[judged])
    print(f'normals, {label}: {left_out:.3%} of the cloud under the gap rule, worst angle {ang.max():.2e} rad')
    assert left_out <= LEFT_OUT, left_out
    assert ang.max() <= ANGLE
    to_cam = np.asarray(camera, dtype=np.float64)[None] - pos.astype(np.float64)
    assert ((nrm * to_cam).sum(1)[valid != 0] >= -1e-6).all()           # every valid normal faces the camera


# ---------------------------------------------------------------------------------------------------- 1. selection
@pytest.mark.parametrize('max_nn', (1, 3, 16, 50, 64))
@pytest.mark.parametrize('backend', util.backends())
def test_selection_lattice(backend, max_nn):
    eng = util.make_engine(backend)
    p = lattice()
    assert len(p) == 1152
    ref_count, ref_nbr = NR.select_brute(p, RADIUS, max_nn)
    grid_count, grid_nbr, n_in = NR.select(p, RADIUS, max_nn)
    assert np.array_equal(ref_count, grid_count) and np.array_equal(ref_nbr, grid_nbr)      # the referee's two forms agree
    assert n_in.min() > 64                                              # every ball is over the cap: ties decide every rank
    _, _, count, nbr = run(eng, p, max_nn)
    check_selection(count, nbr, ref_count, ref_nbr)
    assert (nbr[:, 0] == np.arange(len(p))).all()                       # d2 = 0: the point itself comes first


@pytest.mark.parametrize('max_nn', (16, 50))
@pytest.mark.parametrize('backend', util.backends())
def test_selection_cloud(backend, max_nn):
    eng = util.make_engine(backend)
    ref_count, ref_nbr, n_in, _, _ = referee_b(max_nn)
    binding = n_in > max_nn
    print(f'selection, cloud (b), max_nn {max_nn}: the cap binds on {binding.sum()} of {len(binding)} points '
          f'(candidates per ball: mean {n_in.mean():.1f}, max {n_in.max()})')
    assert binding.any() and not binding.all()
    _, _, count, nbr = run(eng, cloud_b(), max_nn)
    check_selection(count, nbr, ref_count, ref_nbr)


@pytest.mark.parametrize('backend', util.backends())
def test_selection_isolated(backend):
    eng = util.make_engine(backend)
    p = isolated()
    ref_count, ref_nbr = NR.select_brute(p, RADIUS, 50)
    assert ref_count.tolist() == [2, 1, 1, 1, 1, 1, 1, 1, 2]
    nrm, valid, count, nbr = run(eng, p, 50)
    check_selection(count, nbr, ref_count, ref_nbr)
    assert not valid.any() and not nrm.any()


def test_referee_gap_share_cpu():
    """The referee alone: input (b) stays within the 10 % the gap rule may leave out at each max_nn used (measured 3.1 % at 16, 2.7 % at 50)."""
    for max_nn in (16, 50):
        count, _, _, _, gap = referee_b(max_nn)
        left_out = 1.0 - ((count >= 3) & (gap >= GAP)).mean()
        print(f'referee, cloud (b), max_nn {max_nn}: {left_out:.3%} under the gap rule')
        assert left_out <= LEFT_OUT


# ---------------------------------------------------------------------------------------------------- 2. normals
@pytest.mark.parametrize('max_nn', (16, 50))
@pytest.mark.parametrize('backend', util.backends())
def test_normals(backend, max_nn):
    eng = util.make_engine(backend)
    ref_count, _, _, ref_nrm, gap = referee_b(max_nn)
    nrm, valid, _, _ = run(eng, cloud_b(), max_nn)
    check_normals(nrm, valid, cloud_b(), ref_count, ref_nrm, gap, R.CAMERA, f'cloud (b), max_nn {max_nn}')


# ---------------------------------------------------------------------------------------------------- 3. a cap that never binds
@functools.lru_cache(maxsize=None)
def thinned():
    """Input (b) thinned until no 0.1-m ball holds more than 64 points: points are dropped from the fullest balls first."""
    p = cloud_b()
    for _ in range(20):
        _, _, n_in = NR.select(p, RADIUS, 1)
        if n_in.max() <= 64:
            break
        keep = np.ones(len(p), dtype=bool)
        keep[np.nonzero(n_in > 48)[0][::2]] = False
        p = np.ascontiguousarray(p[keep])
    assert n_in.max() <= 64 and len(p) > 10000
    return p


@pytest.mark.parametrize('backend', util.backends())
def test_cap_that_never_binds(backend):
    eng = util.make_engine(backend)
    p = thinned()
    nrm_nn, valid_nn, count, _ = run(eng, p, 64)
    nrm_all, valid_all = [x.cpu().numpy() for x in LC.estimate_normals(eng, eng.f32(p), RADIUS, R.CAMERA)]
    assert np.array_equal(valid_nn, valid_all)
    ref_count, ref_nbr, n_in = NR.select(p, RADIUS, 64)
    assert np.array_equal(count.astype(np.int64), n_in)                # nothing was cut
    _, gap = NR.normals(p, ref_nbr, ref_count, R.CAMERA)
    judged = (ref_count >= 3) & (gap >= GAP)
    assert 1.0 - judged.mean() <= LEFT_OUT
    ang = NR.angle(nrm_nn[judged], nrm_all[judged])
    print(f'cap never binding: {len(p)} points, at most {n_in.max()} per ball, worst angle between the two kernels {ang.max():.2e} rad')
    assert ang.max() <= ANGLE


# ---------------------------------------------------------------------------------------------------- 4. repeatability
@pytest.mark.parametrize('backend', util.backends())
def test_repeatable(backend):
    """The lattice (every rank a tie) at max_nn 50 and the first 10 000 points of cloud (b) at max_nn 8 (the cap binds on about half)."""
    eng = util.make_engine(backend)
    for p, max_nn in ((lattice(), 50), (cloud_b()[:10000], 8)):
        pos = eng.f32(p)
        knn = core.KnnIndex(eng, capacity=len(p), cell_size=RADIUS)
        knn.build(pos)
        a = [x.cpu().numpy().tobytes() for x in LC.normals_nn(eng, pos, knn, RADIUS, max_nn, R.CAMERA)]
        b = [x.cpu().numpy().tobytes() for x in LC.normals_nn(eng, pos, knn, RADIUS, max_nn, R.CAMERA)]
        assert a == b
        knn.build(pos)                                                  # the cells' inner order is whatever the build's atomics left
        c = [x.cpu().numpy().tobytes() for x in LC.normals_nn(eng, pos, knn, RADIUS, max_nn, R.CAMERA)]
        knn.close()
        assert a == c


# ---------------------------------------------------------------------------------------------------- 5. arguments
@pytest.mark.parametrize('backend', util.backends())
def test_arguments(backend):
    eng = util.make_engine(backend)
    dll = eng.lib.dll
    p = lattice()
    pos = eng.f32(p)
    N = len(p)
    knn = core.KnnIndex(eng, capacity=N, cell_size=RADIUS)
    knn.build(pos)
    cam = (C.c_float * 3)(0.0, 0.0, 0.0)
    nrm, valid = eng.zeros(N, 3), eng.zeros(N, dtype=torch.uint8)

    def call(n, radius, max_nn, count=None, nbr=None, index=knn):
        return dll.lk_normals_nn(index.h, _ffi.ptr(pos), n, C.c_float(radius), max_nn, cam, _ffi.ptr(nrm), _ffi.ptr(valid), _ffi.ptr(count),
                                 _ffi.ptr(nbr), eng.stream)
    assert _ffi.NORMALS_MAX_NN == 64
    for max_nn in (0, 65, -1):
        assert call(N, RADIUS, max_nn) == -1                            # LK_ERR_ARG
    assert call(N, 0.0, 50) == -1 and call(N, -0.1, 50) == -1
    assert call(N - 1, RADIUS, 50) == -1                                # not the size of the index
    assert not nrm.cpu().numpy().any() and not valid.cpu().numpy().any()            # a refused call writes nothing
    # N = 0: a no-op on an empty index
    empty = core.KnnIndex(eng, capacity=1, cell_size=RADIUS)
    empty.build(pos[:0])
    count = torch.full((4,), 77, dtype=torch.int32, device=eng.device)
    assert call(0, RADIUS, 50, count=count, index=empty) == 0
    assert call(0, RADIUS, 0, index=empty) == -1                        # the arguments are checked first
    empty.close()
    assert (count.cpu().numpy() == 77).all() and not nrm.cpu().numpy().any()
    # NULL out_count / out_nbr, each alone and both
    ref_count, ref_nbr = NR.select_brute(p, RADIUS, 16)
    assert call(N, RADIUS, 16) == 0
    both = nrm.cpu().numpy().copy()
    assert valid.cpu().numpy().all() and both.any()
    count, nbr = torch.zeros(N, dtype=torch.int32, device=eng.device), torch.zeros(N, 16, dtype=torch.int32, device=eng.device)
    assert call(N, RADIUS, 16, count=count) == 0 and np.array_equal(count.cpu().numpy(), ref_count)
    assert call(N, RADIUS, 16, nbr=nbr) == 0 and np.array_equal(nbr.cpu().numpy(), ref_nbr)
    assert nrm.cpu().numpy().tobytes() == both.tobytes()
    knn.close()


# ---------------------------------------------------------------------------------------------------- at size
@pytest.mark.gpu
def test_at_size():
    """The extracted surface cloud of one fused 'furnished' segment at the reference's voxel (5/512 m, truncation 0.04 m): eight frames of
    240 x 320 along the loop.  The kernel runs on the whole cloud; selection and normals are checked on a random 20 000-point subset of the queries (the
    subset is for the referee's sake)."""
    from loopy_slam_amd import synthetic, tsdf
    eng = util.make_engine('hip')
    intr = dict(H=240, W=320, fx=258.65, fy=258.25, cx=159.3, cy=127.65)
    frames = [synthetic.render_frame(k, intr=intr, holes=0.01, scene='furnished') for k in range(0, 40, 5)]
    vol = tsdf.fuse_segment(eng, [(d, c) for d, c, _ in frames], [p for _, _, p in frames], intr['fx'], intr['fy'], intr['cx'], intr['cy'])
    pos = vol.extract_point_cloud()['vertices'].contiguous()
    camera = frames[0][2][:3, 3].numpy().astype(np.float64)
    N = int(pos.shape[0])
    assert N > 100_000
    knn = core.KnnIndex(eng, capacity=N, cell_size=RADIUS)
    knn.build(pos)
    nrm, valid, count, nbr = [x.cpu().numpy() for x in LC.normals_nn(eng, pos, knn, RADIUS, 50, camera)]
    knn.close()
    p = pos.cpu().numpy()
    q = np.sort(np.random.RandomState(7).choice(N, 20000, replace=False))
    ref_count, ref_nbr, n_in = NR.select(p, RADIUS, 50, queries=q, chunk=500)
    print(f'at size: {N} vertices, candidates per 0.1-m ball: mean {n_in.mean():.0f}, max {n_in.max()}; the cap of 50 binds on '
          f'{(n_in > 50).mean():.1%} of the queries')
    check_selection(count[q], nbr[q], ref_count, ref_nbr)
    ref_nrm, gap = NR.normals(p, ref_nbr, ref_count, camera, queries=q)
    check_normals(nrm[q], valid[q], p[q], ref_count, ref_nrm, gap, camera, 'fused surface, max_nn 50')
