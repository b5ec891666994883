"""Loop-closure kernels (csrc/lk_reg.hip: lk_normals, lk_icp_accumulate, lk_apply_correction) against an fp64 NumPy referee
(tests/lc_referee.py), on the host emulator and, under -m gpu, on the chip.

Input: two 30 000-point clouds cut from one permuted synthetic.build_cloud(60000, seed=5) - one third shared points, the rest different
samples of the same surfaces - the source moved by the inverse of a planted transform.  Bounds:
  correspondences  exact against the fp32 brute-force nearest under (d2, index); with a non-identity transform exact on the points whose
                   decision is not a rounding matter (fp64 nearest / second nearest and max_dist^2 more than 1e-5 relative apart).  On this
                   input 0.4 % of the points ARE rounding matters at 0.3 m (the cloud is made of ray triples at 0.98 / 1.0 / 1.02 x depth: a
                   source point that is the middle of a triple has the triple's two ends in the target, equidistant up to rounding), so
                   these are not dropped but decided by the fp32 contract on the kernel's own fused-multiply-add point; at most 0.1 % of
                   the points may escape both comparisons (measured: none)
  sums             every block within 2e-4 of its largest entry (the bound of tests/test_backward_parity.py), count exact
  repeatability    two calls, equal bits
  normals          valid == (referee count >= 3); angle <= 1e-3 rad where the referee's eigen-gap (l1 - l0) / l2 >= 0.05; at most 10 %
                   of the cloud left out
  correction       <= 5e-6 m against fp64 for |coordinates| <= 8 m; identity rows keep their bits; the rebuilt index answers as a fresh one
"""
import numpy as np
import pytest
import torch

import lc_referee as R
import util
from loopy_slam_amd import _ffi, core
from loopy_slam_amd import loop_closure as LC

TOL = 2e-4
_CACHE = {}


def clouds(n):
    if n not in _CACHE:
        src0, tgt = R.clouds(n)
        nrm, cnt, gap = R.normals(tgt, LC.NORMAL_RADIUS, R.CAMERA)
        _CACHE[n] = (src0, tgt, nrm, cnt, gap)
    return _CACHE[n]


def block_errors(got, ref):
    """Worst |got - ref| / max|ref| per block of the 32 outputs."""
    out = {}
    for name, sl in (('JtJ', slice(0, 21)), ('Jtr', slice(21, 27)), ('sum_d2', slice(28, 29)), ('sum_wr2', slice(29, 30))):
        scale = np.abs(ref[sl]).max()
        out[name] = float(np.abs(got[sl] - ref[sl]).max() / scale) if scale > 0 else float(np.abs(got[sl]).max())
    return out


def fma_point(p32, T32):
    """The kernel's s = fma(T0, x, fma(T1, y, fma(T2, z, T3))) per coordinate, replayed through fp64 and rounded to fp32 after every fma."""
    p = p32.astype(np.float64)
    out = np.empty_like(p32)
    for r in range(3):
        a = (T32[r, 2] * p[:, 2] + T32[r, 3]).astype(np.float32).astype(np.float64)
        a = (T32[r, 1] * p[:, 1] + a).astype(np.float32).astype(np.float64)
        out[:, r] = (T32[r, 0] * p[:, 0] + a).astype(np.float32)
    return out


def check_correspondences(eng, n):
    src0, tgt, _, _, _ = clouds(n)
    tc = LC.SegmentCloud(eng, torch.from_numpy(tgt), R.CAMERA)
    src = eng.f32(src0)
    for max_dist in (0.3, 0.03):
        _, corr = LC.icp_sums(eng, tc, src, np.eye(4), max_dist, mode=_ffi.ICP_INFORMATION, want_corr=True)
        ref, _, _ = R.nearest(tgt, src0, max_dist, need_second=False)
        assert np.array_equal(corr.cpu().numpy().astype(np.int64), ref), max_dist
    # planted transform: the kernel's fused multiply-adds and NumPy round differently
    T = R.planted(*R.DRIFTS[0])
    moved = R.move(src0, R.inv4(T))
    T32 = np.eye(4)
    T32[:3, :4] = T[:3, :4].astype(np.float32)
    s64 = moved.astype(np.float64) @ T32[:3, :3].T + T32[:3, 3]
    for max_dist in (0.3, 0.03):
        _, corr = LC.icp_sums(eng, tc, eng.f32(moved), T, max_dist, mode=_ffi.ICP_INFORMATION, want_corr=True)
        r2 = float(np.float32(max_dist) * np.float32(max_dist))
        ref, d1, d2 = R.nearest(tgt.astype(np.float64), s64, max_dist, dtype=np.float64, r2=max_dist ** 2 * (1 + 2e-5))
        with np.errstate(invalid='ignore'):
            clear = (np.abs(d1 - r2) > 1e-5 * r2) | ~np.isfinite(d1)
        with np.errstate(invalid='ignore'):
            clear &= ~np.isfinite(d2) | ((d2 - d1) > 1e-5 * np.maximum(d2, 1e-300)) | ~np.isfinite(d1)
        ref = np.where(np.isfinite(d1) & (d1 <= r2), ref, -1)
        got = corr.cpu().numpy().astype(np.int64)
        assert np.array_equal(got[clear], ref[clear]), max_dist
        # The points whose decision IS a rounding matter are not dropped: the kernel's own point (its fused multiply-adds replayed through
        # fp64, where the product of two fp32 values is exact) decides them under the fp32 contract.  Only where that replay disagrees
        # (its sum is rounded twice) is a point left out, and then the kernel's choice must still be one of the near-tied candidates.
        s32 = fma_point(moved, T32)
        ref32, _, _ = R.nearest(tgt, s32, max_dist, need_second=False)
        out = ~clear & (got != ref32)
        dk = np.where(got >= 0, ((s64 - tgt.astype(np.float64)[np.maximum(got, 0)]) ** 2).sum(1), np.inf)
        tied = np.where(got >= 0, (dk <= d1 * (1 + 1e-5)) & (dk <= r2 * (1 + 1e-5)), ~np.isfinite(d1) | (d1 >= r2 * (1 - 1e-5)))
        assert tied[out].all()
        left_out = out.mean()
        print(f'correspondences, planted, max_dist {max_dist}: {1.0 - clear.mean():.2e} of the points are rounding matters, '
              f'{left_out:.2e} left out')
        assert left_out <= 1e-3
    # empty target; a source with no match
    empty = LC.SegmentCloud(eng, torch.zeros(0, 3), R.CAMERA)
    s, corr = LC.icp_sums(eng, empty, src[:1000], np.eye(4), 0.3, mode=_ffi.ICP_INFORMATION, want_corr=True)
    assert (corr.cpu().numpy() == -1).all() and not s.any()
    s, corr = LC.icp_sums(eng, tc, src[:1000] + 100.0, np.eye(4), 0.3, want_corr=True)
    assert (corr.cpu().numpy() == -1).all() and not s.any()
    tc.close()


def check_sums(eng, n):
    src0, tgt, _, _, _ = clouds(n)
    tc = LC.SegmentCloud(eng, torch.from_numpy(tgt), R.CAMERA)
    nrm, valid = [x.cpu().numpy() for x in tc.normals]         # the sums are checked on the library's own normals
    T = R.planted(*R.DRIFTS[0])
    moved = R.move(src0, R.inv4(T))
    T32 = np.eye(4)
    T32[:3, :4] = T[:3, :4].astype(np.float32)
    worst = {}
    for label, pts, M, max_dist, k in (('identity plain 0.3', src0, np.eye(4), 0.3, 0.0), ('planted plain 0.03', moved, T32, 0.03, 0.0),
                                       ('planted tukey 0.03', moved, T32, 0.03, 0.01), ('unaligned tukey 0.3', moved, np.eye(4), 0.3, 0.01)):
        got, corr = LC.icp_sums(eng, tc, eng.f32(pts), M, max_dist, k, want_corr=True)
        corr = corr.cpu().numpy().astype(np.int64)
        s64 = pts.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
        d2 = np.where(corr >= 0, ((s64 - tgt.astype(np.float64)[np.maximum(corr, 0)]) ** 2).sum(1), 0.0)
        ref = R.p2p_sums(tgt, nrm, valid, pts, M, corr, d2, k)
        err = block_errors(got, ref)
        print(f'sums, point-to-plane, {label}: count {int(got[27])}, worst error / bound', {a: round(b / TOL, 4) for a, b in err.items()})
        assert got[27] == ref[27] and got[27] > 0 and got[30] == 0 and got[31] == 0
        assert max(err.values()) <= TOL, (label, err)
        worst[label] = max(err.values())
    for label, pts, M in (('identity', src0, np.eye(4)), ('planted', moved, T32)):
        got, corr = LC.icp_sums(eng, tc, eng.f32(pts), M, 0.03, mode=_ffi.ICP_INFORMATION, want_corr=True)
        corr = corr.cpu().numpy().astype(np.int64)
        s64 = pts.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
        d2 = np.where(corr >= 0, ((s64 - tgt.astype(np.float64)[np.maximum(corr, 0)]) ** 2).sum(1), 0.0)
        ref = R.info_sums(tgt, corr, d2)
        err = block_errors(got, ref)
        print(f'sums, information, {label}: count {int(got[27])}, worst error / bound', {a: round(b / TOL, 4) for a, b in err.items()})
        assert got[27] == ref[27] and got[27] == got[20] and not got[21:27].any()
        assert max(err.values()) <= TOL, (label, err)
    tc.close()
    return worst


def check_repeatable(eng, n):
    src0, tgt, _, _, _ = clouds(n)
    tc = LC.SegmentCloud(eng, torch.from_numpy(tgt), R.CAMERA)
    T = R.planted(*R.DRIFTS[1])
    src = eng.f32(R.move(src0, R.inv4(T)))
    for mode, k in ((_ffi.ICP_POINT_TO_PLANE, 0.0), (_ffi.ICP_POINT_TO_PLANE, 0.01), (_ffi.ICP_INFORMATION, 0.0)):
        a, ca = LC.icp_sums(eng, tc, src, T, 0.3, k, mode=mode, want_corr=True)
        b, cb = LC.icp_sums(eng, tc, src, T, 0.3, k, mode=mode, want_corr=True)
        assert a.tobytes() == b.tobytes() and torch.equal(ca, cb)
    n1, v1 = LC.estimate_normals(eng, tc.pos, LC.NORMAL_RADIUS, R.CAMERA, knn=tc.knn)
    n2, v2 = LC.estimate_normals(eng, tc.pos, LC.NORMAL_RADIUS, R.CAMERA, knn=tc.knn)
    assert n1.cpu().numpy().tobytes() == n2.cpu().numpy().tobytes() and torch.equal(v1, v2)
    tc.close()


@pytest.mark.parametrize('backend', util.backends())
def test_correspondences(backend):
    check_correspondences(util.make_engine(backend), 30000)


@pytest.mark.parametrize('backend', util.backends())
def test_sums(backend):
    check_sums(util.make_engine(backend), 30000)


@pytest.mark.parametrize('backend', util.backends())
def test_repeatable(backend):
    check_repeatable(util.make_engine(backend), 30000)


@pytest.mark.gpu
def test_at_size_100k():
    eng = util.make_engine('hip')
    check_correspondences(eng, 100000)
    check_sums(eng, 100000)
    check_repeatable(eng, 100000)


@pytest.mark.parametrize('backend', util.backends())
def test_normals(backend):
    eng = util.make_engine(backend)
    _, tgt, ref, cnt, gap = clouds(30000)
    nrm, valid = LC.estimate_normals(eng, eng.f32(tgt), LC.NORMAL_RADIUS, R.CAMERA)
    nrm, valid = nrm.cpu().numpy().astype(np.float64), valid.cpu().numpy()
    assert np.array_equal(valid != 0, cnt >= 3)
    assert not nrm[valid == 0].any()
    judged = (cnt >= 3) & (gap >= 0.05)
    left_out = 1.0 - judged.mean()
    assert left_out <= 0.10, left_out
    assert np.abs(np.linalg.norm(nrm[valid != 0], axis=1) - 1.0).max() < 1e-5
    cosang = np.clip((nrm[judged] * ref[judged]).sum(1), -1.0, 1.0)
    sinang = np.linalg.norm(np.cross(nrm[judged], ref[judged]), axis=1)
    angle = np.arctan2(sinang, cosang)
    print(f'normals: {left_out:.3%} of the cloud left out, worst angle {angle.max():.2e} rad')
    assert angle.max() <= 1e-3
    # every valid normal faces the camera
    to_cam = np.asarray(R.CAMERA)[None] - tgt.astype(np.float64)
    assert ((nrm * to_cam).sum(1)[valid != 0] >= -1e-6).all()


@pytest.mark.parametrize('backend', util.backends())
def test_apply_correction(backend):
    eng = util.make_engine(backend)
    src0, _, _, _, _ = clouds(30000)
    rng = np.random.RandomState(3)
    pos0 = (src0 * np.float32(8.0 / np.abs(src0).max() * 0.999)).astype(np.float32)        # coordinates up to 8 m
    pos0[:7] = np.float32(-0.0)                                                             # signed zeros must survive an identity row
    n_seg = 5
    seg = rng.randint(0, n_seg, size=len(pos0)).astype(np.int32)
    mats = np.stack([np.eye(4)] + [R.planted(rng.uniform(-3, 3, 3), rng.uniform(-0.2, 0.2, 3)) for _ in range(n_seg - 1)])
    mats[3] = np.eye(4)
    m32 = mats[:, :3, :4].astype(np.float32)
    pos = eng.f32(pos0.copy())
    knn = core.KnnIndex(eng, capacity=len(pos0))
    knn.build(pos)
    seg_t, mats_t = torch.from_numpy(seg).to(eng.device), eng.f32(m32.reshape(n_seg, 12))
    eng.lib.check(eng.lib.dll.lk_apply_correction(_ffi.ptr(pos), len(pos0), _ffi.ptr(seg_t), _ffi.ptr(mats_t), n_seg, eng.stream),
                  'lk_apply_correction')
    got = pos.cpu().numpy()
    m64 = m32.astype(np.float64)
    ref = np.einsum('nij,nj->ni', m64[seg][:, :, :3], pos0.astype(np.float64)) + m64[seg][:, :, 3]
    ident = (seg == 0) | (seg == 3)
    assert got[ident].tobytes() == pos0[ident].tobytes()
    assert np.abs(got.astype(np.float64) - ref)[~ident].max() <= 5e-6
    # the live index after a rebuild answers as a fresh one
    knn.build(pos)
    fresh = core.KnnIndex(eng, capacity=len(pos0))
    fresh.build(pos.clone())
    q = pos[:4000] + 0.01
    a, b = knn.query(q, 0.08 ** 2), fresh.query(q, 0.08 ** 2)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    # a row without a segment stays where it is
    seg_bad = torch.full((10,), 9, dtype=torch.int32, device=eng.device)
    before = pos[:10].clone()
    eng.lib.check(eng.lib.dll.lk_apply_correction(_ffi.ptr(pos), 10, _ffi.ptr(seg_bad), _ffi.ptr(mats_t), n_seg,
                                                  eng.stream), 'lk_apply_correction')
    assert torch.equal(before, pos[:10])
