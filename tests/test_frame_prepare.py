"""lk_frame_prepare (csrc/lk_frame.hip) against tests/datasets_referee.py, on the host emulator and on the chip.

What is exact and what is bounded
  * colour -> float and depth -> float are single correctly rounded fp32 divisions: bit-exact against the referee rounded to fp32, and so is
    every case without a float resampling (crop_edge is an offset).  The undistortion is integer arithmetic on double coordinates evaluated in
    the contract's operation order: its uint8 image is bit-exact.  Nearest-neighbour depth is bit-exact.
  * a float resampling stage (resize to the depth size, crop_size) is held to a first-order bound in u = 2^-24 on values in [0, 1]:
      inputs    p = fl(c / 255) carries eps_in <= u (a later stage inherits the earlier stage's bound);
      fraction  the source cell is an integer quotient (exact), the fraction f = fl(r / d) is off by <= u f <= u, g = fl(1 - f) by <= u more;
                through g p0 + f p1 that is <= u |p1 - p0| + u p0 <= 2 u: the coordinate's rounding times the local gradient (<= 1 per pixel);
      one lerp  two products and one sum, each <= u times a value <= 1 - together <= 2 u on the convex combination;
    so one lerp adds 4 u and a bilinear tap pair (a lerp of two lerps) adds 8 u: ONE STAGE <= eps_in + 8 u = 9 u, TWO STAGES (every crop_size
    tap composed of four resize taps) <= 9 u + 8 u = 17 u.  The referee works in float64 (its own error is ~1e-16), and the output is
    compared with it unrounded.  Source cells agree: a float64 source coordinate is within 1e-12 of the rational one, and at an integer
    boundary the two choices of cell give the same value (the weight of the other tap is then < 1e-12).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import datasets_referee as ref
from loopy_slam_amd import _ffi, datasets
from util import backends, make_engine

torch.set_num_threads(1)
U = 2.0 ** -24
ONE_STAGE, TWO_STAGES = 9 * U, 17 * U
TUM_DISTORTION = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)          # k1 k2 p1 p2 k3 of TUM freiburg1


def intrinsics(H, W):
    """TUM's 640 x 480 camera scaled to the image."""
    return dict(fx=517.3 * W / 640, fy=516.5 * H / 480, cx=318.6 * W / 640, cy=255.3 * H / 480)


def planted(Hc, Wc, Hd, Wd, seed):
    """colour with all of 0..255 in it, depth with holes (0), 1 and 65535 among random values."""
    g = np.random.RandomState(seed)
    color = g.randint(0, 256, size=(Hc, Wc, 3)).astype(np.uint8)
    color.reshape(-1)[g.permutation(color.size)[:256]] = np.arange(256, dtype=np.uint8)
    depth = g.randint(0, 65536, size=(Hd, Wd)).astype(np.uint16)
    spots = g.permutation(depth.size)[:30]
    depth.reshape(-1)[spots[:10]], depth.reshape(-1)[spots[10:20]], depth.reshape(-1)[spots[20:]] = 0, 1, 65535
    assert set(np.unique(color)) == set(range(256)) and {0, 1, 65535} <= set(np.unique(depth))
    return color, depth


def run(eng, color, depth, scale, K=None, distortion=None, crop_size=None, edge=0, bgr=False):
    """-> colour [Ho,Wo,3] and depth [Ho,Wo] float32 arrays, the undistorted uint8 image (or None).  The outputs start as NaN."""
    K = K or dict(fx=0.0, fy=0.0, cx=0.0, cy=0.0)
    Ho, Wo = datasets.output_size(depth.shape[0], depth.shape[1], crop_size, edge)
    out = (eng.empty(Ho, Wo, 3).fill_(float('nan')), eng.empty(Ho, Wo).fill_(float('nan')))
    undist = eng.zeros(*color.shape, dtype=torch.uint8) if distortion is not None else None
    dev_c = torch.from_numpy(color).to(eng.device)
    dev_d = torch.from_numpy(depth.view(np.int16) if depth.dtype == np.uint16 else depth).to(eng.device)
    datasets.prepare_frame(eng, dev_c, dev_d, scale, distortion=distortion, crop_size=crop_size, crop_edge=edge, bgr=bgr, undist=undist, out=out,
                           **K)
    c, d = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert np.isfinite(c).all() and np.isfinite(d).all()
    return c, d, None if undist is None else undist.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and bool((a.view(np.uint32) == b.view(np.uint32)).all())


#        name        colour    depth     crop_size  distorted  float stages
STAGES = {
    'identity': ((37, 53), (37, 53), None, False, 0),
    'resize': ((61, 83), (30, 41), None, False, 1),
    'crop_size': ((37, 53), (37, 53), (24, 33), False, 1),
    'distortion': ((37, 53), (37, 53), None, True, 0),
    'all': ((61, 83), (30, 41), (24, 33), True, 2),
}


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('bgr', [False, True], ids=['rgb', 'bgr'])
@pytest.mark.parametrize('edge', [0, 3])
@pytest.mark.parametrize('stage', list(STAGES))
def test_stages(backend, stage, edge, bgr):
    eng = make_engine(backend)
    (Hc, Wc), (Hd, Wd), crop_size, distorted, n_float = STAGES[stage]
    color, depth = planted(Hc, Wc, Hd, Wd, seed=len(stage) + 7 * edge + bgr)
    scale = 5000.0 if edge == 0 else 6553.5
    K, dist = intrinsics(Hc, Wc), (TUM_DISTORTION if distorted else None)
    got_c, got_d, got_u8 = run(eng, color, depth, scale, K, dist, crop_size, edge, bgr)
    want_c, want_d, want_u8 = ref.prepare(color, depth, scale, distortion=dist, crop_size=crop_size, edge=edge, bgr=bgr, **K)
    if distorted:
        stats = {}
        ref.undistort_u8(color, K['fx'], K['fy'], K['cx'], K['cy'], dist, stats)
        assert 0.5 * stats['taps'] < stats['taps_inside'] < stats['taps']          # some taps outside the image, most inside
        assert (got_u8 == want_u8).all() and (want_u8 != color).any()
    assert same_bits(got_d, want_d)
    err = float(np.abs(got_c.astype(np.float64) - want_c).max())
    print(f'{stage} edge {edge} bgr {bgr}: max |colour - referee| = {err / U:.2f} u')
    if n_float == 0:
        assert same_bits(got_c, want_c.astype(np.float32))
    else:
        assert err <= (ONE_STAGE if n_float == 1 else TWO_STAGES)


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('scale', [5000.0, 6553.5])
def test_identity_both_depth_scales_and_float_depth(backend, scale):
    eng = make_engine(backend)
    color, depth = planted(37, 53, 37, 53, seed=3)
    got_c, got_d, _ = run(eng, color, depth, scale)
    want_c, want_d, _ = ref.prepare(color, depth, scale)
    assert same_bits(got_c, want_c.astype(np.float32)) and same_bits(got_d, want_d)
    # float depth behind its flag: the same division
    _, got_f, _ = run(eng, color, depth.astype(np.float32), scale, edge=3)
    assert same_bits(got_f, np.ascontiguousarray(want_d[3:-3, 3:-3]))


@pytest.mark.parametrize('backend', backends())
def test_full_size_identity(backend):
    """480 x 640: every row aligned for the four-pixel lanes."""
    eng = make_engine(backend)
    color, depth = planted(480, 640, 480, 640, seed=11)
    got_c, got_d, _ = run(eng, color, depth, 6553.5)
    want_c, want_d, _ = ref.prepare(color, depth, 6553.5)
    assert same_bits(got_c, want_c.astype(np.float32)) and same_bits(got_d, want_d)


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('width', [16, 5])
def test_all_256_colour_values(backend, width):
    """float(c) / 255.0f in fp32 equals the float64 division rounded to fp32 for every c - on the wide path (16 columns) and pixel by pixel (5)."""
    eng = make_engine(backend)
    n = 256 * 3
    rows = -(-n // (3 * width))
    color = np.zeros((rows, width, 3), np.uint8)
    color.reshape(-1)[:n] = np.repeat(np.arange(256, dtype=np.uint8), 3)
    got_c, _, _ = run(eng, color, np.ones((rows, width), np.uint16), 5000.0)
    table = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    assert same_bits(got_c.reshape(-1)[:n], np.repeat(table, 3))
    assert same_bits(table, np.arange(256, dtype=np.float32) / np.float32(255.0))


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('shape,crop_size', [((37, 53), (24, 33)), ((36, 48), (24, 32))])
def test_crop_size_against_torch(backend, shape, crop_size):
    """The crop_size stage alone against F.interpolate on the CPU - a reference that is not the referee.  Colour in float64, as the reference's
    reader feeds it.  36 x 48 -> 24 x 32 has a ratio of 1.5: every second output index lands on an integer source boundary."""
    eng = make_engine(backend)
    color, depth = planted(*shape, *shape, seed=5)
    got_c, got_d, _ = run(eng, color, depth, 5000.0, crop_size=crop_size)
    c64 = torch.from_numpy(color.astype(np.float64) / 255.0).permute(2, 0, 1)[None]
    want_c = F.interpolate(c64, crop_size, mode='bilinear', align_corners=True)[0].permute(1, 2, 0).numpy()
    want_d = F.interpolate(torch.from_numpy(depth.astype(np.float32) / 5000.0)[None, None], crop_size, mode='nearest')[0, 0].numpy()
    assert float(np.abs(got_c.astype(np.float64) - want_c).max()) <= ONE_STAGE
    assert same_bits(got_d, np.ascontiguousarray(want_d))
    if shape == (36, 48):
        assert (ref.nearest_index(36, 24)[2], ref.nearest_index(48, 32)[2]) == (3, 3)


@pytest.mark.parametrize('backend', backends())
def test_argument_errors(backend):
    eng = make_engine(backend)
    dll = eng.lib.dll
    color, depth = planted(12, 16, 12, 16, seed=1)
    c, d = torch.from_numpy(color).to(eng.device), torch.from_numpy(depth.view(np.int16)).to(eng.device)
    oc, od, un = eng.zeros(12, 16, 3), eng.zeros(12, 16), eng.zeros(12, 16, 3, dtype=torch.uint8)
    dist = (C.c_double * 5)(*TUM_DISTORTION)

    def call(color=c, depth=d, flags=0, scale=5000.0, fx=13.0, distortion=None, crop=(0, 0), edge=0, undist=un, out_color=oc, out_depth=od,
             Hc=12):
        p = lambda t: 0 if t is None else t.data_ptr()          # noqa: E731
        return dll.lk_frame_prepare(p(color), Hc, 16, p(depth), 12, 16, flags, scale, fx, 13.0, 7.5, 5.5, distortion, crop[0], crop[1], edge,
                                    p(undist), p(out_color), p(out_depth), eng.stream)

    assert call() == 0 and call(distortion=dist) == 0 and call(crop=(6, 8), edge=2) == 0
    bad = [dict(color=None), dict(depth=None), dict(out_color=None), dict(out_depth=None), dict(distortion=dist, undist=None),
           dict(edge=6), dict(edge=8), dict(edge=-1), dict(crop=(6, 8), edge=3), dict(crop=(1, 8)), dict(crop=(6, 1)), dict(crop=(6, 0)),
           dict(crop=(-2, 8)), dict(flags=4), dict(flags=1 << 31), dict(scale=0.0), dict(scale=float('nan')), dict(Hc=0),
           dict(distortion=dist, fx=0.0)]
    for kw in bad:
        dll.lk_last_error.restype = C.c_char_p
        assert call(**kw) == -1, kw
        assert b'lk_frame_prepare' in dll.lk_last_error(), kw
    with pytest.raises(_ffi.LoopyError, match='crop_edge'):
        datasets.prepare_frame(eng, c, d, 5000.0, crop_edge=6)
