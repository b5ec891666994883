"""The fp16 two-piece cut of the forward products (csrc/lk_common.h: lk_cut2h): hi = rtz_f16(x), lo = rtz_f16(x - hi).  The remainder is
taken as fma((float)hi, -1, x) - ONE instruction that reads the half operand directly - instead of convert + subtract.  The product is exact, so
the fma rounds x - hi once, exactly as the subtraction does: the pieces must not move by a bit, for any input.

  * CPU: the identity itself in numpy float32 over the sweep below (the fma as the float64 product-sum, rounded once, against the float32
    subtraction), through the second pack-convert.
  * GPU: lk_debug_split_forms runs the production cut and a test-only kernel with the convert-and-subtract form over the same 65 536
    values; both pieces agree bit for bit, and (float)hi + (float)lo gives x back.
  * GPU: one lk_render_fwd of R = 7 rays, S = 5 (P = 35 = 32 + 3 in the decoders' 32-sample tiles, 8 x 4 + 3 in the rel-pos MLP's 4-sample
    waves: a tail and dead lanes in every tile form) with and without the rel-pos MLP equals the bytes recorded from the build BEFORE the change
    (tests/golden/split_forms_render_parent.npz, written by record_render_fixture below on an MI355X with the parent commit's library).

How well two pieces reproduce x (asserted, from the format alone): hi keeps 11 significand bits by truncation, so r = x - hi is exact in fp32 and
|r| < 2^(e-10) for 2^e <= |x| < 2^(e+1); lo truncates r to 11 bits again, |r - lo| < 2^(e-21) <= 2^-21 |x| - as long as lo is a NORMAL half or
its subnormal step 2^-24 is no coarser than that, i.e. e >= -3, and x is below fp16's ceiling: 2^-3 <= |x| <= 65 504 is "the normal range" of
the 2^-21 bound.  Below it the bound is the subnormal step, |x - hi - lo| < 2^-24 absolute."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from loopy_slam_amd import core
from util import GOLDEN, load, tens, weights, make_engine
from test_forward_parity import rcfg

torch.set_num_threads(1)
N_SWEEP = 65536
FIXTURE = os.path.join(GOLDEN, 'split_forms_render_parent.npz')
R_USED = 7


def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def sweep():
    """65 536 float32 values: every class of input the cut can meet, then random normals at the scales 2^-30 .. 2^17."""
    rng = np.random.default_rng(20261)
    parts = []
    parts.append(_bits([0x00000000, 0x80000000]))                                                   # +-0
    den = np.concatenate([[1, 2, 0x007fffff, 0x00400000, 0x00000100], rng.integers(1, 0x00800000, 1019)]).astype(np.uint32)
    parts.append(_bits(den)); parts.append(_bits(den | 0x80000000))                                 # f32 denormals
    tiny = (rng.uniform(1.0, 2.0, 2048) * np.exp2(rng.integers(-60, -25, 2048))).astype(np.float32)  # below half's smallest subnormal, 2^-24
    tiny[:4] = np.float32(2.0 ** -24) * np.float32([1.0 - 2.0 ** -24, 0.5, 0.75, 1.0 - 2.0 ** -12])
    parts.append(tiny * np.where(rng.integers(0, 2, 2048) == 1, np.float32(-1), np.float32(1)))
    hb = rng.integers(0, 0x7c00, 8192).astype(np.uint16)                                            # exact halves (subnormal ones included): lo = 0
    hb[:6] = [0x0001, 0x03ff, 0x0400, 0x7bff, 0x3c00, 0x0000]
    hb |= (rng.integers(0, 2, 8192) << 15).astype(np.uint16)
    parts.append(hb.view(np.float16).astype(np.float32))
    top = np.float32([65504.0, 65503.996, 65504.004, 65519.996, 65520.0, 65535.0, 65536.0, 65472.0, 65488.0, 1e5, 1e10, 3e38, 3.4028235e38])
    parts.append(np.concatenate([top, -top, np.float32([np.inf, -np.inf])]))                        # around and above fp16's ceiling, +-inf
    parts.append(_bits([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fc00001, 0x7fffffff, 0x7fa00000, 0x7f801000]))   # NaN
    n_fixed = sum(len(p) for p in parts)
    n_rand = N_SWEEP - n_fixed
    e = rng.integers(-30, 18, n_rand)
    rnd = (rng.standard_normal(n_rand) * np.exp2(e)).astype(np.float32)
    parts.append(rnd)
    x = np.concatenate([np.asarray(p, dtype=np.float32) for p in parts])
    assert x.shape == (N_SWEEP,) and x.dtype == np.float32
    return x


def rtz_f16(x):
    """round toward zero to a half, saturating at 65 504 (v_cvt_pkrtz_f16_f32), as the float32 value of that half; inf and NaN pass"""
    x = np.asarray(x, dtype=np.float32)
    a = np.abs(x)
    u = a.view(np.uint32)
    normal = (u & np.uint32(0xffffe000)).view(np.float32)                      # 10 fraction bits kept
    with np.errstate(invalid='ignore', over='ignore'):
        sub = (np.floor(a.astype(np.float64) * 2.0 ** 24) * 2.0 ** -24).astype(np.float32)   # multiples of 2^-24 below 2^-14
    h = np.where(a < np.float32(2.0 ** -14), sub, normal)
    h = np.where(np.isfinite(a) & (a > np.float32(65504.0)), np.float32(65504.0), h)
    h = np.where(np.isfinite(a), h, a)
    return np.copysign(h, x).astype(np.float32)


def same_or_both_nan(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def test_fma_remainder_is_the_subtraction_cpu():
    """fma((float)hi, -1, x), one rounding of the exact product-sum, against the float32 subtraction x - (float)hi - and through the second cut.
    float64 holds hi * -1 + x exactly whenever |x| < 2^57 (both operands have 24-bit significands, the smaller one's lowest bit is >= 2^-24 of
    fp16's ceiling ... 2^5 at the saturated hi); above that hi is less than 2^-17 of an fp32 ulp of x and nowhere near a rounding tie, so the
    two roundings (to float64, then to float32) land where one would."""
    x = sweep()
    hi = rtz_f16(x)
    with np.errstate(invalid='ignore', over='ignore'):
        r_sub = (x - hi).astype(np.float32)
        r_fma = (hi.astype(np.float64) * -1.0 + x.astype(np.float64)).astype(np.float32)
    assert same_or_both_nan(r_sub, r_fma).all()
    assert same_or_both_nan(rtz_f16(r_sub), rtz_f16(r_fma)).all()
    # the sweep holds what it is meant to hold
    fin = np.isfinite(x)
    assert (x == 0).sum() >= 2 and np.isnan(x).sum() >= 8 and np.isinf(x).sum() == 2
    assert ((np.abs(x) < np.float32(2.0 ** -126)) & (x != 0)).sum() >= 2000            # f32 denormals
    assert ((np.abs(x) < np.float32(2.0 ** -24)) & (np.abs(x) >= np.float32(2.0 ** -126))).sum() >= 2000
    assert (fin & (r_sub == 0) & (x != 0)).sum() >= 8000                                   # exact halves
    assert (fin & (np.abs(x) > 65504)).sum() >= 16
    ex = np.floor(np.log2(np.abs(x[fin & (x != 0)]).astype(np.float64)))
    for e in range(-30, 18):
        assert (ex == e).sum() >= 200, e


def _split_on_gpu(eng, x):
    n = x.shape[0]
    xd = eng.f32(x)
    assert xd.cpu().numpy().tobytes() == x.tobytes()                                        # NaN payloads and denormals reach the device as they are
    out = [eng.zeros(n // 2, dtype=torch.int32) for _ in range(4)]
    eng.lib.check(eng.lib.dll.lk_debug_split_forms(xd.data_ptr(), C.c_int32(n), *[o.data_ptr() for o in out], eng.stream), 'lk_debug_split_forms')
    torch.cuda.synchronize()
    return [o.cpu().numpy().view(np.uint32) for o in out]


@pytest.mark.gpu
def test_production_cut_equals_convert_and_subtract_gpu():
    eng = make_engine('hip')
    x = sweep()
    hi, lo, hi_ref, lo_ref = _split_on_gpu(eng, x)
    bad_hi, bad_lo = np.flatnonzero(hi != hi_ref), np.flatnonzero(lo != lo_ref)
    print('pairs', hi.shape[0], 'high pieces that differ', bad_hi.size, 'low pieces that differ', bad_lo.size)
    for i in bad_lo[:8]:
        print('  x', x[2 * i:2 * i + 2].view(np.uint32), 'hi %08x lo %08x lo_ref %08x' % (hi[i], lo[i], lo_ref[i]))
    assert bad_hi.size == 0 and bad_lo.size == 0
    # the two pieces give x back (module docstring): 2^-21 relative in 2^-3 <= |x| <= 65 504, the subnormal step 2^-24 absolute below
    h = hi.view(np.float16).astype(np.float64)                # little endian: element 0 of a pair is the low half of the register
    l = lo.view(np.float16).astype(np.float64)
    assert h.shape == (N_SWEEP,)
    with np.errstate(invalid='ignore'):
        x64 = x.astype(np.float64)
        a = np.abs(x64)
        err = np.abs(h + l - x64)
    normal = (a >= 2.0 ** -3) & (a <= 65504.0)
    small = a < 2.0 ** -3
    rel = float((err[normal] / a[normal]).max())
    print('values in the normal range', int(normal.sum()), 'max relative error %.3g (2^-21 = %.3g)' % (rel, 2.0 ** -21),
          '; below 2^-3:', int(small.sum()), 'max absolute error %.3g (2^-24 = %.3g)' % (float(err[small].max()), 2.0 ** -24))
    assert normal.sum() > 20000 and small.sum() > 20000
    assert (err[normal] <= 2.0 ** -21 * a[normal]).all()
    assert (err[small] < 2.0 ** -24).all()
    exact = np.isfinite(x) & (x == rtz_f16(x))
    assert (l[exact] == 0).all() and (h[exact] == x64[exact]).all()


# ---------------------------------------------------------------------------------------------- one small render against the parent's bytes
RENDERS = {'relpos': 'replica', 'plain': 'tum'}               # with / without the rel-pos MLP (util.CFG)
KEYS = ('depth', 'var', 'color', 'raw', 'c_geo', 'c_col')


def render_outputs(eng, label):
    name = RENDERS[label]
    g = load('g6_render_%s_map_color' % name)
    cfg = rcfg(name)
    assert cfg.S == 5 and cfg.rel_pos == (label == 'relpos')
    dec = core.DecoderBlob(eng).pack(weights(name))
    ro, rd, gd, pos, geo, col = tens(g, 'rays_o', 'rays_d', 'gt_depth', 'pos', 'geo', 'col')
    pos_d = eng.f32(pos)
    knn = core.KnnIndex(eng, capacity=pos.shape[0])
    knn.build(pos_d)
    st = core.RenderState(eng, R_USED, cfg.S, need_act=True)
    for k in KEYS:
        getattr(st, k).zero_()                    # rows the kernels leave alone (samples below min_nn) compare as zeros
    core.render_forward(eng, cfg, st, eng.f32(ro[:R_USED]), eng.f32(rd[:R_USED]), eng.f32(gd[:R_USED]), knn, pos_d, eng.f32(geo), eng.f32(col), dec,
                        'color', noise_geo=eng.f32(g['noise_geo']), noise_col=eng.f32(g['noise_col']), save_act=True)
    torch.cuda.synchronize()
    return {k: getattr(st, k).detach().cpu().numpy().copy() for k in KEYS}


def record_render_fixture(path=FIXTURE):
    """Run with the library of the commit BEFORE the change loaded: python -c "import test_split_forms as t; t.record_render_fixture()"."""
    eng = make_engine('hip')
    out = {}
    for label in RENDERS:
        for k, v in render_outputs(eng, label).items():
            out[label + '.' + k] = v
    np.savez_compressed(path, **out)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('label', list(RENDERS))
def test_small_render_equals_parent_bytes_gpu(label):
    with np.load(FIXTURE, allow_pickle=False) as z:
        want = {k: z[k] for k in z.files}
    got = render_outputs(make_engine('hip'), label)
    assert float(np.abs(got['color']).sum()) > 0 and float(np.abs(got['depth']).sum()) > 0
    for k in KEYS:
        w = want[label + '.' + k]
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
        assert got[k].tobytes() == w.tobytes(), (k, int((got[k].view(np.uint32) != w.view(np.uint32)).sum()))
