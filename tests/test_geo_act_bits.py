"""The geometry trunk's saved activations are relu BITS, not relu rows (csrc/lk_kernels.h: LK_ACT_GEO_BITS).  The decoder backward needs of
a_i = relu(z_i) only the decision a_i > 0: the forward packs it, 160 bits per sample, into 8 words addressed by sample behind the other act
regions, and the backward forms d y_i from the bits.  The pattern is exact, so nothing a render or a loop produces may move by a bit.

  T1  packer and reader against the plain compare (lk_debug_geo_bits), on the chip and on the emulator: the forward's lane-to-sample
      mapping at tile strides 32 and 30 (the tracker's whole-ray tiles at S = 5), the backward's 32-sample tiles, every special value in
      every one of the 160 positions.
  T2  lk_render_fwd(save_act) + lk_render_bwd on the g6_render_*_map_color goldens cut to 7 and 26 rays against the parent's bytes.
  T3  one lk_track_frame call and one lk_map_frame call against the parent's bytes.
  T4  LK_FLAG_GRAD_GEO_DECODER behind a standalone forward: the fp32 rows are still there for k_geo_wgrad.

T2-T4 compare with tests/golden/geo_act_bits_parent.npz, written by record_parent_fixture() below on an MI355X with the library of the
commit BEFORE the change.  Arrays above 4 096 elements are recorded as the SHA-256 of their bytes (the weight-gradient blob of one colour
case alone is 0.5 MB), everything smaller in full."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import hotpath as H
from loopy_slam_amd import _ffi, core, optim, steps, synthetic as syn
from util import GOLDEN, load, tens, weights, CFG, make_engine, backends
from test_forward_parity import rcfg
from test_steps_parity import mini_scene, HH, WW, INTR

torch.set_num_threads(1)
FIXTURE = os.path.join(GOLDEN, 'geo_act_bits_parent.npz')
FULL_BELOW = 4096
UNITS = 160                       # LK_ACT_GEO_A: five layers of 32 relu outputs per sample
WORDS = 8                         # LK_ACT_GEO_BITS
SENTINEL_W, SENTINEL_B = 0x5a5a5a5a, 0x77


def _sync(eng):
    if eng.device.type == 'cuda':
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- T1
def _f32(bits_):
    return np.asarray(bits_, dtype=np.uint32).view(np.float32)


# +0, -0, smallest and largest fp32 denormal, FLT_MIN, 1e-30, 1, +inf, NaN
SPECIALS = np.concatenate([_f32([0x00000000, 0x80000000, 0x00000001, 0x007fffff, 0x00800000]), np.float32([1e-30, 1.0, np.inf]), _f32([0x7fc00000])])
N_SPECIAL_ROWS, N_BANK = len(SPECIALS), 32
T1_CASES = [(P, 32) for P in (1, 31, 32, 33, 35, 64, 65)] + [(P, 30) for P in (30, 31, 60, 61)]


def bank():
    """32 rows of 160 values.  Rows 0..8: position j of row r holds SPECIALS[(r + j) % 9] - every special value in every position.
    Rows 9..31: seeded random patterns, half of the values negative (and a few negative zeros, negative denormals, -inf and negative NaN):
    every bit position sees both decisions."""
    rng = np.random.default_rng(20262)
    x = np.empty((N_BANK, UNITS), dtype=np.float32)
    for r in range(N_SPECIAL_ROWS):
        x[r] = SPECIALS[(r + np.arange(UNITS)) % N_SPECIAL_ROWS]
    rnd = (rng.standard_normal((N_BANK - N_SPECIAL_ROWS, UNITS)) * np.exp2(rng.integers(-40, 20, (N_BANK - N_SPECIAL_ROWS, UNITS)))).astype(np.float32)
    neg = _f32([0x80000000, 0x80000001, 0x807fffff, 0xff800000, 0xffc00000, 0x80800000])
    for k, v in enumerate(neg):
        rnd[k % rnd.shape[0], (37 * k + 5) % UNITS] = v
    x[N_SPECIAL_ROWS:] = rnd
    return x


def test_bank_holds_what_it_is_meant_to_hold():
    x = bank()
    for v in SPECIALS.view(np.uint32):
        assert ((x[:N_SPECIAL_ROWS].view(np.uint32) == v).sum(0) == 1).all()           # every special once in every position
    with np.errstate(invalid='ignore'):
        dec = x > 0
    assert dec.any(0).all() and (~dec).any(0).all()                                      # both decisions in every position
    assert dec[N_SPECIAL_ROWS:].any(0).all() and (~dec[N_SPECIAL_ROWS:]).any(0).all()     # ... among the random rows alone as well
    # the compare, not the sign bit or an integer test on the pattern: the two smallest positives decide 1, -0 and NaN (sign bit clear) 0
    assert dec[0, 0] == False and dec[0, 2] == True and dec[0, 3] == True and dec[0, 8] == False and dec[0, 1] == False


def _geo_bits(eng, x, stride):
    """lk_debug_geo_bits over x [P][160]: (decisions of the reader, plain compare on the device, words), with guards behind all three."""
    P = x.shape[0]
    xd = eng.f32(np.ascontiguousarray(x))
    assert xd.cpu().numpy().tobytes() == x.tobytes()                    # NaN payloads and denormals reach the device as they are
    words = torch.full((P * WORDS + 64,), SENTINEL_W, dtype=torch.int32, device=eng.device)
    dec = torch.full((P * UNITS + 64,), SENTINEL_B, dtype=torch.uint8, device=eng.device)
    ref = torch.full((P * UNITS + 64,), SENTINEL_B, dtype=torch.uint8, device=eng.device)
    eng.lib.check(eng.lib.dll.lk_debug_geo_bits(xd.data_ptr(), C.c_int32(P), C.c_int32(stride), words.data_ptr(), dec.data_ptr(), ref.data_ptr(), eng.stream),
                  'lk_debug_geo_bits')
    _sync(eng)
    words, dec, ref = words.cpu().numpy(), dec.cpu().numpy(), ref.cpu().numpy()
    assert (words[P * WORDS:] == SENTINEL_W).all() and (dec[P * UNITS:] == SENTINEL_B).all() and (ref[P * UNITS:] == SENTINEL_B).all(), 'a dead lane stored'
    return dec[:P * UNITS].reshape(P, UNITS), ref[:P * UNITS].reshape(P, UNITS), words[:P * WORDS].reshape(P, WORDS).view(np.uint32)


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('P,stride', T1_CASES, ids=['P%d-stride%d' % c for c in T1_CASES])
def test_packer_and_reader_equal_the_compare(backend, P, stride):
    """The production packer in the forward's mapping (tiles of `stride` samples, lanes >= stride and samples >= P dead), the production reader
    in the backward's (tiles of 32), against x > 0.0f from a plain kernel on the same device - and against numpy's compare.  The bank's 32 rows
    pass through in windows of P samples, so that every row is seen at every size (P = 1: one row per call)."""
    eng = make_engine(backend)
    b = bank()
    seen = np.zeros(N_BANK, dtype=bool)
    for off in range(0, N_BANK, P):
        rows = (off + np.arange(P)) % N_BANK
        x = b[rows]
        dec, ref, words = _geo_bits(eng, x, stride)
        bad = np.argwhere(dec != ref)
        for p, j in bad[:8]:
            print('sample', p, 'position', j, 'x bits %08x' % x[p, j].view(np.uint32), 'reader', dec[p, j], 'compare', ref[p, j])
        assert bad.shape[0] == 0
        with np.errstate(invalid='ignore'):
            assert np.array_equal(ref.astype(bool), x > 0)              # (no flush of denormals, NaN compares false)
        assert (words[:, 3] == 0).all() and (words[:, 7] == 0).all() and (words[:, 2] >> 16 == 0).all() and (words[:, 6] >> 16 == 0).all()
        seen[rows] = True
    assert seen.all()


# ---------------------------------------------------------------------------------------------- T2 / T4: small renders
S_USED = 5
R_CASES = (7, 26)                 # P = 35: one tile + three samples; P = 130: a second geometry workgroup whose only live wave holds two samples
# (model, stage, tracker): 'geometry' and 'color' with and without the rel-pos MLP in the mapper's form (unit loss gradients: fp16 pieces in
# both decoder backwards), 'rays': tracker mode with GRAD_RAYS - the geometry backward on bf16 pieces
# (the 'geometry' stage launches no rel-pos MLP on either model; 'geometry-plain' is the model without one all the same, with its per-ray radius)
RENDER_CASES = {'geometry': ('replica', 'geometry', False), 'geometry-plain': ('tum', 'geometry', False), 'color-relpos': ('replica', 'color', False),
                'color-plain': ('tum', 'color', False), 'rays': ('replica', 'color', True)}
FWD_KEYS = ('depth', 'var', 'color', 'raw', 'c_geo')


def render_case(eng, label, R, geo_dec=False):
    model, stage, tracker = RENDER_CASES[label]
    g = load('g6_render_%s_map_color' % model)
    cfg = rcfg(model, S_USED)
    W = weights(model)
    dec = core.DecoderBlob(eng).pack(W)
    ro, rd, gd = (eng.f32(t[:R]) for t in tens(g, 'rays_o', 'rays_d', 'gt_depth'))
    pos, geo, col = (eng.f32(t) for t in tens(g, 'pos', 'geo', 'col'))
    knn = core.KnnIndex(eng, capacity=pos.shape[0])
    knn.build(pos)
    r2d = eng.f32((torch.from_numpy(g['r_query'][:R]) ** 2).float()) if CFG[model]['dynamic'] else None
    st = core.RenderState(eng, R, S_USED, need_act=True)
    for k in FWD_KEYS:
        getattr(st, k).zero_()                    # rows the kernels leave alone (samples below min_nn) compare as zeros
    gc, w_color = eng.f32(g['gt_color'][:R]), float(g['w_color'])
    d_depth, d_color, out4 = eng.zeros(R), eng.zeros(R, 3), eng.zeros(4)
    xf = _ffi.FLAG_ZERO_ABSENT | (0 if tracker else _ffi.FLAG_UNIT_LOSS_GRADS)
    core.render_forward(eng, cfg, st, ro, rd, gd, knn, pos, geo, col, dec, stage, tracker=tracker, r2_ray=r2d, save_act=True, extra_flags=xf,
                        noise_geo=eng.f32(g['noise_geo']), noise_col=eng.f32(g['noise_col']),
                        mapper_loss=None if tracker else (gc, w_color, d_depth, d_color, out4))
    if tracker:
        optim.loss_tracker(eng, st, gd, gc, w_color, True, d_depth, d_color, out4, eng.empty(R + 8))
    gs = core.GradState(eng, pos.shape[0], R, dec.n, feats=not tracker, weights=not tracker, rays=tracker)
    gs.geo_decoder = geo_dec
    core.render_backward(eng, st, gs, d_depth, d_color)
    _sync(eng)
    out = {k: getattr(st, k).detach().cpu().numpy().copy() for k in FWD_KEYS}
    out.update(d_depth=d_depth.cpu().numpy(), d_color=d_color.cpu().numpy(), out4=out4.cpu().numpy())
    if tracker:
        out.update(g_rays_o=gs.g_rays_o.cpu().numpy(), g_rays_d=gs.g_rays_d.cpu().numpy())
    else:
        out.update(g_geo=gs.g_geo.cpu().numpy(), g_col=gs.g_col.cpu().numpy(), g_weights=gs.g_weights.cpu().numpy())
    if geo_dec:
        gW = dec.unpack(gs.g_weights)
        names = sorted(n for n in gW if n.startswith('geo_decoder.') and n != 'geo_decoder.embedder._B')
        assert len(names) == 22, names
        for n in names:
            out['gW.' + n] = gW[n].detach().cpu().numpy().copy()
    return out


# ---------------------------------------------------------------------------------------------- T3: the native loops
TRACK_R, TRACK_ITERS, TRACK_WIN = 12, 3, (2, HH - 2, 2, WW - 2)
MAP_R, MAP_ITERS, MAP_GEO_ITERS = 26, 4, 2
MAP_LRS = {'geometry': (0.001, 0.03, 0.0), 'color': (0.005, 0.005, 0.005)}


def track_case(eng):
    """One lk_track_frame call, 3 iterations x 12 rays at S = 5: forward tiles of 30 samples (6 whole rays), backward tiles of 32."""
    c2w, depth_img, color_img, pos, geo, col = mini_scene(1)
    dec = core.DecoderBlob(eng).pack(syn.default_weights(seed=8))
    pos_d, geo_d, col_d = eng.f32(pos), eng.f32(geo), eng.f32(col)
    knn = core.KnnIndex(eng, capacity=pos.shape[0])
    knn.build(pos_d)
    cam0 = H.c2w_to_cam(c2w) + torch.tensor([0.0, 0.002, -0.001, 0.0015, 0.004, -0.003, 0.002])
    w_w = TRACK_WIN[3] - TRACK_WIN[2]
    rnd = torch.randint(0, (TRACK_WIN[1] - TRACK_WIN[0]) * w_w, (TRACK_ITERS, TRACK_R), generator=torch.Generator().manual_seed(31), dtype=torch.int32)
    to = steps.TrackOptimizer(eng, core.RenderCfg(S=S_USED, rel_pos=True), dec, knn, pos_d, geo_d, col_d, TRACK_R, 0.002, separate_lr=True, w_color=0.5)
    assert to.native_loop
    best, log = to.track(eng.f32(cam0), eng.f32(depth_img), eng.f32(color_img), TRACK_ITERS, TRACK_WIN, INTR, rnd.to(eng.device))
    _sync(eng)
    hist = to._keep_native[5]
    assert tuple(hist.shape) == (TRACK_ITERS, 7)
    return dict(best=best.cpu().numpy(), hist=hist.cpu().numpy(), log=log.cpu().numpy(), geo=geo_d.cpu().numpy(), col=col_d.cpu().numpy(), blob=dec.blob.cpu().numpy())


def map_case(eng):
    """One lk_map_frame call, 2 'geometry' + 2 'color' iterations x 26 rays at S = 5, every second point in the row list, a depth image with
    holes: the live prefix of every iteration's batch is shorter than the batch."""
    c2w, depth_img, color_img, pos, geo, col = mini_scene()
    rnd = torch.randint(0, HH * WW, (MAP_ITERS, MAP_R), generator=torch.Generator().manual_seed(41), dtype=torch.int32)
    rnd[:, :4] = torch.tensor([0, 5, 17, 34], dtype=torch.int32)
    for it in range(MAP_ITERS):
        gd = depth_img.reshape(-1)[rnd[it].long()]
        n_live = int(((gd > 0) & (gd < 10)).sum())
        assert 0 < n_live < MAP_R, (it, n_live)
    dec = core.DecoderBlob(eng).pack(syn.default_weights(seed=7))
    pos_d, geo_d, col_d = eng.f32(pos), eng.f32(geo).clone(), eng.f32(col).clone()
    knn = core.KnnIndex(eng, capacity=pos.shape[0])
    knn.build(pos_d)
    rows = torch.arange(0, pos.shape[0], 2, dtype=torch.int32)
    mo = steps.MapOptimizer(eng, core.RenderCfg(S=S_USED, rel_pos=True), dec, knn, pos_d, geo_d, col_d, rows.to(eng.device), MAP_R, MAP_LRS, w_color=0.1)
    assert mo.fix_geo_decoder and mo._takes_native_loop()
    mo.begin_frame()
    frames = (eng.f32(depth_img).reshape(1, HH, WW), eng.f32(color_img).reshape(1, HH, WW, 3), eng.f32(c2w).reshape(1, 4, 4), None)
    log = eng.zeros(MAP_ITERS, 4)
    mo.run(MAP_ITERS, MAP_GEO_ITERS, frames, rnd.to(eng.device), torch.zeros(MAP_R, dtype=torch.int32, device=eng.device), (0, HH, 0, WW), INTR, HH, WW, log)
    _sync(eng)
    return dict(log=log.cpu().numpy(), geo=geo_d.cpu().numpy(), col=col_d.cpu().numpy(), blob=dec.blob.cpu().numpy())


# ---------------------------------------------------------------------------------------------- the fixture
def _entry(a):
    a = np.ascontiguousarray(a)
    if a.size <= FULL_BELOW:
        return a
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()


def all_cases(eng, which=None):
    out = {}
    for label in RENDER_CASES:
        for R in R_CASES:
            if which in (None, ('render', label, R)):
                for k, v in render_case(eng, label, R).items():
                    out['render.%s.R%d.%s' % (label, R, k)] = v
    if which in (None, 'geodec'):
        for k, v in render_case(eng, 'color-relpos', 7, geo_dec=True).items():
            out['geodec.' + k] = v
    if which in (None, 'track'):
        for k, v in track_case(eng).items():
            out['track.' + k] = v
    if which in (None, 'map'):
        for k, v in map_case(eng).items():
            out['map.' + k] = v
    return out


def record_parent_fixture(path=FIXTURE):
    """Run with the library of the commit BEFORE the change loaded: python -c "import test_geo_act_bits as t; t.record_parent_fixture()"."""
    out = all_cases(make_engine('hip'))
    np.savez_compressed(path, **{k: _entry(v) for k, v in out.items()}, **{'dtype.' + k: np.array(str(v.dtype) + str(v.shape)) for k, v in out.items()})
    return out


_WANT = {}


def _check(prefix, got):
    if not _WANT:
        with np.load(FIXTURE, allow_pickle=False) as z:
            _WANT.update({k: z[k] for k in z.files})
    keys = [k for k in _WANT if k.startswith(prefix + '.')]
    assert sorted(keys) == sorted(prefix + '.' + k for k in got), (sorted(keys), sorted(got))
    bad = []
    for k, v in got.items():
        name = prefix + '.' + k
        assert str(_WANT['dtype.' + name]) == str(v.dtype) + str(v.shape), name
        e, w = _entry(v), _WANT[name]
        if e.dtype != w.dtype or e.shape != w.shape or e.tobytes() != w.tobytes():
            bad.append((k, 'digest' if v.size > FULL_BELOW else int((np.ascontiguousarray(v).view(np.uint8) != w.view(np.uint8)).sum())))
    assert not bad, (prefix, bad)


@pytest.mark.gpu
@pytest.mark.parametrize('R', R_CASES)
@pytest.mark.parametrize('label', list(RENDER_CASES))
def test_small_render_and_backward_equal_parent_bytes_gpu(label, R):
    got = render_case(make_engine('hip'), label, R)
    assert float(np.abs(got['depth']).sum()) > 0 and float(np.abs(got['raw'][:, 3]).sum()) > 0
    if label == 'rays':
        assert float(np.abs(got['g_rays_d']).sum()) > 0
    else:
        assert float(np.abs(got['g_geo']).sum()) > 0 and float(np.abs(got['g_weights']).sum()) > 0
    _check('render.%s.R%d' % (label, R), got)


@pytest.mark.gpu
def test_track_frame_equals_parent_bytes_gpu():
    got = track_case(make_engine('hip'))
    assert np.isfinite(got['log']).all() and float(np.abs(got['hist'][-1] - got['hist'][0]).sum()) > 0
    _check('track', got)


@pytest.mark.gpu
def test_map_frame_equals_parent_bytes_gpu():
    got = map_case(make_engine('hip'))
    assert np.isfinite(got['log']).all() and (got['log'][:, 3] > 0).all() and (got['log'][:, 3] < MAP_R).all()
    _check('map', got)


@pytest.mark.gpu
def test_geo_decoder_gradients_still_get_their_rows_gpu():
    """LK_FLAG_GRAD_GEO_DECODER is decided AFTER the standalone forward has run: it wrote the fp32 relu rows beside the bits, and k_geo_wgrad
    reads them - the 22 matrices and biases of the geometry decoder receive the parent's gradients."""
    got = render_case(make_engine('hip'), 'color-relpos', 7, geo_dec=True)
    n = [k for k in got if k.startswith('gW.')]
    assert len(n) == 22 and all(float(np.abs(got[k]).sum()) > 0 for k in n)
    _check('geodec', got)


@pytest.mark.parametrize('backend', backends())
def test_misaligned_act_is_refused(backend):
    """The bits region is read and written 16 bytes at a time: an activation buffer that is not 16-byte aligned is an error of the call."""
    eng = make_engine(backend)
    g = load('g6_render_replica_map_color')
    dec = core.DecoderBlob(eng).pack(weights('replica'))
    ro, rd, gd = (eng.f32(t[:7]) for t in tens(g, 'rays_o', 'rays_d', 'gt_depth'))
    pos, geo, col = (eng.f32(t) for t in tens(g, 'pos', 'geo', 'col'))
    knn = core.KnnIndex(eng, capacity=pos.shape[0])
    knn.build(pos)
    st = core.RenderState(eng, 7, S_USED, need_act=True)
    whole = eng.zeros(st.act.numel() + 4)
    st.act = whole[1:1 + st.act.numel()]
    assert st.act.data_ptr() % 16 == 4
    with pytest.raises(Exception, match='16-byte aligned'):
        core.render_forward(eng, rcfg('replica', S_USED), st, ro, rd, gd, knn, pos, geo, col, dec, 'geometry', save_act=True)
    _sync(eng)
