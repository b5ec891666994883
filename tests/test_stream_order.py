"""Order between the library's own streams ("Forks and joins"): every fork is a promise "nothing the other stream writes before
the join is read here, nothing it still reads is rewritten here".  The host emulator runs every stream in enqueue order and the chip keeps
a missing wait hidden whenever the timing is kind, so the promises are tested by making the timing unkind on purpose:
lk_debug_stream_delay(site, us) parks one spinning wave

  LK_DELAY_WGRAD   on the weight-gradient stream in front of the forked k_wgrad            (that stream LATE: a missing join)
  LK_DELAY_SORT    on the same stream in front of the forked counting sort of a standalone backward
  LK_DELAY_AHEAD   on the look-ahead stream in front of every chunk's search and between its search and its sorts
  LK_DELAY_LAUNCH  on the LAUNCH stream behind every fork (the other streams run AHEAD of it: a buffer reused too early)

and a whole call with ONE site at 500 us (or more, _delay_for) has to leave the bits of the same call without a delay: the loss log, the decoder blob, both
feature tables (rows inside and outside the list), the tracker's poses, the gradient tensors of a standalone backward.  The loops sum in
a fixed order, so there is no tolerance to hide in: a misordering that moves one float fails.

What keeps the comparison honest is asserted, not assumed:
  * the premise: the undelayed call twice gives equal bits (one form does not: NOISE);
  * the delay can reorder: the undelayed call, timed with events, spends at most half the delay per iteration (_delay_for);
  * a miss gives wrong NUMBERS, not a wild address: uninitialised buffers are NaN in the tests and the work buffers keep index lists in
    float storage, so before every compared call the SAME optimiser / render state has run the same form with OTHER draws - every region
    a misordered kernel could read early holds valid lists of another batch (OTHER_SEED), different from the right ones;
  * the one-stream call (lk_set_serial) of every form runs too.  It takes other launches (no fork, no split step: the whole Adam step
    in one reduction launch) and was measured to leave the bits of the overlapped call in every form that repeats bit for bit
    (profiles/stream_order.md), so it is held to equal bits there; the NOISE form to the bounds of tests/test_split_step_order.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import atsize as A
from oracle import hotpath as H
from loopy_slam_amd import _ffi, core, optim, steps, synthetic as syn
from util import make_engine

WGRAD, SORT, AHEAD, LAUNCH = 0, 1, 2, 3
SITE_NAME = {WGRAD: 'wgrad', SORT: 'sort', AHEAD: 'ahead', LAUNCH: 'launch'}
ERR_ARG = -1                          # LK_ERR_ARG
DELAY_US = 500                        # what a site spins for ...
# ... and never less than twice the undelayed iteration as this run measured it: most forms here are bound by their launches, not by R
# (the geometry decoder's weight-gradient form takes 260-270 us per iteration at 512 rays and at 128; the standalone backward 195 us alone
# and 276 us late in a long pytest process), so where an iteration takes more than 250 us the sites spin for twice that, rounded up to
# 100 us, instead of the test lowering R to no effect.  The assertion stays "an iteration takes at most half the delay".
MAX_DELAY_US = 2000                   # LK_DELAY_MAX_US


def _delay_for(iter_us):
    return max(DELAY_US, int(-(-2.0 * iter_us // 100) * 100))


MAP_LRS = {'geometry': (0.001, 0.03, 0.0), 'color': (0.005, 0.005, 0.005)}
N_POINTS, WINDOW = 20_000, 4
N_GEO, N_COL = 2, 12                  # look-ahead chunks {0}, {1..6}, {7..12}, {13}; step rider + split step in 11 iterations
SEED, OTHER_SEED = 91, 1777
HH, WW = A.I['H'], A.I['W']
# The one form whose undelayed call does not repeat bit for bit: the exposure variant of the loss sums d affine with one LDS float add per
# wave, in the order the waves arrive.  Its delayed calls are held to 4 x the largest pairwise difference, per array,
# of five undelayed calls of this form on the commit before the delay sites existed (profiles/stream_order.md; five samples
# under-estimate the tail of a maximum, and a misordered feature or weight read moves sign-like Adam steps by a whole lr = 5e-3 .. 3e-2).
NOISE = {'exposure': dict(log=1.220703125e-4, blob=1.697540283203125e-4, geo=1.2259706854820251e-3, col=4.172325134277344e-07,
                          x_mlp=5.960464477539063e-08, x_feats=3.725290298461914e-09)}
NOISE_FACTOR = 4.0


# ---------------------------------------------------------------------------------------------- the hook itself
def _delay(dll, site, us):
    return int(dll.lk_debug_stream_delay(C.c_int32(site), C.c_int32(us)))


def _all_off(dll):
    for s in SITE_NAME:
        assert _delay(dll, s, 0) == 0
    dll.lk_set_serial(0)


def test_hook_accepts_and_refuses_and_serial_ignores_it():
    """Sites 0..3 at 0..2000 us are accepted, everything else is LK_ERR_ARG; lk_debug_side_delay is site 0; a one-stream call with every
    site on equals the call with every site off (no site launches anything there - on the emulator, whose streams run in order anyway,
    this checks that the hooked call still runs and computes the same)."""
    eng = make_engine('emu')
    dll = eng.lib.dll
    try:
        for s in SITE_NAME:
            for us in (0, 1, 500, 2000, 0):
                assert _delay(dll, s, us) == 0, (s, us)
            for us in (-1, 2001, 10 ** 6, -2 ** 31):
                assert _delay(dll, s, us) == ERR_ARG, (s, us)
        for s in (-1, 4, 5, 1000):
            assert _delay(dll, s, 0) == ERR_ARG and _delay(dll, s, 100) == ERR_ARG, s
        assert b'lk_debug_stream_delay' in dll.lk_last_error()
        assert int(dll.lk_debug_side_delay(400)) == 0 and int(dll.lk_debug_side_delay(-3)) == 0 and int(dll.lk_debug_side_delay(0)) == 0
        assert int(dll.lk_debug_side_delay(2001)) != 0
        form = BwdForm(eng, 'bwd-relpos', R=6, n_points=None)
        ref = form.run(SEED)
        dll.lk_set_serial(1)
        for s in SITE_NAME:
            assert _delay(dll, s, 2000) == 0
        _same_bits(form.run(SEED), ref, 'serial call with every site on')
        dll.lk_set_serial(0)
        _same_bits(form.run(SEED), ref, 'emulated call with every site on')
    finally:
        _all_off(dll)


# ---------------------------------------------------------------------------------------------- comparison
def _np(t):
    return t.detach().cpu().numpy().copy()


def _same_bits(got, want, what):
    assert sorted(got) == sorted(want), what
    bad = []
    for k in sorted(want):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        if a.tobytes() != b.tobytes():
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            bad.append((k, int((a.view(np.uint8) != b.view(np.uint8)).reshape(a.shape + (-1,)).any(-1).sum()), a.size, float(np.nanmax(d))))
    assert not bad, '%s: (array, differing entries, of, largest difference) %s' % (what, bad)


def _same(got, want, what, name):
    """Equal bits - or, for a form in NOISE, every array within NOISE_FACTOR times its run-to-run difference."""
    if name not in NOISE:
        return _same_bits(got, want, what)
    assert sorted(got) == sorted(want) == sorted(NOISE[name]), what
    d = _largest(got, want)
    print('%s: largest differences %s' % (what, d))
    bad = {k: (v, NOISE_FACTOR * NOISE[name][k]) for k, v in d.items() if not v <= NOISE_FACTOR * NOISE[name][k]}
    assert not bad, '%s: (largest difference, bound) %s' % (what, bad)


def _serial_bounds(form, got, want, what):
    """A form whose one-stream call does not leave the overlapped call's bits: the bounds tests/test_split_step_order.py holds that pair to
    (losses 5e-5 relative in the first 'color' iterations and 2e-3 throughout, at most 2 % of the fc_c entries half a learning rate apart,
    rows within 2 lr per 'color' iteration); the exposure MLP and features, which that file does not have, as the rows."""
    lr = MAP_LRS['color'][0]
    lw, lg = want['log'][:, 0].astype(np.float64), got['log'][:, 0].astype(np.float64)
    rel = np.abs(lg - lw) / np.abs(lw)
    assert rel[:N_GEO + 3].max() <= 5e-5 and rel.max() <= 2e-3, (what, rel.tolist())
    Wg, Ww = (form.dec.unpack(torch.from_numpy(o['blob'])) for o in (got, want))
    fc = [n for n in Ww if n.startswith('color_decoder.fc_c.') and n.endswith('.weight')]
    assert len(fc) == 5
    for n in fc:
        frac = float(((Wg[n] - Ww[n]).abs() > 0.5 * lr).float().mean())
        assert frac <= 0.02, (what, n, frac)
    for k in sorted(set(want) - {'log', 'blob'}):
        assert float(np.abs(got[k].astype(np.float64) - want[k]).max()) <= 2.0 * lr * N_COL, (what, k)


def _largest(got, want):
    return {k: float(np.nanmax(np.abs(got[k].astype(np.float64) - want[k].astype(np.float64)))) if want[k].size else 0.0 for k in want}


# ---------------------------------------------------------------------------------------------- scene shared by the forms
_SHARED = {}


def _frames():
    if 'frames' not in _SHARED:
        fr = [syn.render_frame(3 * k, device='cpu', holes=0.02) for k in range(WINDOW)]
        _SHARED['frames'] = tuple(torch.stack([f[q] for f in fr]).contiguous() for q in range(3))
    return _SHARED['frames']


def _draws(seed, iters, R):
    return torch.randint(0, HH * WW, (iters, R), generator=torch.Generator().manual_seed(seed + R), dtype=torch.int32)


class MapForm:
    """One MapOptimizer (one `work` buffer, one bwd_scratch, one index handle) that runs the same lk_map_frame call again and again from
    the same start, with the draws of `seed`."""

    def __init__(self, eng, name, rel_pos, R, per_ray_radii=False, whole_map=False, train_geo=False, exposure=False, surfaces=(0.98, 1.02)):
        self.eng, self.name, self.R = eng, name, R
        pos, geo, col = A.scene(N_POINTS)
        depth_s, color_s, pose_s = _frames()
        self.W0 = syn.default_weights(rel_pos=rel_pos, exposure=exposure)
        self.dec = core.DecoderBlob(eng).pack(self.W0)
        self.blob0 = self.dec.blob.clone()
        self.geo0, self.col0 = eng.f32(geo), eng.f32(col)
        self.dpos, self.dgeo, self.dcol = eng.f32(pos), self.geo0.clone(), self.col0.clone()
        self.knn = core.KnnIndex(eng, capacity=pos.shape[0])
        self.knn.build(self.dpos)
        r2 = None
        if per_ray_radii:
            r2 = torch.stack([optim.radius_maps(eng, eng.f32(color_s[k]), 0.15, 0.08, 0.02, 2.0)[2] for k in range(WINDOW)]).contiguous()
        self.frames = (eng.f32(depth_s), eng.f32(color_s), eng.f32(pose_s), r2)
        # (exposure encoding: the rays grouped by keyframe, as the loss kernel sums d affine over the lanes of a keyframe)
        self.fid = ((torch.arange(R) * WINDOW // R) if exposure else (torch.arange(R) % WINDOW)).to(torch.int32).to(eng.device)
        self.rows = self.mask = None
        self.x = None
        if exposure:          # mlp_exposure as the torch module that owns its parameters (the kernels step them in place) + one feature per keyframe
            m = torch.nn.Sequential(torch.nn.Linear(8, 128), torch.nn.Softplus(beta=100), torch.nn.Linear(128, 12)).to(eng.device)
            with torch.no_grad():
                for lin, n in ((m[0], 'linear1'), (m[2], 'linear2')):
                    lin.weight.copy_(self.W0['color_decoder.mlp_exposure.%s.weight' % n]); lin.bias.copy_(self.W0['color_decoder.mlp_exposure.%s.bias' % n])
            g = torch.Generator().manual_seed(5)
            feats = [eng.f32(0.1 * torch.randn(8, generator=g)).requires_grad_(True) for _ in range(WINDOW)]
            self.x = (m, feats, [q.detach().clone() for q in m.parameters()], [f.detach().clone() for f in feats])
        if not whole_map:
            rows = torch.from_numpy(H.frustum_rows(pos.numpy(), pose_s[0].numpy(), depth_s[0].numpy(), *A.INTR, HH, WW, -4)).long()
            assert 0 < rows.numel() < pos.shape[0]
            mask = torch.zeros(pos.shape[0], dtype=torch.uint8)
            mask[rows] = 1
            self.rows, self.mask = rows.to(torch.int32).to(eng.device), mask.to(eng.device)
        self.whole_map = whole_map
        cfg = core.RenderCfg(rel_pos=rel_pos, exposure=exposure, near_surface=surfaces[0], far_surface=surfaces[1])
        self.mo = steps.MapOptimizer(eng, cfg, self.dec, self.knn, self.dpos, self.dgeo, self.dcol, self.rows, R, MAP_LRS,
                                     w_color=0.1, dynamic_radius=per_ray_radii, fix_color_decoder=whole_map, fix_geo_decoder=not train_geo,
                                     exposure=self.x[:2] if exposure else None)
        assert self.mo._takes_native_loop()
        self.last_us = None

    def reset(self):
        self.dec.blob.copy_(self.blob0)
        self.dec.repack()
        self.dgeo.copy_(self.geo0)
        self.dcol.copy_(self.col0)
        if self.x is not None:
            with torch.no_grad():
                for q, q0 in zip(list(self.x[0].parameters()) + self.x[1], self.x[2] + self.x[3]):
                    q.copy_(q0)
            self.mo.exposure = steps.ExposureState(self.eng, self.x[0], self.x[1])
        self.mo.new_frame(self.rows, self.mask)

    def run(self, seed, n_geo=N_GEO, n_col=N_COL, reset=True, timed=False):
        eng, iters = self.eng, n_geo + n_col
        if reset:
            self.reset()
        else:
            self.mo.new_frame(self.rows, self.mask)
        rnd = _draws(seed, iters, self.R).to(eng.device)
        log = eng.zeros(iters, 4)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if timed:
            torch.cuda.synchronize()
            e0.record()
        self.mo.run(iters, n_geo, self.frames, rnd, self.fid, (0, HH, 0, WW), A.INTR, HH, WW, log)
        if timed:
            e1.record()
        self.mo.finish()
        torch.cuda.synchronize()
        if timed:
            self.last_us = 1e3 * e0.elapsed_time(e1) / iters
        assert eng.status(sync=True) == 0
        out = dict(log=_np(log), blob=_np(self.dec.blob), geo=_np(self.dgeo), col=_np(self.dcol))
        if self.x is not None:
            out.update(x_mlp=np.concatenate([_np(q).reshape(-1) for q in self.x[0].parameters()]), x_feats=np.stack([_np(f) for f in self.x[1]]))
        return out

    def check_path(self, out):
        """The call did what the form is about: finite losses over live rays, rows outside the list untouched, and the colour trunk stepped
        (rider + split step) - or, whole map, stayed frozen while rows moved."""
        assert np.isfinite(out['log']).all() and (out['log'][:, 3] > 0).all()
        blob0, lr = _np(self.blob0), MAP_LRS['color'][0]
        Wk = {n: v.clone().cpu() for n, v in self.dec.unpack(torch.from_numpy(out['blob']).to(self.eng.device)).items()}
        fc = [n for n in Wk if n.startswith('color_decoder.fc_c.') and n.endswith('.weight')]
        assert len(fc) == 5
        moved = max(float((Wk[n].reshape(-1) - self.W0[n].reshape(-1)).abs().max()) for n in fc)
        g0 = _np(self.geo0)
        if self.whole_map:
            assert moved == 0.0 and float(np.abs(out['geo'] - g0).max()) > 0
        else:
            assert moved > 0.5 * lr, 'the colour decoder did not step: the call did not take the rider path'
            outside = np.ones(g0.shape[0], dtype=bool)
            outside[_np(self.rows).astype(np.int64)] = False
            assert out['geo'][outside].tobytes() == g0[outside].tobytes() and out['col'][outside].tobytes() == _np(self.col0)[outside].tobytes()
            assert float(np.abs(out['geo'][~outside] - g0[~outside]).max()) > 0
        assert out['blob'].tobytes() != blob0.tobytes()
        if self.x is not None:          # the mapped frame's feature (the last) and mlp_exposure are parameters, the keyframes' features constants
            f0 = np.stack([_np(f) for f in self.x[3]])
            assert float(np.abs(out['x_feats'][-1] - f0[-1]).max()) > 1e-4 and out['x_feats'][:-1].tobytes() == f0[:-1].tobytes()
            assert out['x_mlp'].tobytes() != np.concatenate([_np(q).reshape(-1) for q in self.x[2]]).tobytes()


MAP_FORMS = {
    # name: (constructor arguments, sites)
    'replica': (dict(rel_pos=True, R=512), (WGRAD, AHEAD, LAUNCH)),
    'tum': (dict(rel_pos=False, R=1024, per_ray_radii=True), (WGRAD, AHEAD, LAUNCH)),          # no `mid`: the next interpolation rewrites c_col soonest
    'whole-map': (dict(rel_pos=True, R=512, whole_map=True), (AHEAD, LAUNCH)),                  # rows = NULL, act_flag, colour decoder frozen: no weight-gradient fork
    'train-geo': (dict(rel_pos=True, R=512, train_geo=True), (WGRAD, AHEAD, LAUNCH)),           # k_geo_wgrad, no rider
    # ScanNet model: exposure encoding, no rider, the exposure step rides in the gather launch
    'exposure': (dict(rel_pos=False, R=1024, per_ray_radii=True, exposure=True, surfaces=(0.96, 1.04)), (WGRAD, AHEAD, LAUNCH)),
}


def _run_with(dll, form, site, serial, fn, delay_us=DELAY_US):
    """fn() with `site` at delay_us (None: none), behind a call of the same form with OTHER draws (see the module text)."""
    _all_off(dll)
    form.run(OTHER_SEED)
    try:
        dll.lk_set_serial(1 if serial else 0)
        if site is not None:
            assert _delay(dll, site, delay_us) == 0
        return fn()
    finally:
        _all_off(dll)


def _order_test(form, sites, name):
    dll = form.eng.lib.dll
    try:
        ref = _run_with(dll, form, None, False, lambda: form.run(SEED, timed=True))
        form.check_path(ref)
        print('%s: %.1f us per iteration undelayed' % (name, form.last_us))
        delay_us = _delay_for(form.last_us)
        assert delay_us <= MAX_DELAY_US and form.last_us <= 0.5 * delay_us, 'an iteration takes %.0f us: no delay the hook accepts is twice that - lower R' % form.last_us
        _same(_run_with(dll, form, None, False, lambda: form.run(SEED)), ref, name + ': the undelayed call twice (the premise)', name)
        for site in sites:
            got = _run_with(dll, form, site, False, lambda: form.run(SEED), delay_us)
            _same(got, ref, '%s with the %s site at %d us' % (name, SITE_NAME[site], delay_us), name)
        ser = _run_with(dll, form, None, True, lambda: form.run(SEED))
        print('%s: one-stream call against the overlapped one, largest differences %s' % (name, _largest(ser, ref)))
        if name in NOISE:
            _serial_bounds(form, ser, ref, name + ': the one-stream call')
        else:
            _same_bits(ser, ref, name + ': the one-stream call')
    finally:
        _all_off(dll)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(MAP_FORMS))
def test_map_frame_with_one_stream_delayed_leaves_the_same_bits(name):
    kw, sites = MAP_FORMS[name]
    _order_test(MapForm(make_engine('hip'), name, **kw), sites, name)


# ---------------------------------------------------------------------------------------------- two calls on one work buffer, then the tracker
class TwoCalls:
    """The replica form twice in a row on the same `work` buffer and index handle with different draws - the second call 2 + 3 iterations, so
    it ends inside a look-ahead chunk - and then one lk_track_frame on the map they leave: the e1 join, the ev ring and the handle's seg_*
    counters across calls, the trunk fragments the tracker reads behind a split step.  No host synchronisation in between."""
    TRACK_R, TRACK_ITERS = 64, 4

    def __init__(self, eng):
        self.eng = eng
        self.m = MapForm(eng, 'two-calls', rel_pos=True, R=512)
        m = self.m
        self.to = steps.TrackOptimizer(eng, core.RenderCfg(rel_pos=True), m.dec, m.knn, m.dpos, m.dgeo, m.dcol, self.TRACK_R, 0.002, separate_lr=True, w_color=0.5)
        assert self.to.native_loop
        depth_s, color_s, pose_s = _frames()
        self.cam0 = eng.f32(H.c2w_to_cam(pose_s[1]) + torch.tensor([0.0, 0.002, -0.001, 0.0015, 0.004, -0.003, 0.002]))
        self.last_us = None

    def run(self, seed, timed=False):
        eng, m = self.eng, self.m
        m.reset()
        win = (20, HH - 20, 20, WW - 20)
        rnd_t = torch.randint(0, (win[1] - win[0]) * (win[3] - win[2]), (self.TRACK_ITERS, self.TRACK_R), generator=torch.Generator().manual_seed(seed + 5),
                              dtype=torch.int32).to(eng.device)
        rnd1, rnd2 = _draws(seed, N_GEO + N_COL, m.R).to(eng.device), _draws(seed + 31, 5, m.R).to(eng.device)
        log1, log2 = eng.zeros(N_GEO + N_COL, 4), eng.zeros(5, 4)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        m.mo.run(N_GEO + N_COL, N_GEO, m.frames, rnd1, m.fid, (0, HH, 0, WW), A.INTR, HH, WW, log1)
        e1.record()
        m.mo.new_frame(m.rows, m.mask)
        m.mo.run(5, 2, m.frames, rnd2, m.fid, (0, HH, 0, WW), A.INTR, HH, WW, log2)
        best, tlog = self.to.track(self.cam0, m.frames[0][1], m.frames[1][1], self.TRACK_ITERS, win, A.INTR, rnd_t)
        torch.cuda.synchronize()
        self.last_us = 1e3 * e0.elapsed_time(e1) / (N_GEO + N_COL)
        hist = self.to._keep_native[5]
        assert tuple(hist.shape) == (self.TRACK_ITERS, 7) and eng.status(sync=True) == 0
        return dict(log=_np(log1), log2=_np(log2), blob=_np(m.dec.blob), geo=_np(m.dgeo), col=_np(m.dcol), best=_np(best), hist=_np(hist), tlog=_np(tlog))

    def check_path(self, out):
        self.m.check_path(out)
        assert np.isfinite(out['log2']).all() and np.isfinite(out['tlog']).all() and float(np.abs(out['hist'][-1] - out['hist'][0]).sum()) > 0


@pytest.mark.gpu
def test_two_map_calls_and_a_track_call_with_one_stream_delayed_leave_the_same_bits():
    _order_test(TwoCalls(make_engine('hip')), (AHEAD, LAUNCH, WGRAD), 'two-calls')


# ---------------------------------------------------------------------------------------------- standalone forward + backward
class BwdForm:
    """core.render_forward + core.render_backward ('color' stage, feature and weight gradients, 96 rays with holes), twice back to back on
    ONE index handle and one stream without a host synchronisation: the second call's counting sort meets the first gather's counters.
    unit False: without LK_FLAG_UNIT_LOSS_GRADS the rel-pos backward is the unfused one, whose rows the weight-gradient stream waits for
    (`mid`).  (LK_FUSE_SMALL is a flag of the tracker's loop; lk_render_bwd never takes it.)"""

    def __init__(self, eng, name, R=96, n_points=N_POINTS):
        self.eng, self.name, self.R = eng, name, R
        rel_pos, self.unit = name != 'bwd-plain', name != 'bwd-relpos-unfused'
        if n_points is None:          # emulator: the small golden scene
            from util import load, tens
            g = load('g6_render_replica_map_color')
            pos, geo, col = tens(g, 'pos', 'geo', 'col')
            self.batches = {}
            self._golden = g
        else:
            pos, geo, col = A.scene(n_points)
            self._golden = None
        self.cfg = core.RenderCfg(rel_pos=rel_pos)
        self.dec = core.DecoderBlob(eng).pack(syn.default_weights(rel_pos=rel_pos))
        self.dpos, self.dgeo, self.dcol = eng.f32(pos), eng.f32(geo), eng.f32(col)
        self.knn = core.KnnIndex(eng, capacity=pos.shape[0])
        self.knn.build(self.dpos)
        self.pair = [(core.RenderState(eng, R, self.cfg.S, need_act=True), core.GradState(eng, pos.shape[0], R, self.dec.n, feats=True, weights=True)) for _ in range(2)]
        self.last_us = None

    def _batch(self, seed, k):
        if self._golden is not None:
            from util import tens
            ro, rd, gd, gc = tens(self._golden, 'rays_o', 'rays_d', 'gt_depth', 'gt_color')
            o = (seed + 3 * k) % 5
            return dict(rays_o=ro[o:o + self.R].contiguous(), rays_d=rd[o:o + self.R].contiguous(), gt_depth=gd[o:o + self.R].contiguous(), gt_color=gc[o:o + self.R].contiguous())
        return A.ray_batch(self.R, frame=7 + k, holes=0.3, seed=seed + k)

    def run(self, seed, timed=False):
        eng = self.eng
        cuda = eng.device.type == 'cuda'
        ins = []
        for k in range(2):
            b = self._batch(seed, k)
            ins.append(tuple(eng.f32(b[q]) for q in ('rays_o', 'rays_d', 'gt_depth', 'gt_color')) + (eng.zeros(self.R), eng.zeros(self.R, 3), eng.zeros(4)))
        xf = _ffi.FLAG_ZERO_ABSENT | (_ffi.FLAG_UNIT_LOSS_GRADS if self.unit else 0)
        if cuda:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
        for (st, gs), (ro, rd, gd, gc, d_depth, d_color, out4) in zip(self.pair, ins):
            gs.zero_()
            core.render_forward(eng, self.cfg, st, ro, rd, gd, self.knn, self.dpos, self.dgeo, self.dcol, self.dec, 'color', save_act=True, extra_flags=xf,
                                mapper_loss=(gc, 0.1, d_depth, d_color, out4))
            core.render_backward(eng, st, gs, d_depth, d_color)
        if cuda:
            e1.record()
            torch.cuda.synchronize()
            self.last_us = 1e3 * e0.elapsed_time(e1) / 2
        assert eng.status(sync=cuda) == 0
        out = {}
        for k, ((st, gs), i) in enumerate(zip(self.pair, ins)):
            out.update({'%s%d' % (n, k): _np(t) for n, t in (('depth', st.depth), ('color', st.color), ('out4', i[6]), ('g_geo', gs.g_geo), ('g_col', gs.g_col),
                                                              ('g_weights', gs.g_weights))})
        return out

    def check_path(self, out):
        for k in range(2):
            assert np.isfinite(out['out4%d' % k]).all() and 0 < out['out4%d' % k][3] < self.R, 'holes: some rays live, some not'
            for n in ('g_geo', 'g_col', 'g_weights'):
                assert np.isfinite(out['%s%d' % (n, k)]).all() and float(np.abs(out['%s%d' % (n, k)]).sum()) > 0, (n, k)
        assert out['g_geo0'].tobytes() != out['g_geo1'].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['bwd-plain', 'bwd-relpos', 'bwd-relpos-unfused'])
def test_standalone_backward_with_one_stream_delayed_leaves_the_same_bits(name):
    _order_test(BwdForm(make_engine('hip'), name), (SORT, WGRAD, LAUNCH), name)


# ---------------------------------------------------------------------------------------------- phase-split caller
class PhaseSplit:
    """lk_map_frame with phases = 1 then 2 per iteration, as parallel.py drives it: between the phases a second torch stream waits with
    lk_map_wait_rows / lk_map_wait_lists and copies that iteration's feature-gradient rows and neighbour lists; the launch stream waits
    for the copies before the step clears the gradients."""
    ITERS, N_GEO_IT = 9, 2                  # chunks {0}, {1..6}, {7, 8}

    def __init__(self, eng):
        self.eng = eng
        self.m = MapForm(eng, 'phase-split', rel_pos=True, R=512)
        self.side = torch.cuda.Stream(eng.device)
        self.last_us = None

    def run(self, seed, timed=False):
        eng, m, iters = self.eng, self.m, self.ITERS
        dll = eng.lib.dll
        m.reset()
        rnd = _draws(seed, iters, m.R).to(eng.device)
        log = eng.zeros(iters, 4)
        mo = m.mo
        d, _ = mo._native_desc(iters, self.N_GEO_IT, m.frames, rnd, m.fid, (0, HH, 0, WW), A.INTR, HH, WW, log)
        d.signal_rows = 1
        mo._nat_desc = d
        n_rows = m.rows.numel()
        rows_l = m.rows.long()
        g_copy = eng.zeros(iters, n_rows, 32)
        idx_copy = torch.zeros(iters, m.R * mo.cfg.S * 8, dtype=torch.int32, device=eng.device)
        main = torch.cuda.current_stream(eng.device)
        ev = [torch.cuda.Event() for _ in range(iters)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for it in range(iters):
            eng.lib.check(dll.lk_map_frame(C.byref(d), it, it + 1, 1, eng.stream), 'lk_map_frame')
            with torch.cuda.stream(self.side):
                # ordered behind nothing but the library's own events: the rows event and the look-ahead chunk's event
                eng.lib.check(dll.lk_map_wait_rows(C.byref(d), eng.stream), 'lk_map_wait_rows')
                mo.wait_lists(it)
                torch.index_select(mo.gs.g_geo, 0, rows_l, out=g_copy[it])
                idx_copy[it].copy_(mo.nbr_idx_of(it))
                ev[it].record(self.side)
            main.wait_event(ev[it])
            eng.lib.check(dll.lk_map_frame(C.byref(d), it, it + 1, 2, eng.stream), 'lk_map_frame')
        e1.record()
        torch.cuda.synchronize()
        self.last_us = 1e3 * e0.elapsed_time(e1) / iters
        assert eng.status(sync=True) == 0
        return dict(log=_np(log), blob=_np(m.dec.blob), geo=_np(m.dgeo), col=_np(m.dcol), g_rows=_np(g_copy), nbr_idx=_np(idx_copy))

    def check_path(self, out):
        self.m.check_path(out)
        assert all(float(np.abs(out['g_rows'][it]).sum()) > 0 for it in range(self.ITERS)), 'a copy of the gradient rows ran ahead of the gather (or behind the step)'
        N = self.m.dpos.shape[0]
        assert (out['nbr_idx'] >= -1).all() and (out['nbr_idx'] < N).all() and all((out['nbr_idx'][it] >= 0).any() for it in range(self.ITERS))


@pytest.mark.gpu
def test_phase_split_caller_with_one_stream_delayed_sees_the_same_rows_and_lists():
    _order_test(PhaseSplit(make_engine('hip')), (LAUNCH, AHEAD), 'phase-split')


# ---------------------------------------------------------------------------------------------- the workload's render stream
RS_CAM = dict(H=120, W=160, fx=129.3, fy=129.1, cx=79.6, cy=63.8)          # a quarter of the 640 x 480 camera: 19 200 rays per full-frame render


def _sleep_cycles(us):
    """torch.cuda._sleep counts device clock cycles: calibrated here with events, 1.5 x the cycles that took `us`."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    n = 2_000_000
    e0.record(); torch.cuda._sleep(n); e1.record()
    torch.cuda.synchronize()
    per_us = n / (1e3 * e0.elapsed_time(e1))
    return int(1.5 * us * per_us), e0, e1


def _workload_run(eng, tmp, sleep_on, cycles):
    """Two steps of the smallest Replica-model budget that maps and renders a frame: step 0 maps (insertion, iterations, full-frame render on
    wl.render_stream), step 1 tracks beside that render and joins it in front of its own mapping iterations.  sleep_on 'render': a sleep on
    the render stream before each step (the render LATE: it must still read the map of step 0); 'launch': a sleep on the current stream
    right behind step 0 (the render AHEAD of the launch stream).  Returns bench.dump_outputs' arrays and the sleep's measured microseconds."""
    import bench
    from loopy_slam_amd import workload
    b = workload.Budget(window=3, every_frame=2, track_iters=3, track_rays=48, map_iters=5, map_geo_iters=2, map_rays=240, n_points=6000, pixels_adding=200,
                        ignore_edge=8, online_cloud=False)
    pos, geo, col = (t.to(eng.device) for t in syn.build_cloud(b.n_points, device='cpu', seed=3, intr=RS_CAM))
    wl = workload.FrameWorkload(eng, b, cloud=(pos, geo, col, 1), intr=RS_CAM)
    assert wl.render_stream is not None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    for k in range(2):
        if sleep_on == 'render':
            with torch.cuda.stream(wl.render_stream):
                if k == 0:
                    e0.record()
                torch.cuda._sleep(cycles)
                if k == 0:
                    e1.record()
        last = wl.step(full=True)
        if sleep_on == 'launch' and k == 0:
            e0.record(); torch.cuda._sleep(cycles); e1.record()
    torch.cuda.synchronize()
    assert wl.n_added > 0 and wl.img_state is not None and eng.status(sync=True) == 0
    slept = 1e3 * e0.elapsed_time(e1) if sleep_on else 0.0
    bench.dump_outputs(str(tmp), wl, last)
    return {q.stem: np.load(q) for q in tmp.glob('*.npy')}, slept


@pytest.mark.gpu
def test_workload_render_stream_late_or_ahead_leaves_the_same_dump(tmp_path):
    eng = make_engine('hip')
    cycles, _, _ = _sleep_cycles(DELAY_US)
    ref, _ = _workload_run(eng, tmp_path / 'ref', None, cycles)
    assert np.isfinite(ref['render_depth']).all() and float(np.abs(ref['render_color']).sum()) > 0 and np.isfinite(ref['map_log']).all()
    again, _ = _workload_run(eng, tmp_path / 'again', None, cycles)
    _same_bits(again, ref, 'the undelayed workload twice (the premise)')
    for where in ('render', 'launch'):
        got, slept = _workload_run(eng, tmp_path / where, where, cycles)
        print('render-stream: sleep on the %s stream took %.0f us' % (where, slept))
        assert slept >= DELAY_US, (where, slept)
        _same_bits(got, ref, 'the workload with a %d us sleep on the %s stream' % (DELAY_US, where))
