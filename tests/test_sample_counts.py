"""Every samples-per-ray count the ABI accepts (1 <= S <= LK_S_MAX = 8), not only the S = 5 of the shipped configs: the render's forward and
backward per call, the fused loss forms, the two per-frame loops, the tile switch of the tracker's fused forward, and the refusal of a
count outside the range.  S decides which launch form is taken and how lanes map to rays:

  S      tracker forward (lk_launch_relpos_decode_fwd)                 decoder backward (32-sample tiles)
  1-3    plain 32-sample tiles, pass 1 of the loss in k_track_composite  rays straddle tiles at S = 3
  4, 8   loss epilogue, tile stride 32 (8 / 4 whole rays per tile)      tiles hold whole rays
  6, 7   loss epilogue, tile stride 30 / 28 (5 / 4 rays, lanes idle)    rays straddle tiles

Reference: oracle/hotpath.py, which is generic in S, on the committed replica / tum inputs (96 rays, 1 308 points) and on
test_steps_parity.mini_scene; gradients through the float64 referee of tests/test_parity_at_size.py.  Both back-ends (see
test_forward_parity.py) unless a case says why not.  Measured distances: sample_counts.json, beside the
report of tests/test_parity_at_size.py."""
import numpy as np
import pytest
import torch

import atsize as A
import switch_referee as sw
import test_parity_at_size as P
from oracle import hotpath as H
from loopy_slam_amd import _ffi, core, optim, steps, synthetic as syn
from util import load, tens, weights, CFG, make_engine, backends
from test_forward_parity import rcfg, ocfg, check_outputs
from test_steps_parity import mini_scene, oracle_rays, HH, WW, INTR
from test_loss_forms import same_bits, check_sums, SUM_RTOL, _St
from test_loops_at_size import param_error_stats, stiff_call_ok
from test_size_switches import guarded, bits

torch.set_num_threads(1)

S_CALL = (1, 2, 3, 4, 6, 7, 8)          # section A: every accepted count but the 5 of the rest of the suite
S_LOOP = (3, 4, 7, 8)                   # sections B and C: k_track_composite, stride 32 with 8 rays, stride 28, stride 32 with 4 rays (full arrays)
SENTINEL = 77.0
_REPORT = {}


def _record(case, **kv):
    """This module's report, written as and where test_parity_at_size._record writes its own."""
    P._record(case, _file='sample_counts.json', _report=_REPORT, **kv)


def _sync(eng):
    if eng.device.type == 'cuda':
        torch.cuda.synchronize()


def tile_stride(S):
    """Samples per tile of the tracker's fused forward: whole rays (lk_decode.hip: tile_stride = (32 / S) * S)."""
    return (32 // S) * S


def test_counts_mirror_the_define():
    """The lists of this module against LK_S_MAX (switch_referee.S_MAX, which test_size_switches.py holds to the header)."""
    assert sw.S_MAX == _ffi.LK_S_MAX
    assert S_CALL == tuple(s for s in range(1, sw.S_MAX + 1) if s != sw.S)
    assert set(S_LOOP) <= set(S_CALL) and max(S_LOOP) == sw.S_MAX
    assert [tile_stride(s) for s in (4, 5, 6, 7, 8)] == [32, 30, 30, 28, 32]


# ---------------------------------------------------------------------------- A. per-call forward and backward
R_GOLDEN = 96


def ragged_rays(S):
    """The largest prefix of the golden's 96 rays whose sample count P = R S is ragged against all three tilings: the 32-sample tiles of
    the decoders (P % 32), the whole-ray tiles of the tracker's fused forward (P % tile_stride) and the four samples per wave of the
    rel-pos MLP (P % 4, where S allows it: not at S = 4 and 8)."""
    for R in range(R_GOLDEN - 1, 0, -1):
        Pn = R * S
        if Pn % 32 and Pn % tile_stride(S) and (Pn % 4 or S % 4 == 0):
            return R
    raise AssertionError(S)


def prefixes(S):
    """(ragged, full): `ragged` as above - the last tile of every tiling is partial; `full` = all 96 rays: P = 96 S is a multiple of 32
    at every S, the last 32-sample tile is full (and at S = 3, 6, 7 the whole-ray tiles are still ragged: 288 % 30, 576 % 30, 672 % 28)."""
    return ragged_rays(S), R_GOLDEN


def test_prefixes_are_ragged_and_full():
    assert {S: prefixes(S) for S in S_CALL} == {1: (95, 96), 2: (95, 96), 3: (95, 96), 4: (95, 96), 6: (93, 96), 7: (95, 96), 8: (95, 96)}
    for S in S_CALL:
        r, f = prefixes(S)
        assert (f * S) % 32 == 0 and (r * S) % 32 != 0 and (r * S) % tile_stride(S) != 0 and r * S > 32


MODES = {'geometry': 'map_geometry', 'color': 'map_color', 'track': 'track', 'img': 'img'}
# (kind, mode, LK_FLAG_UNIT_LOSS_GRADS, LK_FLAG_GRAD_GEO_DECODER)
KINDS = (('map-geometry', 'geometry', False, False), ('map-geometry-unit', 'geometry', True, False), ('map-geometry-unit-geodec', 'geometry', True, True),
         ('map-color', 'color', False, False), ('map-color-unit', 'color', True, False), ('map-color-unit-geodec', 'color', True, True),
         ('track', 'track', False, False), ('img', 'img', False, False))
# Share of a case's rays that may leave the gradient comparison because they sit on a branch point (atsize.branch_point_rays).  Counted
# over the rays that SEE the cloud (valid_ray): 24 of the golden's 96 rays - every fourth - look past it, all their samples carry the same
# weight, and with samples symmetric about the reading they render depth == gt_depth to rounding at every S >= 2: the L1 kink.  The mapper's
# loss leaves such rays out anyway (valid_ray); the tracker's does not, so in tracker mode they are zeroed on both sides at any prefix.
MAX_EXCLUDED = 0.05
PAST_THE_CLOUD = 24          # and the share of ALL excluded rays is capped as well: those 24 of 96 plus 5 %
_GOLD, _ORACLE = {}, {}


def _golden(model, mode):
    if (model, mode) not in _GOLD:
        _GOLD[(model, mode)] = (load(f'g6_render_{model}_{MODES[mode]}'), weights(model))
    return _GOLD[(model, mode)]


def _r2_ray(model, g, R):
    return (torch.from_numpy(g['r_query'][:R]) ** 2).float() if CFG[model]['dynamic'] else None


def _oracle_run(model, mode, S, R, knn=None, exclude=None, grads=True, f64=False, var_const=None):
    """oracle/hotpath.py on the first R rays of the golden at S samples per ray (no feature noise: atsize.geo_gate_margin has none), the
    mapper's or the tracker's loss and its autograd - to feature rows and decoder weights (mapper), to the rays (tracker).
    f64: inside atsize.ref64, the float64 referee on the same rounded inputs."""
    g, W = _golden(model, mode)
    c = A.to64 if f64 else (lambda x: x)
    tracker, stage = mode == 'track', 'geometry' if mode == 'geometry' else 'color'
    ro, rd, gd = (t[:R] for t in tens(g, 'rays_o', 'rays_d', 'gt_depth'))
    pos, geo, col = tens(g, 'pos', 'geo', 'col')
    names = [k for k in W if k != 'color_decoder.embedder._B']
    gp, gr = grads and not tracker, grads and tracker
    Wr = {k: c(v).clone().requires_grad_(gp and k in names) for k, v in W.items()}
    geo_r, col_r = c(geo).clone().requires_grad_(gp), c(col).clone().requires_grad_(gp)
    ro_r, rd_r = c(ro).clone().requires_grad_(gr), c(rd).clone().requires_grad_(gr)
    o = H.render_batch(ocfg(model, S), ro_r, rd_r, c(gd), c(pos), geo_r, col_r, Wr, stage, tracker=tracker, r2_ray=_r2_ray(model, g, R),
                       knn=None if knn is None else c(tuple(knn)))
    res = dict(out=o)
    if mode == 'img':
        return res
    gc, w_color = c(torch.from_numpy(g['gt_color'][:R])), float(g['w_color'])
    if tracker:
        var = o['var'] if var_const is None else var_const
        res['loss'] = loss = H.tracker_loss(o['depth'], var, o['color'], c(gd), gc, w_color)
        if grads and exclude is not None:           # the same loss without the excluded rays' terms (mask and mean are the full batch's)
            m = loss[3] & ~exclude
            tmp = torch.abs(c(gd) - o['depth']) / torch.sqrt(var.detach() + 1e-10)
            (torch.clamp(tmp, min=0.0, max=1e3)[m].sum() + w_color * torch.abs(gc - o['color'])[m].sum()).backward()
        elif grads:
            loss[0].backward()
        res.update(g_rays_o=ro_r.grad, g_rays_d=rd_r.grad)
    else:
        res['loss'] = H.mapper_loss(o['depth'], o['color'], o['valid_ray'], c(gd), gc, stage, w_color)
        if grads:
            valid = o['valid_ray'] if exclude is None else o['valid_ray'] & ~exclude
            H.mapper_loss(o['depth'], o['color'], valid, c(gd), gc, stage, w_color)[0].backward()
            res.update(g_geo=geo_r.grad, g_col=col_r.grad if col_r.grad is not None else torch.zeros_like(col),
                       gW={k: Wr[k].grad for k in names if Wr[k].grad is not None})
    return res


EPS32 = 2.0 ** -23


def _residue_scale(model, mode, R, knn, exclude):
    """S = 1: the size a rounding residue may have in the geometry path's gradients, from the fp32 oracle alone.  With one sample
    depth = w z / (w + 1e-10) and d depth / d w = (z - depth) / (w + 1e-10): z - depth is 1e-10 z / (w + 1e-10) in exact arithmetic (~4e-10 z
    at the w >= 0.27 of a sample with neighbours) and, in fp32, the three roundings of depth (product, sum, quotient: half an ulp each, the
    difference itself is exact), |z - depth| <= 2 eps z with eps = 2^-23; the colour (w rgb / (w + 1e-10)) likewise.  What a correct fp32
    implementation hands on is therefore sum_r c_r dw_r / d theta with |c_r| <= 2 eps (|d L / d depth_r| z_r + sum_c |d L / d colour_rc| rgb_rc) / w_r.
    Returned per tensor: the largest entry of that sum with every c_r at its limit and of one sign, WITHOUT the 2 eps - the gradient of
    sum_r (|d depth_r| z_r + |d colour_r| . rgb_r) log w_r.  A value routed through a wrong lane or sample is of that size, not 2 eps of it."""
    g, W = _golden(model, mode)
    ro, rd, gd = (t[:R] for t in tens(g, 'rays_o', 'rays_d', 'gt_depth'))
    pos, geo, col = tens(g, 'pos', 'geo', 'col')
    names = [k for k in W if k.startswith('geo_decoder.')]
    Wr = {k: v.clone().requires_grad_(k in names) for k, v in W.items()}
    geo_r = geo.clone().requires_grad_(True)
    o = H.render_batch(ocfg(model, 1), ro, rd, gd, pos, geo_r, col, Wr, mode, r2_ray=_r2_ray(model, g, R), knn=tuple(knn))
    depth, color = o['depth'].detach().requires_grad_(True), o['color'].detach().requires_grad_(True)
    H.mapper_loss(depth, color, o['valid_ray'] & ~exclude, gd, torch.from_numpy(g['gt_color'][:R]), mode, float(g['w_color']))[0].backward()
    dd = depth.grad.abs()
    dc = color.grad.abs() if color.grad is not None else torch.zeros(R, 3)
    ((dd * o['z'][:, 0] + (dc * o['rgb'].detach().reshape(R, 3).abs()).sum(1)) * torch.log(o['w'][:, 0])).sum().backward()
    res = {k: float(Wr[k].grad.abs().max()) for k in names if Wr[k].grad is not None}
    res['geo_feats'] = float(geo_r.grad.abs().max())
    return res


def _oracle(model, mode, S, R):
    """Everything the oracle says about a case, computed once per process: forward, branch-point rays, fp32 and float64 gradients."""
    key = (model, mode, S, R)
    if key in _ORACLE:
        return _ORACLE[key]
    g, W = _golden(model, mode)
    with torch.no_grad():
        r0 = _oracle_run(model, mode, S, R, grads=False)
    o = r0['out']
    kn = (o['d2'].numpy(), o['idx'].numpy(), o['count'].numpy())
    res = dict(r0=r0, knn=kn)
    if mode == 'img' or S == 1:
        with torch.no_grad(), A.ref64():
            res['var64'] = _oracle_run(model, mode, S, R, knn=kn, grads=False, f64=True)['out']['var']
    if mode != 'img':
        pos, geo = tens(g, 'pos', 'geo')
        r2 = _r2_ray(model, g, R)
        bp, margin = A.branch_point_rays(o, dict(gt_depth=torch.from_numpy(g['gt_depth'][:R])), pos, geo, W, tracker_loss=True if mode == 'track' else None,
                                         r2=None if r2 is None else r2.reshape(-1, 1).repeat(1, S).reshape(-1))
        res.update(bp=bp, margin=margin)
        res['r32'] = _oracle_run(model, mode, S, R, knn=kn, exclude=bp)
        if S == 1 and mode != 'track':
            res['residue_scale'] = _residue_scale(model, mode, R, kn, bp)
        with A.ref64():
            res['r64'] = _oracle_run(model, mode, S, R, knn=kn, exclude=bp, f64=True,
                                     var_const=res['r32']['out']['var'].detach().double() if mode == 'track' else None)
    _ORACLE[key] = res
    return res


def _cases():
    return [(model, S, R) for model in ('replica', 'tum') for S in S_CALL for R in prefixes(S)]


def _call_cases():
    """(LK_FLAG_GRAD_GEO_DECODER with the replica model only: the stand-alone geometry weight-gradient launch does not depend on the model.)"""
    return [c + k for c in _cases() for k in KINDS if c[0] == 'replica' or not k[3]]


@pytest.mark.parametrize('model', ('replica', 'tum'))
def test_prefixes_stay_within_the_exclusion_cap(model):
    """With the oracle alone: at most 5 % of the rays of every chosen prefix sit on a branch point of the graph (a ReLU gate or an L1 kink at
    rounding level, a neighbour on the radius edge or a residual on the mask's threshold in tracker mode) and leave the gradient comparison."""
    worst = 0.0
    for m, S, R in _cases():
        if m != model:
            continue
        for mode in ('geometry', 'color', 'track'):
            with torch.no_grad():
                o = _oracle_run(model, mode, S, R, grads=False)['out']
            g, W = _golden(model, mode)
            r2 = _r2_ray(model, g, R)
            bp, _ = A.branch_point_rays(o, dict(gt_depth=torch.from_numpy(g['gt_depth'][:R])), *tens(g, 'pos', 'geo'), W,
                                        tracker_loss=True if mode == 'track' else None, r2=None if r2 is None else r2.reshape(-1, 1).repeat(1, S).reshape(-1))
            n_ex = int((bp & o['valid_ray']).sum())
            worst = max(worst, n_ex / R)
            assert n_ex <= MAX_EXCLUDED * R, (model, mode, S, R, n_ex)
            assert int((bp & ~o['valid_ray']).sum()) <= PAST_THE_CLOUD
            assert int(bp.sum()) <= PAST_THE_CLOUD + MAX_EXCLUDED * R, (model, mode, S, R, int(bp.sum()))
    print(f'{model}: largest excluded share {worst:.3f}')


def _referee_value(name, got, o32, r64, case):
    """A rendered VALUE by the rule of test_parity_at_size._check_grad: no farther from the float64 evaluation of the same rounded inputs than
    REF_FACTOR times the fp32 oracle is, or than the max-norm floor."""
    got, o32, r64 = (torch.as_tensor(x).double().reshape(-1) for x in (got, o32, r64))
    s = float(r64.abs().max()) + 1e-300
    e_hip, e_o32 = float((got - r64).abs().max()) / s, float((o32 - r64).abs().max()) / s
    _record(case, **{f'{name}_hip_vs_f64_max': e_hip, f'{name}_o32_vs_f64_max': e_o32})
    assert e_hip <= max(P.REF_FACTOR * e_o32, P.REF_FLOOR_MAX), (case, name, 'max-norm vs float64', e_hip, e_o32)


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('model,S,R,kind,mode,unit,geo_dec', _call_cases(), ids=['-'.join(str(x) for x in c[:4]) for c in _call_cases()])
def test_render_call_vs_oracle(backend, model, S, R, kind, mode, unit, geo_dec):
    """lk_render_fwd (+ the fused mapper loss / lk_loss_tracker) and lk_render_bwd on a prefix of the golden's rays (prefixes: why these) at S
    samples per ray.  replica: rel-pos colour MLP; tum: per-ray dynamic radius.  Sample depths, neighbour lists, counts and valid_ray bit for
    bit; depth / colour / variance at check_outputs' bounds - at S = 1 the variance w (z - depth)^2 is a rounding residue of z - depth and
    is held by the referee rule instead (and the geometry path's gradients are a residue too: `held`); the mapper's loss at 1e-4; every
    gradient tensor by test_parity_at_size._check_grad against the float64 referee, rays on a branch point excluded on both sides
    (MAX_EXCLUDED: at most 5 % of the case's rays).  img: the render_img-style forward on the golden with 20 rays without a depth reading -
    the absent-ray path of lk_composite_vals."""
    case = f'{model}-{kind}-S{S}-R{R}'
    eng = make_engine(backend)
    g, W = _golden(model, mode)
    ref = _oracle(model, mode, S, R)
    o = ref['r0']['out']
    tracker, stage = mode == 'track', 'geometry' if mode == 'geometry' else 'color'
    cfg = rcfg(model, S)
    dec = core.DecoderBlob(eng).pack(W)
    ro, rd, gd = (eng.f32(t[:R]) for t in tens(g, 'rays_o', 'rays_d', 'gt_depth'))
    pos, geo, col = (eng.f32(t) for t in tens(g, 'pos', 'geo', 'col'))
    knn = core.KnnIndex(eng, capacity=pos.shape[0])
    knn.build(pos)
    r2 = _r2_ray(model, g, R)
    r2d = eng.f32(r2) if r2 is not None else None
    st = core.RenderState(eng, R, S, need_act=mode != 'img')
    if mode == 'img':
        assert int((g['gt_depth'][:R] == 0).sum()) >= 19
        core.render_forward(eng, cfg, st, ro, rd, gd, knn, pos, geo, col, dec, 'color', r2_ray=r2d)
    else:
        gc, w_color = eng.f32(g['gt_color'][:R]), float(g['w_color'])
        d_depth, d_color, out4 = eng.empty(R), eng.empty(R, 3), eng.zeros(4)
        xf = _ffi.FLAG_ZERO_ABSENT | (_ffi.FLAG_UNIT_LOSS_GRADS if unit else 0)
        core.render_forward(eng, cfg, st, ro, rd, gd, knn, pos, geo, col, dec, stage, tracker=tracker, r2_ray=r2d, save_act=True, extra_flags=xf,
                            mapper_loss=None if tracker else (gc, w_color, d_depth, d_color, out4))
        if tracker:
            optim.loss_tracker(eng, st, gd, gc, w_color, True, d_depth, d_color, out4, eng.empty(R + 8))
    _sync(eng)
    # ---- forward
    assert np.array_equal(st.z.cpu().numpy(), o['z'].numpy())
    assert np.array_equal(st.nbr_idx.cpu().numpy(), o['idx'].numpy())
    assert np.array_equal(st.nbr_count.cpu().numpy(), o['count'].numpy())
    _record(case, depth_rel=A.errs(st.depth.cpu(), o['depth'])[0], color_rel=A.errs(st.color.cpu(), o['color'])[0], var_rel=A.errs(st.var.cpu(), o['var'])[0])
    check_outputs(st, dict(valid_ray=o['valid_ray'].numpy(), depth=o['depth'].numpy(), var=o['var'].numpy(), color=o['color'].numpy()), has_var=S > 1)
    if S == 1:
        _referee_value('var', st.var.cpu(), o['var'], ref['var64'], case)
    if mode == 'img':
        return
    loss = ref['r0']['loss']
    o4 = out4.cpu().numpy()
    _record(case, loss_rel=abs(o4[0] - float(loss[0])) / abs(float(loss[0])), masked=int(loss[3].sum()))
    if tracker:
        # The tracker's loss divides |gt - depth| by sqrt(var): on the rays that look past the cloud (MAX_EXCLUDED) the residual is a rounding
        # residue over a variance of ~4e-8, a term of rounding-level SIGN and size ~1e-3 each - 2e-4 of the loss between any two fp32 renders.
        # So the loss kernel is held on the kernel's own render (which check_outputs has just held to the oracle's), at the bound of
        # test_parity_at_size.py::test_tracker_median_mask_at_bench_size; the distance to the oracle's loss is recorded.
        loss = H.tracker_loss(st.depth.cpu(), st.var.cpu(), st.color.cpu(), torch.from_numpy(g['gt_depth'][:R]), torch.from_numpy(g['gt_color'][:R]), w_color)
        _record(case, loss_rel_on_own_render=abs(o4[0] - float(loss[0])) / abs(float(loss[0])))
    assert int(o4[3]) == int(loss[3].sum()) > R // 2
    assert abs(o4[0] - float(loss[0])) <= (2e-5 if tracker else P.TOL_OUT) * abs(float(loss[0]))
    # ---- backward: rays on a branch point get a zero loss gradient on both sides
    bp = ref['bp']
    n_ex = int((bp & o['valid_ray']).sum())
    _record(case, excluded_rays=n_ex, excluded_share=n_ex / R, excluded_rays_past_the_cloud=int((bp & ~o['valid_ray']).sum()), relu_margin_min=ref['margin'])
    _record(case, excluded_share_total=int(bp.sum()) / R)
    assert n_ex <= MAX_EXCLUDED * R and int(bp.sum()) <= PAST_THE_CLOUD + MAX_EXCLUDED * R
    if int(bp.sum()):
        d_depth[bp.to(eng.device)] = 0.0
        d_color[bp.to(eng.device)] = 0.0
    gs = core.GradState(eng, pos.shape[0], R, dec.n, feats=not tracker, weights=not tracker, rays=tracker)
    gs.geo_decoder = geo_dec
    core.render_backward(eng, st, gs, d_depth, d_color)
    _sync(eng)
    r32, r64 = ref['r32'], ref['r64']
    if tracker:
        P._check_grad('rays_o', gs.g_rays_o.cpu(), r32['g_rays_o'], case, ref64=r64['g_rays_o'], record=_record)
        P._check_grad('rays_d', gs.g_rays_d.cpu(), r32['g_rays_d'], case, ref64=r64['g_rays_d'], record=_record)
    else:
        def held(name, got, gref, g64):
            """At S = 1 the rendered depth and colour do not depend on the occupancy (w z / (w + 1e-10)): what reaches the geometry decoder and
            its feature rows is a rounding residue of z - depth in every implementation (float64: ~1e-10 of the gradient at S = 2), as
            the variance is - the referee's relative rule has nothing to hold on to.  A residue has a size, though (_residue_scale): the
            tensor's largest entry is held to REF_FACTOR times the larger of the fp32 oracle's own, the float64 value and 2 eps of the scale
            computed there.  Every other tensor goes to the referee."""
            if S == 1 and (name == 'geo_feats' or name.startswith('geo_decoder.')):
                scale = ref['residue_scale'][name]
                e_hip, e_o32, e_f64 = float(got.abs().max()), float(gref.abs().max()), float(g64.abs().max())
                _record(case, **{f'g[{name}]_residue_hip_max': e_hip, f'g[{name}]_residue_o32_max': e_o32, f'g[{name}]_residue_f64_max': e_f64,
                                 f'g[{name}]_residue_limit_2eps_scale': 2.0 * EPS32 * scale})
                assert bool(torch.isfinite(got).all()), (case, name)
                assert scale > 0 and e_hip <= P.REF_FACTOR * max(e_o32, e_f64, 2.0 * EPS32 * scale), (case, name, 'residue', e_hip, e_o32, e_f64, 2.0 * EPS32 * scale)
                return
            P._check_grad(name, got, gref, case, ref64=g64, record=_record)
        held('geo_feats', gs.g_geo.cpu(), r32['g_geo'], r64['g_geo'])
        if stage == 'color':
            P._check_grad('col_feats', gs.g_col.cpu(), r32['g_col'], case, ref64=r64['g_col'], record=_record)
        gW = dec.unpack(gs.g_weights)
        n = 0
        for name, gref in r32['gW'].items():
            if name.startswith('geo_decoder.') and name != 'geo_decoder.embedder._B' and not geo_dec:
                continue                          # frozen in every reference config
            if name not in gW or (stage == 'geometry' and not name.startswith('geo_decoder.')):
                continue
            held(name, gW[name].reshape(gref.shape), gref, r64['gW'][name])
            n += 1
        assert n >= (1 if stage == 'geometry' else (27 if CFG[model]['rel_pos'] else 22)) + (22 if geo_dec else 0)


# ---------------------------------------------------------------------------- B. fused loss forms
FORM_R = (93, 96)


def fwd_pairs(R, S):
    """(sum, count) pairs pass 1 of the tracker's loss leaves: one per tile of whole rays where it is the fused forward's epilogue
    (4 <= S), one per 256 rays where it is k_track_composite (S <= 3, plain 32-sample forward tiles)."""
    return -(-R * S // tile_stride(S)) if S >= 4 else -(-R // 256)


def _regions(sizes):
    """{name: (offset, floats used)} of consecutive regions, each rounded up to 4 floats, and the total."""
    lay, o = {}, 0
    for name, n in sizes:
        lay[name] = (o, n)
        o += (n + 3) // 4 * 4
    return lay, o


def track_work_layout(R, S, iters):
    """lk_track_frame's work buffer, region by region, worked out HERE from what each launch writes (the guard behind the buffer only
    sees a write past its end; kernels and launcher share lk_loop.hip's track_work, so a region sized too small inside it spills into
    the next one unseen): the readings and pixels of every iteration's batch, one threshold per iteration, one residual per ray, pass 1's
    pairs - room for either form, ceil(P / tile_stride) of the epilogue or ceil(R / 256) -, and per 32-sample tile of the decoder
    BACKWARD 12 pose terms and a loss row of 4, then two poses [2][8] with their Adam moments [2][16]."""
    P = R * S
    tiles_bwd = -(-P // 32)
    return _regions((('gt_depth', iters * R), ('gt_color', iters * R * 3), ('pix_i', iters * R), ('pix_j', iters * R), ('r2_ray', iters * R), ('thr', iters),
                     ('resid', R), ('loss_part', 2 * max(-(-P // tile_stride(S)), -(-R // 256))), ('pose_part', 12 * tiles_bwd), ('row_part', 4 * tiles_bwd),
                     ('ring', 48)))


def map_work_layout(eng, R, S, iters):
    """lk_map_frame's work buffer likewise: the batches of every iteration (rays, readings, radius, threshold, live count, keyframe), their
    search results [iters][P] / [iters][P][K], the rows sorted by point (list, totals, rank and scratch for LK_SEG_BATCH iterations), the
    stepped decoder blob, a loss row of 4 per 32-sample BACKWARD tile and iteration, the second colour-feature buffer [P][C]."""
    K, C = (sw.source_define('../../include/loopy_hip.h', n) for n in ('LK_K', 'LK_C'))
    B = sw.source_define('lk_common.h', 'LK_SEG_BATCH')
    P = R * S
    return _regions((('rays_o', iters * R * 3), ('rays_d', iters * R * 3), ('gt_depth', iters * R), ('gt_color', iters * R * 3), ('r2_ray', iters * R), ('thr', iters),
                     ('n_live', iters), ('frame_id', iters * R), ('z', iters * P), ('nbr_idx', iters * P * K), ('nbr_w', iters * P * K), ('nbr_count', iters * P),
                     ('seg_list', iters * P * K), ('seg_total', iters), ('seg_rank', P * K * B), ('w_next', int(eng.lib.dll.lk_weight_blob_floats())),
                     ('loss_rows', iters * 4 * -(-P // 32)), ('c_col_alt', P * C), ('seg_tmp', P * K * B)))


def test_form_ray_counts():
    """93 rays leave the last whole-ray tile of the tracker's fused forward with fewer than 32 / S rays at every S of S_LOOP.  At S = 7 they
    make that forward's tile count differ from the backward's ceil(P / 32): 24 tiles of 28 samples against 21 of 32.  (S = 3 and 6 are the
    other counts at which the two would differ - 10 against 9 tiles at S = 3 - but at S = 3 the forward takes plain 32-sample tiles and pass 1
    runs in k_track_composite, one pair per 256 rays: the stride is arithmetic that path does not use; S = 6 is not among the loop
    counts the issue sets.)  96 rays fill the last tile at S = 4 and 8."""
    for S in S_LOOP:
        assert 93 % (32 // S) != 0
    assert fwd_pairs(93, 7) == 24 and -(-93 * 7 // 32) == 21
    assert [fwd_pairs(93, S) for S in S_LOOP] == [1, 12, 24, 24] and [fwd_pairs(96, S) for S in S_LOOP] == [1, 12, 24, 24]
    assert 96 % (32 // 4) == 0 and 96 % (32 // 8) == 0


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('S', S_LOOP)
def test_work_buffer_regions_add_up(backend, S):
    """lk_track_work_floats / lk_map_work_floats against the region sizes recomputed in this module (track_work_layout, map_work_layout),
    at the ray counts and iteration counts of the cases below: a region of the library's that shrinks - the forward's pairs counted in
    32-sample tiles, say: 21 against 24 at S = 7 - moves the total."""
    eng = make_engine(backend)
    for R in FORM_R:
        for iters in (1, LOOP_ITERS):
            assert track_work_layout(R, S, iters)[1] == int(eng.lib.dll.lk_track_work_floats(R, S, iters)), (R, iters)
            assert map_work_layout(eng, R, S, iters)[1] == int(eng.lib.dll.lk_map_work_floats(R, S, iters)), (R, iters)


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('stage', ('geometry', 'color'))
@pytest.mark.parametrize('R', FORM_R)
@pytest.mark.parametrize('S', S_LOOP)
def test_mapper_loss_inside_the_decoder_backward(backend, S, R, stage):
    """test_loss_forms.py::test_mapper_inside_the_decoder_backward at S samples per ray: one native one-iteration lk_map_frame call
    (lk_map_draw: every lane recomputes its whole ray with r = sp / S, the lane with sp % S == 0 stores it), then
      lk_loss_mapper on the depth / colour / valid_ray the call left: d depth / d colour bit for bit, the loss row at that file's bound;
      k_composite with the loss riding along (lk_render_fwd with LK_FLAG_MAPPER_LOSS) on the call's own batch and the parameters it started
        from: d depth / d colour bit for bit (+-1 / +-w), the masked-ray count exactly, valid_ray exactly, depth / colour / loss row at the
        forward's 1e-4 (the two launches reach the decoder through different forward kernels).
    The call's work buffer is the test's: exactly lk_map_work_floats floats, the guard behind it intact (a write past the END of the buffer;
    the regions inside it: map_work_layout, test_work_buffer_regions_add_up)."""
    eng = make_engine(backend)
    c2w, depth_img, color_img, pos, geo, col = mini_scene()
    rnd = torch.randint(0, HH * WW, (1, R), generator=torch.Generator().manual_seed(11), dtype=torch.int32)
    rnd[0, :4] = torch.tensor([0, 5, 17, 34], dtype=torch.int32)
    cfg = core.RenderCfg(S=S, rel_pos=True)
    W = syn.default_weights(seed=7)
    dec = core.DecoderBlob(eng).pack(W)
    pos_d, geo_d, col_d = eng.f32(pos), eng.f32(geo).clone(), eng.f32(col).clone()
    knn = core.KnnIndex(eng, capacity=pos.shape[0])
    knn.build(pos_d)
    rows = torch.arange(0, pos.shape[0], 2, dtype=torch.int32)
    lrs = {'geometry': (0.001, 0.03, 0.0), 'color': (0.005, 0.005, 0.005)}
    mo = steps.MapOptimizer(eng, cfg, dec, knn, pos_d, geo_d, col_d, rows.to(eng.device), R, lrs, w_color=0.1)
    mo.begin_frame()
    wfull, mo._work = guarded(eng, int(eng.lib.dll.lk_map_work_floats(R, S, 1)), torch.float32, SENTINEL)
    frames = (eng.f32(depth_img).reshape(1, HH, WW), eng.f32(color_img).reshape(1, HH, WW, 3), eng.f32(c2w).reshape(1, 4, 4), None)
    log = eng.zeros(1, 4)
    mo.run(1, 1 if stage == 'geometry' else 0, frames, rnd.to(eng.device), torch.zeros(R, dtype=torch.int32, device=eng.device), (0, HH, 0, WW), INTR, HH, WW, log)
    _sync(eng)
    assert bool((wfull[mo._work.numel():] == SENTINEL).all()), 'lk_map_frame wrote behind lk_map_work_floats'
    # the call's own batch (work buffer of a one-iteration call: rays_o [R][3] | rays_d [R][3] | gt_depth [R] | gt_color [R][3] | ..., each
    # rounded up to 4 floats)
    lay, total = map_work_layout(eng, R, S, 1)
    assert total == mo._work.numel()
    o_rd, o_gd, o_gc = lay['rays_d'][0], lay['gt_depth'][0], lay['gt_color'][0]
    ro, rd = mo._work[:3 * R].reshape(R, 3).clone(), mo._work[o_rd:o_rd + 3 * R].reshape(R, 3).clone()
    gd, gc = mo._work[o_gd:o_gd + R].clone(), mo._work[o_gc:o_gc + 3 * R].reshape(R, 3).clone()
    ref_gd = depth_img.reshape(-1)[rnd[0].long()]
    keep = (ref_gd > 0) & (ref_gd < 10)
    n_live = int((gd > 0).sum())
    assert n_live == int(keep.sum()) and 0 < n_live < R and bool((gd[:n_live] > 0).all())
    assert torch.equal(gd[:n_live].cpu(), ref_gd[keep])                       # the rays that keep a reading first, in draw order
    n = n_live
    st = _St()
    st.depth, st.color, st.valid_ray = mo.st.depth[:n].clone(), mo.st.color[:n].clone(), mo.st.valid_ray[:n].clone()
    dd, dc, out = eng.empty(n), eng.empty(n, 3), eng.empty(4)
    optim.loss_mapper(eng, st, gd[:n].clone(), gc[:n].clone(), 0.1, stage == 'color', dd, dc, out)
    assert same_bits(mo.batch.d_depth[:n], dd) and same_bits(mo.batch.d_color[:n], dc)
    assert float(dd.abs().sum()) > 0 and (float(dc.abs().sum()) > 0) == (stage == 'color')
    check_sums(log[0], out)
    # k_composite + loss on the same batch, from the parameters the call started with
    dec2 = core.DecoderBlob(eng).pack(W)
    st2 = core.RenderState(eng, n, S)
    dd2, dc2, out2 = eng.empty(n), eng.empty(n, 3), eng.zeros(4)
    core.render_forward(eng, cfg, st2, ro[:n].contiguous(), rd[:n].contiguous(), gd[:n].clone(), knn, pos_d, eng.f32(geo), eng.f32(col), dec2, stage,
                        extra_flags=_ffi.FLAG_ZERO_ABSENT, mapper_loss=(gc[:n].contiguous(), 0.1, dd2, dc2, out2))
    _sync(eng)
    assert same_bits(st2.valid_ray, st.valid_ray)
    np.testing.assert_allclose(st.depth.cpu().numpy(), st2.depth.cpu().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(st.color.cpu().numpy(), st2.color.cpu().numpy(), rtol=1e-4, atol=2e-5)
    assert same_bits(mo.batch.d_depth[:n], dd2) and same_bits(mo.batch.d_color[:n], dc2)
    a, b = log[0].cpu().numpy(), out2.cpu().numpy()
    assert a[3] == b[3]
    np.testing.assert_allclose(a[:3], b[:3], rtol=1e-4, atol=0)


def _track_scene(eng, S, handle_dynamic=True, seed=1):
    c2w, depth_img, color_img, pos, geo, col = mini_scene(seed)
    if not handle_dynamic:          # depth outliers (a moving object in front of the wall) that 10 x the median residual rejects
        hit = torch.rand(depth_img.shape, generator=torch.Generator().manual_seed(5)) < 0.04
        depth_img = torch.where(hit & (depth_img > 0), depth_img * 0.8, depth_img)
    W = syn.default_weights(seed=8)
    dec = core.DecoderBlob(eng).pack(W)
    pos_d, geo_d, col_d = eng.f32(pos), eng.f32(geo), eng.f32(col)
    knn = core.KnnIndex(eng, capacity=pos.shape[0])
    knn.build(pos_d)
    cam0 = H.c2w_to_cam(c2w) + torch.tensor([0.0, 0.002, -0.001, 0.0015, 0.004, -0.003, 0.002])
    return dict(depth=depth_img, color=color_img, pos=pos, geo=geo, col=col, W=W, dec=dec, dev=(pos_d, geo_d, col_d), knn=knn, cam0=cam0,
                cfg=core.RenderCfg(S=S, rel_pos=True))


TRACK_WIN = (2, HH - 2, 2, WW - 2)


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('handle_dynamic', (True, False))
@pytest.mark.parametrize('R', FORM_R)
@pytest.mark.parametrize('S', S_LOOP)
def test_tracker_two_pass_loss_matches_lk_loss_tracker(backend, S, R, handle_dynamic):
    """lk_track_frame's loss in two passes - pass 1 (residuals, per-tile sums) as the epilogue of the fused forward for S >= 4 (tiles of
    whole rays: test_form_ray_counts) or in k_track_composite at S = 3, pass 2 (mask, d depth / d colour, loss row) as the prologue of
    k_decode_bwd (lk_track_draw) - against lk_loss_tracker on the depth / variance / colour that one-iteration call left and on the batch it
    assembled: the masked-ray count exactly, the loss row at test_loss_forms.py's bound, both mask modes; pass 1's per-ray residuals and
    per-tile (sum, count) pairs - the 8-lane reduction of the epilogue, full at S = 4 - against the call's own render: counts exactly,
    sums at that file's bound.  (lk_track_draw hands d raw
    to the decoder backward and stores no d depth / d colour: the per-ray gradients of this form cannot be read back; the per-ray OUTPUTS
    of the fused forward are held to the oracle's render of the call's own rays at check_outputs' bounds.)  The work buffer is the test's:
    exactly lk_track_work_floats floats, the guard behind it intact - which shows a write past the END of the buffer only; the regions inside
    it are recomputed in track_work_layout (test_work_buffer_regions_add_up)."""
    eng = make_engine(backend)
    sc = _track_scene(eng, S, handle_dynamic)
    w_w = TRACK_WIN[3] - TRACK_WIN[2]
    rnd = torch.randint(0, (TRACK_WIN[1] - TRACK_WIN[0]) * w_w, (1, R), generator=torch.Generator().manual_seed(12 + R), dtype=torch.int32)
    to = steps.TrackOptimizer(eng, sc['cfg'], sc['dec'], sc['knn'], *sc['dev'], R, 0.002, separate_lr=True, w_color=0.5, handle_dynamic=handle_dynamic)
    need = int(eng.lib.dll.lk_track_work_floats(R, S, 1))
    wfull, to._work = guarded(eng, need, torch.float32, SENTINEL)
    best, log = to.track(eng.f32(sc['cam0']), eng.f32(sc['depth']), eng.f32(sc['color']), 1, TRACK_WIN, INTR, rnd.to(eng.device))
    _sync(eng)
    assert bool((wfull[need:] == SENTINEL).all()), 'lk_track_frame wrote behind lk_track_work_floats'
    # the call's own batch (work buffer of a one-iteration call: gt_depth [R] | gt_color [R][3] | ..., track_work_layout)
    lay, total = track_work_layout(R, S, 1)
    assert total == need
    o_gc = lay['gt_color'][0]
    gd, gc = to._work[:R].clone(), to._work[o_gc:o_gc + 3 * R].reshape(R, 3).clone()
    i, j = (TRACK_WIN[2] + rnd[0] % w_w).long(), (TRACK_WIN[0] + rnd[0] // w_w).long()
    ref_gd = sc['depth'][j, i]
    keep = ref_gd > 0
    keep = keep & (ref_gd <= H.inside_threshold(ref_gd[keep]))
    assert torch.equal(gd.cpu(), torch.where(keep, ref_gd, torch.zeros(()))) and 0 < int(keep.sum()) < R      # absent rays stay in place
    assert torch.equal(gc.cpu(), sc['color'][j, i])
    st = _St()
    st.depth, st.var, st.color = to.st.depth.clone(), to.st.var.clone(), to.st.color.clone()
    dd, dc, out, scr = eng.empty(R), eng.empty(R, 3), eng.empty(4), eng.empty(R + 8)
    optim.loss_tracker(eng, st, gd, gc, 0.5, True, dd, dc, out, scr, handle_dynamic=handle_dynamic)
    _sync(eng)
    assert float(dd.abs().sum()) > 0 and float(dc.abs().sum()) > 0
    check_sums(log[0], out)
    n_in = int(out[3])
    assert int((dc != 0).any(1).sum()) == n_in <= int(keep.sum())           # the rays inside the mask, one by one, are the count of both forms
    # pass 1 itself: the residual of every ray and the (sum, count) pair of every tile of whole rays (k_track_composite: of every 256 rays),
    # read where the call left them.  The loss row and the count above do not show them: the pairs only move the 10 x mean threshold, which
    # no ray of this scene is near, and the median's mask does not read them.
    n_pairs, per = fwd_pairs(R, S), (32 // S if S >= 4 else 256)
    o_lp, o_rs = lay['loss_part'][0], lay['resid'][0]
    part = to._work[o_lp:o_lp + 2 * n_pairs].cpu().reshape(n_pairs, 2)
    assert bool((to._work[o_lp + 2 * n_pairs:lay['pose_part'][0]] == SENTINEL).all()), 'more pairs written than the form has tiles'
    resid, gdc = to._work[o_rs:o_rs + R].cpu(), gd.cpu()
    present = gdc > 0
    adiff = (gdc - st.depth.cpu()).abs()
    tv = torch.where(present, adiff / torch.sqrt(st.var.cpu() + 1e-10), torch.zeros(()))           # Tracker.py:169-173 on the call's own render
    if handle_dynamic:
        # 10 x mean: the residual is the uncertainty-normalised one.  fp32 difference and sum are exact / correctly rounded on both sides; a
        # device square root and quotient that are not correctly rounded are within 1 ulp each, the product in the quotient half of one: 4 eps
        e = float(((resid - tv).abs() / tv.clamp_min(1e-30))[present].max())
        _record(f'track-form-S{S}-R{R}', resid_rel_max=e)
        assert e <= 4 * EPS32 and not bool(resid[~present].any()), e
        terms = resid
    else:
        # 10 x median of |gt - depth|: that residual bit for bit (-1: no reading); the pairs still hold the normalised sums, but pair 0's sum
        # is where k_track_median then leaves its threshold
        assert torch.equal(resid, torch.where(present, adiff, -torch.ones(())))
        assert float(part[0, 0]) > 0
        terms = tv
    for t in range(n_pairs):
        rays = slice(t * per, min((t + 1) * per, R))
        assert float(part[t, 1]) == float(present[rays].sum()), (t, 'rays with a reading in the tile')
        if handle_dynamic or t > 0:
            np.testing.assert_allclose(float(part[t, 0]), float(terms[rays].double().sum()), rtol=SUM_RTOL, atol=0, err_msg=f'residual sum of tile {t}')
    assert len({float(c) for c in part[:, 1]}) > 1 or n_pairs == 1           # (absent rays sit inside the tiles: the counts differ)
    # per-ray outputs of the fused forward: the oracle's render of the call's own rays
    pix_i, pix_j = i.float(), j.float()
    ro, rd = H.rays_from_uv(pix_i, pix_j, H.quat_to_c2w(sc['cam0']), *INTR)
    np.testing.assert_allclose(to.batch.rays_d.cpu().numpy(), rd.numpy(), rtol=2e-6, atol=1e-7)
    with torch.no_grad():
        o = H.render_batch(H.RenderCfg(S=S, rel_pos=True), to.batch.rays_o.cpu()[keep], to.batch.rays_d.cpu()[keep], ref_gd[keep], sc['pos'], sc['geo'], sc['col'],
                           sc['W'], 'color', tracker=True)
    kd = keep.to(eng.device)
    assert np.array_equal(to.st.valid_ray[kd].cpu().numpy().astype(bool), o['valid_ray'].numpy())
    np.testing.assert_allclose(to.st.depth[kd].cpu().numpy(), o['depth'].numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(to.st.color[kd].cpu().numpy(), o['color'].numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(to.st.var[kd].cpu().numpy(), o['var'].numpy(), rtol=2e-4, atol=1e-9)
    assert not bool(to.st.depth[~kd].any())                                  # absent rays render depth 0


# ---------------------------------------------------------------------------- C. the per-frame loops
LOOP_R, LOOP_ITERS = 96, 3
MAP_LRS = {'geometry': (0.001, 0.03, 0.0), 'color': (0.005, 0.005, 0.005)}
MAP_STAGES = ('geometry', 'color', 'color')
OPEN_SIGN_MAX = 0.1          # largest share of a decoder tensor's entries that may be of open sign (from the oracle alone: at most 7.1 % here)
_MAP_IN, _MAP_ORACLE, _MAP_RUN = {}, {}, {}


def _map_inputs():
    if not _MAP_IN:
        c2w, depth_img, color_img, pos, geo, col = mini_scene()
        W = syn.default_weights(seed=7)
        rnd_all = torch.randint(0, HH * WW, (LOOP_ITERS, LOOP_R), generator=torch.Generator().manual_seed(11), dtype=torch.int32)
        rows = torch.arange(0, pos.shape[0], 2, dtype=torch.int32)
        names = list(steps.GEO_DECODER_PARAMS) + list(steps.COLOR_DECODER_PARAMS)
        _MAP_IN.update(c2w=c2w, depth=depth_img, color=color_img, pos=pos, geo=geo, col=col, W=W, rnd=rnd_all, rows=rows, names=names)
    return _MAP_IN


def _oracle_map_loop(S, geo, col):
    """test_steps_parity.py::test_map_iterations_match_oracle's oracle loop (autograd + torch.optim.Adam over the oracle's render) at S
    samples per ray, from the feature tables given: (losses, masked-ray counts, stepped geo rows, stepped colour rows, stepped weights)."""
    m = _map_inputs()
    r = m['rows'].long()
    cfg = H.RenderCfg(S=S, rel_pos=True)
    Wt = {k: v.clone() for k, v in m['W'].items()}
    for n in m['names']:
        Wt[n].requires_grad_(True)
    geo_p, col_p = geo[r].clone().requires_grad_(True), col[r].clone().requires_grad_(True)
    opt = torch.optim.Adam([{'params': [Wt[n] for n in m['names']], 'lr': 0}, {'params': [geo_p], 'lr': 0}, {'params': [col_p], 'lr': 0}])
    losses, masked, open_sign = [], [], {}
    for it, stage in enumerate(MAP_STAGES):
        for gi in range(3):
            opt.param_groups[gi]['lr'] = MAP_LRS[stage][gi]
        opt.zero_grad()
        geo_t = geo.clone(); geo_t[r] = geo_p
        col_t = col.clone(); col_t[r] = col_p
        ro, rd, gd, gc, _, _ = oracle_rays(m['c2w'], m['depth'], m['color'], m['rnd'][it])
        keep = gd > 0
        keep = keep & (gd <= H.inside_threshold(gd[keep]))
        out = H.render_batch(cfg, ro[keep], rd[keep], gd[keep], m['pos'], geo_t, col_t, Wt, stage)
        loss, _, _, msk = H.mapper_loss(out['depth'], out['color'], out['valid_ray'], gd[keep], gc[keep], stage, 0.1)
        loss.backward()
        for n in m['names']:        # entries whose gradient is within the kernels' gradient bound of zero in an iteration: their sign is open
            gr = Wt[n].grad
            if gr is not None and float(gr.abs().max()) > 0:
                low = (gr != 0) & (gr.abs() <= P.TOL_GRAD * gr.abs().max())
                open_sign[n] = low if n not in open_sign else (open_sign[n] | low)
        opt.step()
        losses.append(loss.item())
        masked.append(int(msk.sum()))
    return losses, masked, geo_p.detach(), col_p.detach(), {n: Wt[n].detach() for n in m['names']}, open_sign


def _map_oracle(S):
    """The oracle loop and its YARDSTICK: the same loop from feature tables perturbed by 1e-7 relative - how far two fp32 evaluations of
    this call drift apart by themselves (docs/HISTORY.md round 5, test_loops_at_size.py)."""
    if S not in _MAP_ORACLE:
        m = _map_inputs()
        gp = torch.Generator().manual_seed(3)
        pert = lambda x: x * (1 + 1e-7 * torch.randn(x.shape, generator=gp))
        _MAP_ORACLE[S] = (_oracle_map_loop(S, m['geo'], m['col']), _oracle_map_loop(S, pert(m['geo']), pert(m['col'])))
    return _MAP_ORACLE[S]


def _map_run(backend, S, native):
    """The three iterations by the kernels, once per process: (loss log [3][4], geo table, colour table, weights).  The native call's work
    buffer is the test's (exactly lk_map_work_floats floats + guard: the end of the buffer only, see test_work_buffer_regions_add_up)."""
    key = (backend, S, native)
    if key not in _MAP_RUN:
        eng = make_engine(backend)
        m = _map_inputs()
        cfg = core.RenderCfg(S=S, rel_pos=True)
        dec = core.DecoderBlob(eng).pack(m['W'])
        pos_d, geo_d, col_d = eng.f32(m['pos']), eng.f32(m['geo']).clone(), eng.f32(m['col']).clone()
        knn = core.KnnIndex(eng, capacity=m['pos'].shape[0])
        knn.build(pos_d)
        mo = steps.MapOptimizer(eng, cfg, dec, knn, pos_d, geo_d, col_d, m['rows'].to(eng.device), LOOP_R, MAP_LRS, w_color=0.1)
        mo.begin_frame()
        frames = (eng.f32(m['depth']).reshape(1, HH, WW), eng.f32(m['color']).reshape(1, HH, WW, 3), eng.f32(m['c2w']).reshape(1, 4, 4), None)
        fid = torch.zeros(LOOP_R, dtype=torch.int32, device=eng.device)
        log = eng.zeros(LOOP_ITERS, 4)
        if native:
            assert mo._takes_native_loop()
            need = int(eng.lib.dll.lk_map_work_floats(LOOP_R, S, LOOP_ITERS))
            wfull, mo._work = guarded(eng, need, torch.float32, SENTINEL)
            mo.run(LOOP_ITERS, 1, frames, m['rnd'].to(eng.device), fid, (0, HH, 0, WW), INTR, HH, WW, log)
            _sync(eng)
            assert mo._work.numel() == need and bool((wfull[need:] == SENTINEL).all()), 'lk_map_frame wrote behind lk_map_work_floats'
        else:
            for it in range(LOOP_ITERS):
                mo.iterate(MAP_STAGES[it], frames, m['rnd'][it].to(eng.device), fid, (0, HH, 0, WW), INTR, HH, WW, log_row=log[it])
            _sync(eng)
        _MAP_RUN[key] = (log.cpu().numpy().astype(np.float64), geo_d.cpu().clone(), col_d.cpu().clone(), {k: v.clone() for k, v in dec.unpack().items()})
    return _MAP_RUN[key]


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('native', (True, False), ids=('native', 'statements'))
@pytest.mark.parametrize('S', S_LOOP)
def test_map_loop_matches_oracle(backend, S, native):
    """MapOptimizer.run (one lk_map_frame call) and the per-statement path, 96 rays, one 'geometry' and two 'color' iterations, rel-pos on,
    against the oracle loop at the same S: losses at rtol 2e-4, the masked-ray counts equal, rows outside the row list bit for bit where
    they were.  The stepped rows and weights are NOT held to test_steps_parity.py's fixed bounds (tuned to S = 5: Adam's first steps are
    sign-like, an entry whose gradient is rounding noise steps either way) but to the yardstick of test_loops_at_size.py::run_map_case,
    measured here from the oracle alone: 3 x the quantiles of the oracle loop re-run from tables perturbed by 1e-7 relative, with that
    function's floors (2 % / 10 % of one lr step x sqrt(iterations) at the 99 % / 99.9 % level: a random walk of the noise-level entries;
    Adam's hard limit of 2 lr per iteration for the worst entry; weights: 2e-4 of the tensor's scale + 0.15 (0.5 below 1 024 entries, where
    the 99.9 % level is the worst entry) of what the tensor moved).
    ENTRIES OF OPEN SIGN.  The issue's rule - EVERY stepped entry within 3 x the yardstick's quantiles - cannot be met by a correct kernel,
    and this test does not apply it to the entries named here; it is looser than the issue's wording by exactly them.  A perturbation of 1e-7 moves the oracle's gradients by fp32 rounding; the kernels' products run on split fp16 /
    bf16 pieces and are held to 1e-4 of a gradient tensor's largest entry (test_parity_at_size.TOL_GRAD; measured 8e-6).  A decoder entry
    whose oracle gradient is non-zero and within that bound of zero in any iteration may take either sign in a correct kernel, and Adam's step
    lr g / (|g| + 1e-8) then goes the other way by up to 2 lr - which the fp32 yardstick cannot show (its 99.9 % level is ~1e-6 where the
    kernels' was 0.0036 on color_decoder.pts_linears.4.weight at S = 4 and 6, 0.010 moved).  Those entries - found from the oracle's
    gradients alone, at most 7.1 % of a tensor here, capped at 10 % - are held to Adam's hard limit; all others to the yardstick rule
    above (measured on the emulator: 99.9 % level <= 9.4e-5, worst entry <= 3.3e-4)."""
    case = f'map-loop-S{S}-{"native" if native else "statements"}'
    m = _map_inputs()
    (o_losses, o_masked, geo_o, col_o, W_o, open_sign), (y_losses, _, geo_y, col_y, W_y, _) = _map_oracle(S)
    log, gk, ck, Wk = _map_run(backend, S, native)
    rel = np.abs(log[:, 0] - np.array(o_losses)) / np.abs(np.array(o_losses))
    yrel = np.abs(np.array(y_losses) - np.array(o_losses)) / np.abs(np.array(o_losses))
    _record(case, loss_rel=rel.tolist(), yard_loss_rel=yrel.tolist(), masked=o_masked)
    checks = []          # (every statistic is recorded before the first assertion)
    checks.append((bool((rel <= 2e-4).all()), ('losses', rel.tolist())))
    checks.append((log[:, 3].astype(int).tolist() == o_masked, ('masked-ray counts', log[:, 3].tolist(), o_masked)))
    r = m['rows'].long()
    other = torch.ones(m['pos'].shape[0], dtype=torch.bool)
    other[r] = False
    checks.append((torch.equal(bits(gk[other]), bits(m['geo'][other])) and torch.equal(bits(ck[other]), bits(m['col'][other])), 'rows outside the list untouched'))
    n_it = {'geo': LOOP_ITERS, 'col': LOOP_ITERS - 1}
    for name, mine, ref, yard, before, lr in (('geo', gk[r], geo_o, geo_y, m['geo'][r], 0.03), ('col', ck[r], col_o, col_y, m['col'][r], 0.005)):
        st, sy = param_error_stats(mine, ref, before), param_error_stats(yard, ref, before)
        _record(case, **{f'{name}_rows_{k}': v for k, v in st.items()}, **{f'{name}_rows_yard_{k}': v for k, v in sy.items()})
        n = n_it[name] ** 0.5
        checks.append((st['moved_max'] > 1e-3 and st['err_q99'] <= max(3.0 * sy['err_q99'], 0.02 * lr * n) and
                       st['err_q999'] <= max(3.0 * sy['err_q999'], 0.1 * lr * n) and st['err_max'] <= 2.0 * lr * n_it[name], (name + ' rows', st, sy)))
    worst, n_w = {}, 0
    for nm in m['names']:
        if nm not in Wk:
            continue
        mine = Wk[nm].reshape(W_o[nm].shape)
        free = open_sign.get(nm, torch.zeros_like(mine, dtype=torch.bool))
        held = ~free
        st, sy = param_error_stats(mine[held], W_o[nm][held], m['W'][nm][held]), param_error_stats(W_y[nm][held], W_o[nm][held], m['W'][nm][held])
        scale = max(1.0, float(m['W'][nm].abs().max()))
        e_free = float((mine[free] - W_o[nm][free]).abs().max()) if bool(free.any()) else 0.0
        worst[nm] = dict(err_q999=st['err_q999'], err_max=st['err_max'], yard_q999=sy['err_q999'], yard_max=sy['err_max'], moved_max=st['moved_max'],
                         open_sign_share=float(free.float().mean()), open_sign_err_max=e_free)
        q_floor = 0.15 if int(held.sum()) >= 1024 else 0.5
        checks.append((st['err_q999'] <= max(3.0 * sy['err_q999'], 2e-4 * scale + q_floor * st['moved_max']) and
                       st['err_max'] <= max(3.0 * sy['err_max'], 2e-4 * scale + 0.5 * st['moved_max']), (nm, st, sy)))
        checks.append((e_free <= 2.0 * sum(MAP_LRS[s][0] for s in MAP_STAGES) and float(free.float().mean()) <= OPEN_SIGN_MAX,
                       (nm, 'entries of open sign', e_free, float(free.float().mean()))))
        n_w += 1
    _record(case, decoder=worst)
    checks.append((n_w >= 28, 'every decoder tensor compared'))
    bad = [c[1] for c in checks if not c[0]]
    assert not bad, bad


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('S', S_LOOP)
def test_map_native_call_matches_the_statement_path(backend, S):
    """The native call against the per-statement path at the same S, at the bounds of
    test_steps_parity.py::test_long_map_call_matches_the_statement_path."""
    (la, geo_a, col_a, W_a), (lb, geo_b, col_b, W_b) = _map_run(backend, S, True), _map_run(backend, S, False)
    assert np.isfinite(la).all() and np.array_equal(la[:, 3], lb[:, 3])
    np.testing.assert_allclose(la[:, 0], lb[:, 0], rtol=2e-3)
    for name, a, b in (('geo', geo_a, geo_b), ('col', col_a, col_b)):
        err = (a - b).abs()
        _record(f'map-loop-S{S}-native-vs-statements', **{f'{name}_rows_q999': float(torch.quantile(err.reshape(-1), 0.999)), f'{name}_rows_max': float(err.max())})
        assert float(torch.quantile(err.reshape(-1), 0.999)) < 2e-4 and float(err.max()) < 0.02, float(err.max())
    for n, w in W_a.items():
        assert float((w - W_b[n]).abs().max()) <= 2e-3 * max(1.0, float(w.abs().max())), n


TRACK_R, TRACK_LR = 96, 0.002
_TRACK_ORACLE = {}


def _track_draws():
    w_w = TRACK_WIN[3] - TRACK_WIN[2]
    return torch.randint(0, (TRACK_WIN[1] - TRACK_WIN[0]) * w_w, (LOOP_ITERS, TRACK_R), generator=torch.Generator().manual_seed(12), dtype=torch.int32)


def _oracle_track_loop(S, sc, geo, col):
    """test_steps_parity.py::test_track_iterations_match_oracle's oracle loop (one leaf tensor: every candidate pose is a STEPPED pose) at S
    samples per ray: (losses, masked counts, candidate poses)."""
    rnd_all, w_w = _track_draws(), TRACK_WIN[3] - TRACK_WIN[2]
    cfg = H.RenderCfg(S=S, rel_pos=True)
    cam = sc['cam0'].clone().requires_grad_(True)
    opt = torch.optim.Adam([{'params': [cam], 'lr': TRACK_LR}])
    losses, masked, cams = [], [], []
    for it in range(LOOP_ITERS):
        opt.zero_grad()
        rr = rnd_all[it]
        i, j = (TRACK_WIN[2] + rr % w_w).float(), (TRACK_WIN[0] + rr // w_w).float()
        ro, rd = H.rays_from_uv(i, j, H.quat_to_c2w(cam), *INTR)
        flat = j.long() * WW + i.long()
        gd, gc = sc['depth'].reshape(-1)[flat], sc['color'].reshape(-1, 3)[flat]
        keep = gd > 0
        keep = keep & (gd <= H.inside_threshold(gd[keep]))
        out = H.render_batch(cfg, ro[keep], rd[keep], gd[keep], sc['pos'], geo, col, sc['W'], 'color', tracker=True)
        loss, _, _, m_o = H.tracker_loss(out['depth'], out['var'], out['color'], gd[keep], gc[keep], 0.5)
        loss.backward()
        opt.step()
        cams.append(cam.detach().clone())           # one leaf stepped in place: the candidate is the pose AFTER the update
        losses.append(loss.item())
        masked.append(int(m_o.sum()))
    return losses, masked, cams


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('native', (True, False), ids=('native', 'statements'))
@pytest.mark.parametrize('S', S_LOOP)
def test_track_loop_matches_oracle(backend, S, native):
    """TrackOptimizer.track - one lk_track_frame call (loss epilogue of the fused forward for S >= 4, k_track_composite at S = 3) or the
    per-statement path - 96 rays, three iterations, against the oracle loop at the same S at the bounds of
    test_steps_parity.py::test_track_iterations_match_oracle: losses (rtol 2e-4 here), the masked-ray counts equal, the chosen pose within
    2e-5.  The yardstick (the oracle loop from feature tables perturbed by 1e-7 relative) is recorded beside the measured values.  The native
    call's work buffer is the test's: exactly lk_track_work_floats floats, the guard behind it intact (the end of the buffer only: see
    test_work_buffer_regions_add_up)."""
    case = f'track-loop-S{S}-{"native" if native else "statements"}'
    eng = make_engine(backend)
    sc = _track_scene(eng, S)
    if S not in _TRACK_ORACLE:
        gp = torch.Generator().manual_seed(3)
        pert = lambda x: x * (1 + 1e-7 * torch.randn(x.shape, generator=gp))
        _TRACK_ORACLE[S] = (_oracle_track_loop(S, sc, sc['geo'], sc['col']), _oracle_track_loop(S, sc, pert(sc['geo']), pert(sc['col'])))
    (o_losses, o_masked, o_cams), (y_losses, _, y_cams) = _TRACK_ORACLE[S]
    to = steps.TrackOptimizer(eng, sc['cfg'], sc['dec'], sc['knn'], *sc['dev'], TRACK_R, TRACK_LR, separate_lr=False, w_color=0.5)
    to.native_loop = native
    if native:
        need = int(eng.lib.dll.lk_track_work_floats(TRACK_R, S, LOOP_ITERS))
        wfull, to._work = guarded(eng, need, torch.float32, SENTINEL)
    best, log = to.track(eng.f32(sc['cam0']), eng.f32(sc['depth']), eng.f32(sc['color']), LOOP_ITERS, TRACK_WIN, INTR, _track_draws().to(eng.device))
    _sync(eng)
    if native:
        assert to._work.numel() == need and bool((wfull[need:] == SENTINEL).all()), 'lk_track_frame wrote behind lk_track_work_floats'
    log = log.cpu().numpy().astype(np.float64)
    k = int(np.argmin(o_losses))
    rel = np.abs(log[:, 0] - np.array(o_losses)) / np.abs(np.array(o_losses))
    yrel = np.abs(np.array(y_losses) - np.array(o_losses)) / np.abs(np.array(o_losses))
    perr = float((best.cpu() - o_cams[k]).abs().max())
    yerr = float((y_cams[int(np.argmin(y_losses))] - o_cams[k]).abs().max())
    _record(case, loss_rel=rel.tolist(), yard_loss_rel=yrel.tolist(), pose_err=perr, yard_pose_err=yerr, masked=o_masked)
    assert bool((rel <= 2e-4).all()), rel.tolist()
    assert log[:, 3].astype(int).tolist() == o_masked
    assert perr <= 2e-5, (perr, yerr)
    assert float((o_cams[k] - sc['cam0']).abs().max()) > 0.5 * TRACK_LR         # (the chosen pose is a stepped one)


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('S', S_LOOP)
def test_track_native_call_matches_the_statement_path(backend, S):
    """lk_track_frame against the per-statement path at the same S, as test_size_switches.py::test_track_loop_forms_match_the_statement_path
    holds them: three stiff iterations (rate / 200: rounding is not amplified), losses within 5e-5 where both sides mask the same number
    of rays (stiff_call_ok), the chosen pose within 5 % of one step."""
    eng = make_engine(backend)
    sc = _track_scene(eng, S)
    lr = TRACK_LR / 200.0
    res = {}
    for native in (True, False):
        to = steps.TrackOptimizer(eng, sc['cfg'], sc['dec'], sc['knn'], *sc['dev'], TRACK_R, lr, separate_lr=True, w_color=0.5)
        to.native_loop = native
        best, log = to.track(eng.f32(sc['cam0']), eng.f32(sc['depth']), eng.f32(sc['color']), LOOP_ITERS, TRACK_WIN, INTR, _track_draws().to(eng.device))
        _sync(eng)
        res[native] = (best.cpu().double(), log.cpu().numpy().astype(np.float64))
    (best_a, la), (best_b, lb) = res[True], res[False]
    assert np.isfinite(la).all() and 0 < la[0, 3] <= TRACK_R
    rel = np.abs(la[:, 0] - lb[:, 0]) / np.abs(lb[:, 0])
    dm = np.abs(la[:, 3] - lb[:, 3])
    perr = float((H.quat_to_c2w(best_a) - H.quat_to_c2w(best_b)).abs().max())
    _record(f'track-loop-S{S}-native-vs-statements', loss_rel=rel.tolist(), masked_diff=dm.tolist(), pose_err=perr)
    assert stiff_call_ok(rel, dm, TRACK_R, 5e-5), (rel.tolist(), dm.tolist())
    assert perr <= 0.05 * lr * LOOP_ITERS + 1e-7, perr


# ---------------------------------------------------------------------------- D. the tile switch of the tracker's fused forward (chip only)
GLDS_MAX_TILES = sw.source_define('lk_decode.hip', 'LK_GLDS_MAX_TILES')
GLDS_NAMES = ('depth', 'var', 'color', 'valid_ray', 'z', 'nbr_idx', 'nbr_count', 'raw')


def glds_rays(S):
    """(R, R + 1): the largest batch whose whole-ray tiles are LK_GLDS_MAX_TILES - the geometry decoder's operands staged in LDS
    (k_relpos_decode_fwd<., ., true>) - and the first that takes the plain form, its last tile holding one ray."""
    R = GLDS_MAX_TILES * tile_stride(S) // S
    assert -(-R * S // tile_stride(S)) == GLDS_MAX_TILES and -(-(R + 1) * S // tile_stride(S)) == GLDS_MAX_TILES + 1
    return R, R + 1


@pytest.mark.gpu
@pytest.mark.parametrize('S', (4, 8))
def test_fused_forward_forms_agree_across_the_tile_switch(S):
    """One lk_track_frame iteration on the first R and the first R + 1 draws of one list (glds_rays: 2048 / 2049 rays at S = 4, 1024 / 1025
    at S = 8, from the define): the two forms of the fused forward are meant to differ in where the geometry decoder's operands come from
    only, so the R shared rays render the same bits in both batches - depth, variance, colour, validity, sample depths, neighbour lists
    and the decoders' raw outputs - and the batch the call assembled for them is the same.  (Frame 5 of the synthetic room with holes and
    40-m outliers, test_size_switches._loop_frame: absent rays sit inside the tiles.)  Chip only: 8 200 colour-stage samples take the
    emulator most of a minute per batch."""
    from test_size_switches import _render_scene, _loop_frame
    eng = make_engine('hip')
    sc = _render_scene(eng, 'hip')
    depth, color, c2w = _loop_frame()
    Hh, Ww = depth.shape
    intr = tuple(syn.TUM_INTR[k] for k in ('fx', 'fy', 'cx', 'cy'))
    win = (20, Hh - 20, 20, Ww - 20)
    R_lo, R_hi = glds_rays(S)
    rnd = torch.randint(0, (win[1] - win[0]) * (win[3] - win[2]), (1, R_hi), generator=torch.Generator().manual_seed(S), dtype=torch.int32)
    cam0 = eng.f32(H.c2w_to_cam(c2w) + torch.tensor([0.0, 0.002, -0.001, 0.0015, 0.004, -0.003, 0.002]))
    cfg = core.RenderCfg(S=S, rel_pos=True)
    dec = core.DecoderBlob(eng).pack(syn.default_weights(rel_pos=True))
    res = {}
    for R in (R_lo, R_hi):
        to = steps.TrackOptimizer(eng, cfg, dec, sc['knn'], sc['pos'], sc['geo'], sc['col'], R, 0.002, separate_lr=True, w_color=0.5)
        best, log = to.track(cam0, eng.f32(depth), eng.f32(color), 1, win, intr, rnd[:, :R].contiguous().to(eng.device))
        torch.cuda.synchronize()
        out = {k: getattr(to.st, k)[:R_lo * (S if getattr(to.st, k).shape[0] == R * S else 1)].clone() for k in GLDS_NAMES}
        out['gt_depth'] = to._work[:R_lo].clone()
        res[R] = (out, log.cpu().numpy())
    a, b = res[R_lo][0], res[R_hi][0]
    assert 0.5 < float(a['valid_ray'].float().mean()) < 1.0 and 0 < int((a['gt_depth'] == 0).sum()) < R_lo // 4
    assert np.isfinite(res[R_lo][1]).all() and np.isfinite(res[R_hi][1]).all() and res[R_lo][1][0, 3] > R_lo // 2
    for k in GLDS_NAMES + ('gt_depth',):
        assert torch.equal(bits(a[k]), bits(b[k])), f'{k} of the shared rays differs between {R_lo} and {R_hi} rays'


# ---------------------------------------------------------------------------- E. ABI edges
@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('S', (0, sw.S_MAX + 1))
def test_bad_sample_counts_are_refused(backend, S):
    """S = 0 and S = LK_S_MAX + 1 through lk_render_fwd, lk_track_frame, lk_map_prepare and lk_map_frame: LK_ERR_ARG with a message, before anything is
    launched - the outputs, the work buffers and the parameters keep their bits.  (The two loops assemble their batches ahead of the render's
    own check of its descriptor, so they check S themselves.)"""
    eng = make_engine(backend)
    bad = core.RenderCfg(S=S, rel_pos=True)
    R, S_ok = 16, sw.S
    sc = _track_scene(eng, S_ok)
    pos_d, geo_d, col_d = sc['dev']

    def painted(st):
        for k in ('depth', 'var', 'color', 'z', 'raw', 'nbr_w'):
            getattr(st, k).fill_(SENTINEL)
        return st

    def untouched(st):
        return all(bool((getattr(st, k) == SENTINEL).all()) for k in ('depth', 'var', 'color', 'z', 'raw', 'nbr_w'))
    # lk_render_fwd
    st = painted(core.RenderState(eng, R, S_ok))
    ro, rd, gd = eng.f32(torch.zeros(R, 3)), eng.f32(torch.ones(R, 3)), eng.f32(torch.ones(R))
    d = core.fill_desc(eng, bad, st, ro, rd, gd, sc['knn'], pos_d, geo_d, col_d, sc['dec'], 'color')
    rc = eng.lib.dll.lk_render_fwd(_ffi.C.byref(d), eng.stream)
    assert rc == -1                                                     # LK_ERR_ARG
    with pytest.raises(_ffi.LoopyError, match=r'lk_render_fwd.*bad R/S'):
        eng.lib.check(rc, 'lk_render_fwd')
    _sync(eng)
    assert untouched(st)
    # lk_track_frame
    to = steps.TrackOptimizer(eng, sc['cfg'], sc['dec'], sc['knn'], pos_d, geo_d, col_d, R, 0.002, separate_lr=True, w_color=0.5)
    to.cfg = bad
    painted(to.st)
    to.batch.rays_o.fill_(SENTINEL); to.batch.d_depth.fill_(SENTINEL)
    to._work = torch.full((int(eng.lib.dll.lk_track_work_floats(R, max(S, sw.S_MAX), 2)) + 64,), SENTINEL, device=eng.device)
    w_w = TRACK_WIN[3] - TRACK_WIN[2]
    rnd = torch.randint(0, (TRACK_WIN[1] - TRACK_WIN[0]) * w_w, (2, R), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(eng.device)
    with pytest.raises(_ffi.LoopyError, match=r'lk_track_frame.*rc=-1.*bad S'):
        to.track(eng.f32(sc['cam0']), eng.f32(sc['depth']), eng.f32(sc['color']), 2, TRACK_WIN, INTR, rnd)
    _sync(eng)
    assert untouched(to.st) and bool((to._work == SENTINEL).all()) and bool((to.batch.rays_o == SENTINEL).all()) and bool((to.batch.d_depth == SENTINEL).all())
    # lk_map_frame
    geo_m, col_m = geo_d.clone(), col_d.clone()
    blob0 = sc['dec'].blob.clone()
    rows = torch.arange(0, pos_d.shape[0], 2, dtype=torch.int32).to(eng.device)
    mo = steps.MapOptimizer(eng, sc['cfg'], sc['dec'], sc['knn'], pos_d, geo_m, col_m, rows, R, MAP_LRS, w_color=0.1)
    mo.begin_frame()
    mo.cfg = bad
    painted(mo.st)
    mo._work = torch.full((int(eng.lib.dll.lk_map_work_floats(R, max(S, sw.S_MAX), 2)) + 64,), SENTINEL, device=eng.device)
    frames = (eng.f32(sc['depth']).reshape(1, HH, WW), eng.f32(sc['color']).reshape(1, HH, WW, 3), torch.eye(4, device=eng.device).reshape(1, 4, 4).contiguous(), None)
    log = torch.full((2, 4), SENTINEL, device=eng.device)
    with pytest.raises(_ffi.LoopyError, match=r'lk_map_prepare.*rc=-1.*bad S'):          # (the batch assembly alone, ahead of the row list)
        mo.prepare(2, 1, frames, rnd, torch.zeros(R, dtype=torch.int32, device=eng.device), (0, HH, 0, WW), INTR, HH, WW, log)
    _sync(eng)
    assert untouched(mo.st) and bool((mo._work == SENTINEL).all()) and bool((log == SENTINEL).all())
    with pytest.raises(_ffi.LoopyError, match=r'lk_map_frame.*rc=-1.*bad R/S'):
        mo.run(2, 1, frames, rnd, torch.zeros(R, dtype=torch.int32, device=eng.device), (0, HH, 0, WW), INTR, HH, WW, log)
    _sync(eng)
    assert untouched(mo.st) and bool((mo._work == SENTINEL).all()) and bool((log == SENTINEL).all())
    assert torch.equal(bits(geo_m), bits(geo_d)) and torch.equal(bits(col_m), bits(col_d)) and torch.equal(bits(sc['dec'].blob), bits(blob0))
