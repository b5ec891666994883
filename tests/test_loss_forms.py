"""One definition of the loss arithmetic (csrc/lk_loss_dev.h): every kernel form of a loss gives the SAME per-ray gradients, bit for bit, and
the same count of masked rays on the same batch - the one-workgroup form (R <= 16 384), the many-workgroup form (the same rays padded with
absent rays to R = 16 385, the smallest batch that takes it) and, for the mapper, the forms inside k_composite and inside k_decode_bwd (their
own depth / colour / valid_ray outputs fed back into lk_loss_mapper).  The forms add their three loss sums in different orders: those agree to relative 2e-5,
the bound test_optim_parity.py::test_losses_large_batch uses for these kernels against the oracle."""
import numpy as np
import pytest
import torch

from loopy_slam_amd import core, optim, synthetic as syn
from test_steps_parity import mini_scene, oracle_rays, HH, WW
from util import make_engine, backends

torch.set_num_threads(1)
R1, RN = 777, 16385
SUM_RTOL = 2e-5


class _St:
    pass


def _state(eng, depth, var, color, valid):
    st = _St()
    st.depth, st.var, st.color = eng.f32(depth), eng.f32(var), eng.f32(color)
    st.valid_ray = valid.to(torch.uint8).to(eng.device).contiguous()
    return st


_BATCH = {}


def batch():
    """R1 rays with everything the masks treat specially: absent rays (gt_depth 0), invalid rays, a NaN depth, depth == gt exactly (sgn 0),
    and a present ray whose normalised residual is above the tracker's clamp at 1e3 (tiny variance)."""
    if not _BATCH:
        gen = torch.Generator().manual_seed(31)
        gd = torch.rand(R1, generator=gen) * 3 + 0.5
        gd[torch.rand(R1, generator=gen) < 0.06] = 0.0
        depth = gd + 0.03 * torch.randn(R1, generator=gen)
        depth[11] = float('nan')
        depth[12] = gd[12]
        var = torch.rand(R1, generator=gen) * 0.01 + 1e-4
        gd[13], depth[13], var[13] = 2.0, 2.01, 1e-12           # 0.01 / sqrt(1e-12 + 1e-10) = 995 ... and the next one 1990
        gd[14], depth[14], var[14] = 2.0, 1.98, 1e-12
        color, gc = torch.rand(R1, 3, generator=gen), torch.rand(R1, 3, generator=gen)
        color[15] = gc[15]
        valid = torch.rand(R1, generator=gen) < 0.9
        _BATCH.update(gd=gd, depth=depth, var=var, color=color, gc=gc, valid=valid)
    return _BATCH


def padded(x, fill=0.0):
    out = torch.full((RN,) + tuple(x.shape[1:]), fill, dtype=x.dtype)
    out[:R1] = x
    return out


def same_bits(a, b):
    return np.array_equal(a.cpu().numpy().view(np.uint32 if a.dtype == torch.float32 else np.uint8),
                          b.cpu().numpy().view(np.uint32 if b.dtype == torch.float32 else np.uint8))


def check_sums(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    print('loss rows', a, b)
    assert a[3] == b[3]                                                                 # the masked-ray count is exact
    assert a[3] > 0
    np.testing.assert_allclose(a[:3], b[:3], rtol=SUM_RTOL, atol=0)


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('use_color', (True, False))
def test_mapper_one_and_many_workgroups(backend, use_color):
    eng = make_engine(backend)
    b = batch()
    res = []
    for pad in (False, True):
        p = padded if pad else (lambda x, fill=0.0: x)
        R = RN if pad else R1
        # the padding rays are absent (gt_depth 0) whatever else they hold: NaN depths, valid
        st = _state(eng, p(b['depth'], float('nan')), p(b['var']), p(b['color'], 0.5), p(b['valid'], True))
        dd, dc, out = eng.empty(R), eng.empty(R, 3), eng.empty(4)
        optim.loss_mapper(eng, st, eng.f32(p(b['gd'])), eng.f32(p(b['gc'])), 0.1, use_color, dd, dc, out)
        res.append((dd, dc, out))
    (dd1, dc1, out1), (ddn, dcn, outn) = res
    assert same_bits(dd1, ddn[:R1]) and same_bits(dc1, dcn[:R1])
    assert float(ddn[R1:].abs().max()) == 0.0 and float(dcn[R1:].abs().max()) == 0.0
    assert float(dd1.abs().sum()) > 0 and (float(dc1.abs().sum()) > 0) == use_color
    check_sums(out1, outn)


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('handle_dynamic', (True, False))
def test_tracker_one_and_many_workgroups(backend, handle_dynamic):
    """Both mask modes: 10 x the batch mean of the normalised residual, and (handle_dynamic False) 10 x the median of |gt - depth|.  The
    padding rays are absent, so they enter neither the mean nor the median.  The NaN depth of the batch is left out: a NaN residual empties
    the mask of either mode (test_optim_parity.py::test_loss_tracker_median_mask pins that), and an empty mask compares nothing."""
    eng = make_engine(backend)
    b = batch()
    depth = torch.nan_to_num(b['depth'], nan=1.0)
    res = []
    for pad in (False, True):
        p = padded if pad else (lambda x, fill=0.0: x)
        R = RN if pad else R1
        st = _state(eng, p(depth, float('nan')), p(b['var'], float('nan')), p(b['color'], 0.5), torch.ones(R, dtype=torch.bool))
        dd, dc, out, scr = eng.empty(R), eng.empty(R, 3), eng.empty(4), eng.empty(R + 8)
        optim.loss_tracker(eng, st, eng.f32(p(b['gd'])), eng.f32(p(b['gc'])), 0.5, True, dd, dc, out, scr, handle_dynamic=handle_dynamic)
        res.append((dd, dc, out))
    (dd1, dc1, out1), (ddn, dcn, outn) = res
    assert same_bits(dd1, ddn[:R1]) and same_bits(dc1, dcn[:R1])
    assert float(ddn[R1:].abs().max()) == 0.0 and float(dcn[R1:].abs().max()) == 0.0
    assert float(dd1.abs().sum()) > 0 and float(dc1.abs().sum()) > 0
    if not handle_dynamic:          # ray 14 is inside the median mask with a residual above the clamp: its term is 1e3 and its d depth 0
        assert float(dd1[14]) == 0.0 and float(dc1[14].abs().sum()) > 0 and float(dd1[13]) != 0.0
    check_sums(out1, outn)


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('stage', ('geometry', 'color'))
def test_mapper_inside_the_composite(backend, stage):
    """k_composite with the mapper loss riding along (lk_render_fwd with LK_FLAG_MAPPER_LOSS) against lk_loss_mapper on k_composite's own
    outputs: a miniature scene with holes in the depth image (absent rays) and a reading far behind the points (an invalid ray)."""
    eng = make_engine(backend)
    c2w, depth_img, color_img, pos, geo, col = mini_scene()
    R = 300
    rnd = torch.randint(0, HH * WW, (R,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    rnd[:4] = torch.tensor([0, 5, 17, 34], dtype=torch.int32)                # two holes and the outlier pixel are in the batch
    ro, rd, gd, gc, _, _ = oracle_rays(c2w, depth_img, color_img, rnd)
    cfg = core.RenderCfg(rel_pos=True)
    dec = core.DecoderBlob(eng).pack(syn.default_weights(seed=7))
    pos_d, geo_d, col_d = eng.f32(pos), eng.f32(geo), eng.f32(col)
    knn = core.KnnIndex(eng, capacity=pos.shape[0])
    knn.build(pos_d)
    st = core.RenderState(eng, R, cfg.S)
    gd_d, gc_d = eng.f32(gd), eng.f32(gc)
    dd_c, dc_c, out_c = eng.empty(R), eng.empty(R, 3), eng.zeros(4)
    core.render_forward(eng, cfg, st, eng.f32(ro), eng.f32(rd), gd_d, knn, pos_d, geo_d, col_d, dec, stage, mapper_loss=(gc_d, 0.1, dd_c, dc_c, out_c))
    dd, dc, out = eng.empty(R), eng.empty(R, 3), eng.empty(4)
    optim.loss_mapper(eng, st, gd_d, gc_d, 0.1, stage == 'color', dd, dc, out)
    valid = st.valid_ray.cpu().bool()
    assert int((gd == 0).sum()) >= 2 and 0 < int((~valid & (gd > 0)).sum()) and int(valid.sum()) > R // 2
    assert same_bits(dd_c, dd) and same_bits(dc_c, dc)
    assert float(dd.abs().sum()) > 0 and (float(dc.abs().sum()) > 0) == (stage == 'color')
    check_sums(out_c, out)


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('stage', ('geometry', 'color'))
def test_mapper_inside_the_decoder_backward(backend, stage):
    """lk_map_draw (lk_composite_dev.h), the prologue of k_decode_bwd inside lk_map_frame, spells the mapper's loss out instead of calling
    lk_map_ray_loss (why: see its comment) - so it is pinned here: one native one-iteration call, then lk_loss_mapper on the depth / colour /
    valid_ray that call left, against the d depth / d colour and the loss row it left.  The call assembles its batch itself (rays that keep
    a reading first); the rays behind them are not processed and not compared."""
    from loopy_slam_amd import steps
    from test_steps_parity import INTR
    eng = make_engine(backend)
    c2w, depth_img, color_img, pos, geo, col = mini_scene()
    R = 96
    rnd = torch.randint(0, HH * WW, (1, R), generator=torch.Generator().manual_seed(11), dtype=torch.int32)
    rnd[0, :4] = torch.tensor([0, 5, 17, 34], dtype=torch.int32)
    cfg = core.RenderCfg(rel_pos=True)
    dec = core.DecoderBlob(eng).pack(syn.default_weights(seed=7))
    pos_d, geo_d, col_d = eng.f32(pos), eng.f32(geo).clone(), eng.f32(col).clone()
    knn = core.KnnIndex(eng, capacity=pos.shape[0])
    knn.build(pos_d)
    rows = torch.arange(0, pos.shape[0], 2, dtype=torch.int32)
    lrs = {'geometry': (0.001, 0.03, 0.0), 'color': (0.005, 0.005, 0.005)}
    mo = steps.MapOptimizer(eng, cfg, dec, knn, pos_d, geo_d, col_d, rows.to(eng.device), R, lrs, w_color=0.1)
    mo.begin_frame()
    frames = (eng.f32(depth_img).reshape(1, HH, WW), eng.f32(color_img).reshape(1, HH, WW, 3), eng.f32(c2w).reshape(1, 4, 4), None)
    log = eng.zeros(1, 4)
    mo.run(1, 1 if stage == 'geometry' else 0, frames, rnd.to(eng.device), torch.zeros(R, dtype=torch.int32, device=eng.device), (0, HH, 0, WW), INTR, HH, WW, log)
    # the call's own batch (work buffer of a one-iteration call: rays_o [R][3] | rays_d [R][3] | gt_depth [R] | gt_color [R][3] | ...)
    gd = mo._work[6 * R:7 * R].clone()
    gc = mo._work[7 * R:10 * R].reshape(R, 3).clone()
    ref_gd = depth_img.reshape(-1)[rnd[0].long()]
    n_live = int((gd > 0).sum())
    assert n_live == int(((ref_gd > 0) & (ref_gd < 10)).sum()) and 0 < n_live < R and bool((gd[:n_live] > 0).all())
    assert sorted(gd[:n_live].cpu().tolist()) == sorted(ref_gd[(ref_gd > 0) & (ref_gd < 10)].tolist())
    st = _St()
    st.depth, st.color, st.valid_ray = mo.st.depth[:n_live].clone(), mo.st.color[:n_live].clone(), mo.st.valid_ray[:n_live].clone()
    dd, dc, out = eng.empty(n_live), eng.empty(n_live, 3), eng.empty(4)
    optim.loss_mapper(eng, st, gd[:n_live].clone(), gc[:n_live].clone(), 0.1, stage == 'color', dd, dc, out)
    assert same_bits(mo.batch.d_depth[:n_live], dd) and same_bits(mo.batch.d_color[:n_live], dc)
    assert float(dd.abs().sum()) > 0 and (float(dc.abs().sum()) > 0) == (stage == 'color')
    check_sums(log[0], out)
