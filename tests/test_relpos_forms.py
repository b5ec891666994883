"""One definition of the rel-pos neighbour MLP's wave tile (csrc/lk_relpos_dev.h): the three kernel bodies that share it - relpos_fwd_wave,
relpos_bwd_wave, relpos_bwd_wave_fused - and their template instantiations are pinned to EACH OTHER, bit for bit, on a batch with every
special row in it (samples below min_nn, partly filled neighbour lists, padded slots inside kept samples) and with a tail in every tile
size: the first 95 of the replica golden's 96 rays, S = 5, P = 475 = 118 x 4 + 3 (the plain kernels' 4-sample waves) = 29 x 16 + 11 (the
fused kernel's 16-sample tiles).

  1. Half feature tables are a storage format in every form: fp32 tables that hold the half-rounded values and the half tables themselves
     (LK_FLAG_FEATS_F16: the F16 instantiations) give the same bits - c_col, colour, depth, both feature gradients, the weight gradients.
  2. k_relpos_bwd_fused<WG = false> (LK_FLAG_EMBED_GRADS_ONLY) is "the same d x / d feature / d B arithmetic" as <WG = true>: the same
     feature gradients, bit for bit.

Both held before the bodies shared a definition (host emulator and MI355X): the test pins the forms, not a refactoring."""
import numpy as np
import pytest
import torch

from loopy_slam_amd import core, _ffi
from util import load, tens, weights, make_engine, backends
from test_forward_parity import rcfg

torch.set_num_threads(1)
R_USED = 95
UNIT, EMBED = _ffi.FLAG_UNIT_LOSS_GRADS, _ffi.FLAG_EMBED_GRADS_ONLY
#            label: (weight gradients, extra flags)                        kernel
CONFIGS = {'feats': (False, 0),                                          # k_relpos_bwd, no weight rows
           'plain-w': (True, 0),                                         # k_relpos_bwd with rows for k_wgrad
           'fused': (True, UNIT),                                        # k_relpos_bwd_fused<true, .>
           'fused-E': (True, UNIT | EMBED)}                              # k_relpos_bwd_fused<false, .>
_RUNS = {}


def run(backend, label, half):
    """One forward + backward of the batch; cached per (backend, label, half) - every test reads, none writes."""
    key = (backend, label, half)
    if key in _RUNS:
        return _RUNS[key]
    eng = make_engine(backend)
    g = load('g6_render_replica_map_color')
    cfg = rcfg('replica')
    assert cfg.S == 5 and cfg.rel_pos
    dec = core.DecoderBlob(eng).pack(weights('replica'))
    ro, rd, gd, pos, geo, col = tens(g, 'rays_o', 'rays_d', 'gt_depth', 'pos', 'geo', 'col')
    ro, rd, gd = ro[:R_USED], rd[:R_USED], gd[:R_USED]
    geo_h, col_h = geo.half(), col.half()
    geo_t, col_t = (geo_h, col_h) if half else (geo_h.float(), col_h.float())
    pos_d = eng.f32(pos)
    knn = core.KnnIndex(eng, capacity=pos.shape[0])
    knn.build(pos_d)
    st = core.RenderState(eng, R_USED, cfg.S, need_act=True)
    want_w, flags = CONFIGS[label]
    core.render_forward(eng, cfg, st, eng.f32(ro), eng.f32(rd), eng.f32(gd), knn, pos_d, geo_t.to(eng.device).contiguous(),
                        col_t.to(eng.device).contiguous(), dec, 'color', noise_geo=eng.f32(g['noise_geo']), noise_col=eng.f32(g['noise_col']),
                        save_act=True, extra_flags=flags)
    assert bool(st.desc.flags & _ffi.FLAG_FEATS_F16) == half
    gen = torch.Generator().manual_seed(95)                               # unit-scale loss gradients, as the mapper's: +-1, +-w_color
    d_depth = (torch.randint(0, 2, (R_USED,), generator=gen) * 2 - 1).float()
    d_color = 0.1 * (torch.randint(0, 2, (R_USED, 3), generator=gen) * 2 - 1).float()
    gs = core.GradState(eng, pos.shape[0], R_USED, dec.n, feats=True, weights=want_w)
    core.render_backward(eng, st, gs, eng.f32(d_depth), eng.f32(d_color))
    out = dict(c_col=st.c_col, color=st.color, depth=st.depth, g_geo=gs.g_geo, g_col=gs.g_col, g_weights=gs.g_weights)
    out = {k: (v.detach().cpu().numpy().copy() if v is not None else None) for k, v in out.items()}
    out['nbr_count'] = st.nbr_count.cpu().numpy().reshape(-1).copy()
    out['nbr_idx'] = st.nbr_idx.cpu().numpy().reshape(-1, 8).copy()
    out['min_nn'] = cfg.min_nn
    out['gW'] = {k: v.cpu().numpy().copy() for k, v in dec.unpack(gs.g_weights).items()} if want_w else None
    _RUNS[key] = out
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('backend', backends())
def test_batch_has_every_special_row(backend):
    """The batch must keep exercising what the tile conventions are about, or the comparisons below pin nothing."""
    o = run(backend, 'feats', False)
    cnt, idx, min_nn = o['nbr_count'], o['nbr_idx'], o['min_nn']
    assert cnt.shape[0] == R_USED * 5 == 475
    kept = cnt >= min_nn
    below = int((~kept).sum())
    partly = int((kept & (idx < 0).any(axis=1)).sum())
    padded = int((idx[kept] < 0).sum())
    print('samples below min_nn', below, 'partly filled lists', partly, 'padded slots inside kept samples', padded)
    assert below > 0 and partly > 0 and padded > 0
    assert float(np.abs(o['g_col']).sum()) > 0 and float(np.abs(o['g_geo']).sum()) > 0


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('label', list(CONFIGS))
def test_half_tables_are_a_storage_format(backend, label):
    a, b = run(backend, label, False), run(backend, label, True)
    for k in ('c_col', 'color', 'depth', 'g_geo', 'g_col'):
        assert same_bits(a[k], b[k]), k
    if a['gW'] is not None:
        assert float(np.abs(a['gW']['color_decoder.embedder_rel_pos._B']).sum()) > 0
        if not (label == 'fused-E'):
            assert float(np.abs(a['gW']['color_decoder.mlp_col_neighbor.linear1.weight']).sum()) > 0
        for name in a['gW']:
            assert same_bits(a['gW'][name], b['gW'][name]), name
        assert same_bits(a['g_weights'], b['g_weights'])


@pytest.mark.parametrize('backend', backends())
@pytest.mark.parametrize('half', (False, True))
def test_embed_grads_only_is_the_same_arithmetic(backend, half):
    a, b = run(backend, 'fused', half), run(backend, 'fused-E', half)
    assert same_bits(a['g_col'], b['g_col']) and same_bits(a['g_geo'], b['g_geo'])
    assert float(np.abs(a['g_col']).sum()) > 0
    # the frozen matrices get nothing, the Fourier matrix gets the same partial sums
    assert float(np.abs(b['gW']['color_decoder.mlp_col_neighbor.linear1.weight']).sum()) == 0.0
