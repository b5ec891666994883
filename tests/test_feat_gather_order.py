"""The feature-row gradients are fixed-order sums: k_feat_gather adds the rows of a point one by one in the order of the sorted list
(point, then row index), each sum from 0.0f with one rounded add per row, and flushes it once.  These tests rebuild the list and the sums
on the host from what the backward left in its scratch and ask for EQUAL bits - on a scene small enough for the emulator that still holds
every case of the walk: a run over more than two 32-entry windows, a run of one row, a run that starts in the last slot of a 16-row chunk
and goes on, a chunk inside one run, and a list whose length is no multiple of 4, 16 or 32."""
import numpy as np
import pytest
import torch

from loopy_slam_amd import core, workload, synthetic as syn
from util import make_engine, backends

CAM = dict(fx=50.0, fy=50.0, cx=31.5, cy=23.5, W=64, H=48)
DEPTH = 2.0
CHUNK = 16          # LK_GATHER_CHUNK: list entries per half-wave


def _rays(i, j):
    d = torch.stack([(i - CAM['cx']) / CAM['fx'], -(j - CAM['cy']) / CAM['fy'], -torch.ones_like(i)], dim=1)
    return torch.zeros_like(d), d.contiguous()


def _scene(seed=0):
    """A hot cluster of 24 points (a 4 x 2 pixel patch at 0.98 / 1.0 / 1.02 x depth) with 36 rays through it, 300 background points with
    28 rays spread over the image, three rays without a depth reading, and a row mask that drops every ninth point."""
    g = torch.Generator().manual_seed(seed)
    pi, pj = torch.meshgrid(torch.arange(4.0) + 30.0, torch.arange(2.0) + 22.0, indexing='ij')
    bi, bj = torch.rand(100, generator=g) * 63.0, torch.rand(100, generator=g) * 47.0
    far = (bi - 31.0).abs() > 6.0                                  # background pixels keep clear of the patch
    bi, bj = bi[far], bj[far]
    si, sj = torch.cat([pi.reshape(-1), bi]), torch.cat([pj.reshape(-1), bj])
    _, sd = _rays(si, sj)
    pos = torch.cat([sd * (DEPTH * f) for f in (0.98, 1.0, 1.02)]).contiguous()
    N = pos.shape[0]
    geo, col = 0.3 * torch.randn(N, 32, generator=g), 0.3 * torch.randn(N, 32, generator=g)
    ri = torch.cat([30.0 + 3.0 * torch.rand(36, generator=g), bi[:28] + torch.rand(28, generator=g) - 0.5])
    rj = torch.cat([22.0 + torch.rand(36, generator=g), bj[:28] + torch.rand(28, generator=g) - 0.5])
    ro, rd = _rays(ri, rj)
    gd = torch.full((64,), DEPTH)
    gd[[5, 40, 63]] = 0.0                                          # holes of the depth image
    mask = torch.ones(N, dtype=torch.uint8)
    mask[::9] = 0
    d_depth, d_color = torch.randn(64, generator=g), torch.randn(64, 3, generator=g)
    return dict(pos=pos, geo=geo, col=col, ro=ro, rd=rd, gd=gd, mask=mask, d_depth=d_depth, d_color=d_color)


def _al(x):
    return (x + 3) // 4 * 4


def _cdiv(a, b):
    return (a + b - 1) // b


def _offsets(P, color, rel_pos):
    """lk_api.hip::bwd_layout for a backward with feature gradients and no weight gradients (floats)."""
    o = {}
    o['dc_geo'] = _al(4 * P)
    o['dc_col'] = o['dc_geo'] + _al(32 * P)
    at = o['dc_col'] + _al(32 * P) + 4 * _al(4 * P) + 2 * _al(8 * P) + _al(4 * P)          # dp_embed .. dlogit
    at += _al(_cdiv(P, 32) * 12) + _al(_cdiv(_cdiv(P, 32), 4) * 288) + _al(_cdiv(_cdiv(P, 4), 4) * 32)      # aff_part, part_bg, part_br
    o['dfeat'] = at
    if color and rel_pos:
        at += _al(8 * 32 * P)
    at += _al(P)                                                   # w_sum
    o['seg_rank'] = at
    o['seg_list'] = at + _al(8 * P)
    return o


def _run(backend, rel_pos=True, stage='color', R=64, mask_zero=False, f16=False):
    eng = make_engine(backend)
    sc = _scene()
    dev = eng.device
    pos, geo, col, ro, rd, gd = (sc[k].to(dev) for k in ('pos', 'geo', 'col', 'ro', 'rd', 'gd'))
    ro, rd, gd = ro[:R].contiguous(), rd[:R].contiguous(), gd[:R].contiguous()
    if f16:
        geo, col = geo.half(), col.half()
    cfg = core.RenderCfg(rel_pos=rel_pos)
    blob = core.DecoderBlob(eng).pack(syn.default_weights(rel_pos=rel_pos))
    knn = core.KnnIndex(eng, capacity=pos.shape[0])
    knn.build(pos)
    st = core.RenderState(eng, R, cfg.S, need_act=True)
    core.render_forward(eng, cfg, st, ro, rd, gd, knn, pos, geo, col, blob, stage, save_act=True)
    gs = core.GradState(eng, pos.shape[0], R, blob.n, feats=True, weights=False)
    gs.row_mask = (torch.zeros_like(sc['mask']) if mask_zero else sc['mask']).to(dev)
    core.render_backward(eng, st, gs, sc['d_depth'][:R].contiguous().to(dev), sc['d_color'][:R].contiguous().to(dev))
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    P = R * cfg.S
    color = stage == 'color'
    off = _offsets(P, color, rel_pos)
    scr = gs.scratch.cpu()
    idx, w, cnt = st.nbr_idx.cpu().reshape(-1).numpy(), st.nbr_w.cpu().reshape(-1).numpy(), st.nbr_count.cpu().numpy()
    mask = gs.row_mask.cpu().numpy()
    # the rows that take part, in the order of the list: by point, then by row
    live = (idx >= 0) & (w != 0) & (np.repeat(cnt, 8) >= cfg.min_nn)
    live[live] &= mask[idx[live]] != 0
    rows = np.nonzero(live)[0]
    rows = rows[np.lexsort((rows, idx[rows]))]
    total = rows.size
    seg_list = scr[off['seg_list']:off['seg_list'] + 8 * P].view(torch.int32).numpy()[:total]
    assert np.array_equal(seg_list, rows)
    # the sequential sums: rank by rank over the points, one rounded product and one rounded add per row
    dc_geo = scr[off['dc_geo']:off['dc_geo'] + 32 * P].reshape(P, 32).numpy()
    pts, first, runlen = np.unique(idx[rows], return_index=True, return_counts=True)
    want_geo = np.zeros((pos.shape[0], 32), np.float32)
    want_col = np.zeros((pos.shape[0], 32), np.float32)
    if color and rel_pos:
        dfeat = scr[off['dfeat']:off['dfeat'] + 256 * P].reshape(8 * P, 32).numpy()
    elif color:
        dc_col = scr[off['dc_col']:off['dc_col'] + 32 * P].reshape(P, 32).numpy()
    for k in range(int(runlen.max()) if total else 0):
        on = runlen > k
        r = rows[first[on] + k]
        wk = w[r].astype(np.float32)[:, None]
        want_geo[pts[on]] = want_geo[pts[on]] + (wk * dc_geo[r >> 3]).astype(np.float32)
        if color and rel_pos:
            want_col[pts[on]] = want_col[pts[on]] + dfeat[r]
        elif color:
            want_col[pts[on]] = want_col[pts[on]] + (wk * dc_col[r >> 3]).astype(np.float32)
    assert total == 0 or np.isfinite(want_geo).all() and np.abs(want_geo).max() > 0
    assert torch.equal(gs.g_geo.cpu(), torch.from_numpy(want_geo))
    assert torch.equal(gs.g_col.cpu(), torch.from_numpy(want_col))
    assert not color or total == 0 or np.abs(want_col).max() > 0
    return first, runlen, total


@pytest.mark.parametrize('backend', backends())
def test_relpos_rows_and_the_cases_of_the_walk(backend):
    first, runlen, total = _run(backend)
    end = first + runlen
    assert runlen.max() > 64                                                       # more than two windows
    assert (runlen == 1).any()
    assert ((first % CHUNK == CHUNK - 1) & (runlen > 1)).any()                     # starts in a chunk's last slot and goes on
    c0 = (first // CHUNK + 1) * CHUNK                                              # first chunk behind the run's start
    assert (end >= c0 + CHUNK).any()                                               # a chunk that lies inside one run
    assert end.max() == total and total % 4 and total % 16 and total % 32


@pytest.mark.parametrize('backend', backends())
def test_plain_colour_model(backend):
    _run(backend, rel_pos=False)


@pytest.mark.parametrize('backend', backends())
def test_geometry_stage_leaves_the_colour_table(backend):
    _run(backend, stage='geometry')


@pytest.mark.parametrize('backend', backends())
def test_one_ray(backend):
    _run(backend, R=1)


@pytest.mark.parametrize('backend', backends())
def test_empty_list(backend):
    assert _run(backend, mask_zero=True)[2] == 0


@pytest.mark.parametrize('backend', backends())
def test_half_feature_tables(backend):
    _run(backend, f16=True)


@pytest.mark.parametrize('backend', backends())
def test_mapping_loop_repeats_bit_for_bit(backend):
    """The loop path (rows sorted ahead of the loop in batches, sort keys of the optimised rows, list lengths on the device): the same
    mapping call from the same state twice leaves the same bits in the feature tables and the decoder blob."""
    eng = make_engine(backend)
    cam = dict(H=48, W=64, fx=51.7, fy=51.6, cx=31.9, cy=25.5)
    # the mapping budget of tests/test_workload.py on the emulator; one small tracking iteration, which the step needs and this test does not
    cloud = syn.build_cloud(4000, device='cpu', seed=3, intr=cam)
    out = []
    for _ in range(2):
        b = workload.Budget(window=3, every_frame=2, track_iters=1, track_rays=8, map_iters=4, map_geo_iters=2, map_rays=48, n_points=4000,
                            pixels_adding=120)
        b.ignore_edge = 4
        pos, geo, col = (t.clone().to(eng.device) for t in cloud)
        wl = workload.FrameWorkload(eng, b, cloud=(pos, geo, col, 1), intr=cam)
        wl.step(full=False)
        if eng.device.type == 'cuda':
            torch.cuda.synchronize()
        out.append((wl.geo[:wl.n].clone(), wl.col[:wl.n].clone(), wl.dec.blob.clone()))
    assert float((out[0][0][:4000] - cloud[1].to(eng.device)).abs().max()) > 0          # the call stepped the rows
    for a, c in zip(*out):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))
