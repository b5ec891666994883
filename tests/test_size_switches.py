"""Every launcher of loopy_slam_amd/csrc that chooses a kernel form from the problem size, on both sides of its switch (the sizes:
tests/switch_referee.py), against NumPy / float64 references or - for the render, whose forms are meant to differ in scheduling only -
against the same rays in a batch on the other side of the switch.  Both back-ends (see test_forward_parity.py) unless a case says why not."""
import ctypes as C

import numpy as np
import pytest
import torch

from loopy_slam_amd import _ffi, core, optim, steps, synthetic as syn
from loopy_slam_amd._ffi import ptr
from oracle import hotpath as H
from util import make_engine, backends
import switch_referee as sw

GUARD = 8


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def guarded(eng, n, dtype, fill):
    """(whole buffer, the n elements the kernel is given): GUARD elements of `fill` follow them."""
    full = torch.full((n + GUARD,), fill, dtype=dtype, device=eng.device)
    return full, full[:n]


def test_sizes_mirror_the_sources():
    """The sizes of switch_referee.py against the `#define`s of loopy_slam_amd/csrc and the header they mirror: a knob that moves there
    fails here until the sizes of this module move with it (the render cases compare the forms of a launch with each other, so they are
    blind to a switch that has left the range of their batches).  The thresholds written as literals inside conditions are not read."""
    import os
    define = sw.source_define                                                                                         # 8192 or (1 << 14)
    assert define('lk_mask_dev.h', 'LK_MASK_REG_MAX') == sw.MASK_REG_MAX
    assert define('lk_sample.hip', 'LK_T16_MAX_P') == sw.T16_MAX_P
    assert define('lk_kernels.h', 'LK_DEEP_MAX_TILES') == define('lk_kernels.h', 'LK_DEEP_MAX_TILES_FWD') == sw.DEEP_MAX_TILES
    assert define('lk_kernels.h', 'LK_COMPACT_ONE_BLOCK_MAX') == sw.COMPACT_ONE_BLOCK_MAX
    header = os.path.join('..', '..', 'include', 'loopy_hip.h')
    assert define(header, 'LK_EXPOSURE_MAX_F') == sw.EXPOSURE_MAX_F and define(header, 'LK_ADAM_MAX_SEG') == sw.ADAM_MAX_SEG
    # the counts of tests/test_sample_counts.py: every S the ABI accepts
    assert define(header, 'LK_S_MAX') == sw.S_MAX == _ffi.LK_S_MAX


# ---------------------------------------------------------------------------- A. lk_inside_mask
MASK_SIZES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025) + sw.straddle(sw.MASK_REG_MAX) + (16384, 20001)


def test_mask_patterns_take_both_threshold_paths():
    """The patterns are meant to reach the one-pass shortcut AND the radix select on each side of LK_MASK_REG_MAX."""
    for n in (sw.MASK_REG_MAX, sw.MASK_REG_MAX + 1):
        need = {p: sw.needs_median(sw.depth_pattern(p, n, n)) for p in sw.MASK_PATTERNS}
        assert need == dict(uniform=False, outlier=True, equal=False, two=True, lowbyte=True, subnormal=False, inf=True, nonpos=False)
    # the lower median: with 1.0 and 30.0 in equal numbers the upper one would give thr = 36 and keep everything
    thr, mask, _ = sw.inside_mask_ref(sw.depth_pattern('two', 64, 0))
    assert thr == 10.0 and int(mask.sum()) == 32


@pytest.mark.parametrize('n', MASK_SIZES)
@pytest.mark.parametrize('backend', backends())
def test_inside_mask(backend, n):
    """Threshold, mask and filtered depth bit for bit, for every depth pattern with the mask alone, depth_filtered alone and both;
    what lies behind the n-th element of either output stays as it was."""
    eng = make_engine(backend)
    for pat in sw.MASK_PATTERNS:
        d = sw.depth_pattern(pat, n, 1000 * n + len(pat))
        ref_thr, ref_mask, ref_f = sw.inside_mask_ref(d)
        dev = eng.f32(torch.from_numpy(d))
        assert torch.equal(bits(dev).cpu(), torch.from_numpy(d.view(np.int32)))          # (subnormals and -0 arrive as they are)
        for want_mask, want_f in ((True, False), (False, True), (True, True)):
            mfull, mask = guarded(eng, n, torch.uint8, 0xEE)
            ffull, filt = guarded(eng, n, torch.float32, 77.0)
            thr = eng.f32(torch.tensor([-5.0]))
            scratch = eng.empty(n, dtype=torch.int32)
            optim.inside_mask(eng, dev, mask if want_mask else None, thr, scratch, depth_filtered=filt if want_f else None)
            what = f'{pat} n={n} mask={want_mask} filtered={want_f}'
            assert thr.cpu().numpy().view(np.int32)[0] == ref_thr.view(np.int32), f'{what}: thr {float(thr.cpu())} != {float(ref_thr)}'
            got_m, got_f = mfull.cpu().numpy(), ffull.cpu().numpy()
            assert np.array_equal(got_m[:n], ref_mask.astype(np.uint8) if want_mask else np.full(n, 0xEE, np.uint8)), what
            assert np.array_equal(got_f[:n].view(np.int32), (ref_f if want_f else np.full(n, 77.0, np.float32)).view(np.int32)), what
            assert (got_m[n:] == 0xEE).all() and (got_f[n:] == 77.0).all(), f'{what}: wrote behind the output'


# ---------------------------------------------------------------------------- B. compaction
COMPACT_LARGE_SIZES = (0, 1, 255, 256, 257, 1024) + sw.straddle(sw.COMPACT_ONE_BLOCK_MAX, sw.COMPACT_ONE_BLOCK_MAX + 256) + \
    sw.straddle(sw.COMPACT_PASS * sw.COMPACT_BLOCK, sw.COMPACT_PASS * sw.COMPACT_BLOCK + 257) + (600001,)
COMPACT_SIZES = sw.straddle(sw.COMPACT_PASS) + (16385, 100000)
SENTINEL = -7


def _check_compact(eng, n, large):
    for name in sw.COMPACT_MASKS if n else ('zeros',):
        m = sw.compact_mask(name, n, 31 * n + len(name))
        ref = np.flatnonzero(m).astype(np.int32)
        mask = torch.from_numpy(m).to(eng.device) if n else eng.zeros(1, dtype=torch.uint8)
        out = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=eng.device)
        cnt = torch.full((1 + GUARD,), SENTINEL, dtype=torch.int32, device=eng.device)
        if large:
            nb = -(-n // sw.COMPACT_BLOCK)                       # block_scratch: ceil(n / 256) ints, and not one more
            scr = torch.full((nb + GUARD,), SENTINEL, dtype=torch.int32, device=eng.device)
            eng.lib.check(eng.lib.dll.lk_compact_large(ptr(mask), n, ptr(out), ptr(cnt), ptr(scr), eng.stream), 'lk_compact_large')
            assert bool((scr[nb:] == SENTINEL).all()), f'{name} n={n}: wrote behind block_scratch'
        else:
            eng.lib.check(eng.lib.dll.lk_compact(ptr(mask), n, ptr(out), ptr(cnt), eng.stream), 'lk_compact')
        k, got = int(cnt[0]), out.cpu().numpy()
        assert k == ref.size, f'{name} n={n}: count {k} != {ref.size}'
        assert np.array_equal(got[:k], ref), f'{name} n={n}: indices'
        assert (got[k:] == SENTINEL).all() and bool((cnt[1:] == SENTINEL).all()), f'{name} n={n}: wrote behind the count-th index'


@pytest.mark.parametrize('n', COMPACT_LARGE_SIZES)
@pytest.mark.parametrize('backend', backends())
def test_compact_large(backend, n):
    """One workgroup up to 16 384 entries, count / scan / scatter above (the scan carries across passes of 1024 blocks = 262 144
    entries): count, indices (ascending: np.flatnonzero) and everything behind them, for eight kinds of mask."""
    _check_compact(make_engine(backend), n, large=True)


@pytest.mark.parametrize('n', COMPACT_SIZES)
@pytest.mark.parametrize('backend', backends())
def test_compact(backend, n):
    """The one-workgroup form on its own entry point: 1024 entries per pass, the running base carried across passes."""
    _check_compact(make_engine(backend), n, large=False)


# ---------------------------------------------------------------------------- C. lk_touch_rows
TOUCH_SHAPES = ((1, 1), (5000, 300), (sw.GRID_CAP_ROWS * 256, 70000), (sw.GRID_CAP_ROWS * 256 + 4097, 70000))


@pytest.mark.parametrize('n,N', TOUCH_SHAPES)
@pytest.mark.parametrize('backend', backends())
def test_touch_rows_across_the_grid_cap(backend, n, N):
    """Indices uniform in [-3, N + 5): -1, other negative and out-of-range values all occur; the flags are a NumPy scatter of ones over
    the in-range indices, every other flag stays 0 and the bytes behind the N-th keep their fill.  1 048 576 indices are the last
    launch with one index per thread, 1 052 673 the first whose grid-stride loop runs twice in some blocks and once in others."""
    eng = make_engine(backend)
    idx = torch.randint(-3, N + 5, (n,), generator=torch.Generator().manual_seed(n + N), dtype=torch.int32)
    if n == 1:
        idx[0] = 0
    ffull, flags = guarded(eng, N, torch.uint8, 9)
    flags.zero_()
    idx_dev = idx.to(eng.device)
    eng.lib.check(eng.lib.dll.lk_touch_rows(ptr(idx_dev), n, ptr(flags), N, eng.stream), 'lk_touch_rows')
    ref = np.full(N + GUARD, 9, dtype=np.uint8)
    ref[:N] = 0
    i64 = idx.numpy().astype(np.int64)
    ref[i64[(i64 >= 0) & (i64 < N)]] = 1
    assert np.array_equal(ffull.cpu().numpy(), ref)
    if n > 1:
        assert (i64 == -1).any() and (i64 < -1).any() and (i64 >= N).any() and 0 < int(ref[:N].sum())


FLAG_ROWS_N = (1, 300, 70000)
FLAG_ROWS_CASES = [pytest.param(be, n, marks=[pytest.mark.gpu] if be == 'hip' else [], id=f'{be}-{n}') for be in ('emu', 'hip') for n in FLAG_ROWS_N] + \
    [pytest.param('hip', sw.GRID_CAP_ROWS * 256 + 4097, marks=pytest.mark.gpu, id=f'hip-{sw.GRID_CAP_ROWS * 256 + 4097}')]


@pytest.mark.parametrize('backend,n', FLAG_ROWS_CASES)
def test_knn_flag_rows_through_the_flagged_step(backend, n):
    """lk_knn_flag_rows ORs a flag array into the row flags of a KnnIndex, which have no read-back: they are observed through the step
    they steer.  lk_map_frame with rows = NULL, union_rows_flagged = 1 and phases = 2 (the step half of a data-parallel caller's
    iteration: no batch, no backward, the flags are not cleared) is one lk_adam_step over the rows of both feature tables whose flag
    is set.  Both gradient tables hold 0.5 everywhere, so Adam's first step moves every element of a stepped row by lr (0.03 / 0.005)
    to rounding and clears its gradient; every other row keeps its bits, its gradient and its zero moments.
    Two calls: NumPy-known flags over all n rows (bytes 1 .. 255, density 0.3), then other flags over the first n / 2 rows only - the
    result is the OR, the rows behind n / 2 keep the first call's flags.  1 052 673 rows: above the cap of 4096 blocks x 256, the
    grid-stride loop runs twice in some blocks; chip only (1.1 GB of tables, gradients and moments)."""
    eng = make_engine(backend)
    dev = eng.device
    rng = np.random.default_rng(n)
    fa = np.where(rng.random(n) < 0.3, rng.integers(1, 256, n), 0).astype(np.uint8)
    fa[-1] = 255 if n > 1 else 1
    n2 = n // 2
    fb = (rng.random(n2) < 0.2).astype(np.uint8)
    want = fa != 0
    want[:n2] |= fb != 0
    knn = core.KnnIndex(eng, capacity=n, max_cells=1 << 12)
    dll = eng.lib.dll
    fa_d, fb_d = torch.from_numpy(fa).to(dev), torch.from_numpy(fb).to(dev) if n2 else None
    eng.lib.check(dll.lk_knn_flag_rows(knn.h, ptr(fa_d), n, eng.stream), 'lk_knn_flag_rows')
    eng.lib.check(dll.lk_knn_flag_rows(knn.h, ptr(fb_d), n2, eng.stream), 'lk_knn_flag_rows')
    # the step: a 'color' iteration without decoder spans - the two feature-row segments and nothing else
    g = torch.Generator().manual_seed(n)
    geo0, col0 = (torch.randn(n, 32, generator=g) * 0.1 for _ in range(2))
    geo, col = eng.f32(geo0).clone(), eng.f32(col0).clone()
    g_geo, g_col = torch.full((n, 32), 0.5, device=dev), torch.full((n, 32), 0.5, device=dev)
    adam_rows = eng.zeros(4 * n * 32)
    nb = eng.lib.blob_floats()
    blob, frag = eng.zeros(nb), eng.zeros(int(dll.lk_weight_frag_floats()))
    g_w, adam_dec = eng.zeros(nb), eng.zeros(2 * nb)
    small = {k: eng.zeros(64) for k in ('depth', 'color', 'c2w', 'log', 'gt_color', 'thr', 'd_depth', 'd_color', 'scratch', 'act')}
    rnd, scratch_u32 = eng.zeros(8, dtype=torch.int32), eng.zeros(8, dtype=torch.int32)
    d = _ffi.MapDesc()
    r = d.render
    r.R, r.S, r.stats_chunk, r.flags, r.knn = 1, sw.S, 1, 0, knn.h
    r.g_geo_feats, r.g_col_feats, r.g_weights = ptr(g_geo), ptr(g_col), ptr(g_w)
    r.d_depth, r.d_color, r.bwd_scratch, r.bwd_scratch_cap, r.act = ptr(small['d_depth']), ptr(small['d_color']), ptr(small['scratch']), 64, ptr(small['act'])
    d.depth_stack, d.color_stack, d.c2w_stack, d.c2w_stride, d.rnd, d.log = ptr(small['depth']), ptr(small['color']), ptr(small['c2w']), 16, ptr(rnd), ptr(small['log'])
    d.gt_color, d.thr, d.scratch_u32 = ptr(small['gt_color']), ptr(small['thr']), ptr(scratch_u32)
    d.H, d.W, d.w = 1, 1, 1
    d.weights_rw, d.weights_frag_rw, d.geo_feats_rw, d.col_feats_rw = ptr(blob), ptr(frag), ptr(geo), ptr(col)
    d.rows, d.n_rows, d.adam_rows, d.adam_dec = None, n, ptr(adam_rows), ptr(adam_dec)
    d.n_geo_dec, d.n_col_dec = 0, 0
    lr_geo, lr_col = 0.03, 0.005
    d.lr[1][0], d.lr[1][1], d.lr[1][2] = 0.0, lr_geo, lr_col
    d.iters, d.n_geo_iters, d.union_rows_flagged = 1, 0, 1
    eng.lib.check(dll.lk_map_frame(C.byref(d), 0, 1, 2, eng.stream), 'lk_map_frame')
    w = torch.from_numpy(want)
    assert 0 < int(w.sum()) <= n and (n < 300 or int(w.sum()) < n)
    m = adam_rows.view(4, n, 32).cpu()
    for name, tab, tab0, grad, lr, mv in (('geo', geo, geo0, g_geo, lr_geo, m[0:2]), ('col', col, col0, g_col, lr_col, m[2:4])):
        tab, grad = tab.cpu(), grad.cpu()
        moved = (bits(tab) != bits(tab0)).any(1)
        assert torch.equal(moved, w), f'{name}: {int((moved != w).sum())} rows stepped or left against the flags, first {int((moved != w).nonzero()[0])}'
        assert torch.equal(bits(tab[~w]), bits(tab0[~w])) and bool((grad[~w] == 0.5).all()) and not bool(mv[:, ~w].any())
        assert not bool(grad[w].any()) and bool((mv[:, w] > 0).all())
        np.testing.assert_allclose(tab[w].numpy(), (tab0[w].double() - lr).numpy(), rtol=0, atol=1e-4 * lr + 2e-8)


# ---------------------------------------------------------------------------- D. lk_bucket_copy
def _copy_segs(items):
    """items: (tensor or None, n, row_index or None, row_len)."""
    arr = (_ffi.CopySeg * max(1, len(items)))()
    for i, (data, n, rows, row_len) in enumerate(items):
        arr[i].data, arr[i].n, arr[i].row_index, arr[i].row_len = ptr(data), n, ptr(rows), row_len
    return arr


@pytest.mark.parametrize('backend', backends())
def test_bucket_copy_across_the_grid_cap(backend):
    """One call, four segments: plain spans of 262 657 floats (above the cap of 1024 blocks x 256: the grid-stride loop runs twice in
    the first 513 threads), 0 floats (NULL, in the middle: the offsets behind it must not move) and 262 144 floats (the last
    one-element-per-thread launch - the LARGEST segment sizes the grid, so it strides too when alone: run alone as well), and 123
    sorted rows of a [500, 3] table.  Modes 0 (pack), 1 (unpack) and 2 (pack and clear) against the torch formulation, bit for bit."""
    eng = make_engine(backend)
    g = torch.Generator().manual_seed(11)
    na, nb = sw.GRID_CAP_BUCKET * 256 + 513, sw.GRID_CAP_BUCKET * 256
    A, B, T = (eng.f32(torch.randn(k, generator=g)) for k in (na + 20, nb + 20, 1500))
    T = T.view(500, 3)
    rows = torch.randperm(500, generator=g)[:123].sort().values.to(torch.int32).to(eng.device)
    sa, sb = A[7:7 + na], B[13:13 + nb]                    # spans inside larger tensors: what lies around them must not move
    items = [(sa, na, None, 0), (None, 0, None, 0), (sb, nb, None, 0), (T, 123 * 3, rows, 3)]
    total = na + nb + 123 * 3
    dll = eng.lib.dll

    def call(segs, n_seg, bucket, mode):
        eng.lib.check(dll.lk_bucket_copy(segs, n_seg, ptr(bucket), mode, eng.stream), 'lk_bucket_copy')
    segs = _copy_segs(items)
    cat = torch.cat([sa, sb, T[rows.long()].reshape(-1)])
    # mode 0
    bucket = torch.full((total + 5,), 77.0, device=eng.device)
    snap = [x.clone() for x in (A, B, T)]
    call(segs, 4, bucket, 0)
    assert torch.equal(bits(bucket[:total]), bits(cat)) and bool((bucket[total:] == 77.0).all())
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip((A, B, T), snap))
    alone = torch.full((nb + 5,), 77.0, device=eng.device)
    call(_copy_segs(items[2:3]), 1, alone, 0)
    assert torch.equal(bits(alone[:nb]), bits(sb)) and bool((alone[nb:] == 77.0).all())
    # mode 1: the doubled bucket goes back; only the addressed spans and rows change
    bucket[:total] *= 2
    call(segs, 4, bucket, 1)
    want = [x.clone() for x in snap]
    want[0][7:7 + na] *= 2
    want[1][13:13 + nb] *= 2
    want[2][rows.long()] *= 2
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip((A, B, T), want))
    assert bool((bucket[total:] == 77.0).all())
    # mode 2: the bucket as in mode 0, the addressed source elements zero (+0.0), the rest keeps its bits
    cat2 = torch.cat([sa, sb, T[rows.long()].reshape(-1)])
    b2 = torch.full((total + 5,), 77.0, device=eng.device)
    call(segs, 4, b2, 2)
    assert torch.equal(bits(b2[:total]), bits(cat2)) and bool((b2[total:] == 77.0).all())
    want[0][7:7 + na] = 0
    want[1][13:13 + nb] = 0
    want[2][rows.long()] = 0
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip((A, B, T), want))


@pytest.mark.parametrize('backend', backends())
def test_bucket_copy_segment_limit(backend):
    """LK_ADAM_MAX_SEG = 16 segments are accepted, 17 are refused before anything is copied."""
    eng = make_engine(backend)
    src = eng.f32(torch.arange(17 * 5, dtype=torch.float32))
    items = [(src[5 * i:5 * i + 5], 5, None, 0) for i in range(17)]
    bucket = torch.full((17 * 5 + 5,), 77.0, device=eng.device)
    assert sw.ADAM_MAX_SEG == 16
    eng.lib.check(eng.lib.dll.lk_bucket_copy(_copy_segs(items[:16]), 16, ptr(bucket), 0, eng.stream), 'lk_bucket_copy')
    assert torch.equal(bucket[:80], src[:80]) and bool((bucket[80:] == 77.0).all())
    bucket.fill_(77.0)
    rc = eng.lib.dll.lk_bucket_copy(_copy_segs(items), 17, ptr(bucket), 0, eng.stream)
    assert rc != 0
    with pytest.raises(_ffi.LoopyError):
        eng.lib.check(rc, 'lk_bucket_copy')
    assert bool((bucket == 77.0).all())


# ---------------------------------------------------------------------------- E. lk_knn_query, 8 lanes per query
_KNN_REF = {}


def _knn_case(kind):
    """Cloud, queries and the oracle's answer for the LONGEST query list, computed once per kind: a query's answer does not depend on
    the others, so the answer for a prefix of the list is the prefix of the answer.
    uniform / per_query: 1 500 points uniform in [-1, 1]^3 - a row of 0.08-m cells holds a point or two, so only the first lanes of a
    query ever meet a candidate; dense: the same number of points in [-0.16, 0.16]^3, ~90 per row of cells: every lane of either
    form has candidates in every row, r = 0.08 (one cell edge: the nine-row walk, where the two radii above take the row loop)."""
    if kind not in _KNN_REF:
        g = torch.Generator().manual_seed(65537)
        half = 0.16 if kind == 'dense' else 1.0
        pts = (torch.rand(1500, 3, generator=g) * 2 - 1) * half
        q = (torch.rand(sw.KNN_T16_BELOW + 1, 3, generator=g) * 2.2 - 1.1) * half
        r2 = {'uniform': np.float32(0.0256), 'dense': np.float32(0.0064)}.get(kind)
        if kind == 'per_query':
            r2 = ((0.04 + 0.26 * torch.rand(q.shape[0], generator=g)) ** 2).float()
        _KNN_REF[kind] = (pts, q, r2, H.knn_exact(pts.numpy(), q.numpy(), 8, r2.numpy() if kind == 'per_query' else r2))
    return _KNN_REF[kind]


@pytest.mark.parametrize('P,kind', [(P, 'uniform') for P in sw.straddle(sw.KNN_T16_BELOW)] + [(sw.KNN_T16_BELOW + 1, 'per_query')] +
                         [(sw.KNN_T16_BELOW - 1, 'dense'), (sw.KNN_T16_BELOW, 'dense')])
@pytest.mark.parametrize('backend', backends())
def test_knn_query_lanes_per_query(backend, P, kind):
    """65 535 queries are the last launch with 16 lanes per query, 65 536 the first with 8: indices, distances and counts bit for bit
    against hotpath.knn_exact, with r^2 = 0.0256, (P = 65 537) with per-query radii of 0.04 .. 0.3, and on a dense cloud."""
    eng = make_engine(backend)
    pts, q, r2, (od, oi, oc) = _knn_case(kind)
    knn = core.KnnIndex(eng, capacity=pts.shape[0])
    knn.build(eng.f32(pts))
    d2, idx, cnt = knn.query(eng.f32(q[:P]), eng.f32(r2[:P]) if kind == 'per_query' else float(r2))
    assert np.array_equal(idx.cpu().numpy(), oi[:P])
    assert np.array_equal(d2.cpu().numpy().view(np.int32), od[:P].view(np.int32))
    assert np.array_equal(cnt.cpu().numpy(), oc[:P])
    if kind == 'dense':
        assert float((oi[:P, 7] >= 0).mean()) > 0.9                                      # nearly every list is full
    else:
        assert 0 < int((oc[:P] == 0).sum()) < P and int((oi[:P, 7] >= 0).sum()) > 0      # empty and full lists both occur


# ---------------------------------------------------------------------------- H. exposure MLP at its limits
def _exposure_inputs(eng, F):
    g = torch.Generator().manual_seed(100 + F)
    shapes = dict(feats=((F, 8), 0.5), W1=((128, 8), 0.3), b1=((128,), 0.05), W2=((12, 128), 0.1), b2=((12,), 0.1), g_aff=((F, 12), 1.0))
    return {k: eng.f32(s * torch.randn(*shape, generator=g)) for k, (shape, s) in shapes.items()}


@pytest.mark.parametrize('F', (1, 2, sw.EXPOSURE_MAX_F - 1, sw.EXPOSURE_MAX_F))
@pytest.mark.parametrize('backend', backends())
def test_exposure_mlp(backend, F):
    """lk_exposure_fwd / lk_exposure_bwd for 1, 2, 31 and LK_EXPOSURE_MAX_F = 32 features against float64 autograd, every output element
    within its own bound (switch_referee.exposure_ref: (L + 8) 2^-24 sum|terms| of the element's chain plus what the bounds of the
    chain's inputs amount to - the softplus of beta 100 makes its derivative 100 times as sensitive as its argument), and the root
    mean square of every tensor's errors within the same expression under the probabilistic rounding model, sqrt(L + 8).  The gradient
    buffer is [W1 1024 | b1 128 | W2 1536 | b2 12 | feats 8F]; what lies behind 2700 + 8F floats stays as it was."""
    eng = make_engine(backend)
    x = _exposure_inputs(eng, F)
    aff, hid = eng.empty(F, 12), eng.empty(F, 128)
    g = torch.full((_ffi.EXPOSURE_GRAD_FLOATS + GUARD,), 77.0, device=eng.device)
    dll = eng.lib.dll
    eng.lib.check(dll.lk_exposure_fwd(ptr(x['feats']), ptr(x['W1']), ptr(x['b1']), ptr(x['W2']), ptr(x['b2']), F, ptr(aff), ptr(hid), eng.stream),
                  'lk_exposure_fwd')
    eng.lib.check(dll.lk_exposure_bwd(ptr(x['feats']), ptr(x['W1']), ptr(x['W2']), ptr(hid), ptr(x['g_aff']), F, ptr(g), eng.stream), 'lk_exposure_bwd')
    val, bound = sw.exposure_ref(*(x[k].cpu().numpy() for k in ('feats', 'W1', 'b1', 'W2', 'b2', 'g_aff')))
    _, typical = sw.exposure_ref(*(x[k].cpu().numpy() for k in ('feats', 'W1', 'b1', 'W2', 'b2', 'g_aff')), k=lambda L: np.sqrt(L + 8))
    gh = g.cpu().numpy().astype(np.float64)
    got = dict(aff=aff.cpu().numpy(), hid=hid.cpu().numpy(), gW1=gh[:1024].reshape(128, 8), gb1=gh[1024:1152], gW2=gh[1152:2688].reshape(12, 128),
               gb2=gh[2688:2700], gfeats=gh[2700:2700 + 8 * F].reshape(F, 8))
    assert (gh[2700 + 8 * F:] == 77.0).all(), 'wrote behind the gradient layout'
    for k in ('aff', 'hid', 'gW1', 'gb1', 'gW2', 'gb2', 'gfeats'):
        err = np.abs(got[k].astype(np.float64) - val[k])
        worst = float((err / np.maximum(bound[k], 1e-300)).max())
        print(f'exposure F={F} {k}: worst error {float(err.max()):.3e} ({float(err.max() / np.abs(val[k]).max()):.2e} of the largest entry), '
              f'{worst:.3f} of its bound, bound {float(bound[k].max() / np.abs(val[k]).max()):.2e} of the largest entry')
        assert np.isfinite(got[k]).all() and float(np.abs(val[k]).max()) > 0
        assert (err <= bound[k]).all(), f'{k}: {worst:.2f} x its bound'
        rms, rms_b = float(np.sqrt((err ** 2).mean())), float(np.sqrt((typical[k] ** 2).mean()))
        print(f'exposure F={F} {k}: rms error {rms:.3e}, {rms / max(rms_b, 1e-300):.3f} of the probabilistic size {rms_b:.3e} '
              f'({rms_b / np.abs(val[k]).max():.2e} of the largest entry)')
        assert rms <= rms_b, f'{k}: rms error {rms:.3e} above the probabilistic size {rms_b:.3e}'


@pytest.mark.parametrize('F', (0, sw.EXPOSURE_MAX_F + 1))
@pytest.mark.parametrize('backend', backends())
def test_exposure_mlp_refuses_bad_feature_counts(backend, F):
    eng = make_engine(backend)
    x = _exposure_inputs(eng, max(F, 1))
    aff, hid = eng.zeros(max(F, 1), 12), eng.zeros(max(F, 1), 128)
    g = torch.full((_ffi.EXPOSURE_GRAD_FLOATS + 8 * F + GUARD,), 77.0, device=eng.device)
    dll = eng.lib.dll
    rcs = (dll.lk_exposure_fwd(ptr(x['feats']), ptr(x['W1']), ptr(x['b1']), ptr(x['W2']), ptr(x['b2']), F, ptr(aff), ptr(hid), eng.stream),
           dll.lk_exposure_bwd(ptr(x['feats']), ptr(x['W1']), ptr(x['W2']), ptr(hid), ptr(x['g_aff']), F, ptr(g), eng.stream))
    for rc in rcs:
        assert rc != 0
        with pytest.raises(_ffi.LoopyError):
            eng.lib.check(rc, 'lk_exposure')
    assert bool((g == 77.0).all()) and not bool(aff.any()) and not bool(hid.any())


# ---------------------------------------------------------------------------- F. the 16384-sample switch of the render
R_EPILOGUE = sw.rays_at(sw.TRACK_EPILOGUE_TILE * sw.DEEP_MAX_TILES)            # 3072: lk_track_frame's loss epilogue up to here
R_T16 = sw.rays_at(sw.T16_MAX_P)                                               # 3276: 16 lanes per sample, 512 tiles, up to here
RENDER_R = (R_EPILOGUE, R_EPILOGUE + 1, R_T16, R_T16 + 1, 3300)
R_SHARED = RENDER_R[0]
SIGNAL = slice(R_SHARED - 12, R_SHARED)            # the rays that carry the whole loss gradient: the last of the smallest batch
_RENDER = {}


def test_render_batches_straddle_the_switches():
    S = sw.S
    assert RENDER_R == (3072, 3073, 3276, 3277, 3300)
    assert -(-R_T16 * S // 32) == sw.DEEP_MAX_TILES and R_T16 * S % 32 != 0 and R_T16 * S <= sw.T16_MAX_P           # 512 tiles, the last partial, 16 lanes
    assert -(-(R_T16 + 1) * S // 32) == sw.DEEP_MAX_TILES + 1 and (R_T16 + 1) * S % 32 == 1 and (R_T16 + 1) * S > sw.T16_MAX_P
    assert -(-R_EPILOGUE * S // sw.TRACK_EPILOGUE_TILE) == sw.DEEP_MAX_TILES < -(-(R_EPILOGUE + 1) * S // sw.TRACK_EPILOGUE_TILE)


def _render_scene(eng, backend):
    """20 000-point synthetic room, 3 300 random pixels of frame 5 (2 % of them without a depth reading), drawn once per back-end."""
    if backend not in _RENDER:
        pos, geo, col = (eng.f32(x) for x in syn.build_cloud(20000, device='cpu'))
        knn = core.KnnIndex(eng, capacity=pos.shape[0])
        knn.build(pos)
        depth, _, c2w = syn.render_frame(5, device='cpu', holes=0.02)
        g = torch.Generator().manual_seed(3300)
        i = torch.randint(0, syn.TUM_INTR['W'], (RENDER_R[-1],), generator=g)
        j = torch.randint(0, syn.TUM_INTR['H'], (RENDER_R[-1],), generator=g)
        ro, rd = syn.pixel_rays(c2w, i.float(), j.float())
        _RENDER[backend] = dict(pos=pos, geo=geo, col=col, knn=knn, ro=eng.f32(ro), rd=eng.f32(rd), gd=eng.f32(depth[j, i]), blob={})
    return _RENDER[backend]


def _render_cases():
    out = []
    for tracker in (False, True):
        for stage in ('geometry', 'color'):
            for rel_pos in (True, False):
                for be in ('emu', 'hip') if (stage == 'geometry' and not tracker) else ('hip',):
                    for R in RENDER_R:
                        out.append(pytest.param(be, rel_pos, stage, tracker, R, marks=[pytest.mark.gpu] if be == 'hip' else [],
                                                id=f'{be}-{"relpos" if rel_pos else "plain"}-{stage}-{"tracker" if tracker else "mapper"}-{R}'))
    return out


def _render_run(eng, sc, rel_pos, stage, tracker, R):
    """Forward and backward of the first R rays of the list: the outputs and saved state of the 3072 shared rays, and the gradients."""
    if rel_pos not in sc['blob']:
        sc['blob'][rel_pos] = core.DecoderBlob(eng).pack(syn.default_weights(rel_pos=rel_pos))
    blob, cfg = sc['blob'][rel_pos], core.RenderCfg(rel_pos=rel_pos)
    N, S = sc['pos'].shape[0], cfg.S
    ro, rd, gd = (sc[k][:R].contiguous() for k in ('ro', 'rd', 'gd'))
    st = core.RenderState(eng, R, S, need_act=True)
    core.render_forward(eng, cfg, st, ro, rd, gd, sc['knn'], sc['pos'], sc['geo'], sc['col'], blob, stage, tracker=tracker, save_act=True,
                        stats_chunk=R_SHARED)
    d_depth, d_color, d_var = eng.zeros(R), eng.zeros(R, 3), (eng.zeros(R) if tracker else None)
    d_depth[SIGNAL], d_color[SIGNAL] = 1.0, 0.5
    if tracker:
        d_var[SIGNAL] = 0.25
    gs = core.GradState(eng, N, R, blob.n, feats=not tracker, weights=not tracker, rays=tracker)
    core.render_backward(eng, st, gs, d_depth, d_color, d_var)
    out = {k: getattr(st, k)[:R_SHARED * (S if getattr(st, k).shape[0] == R * S else 1)].clone() for k in FWD_NAMES}
    if tracker:
        out['g_rays_o'], out['g_rays_d'] = gs.g_rays_o[:R_SHARED].clone(), gs.g_rays_d[:R_SHARED].clone()
        assert not bool(gs.g_rays_o[R_SHARED:].any()) and not bool(gs.g_rays_d[R_SHARED:].any())
    else:
        out.update({k: getattr(gs, k).clone() for k in ('g_geo', 'g_col', 'g_weights')})
    return out


FWD_NAMES = ('depth', 'color', 'var', 'valid_ray', 'z', 'nbr_idx', 'nbr_w', 'nbr_count', 'c_geo', 'c_col')
_RENDER_BASE = {}


@pytest.mark.parametrize('backend,rel_pos,stage,tracker,R', _render_cases())
def test_render_forms_agree_across_the_sample_switch(backend, rel_pos, stage, tracker, R):
    """Prefixes of 3072, 3073, 3276, 3277 and 3300 rays of ONE ray list, S = 5, through core.render_forward / render_backward (the
    stand-alone lk_render_fwd / lk_render_bwd).  At 3276 rays the batch has 16 380 samples (512 tiles, the last partial): the in-line
    search k_sample_interp<16, 0> and, in the colour stage, the deep-prefetch k_decode_fwd<true> and k_decode_bwd.  At 3277 rays it has
    16 385 (513 tiles, the last with one sample): k_sample_interp<8, 0> and the plain decoder forms.  These are the only switches a
    stand-alone render has here: the fused rel-pos + decode forward, fuse_small and the tracker's loss epilogue exist inside
    lk_track_frame only (test_track_loop_forms_match_the_statement_path), so 3072 and 3073 rays straddle nothing in this test; 3072 is
    the batch every other one is compared with.
    The forms are meant to differ in scheduling only, so the 3072 rays that every batch shares give the same bits in every batch:
    depth, colour, variance, validity, sample depths, neighbour lists and weights, the interpolated features (c_col for the plain
    colour stage only).  (The far bound of the rays without a depth reading is a statistic over `stats_chunk` rays: 3072 here, so
    that it is the same rays' in every batch.)
    Backward: d depth = 1, d colour = 0.5 (tracker: d var = 0.25 too) on rays 3060 .. 3071 only - all of the signal passes through the
    boundary tiles of the smallest batch, a dropped or garbled tile is a gross error - and every gradient is compared with the
    3072-ray batch's.  On the emulator value for value.  On the chip value for value for the ray gradients (one owner per ray, no sum
    across launches' partitions: DESIGN.md section 4, test_tracker_backward_is_deterministic_at_scale) and within 1e-4 max|g| - the
    at-size bound - for the feature rows (one float atomic per point and table, DESIGN.md section 3 k_feat_gather) and the decoder
    gradients (partial tiles whose partition follows the launch's size).
    Only the 'geometry' mapper cases run on the emulator, where one batch (forward and backward) takes 5 - 7 s - a case is one batch,
    the 3072-ray one is computed once per parameter set and kept; a colour-stage batch takes the emulator 20 - 45 s."""
    eng = make_engine(backend)
    sc = _render_scene(eng, backend)
    key = (backend, rel_pos, stage, tracker)
    if key not in _RENDER_BASE:
        _RENDER_BASE[key] = _render_run(eng, sc, rel_pos, stage, tracker, R_SHARED)
    base = _RENDER_BASE[key]
    grad_names = ('g_rays_o', 'g_rays_d') if tracker else ('g_geo', 'g_weights') + (('g_col',) if stage == 'color' else ())
    if R == R_SHARED:
        assert 0.9 < float(base['valid_ray'].float().mean()) < 1.0 and bool(base['valid_ray'][SIGNAL].any())
        for k in grad_names:
            assert bool(torch.isfinite(base[k]).all()) and float(base[k].abs().max()) > 0, f'{k}: no signal'
        if not tracker and stage == 'geometry':
            assert not bool(base['g_col'].any())
        return
    run = _render_run(eng, sc, rel_pos, stage, tracker, R)
    for k in FWD_NAMES:
        if k == 'c_col' and not (stage == 'color' and not rel_pos):
            continue
        assert torch.equal(bits(run[k]), bits(base[k])), f'{k} of the shared rays differs between {R_SHARED} and {R} rays'
    for k in grad_names + (() if tracker or stage == 'color' else ('g_col',)):
        a, b = run[k], base[k]
        scale = float(b.abs().max())
        diff = float((a - b).abs().max())
        print(f'{k} R={R}: max|g| {scale:.3e}, max difference to the {R_SHARED}-ray batch {diff:.3e}')
        if backend == 'emu' or tracker:
            assert torch.equal(a, b), f'{k} differs between {R_SHARED} and {R} rays by {diff:.3e} (max|g| {scale:.3e})'
        else:
            assert diff <= 1e-4 * scale, f'{k} differs between {R_SHARED} and {R} rays by {diff:.3e} (max|g| {scale:.3e})'


# ---------------------------------------------------------------------------- G. loop-level switches (chip only)
R_LOOKAHEAD = sw.rays_at(sw.LOOKAHEAD_T16_MAX_P)           # 13107: 65 535 samples, modes 1 and 2 at 16 lanes, k_interp_repack<16>
MAP_LOOP_R = (sw.MASK_REG_MAX, sw.MASK_REG_MAX + 1, R_LOOKAHEAD, R_LOOKAHEAD + 1)
TRACK_LOOP_R = (R_EPILOGUE, R_EPILOGUE + 1, R_T16, R_T16 + 1, sw.MASK_REG_MAX, sw.MASK_REG_MAX + 1)


def _loop_frame():
    """Frame 5 of the synthetic room with 2 % holes and, every 211th pixel, a reading of 40 m: beyond 10 x the median, so the inside
    mask takes its radix select and rejects rays."""
    depth, color, c2w = syn.render_frame(5, device='cpu', holes=0.02)
    depth = depth.clone()
    depth.view(-1)[::211] = 40.0
    return depth, color, c2w


@pytest.mark.gpu
@pytest.mark.parametrize('R', MAP_LOOP_R)
def test_map_loop_forms_match_the_statement_path(R):
    """lk_map_frame, TUM model (no rel-pos), one 'geometry' and one 'color' iteration in ONE call against the same two iterations as one
    launch sequence per statement (MapOptimizer.iterate: lk_inside_mask, the in-line search k_sample_interp<*, 0>), through the
    comparison and at the bounds of test_steps_parity.py::test_long_map_call_matches_the_statement_path.  8192 / 8193 rays: the batch
    assembly k_pregather<8> / <16>; 13 107 / 13 108 rays: 65 535 / 65 540 samples, the look-ahead search and the interpolation at
    16 / 8 lanes per sample, k_interp_repack<16> / <8>.  Neighbour lists of both iterations and the masked-ray counts exactly: the
    native batch puts the rays its own inside-mask threshold keeps first, so its lists equal the statement path's lists of the rays
    that the NumPy reference of lk_inside_mask keeps only if that threshold keeps the same rays (the loop holds the threshold in its
    work buffer, which has no read-back); lk_inside_mask's own threshold on these depths against the reference bit for bit.
    Chip only: both loops over up to 65 000 samples take the emulator minutes."""
    eng = make_engine('hip')
    sc = _render_scene(eng, 'hip')
    W = syn.default_weights(rel_pos=False)
    depth, color, c2w = _loop_frame()
    Hh, Ww = depth.shape
    intr = tuple(syn.TUM_INTR[k] for k in ('fx', 'fy', 'cx', 'cy'))
    iters, n_geo = 2, 1
    rnd_cpu = torch.randint(0, Hh * Ww, (iters, R), generator=torch.Generator().manual_seed(R), dtype=torch.int32)
    rnd_all = rnd_cpu.to(eng.device)
    N = sc['pos'].shape[0]
    rows = torch.arange(0, N, 2, dtype=torch.int32).to(eng.device)
    lrs = {'geometry': (1e-4, 1e-3, 0.0), 'color': (2e-4, 2e-4, 2e-4)}
    frames = (eng.f32(depth).reshape(1, Hh, Ww), eng.f32(color).reshape(1, Hh, Ww, 3), eng.f32(c2w).reshape(1, 4, 4), None)
    fid = torch.zeros(R, dtype=torch.int32, device=eng.device)
    win = (0, Hh, 0, Ww)
    # what lk_inside_mask must answer on these draws
    ref = [sw.inside_mask_ref(depth.reshape(-1)[rnd_cpu[it].long()].numpy()) for it in range(iters)]
    for it in range(iters):
        d_it = depth.reshape(-1)[rnd_cpu[it].long()].numpy()
        assert sw.needs_median(d_it) and 0 < int(ref[it][1].sum()) < int((d_it > 0).sum())         # the mask bites
    res = {}
    for native in (True, False):
        cfg = core.RenderCfg(rel_pos=False)
        dec = core.DecoderBlob(eng).pack(W)
        geo_d, col_d = sc['geo'].clone(), sc['col'].clone()
        mo = steps.MapOptimizer(eng, cfg, dec, sc['knn'], sc['pos'], geo_d, col_d, rows, R, lrs, w_color=0.1)
        mo.begin_frame()
        lists, thr = [], []
        if native:
            assert mo._takes_native_loop()
            log = eng.zeros(iters, 4)
            mo.run(iters, n_geo, frames, rnd_all, fid, win, intr, Hh, Ww, log)
            torch.cuda.synchronize()
            lists = [mo.nbr_idx_of(it).clone() for it in range(iters)]
            log = log.cpu().numpy().copy()
        else:
            rows4 = []
            for it in range(iters):
                rows4.append(mo.iterate('geometry' if it < n_geo else 'color', frames, rnd_all[it], fid, win, intr, Hh, Ww).cpu().numpy().copy())
                lists.append(mo.st.nbr_idx.reshape(-1).clone())
                thr.append(mo.batch.thr.cpu().numpy().copy())
            log = np.stack(rows4)
        res[native] = (log, lists, thr, geo_d.cpu(), col_d.cpu(), {k: v.clone() for k, v in dec.unpack().items()})
    (la, lists_a, _, geo_a, col_a, W_a), (lb, lists_b, thr_b, geo_b, col_b, W_b) = res[True], res[False]
    for it in range(iters):
        assert thr_b[it].view(np.int32)[0] == ref[it][0].view(np.int32), f'iteration {it}: lk_inside_mask thr {thr_b[it]} != {ref[it][0]}'
        # the native batch is partitioned (k_pregather): the rays the inside mask keeps come first, in draw order
        keep = torch.from_numpy(ref[it][1]).to(eng.device)
        n_keep = int(keep.sum())
        mine, theirs = lists_a[it].reshape(R, -1)[:n_keep], lists_b[it].reshape(R, -1)[keep]
        assert torch.equal(mine, theirs), f'iteration {it}: neighbour lists of the {n_keep} kept rays differ'
        assert float((theirs >= 0).any(1).float().mean()) > 0.9
    assert np.array_equal(la[:, 3], lb[:, 3]) and 0 < la[0, 3] < R, (la[:, 3], lb[:, 3])
    print(f'map loop R={R}: losses native {la[:, 0]}, per statement {lb[:, 0]}')
    assert np.isfinite(la).all()
    np.testing.assert_allclose(la[:, 0], lb[:, 0], rtol=2e-3)
    for a, b, start in ((geo_a, geo_b, sc['geo']), (col_a, col_b, sc['col'])):
        err = (a - b).abs()
        assert float(torch.quantile(err.reshape(-1), 0.999)) < 2e-4 and float(err.max()) < 0.02, float(err.max())
        assert float((a - start.cpu()).abs().max()) > 1e-5                                       # the rows did move
    for n, w in W_a.items():
        assert float((w - W_b[n]).abs().max()) <= 2e-3 * max(1.0, float(w.abs().max())), n


@pytest.mark.gpu
@pytest.mark.parametrize('R', TRACK_LOOP_R)
def test_track_loop_forms_match_the_statement_path(R):
    """lk_track_frame (Replica model) against the per-statement path on both sides of every size switch of the tracking loop:
      3072 / 3073 rays  the loss epilogue inside the decoder forward while cdiv(P, 30) <= 512 tiles (lk_decode.hip), a launch of its own above;
      3276 / 3277 rays  512 / 513 tiles of 32 samples: fuse_small with the fused rel-pos + decode forward and k_relpos_interp_bwd, the deep
                        and the plain k_decode_bwd with the loss prologue, the search at 16 / 8 lanes per sample (16 380 / 16 385 samples);
      8192 / 8193 rays  batch assembly, inside mask and rays in one fused workgroup with the values in registers, or the unfused sequence
                        (lk_gather_rays, lk_inside_mask from scratch memory).
    Two stiff iterations (rate / 200, test_loops_at_size.py: rounding is not amplified) at that file's bounds - losses 5e-5 where both
    sides mask the same number of rays (stiff_call_ok), the chosen pose within 5 % of one step.  Chip only, like that file."""
    from test_loops_at_size import stiff_call_ok
    eng = make_engine('hip')
    sc = _render_scene(eng, 'hip')
    W = syn.default_weights(rel_pos=True)
    depth, color, c2w = _loop_frame()
    Hh, Ww = depth.shape
    intr = tuple(syn.TUM_INTR[k] for k in ('fx', 'fy', 'cx', 'cy'))
    iters, lr = 2, 0.002 / 200.0
    win = (20, Hh - 20, 20, Ww - 20)
    rnd_all = torch.randint(0, (win[1] - win[0]) * (win[3] - win[2]), (iters, R), generator=torch.Generator().manual_seed(R + 1), dtype=torch.int32).to(eng.device)
    cam0 = eng.f32(H.c2w_to_cam(c2w) + torch.tensor([0.0, 0.002, -0.001, 0.0015, 0.004, -0.003, 0.002]))
    res = {}
    for native in (True, False):
        cfg = core.RenderCfg(rel_pos=True)
        dec = core.DecoderBlob(eng).pack(W)
        to = steps.TrackOptimizer(eng, cfg, dec, sc['knn'], sc['pos'], sc['geo'], sc['col'], R, lr, separate_lr=True, w_color=0.5)
        to.native_loop = native
        best, log = to.track(cam0, eng.f32(depth), eng.f32(color), iters, win, intr, rnd_all)
        torch.cuda.synchronize()
        res[native] = (best.cpu().double(), log.cpu().numpy().astype(np.float64))
    (best_a, la), (best_b, lb) = res[True], res[False]
    print(f'track loop R={R}: native {la.tolist()}, per statement {lb.tolist()}')
    assert np.isfinite(la).all() and 0 < la[0, 3] < R
    rel = np.abs(la[:, 0] - lb[:, 0]) / np.abs(lb[:, 0])
    dm = np.abs(la[:, 3] - lb[:, 3])
    assert stiff_call_ok(rel, dm, R, 5e-5), (rel.tolist(), dm.tolist())
    perr = float((H.quat_to_c2w(best_a) - H.quat_to_c2w(best_b)).abs().max())
    assert perr <= 0.05 * lr * iters + 1e-7, perr
