"""The integer selection machinery of csrc/lk_scan_dev.h (wave scan, ballot rank, histogram add, bin of a rank, 4-pass radix select, carry
scan) at the shapes the other test files do not reach: the second pass of the carry scan behind the index build, the tracker's median
mask at every wave / workgroup / form boundary, and the pixel pool with ties that are ranked in pixel order only.  Everything here is
integer arithmetic on bit patterns, so every comparison is exact; both back-ends (see test_forward_parity.py).  The compactions are
covered at every switch by test_size_switches.py (B)."""
import numpy as np
import pytest
import torch

from loopy_slam_amd import core, optim
from oracle import hotpath as H
from util import make_engine, backends
import switch_referee as sw


# ---------------------------------------------------------------------------- index build: k_scan_block and the carry scan
# cell counts + 1 (the scanned length): one entry, around one k_scan_block block (1024), two blocks and a bit; then around 256 block sums x
# 1024 items = 262 144, where k_carry_scan<256, ..> takes a second pass with the carry of the first
SCAN_TOTALS = (2, 1023, 1024, 1025, 2049, 262143, 262144, 262145, 263169)


@pytest.mark.parametrize('total', SCAN_TOTALS)
@pytest.mark.parametrize('backend', backends())
def test_index_build_scan(backend, total):
    """A 1-D cloud along x with cell_size 1 and points at k + 0.5: k_grid_finalize gives it exactly (largest k) + 1 cells (origin = the
    smallest coordinate, dx = floor((max - min) / cell) + 1, dy = dz = 1), cell k holds the points at k + 0.5.  Points - some of them two or
    three times - in the first cell, the last cell and about every 1000th in between: a wrong offset anywhere moves the range of every
    later cell.  Every point is queried with a radius below the cell size and compared with the exact search bit for bit."""
    eng = make_engine(backend)
    ncells = total - 1
    ks = sorted({0, ncells - 1, *range(997, ncells - 1, 997)})
    rng = np.random.default_rng(total)
    reps = rng.integers(1, 4, len(ks))
    reps[0] = reps[-1] = 2
    x = np.repeat(np.asarray(ks, dtype=np.float64) + 0.5, reps)
    pos = np.zeros((x.size, 3), dtype=np.float32)
    pos[:, 0] = x
    pos = pos[rng.permutation(x.size)]                                       # the index of a point says nothing about its cell
    assert np.array_equal(np.floor(pos[:, 0] - pos[:, 0].min()).max() + 1, ncells)
    knn = core.KnnIndex(eng, capacity=pos.shape[0], cell_size=1.0, max_cells=ncells)
    knn.build(eng.f32(torch.from_numpy(pos)))
    r2 = float(np.float32(0.81))
    od, oi, oc = H.knn_exact(pos, pos, 8, np.float32(r2))
    assert oc.min() >= 1 and oc.max() <= 3 and (ncells < 3 or oc.max() > 1)  # every point finds itself and its duplicates, nothing else
    d2, idx, cnt = knn.query(eng.f32(torch.from_numpy(pos)), r2)
    assert np.array_equal(idx.cpu().numpy(), oi)
    assert np.array_equal(d2.cpu().numpy().view(np.int32), od.view(np.int32))
    assert np.array_equal(cnt.cpu().numpy(), oc)


# ---------------------------------------------------------------------------- the tracker's median mask (lk_block_median10)
MEDIAN_SIZES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 16384, 16385)
# the patterns of switch_referee.depth_pattern that make sense for a residual |gt - depth|; outlier, lowbyte and inf come with absent rays
# (a tenth of the batch) mixed in
MEDIAN_PATTERNS = ('equal', 'two', 'lowbyte', 'subnormal', 'inf', 'outlier')


class _State:
    pass


def _median_case(eng, resid, nan_at=None):
    """lk_loss_tracker with handle_dynamic off on rays whose residual |gt - depth| is `resid` exactly (depth 0, gt = resid; resid 0: an
    absent ray): (masked-ray count, mask [R] read off d depth, the threshold where the launch stores it)."""
    R = resid.shape[0]
    depth = np.zeros(R, dtype=np.float32)
    if nan_at is not None:
        depth[nan_at] = np.nan
    st = _State()
    st.depth, st.var, st.color = eng.f32(torch.from_numpy(depth)), eng.f32(torch.ones(R)), eng.zeros(R, 3)
    dd, dc, out, scr = eng.empty(R), eng.empty(R, 3), eng.empty(4), eng.empty(R + 8)
    optim.loss_tracker(eng, st, eng.f32(torch.from_numpy(resid)), eng.zeros(R, 3), 0.5, True, dd, dc, out, scr, handle_dynamic=False)
    # d depth = sgn(depth - gt) / sqrt(var) = -1 for a masked ray (every residual here is at most 1e3, the clamp of the loss term)
    thr = scr.cpu().numpy()[R:R + 1].view(np.uint32)[0] if R > 16384 else None        # the three-launch form leaves it in scratch[R]
    return float(out.cpu()[3]), dd.cpu().numpy() != 0, thr


@pytest.mark.parametrize('R', MEDIAN_SIZES)
@pytest.mark.parametrize('backend', backends())
def test_median_mask(backend, R):
    """mask = present and |gt - depth| < fl(10 x the LOWER median of the present rays' residuals) in float32: the count exactly, the mask
    itself, and the stored threshold bit for bit (only the three-launch form, R > 16 384, stores it; the one-workgroup form keeps it in a
    register).  One NaN empties the mask."""
    eng = make_engine(backend)
    for pat in MEDIAN_PATTERNS:
        resid = sw.depth_pattern(pat, R, 77 * R + len(pat))
        present = resid > 0
        cnt, mask, thr = _median_case(eng, resid)
        if not present.any():
            assert cnt == 0 and not mask.any(), pat
            continue
        srt = np.sort(resid[present])
        ref_thr = np.float32(10.0) * srt[(srt.size - 1) // 2]
        ref_mask = present & (resid < ref_thr)
        assert cnt == int(ref_mask.sum()), (pat, cnt, int(ref_mask.sum()))
        assert np.array_equal(mask, ref_mask), pat
        if thr is not None:
            assert thr == ref_thr.view(np.uint32), (pat, hex(thr), ref_thr)
    # the lower median decides: with 1.0 and 30.0 in equal numbers the upper one would keep everything
    if R >= 2 and R % 2 == 0:
        resid = sw.depth_pattern('two', R, R)
        assert _median_case(eng, resid)[0] == R // 2
    resid = sw.depth_pattern('outlier', R, R + 1)
    if (resid > 0).any():
        cnt, mask, thr = _median_case(eng, resid, nan_at=int(np.nonzero(resid > 0)[0][-1]))
        assert cnt == 0 and not mask.any()
        assert thr is None or thr == 0x7fc00000


# ---------------------------------------------------------------------------- the high-gradient pixel pool
# 128 x 128 = 16 384 pixels is the last one-workgroup size, 129 x 128 the first many-workgroup one (slices of 256 pixels); 97 x 131 and
# 129 x 128 are no multiples of 256
POOL_SIZES = ((1, 1), (1, 65), (97, 131), (128, 128), (129, 128))
POOL_IMAGES = ('constant', 'lowbyte', 'quantised')


def _pool_image(name, n, seed):
    rng = np.random.default_rng(seed)
    if name == 'constant':                                       # every pixel ties: the cut is pixel order alone
        return np.full(n, 0.125, dtype=np.float32)
    if name == 'lowbyte':                                        # the select is decided in its last pass
        g = (1.0 + (np.arange(n) % 200).astype(np.float64) * 2.0 ** -23).astype(np.float32)
        rng.shuffle(g)
        return g
    return (rng.integers(0, 4, n) / 4.0).astype(np.float32)      # four levels: the ties at any cut lie all over the image


@pytest.mark.parametrize('size', POOL_SIZES)
@pytest.mark.parametrize('backend', backends())
def test_top_grad_pool(backend, size):
    """K in {1, n / 2, n - 1, n} of every image against the oracle, whole window, no depth filter: the pool is the selection itself."""
    eng = make_engine(backend)
    Hh, Ww = size
    n = Hh * Ww
    for name in POOL_IMAGES:
        g = _pool_image(name, n, n + len(name)).reshape(Hh, Ww)
        if name == 'quantised' and n > 16384:
            # the ties at the n / 2 cut span slice boundaries of the many-workgroup form, and the cut falls inside them
            kth = np.sort(g.reshape(-1))[n - n // 2]
            ties = np.nonzero(g.reshape(-1) == kth)[0]
            assert np.unique(ties // 256).size > 8 and 0 < n // 2 - int((g > kth).sum()) < ties.size
        ge = eng.f32(torch.from_numpy(g))
        for K in sorted({1, n // 2, n - 1, n}):
            ref = H.top_grad_pixels(g, K, (0, Hh, 0, Ww), None, False)
            got = optim.top_grad_pixels(eng, ge, K, (0, Hh, 0, Ww), None, False)
            assert np.array_equal(got.cpu().numpy(), ref), (name, K, got.shape, ref.shape)
            assert ref.shape[0] == K
