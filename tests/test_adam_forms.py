"""lk_adam_step in every addressing form (dense, row_index, row_index + g_compact, row_flags, each with p_f16 and zero_grad, up to 16
segments per launch) against Adam in float64, and lk_touch_rows against numpy (both back-ends, see test_forward_parity.py).

The reference is torch.optim.Adam's arithmetic (amsgrad=False, weight_decay=0) written out in float64 on the values that cross the ABI:
beta1, beta2, eps and lr are C floats, so the reference takes their float32 values.  In the row forms its parameters are clones of the
selected / flagged rows.  Every buffer the kernel is handed sits between guard elements, rows that are not stepped carry non-zero
gradients (and non-zero garbage where the flag form has their moments), and whatever must not move is compared bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from loopy_slam_amd import _ffi
from loopy_slam_amd._ffi import ptr
from util import make_engine, backends

B1, B2, EPS = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8))
GUARD = 64                 # elements before and after every buffer
G_LO, G_HI = 1e-12, 1e3    # gradient magnitudes: log-uniform in between, plus exact zeros (g * g stays finite in fp32)
# m and v of the stepped elements against the float64 reference, relative to the size of the terms they are summed from (for v that is v
# itself; for m the same recurrence over |g|, so a cancelling sum is not held to the size of its result).  Measured on the host emulator
# over all cases of this module: worst m 2.364e-7, worst v 2.868e-7 (printed when the module is done: pytest -s).  Bounds: 8 x that, rounded
# up to one digit (1.89e-6 -> 2e-6, 2.29e-6 -> 3e-6) - the margin is for FMA contraction on the chip.
MV_RTOL = {'m': 2e-6, 'v': 3e-6}
_WORST = {'m': 0.0, 'v': 0.0}
_BITS = {torch.float32: torch.int32, torch.float16: torch.int16}


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    print(f'\ntest_adam_forms: worst deviation of m {_WORST["m"]:.3e}, of v {_WORST["v"]:.3e} (bounds {MV_RTOL["m"]:.0e}, {MV_RTOL["v"]:.0e})')


def bits(t):
    return t.view(_BITS[t.dtype]) if t.dtype in _BITS else t


def rows_per_wave(n_rows, row_len, nmax=None):
    """RW of lk_adam_seg_flagged for a [n_rows, row_len] segment in a launch whose largest segment has nmax elements."""
    gx = min(2048, max(1, -(-(nmax or n_rows * row_len) // 256)))
    rw = 64
    while rw > 2 and n_rows < gx * 4 * rw:
        rw >>= 1
    return rw


def rand_grad(shape, gen, dev):
    u = torch.rand(shape, generator=gen, device=dev)
    mag = torch.exp(u * (math.log(G_HI) - math.log(G_LO)) + math.log(G_LO))
    s = torch.rand(shape, generator=gen, device=dev)
    return torch.where(s > 0.9, torch.zeros_like(mag), torch.where(s < 0.45, mag, -mag))


class Buf:
    """`n` elements the kernel is given, between GUARD elements it is not."""

    def __init__(self, eng, n, dtype):
        self.n = n
        self.full = torch.full((n + 2 * GUARD,), 77, dtype=dtype, device=eng.device)
        self.body = self.full[GUARD:GUARD + n]

    def rows(self, row_len, full=None):
        return (self.full if full is None else full)[GUARD:GUARD + self.n].view(self.n // row_len, row_len)

    def assert_only_rows_changed(self, snap, row_len, sel, what):
        """Everything but the rows `sel` of the [*, row_len] body, guards included, has the bytes of `snap`."""
        tmp = self.full.clone()
        if sel is not None and sel.numel():
            self.rows(row_len, tmp)[sel] = self.rows(row_len, snap)[sel]
        assert torch.equal(bits(tmp), bits(snap)), f'{what}: an element outside the stepped rows (or a guard) changed'


class Seg:
    """One lk_adam_seg with its buffers and its float64 reference.
    form 'dense': n elements (n_rows = 1, row_len = n);  'index': rows `sel` (in list order) of a [n_rows, row_len] table;
    'flags': the rows of the table whose byte of `flags` is non-zero.  step0 > 1: the moments start from random values."""

    def __init__(self, eng, gen, form, n_rows, row_len, sel=None, flags=None, f16=False, g_compact=False, lr=0.005, step0=1):
        dev = eng.device
        self.eng, self.gen, self.form, self.L, self.f16, self.compact = eng, gen, form, row_len, f16, g_compact
        self.lr, self.step0 = float(np.float32(lr)), step0
        if form == 'dense':
            assert n_rows == 1
            self.sel = torch.zeros(1, dtype=torch.long, device=dev)
        elif form == 'index':
            self.sel = torch.as_tensor(sel, dtype=torch.long).to(dev)
            self.idx = Buf(eng, self.sel.numel(), torch.int32)
            self.idx.body.copy_(self.sel.to(torch.int32))
        else:
            self.flg = Buf(eng, n_rows, torch.uint8)
            self.flg.body.copy_(torch.as_tensor(flags, dtype=torch.uint8).to(dev))
            self.sel = torch.nonzero(self.flg.body).reshape(-1)
        ns = self.ns = self.sel.numel()
        every = torch.arange(ns, device=dev)
        n_tab = n_rows * row_len
        self.p = Buf(eng, n_tab, torch.float16 if f16 else torch.float32)
        p0 = 0.1 * torch.randn(n_tab, generator=gen, device=dev)
        if f16:
            # The half measure in check() holds a TRAJECTORY to the spacing at its last value.  Where the fp32 and the float64 step fall on
            # either side of a rounding boundary (about 1e-4 of the element-steps) the two differ by one spacing from then on, and that
            # spacing counts for more where |p| has shrunk since: with 0.1 * randn, 524 291 elements and three steps of 0.005 a few end up
            # near zero, 2 to 7 of their spacings from the reference, on the emulator as on the chip.  Adam moves an element by at most
            # about lr a step (the moments start at zero or with v >= m^2), 0.015 in all, so from |p| >= 0.06 the magnitude keeps three
            # quarters of itself and a carried spacing stays below 1.34.
            p0 = torch.where(p0 < 0, -1.0, 1.0) * (0.06 + 0.19 * torch.rand(n_tab, generator=gen, device=dev))
        self.p.body.copy_(p0)
        self.g = Buf(eng, ns * row_len if g_compact else n_tab, torch.float32)
        self.g.body.copy_(torch.rand(self.g.n, generator=gen, device=dev) + 0.5)       # rows that are not stepped: never zero
        self.g_sel = every if g_compact else self.sel
        self.m, self.v = (Buf(eng, n_tab if form == 'flags' else ns * row_len, torch.float32) for _ in range(2))
        self.mv_sel = self.sel if form == 'flags' else every
        for b in (self.m, self.v):
            b.body.fill_(0.25)                                                          # (flag form: moments of rows without a flag)
            b.rows(row_len)[self.mv_sel] = 0.0
        self.zero_init = step0 == 1
        if not self.zero_init:
            self.m.rows(row_len)[self.mv_sel] = 1e-3 * torch.randn(ns, row_len, generator=gen, device=dev)
            m0 = self.m.rows(row_len)[self.mv_sel]
            self.v.rows(row_len)[self.mv_sel] = m0 * m0 + 1e-6 * torch.rand(ns, row_len, generator=gen, device=dev)
        # elements whose gradient is zero in every step: with zero moments Adam leaves them bit for bit where they are
        self.zmask = torch.rand(ns, row_len, generator=gen, device=dev) < 0.1
        if ns:
            self.zmask[0, 0] = False
        self.P = self.p.rows(row_len)[self.sel].cpu().double()
        self.M = self.m.rows(row_len)[self.mv_sel].cpu().double()
        self.V = self.v.rows(row_len)[self.mv_sel].cpu().double()
        self.AM = self.M.abs()
        self.bufs = [('p', self.p), ('g', self.g), ('m', self.m), ('v', self.v)]
        self.bufs += [('row_index', self.idx)] if form == 'index' else [('row_flags', self.flg)] if form == 'flags' else []

    @property
    def n(self):
        return self.ns * self.L

    def fill(self, a, k, zero_grad):
        a.p, a.g, a.m, a.v = ptr(self.p.body), ptr(self.g.body), ptr(self.m.body), ptr(self.v.body)
        a.n, a.lr, a.step = (self.p.n if self.form == 'flags' else self.n), self.lr, self.step0 + k
        a.row_index = ptr(self.idx.body) if self.form == 'index' else None
        a.row_flags = ptr(self.flg.body) if self.form == 'flags' else None
        a.row_len = 1 if self.form == 'dense' else self.L
        a.zero_grad, a.p_f16, a.g_compact = int(zero_grad), int(self.f16), int(self.compact)

    def prepare(self, k):
        """Fresh gradients in the stepped rows; the second step leaves every other stepped row (half of a single row) without any."""
        gs = rand_grad((self.ns, self.L), self.gen, self.eng.device)
        gs[self.zmask] = 0.0
        if k == 1:
            if self.ns > 1:
                gs[0::2] = 0.0
            else:
                gs[:, :(self.L + 1) // 2] = 0.0
        self.g.rows(self.L)[self.g_sel] = gs
        self.Gd = gs.cpu().double()
        self.snap = {name: b.full.clone() for name, b in self.bufs}

    def check(self, k, zero_grad, what):
        L, step = self.L, self.step0 + k
        clears = bool(zero_grad) and not self.compact
        may_change = {'p': self.sel if self.lr != 0.0 else None, 'g': self.g_sel if clears else None, 'm': self.mv_sel, 'v': self.mv_sel}
        for name, b in self.bufs:
            b.assert_only_rows_changed(self.snap[name], L, may_change.get(name), f'{what} step {step} {name}')
        if clears:
            assert not bool(bits(self.g.rows(L)[self.g_sel]).any()), f'{what} step {step}: zero_grad left a consumed gradient'
        # float64 Adam over the stepped rows
        G = self.Gd
        self.M = B1 * self.M + (1.0 - B1) * G
        self.AM = B1 * self.AM + (1.0 - B1) * G.abs()
        self.V = B2 * self.V + (1.0 - B2) * G * G
        denom = self.V.sqrt() / math.sqrt(1.0 - B2 ** step) + EPS
        self.P = self.P - (self.lr / (1.0 - B1 ** step)) * (self.M / denom)
        if self.f16:
            self.P = self.P.to(torch.float16).double()
        for name, b, ref, scale in (('m', self.m, self.M, self.AM), ('v', self.v, self.V, self.V)):
            d = (b.rows(L)[self.mv_sel].cpu().double() - ref).abs()
            if bool((scale > 0).any()):
                _WORST[name] = max(_WORST[name], float((d[scale > 0] / scale[scale > 0]).max()))
            # MV_RTOL: 8 x the emulator's worst deviation (2.364e-7 for m, 2.868e-7 for v), rounded up to one digit: 2e-6 and 3e-6
            assert bool((d <= MV_RTOL[name] * scale).all()), f'{what} step {step}: {name} off by {float((d / scale.clamp_min(1e-300)).max()):.3e} of its terms'
        got = self.p.rows(L)[self.sel]
        if self.zero_init and self.ns:
            z = self.zmask
            before = self.p.rows(L, self.snap['p'])[self.sel]
            assert torch.equal(bits(got)[z], bits(before)[z]), f'{what} step {step}: p moved without gradient or moments'
            assert not bool(bits(self.m.rows(L)[self.mv_sel])[z].any()) and not bool(bits(self.v.rows(L)[self.mv_sel])[z].any())
        got = got.cpu().double()
        if self.f16:            # the measure of test_feats_f16.py::test_adam_on_half_rows
            d = (got - self.P).abs()
            ulp = self.P.abs().clamp_min(2.0 ** -14) * 2.0 ** -10
            if d.numel():
                frac, worst = float((d <= ulp).double().mean()), float((d / ulp).max())
                assert frac > 0.999 and worst <= 2.0, f'{what} step {step}: {1 - frac:.2e} of p beyond one half spacing, worst {worst:.2f}'
        elif self.lr != 0.0:
            np.testing.assert_allclose(got.numpy(), self.P.numpy(), rtol=3e-6, atol=1e-7, err_msg=f'{what} step {step}: p')


class NullSeg:
    """n = 0 with NULL pointers."""
    n = 0

    def fill(self, a, k, zero_grad):
        a.n, a.lr, a.step, a.row_len = 0, 0.001, 1 + k, 1

    def prepare(self, k):
        pass

    def check(self, k, zero_grad, what):
        pass


def seg_array(segs, k, zero_grad):
    arr = (_ffi.AdamSeg * max(1, len(segs)))()
    for i, s in enumerate(segs):
        s.fill(arr[i], k, zero_grad[i] if isinstance(zero_grad, (list, tuple)) else zero_grad)
    return arr


def adam_step(eng, arr, n_seg):
    return eng.lib.dll.lk_adam_step(arr, n_seg, C.c_float(0.9), C.c_float(0.999), C.c_float(1e-8), eng.stream)


def run_steps(eng, segs, what, zero_grads=(1, 0, 1)):
    """Three consecutive steps of one launch each; zero_grad on in the first and third."""
    for k, zg in enumerate(zero_grads):
        for s in segs:
            s.prepare(k)
        eng.lib.check(adam_step(eng, seg_array(segs, k, zg), len(segs)), 'lk_adam_step')
        for i, s in enumerate(segs):
            s.check(k, zg, f'{what} seg {i}')


def gens(eng, seed):
    return torch.Generator(device=eng.device).manual_seed(seed)


# ---------------------------------------------------------------------------- flagged rows
def flag_pattern(name, n_rows, row_len, gen):
    """Flag bytes of a [n_rows, row_len] table (torch generator on the CPU: the same flags on both back-ends)."""
    f = torch.zeros(n_rows, dtype=torch.uint8)
    rw = rows_per_wave(n_rows, row_len)
    if name == 'all':
        f[:] = 1
    elif name.startswith('single'):
        f[{'single0': 0, 'single63': 63, 'single64': 64, 'single_last': n_rows - 1}[name]] = 1
    elif name == 'odd':
        # an odd number of flags inside one group of RW rows (the last pair of the wave's walk has one row): in the first group, in one
        # in the middle and in the last, partial one - three where the group has room, else one
        for g0 in sorted({0, (n_rows // 2) // rw * rw, (n_rows - 1) // rw * rw}):
            room = min(rw, n_rows - g0)
            f[g0 + torch.randperm(room, generator=gen)[:3 if room >= 3 else 1]] = 1
    elif name in ('r05', 'r30', 'bytes'):
        f[torch.rand(n_rows, generator=gen) < (0.05 if name == 'r05' else 0.3)] = 1
        if name == 'bytes':
            f *= torch.tensor([1, 2, 7, 255], dtype=torch.uint8)[torch.randint(0, 4, (n_rows,), generator=gen)]
    else:
        assert name == 'none'
    return f


def flag_cases(shapes):
    out = []
    for n_rows, row_len in shapes:
        for pat in ('none', 'all', 'single0', 'single63', 'single64', 'single_last', 'odd', 'r05', 'r30', 'bytes'):
            if pat == 'all' and n_rows > 32771:                     # dense flags on a large table: only a longer run of the same walk
                continue
            if (pat == 'single63' and n_rows <= 63) or (pat == 'single64' and n_rows <= 64):
                continue
            if pat == 'single_last' and n_rows - 1 in (0, 63, 64):
                continue
            out.append(pytest.param(n_rows, row_len, pat, id=f'{n_rows}x{row_len}-{pat}'))
    return out


# rows per wave and pass the shapes below are meant to reach (row_len 32: 2 up to 1000 rows, then 4, 16 and 64 with a 37-row second trip)
EXPECTED_RW = {(1, 32): 2, (2, 32): 2, (3, 32): 2, (63, 32): 2, (64, 32): 2, (65, 32): 2, (1000, 32): 2, (32771, 32): 4, (131077, 32): 16,
               (524325, 32): 64, (524293, 1): 64, (1000, 1): 32, (1000, 7): 8, (1000, 33): 2, (1000, 64): 2}


def test_shapes_reach_every_rows_per_wave_count():
    for (n_rows, row_len), rw in EXPECTED_RW.items():
        assert rows_per_wave(n_rows, row_len) == rw, (n_rows, row_len)
    assert 524325 - 2048 * 4 * 64 == 37 and 32771 > 2048 * 4 * 4 and 131077 > 2048 * 4 * 16       # tails taken by a second trip


@pytest.mark.parametrize('n_rows,row_len,pattern', flag_cases(EXPECTED_RW))
@pytest.mark.parametrize('backend', backends())
def test_flagged_rows(backend, n_rows, row_len, pattern):
    """row_len 32: two rows per wave and walk step.  1: one lane per row; 7: less than a half-wave; 33 and 64: one row per wave, partial
    and full."""
    eng = make_engine(backend)
    flags = flag_pattern(pattern, n_rows, row_len, torch.Generator().manual_seed(n_rows + row_len))
    run_steps(eng, [Seg(eng, gens(eng, 1), 'flags', n_rows, row_len, flags=flags)], f'flags {pattern} [{n_rows},{row_len}]')


@pytest.mark.parametrize('n_rows,row_len', ((65, 32), (1000, 32), (1000, 7), (1000, 33)))
@pytest.mark.parametrize('pattern', ('all', 'odd', 'bytes'))
@pytest.mark.parametrize('backend', backends())
def test_flagged_rows_half(backend, pattern, n_rows, row_len):
    eng = make_engine(backend)
    flags = flag_pattern(pattern, n_rows, row_len, torch.Generator().manual_seed(7 + n_rows))
    run_steps(eng, [Seg(eng, gens(eng, 3), 'flags', n_rows, row_len, flags=flags, f16=True)], f'half flags {pattern} [{n_rows},{row_len}]')


# ---------------------------------------------------------------------------- row index
def index_rows(kind, n_tab):
    g = torch.Generator().manual_seed(n_tab)
    if kind == 'one':
        return torch.tensor([n_tab - 2])
    rows = torch.randperm(n_tab, generator=g)[:77]             # 77 rows: no multiple of 8, so the 256-thread blocks straddle rows
    return rows.sort().values if kind == 'ascending' else rows


@pytest.mark.parametrize('row_len', (32, 5))
@pytest.mark.parametrize('kind', ('ascending', 'permuted', 'one'))
@pytest.mark.parametrize('g_compact', (False, True), ids=('g_table', 'g_compact'))
@pytest.mark.parametrize('f16', (False, True), ids=('f32', 'f16'))
@pytest.mark.parametrize('backend', backends())
def test_row_index(backend, f16, g_compact, kind, row_len):
    """Under g_compact the gradient rows are compact in row-list order and zero_grad is ignored; without it zero_grad clears the rows of
    the index in the table and no others."""
    eng = make_engine(backend)
    seg = Seg(eng, gens(eng, 4), 'index', 300, row_len, sel=index_rows(kind, 300), f16=f16, g_compact=g_compact)
    run_steps(eng, [seg], f'index {kind} row_len {row_len}')


# ---------------------------------------------------------------------------- dense
@pytest.mark.parametrize('n', (1, 255, 256, 257, 524288 + 3))
@pytest.mark.parametrize('f16', (False, True), ids=('f32', 'f16'))
@pytest.mark.parametrize('backend', backends())
def test_dense(backend, f16, n):
    """524 291 elements: above the 2048-block cap, the grid-stride loop runs twice."""
    eng = make_engine(backend)
    run_steps(eng, [Seg(eng, gens(eng, 5), 'dense', 1, n, f16=f16)], f'dense {n}')


# ---------------------------------------------------------------------------- many segments in one launch
@pytest.mark.parametrize('backend', backends())
def test_sixteen_segments_one_launch(backend):
    """The maximum of 16 segments: lengths from 0, every form, fp32 and half, lr 0, steps 1, 2 and 4000.  The dense segment of 600 000
    elements sizes the grid (2048 blocks), so nearly every wave of the 3-row flagged segment beside it is idle."""
    eng = make_engine(backend)
    gen = gens(eng, 6)
    cpu = torch.Generator().manual_seed(6)

    def S(*a, **kw):
        return Seg(eng, gen, *a, **kw)
    segs = [
        NullSeg(),
        S('dense', 1, 1, lr=0.03),
        S('dense', 1, 600000, lr=0.001),
        S('flags', 3, 32, flags=[1, 0, 1], lr=0.005),
        S('index', 100, 32, sel=index_rows('permuted', 100), lr=0.005, step0=2),
        S('index', 100, 32, sel=index_rows('ascending', 100), g_compact=True, lr=0.001, step0=4000),
        S('flags', 1000, 7, flags=flag_pattern('r30', 1000, 7, cpu), lr=0.03, step0=4000),
        S('dense', 1, 300, lr=0.0, step0=2),
        S('dense', 1, 257, f16=True, lr=0.005),
        S('index', 50, 5, sel=index_rows('permuted', 50), f16=True, lr=0.005, step0=2),
        S('flags', 65, 32, flags=flag_pattern('bytes', 65, 32, cpu), f16=True, lr=0.001),
        S('dense', 1, 255, lr=0.005, step0=4000),
        S('flags', 1000, 33, flags=flag_pattern('r05', 1000, 33, cpu), lr=0.0, step0=2),
        S('index', 100, 32, sel=index_rows('one', 100), lr=0.03),
        S('dense', 1, 256, lr=0.001, step0=2),
        S('flags', 64, 64, flags=flag_pattern('none', 64, 64, cpu), lr=0.005),
    ]
    assert len(segs) == _ffi.ADAM_MAX_SEG
    assert rows_per_wave(3, 32, nmax=600000) == 2
    # zero_grad differs between the segments of a launch as well as between the steps
    for k in range(3):
        zg = [(i + k) % 2 for i in range(len(segs))]
        for s in segs:
            s.prepare(k)
        eng.lib.check(adam_step(eng, seg_array(segs, k, zg), len(segs)), 'lk_adam_step')
        for i, s in enumerate(segs):
            s.check(k, zg[i], f'16 segments, seg {i}')


# ---------------------------------------------------------------------------- refusals
def _bad_seventeen(eng, arr):
    big = (_ffi.AdamSeg * 17)()
    for i in range(17):
        big[i] = arr[i % 3]
    return big, 17


def _set(i, **fields):
    def f(eng, arr):
        for k, v in fields.items():
            setattr(arr[i], k, v(arr[i]) if callable(v) else v)
        return arr, 3
    return f


# segments of the valid launch: 0 dense 300, 1 flagged [10, 65 or 32], 2 row_index 7 rows of [20, 32]
REFUSALS = {
    'seventeen_segments': _bad_seventeen,
    'step_zero': _set(0, step=0),
    'negative_n': _set(0, n=-5),
    'null_tensor': _set(0, g=None),
    'flags_with_index': _set(2, row_flags=lambda a: a.p),       # (any non-NULL address: the call is refused before anything reads it)
    'flags_row_len_65': None,
    'flags_n_not_multiple': _set(1, n=10 * 32 - 5),
}


@pytest.mark.parametrize('case', sorted(REFUSALS))
@pytest.mark.parametrize('backend', backends())
def test_refusals(backend, case):
    """Each is an error through LoopyLib.check and leaves every buffer as it was.  (Every segment is backed by whole tables, so that a launch
    that went ahead regardless would stay inside them.)"""
    eng = make_engine(backend)
    gen = gens(eng, 8)
    wide = 65 if case == 'flags_row_len_65' else 32
    segs = [Seg(eng, gen, 'dense', 1, 300), Seg(eng, gen, 'flags', 10, wide, flags=[1, 0] * 5),
            Seg(eng, gen, 'index', 20, 32, sel=[3, 1, 19, 0, 7, 8, 12])]
    for s in segs:
        s.prepare(0)
    arr = seg_array(segs, 0, 1)
    if case != 'flags_row_len_65':
        eng.lib.check(adam_step(eng, arr, 3), 'lk_adam_step')       # the launch is valid until it is broken below
        for s in segs:
            s.check(0, 1, case)
            s.prepare(1)
        arr = seg_array(segs, 1, 1)
        arr, n_seg = REFUSALS[case](eng, arr)
    else:
        n_seg = 3
    rc = adam_step(eng, arr, n_seg)
    assert rc != 0
    with pytest.raises(_ffi.LoopyError):
        eng.lib.check(rc, 'lk_adam_step')
    for s in segs:
        for name, b in s.bufs:
            assert torch.equal(bits(b.full), bits(s.snap[name])), f'{case}: {name} changed'


# ---------------------------------------------------------------------------- lk_touch_rows
@pytest.mark.parametrize('n', (0, 1, 255, 256, 257, 4096 * 256 + 3))
@pytest.mark.parametrize('backend', backends())
def test_touch_rows(backend, n):
    """flags[j] = 1 for every 0 <= nbr_idx[i] = j < N and nothing else: indices of -1, N and N + 5 and duplicates, flags set beforehand stay
    set (the call only ever sets), bytes at and beyond N are untouched.  4096 * 256 + 3 indices: above the grid cap."""
    eng = make_engine(backend)
    N = 1000
    g = torch.Generator().manual_seed(n)
    allowed = torch.cat([torch.randperm(N, generator=g)[:300], torch.tensor([0, N - 1, -1, N, N + 5])])
    idx = allowed[torch.randint(0, allowed.numel(), (n,), generator=g)].to(torch.int32)
    if n == 1:
        idx[0] = N - 1
    if n >= 255:
        idx[:7] = torch.tensor([-1, N, N + 5, 0, 0, N - 1, N - 1], dtype=torch.int32)
        assert int(np.unique(idx.numpy()).size) < n                    # duplicates
    ibuf, fbuf = Buf(eng, n, torch.int32), Buf(eng, N + 8, torch.uint8)     # flags [N], then 8 bytes that index N and N + 5 would hit
    ibuf.body.copy_(idx)
    before = torch.zeros(N + 8, dtype=torch.uint8)
    before[torch.randperm(N, generator=g)[:50]] = 1
    before[N:] = 9
    fbuf.body.copy_(before)
    snap_i = ibuf.full.clone()
    eng.lib.check(eng.lib.dll.lk_touch_rows(ptr(ibuf.body), n, ptr(fbuf.body), N, eng.stream), 'lk_touch_rows')
    ref = np.full(N + 8 + 2 * GUARD, 77, dtype=np.uint8)
    ref[GUARD:GUARD + N + 8] = before.numpy()
    i64 = idx.numpy().astype(np.int64)
    ref[GUARD + i64[(i64 >= 0) & (i64 < N)]] = 1
    assert np.array_equal(fbuf.full.cpu().numpy(), ref)
    assert torch.equal(ibuf.full, snap_i)
    if n >= 255:
        assert 50 < int(ref[GUARD:GUARD + N].sum()) < N                 # some rows touched, some not
