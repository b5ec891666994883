"""Sizes and NumPy / float64 references for tests/test_size_switches.py: every size at which a launcher of loopy_slam_amd/csrc picks
another kernel form, read from the binding where it exposes the constant and written next to the `#define` it mirrors where not.

Test infrastructure only."""
import numpy as np
import torch

from loopy_slam_amd import _ffi

# ---------------------------------------------------------------------------- the switches
MASK_REG_MAX = 8192             # lk_mask_dev.h: #define LK_MASK_REG_MAX 8192 (lk_inside_mask: registers / scratch; k_pregather<8> / <16>)
COMPACT_ONE_BLOCK_MAX = 16384   # lk_kernels.h: #define LK_COMPACT_ONE_BLOCK_MAX 16384 (lk_launch_compact_any: one workgroup up to it, else count / scan / scatter)
COMPACT_PASS = 1024             # k_compact: 1024 elements per pass; k_carry_scan<1024, 1, true>: 1024 block counts per pass (= 262 144 elements)
COMPACT_BLOCK = 256             # k_compact_count / k_compact_scatter: elements per block, one int of block_scratch each
GRID_CAP_ROWS = 4096            # lk_touch_rows / lk_knn_flag_rows: `if (gx > 4096) gx = 4096`, 256 threads: grid-stride above 1 048 576
GRID_CAP_BUCKET = 1024          # lk_bucket_copy: `if (gx > 1024) gx = 1024`, 256 threads: grid-stride above 262 144 floats per segment
KNN_T16_BELOW = 1 << 16         # lk_knn.hip::lk_knn_query: `if (P < (1 << 16))` 16 lanes per query, else 8
T16_MAX_P = 1 << 14             # lk_sample.hip: #define LK_T16_MAX_P (1 << 14): k_sample_interp<16, 0> up to it, <8, 0> above
DEEP_MAX_TILES = 512            # lk_kernels.h: #define LK_DEEP_MAX_TILES 512 and LK_DEEP_MAX_TILES_FWD 512 (32-sample tiles)
TRACK_EPILOGUE_TILE = 30        # lk_api.hip: the tracker's loss epilogue while cdiv(P, 30) <= LK_DEEP_MAX_TILES
LOOKAHEAD_T16_MAX_P = 1 << 16   # lk_sample.hip: `a.P <= (1 << 16)` for k_sample_interp<16, 1> / <16, 2> and k_interp_repack<16>
EXPOSURE_MAX_F = _ffi.EXPOSURE_MAX_F
ADAM_MAX_SEG = _ffi.ADAM_MAX_SEG
S = 5                           # samples per ray of every config (core.RenderCfg.S)
S_MAX = 8                       # include/loopy_hip.h: #define LK_S_MAX 8 (lk_render_fwd accepts 1 <= S <= LK_S_MAX: tests/test_sample_counts.py)


def source_define(file, name):
    """Value of `#define name 8192` / `(1 << 14)` in loopy_slam_amd/csrc/<file> (a path relative to it reaches include/)."""
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.abspath(_ffi.__file__)), 'csrc', file)) as f:
        text = f.read()
    m = re.search(r'^#define\s+' + name + r'\s+\(?\s*(\d+)\s*(?:<<\s*(\d+))?\s*\)?\s*(?://.*|/\*.*\*/\s*)?$', text, re.M)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


def straddle(limit, *more):
    """limit - 1, limit, limit + 1 and whatever else the case wants, ascending."""
    return tuple(sorted({limit - 1, limit, limit + 1, *more}))


def rays_at(samples):
    """Largest ray count whose S samples per ray stay at or below `samples`."""
    return samples // S


# ---------------------------------------------------------------------------- A. lk_inside_mask
MASK_PATTERNS = ('uniform', 'outlier', 'equal', 'two', 'lowbyte', 'subnormal', 'inf', 'nonpos')
_NO_ZEROS = ('equal', 'two', 'subnormal', 'nonpos')


def depth_pattern(name, n, seed):
    """float32 [n].  uniform: [1, 5) - thr = 1.2 max without a median; outlier: the same with one 1000 - radix select; equal; two: 1.0 and
    30.0 in equal numbers (the LOWER median decides at even counts); lowbyte: 1 + k 2^-23, k < 200, and one 100 - the select is decided
    in the lowest byte; subnormal: bit patterns 1..999; inf: one +inf; nonpos: nothing positive.  A tenth of the entries is 0 (absent)
    except in the equal, two, subnormal and nonpos patterns; the single special value is placed after that."""
    rng = np.random.default_rng(seed)
    if name in ('uniform', 'outlier', 'inf'):
        d = (1.0 + 4.0 * rng.random(n)).astype(np.float32)
    elif name == 'equal':
        d = np.full(n, 2.5, dtype=np.float32)
    elif name == 'two':
        d = np.where(np.arange(n) < n // 2, 30.0, 1.0).astype(np.float32)
        rng.shuffle(d)
    elif name == 'lowbyte':
        d = (1.0 + (np.arange(n) % 200).astype(np.float64) * 2.0 ** -23).astype(np.float32)
        rng.shuffle(d)
    elif name == 'subnormal':
        bits = (np.arange(n) % 999 + 1).astype(np.uint32)
        rng.shuffle(bits)
        d = bits.view(np.float32).copy()
    else:
        assert name == 'nonpos'
        d = np.array([0.0, -0.0, -1.5, -np.inf], dtype=np.float32)[rng.integers(0, 4, n)]
    if name not in _NO_ZEROS:
        d[rng.random(n) < 0.1] = 0.0
    special = {'outlier': (n // 2, 1000.0), 'lowbyte': (n // 3, 100.0), 'inf': (n // 2, np.inf)}.get(name)
    if special:
        d[special[0]] = special[1]
    return d


def inside_mask_ref(d):
    """(thr float32, mask bool [n], depth_filtered float32 [n]): median = the LOWER middle of the sorted positive values, each of the
    two products rounded once to float32, nothing positive: thr = 0 and everything masked out."""
    d = np.asarray(d, dtype=np.float32)
    pos = np.sort(d[d > 0])
    if pos.size == 0:
        return np.float32(0.0), np.zeros(d.shape, bool), np.zeros(d.shape, np.float32)
    med = pos[(pos.size - 1) // 2]
    with np.errstate(over='ignore'):
        thr = min(np.float32(10.0) * med, np.float32(1.2) * pos[-1])
    mask = (d > 0) & (d <= thr)
    return np.float32(thr), mask, np.where(mask, d, np.float32(0.0)).astype(np.float32)


def needs_median(d):
    """Whether lk_inside_thr's counting shortcut hands over to the radix select: more than (m - 1) / 2 values with fl(10 v) < fl(1.2 max)."""
    pos = np.asarray(d, np.float32)
    pos = pos[pos > 0]
    if pos.size == 0:
        return False
    with np.errstate(over='ignore'):
        return int((np.float32(10.0) * pos < np.float32(1.2) * pos.max()).sum()) > (pos.size - 1) // 2


# ---------------------------------------------------------------------------- B. compaction
COMPACT_MASKS = ('zeros', 'ones', 'first', 'last', 'd01', 'd50', 'd99', 'bytes')


def compact_mask(name, n, seed):
    """uint8 [n]."""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return m
    if name == 'ones':
        m[:] = 1
    elif name == 'first':
        m[0] = 1
    elif name == 'last':
        m[-1] = 1
    elif name in ('d01', 'd50', 'd99'):
        m[rng.random(n) < {'d01': 0.01, 'd50': 0.5, 'd99': 0.99}[name]] = 1
    elif name == 'bytes':
        m = np.where(rng.random(n) < 0.5, rng.integers(1, 256, n), 0).astype(np.uint8)
    else:
        assert name == 'zeros'
    return m


# ---------------------------------------------------------------------------- H. exposure MLP
U = 2.0 ** -24          # unit round-off of float32
EPS_SOFTPLUS = 8 * U * np.log(2.0) / 100.0


def exposure_ref(feats, W1, b1, W2, b2, g_aff, k=lambda L: L + 8):
    """float64 autograd of aff = softplus(feats @ W1.T + b1, beta=100) @ W2.T + b2 under the output gradient g_aff, and for every output
    element of lk_exposure_fwd / lk_exposure_bwd the bound (L + 8) 2^-24 sum|terms| of its own accumulation chain of length L (8 for the
    pre-activation, 128 for aff and g feats, F for the four parameter gradients, 12 for d hid) PLUS what the bounds of the chain's inputs
    amount to at its output.  The second part is what the elements behind the softplus need; in first order, with s = sigmoid(100 pre):

      pre  : E_pre = 16 U S_pre,  S_pre = |b1| + sum_k |W1 feats|
      hid  : softplus is monotone with slope s <= 1, so its value moves by at most s(pre + E_pre) E_pre; the kernel evaluates it as
             log2(1 + 2^(c pre)) ln2 / 100 (lk_common.h: ABSOLUTE error ~3e-9: the sum 1 + e is rounded at 1, so a unit far below zero
             gives hid = 0, not a small number of equal relative accuracy) - EPS_SOFTPLUS = 8 U ln2 / 100 - and the result is rounded:
             E_h = s+ E_pre + EPS_SOFTPLUS + U hid
      s    : the backward takes s = 1 - exp(-100 hid) from the SAVED hid: d s / d hid = 100 (1 - s), two roundings and exp2's:
             E_s = 100 (1 - s-) E_h + 4 U, s- = s(pre - E_pre).  This is the factor 100 of softplus(beta = 100): a relative bound on
             sum|terms| alone fails at F = 1, where one unit with pre << 0 is the whole sum.
      d hid: E_dh = 20 U A,  A = sum_o |W2 g_aff|;    dp = d hid s:  E_dp = s E_dh + |d hid| E_s + E_dh E_s + U |dp|
      aff  : 136 U (|b2| + sum_u |W2 hid|) + sum_u |W2| E_h
      g W1 : (F + 8) U sum_f |dp feats| + sum_f |feats| E_dp          g b1: (F + 8) U sum_f |dp| + sum_f E_dp
      g W2 : (F + 8) U sum_f |g_aff hid| + sum_f |g_aff| E_h          g b2: (F + 8) U sum_f |g_aff|
      g feats: 136 U sum_u |W1 dp| + sum_u |W1| E_dp

    k(L): the rounding count of a chain of length L.  L + 8 is the worst case, every rounding in the same direction, and holds for
    every element.  k = sqrt(L + 8) is the probabilistic model of rounding-error analysis (independent roundings of mean zero: the error
    of n of them grows like sqrt(n) u, Higham & Mary 2019) - no bound for a single element, but the size the ROOT MEAN SQUARE of a
    tensor's errors has if the chains are what they should be: an accumulation that loses or doubles terms, or runs in a lower
    precision, shows there long before it reaches the worst case.

    Returns (values, bounds): dicts over aff [F,12], hid [F,128], gW1 [128,8], gb1 [128], gW2 [12,128], gb2 [12], gfeats [F,8]."""
    t = [torch.from_numpy(np.asarray(x, dtype=np.float32)).double().requires_grad_(True) for x in (feats, W1, b1, W2, b2)]
    f, w1, c1, w2, c2 = t
    ga = torch.from_numpy(np.asarray(g_aff, dtype=np.float32)).double()
    pre = f @ w1.T + c1
    hid = torch.nn.functional.softplus(pre, beta=100)
    aff = hid @ w2.T + c2
    (aff * ga).sum().backward()
    val = dict(aff=aff, hid=hid, gW1=w1.grad, gb1=c1.grad, gW2=w2.grad, gb2=c2.grad, gfeats=f.grad)
    val = {k: v.detach().numpy() for k, v in val.items()}
    f, w1, c1, w2, c2, ga, pre, hid = (x.detach().numpy() for x in (f, w1, c1, w2, c2, ga, pre, hid))
    F = f.shape[0]
    S_pre = np.abs(c1)[None, :] + np.abs(f) @ np.abs(w1).T                    # [F,128]
    E_pre = k(8) * U * S_pre
    sig = lambda x: 1.0 / (1.0 + np.exp(-100.0 * x))
    s, s_up = sig(pre), sig(pre + E_pre)
    E_h = s_up * E_pre + EPS_SOFTPLUS + U * hid
    E_s = 100.0 * (1.0 - sig(pre - E_pre)) * E_h + 4 * U
    dh = ga @ w2                                                               # [F,128]
    A = np.abs(ga) @ np.abs(w2)
    E_dh = k(12) * U * A
    dp = dh * s
    E_dp = s * E_dh + np.abs(dh) * E_s + E_dh * E_s + U * np.abs(dp)
    bound = dict(
        hid=E_h,
        aff=k(128) * U * (np.abs(c2)[None, :] + hid @ np.abs(w2).T) + E_h @ np.abs(w2).T,
        gW1=k(F) * U * (np.abs(dp).T @ np.abs(f)) + E_dp.T @ np.abs(f),
        gb1=k(F) * U * np.abs(dp).sum(0) + E_dp.sum(0),
        gW2=k(F) * U * (np.abs(ga).T @ hid) + np.abs(ga).T @ E_h,
        gb2=k(F) * U * np.abs(ga).sum(0),
        gfeats=k(128) * U * (np.abs(dp) @ np.abs(w1)) + E_dp @ np.abs(w1),
    )
    return val, bound
