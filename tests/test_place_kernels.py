"""The place-recognition kernels (csrc/lk_place.hip) against the NumPy referee tests/place_referee.py, on the host emulator and, under
-m gpu, on the chip.  The contract is integer arithmetic from the grey image onward, so every comparison is for EQUAL values: the keypoints,
the descriptor words and their number; the best / second-best distances, the best index and the per-segment counts of the matcher."""
import numpy as np
import pytest
import torch

import place_referee as R
import util
from loopy_slam_amd import place

MAX_HAMMING = 64


# ------------------------------------------------------------------------------------------------ inputs
def blocks_image(h, w, seed):
    """Random-brightness blocks of 5 - 9 pixels, a random colour per block."""
    rng = np.random.RandomState(seed)

    def cuts(n):
        out = [0]
        while out[-1] < n:
            out.append(out[-1] + rng.randint(5, 10))
        return np.searchsorted(np.array(out[1:]), np.arange(n), side='right')
    by, bx = cuts(h), cuts(w)
    table = rng.rand(by.max() + 1, bx.max() + 1, 3).astype(np.float32)
    return table[by[:, None], bx[None, :]]


def checkerboard(h, w, square=8):
    y, x = np.mgrid[0:h, 0:w]
    v = np.where(((y // square) + (x // square)) % 2 == 0, np.float32(0.2), np.float32(0.8))
    return np.repeat(v[:, :, None], 3, axis=2).astype(np.float32)


def squares(h, w, pitch=12):
    """2 x 2 dark squares every `pitch` pixels on a bright ground: four corners of equal score side by side in each, and every square alike."""
    img = np.full((h, w, 3), 0.8, dtype=np.float32)
    for y in range(6, h - 2, pitch):
        for x in range(6, w - 2, pitch):
            img[y:y + 2, x:x + 2] = 0.2
    return img


def planted_corners(h=100, w=120):
    """A dark quadrant corner at 20 and at 19 pixels from each border: the first of each pair lies inside the border region."""
    img = np.full((h, w, 3), 0.85, dtype=np.float32)
    for cx, cy in ((20, 50), (19, 70), (w - 21, 40), (w - 20, 60), (50, 20), (75, 19), (60, h - 21), (85, h - 20)):
        img[cy:cy + 4, cx:cx + 4] = 0.1
    return img


IMAGES = {
    'blocks_97x131': (lambda: blocks_image(97, 131, 1), 500),
    'blocks_131x97': (lambda: blocks_image(131, 97, 2), 500),
    'blocks_160x213_quota64': (lambda: blocks_image(160, 213, 3), 64),
    'constant': (lambda: np.full((97, 131, 3), 0.5, dtype=np.float32), 500),
    'checkerboard_120x160': (lambda: checkerboard(120, 160), 500),
    'squares_120x160_quota40': (lambda: squares(120, 160), 40),
    'planted_border': (planted_corners, 500),
}
_REF = {}


def referee(name):
    if name not in _REF:
        make, n_features = IMAGES[name]
        img = make()
        _REF[name] = (img,) + R.describe(img, n_features=n_features)
    return _REF[name]


def nan_bytes(eng, n):
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=eng.device)


def run_describe(eng, img, n_features):
    pr = place.PlaceRecognizer(eng, n_features=n_features)
    pr.workspace(img.shape[0], img.shape[1])
    ws = nan_bytes(eng, pr.layout[0])
    kp, desc = pr.describe(torch.from_numpy(img), ws=ws)
    return kp.cpu().numpy(), desc.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ tables
def test_tables():
    cs, pat = place.pattern_tables()
    rcs, rpat = R.tables()
    assert cs.dtype == np.int32 and pat.dtype == np.int8 and cs.shape == (2, 30) and pat.shape == (30, 256, 4)
    assert np.array_equal(cs, rcs) and np.array_equal(pat, rpat)
    assert np.abs(pat.astype(np.int64)).max() <= 17 and np.abs(pat[0].astype(np.int64)).max() <= 12
    assert place.level_quotas(500, 8) == R.quotas(500, 8) and sum(R.quotas(500, 8)) == 500
    assert place.level_quotas(64, 8) == R.quotas(64, 8)


# ------------------------------------------------------------------------------------------------ describe
@pytest.mark.parametrize('name', list(IMAGES))
@pytest.mark.parametrize('backend', util.backends())
def test_describe(backend, name):
    eng = util.make_engine(backend)
    img, rkp, rdesc = referee(name)
    kp, desc = run_describe(eng, img, IMAGES[name][1])
    levels = np.bincount(rkp[:, 2], minlength=8).tolist() if len(rkp) else []
    print(f'{name}: {len(rkp)} keypoints of the referee (per level {levels}), {len(kp)} of the device')
    assert kp.shape == rkp.shape and desc.shape == rdesc.shape
    assert np.array_equal(kp, rkp)
    assert np.array_equal(desc, rdesc)


def test_the_inputs_reach_what_they_are_for():
    """The referee alone: the cases the inputs were built for do occur in them."""
    _, kp, _ = referee('blocks_97x131')
    assert len(kp) > 50 and kp[:, 2].max() <= 4                  # 97 -> 80 -> 66 -> 55 -> 45 -> 37: levels 5 .. 7 have no interior
    assert [s[0] for s in place.level_sizes(97, 131, 6)[0]] == [97, 80, 66, 55, 45, 37]
    _, kp, _ = referee('blocks_160x213_quota64')
    quota = R.quotas(64, 8)
    full = [int((kp[:, 2] == l).sum()) == quota[l] for l in range(3)]
    assert all(full) and len(kp) <= 64                           # more corners than quota on the large levels
    assert len(referee('constant')[1]) == 0
    # FAST-9 finds no corner at the X junctions of an exact checkerboard (two opposite quadrants: runs of 5 at most) - level 0 of that input is
    # empty and only resampled levels carry keypoints; the 2 x 2 squares are the input where equal scores meet
    assert len(R.keys_of_level(R.grey_image(referee('checkerboard_120x160')[0]))[0]) == 0
    grey = R.grey_image(referee('squares_120x160_quota40')[0])
    hit, Rs = R.corners(grey)
    idx, key_R = R.keys_of_level(grey)
    side_by_side = hit[:, :-1] & hit[:, 1:] & (Rs[:, :-1] == Rs[:, 1:])
    assert side_by_side.sum() > 20                               # neighbours of equal score: the index decides the suppression
    assert len(idx) > R.quotas(40, 8)[0] and key_R[R.quotas(40, 8)[0] - 1] == key_R[R.quotas(40, 8)[0]]      # and the cut of the quota
    _, kp, _ = referee('planted_border')
    lvl0 = {(int(x), int(y)) for x, y, l, _ in kp if l == 0}
    xs, ys = {x for x, _ in lvl0}, {y for _, y in lvl0}
    assert min(xs) >= 20 and max(xs) <= 120 - 21 and min(ys) >= 20 and max(ys) <= 100 - 21
    assert any(x <= 23 for x in xs) and any(x >= 120 - 24 for x in xs) and any(y <= 23 for y in ys) and any(y >= 100 - 24 for y in ys)


@pytest.mark.parametrize('backend', util.backends())
def test_describe_repeatable(backend):
    eng = util.make_engine(backend)
    img = referee('blocks_160x213_quota64')[0]
    a, b = run_describe(eng, img, 64), run_describe(eng, img, 64)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------------------------------------ match and score
def descriptor_sets(na, nb_list, seed):
    """A query set of na rows and database sets of nb_list rows: random words, then the planted cases where the sizes allow them."""
    rng = np.random.RandomState(seed)

    def rand(n):
        return rng.randint(0, 2 ** 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)

    def flipped(row, n):
        out = row.copy()
        for b in range(n):
            out[b // 32] ^= np.uint32(1 << (b % 32))
        return out
    A, Bs = rand(na), [rand(nb) for nb in nb_list]
    for B in Bs:
        nb = len(B)
        if na >= 5 and nb >= 8:
            B[2] = flipped(A[0], 7)
            B[5] = B[2]                                              # duplicate rows: the lower index wins, second == best, 5 best > 4 second
            B[1] = flipped(A[1], MAX_HAMMING)                        # a pair at exactly max_hamming
            B[3] = flipped(A[2], MAX_HAMMING + 1)                    # and one beyond it
            B[4] = flipped(A[3], 40)                                 # 5 x 40 == 4 x 50
            B[7] = A[4]                                              # an exact match
            row = A[3].copy()                                        # the second-best of query row 3 at exactly 50: 50 OTHER bits flipped
            for b in range(255, 205, -1):
                row[b // 32] ^= np.uint32(1 << (b % 32))
            B[6] = row
    if na >= 8:
        A[7] = A[6]                                                  # duplicate query rows: the backward match picks the lower
    return A, Bs


SIZES = [(0, 5), (5, 0), (1, 1), (63, 65), (65, 63), (500, 500)]


@pytest.mark.parametrize('n_seg', [1, 7])
@pytest.mark.parametrize('na,nb', SIZES)
@pytest.mark.parametrize('backend', util.backends())
def test_match_score(backend, na, nb, n_seg):
    eng = util.make_engine(backend)
    F = 500
    # unequal counts: the first segment has nb rows, the others shrink, one is a single row (second = 257) and one is empty
    nbs = [nb] if n_seg == 1 else [nb, max(nb - 1, 0), nb // 2, 1, 0, min(nb + 3, F), max(nb - 7, 0)]
    A, Bs = descriptor_sets(na, nbs, 100 * na + nb + n_seg)
    pr = place.PlaceRecognizer(eng, n_features=F, max_hamming=MAX_HAMMING, capacity=2)
    for B in Bs:
        pr.add(torch.from_numpy(B.view(np.int32)))
    assert pr.n_segments == n_seg and pr.db.shape[0] >= n_seg
    q = torch.from_numpy(A.view(np.int32).reshape(na, 8))
    count, rows = pr.match_counts(q)
    count, rows = count.cpu().numpy(), rows.cpu().numpy()
    scores = pr.scores(q)
    for s, B in enumerate(Bs):
        n, fw, bw = R.good_count(A, B, MAX_HAMMING)
        assert count[s] == n, (s, count[s], n)
        for d, (ref, m) in enumerate(((fw, na), (bw, len(B)))):
            got = rows[s, d, :m].astype(np.int64)
            assert np.array_equal(got[:, 0], ref[0]) and np.array_equal(got[:, 1], ref[1]) and np.array_equal(got[:, 2], ref[2]), (s, d)
        assert scores[s] == R.score(A, B, MAX_HAMMING)
        if len(B) == 1 and na:
            assert (rows[s, 0, :na, 1] == R.NO_MATCH).all()
    if na >= 5 and nbs[0] >= 8:
        fw = R.match(A, Bs[0])
        assert fw[2][0] == 2 and fw[0][0] == fw[1][0] == 7                     # the duplicate: lowest index, no distinctive best
        assert fw[0][1] == MAX_HAMMING and fw[0][2] == MAX_HAMMING + 1
        assert fw[0][3] == 40 and fw[1][3] == 50 and fw[0][4] == 0
        # rows 1, 3 and 4 count, rows 0 (ratio) and 2 (distance) do not - if their matches are mutual, which random rows do not disturb
        n, _, bw = R.good_count(A, Bs[0], MAX_HAMMING)
        assert bw[2][1] == 1 and bw[2][4] == 3 and bw[2][7] == 4 and n >= 3


@pytest.mark.parametrize('backend', util.backends())
def test_match_repeatable(backend):
    eng = util.make_engine(backend)
    A, Bs = descriptor_sets(65, [63, 20, 0], 9)
    pr = place.PlaceRecognizer(eng, n_features=80, max_hamming=MAX_HAMMING)
    for B in Bs:
        pr.add(torch.from_numpy(B.view(np.int32)))
    q = torch.from_numpy(A.view(np.int32))
    runs = []
    for _ in range(2):
        count, rows = pr.match_counts(q)
        rows = rows.cpu().numpy()
        runs.append((count.cpu().numpy().tobytes(), rows[0, 0, :65].tobytes(), rows[0, 1, :63].tobytes(), rows[1, 1, :20].tobytes()))
    assert runs[0] == runs[1]
