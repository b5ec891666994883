"""Place recognition: which earlier segment does a keyframe look at?

Reference                                                          here
  src/neural_point.py:126-142   cv2.ORB_create(500) descriptors     PlaceRecognizer.describe -> lk_place_detect, lk_place_describe
  src/neural_point.py:619-644   pydbow3 database, query top kval    PlaceRecognizer.add / scores -> lk_place_match_score
  src/neural_point.py:1076-1107 compute_dbow_score                  loop_closure.LoopCloser.on_mapped_frame (the running minimum)

Neither OpenCV nor pydbow3 (nor its vocabulary file) can be assumed, so the descriptor is the library's own ORB-like contract
(include/loopy_hip.h, "place recognition": integer arithmetic from the grey image onward) and the score is a direct one: the share of
descriptors with a mutual, near and distinctive best match.  With a few hundred segments of 500 descriptors each, brute force on the device
is microseconds.  Parity with OpenCV's ORB and with DBoW scores is not claimed.
"""
import ctypes as C

import numpy as np
import torch

from . import _ffi
from ._ffi import ptr

N_TESTS = 256


def philox(key, c0, c1):
    """Philox4x32-10, key (key, 0), counter (c0, c1, 0, 0): [n,4] words as uint64 values (the rule of include/loopy_hip.h)."""
    M = np.uint64(0xFFFFFFFF)
    c0, c1 = np.broadcast_arrays(np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64))
    c = [c0 & M, c1 & M, np.zeros_like(c0), np.zeros_like(c0)]
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64(0)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack(c, -1)


def pattern_tables():
    """(cos_sin int32 [2][30], pattern int8 [30][256][4]): the orientation table and the 30 rotated test patterns of the contract."""
    test, coord = np.meshgrid(np.arange(N_TESTS), np.arange(4), indexing='ij')
    u = philox(_ffi.PLACE_SEED, test, coord)                                   # [256,4,4]
    base = (u % np.uint64(7)).sum(-1).astype(np.int64) - 12                    # [256,4] = (ax, ay, bx, by)
    ang = np.arange(_ffi.PLACE_BINS, dtype=np.float64) * (np.pi / 15.0)
    c, s = np.cos(ang), np.sin(ang)
    cos_sin = np.stack([np.rint(16384.0 * c), np.rint(16384.0 * s)]).astype(np.int32)
    x, y = base[None, :, 0::2].astype(np.float64), base[None, :, 1::2].astype(np.float64)     # [1,256,2]: the a and the b point
    xr = np.rint(c[:, None, None] * x - s[:, None, None] * y)
    yr = np.rint(s[:, None, None] * x + c[:, None, None] * y)
    pattern = np.empty((_ffi.PLACE_BINS, N_TESTS, 4), dtype=np.int8)
    pattern[:, :, 0::2], pattern[:, :, 1::2] = xr, yr
    return cos_sin, pattern


def level_sizes(H, W, n_levels):
    """[(h, w)] of the pyramid and the first pixel of each level in the concatenated arrays (one entry more: the total)."""
    sizes, off = [], [0]
    for _ in range(n_levels):
        sizes.append((H, W))
        off.append(off[-1] + H * W)
        H, W = 5 * H // 6, 5 * W // 6
    return sizes, off


def level_quotas(n_features, n_levels):
    """ORB's geometric share of n_features per level (include/loopy_hip.h, "Selection")."""
    f = 5.0 / 6.0
    d = n_features * (1.0 - f) / (1.0 - f ** n_levels)
    out = []
    for _ in range(n_levels - 1):
        out.append(int(np.floor(d + 0.5)))
        d *= f
    return out + [max(n_features - sum(out), 0)]


class PlaceRecognizer:
    """Descriptors of keyframes and a database of one descriptor set per segment, both on the device.

    describe(color) -> (kp int32 [N,4] = (x, y, level, bin), desc int32 [N,8] holding the uint32 words)
    add(desc)       -> the new segment's number
    scores(desc)    -> float64 [S]: mutual good matches / min(N_query, N_t), 0 if either set is empty."""

    def __init__(self, eng, n_features=500, n_levels=8, max_hamming=64, capacity=16):
        if not (1 <= n_levels <= _ffi.PLACE_MAX_LEVELS and n_features >= 1):
            raise ValueError(f'n_levels {n_levels} (1 .. {_ffi.PLACE_MAX_LEVELS}), n_features {n_features} (>= 1)')
        self.eng, self.n_features, self.n_levels, self.max_hamming = eng, int(n_features), int(n_levels), int(max_hamming)
        self.quota = level_quotas(self.n_features, self.n_levels)
        cos_sin, pattern = pattern_tables()
        self.cos_sin = torch.from_numpy(cos_sin).to(eng.device).contiguous()
        self.pattern = torch.from_numpy(pattern).to(eng.device).contiguous()
        self.db = eng.zeros(max(int(capacity), 1), self.n_features, 8, dtype=torch.int32)
        self.counts = eng.zeros(max(int(capacity), 1), dtype=torch.int32)
        self.n_segments = 0
        self._ws, self._ws_key, self.layout = None, None, None
        self.last_rows = None

    # ---- descriptors
    def workspace(self, H, W):
        """The uint8 workspace of an H x W image, kept between calls; self.layout = lk_place_ws_bytes' record."""
        if self._ws_key != (H, W):
            lay = (C.c_int64 * 8)()
            self.eng.lib.check(self.eng.lib.dll.lk_place_ws_bytes(H, W, self.n_levels, lay), 'lk_place_ws_bytes')
            self.layout = [int(v) for v in lay]
            self._ws = self.eng.empty(self.layout[0], dtype=torch.uint8)
            self._ws_key = (H, W)
        return self._ws

    def describe(self, color, ws=None):
        """color [H,W,3] in [0,1] (the frame readers' RGB).  ws: a caller's workspace of self.workspace(H, W)'s size (tests)."""
        eng, dll = self.eng, self.eng.lib.dll
        color = color.detach().to(eng.device, torch.float32).contiguous()
        H, W = int(color.shape[0]), int(color.shape[1])
        own = self.workspace(H, W)
        ws = own if ws is None else ws
        lay = self.layout
        P = lay[1]
        level_counts = eng.empty(self.n_levels, dtype=torch.int32)
        eng.lib.check(dll.lk_place_detect(ptr(color), H, W, self.n_levels, ptr(ws), ptr(level_counts), eng.stream), 'lk_place_detect')
        cnt = level_counts.cpu().tolist()                       # the one synchronisation of an image
        score = ws[lay[4]:lay[4] + 8 * P].view(torch.int64)
        index = ws[lay[5]:lay[5] + 4 * P].view(torch.int32)
        chosen, start = [], 0
        for n, quota in zip(cnt, self.quota):
            keys = index[start:start + n]
            start += n
            if n == 0 or quota == 0:
                continue
            # (score descending, pixel ascending): the list is ascending in the pixel and the sort is stable
            chosen.append(keys[torch.sort(-score[keys.long()], stable=True).indices[:quota]])
        N = sum(int(k.shape[0]) for k in chosen)
        kp, desc = eng.empty(N, 4, dtype=torch.int32), eng.empty(N, 8, dtype=torch.int32)
        if N:
            sel = torch.cat(chosen).contiguous()
            eng.lib.check(dll.lk_place_describe(ptr(ws), H, W, self.n_levels, ptr(sel), N, ptr(self.cos_sin), ptr(self.pattern), ptr(kp),
                                                ptr(desc), eng.stream), 'lk_place_describe')
        return kp, desc

    # ---- database
    def add(self, desc):
        n = int(desc.shape[0])
        if n > self.n_features:
            raise ValueError(f'{n} descriptors for a database of {self.n_features} per segment')
        if self.n_segments == self.db.shape[0]:                 # grown geometrically
            cap = 2 * self.n_segments
            db, counts = self.eng.zeros(cap, self.n_features, 8, dtype=torch.int32), self.eng.zeros(cap, dtype=torch.int32)
            db[:self.n_segments], counts[:self.n_segments] = self.db, self.counts
            self.db, self.counts = db, counts
        s = self.n_segments
        self.db[s, :n] = desc.to(self.eng.device, torch.int32)
        self.counts[s] = n
        self.n_segments += 1
        return s

    def match_counts(self, desc, db=None, counts=None, n_segments=None):
        """(count int32 [S], rows int32 [S,2,F,3]) of lk_place_match_score on the device, against the database or a caller's."""
        eng = self.eng
        db = self.db if db is None else db
        counts = self.counts if counts is None else counts
        S = self.n_segments if n_segments is None else int(n_segments)
        F, n = int(db.shape[1]), int(desc.shape[0])
        desc = desc.to(eng.device, torch.int32).contiguous()
        rows, out = eng.empty(max(S, 1), 2, F, 3, dtype=torch.int32), eng.zeros(max(S, 1), dtype=torch.int32)
        eng.lib.check(eng.lib.dll.lk_place_match_score(ptr(desc), n, ptr(db), ptr(counts), S, F, self.max_hamming, ptr(rows), ptr(out),
                                                       eng.stream), 'lk_place_match_score')
        return out[:S], rows[:S]

    def scores(self, desc):
        S, n = self.n_segments, int(desc.shape[0])
        if S == 0:
            return np.zeros(0)
        count, self.last_rows = self.match_counts(desc)
        count = count.cpu().numpy().astype(np.float64)
        nt = self.counts[:S].cpu().numpy().astype(np.float64)
        den = np.minimum(float(n), nt)
        return np.where(den > 0, count / np.maximum(den, 1.0), 0.0)
