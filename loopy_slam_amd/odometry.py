"""RGB-D visual odometry: the tracker's starting pose from the previous and the current frame.

Reference                                                          here
  src/utils/visual_odometer.py  VisualOdometer (Open3D, Hybrid)     VisualOdometer -> lk_odom_prepare, lk_odom_estimate
  src/Tracker.py:92-97          the odometer of tracking.visual_odometer
  src/Tracker.py:275-277, 291-295, 304-309                          slam.Tracker.track_frame (the reference's precedence, kept)

Open3D cannot be assumed, so the contract is the library's own (include/loopy_hip.h, "visual odometry"): bilinear lookups in
the target frame and a correct pose composition are its two deliberate departures.  A frame's pyramid is built once and serves as the source
of one estimate and the target of the next; the whole multi-scale loop is enqueued without a host synchronisation, and T with the last
iteration's record come back in one copy per frame.
"""
import ctypes as C

import torch

from . import _ffi
from ._ffi import ptr

DEFAULTS = dict(levels=None, iters=(100, 50, 30), max_depth=10.0, outlier_trunc=0.07, huber_intensity=0.1, huber_depth=0.05,
                min_valid_fraction=0.1)
# camera frame of this project (common.get_rays_from_uv: directions (x, -y, -1)) <-> the pinhole frame of the estimate
FLIP = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=torch.float64))


def options(value):
    """cfg['tracking']['visual_odometer'] -> the resolved options, or None when it is off (absent, False, None)."""
    if not value:
        return None
    opt = dict(DEFAULTS)
    if isinstance(value, dict):
        unknown = set(value) - set(DEFAULTS)
        if unknown:
            raise ValueError(f'tracking.visual_odometer: unknown keys {sorted(unknown)}')
        opt.update(value)
    opt['iters'] = [int(v) for v in opt['iters']]
    opt['levels'] = len(opt['iters']) if opt['levels'] is None else int(opt['levels'])
    if opt['levels'] != len(opt['iters']):
        raise ValueError(f"tracking.visual_odometer: {opt['levels']} levels but {len(opt['iters'])} iteration counts (coarse to fine)")
    return opt


class VisualOdometer:
    """set_init_state(color, depth, c2w), update_est_abs_pose(c2w), estimate_pose(color, depth) -> c2w, get_last_frame() - the reference's
    names.  color [H,W,3] in [0,1] and depth [H,W] are device tensors; poses are 4 x 4 c2w in this project's camera frame, kept on the host.

    intr: H, W, fx, fy, cx, cy (a mapping).  cfg: True or the dict of cfg['tracking']['visual_odometer'].
    After estimate_pose: last_T (float64 [4,4], source = current to target = previous, pinhole frame), last_record (float64 [ODOM_REC]),
    last_ok (False: the copied pose was returned; counted in `fallbacks`)."""

    def __init__(self, eng, intr, cfg=True):
        opt = options(cfg)
        if opt is None:
            raise ValueError('VisualOdometer: tracking.visual_odometer is off')
        self.eng, self.opt = eng, opt
        self.H, self.W = int(intr['H']), int(intr['W'])
        self.K = tuple(float(intr[k]) for k in ('fx', 'fy', 'cx', 'cy'))
        self.n_levels = opt['levels']
        lay = (C.c_int64 * (4 + 2 * _ffi.ODOM_MAX_LEVELS))()
        eng.lib.check(eng.lib.dll.lk_odom_ws_bytes(self.H, self.W, self.n_levels, lay), 'lk_odom_ws_bytes')
        self.layout = [int(v) for v in lay]
        self.iters = (C.c_int32 * self.n_levels)(*opt['iters'])
        self.n_iters = sum(opt['iters'])
        self.pyr = [eng.empty(self.layout[0] // 4), eng.empty(self.layout[0] // 4)]        # previous, current
        self.ws = eng.empty(self.layout[1], dtype=torch.uint8)
        self.state = eng.empty(16 + max(self.n_iters, 1) * _ffi.ODOM_REC, dtype=torch.float64)      # T, then the log
        self.eye = torch.eye(4, dtype=torch.float64).reshape(16).to(eng.device)
        self.last_abs_pose = None
        self.last_frame = None
        self.last_T = self.last_record = None
        self.last_ok = True
        self.fallbacks = 0

    # ---- kernels
    def prepare(self, color, depth, out):
        """The pyramid of one frame into `out` (layout[0] bytes of float32)."""
        eng, o = self.eng, self.opt
        color = color.detach().to(eng.device, torch.float32).contiguous()
        depth = depth.detach().to(eng.device, torch.float32).contiguous()
        if tuple(color.shape) != (self.H, self.W, 3) or tuple(depth.shape) != (self.H, self.W):
            raise ValueError(f'VisualOdometer: frame of {tuple(color.shape)} / {tuple(depth.shape)} for {self.H} x {self.W}')
        eng.lib.check(eng.lib.dll.lk_odom_prepare(ptr(color), ptr(depth), self.H, self.W, self.n_levels, *self.K, o['max_depth'],
                                                  2.0 * o['outlier_trunc'], ptr(out), eng.stream), 'lk_odom_prepare')
        return out

    def estimate(self, pyr_src, pyr_tgt, state=None, ws=None, iters=None, T0=None):
        """Enqueue one estimate: state[:16] = T (identity or T0 on entry), state[16:] = the log.  No synchronisation."""
        eng, o = self.eng, self.opt
        state = self.state if state is None else state
        ws = self.ws if ws is None else ws
        iters = self.iters if iters is None else (C.c_int32 * self.n_levels)(*iters)
        state[:16] = self.eye if T0 is None else T0.to(eng.device, torch.float64).reshape(16)
        log = state[16:]
        eng.lib.check(eng.lib.dll.lk_odom_estimate(ptr(pyr_src), ptr(pyr_tgt), self.H, self.W, self.n_levels, *self.K, iters, o['outlier_trunc'],
                                                   o['huber_intensity'], o['huber_depth'], ptr(state), ptr(log) if log.numel() else 0,
                                                   ptr(ws), eng.stream), 'lk_odom_estimate')
        return state

    def level_planes(self, pyr, level):
        """[ODOM_PLANES, h, w] view of one level of a pyramid: I, Vx, Vy, D, Ix, Iy, Dx, Dy."""
        h, w = self.H >> level, self.W >> level
        off = self.layout[4 + level]
        return pyr[off:off + _ffi.ODOM_PLANES * h * w].view(_ffi.ODOM_PLANES, h, w)

    # ---- the reference's interface
    def set_init_state(self, color, depth, c2w):
        self.prepare(color, depth, self.pyr[0])
        self.last_frame = (color, depth)
        self.update_est_abs_pose(c2w)

    def update_est_abs_pose(self, c2w):
        self.last_abs_pose = c2w.detach().to('cpu', torch.float64).clone()

    def get_last_frame(self):
        return self.last_frame

    def estimate_pose(self, color, depth):
        """c2w of the new frame (float64 [4,4], host): last_abs_pose @ F T F, or last_abs_pose itself when the estimate is not usable."""
        if self.last_abs_pose is None:
            raise RuntimeError('VisualOdometer.estimate_pose before set_init_state')
        self.prepare(color, depth, self.pyr[1])
        state = self.estimate(self.pyr[1], self.pyr[0])
        n = self.n_iters
        if n:
            back = torch.cat([state[:16], state[16 + (n - 1) * _ffi.ODOM_REC:16 + n * _ffi.ODOM_REC]]).cpu()      # the one read-back of a frame
            self.last_T, self.last_record = back[:16].reshape(4, 4), back[16:]
            valid, pixels = float(self.last_record[2]), self.layout[4 + _ffi.ODOM_MAX_LEVELS + int(self.last_record[0])]
            self.last_ok = bool(self.last_record[32] == 0.0) and valid >= self.opt['min_valid_fraction'] * pixels \
                and bool(torch.isfinite(self.last_T).all())
        else:
            self.last_T, self.last_record, self.last_ok = torch.eye(4, dtype=torch.float64), None, True
        self.pyr.reverse()                                  # the current frame is the next estimate's target
        self.last_frame = (color, depth)
        if self.last_ok:
            c2w = self.last_abs_pose @ FLIP @ self.last_T @ FLIP
        else:
            self.fallbacks += 1
            c2w = self.last_abs_pose.clone()
        self.last_abs_pose = c2w.clone()
        return c2w
