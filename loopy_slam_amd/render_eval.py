"""Rendering evaluation of a finished run (csrc/lk_imgeval.hip; include/loopy_hip.h "rendering evaluation").

Reference                                                       here
  src/Mapper.py:1120-1160  depth L1, PSNR of a re-rendered frame  frame_metrics -> lk_img_eval, summarise
  pytorch_msssim.ms_ssim(data_range=1.0, size_average=True)       frame_metrics -> lk_img_eval, summarise / ms_ssim
  src/tools/eval_ate.py    evaluate_ate, align, convert_poses     ate
  src/Mapper.py:1056-1218  the evaluation at the end of a run     eval_run (slam.Mapper.run, cfg['rendering_eval'])

One frame pair is six launches (five pyramid levels and one fixed-order reduction) into a 33-entry fp64 record of sums and means on the
device; nothing is read back until summarise copies every frame's record at once and combines them in fp64 on the host.  pytorch_msssim
is not a dependency: the arithmetic is restated from its documented behaviour.  LPIPS is not computed.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import torch

from ._ffi import IMG_REC, ptr

LEVELS = 5
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MIN_SIDE = 160                                        # ms_ssim is defined above this (the package asserts (11 - 1) * 2 ** 4 < min(H, W))
DEFAULTS = {'enabled': False, 'ms_ssim': True}
ATE_KEYS = ('compared_pose_pairs',) + tuple(f'absolute_translational_error.{k}' for k in ('rmse', 'mean', 'median', 'std', 'min', 'max'))
TOO_SMALL = 'ms_ssim is defined for min(H, W) > 160 only (five levels of an 11-tap window)'


def settings(cfg):
    """cfg['rendering_eval'] over the defaults (absent key: disabled)."""
    out = dict(DEFAULTS)
    out.update(cfg.get('rendering_eval') or {})
    return out


def frame_metrics(eng, gt_color, color, gt_depth, depth, msssim=True):
    """The device record [33] f64 of one frame pair (lk_img_eval; no synchronisation).  gt_color, color [H,W,3] in [0, 1]; gt_depth,
    depth [H,W]; msssim=False leaves entries 3 .. 32 unwritten (NaN here)."""
    gt_color, color, gt_depth, depth = (eng.f32(a) for a in (gt_color, color, gt_depth, depth))
    H, W = int(gt_depth.shape[0]), int(gt_depth.shape[1])
    if tuple(depth.shape) != (H, W) or tuple(gt_color.shape) != (H, W, 3) or tuple(color.shape) != (H, W, 3):
        raise ValueError(f'frame_metrics: shapes {tuple(gt_color.shape)}, {tuple(color.shape)}, {tuple(gt_depth.shape)}, {tuple(depth.shape)} '
                         f'are not [H,W,3], [H,W,3], [H,W], [H,W]')
    if msssim and min(H, W) <= MIN_SIDE:
        raise ValueError(f'frame_metrics: {TOO_SMALL}; got {H} x {W}')
    n = C.c_int64(0)
    eng.lib.check(eng.lib.dll.lk_img_eval_ws_bytes(H, W, C.byref(n)), 'lk_img_eval_ws_bytes')
    ws = eng.empty((n.value + 7) // 8, dtype=torch.float64)
    rec = torch.full((IMG_REC,), float('nan'), dtype=torch.float64, device=eng.device)
    eng.lib.check(eng.lib.dll.lk_img_eval(ptr(gt_color), ptr(color), ptr(gt_depth), ptr(depth), H, W, int(bool(msssim)), ptr(ws), ptr(rec),
                                          eng.stream), 'lk_img_eval')
    return rec


def combine(rec):
    """ms_ssim of one host record: the mean over the channels of prod_l relu(v[l][c]) ** w[l], v = the cs mean below the last level and
    the SSIM mean at it (fp64)."""
    rec = np.asarray(rec, dtype=np.float64)
    v = np.stack([rec[3 + 6 * l + (0 if l == LEVELS - 1 else 3):][:3] for l in range(LEVELS)])
    return float(np.mean(np.prod(np.maximum(v, 0.0) ** np.asarray(MS_WEIGHTS)[:, None], axis=0)))


def summarise(records, msssim=True, reason=None):
    """One device-to-host copy of every frame's record, then fp64 on the host: per frame depth_l1 = rec[1] / rec[0], psnr =
    -10 log10(rec[2] / (3 rec[0])) (inf for a zero error) and ms_ssim, and their averages.  A frame without a valid pixel is listed under
    'skipped' (its position in `records`) and left out of the averages.  msssim=False: ms_ssim is None for the whole run and `reason`
    says why."""
    out = {'depth_l1': [], 'psnr': [], 'ms_ssim': [] if msssim else None, 'skipped': [],
           'avg_depth_l1': None, 'avg_psnr': None, 'avg_ms_ssim': None}
    if not msssim:
        out['ms_ssim_reason'] = reason or 'ms_ssim was not asked for'
    if not len(records):
        return out
    host = torch.stack(list(records)).cpu().numpy().astype(np.float64)
    kept = []
    for k, rec in enumerate(host):
        if not rec[0] > 0:
            out['skipped'].append(k)
            out['depth_l1'].append(None)
            out['psnr'].append(None)
            if msssim:
                out['ms_ssim'].append(None)
            continue
        kept.append(k)
        mse = rec[2] / (3.0 * rec[0])
        out['depth_l1'].append(float(rec[1] / rec[0]))
        out['psnr'].append(float('inf') if mse == 0 else float(-10.0 * math.log10(mse)))
        if msssim:
            out['ms_ssim'].append(combine(rec))
    if kept:
        out['avg_depth_l1'] = float(np.mean([out['depth_l1'][k] for k in kept]))
        out['avg_psnr'] = float(np.mean([out['psnr'][k] for k in kept]))
        if msssim:
            out['avg_ms_ssim'] = float(np.mean([out['ms_ssim'][k] for k in kept]))
    return out


def ms_ssim(eng, X, Y):
    """pytorch_msssim.ms_ssim(X, Y, data_range=1.0) of one pair of [H,W,3] images in [0, 1]; ValueError for min(H, W) <= 160."""
    X = eng.f32(X)
    H, W = int(X.shape[0]), int(X.shape[1])
    if min(H, W) <= MIN_SIDE:
        raise ValueError(f'{TOO_SMALL}; got {H} x {W}')
    flat = eng.zeros(H, W)
    return combine(frame_metrics(eng, X, Y, flat, flat, True).cpu().numpy())


# ------------------------------------------------------------------------------------------------ trajectory
def _poses64(p):
    if torch.is_tensor(p):
        p = p.detach().cpu().numpy()
    else:
        p = [q.detach().cpu().numpy() if torch.is_tensor(q) else q for q in p]
    return np.asarray(p, dtype=np.float64).reshape(-1, 4, 4)


def horn(model, data):
    """eval_ate.py:45-80: (rot [3,3], trans [3,1]) of the rotation and translation (no scale) that move model [3,n] onto data [3,n] in the
    least-squares sense."""
    mz, dz = model - model.mean(1, keepdims=True), data - data.mean(1, keepdims=True)
    Wm = np.zeros((3, 3))
    for k in range(model.shape[1]):                   # the reference's summation order
        Wm += np.outer(mz[:, k], dz[:, k])
    U, _, Vh = np.linalg.svd(Wm.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1.0
    rot = U @ S @ Vh
    return rot, data.mean(1, keepdims=True) - rot @ model.mean(1, keepdims=True)


def ate(est_c2w, gt_c2w, align=True):
    """Absolute trajectory error of camera-to-world poses ([N,4,4] tensors, arrays or lists), eval_ate.py in fp64: frames whose ground-truth
    pose has a non-finite entry are dropped from both lists; align: the estimate is first moved by Horn's closed form.  Returns the
    reference's seven result keys; fewer than two pairs raise ValueError."""
    est, gt = _poses64(est_c2w), _poses64(gt_c2w)
    if est.shape != gt.shape:
        raise ValueError(f'ate: {est.shape[0]} estimated and {gt.shape[0]} ground-truth poses')
    keep = np.isfinite(gt).all((1, 2))
    e, g = est[keep][:, :3, 3].T, gt[keep][:, :3, 3].T
    if e.shape[1] < 2:
        raise ValueError("ate: fewer than two pose pairs with a finite ground-truth pose")
    if align:
        rot, trans = horn(e, g)
        e = rot @ e + trans
    d = e - g
    err = np.sqrt((d * d).sum(0))
    vals = (np.sqrt(np.dot(err, err) / len(err)), np.mean(err), np.median(err), np.std(err), np.min(err), np.max(err))
    return dict(zip(ATE_KEYS, [int(len(err))] + [float(v) for v in vals]))


# ------------------------------------------------------------------------------------------------ the evaluation of a finished run
def frame_indices(estimate_c2w_list, n_frames, every_frame):
    """The reference's render_idx frames: every mapped frame below n_frames whose final pose is finite."""
    return [idx for idx in range(0, n_frames, every_frame) if bool(torch.isfinite(estimate_c2w_list[idx]).all())]


def report(frames, records, est_c2w, gt_c2w, msssim, reason, output):
    """The result dict of a run from its device records, written to {output}/eval/rendering.json if output is given."""
    s = summarise(records, msssim, reason)
    out = {'frames': list(frames)}
    out.update(s)
    for key, align in (('ate', True), ('ate_no_align', False)):
        try:
            out[key] = ate(est_c2w, gt_c2w, align)
        except ValueError as e:
            out[key] = None
            out[key + '_reason'] = str(e)
    if output is not None:
        os.makedirs(os.path.join(output, 'eval'), exist_ok=True)
        with open(os.path.join(output, 'eval', 'rendering.json'), 'w') as f:
            json.dump(out, f, indent=1)
    return out


def wants_msssim(es, H, W):
    """(compute ms_ssim?, the reason if not)."""
    if not es['ms_ssim']:
        return False, 'rendering_eval.ms_ssim is off'
    if min(H, W) <= MIN_SIDE:
        return False, f'{TOO_SMALL}; the frames are {H} x {W}'
    return True, None


class FrameRecords:
    """The device records of a run's evaluated frames, one lk_img_eval call per frame: an instance is the per-frame hook of tsdf.fuse_run
    (each re-rendered frame then serves the mesh and the evaluation) and what eval_run itself fills for the frames still missing."""

    def __init__(self, mapper):
        self.eng, self.es = mapper.eng, settings(mapper.cfg)
        self.records, self.msssim, self.reason = {}, False, 'no frame to evaluate'

    def __call__(self, idx, gt_color, gt_depth, depth, color):
        if not self.records:
            self.msssim, self.reason = wants_msssim(self.es, int(gt_depth.shape[0]), int(gt_depth.shape[1]))
        self.records[idx] = frame_metrics(self.eng, gt_color, color, gt_depth, depth, self.msssim)


def eval_run(mapper, n_frames, output=None, records=None):
    """Every mapped frame below n_frames with a finite final pose re-rendered from the final map (tsdf.rendered_frame) and measured against
    the input frame; ATE of the first n_frames poses with and without alignment.  records: a FrameRecords that tsdf.fuse_run filled while
    it rendered the same frames for the mesh - a frame it holds is not rendered again.  Reads the map, the decoders and the poses; writes
    none.  Returns the dict it writes to {output}/eval/rendering.json (output None: data.output of the config)."""
    from . import tsdf
    s, eng = mapper.slam, mapper.eng
    output = output or mapper.cfg['data'].get('output', 'output')
    records = records if records is not None else FrameRecords(mapper)
    frames = frame_indices(s.estimate_c2w_list, n_frames, mapper.every_frame)
    for idx in frames:
        if idx not in records.records:
            _, gt_color, gt_depth, _ = s.frame_reader[idx]
            depth, color = tsdf.rendered_frame(mapper, idx, gt_color, gt_depth, s.estimate_c2w_list[idx].float().to(eng.device))
            records(idx, gt_color, gt_depth, depth, color)
    return report(frames, [records.records[idx] for idx in frames], s.estimate_c2w_list[:n_frames], s.gt_c2w_list[:n_frames],
                  records.msssim, records.reason, output)
