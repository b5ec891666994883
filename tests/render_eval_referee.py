"""Independent restatement of the rendering-evaluation contract (include/loopy_hip.h "rendering evaluation") and of the
reference's ATE (src/tools/eval_ate.py) for tests/test_render_eval*.py.  torch on the CPU and numpy only; nothing from the package.

record(..., dtype=torch.float64) is the referee; record(..., dtype=torch.float32) is the torch-op path a user would write (grouped conv2d,
avg_pool2d, means) and serves the tests as the measure of what fp32 costs.
"""
import numpy as np
import torch
import torch.nn.functional as F

REC = 33
LEVELS = 5
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2
ATE_KEYS = ('compared_pose_pairs',) + tuple(f'absolute_translational_error.{k}' for k in ('rmse', 'mean', 'median', 'std', 'min', 'max'))


def window(dtype):
    k = torch.arange(11, dtype=torch.float64) - 5.0
    g = torch.exp(-(k * k) / (2.0 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def _filter(x, g):
    """The 11-tap window down the columns, then along the rows, no padding; x [1,3,h,w]."""
    x = F.conv2d(x, g.reshape(1, 1, 11, 1).repeat(3, 1, 1, 1), groups=3)
    return F.conv2d(x, g.reshape(1, 1, 1, 11).repeat(3, 1, 1, 1), groups=3)


def level_means(X, Y, g):
    """(ssim mean [3], cs mean [3]) of one level; X, Y [1,3,h,w]."""
    mu1, mu2 = _filter(X, g), _filter(Y, g)
    mu11, mu22, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = _filter(X * X, g) - mu11, _filter(Y * Y, g) - mu22, _filter(X * Y, g) - mu12
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim = ((2 * mu12 + C1) / (mu11 + mu22 + C1)) * cs
    return ssim.flatten(2).mean(-1)[0], cs.flatten(2).mean(-1)[0]


def pool(x):
    return F.avg_pool2d(x, kernel_size=2, padding=[s % 2 for s in x.shape[2:]])


def masked_sums(gt_color, color, gt_depth, depth):
    """(n_valid, depth sum, colour sum): fp32 differences, fp64 squares and sums."""
    on = gt_depth > 0
    d = (gt_depth - depth)[on].double().abs().sum()
    c = ((gt_color - color)[on].double() ** 2).sum()
    return float(on.sum()), float(d), float(c)


def record(gt_color, color, gt_depth, depth, dtype=torch.float64, msssim=True):
    """The 33-entry record as a float64 numpy array (entries 3.. are NaN with msssim=False)."""
    gt_color, color, gt_depth, depth = (torch.as_tensor(a, dtype=torch.float32).cpu() for a in (gt_color, color, gt_depth, depth))
    rec = np.full(REC, np.nan)
    rec[0:3] = masked_sums(gt_color, color, gt_depth, depth)
    if msssim:
        X, Y = (a.permute(2, 0, 1)[None].to(dtype) for a in (gt_color, color))
        g = window(dtype)
        for l in range(LEVELS):
            ssim, cs = level_means(X, Y, g)
            rec[3 + 6 * l:6 + 6 * l] = ssim.double().numpy()
            rec[6 + 6 * l:9 + 6 * l] = cs.double().numpy()
            if l + 1 < LEVELS:
                X, Y = pool(X), pool(Y)
    return rec


def combine(rec):
    """ms_ssim of a record: mean over the channels of prod_l relu(v[l][c]) ** w[l], v = cs below the last level and ssim at it (fp64)."""
    rec = np.asarray(rec, dtype=np.float64)
    v = np.stack([rec[6 + 6 * l:9 + 6 * l] if l < LEVELS - 1 else rec[3 + 6 * l:6 + 6 * l] for l in range(LEVELS)])
    return float(np.mean(np.prod(np.maximum(v, 0.0) ** np.asarray(WEIGHTS)[:, None], axis=0)))


def figures(rec):
    """(depth_l1, psnr) of a record."""
    rec = np.asarray(rec, dtype=np.float64)
    mse = rec[2] / (3.0 * rec[0])
    return float(rec[1] / rec[0]), (float('inf') if mse == 0 else float(-10.0 * np.log10(mse)))


# ------------------------------------------------------------------------------------------------ ATE
def horn(model, data):
    """eval_ate.py align(): (rot, trans, det(U) det(Vh)) moving model [3,n] onto data [3,n]."""
    mz, dz = model - model.mean(1, keepdims=True), data - data.mean(1, keepdims=True)
    Wm = np.zeros((3, 3))
    for k in range(model.shape[1]):
        Wm += np.outer(mz[:, k], dz[:, k])
    U, _, Vh = np.linalg.svd(Wm.T)
    sign = np.linalg.det(U) * np.linalg.det(Vh)
    S = np.eye(3)
    if sign < 0:
        S[2, 2] = -1.0
    rot = U @ S @ Vh
    return rot, data.mean(1, keepdims=True) - rot @ model.mean(1, keepdims=True), sign


def ate(est, gt, align=True):
    est, gt = np.asarray(est, dtype=np.float64).reshape(-1, 4, 4), np.asarray(gt, dtype=np.float64).reshape(-1, 4, 4)
    keep = np.isfinite(gt).all((1, 2))
    e, g = est[keep][:, :3, 3].T, gt[keep][:, :3, 3].T
    if e.shape[1] < 2:
        raise ValueError('fewer than two pose pairs')
    if align:
        rot, trans, _ = horn(e, g)
        e = rot @ e + trans
    err = np.sqrt(((e - g) ** 2).sum(0))
    vals = (len(err), np.sqrt(np.dot(err, err) / len(err)), np.mean(err), np.median(err), np.std(err), np.min(err), np.max(err))
    return dict(zip(ATE_KEYS, [int(vals[0])] + [float(v) for v in vals[1:]]))
