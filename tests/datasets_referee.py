"""NumPy float64 referee of the frame preparation (include/loopy_hip.h, "frame preparation") and of the readers' pose files.

Stage by stage, in the reference's order (src/utils/datasets.py:95-119), with a uint8 image after the undistortion:

  undistort_u8      cv2's fixed-point remap restated: double source coordinates, rounded to 1/32 pixel, integer weights of sum 2^15
  color_unit        c / 255.0 (float64; rounded to fp32 it is the library's fp32 division for all 256 values: test_frame_prepare)
  depth_metres      float32(d) / png_depth_scale in fp32 (NumPy's float32 array / python float)
  resize_linear     cv2 INTER_LINEAR: source = (dst + 0.5) in / out - 0.5, clamped, plain bilinear
  crop_bilinear     align_corners: source = dst (in - 1) / (out - 1)
  crop_nearest      source = min(floor(dst * fp32(in / out)), in - 1), the product in fp32 (torch's legacy 'nearest')
  crop_edge         rows and columns [e, size - e)

prepare() chains them.  The pose parsers below are written from the file formats, independently of loopy_slam_amd.datasets.
"""
import os
import re

import numpy as np


# ---------------------------------------------------------------------------------------------------------------- frames
def remap_weights():
    """[32][32][4] integer weights of the 5-bit fractions (ay, ax) for the taps (0,0) (0,1) (1,0) (1,1), built the way cv2 builds its table:
    the float products rounded to integers of scale 2^15, a residual of the sum put on the largest weight.  For bilinear weights of 5-bit
    fractions the products are integers already - 32 (32 - ay)(32 - ax) and so on - and the residual is always 0 (asserted here)."""
    a = np.arange(32, dtype=np.float32) / np.float32(32)
    wy = np.stack([1 - a, a], 1)                                         # [32][2]
    w = wy[:, None, :, None] * wy[None, :, None, :]                      # [ay][ax][ty][tx], float32 products (exact)
    q = np.rint(w.reshape(32, 32, 4).astype(np.float64) * 32768).astype(np.int64)
    resid = 32768 - q.sum(-1)
    assert not resid.any()
    big = q.argmax(-1)
    np.put_along_axis(q, big[..., None], np.take_along_axis(q, big[..., None], -1) + resid[..., None], -1)
    i = np.arange(32)
    closed = 32 * np.stack([(32 - i)[:, None] * (32 - i)[None, :], (32 - i)[:, None] * i[None, :], i[:, None] * (32 - i)[None, :],
                            i[:, None] * i[None, :]], -1)
    assert (q == closed).all()
    return q


def undistort_source(H, W, fx, fy, cx, cy, dist):
    """Source coordinates (sx, sy) [H][W] of every destination pixel, in double, in the operation order the contract states."""
    k1, k2, p1, p2, k3 = (float(v) for v in dist)
    u = np.arange(W, dtype=np.float64)[None, :].repeat(H, 0)
    v = np.arange(H, dtype=np.float64)[:, None].repeat(W, 1)
    x, y = (u - cx) / fx, (v - cy) / fy
    r2 = x * x + y * y
    r4 = r2 * r2
    rad = ((1.0 + k1 * r2) + k2 * r4) + k3 * (r4 * r2)
    xd = (x * rad + ((2.0 * p1) * x) * y) + p2 * (r2 + (2.0 * x) * x)
    yd = (y * rad + p1 * (r2 + (2.0 * y) * y)) + ((2.0 * p2) * x) * y
    return fx * xd + cx, fy * yd + cy


def undistort_u8(img, fx, fy, cx, cy, dist, stats=None):
    """uint8 [H][W][3] -> uint8 [H][W][3].  stats (a dict): 'taps_inside' / 'taps' counts of the 2 x 2 taps that fall inside the image."""
    H, W = img.shape[:2]
    sx, sy = undistort_source(H, W, fx, fy, cx, cy, dist)
    lim = 1073741824.0
    qx = np.clip(np.rint(sx * 32.0), -lim, lim).astype(np.int64)
    qy = np.clip(np.rint(sy * 32.0), -lim, lim).astype(np.int64)
    ix, iy, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
    wt = remap_weights()[ay, ax]                                          # [H][W][4]
    acc = np.full((H, W, 3), 1 << 14, dtype=np.int64)
    inside = 0
    for t, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yy, xx = iy + dy, ix + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        inside += int(ok.sum())
        p = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
        acc += np.where(ok[..., None], wt[..., t, None] * p, 0)
    if stats is not None:
        stats['taps_inside'], stats['taps'] = inside, 4 * H * W
    return (acc >> 15).astype(np.uint8)


def color_unit(img_u8):
    return img_u8.astype(np.float64) / 255.0


def depth_metres(depth, png_depth_scale):
    return depth.astype(np.float32) / float(png_depth_scale)


def _bilinear(img, sy, sx):
    """img [H][W][C] float64 at the source coordinates sy [h], sx [w] (already inside [0, size - 1])."""
    H, W = img.shape[:2]
    y0 = np.minimum(np.floor(sy).astype(np.int64), H - 1)
    x0 = np.minimum(np.floor(sx).astype(np.int64), W - 1)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    fy, fx = (sy - y0)[:, None, None], (sx - x0)[None, :, None]
    top = (1 - fx) * img[y0][:, x0] + fx * img[y0][:, x1]
    bot = (1 - fx) * img[y1][:, x0] + fx * img[y1][:, x1]
    return (1 - fy) * top + fy * bot


def resize_linear(img, size):
    H, W = img.shape[:2]
    h, w = size
    sy = np.clip((np.arange(h) + 0.5) * (H / h) - 0.5, 0.0, H - 1.0)
    sx = np.clip((np.arange(w) + 0.5) * (W / w) - 0.5, 0.0, W - 1.0)
    return _bilinear(img, sy, sx)


def crop_bilinear(img, size):
    H, W = img.shape[:2]
    h, w = size
    return _bilinear(img, np.arange(h) * (H - 1) / (h - 1), np.arange(w) * (W - 1) / (w - 1))


def nearest_index(n_in, n_out):
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def crop_nearest(depth, size):
    return depth[nearest_index(depth.shape[0], size[0])][:, nearest_index(depth.shape[1], size[1])]


def crop_edge(img, e):
    return img[e:img.shape[0] - e, e:img.shape[1] - e] if e > 0 else img


def prepare(color_u8, depth, png_depth_scale, fx=None, fy=None, cx=None, cy=None, distortion=None, crop_size=None, edge=0, bgr=False):
    """-> colour float64 [Ho][Wo][3] (R, G, B), depth float32 [Ho][Wo], the uint8 colour after the undistortion (in the input's channel order)."""
    if distortion is not None and np.any(np.asarray(distortion, dtype=np.float64) != 0):
        color_u8 = undistort_u8(color_u8, fx, fy, cx, cy, distortion)
    u8 = color_u8
    c = color_unit(color_u8[..., ::-1] if bgr else color_u8)
    d = depth_metres(depth, png_depth_scale)
    if c.shape[:2] != d.shape:
        c = resize_linear(c, d.shape)
    if crop_size is not None:
        c, d = crop_bilinear(c, crop_size), crop_nearest(d, crop_size)
    return np.ascontiguousarray(crop_edge(c, edge)), np.ascontiguousarray(crop_edge(d, edge)), u8


# ---------------------------------------------------------------------------------------------------------------- poses
def flip_yz(c2w):
    out = np.array(c2w, dtype=np.float64)
    out[:3, 1] *= -1
    out[:3, 2] *= -1
    return out


def quat_matrix(q):
    """Rotation of the quaternion (x, y, z, w), any non-zero norm: R = I + 2 w [v]x + 2 [v]x^2 of the normalised quaternion."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.sqrt((q * q).sum())
    v, w = q[:3], q[3]
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + 2 * w * K + 2 * K @ K


def replica_poses(path, n):
    rows = [ln.split() for ln in open(path).read().splitlines() if ln.strip()]
    return [flip_yz(np.array(rows[i], dtype=np.float64).reshape(4, 4)).astype(np.float32) for i in range(n)]


def scannet_poses(folder):
    files = sorted((f for f in os.listdir(folder) if f.endswith('.txt')), key=lambda f: int(f[:-4]))
    return [flip_yz(np.array(open(os.path.join(folder, f)).read().split(), dtype=np.float64).reshape(4, 4)).astype(np.float32) for f in files]


def azure_poses(path, n):
    if not os.path.exists(path):
        return [np.eye(4, dtype=np.float32) for _ in range(n)]
    lines = open(path).read().splitlines()
    return [flip_yz(np.array(' '.join(lines[i + 1:i + 5]).split(), dtype=np.float64).reshape(4, 4)).astype(np.float32)
            for i in range(0, len(lines) - 4, 5)]


def tum_list(path, skip=0):
    """[(stamp, [fields])] of a TUM list file behind its first `skip` lines; '#' starts a comment."""
    out = []
    for ln in open(path).read().splitlines()[skip:]:
        ln = ln.split('#', 1)[0].strip()
        if ln:
            f = re.split(r'\s+', ln)
            out.append((float(f[0]), f[1:]))
    return out


def tum_sequence(folder, max_dt=0.08, frame_rate=32):
    """-> [(rgb file, depth file, c2w float32)] of a TUM folder: nearest depth and pose within max_dt, at most frame_rate frames per second,
    poses relative to the first kept association."""
    rgb, dep = tum_list(os.path.join(folder, 'rgb.txt')), tum_list(os.path.join(folder, 'depth.txt'))
    name = 'groundtruth.txt' if os.path.isfile(os.path.join(folder, 'groundtruth.txt')) else 'pose.txt'
    pose = tum_list(os.path.join(folder, name), skip=1)          # the reference reads the pose file with skiprows=1
    td, tp = np.array([t for t, _ in dep]), np.array([t for t, _ in pose])
    assoc = []
    for i, (t, _) in enumerate(rgb):
        j, k = int(np.abs(td - t).argmin()), int(np.abs(tp - t).argmin())
        if abs(td[j] - t) < max_dt and abs(tp[k] - t) < max_dt:
            assoc.append((i, j, k))
    keep = [0]
    for a in range(1, len(assoc)):
        if rgb[assoc[a][0]][0] - rgb[assoc[keep[-1]][0]][0] > 1.0 / frame_rate:
            keep.append(a)
    out, inv0 = [], None
    for a in keep:
        i, j, k = assoc[a]
        v = np.array(pose[k][1], dtype=np.float64)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = quat_matrix(v[3:7]), v[:3]
        if inv0 is None:
            inv0 = np.linalg.inv(T)
            T = np.eye(4)
        else:
            T = inv0 @ T
        out.append((os.path.join(folder, rgb[i][1][0]), os.path.join(folder, dep[j][1][0]), flip_yz(T).astype(np.float32)))
    return out
