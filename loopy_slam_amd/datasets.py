"""Sequence readers under the reference's names (src/utils/datasets.py): Replica, ScanNet, Azure, TUM_RGBD behind get_dataset.

Reference                                                   here
  BaseDataset.__getitem__ (datasets.py:87-121)               Pillow decode on the host, raw uint8 / uint16 upload, lk_frame_prepare on the device
    cv2.undistort, BGR->RGB, / 255., cv2.resize,               (undistortion, conversion, resize to the depth size, crop_size, crop_edge:
    F.interpolate to crop_size, the edge crop                   include/loopy_hip.h "frame preparation")
  Replica / Azure / ScanNet / TUM_RGBD (datasets.py:124-331) the same layouts and pose conventions; the quaternion -> rotation is a closed form
  CoFusion                                                   not read: it needs an EXR decoder

Only decoding needs a host library (Pillow).  One background thread decodes the next `data.prefetch` frames (default 2, 0 = off) into a ring
of reusable host buffers (pinned when the device is a GPU); it never touches the GPU.  Upload and launch happen on the calling thread and
its current stream.  Sequential access hits the ring, any other index is decoded on the spot.
"""
import ctypes as C
import glob
import os
import threading

import numpy as np
import torch

from . import _ffi
from ._ffi import ptr


# ---------------------------------------------------------------------------------------------------------------- device
def output_size(Hd, Wd, crop_size=None, crop_edge=0):
    Hb, Wb = (int(crop_size[0]), int(crop_size[1])) if crop_size else (Hd, Wd)
    return Hb - 2 * crop_edge, Wb - 2 * crop_edge


def prepare_frame(eng, color_u8, depth, png_depth_scale, fx=0.0, fy=0.0, cx=0.0, cy=0.0, distortion=None, crop_size=None, crop_edge=0, bgr=False,
                  undist=None, out=None):
    """lk_frame_prepare.  color_u8 [Hc,Wc,3] uint8 and depth [Hd,Wd] (uint16 / int16 bits, or float32) on eng.device -> (color [Ho,Wo,3],
    depth [Ho,Wo]) float32.  undist: uint8 [Hc,Wc,3] scratch of the undistortion (allocated here when missing); out: the two outputs."""
    Hc, Wc = int(color_u8.shape[0]), int(color_u8.shape[1])
    Hd, Wd = int(depth.shape[0]), int(depth.shape[1])
    assert color_u8.dtype == torch.uint8 and color_u8.is_contiguous() and depth.is_contiguous()
    assert color_u8.device == eng.device and depth.device == eng.device
    flags = (_ffi.FRAME_BGR if bgr else 0) | (_ffi.FRAME_DEPTH_F32 if depth.dtype == torch.float32 else 0)
    assert depth.dtype == torch.float32 or depth.element_size() == 2
    ch, cw = (int(crop_size[0]), int(crop_size[1])) if crop_size else (0, 0)
    dist = None
    if distortion is not None:
        dist = (C.c_double * 5)(*[float(v) for v in distortion])
        if undist is None and any(dist):
            undist = eng.empty(Hc, Wc, 3, dtype=torch.uint8)
    Ho, Wo = output_size(Hd, Wd, crop_size, crop_edge)
    if out is None:
        out = (eng.empty(max(Ho, 0), max(Wo, 0), 3), eng.empty(max(Ho, 0), max(Wo, 0)))
    eng.lib.check(eng.lib.dll.lk_frame_prepare(ptr(color_u8), Hc, Wc, ptr(depth), Hd, Wd, flags, float(png_depth_scale), float(fx), float(fy),
                                               float(cx), float(cy), dist, ch, cw, int(crop_edge), ptr(undist), ptr(out[0]), ptr(out[1]),
                                               eng.stream), 'lk_frame_prepare')
    return out


# ---------------------------------------------------------------------------------------------------------------- poses
def flip_pose(c2w):
    """Columns 1 and 2 of the rotation part negated (every reader of the reference does this); float64 in, float32 tensor out."""
    c2w = np.array(c2w, dtype=np.float64).reshape(4, 4)
    c2w[:3, 1] *= -1
    c2w[:3, 2] *= -1
    return torch.from_numpy(c2w).float()


def quaternion_matrix(q):
    """3 x 3 rotation of the quaternion (x, y, z, w) of any non-zero length (the order of a TUM trajectory file)."""
    x, y, z, w = (float(v) for v in q)
    s = 2.0 / (x * x + y * y + z * z + w * w)
    return np.array([[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                     [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                     [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]], dtype=np.float64)


def read_tum_list(path, skip=0):
    """(stamps float64 [n], [the other fields of each line]) of a TUM list file: blank lines and '#' comments dropped, after `skip` lines."""
    stamps, rest = [], []
    with open(path) as f:
        for line in f.read().splitlines()[skip:]:
            line = line.split('#', 1)[0].split()
            if line:
                stamps.append(float(line[0]))
                rest.append(line[1:])
    return np.array(stamps, dtype=np.float64), rest


def associate_frames(t_image, t_depth, t_pose, max_dt=0.08):
    """[(i, j, k)]: for every image stamp the nearest depth and pose stamps, kept when both lie within max_dt (datasets.py:258-275)."""
    out = []
    for i, t in enumerate(t_image):
        j, k = int(np.argmin(np.abs(t_depth - t))), int(np.argmin(np.abs(t_pose - t)))
        if abs(t_depth[j] - t) < max_dt and abs(t_pose[k] - t) < max_dt:
            out.append((i, j, k))
    return out


def thin_frames(t_image, associations, frame_rate=32):
    """Indices into `associations` at most frame_rate per second apart (datasets.py:298-303)."""
    keep = [0] if associations else []
    for a in range(1, len(associations)):
        if t_image[associations[a][0]] - t_image[associations[keep[-1]][0]] > 1.0 / frame_rate:
            keep.append(a)
    return keep


# ---------------------------------------------------------------------------------------------------------------- decoding
def _image_module():
    try:
        from PIL import Image
    except ImportError as e:               # no quiet fall-back: a reader without a decoder is an error
        raise ImportError('loopy_slam_amd.datasets decodes frames with Pillow, which is not installed') from e
    return Image


def decode_color(path, out=None):
    """uint8 [H,W,3] R, G, B of an image file (into `out` when given)."""
    with _image_module().open(path) as im:
        if im.mode != 'RGB':
            im = im.convert('RGB')
        if out is None:
            return np.array(im)
        a = np.asarray(im)
        if a.shape != out.shape:
            raise ValueError(f'{path}: colour image of {a.shape}, the sequence started with {out.shape}')
        np.copyto(out, a)
        return out


def decode_depth(path, out=None):
    """uint16 [H,W] of a 16-bit PNG (into `out` when given)."""
    with _image_module().open(path) as im:
        a = np.asarray(im)
        if a.ndim != 2:
            raise ValueError(f'{path}: a depth map must have one channel, this has shape {a.shape}')
        if a.dtype != np.uint16:
            a = a.astype(np.uint16)
        if out is None:
            return np.array(a)
        if a.shape != out.shape:
            raise ValueError(f'{path}: depth map of {a.shape}, the sequence started with {out.shape}')
        np.copyto(out, a)
        return out


def image_size(path):
    with _image_module().open(path) as im:
        return im.size[1], im.size[0]


class _Slot:
    def __init__(self, color_shape, depth_shape, pin):
        self.color_t = torch.empty(color_shape, dtype=torch.uint8)
        self.depth_t = torch.empty(depth_shape, dtype=torch.int16)
        if pin:
            self.color_t, self.depth_t = self.color_t.pin_memory(), self.depth_t.pin_memory()
        self.color, self.depth = self.color_t.numpy(), self.depth_t.numpy().view(np.uint16)
        self.event = None


class Prefetcher:
    """One thread that decodes frames ahead of the caller into a ring of `depth + 1` host buffers.  get(i) -> a slot holding frame i, or None
    when frame i was not decoded ahead (the caller decodes it itself); the slot stays the caller's until release(slot)."""

    def __init__(self, color_paths, depth_paths, color_shape, depth_shape, depth, pin):
        self.color_paths, self.depth_paths, self.n = color_paths, depth_paths, len(color_paths)
        self.depth = depth
        self.free = [_Slot(color_shape, depth_shape, pin) for _ in range(depth + 1)]
        self.ready, self.errors = {}, {}
        self.cursor, self.target, self.busy = 0, -1, None        # next index to decode, last index wanted, index in the decoder now
        self.epoch = 0                                           # bumped when the caller jumps: a decode of the old epoch is dropped
        self.stop = False
        self.hits = self.misses = 0
        self.cond = threading.Condition()
        self.thread = threading.Thread(target=self._run, name='loopy-frame-decode', daemon=True)
        self.thread.start()

    def _run(self):
        while True:
            with self.cond:
                while not self.stop and not (self.cursor <= self.target and self.cursor < self.n and self.free):
                    self.cond.wait()
                if self.stop:
                    return
                i, epoch, slot = self.cursor, self.epoch, self.free.pop()
                self.cursor += 1
                self.busy = i
            err = None
            try:
                decode_color(self.color_paths[i], slot.color)
                decode_depth(self.depth_paths[i], slot.depth)
            except BaseException as e:               # handed to the caller of __getitem__(i); the thread goes on
                err = e
            with self.cond:
                self.busy = None
                if epoch != self.epoch or err is not None:
                    self.free.append(slot)
                    if epoch == self.epoch:
                        self.errors[i] = err
                else:
                    self.ready[i] = slot
                self.cond.notify_all()

    def get(self, i):
        with self.cond:
            # frame i is in the decoder, or is the very next one it will take: wait for it rather than decode it twice
            while (self.busy == i or (self.cursor == i and i <= self.target and self.free)) and not self.stop:
                self.cond.wait()
            err = self.errors.pop(i, None)
            slot = self.ready.pop(i, None)
            if err is None and slot is None:                     # not sequential: forget what was decoded ahead, start again behind i
                self.epoch += 1
                self.free.extend(self.ready.values())
                self.ready.clear()
                self.errors.clear()
                self.cursor = i + 1
                self.misses += 1
            elif err is None:
                self.hits += 1
            self.cursor = max(self.cursor, i + 1)
            self.target = i + self.depth
            self.cond.notify_all()
        if err is not None:
            raise err
        return slot

    def release(self, slot):
        if slot.event is not None:
            slot.event.synchronize()                             # its upload has long finished when the next frame is asked for
            slot.event = None
        with self.cond:
            self.free.append(slot)
            self.cond.notify_all()

    def close(self):
        with self.cond:
            self.stop = True
            self.cond.notify_all()
        if self.thread.is_alive() and self.thread is not threading.current_thread():
            self.thread.join()


# ---------------------------------------------------------------------------------------------------------------- readers
class BaseDataset:
    """len, [i] -> (i, color [H,W,3] float32 in [0,1], depth [H,W] float32 metres, c2w [4,4] float32) on the device (datasets.py:51-121)."""

    def __init__(self, cfg, args, device='cuda:0', eng=None):
        self.name = cfg['dataset']
        if eng is None:
            from . import core
            eng = core.Engine(device=device)
        self.eng, self.device = eng, eng.device
        cam = cfg['cam']
        self.png_depth_scale = cam['png_depth_scale']
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = cam['H'], cam['W'], cam['fx'], cam['fy'], cam['cx'], cam['cy']
        self.distortion = np.array(cam['distortion'], dtype=np.float64) if cam.get('distortion') is not None else None
        self.crop_size = cam.get('crop_size')
        folder = getattr(args, 'input_folder', None)
        self.input_folder = cfg['data']['input_folder'] if folder is None else folder
        self.crop_edge = cam.get('crop_edge', 0) or 0
        self.prefetch = int(cfg['data'].get('prefetch', 2) or 0)
        self.color_paths, self.depth_paths, self.poses = [], [], []
        self._fetcher = self._held = None
        self._dev = None

    def __len__(self):
        return self.n_img

    def _finish(self):
        """After a subclass has listed its files and poses."""
        self.n_img = len(self.color_paths)
        if len(self.depth_paths) != self.n_img or len(self.poses) < self.n_img:
            raise ValueError(f'{self.input_folder}: {self.n_img} colour images, {len(self.depth_paths)} depth maps, {len(self.poses)} poses')
        self.poses = self.poses[:self.n_img]
        self._poses_dev = torch.stack(self.poses).to(self.device) if self.n_img else None

    def _buffers(self):
        if self._dev is None:
            cs, ds = image_size(self.color_paths[0]) + (3,), image_size(self.depth_paths[0])
            undist = self.eng.empty(*cs, dtype=torch.uint8) if self.distortion is not None and self.distortion.any() else None
            self._dev = (self.eng.empty(*cs, dtype=torch.uint8), self.eng.empty(*ds, dtype=torch.int16), undist)
            if self.prefetch > 0:
                self._fetcher = Prefetcher(self.color_paths, self.depth_paths, cs, ds, self.prefetch, self.device.type == 'cuda')
        return self._dev

    def __getitem__(self, index):
        index = int(index)
        if not 0 <= index < self.n_img:
            raise IndexError(index)
        dev_color, dev_depth, undist = self._buffers()
        if self._held is not None:
            self._fetcher.release(self._held)
            self._held = None
        slot = self._fetcher.get(index) if self._fetcher is not None else None
        if slot is not None:
            color, depth = slot.color_t, slot.depth_t
        else:                                                    # decoded here; the arrays are wrapped, not copied
            color = torch.from_numpy(decode_color(self.color_paths[index]))
            depth = torch.from_numpy(decode_depth(self.depth_paths[index]).view(np.int16))
        if color.shape != dev_color.shape or depth.shape != dev_depth.shape:
            raise ValueError(f'frame {index}: {tuple(color.shape)} / {tuple(depth.shape)}, the sequence started with '
                             f'{tuple(dev_color.shape)} / {tuple(dev_depth.shape)}')
        dev_color.copy_(color, non_blocking=True)
        dev_depth.copy_(depth, non_blocking=True)
        if slot is not None:
            if self.device.type == 'cuda':
                slot.event = torch.cuda.Event()
                slot.event.record(torch.cuda.current_stream(self.device))
            self._held = slot
        out_color, out_depth = prepare_frame(self.eng, dev_color, dev_depth, self.png_depth_scale, self.fx, self.fy, self.cx, self.cy,
                                             self.distortion, self.crop_size, self.crop_edge, undist=undist)
        return index, out_color, out_depth, self._poses_dev[index].clone()

    def close(self):
        """Joins the decoding thread; the reader can be used again afterwards (the thread restarts on the next frame)."""
        if self._fetcher is not None:
            self._fetcher.close()
        self._fetcher = self._held = self._dev = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Replica(BaseDataset):
    """<folder>/results/frame*.jpg, depth*.png in lexical order; <folder>/traj.txt with the 16 numbers of a c2w per line."""

    def __init__(self, cfg, args, device='cuda:0', eng=None):
        super().__init__(cfg, args, device, eng)
        self.color_paths = sorted(glob.glob(os.path.join(self.input_folder, 'results', 'frame*.jpg')))
        self.depth_paths = sorted(glob.glob(os.path.join(self.input_folder, 'results', 'depth*.png')))
        self.load_poses(os.path.join(self.input_folder, 'traj.txt'))
        self._finish()

    def load_poses(self, path):
        with open(path) as f:
            lines = [ln for ln in f.read().splitlines() if ln.strip()]
        self.poses = [flip_pose([float(v) for v in ln.split()]) for ln in lines[:len(self.color_paths)]]


class Azure(BaseDataset):
    """<folder>/color/*.jpg, depth/*.png; scene/trajectory.log in records of five lines (ids and fitness, then a 4 x 4), identity poses without it."""

    def __init__(self, cfg, args, device='cuda:0', eng=None):
        super().__init__(cfg, args, device, eng)
        self.color_paths = sorted(glob.glob(os.path.join(self.input_folder, 'color', '*.jpg')))
        self.depth_paths = sorted(glob.glob(os.path.join(self.input_folder, 'depth', '*.png')))
        self.load_poses(os.path.join(self.input_folder, 'scene', 'trajectory.log'))
        self._finish()

    def load_poses(self, path):
        if not os.path.exists(path):
            self.poses = [torch.eye(4) for _ in self.color_paths]
            return
        with open(path) as f:
            content = f.read().splitlines()
        self.poses = [flip_pose([float(v) for v in ' '.join(content[i + 1:i + 5]).split()]) for i in range(0, len(content) - 4, 5)]


class ScanNet(BaseDataset):
    """<folder>/frames/color/N.jpg, depth/N.png, pose/N.txt in the order of the integer N."""

    def __init__(self, cfg, args, device='cuda:0', eng=None):
        super().__init__(cfg, args, device, eng)
        self.input_folder = os.path.join(self.input_folder, 'frames')

        def by_number(pattern):
            return sorted(glob.glob(os.path.join(self.input_folder, *pattern)), key=lambda p: int(os.path.splitext(os.path.basename(p))[0]))
        self.color_paths, self.depth_paths = by_number(('color', '*.jpg')), by_number(('depth', '*.png'))
        self.poses = []
        for p in by_number(('pose', '*.txt')):
            with open(p) as f:
                self.poses.append(flip_pose([float(v) for v in f.read().split()]))
        self._finish()


class TUM_RGBD(BaseDataset):
    """rgb.txt, depth.txt, groundtruth.txt or pose.txt ('stamp tx ty tz qx qy qz qw'): nearest stamps within 0.08 s, at most 32 frames per second,
    poses relative to the first frame kept (datasets.py:277-322).  The first line of the pose file is skipped, as the reference skips it."""

    def __init__(self, cfg, args, device='cuda:0', eng=None):
        super().__init__(cfg, args, device, eng)
        self.color_paths, self.depth_paths, self.poses = self.loadtum(self.input_folder, frame_rate=32)
        self._finish()

    @staticmethod
    def loadtum(datapath, frame_rate=-1):
        pose_list = os.path.join(datapath, 'groundtruth.txt')
        if not os.path.isfile(pose_list):
            pose_list = os.path.join(datapath, 'pose.txt')
        t_image, images = read_tum_list(os.path.join(datapath, 'rgb.txt'))
        t_depth, depths = read_tum_list(os.path.join(datapath, 'depth.txt'))
        t_pose, vecs = read_tum_list(pose_list, skip=1)
        assoc = associate_frames(t_image, t_depth, t_pose)
        color_paths, depth_paths, poses, inv_first = [], [], [], None
        for a in thin_frames(t_image, assoc, frame_rate):
            i, j, k = assoc[a]
            v = [float(x) for x in vecs[k][:7]]
            c2w = np.eye(4)
            c2w[:3, :3], c2w[:3, 3] = quaternion_matrix(v[3:7]), v[:3]
            if inv_first is None:
                inv_first = np.linalg.inv(c2w)
                c2w = np.eye(4)
            else:
                c2w = inv_first @ c2w
            color_paths.append(os.path.join(datapath, images[i][0]))
            depth_paths.append(os.path.join(datapath, depths[j][0]))
            poses.append(flip_pose(c2w))
        return color_paths, depth_paths, poses


dataset_dict = {'replica': Replica, 'scannet': ScanNet, 'azure': Azure, 'tumrgbd': TUM_RGBD}


def get_dataset(cfg, args, device='cuda:0', eng=None):
    name = cfg.get('dataset')
    if name not in dataset_dict:
        raise ValueError(f'dataset {name!r} has no reader here; supported: {", ".join(sorted(dataset_dict))} (cofusion needs an EXR decoder)')
    return dataset_dict[name](cfg, args, device=device, eng=eng)


def sequence_folder(cfg, args=None):
    """The folder a reader would open and whether it holds that reader's layout: (folder, readable)."""
    folder = getattr(args, 'input_folder', None)
    folder = (cfg.get('data') or {}).get('input_folder') if folder is None else folder
    name = cfg.get('dataset')
    if name not in dataset_dict or not folder or not os.path.isdir(folder):
        return folder, False
    has = {
        'replica': lambda: os.path.isfile(os.path.join(folder, 'traj.txt')) and bool(glob.glob(os.path.join(folder, 'results', 'frame*.jpg'))),
        'scannet': lambda: bool(glob.glob(os.path.join(folder, 'frames', 'color', '*.jpg'))),
        'azure': lambda: bool(glob.glob(os.path.join(folder, 'color', '*.jpg'))) and os.path.isdir(os.path.join(folder, 'depth')),
        'tumrgbd': lambda: all(os.path.isfile(os.path.join(folder, f)) for f in ('rgb.txt', 'depth.txt')) and any(
            os.path.isfile(os.path.join(folder, f)) for f in ('groundtruth.txt', 'pose.txt')),
    }[name]
    return folder, bool(has())


def open_sequence(cfg, args=None, eng=None):
    """The reader of cfg['dataset'] on data.input_folder (args.input_folder first), or None when that folder is not a sequence of its layout."""
    folder, ok = sequence_folder(cfg, args)
    return get_dataset(cfg, args, eng=eng) if ok else None
