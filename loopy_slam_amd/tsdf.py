"""TSDF fusion and marching-cubes meshing of a finished run (csrc/lk_tsdf.hip; include/loopy_hip.h "TSDF fusion and meshing").

Reference                                                       here
  src/tools/get_mesh_tsdf_fusion.py  o3d ScalableTSDFVolume       TSDFVolume.integrate  -> lk_tsdf_touch + lk_tsdf_integrate
  volume.extract_triangle_mesh()                                  TSDFVolume.extract_triangle_mesh -> lk_mc_mark / _vertices / _triangles
  o3d.io.write_triangle_mesh                                      write_ply
  src/neural_point.py  compute_tsdf (a segment's surface cloud)   fuse_segment + TSDFVolume.extract_point_cloud (loop_closure.cloud = 'tsdf')

The class owns every buffer as a torch tensor.  Blocks of 16^3 voxels live in slots in allocation order (existing data never moves inside
its slot); the sorted key array and the slot of each sorted key are rebuilt by a torch sort after each allocation.  Bookkeeping (unique,
sort, searchsorted, cumsum) is torch; everything that touches a pixel, a voxel or a vertex is a kernel.
"""
import ctypes as C
import os

import numpy as np
import torch

from ._ffi import ptr

BLOCK = 16
BLOCK_VOXELS = BLOCK ** 3
PLANES = 5
KEY_BIAS = 1 << 20
KEY_MASK = (1 << 21) - 1


def block_key(b):
    """int64 keys of integer block coordinates b[..., 3] (torch or numpy)."""
    return ((b[..., 0] + KEY_BIAS) << 42) | ((b[..., 1] + KEY_BIAS) << 21) | (b[..., 2] + KEY_BIAS)


def key_block(keys):
    """Block coordinates [..., 3] of int64 keys (torch)."""
    return torch.stack([((keys >> 42) & KEY_MASK) - KEY_BIAS, ((keys >> 21) & KEY_MASK) - KEY_BIAS, (keys & KEY_MASK) - KEY_BIAS], -1)


def _c2w16(c2w):
    m = np.ascontiguousarray(torch.as_tensor(c2w).detach().cpu().numpy(), dtype=np.float32).reshape(16)
    return (C.c_float * 16)(*m.tolist())


class TSDFVolume:
    """Sparse truncated signed distance volume with colour.  The defaults are the reference's (voxel 5/512 m, truncation 4 cm, depth cut at
    30 m); depth_stride is the pixel stride of the block allocation pass (Open3D's depth_sampling_stride)."""

    def __init__(self, eng, voxel_length=5.0 / 512.0, sdf_trunc=0.04, depth_trunc=30.0, depth_stride=4):
        self.eng = eng
        self.voxel_length, self.sdf_trunc, self.depth_trunc = float(voxel_length), float(sdf_trunc), float(depth_trunc)
        self.depth_stride = int(depth_stride)
        if not (self.voxel_length > 0 and self.sdf_trunc > 0 and self.depth_stride > 0):
            raise ValueError('TSDFVolume: voxel_length, sdf_trunc and depth_stride must be positive')
        if np.float32(2) * np.float32(self.sdf_trunc) > np.float32(BLOCK) * np.float32(self.voxel_length):
            raise ValueError(f'TSDFVolume: 2 * sdf_trunc ({2 * self.sdf_trunc}) exceeds a block of 16 voxels ({BLOCK * self.voxel_length}): '
                             f'a pixel could touch more than 8 blocks')
        self.n = 0
        self.keys = eng.zeros(0, dtype=torch.int64)                 # [n] key of every slot, allocation order
        self.planes = eng.zeros(0, PLANES, BLOCK_VOXELS)            # [capacity, 5, 4096]; slots [n, capacity) are zero
        self.sorted_keys = eng.zeros(0, dtype=torch.int64)
        self.sorted_slots = eng.zeros(0, dtype=torch.int32)         # slot of the block at each position of sorted_keys

    # ---------------------------------------------------------------------------------------- allocation
    def _lookup(self, keys):
        """(position in sorted_keys, present) of int64 keys."""
        if self.n == 0:
            return torch.zeros_like(keys), torch.zeros_like(keys, dtype=torch.bool)
        pos = torch.searchsorted(self.sorted_keys, keys).clamp(max=self.n - 1)
        return pos, self.sorted_keys[pos] == keys

    def allocate(self, keys):
        """Gives every key of the ascending, duplicate-free int64 tensor `keys` a slot; returns the slots [len(keys)] int32."""
        _, have = self._lookup(keys)
        new = keys[~have]
        k = int(new.shape[0])
        if k:
            if self.n + k > self.planes.shape[0]:
                cap = max(self.n + k, 2 * int(self.planes.shape[0]), 64)
                planes = self.eng.zeros(cap, PLANES, BLOCK_VOXELS)
                planes[:self.n] = self.planes[:self.n]
                self.planes = planes
            self.keys = torch.cat([self.keys, new])
            self.n += k
            self.sorted_keys, order = torch.sort(self.keys, stable=True)
            self.sorted_slots = order.to(torch.int32).contiguous()
        pos, _ = self._lookup(keys)
        return self.sorted_slots[pos].contiguous() if self.n else self.eng.zeros(0, dtype=torch.int32)

    # ---------------------------------------------------------------------------------------- fusion
    def touch(self, depth, c2w, fx, fy, cx, cy):
        """Ascending, duplicate-free keys of the blocks the depth image touches (lk_tsdf_touch + torch.unique)."""
        eng = self.eng
        depth = eng.f32(depth)
        H, W = int(depth.shape[0]), int(depth.shape[1])
        s = self.depth_stride
        n = ((H + s - 1) // s) * ((W + s - 1) // s)
        keys = eng.empty(n, 8, dtype=torch.int64)
        eng.lib.check(eng.lib.dll.lk_tsdf_touch(ptr(depth), H, W, _c2w16(c2w), C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy), s,
                                                C.c_float(self.depth_trunc), C.c_float(self.sdf_trunc), C.c_float(self.voxel_length),
                                                ptr(keys), eng.stream), 'lk_tsdf_touch')
        uniq = torch.unique(keys)
        return uniq[uniq >= 0]

    def integrate(self, depth, color, c2w, fx, fy, cx, cy):
        """Fuses one frame: depth [H,W] in metres (0 = no measurement), color [H,W,3] in [0, 1], c2w [4,4] in the project's camera
        convention.  Returns the keys of the blocks it integrated into (ascending)."""
        depth = self.eng.f32(depth)
        touched = self.touch(depth, c2w, fx, fy, cx, cy)
        self.integrate_blocks(touched, depth, color, c2w, fx, fy, cx, cy)
        return touched

    def integrate_blocks(self, keys, depth, color, c2w, fx, fy, cx, cy, slots=None):
        """The second half of integrate(): allocates the blocks `keys` (ascending, duplicate-free) and integrates the frame into them
        (lk_tsdf_integrate).  slots: what allocate(keys) returned, if the caller has it already (then this is the kernel launch alone)."""
        eng = self.eng
        depth, color = eng.f32(depth), eng.f32(color)
        H, W = int(depth.shape[0]), int(depth.shape[1])
        if tuple(color.shape) != (H, W, 3):
            raise ValueError(f'TSDFVolume.integrate: color {tuple(color.shape)} does not match depth {(H, W)}')
        slots = self.allocate(keys) if slots is None else slots
        eng.lib.check(eng.lib.dll.lk_tsdf_integrate(ptr(self.planes), ptr(self.keys), self.n, ptr(slots), int(slots.shape[0]), ptr(depth),
                                                    ptr(color), H, W, _c2w16(c2w), C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy),
                                                    C.c_float(self.voxel_length), C.c_float(self.sdf_trunc), C.c_float(self.depth_trunc),
                                                    eng.stream), 'lk_tsdf_integrate')

    @classmethod
    def from_dense(cls, eng, tsdf, weight, color, block_origin, voxel_length=5.0 / 512.0, sdf_trunc=0.04, **kw):
        """A volume filled from dense arrays indexed [x, y, z] (sizes multiples of 16; color [X,Y,Z,3] in 0 .. 255) whose voxel (0, 0, 0) is
        voxel (0, 0, 0) of block `block_origin`.  Blocks whose weights are all zero are not allocated."""
        vol = cls(eng, voxel_length, sdf_trunc, **kw)
        tsdf, weight, color = (torch.as_tensor(np.asarray(a), dtype=torch.float32) for a in (tsdf, weight, color))
        X, Y, Z = tsdf.shape
        if X % BLOCK or Y % BLOCK or Z % BLOCK or weight.shape != tsdf.shape or tuple(color.shape) != (X, Y, Z, 3):
            raise ValueError('TSDFVolume.from_dense: shapes must be [X,Y,Z] (multiples of 16) and [X,Y,Z,3]')
        nb = (X // BLOCK, Y // BLOCK, Z // BLOCK)
        dense = torch.cat([tsdf[..., None], weight[..., None], color], -1)                    # [X,Y,Z,5]
        # -> [bx,by,bz, plane, z,y,x]
        dense = dense.reshape(nb[0], BLOCK, nb[1], BLOCK, nb[2], BLOCK, PLANES).permute(0, 2, 4, 6, 5, 3, 1).reshape(-1, PLANES, BLOCK_VOXELS)
        grid = torch.stack(torch.meshgrid(*[torch.arange(k, dtype=torch.int64) for k in nb], indexing='ij'), -1).reshape(-1, 3)
        keys = block_key(grid + torch.as_tensor(block_origin, dtype=torch.int64))
        keep = (dense[:, 1] > 0).any(-1)
        keys, dense = keys[keep], dense[keep]
        keys, order = torch.sort(keys)
        slots = vol.allocate(keys.to(eng.device))
        vol.planes[slots.long()] = dense[order].to(eng.device)
        return vol

    # ---------------------------------------------------------------------------------------- meshing
    def neighbour_table(self):
        """[n, 8] int32: position (in sorted_keys) of the block at offset o = dx | dy << 1 | dz << 2 of every sorted block, -1 if absent."""
        b = key_block(self.sorted_keys)                                                       # [n,3]
        o = torch.arange(8, device=b.device)
        off = torch.stack([o & 1, (o >> 1) & 1, o >> 2], -1)                                  # [8,3]
        nb = b[:, None, :] + off[None]
        inside = (nb < KEY_BIAS).all(-1)
        pos, have = self._lookup(block_key(nb.clamp(max=KEY_BIAS - 1)).reshape(-1))
        pos = torch.where(have & inside.reshape(-1), pos, torch.full_like(pos, -1))
        return pos.reshape(-1, 8).to(torch.int32).contiguous()

    def _extract(self, triangles=True):
        eng, dll, n = self.eng, self.eng.lib.dll, self.n
        empty = {'vertices': eng.zeros(0, 3), 'colors': eng.zeros(0, 3), 'triangles': eng.zeros(0, 3, dtype=torch.int32),
                 'owners': eng.zeros(0, dtype=torch.int32)}
        if n == 0:
            return empty
        from .loop_closure import _compact
        nbr = self.neighbour_table()
        case, ntri = eng.empty(n * BLOCK_VOXELS, dtype=torch.uint8), eng.empty(n * BLOCK_VOXELS, dtype=torch.uint8)
        flag = eng.zeros(n * BLOCK_VOXELS * 3, dtype=torch.uint8)
        eng.lib.check(dll.lk_mc_mark(ptr(self.planes), ptr(self.sorted_slots), ptr(nbr), n, ptr(case), ptr(ntri), ptr(flag), eng.stream),
                      'lk_mc_mark')
        index, count = _compact(eng, flag)
        V = int(count.cpu()[0])
        if V == 0:
            return empty
        index = index[:V].contiguous()
        pos, col = eng.empty(V, 3), eng.empty(V, 3)
        eng.lib.check(dll.lk_mc_vertices(ptr(self.planes), ptr(self.keys), ptr(self.sorted_slots), ptr(nbr), n, ptr(index), V,
                                         C.c_float(self.voxel_length), ptr(pos), ptr(col), eng.stream), 'lk_mc_vertices')
        out = {'vertices': pos, 'colors': col, 'owners': index, 'triangles': empty['triangles']}
        if triangles:
            tri_end = torch.cumsum(ntri, 0, dtype=torch.int64)
            F = int(tri_end[-1].cpu())
            if 3 * F >= (1 << 31):
                raise ValueError('TSDFVolume: more than 2^31 / 3 triangles')
            tri_end = tri_end.to(torch.int32).contiguous()
            tri = eng.empty(F, 3, dtype=torch.int32)
            eng.lib.check(dll.lk_mc_triangles(ptr(self.sorted_slots), ptr(nbr), n, ptr(case), ptr(tri_end), ptr(index), V, ptr(tri),
                                              eng.stream), 'lk_mc_triangles')
            out['triangles'] = tri
        return out

    def extract_triangle_mesh(self):
        """{'vertices' [V,3] f32, 'colors' [V,3] f32 in [0, 1], 'triangles' [F,3] int32} on the device, plus 'owners' [V] int32: the cut
        edge each vertex sits on, (position of its block among the sorted keys * 4096 + voxel) * 3 + axis, ascending."""
        return self._extract(True)

    def extract_point_cloud(self):
        """The mesh's vertices and colours alone: {'vertices', 'colors'}."""
        m = self._extract(False)
        return {'vertices': m['vertices'], 'colors': m['colors']}


def write_ply(path, mesh):
    """Binary little-endian PLY: x y z float, red green blue uchar (colour * 255 rounded), faces as uchar count + int indices."""
    v = mesh['vertices'].detach().cpu().numpy().astype('<f4')
    c = np.clip(np.rint(mesh['colors'].detach().cpu().numpy().astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    t = mesh['triangles'].detach().cpu().numpy().astype('<i4')
    vert = np.empty(len(v), dtype=[('p', '<f4', 3), ('c', 'u1', 3)])
    vert['p'], vert['c'] = v, c
    face = np.empty(len(t), dtype=[('n', 'u1'), ('i', '<i4', 3)])
    face['n'], face['i'] = 3, t
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    header = ('ply\nformat binary_little_endian 1.0\ncomment loopy_slam_amd TSDF fusion\n'
              f'element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n'
              'property uchar red\nproperty uchar green\nproperty uchar blue\n'
              f'element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n')
    with open(path, 'wb') as f:
        f.write(header.encode('ascii'))
        f.write(vert.tobytes())
        f.write(face.tobytes())


# ------------------------------------------------------------------------------------------------ the mesh of a finished run
DEFAULTS = {'enabled': False, 'source': 'rendered', 'voxel_length': 5.0 / 512.0, 'sdf_trunc': 0.04}
SOURCES = ('rendered', 'sensor')


def settings(cfg):
    """cfg['meshing'] over the defaults (absent key: disabled)."""
    out = dict(DEFAULTS)
    out.update(cfg.get('meshing') or {})
    if out['source'] not in SOURCES:
        raise ValueError(f"meshing.source {out['source']!r}: one of {SOURCES}")
    return out


def scene_name(cfg):
    """The reference names the mesh after the last component of data.input_folder (get_mesh_tsdf_fusion.py)."""
    return os.path.basename(str(cfg['data'].get('input_folder', 'scene')).rstrip('/')) or 'scene'


def mesh_path(cfg, output=None):
    return os.path.join(output or cfg['data'].get('output', 'output'), 'mesh', f'{scene_name(cfg)}_pred_mesh.ply')


def rendered_frame(mapper, idx, gt_color, gt_depth, c2w):
    """Frame idx re-rendered from the final map at pose c2w, zero where the sensor has no depth (Mapper.py:1108-1115)."""
    from . import slam as _slam
    s, eng = mapper.slam, mapper.eng
    rq = None
    if mapper.use_dynamic_radius:
        rq = _slam.frame_radius_maps(eng, mapper.cfg, gt_color)[2].sqrt()
    xf = None
    if s.encode_exposure and mapper.exposure_feat_all:
        xf = mapper.exposure_feat_all[min(idx // mapper.every_frame, len(mapper.exposure_feat_all) - 1)].to(eng.device)
    depth, _, color = mapper.renderer.render_img(mapper.npc, mapper.decoders, c2w, eng.device, 'color', gt_depth=gt_depth,
                                                 dynamic_r_query=rq, exposure_feat=xf)
    depth = depth.float()
    depth[gt_depth == 0] = 0
    depth[~torch.isfinite(depth)] = 0
    return depth, color.float()


def fuse_run(mapper, n_frames, ms=None, save_dir=None, on_frame=None):
    """Every mapped frame (idx % every_frame == 0) below n_frames fused at its final estimate_c2w_list pose - loop-closure corrections and the
    final refinement included - from the re-rendered ('rendered') or the input ('sensor') depth and colour.  save_dir: the re-rendered frames
    are also kept there as depth_XXXXX.npy / color_XXXXX.npy (the reference's rendered_every_frame folder, Mapper.py:1116-1119: what
    tools/get_mesh_tsdf_fusion.py reads).  on_frame(idx, gt_color, gt_depth, depth, color) is called with every re-rendered frame (the
    rendering evaluation's hook: one render serves both).  Returns the volume."""
    s = mapper.slam
    ms = ms or settings(mapper.cfg)
    vol = TSDFVolume(mapper.eng, voxel_length=ms['voxel_length'], sdf_trunc=ms['sdf_trunc'])
    for idx in range(0, n_frames, mapper.every_frame):
        _, color, depth, _ = s.frame_reader[idx]
        c2w = s.estimate_c2w_list[idx].float()
        if not bool(torch.isfinite(c2w).all()):
            continue
        if ms['source'] == 'rendered':
            gt_color, gt_depth = color, depth
            depth, color = rendered_frame(mapper, idx, gt_color, gt_depth, c2w.to(mapper.eng.device))
            if on_frame is not None:
                on_frame(idx, gt_color, gt_depth, depth, color)
            if save_dir is not None:
                os.makedirs(save_dir, exist_ok=True)
                np.save(os.path.join(save_dir, f'depth_{idx:05d}'), depth.cpu().numpy())
                np.save(os.path.join(save_dir, f'color_{idx:05d}'), color.cpu().numpy())
        vol.integrate(depth, color, c2w, s.fx, s.fy, s.cx, s.cy)
    return vol


def pose_usable(c2w):
    """A pose a frame can be fused at: finite, and written at all - Point_SLAM.estimate_c2w_list starts as zeros, and a mapper driven without
    a tracker writes the mapped frames only (a rigid pose has a bottom row of 0 0 0 1)."""
    c2w = torch.as_tensor(c2w)
    return bool(torch.isfinite(c2w).all()) and float(c2w[3, 3]) == 1.0


def fuse_segment(eng, frames, poses, fx, fy, cx, cy, voxel_length=5.0 / 512.0, sdf_trunc=0.04):
    """The sensor frames of one map segment fused into a fresh volume at their poses (loop closure with `cloud: 'tsdf'`; the reference's
    compute_tsdf, src/neural_point.py:960-1017).  frames: an iterable of (depth [H,W], color [H,W,3]); poses: the c2w [4,4] of each.  The
    arithmetic of fuse_run(source='sensor'): the pose as fp32, one TSDFVolume.integrate per frame, in order.  A frame whose pose is not
    usable (pose_usable) is skipped.  Returns the volume."""
    vol = TSDFVolume(eng, voxel_length=voxel_length, sdf_trunc=sdf_trunc)
    for (depth, color), c2w in zip(frames, poses):
        c2w = torch.as_tensor(c2w).float()
        if not pose_usable(c2w):
            continue
        vol.integrate(depth, color, c2w, fx, fy, cx, cy)
    return vol


def mesh_run(mapper, n_frames, output=None, on_frame=None):
    """fuse_run + extract_triangle_mesh + write_ply to {output}/mesh/{scene}_pred_mesh.ply; returns (path, mesh)."""
    path = mesh_path(mapper.cfg, output)
    mesh = fuse_run(mapper, n_frames, save_dir=os.path.join(os.path.dirname(os.path.dirname(path)), 'rendered_every_frame'),
                    on_frame=on_frame).extract_triangle_mesh()
    write_ply(path, mesh)
    return path, mesh
