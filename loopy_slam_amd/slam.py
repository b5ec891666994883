"""Drop-in host classes with the reference's names and call signatures for the render/optimise path:

  NICER             src/conv_onet/models/decoder.py:549-626   (weights container + state_dict, forward)
  NeuralPointCloud  src/neural_point.py:29-124, 1252-1708     (query/store half; per-point segment ids when loop closure is on)
  Renderer          src/utils/Renderer.py:6-276               (render_batch_ray, render_img)
  Mapper            src/Mapper.py:35-1049                     (optimize_map; map_frame = one pass of run()'s body)
  Tracker           src/Tracker.py:29-427                     (optimize_cam_in_batch; track_frame = run()'s body)
  Point_SLAM        src/Point_SLAM.py:37-252                  (single-process orchestration)

All arithmetic of the hot path runs in libloopyhip (loopy_slam_amd.core / .steps / .optim); what remains here is
per-frame bookkeeping in torch.  Loop closure's geometric back end (segment registration, pose graph, map correction) is
loop_closure.py, off by default (cfg['loop_closure']['enabled']); the final mesh (TSDF fusion of the mapped frames + marching
cubes) is tsdf.py, off by default (cfg['meshing']['enabled']); the evaluation of the re-rendered frames and of the trajectory is
render_eval.py, off by default (cfg['rendering_eval']['enabled']); place recognition is place.py
(loop_closure.candidates: 'appearance'); the sequence readers are datasets.py; visualisation stays out of scope.  Every class takes an optional `eng` (core.Engine);
the default is the gfx950 library on the current CUDA device.
"""
import math
import os
import types

import numpy as np
import torch

from . import _ffi, core, datasets, loop_closure, odometry, optim, parallel, steps, synthetic
from .common import get_camera_from_tensor, get_tensor_from_camera, get_rays, get_samples, get_rays_from_uv


def _inv_pose(c2w, device):
    """world->camera of 4x4 poses ([4,4] or [K,4,4]) on `device`, no host round trip.  The reference inverts the general
    matrix (np.linalg.inv / torch.inverse, Mapper.py:173, 247); estimated and ground-truth poses are rigid, so the inverse is
    [R^T | -R^T t] - a transpose and one small product instead of a solver launch chain per keyframe; evaluated in float64
    it agrees with the general inverse to the float32 rounding of the result (tests/test_slam_api.py)."""
    c = c2w.detach().to(device=device, dtype=torch.float64)
    Rt = c[..., :3, :3].transpose(-1, -2)
    w2c = torch.zeros_like(c)
    w2c[..., :3, :3] = Rt
    w2c[..., :3, 3] = -(Rt @ c[..., :3, 3:4])[..., 0]
    w2c[..., 3, 3] = 1.0
    return w2c.float()


def render_cfg_from(cfg, coef):
    r, p = cfg['rendering'], cfg['pointcloud']
    return core.RenderCfg(S=r['N_surface'], near_surface=r['near_end_surface'], far_surface=r['far_end_surface'],
                          near_end=r['near_end'], coef=coef, min_nn=p['min_nn_num'], radius_query=p['radius_query'],
                          rel_pos=cfg['model']['encode_rel_pos_in_col'], exposure=cfg['model']['encode_exposure'])


# ============================================================================================ NICER
class _SubDecoder:
    """View of one decoder's entries ('geo_decoder.' / 'color_decoder.') for load_state_dict / state_dict."""

    def __init__(self, owner, prefix):
        self.owner, self.prefix = owner, prefix

    def state_dict(self):
        return {k[len(self.prefix):]: v for k, v in self.owner.state_dict().items() if k.startswith(self.prefix)}

    def load_state_dict(self, sd, strict=True):
        return self.owner.load_state_dict({self.prefix + k: v for k, v in sd.items()}, strict=strict, _only_prefix=self.prefix)

    def parameters(self):
        return [v for k, v in self.owner.state_dict().items() if k.startswith(self.prefix)]


class NICER:
    """MLP_geometry (hidden 32) + MLP_color (hidden 128) as one packed weight blob on the device."""

    # reference parameters that exist but never influence an output (kept only for state_dict round trips)
    _UNUSED = {'geo_decoder.embedder_rel_pos._B': (3, 10), 'geo_decoder.mlp_col_neighbor.linear1.weight': (32, 52),
               'geo_decoder.mlp_col_neighbor.linear1.bias': (32,), 'geo_decoder.mlp_col_neighbor.linear2.weight': (32, 32),
               'geo_decoder.mlp_col_neighbor.linear2.bias': (32,)}

    def __init__(self, cfg, eng=None, dim=3, c_dim=32, hidden_size=128, pos_embedding_method='fourier',
                 use_view_direction=False):
        assert c_dim == 32 and hidden_size == 128 and dim == 3, 'kernels are built for c_dim 32 / hidden 128'
        self.cfg = cfg
        self.eng = eng if eng is not None else core.Engine()
        self.dec = core.DecoderBlob(self.eng)
        seed = cfg.get('setup_seed', 1219)
        W = synthetic.default_weights(seed, rel_pos=cfg['model']['encode_rel_pos_in_col'])
        self.dec.pack(W)
        g = torch.Generator().manual_seed(seed + 1)
        self.extra = {k: torch.randn(*s, generator=g) * 0.01 for k, s in self._UNUSED.items()}
        self.encode_exposure = cfg['model']['encode_exposure']
        if self.encode_exposure:      # MLP_exposure (decoder.py:326-342): 8 -> 128 softplus(100) -> 12, N(0, 0.01) weights
            self.mlp_exposure = torch.nn.Sequential(torch.nn.Linear(cfg['model']['exposure_dim'], 128), torch.nn.Softplus(beta=100),
                                                    torch.nn.Linear(128, 12)).to(self.eng.device)
            with torch.no_grad():
                self.mlp_exposure[0].weight.normal_(0, 0.01, generator=None)
                self.mlp_exposure[2].weight.normal_(0, 0.01, generator=None)
        self.geo_decoder = _SubDecoder(self, 'geo_decoder.')
        self.color_decoder = _SubDecoder(self, 'color_decoder.')

    # ---- state_dict with the reference's key names
    def state_dict(self):
        sd = {k: v for k, v in self.dec.unpack().items() if k != 'color_decoder.embedder._B'}
        sd.update({k: v.clone() for k, v in self.extra.items()})
        if self.encode_exposure:
            sd['color_decoder.mlp_exposure.linear1.weight'] = self.mlp_exposure[0].weight.detach().cpu()
            sd['color_decoder.mlp_exposure.linear1.bias'] = self.mlp_exposure[0].bias.detach().cpu()
            sd['color_decoder.mlp_exposure.linear2.weight'] = self.mlp_exposure[2].weight.detach().cpu()
            sd['color_decoder.mlp_exposure.linear2.bias'] = self.mlp_exposure[2].bias.detach().cpu()
        return sd

    def load_state_dict(self, sd, strict=True, _only_prefix=None):
        cur = self.dec.unpack()
        known = set(cur) | set(self.extra)
        unexpected = [k for k in sd if k not in known and 'mlp_exposure' not in k]
        missing = [k for k in known if k not in sd and k != 'color_decoder.embedder._B'
                   and (_only_prefix is None or k.startswith(_only_prefix))]
        if strict and (unexpected or missing):
            raise RuntimeError(f'load_state_dict: missing {missing}, unexpected {unexpected}')
        for k, v in sd.items():
            if (k in cur and tuple(torch.as_tensor(v).shape) != tuple(cur[k].shape)) or \
                    (k in self.extra and tuple(torch.as_tensor(v).shape) != tuple(self.extra[k].shape)):
                # torch raises on a size mismatch with or without `strict` (torch.nn.Module.load_state_dict)
                raise RuntimeError(f'load_state_dict: size mismatch for {k}: {tuple(torch.as_tensor(v).shape)} in the checkpoint, '
                                   f'{tuple((cur[k] if k in cur else self.extra[k]).shape)} in the model')
        for k, v in sd.items():
            if k in cur:
                cur[k] = torch.as_tensor(v).float()
            elif k in self.extra:
                self.extra[k] = torch.as_tensor(v).float().clone()
            elif 'mlp_exposure' in k and self.encode_exposure:
                mod = self.mlp_exposure[0] if 'linear1' in k else self.mlp_exposure[2]
                getattr(mod, 'weight' if k.endswith('weight') else 'bias').data.copy_(torch.as_tensor(v))
        self.dec.pack(cur)
        return types.SimpleNamespace(missing_keys=missing, unexpected_keys=unexpected)

    def set_color_embedder_B(self, B):
        """The colour decoder's fixed random Fourier matrix is not in the reference's state_dict (decoder.py:32)."""
        cur = self.dec.unpack()
        cur['color_decoder.embedder._B'] = torch.as_tensor(B).float()
        self.dec.pack(cur)

    def color_embedder_B(self):
        return self.dec.unpack()['color_decoder.embedder._B'].clone()

    def to(self, device):
        return self

    def share_memory(self):
        return self

    def exposure_affine(self, exposure_feat):
        return self.mlp_exposure(exposure_feat) if (self.encode_exposure and exposure_feat is not None) else None

    def forward(self, p, npc, stage, npc_geo_feats, npc_col_feats, pts_num=16, is_tracker=False, cloud_pos=None,
                pts_views_d=None, dynamic_r_query=None, exposure_feat=None):
        """raw [P,4] (rgb, occupancy), ray_mask [P/pts_num], point_mask [P] for arbitrary query points
        (decoder.py:573-610).  Forward only; the differentiable path is Renderer.render_batch_ray."""
        eng = self.eng
        p = p.reshape(-1, 3).float().contiguous()
        P = p.shape[0]
        cfg = render_cfg_from(self.cfg, 0.1)
        cfg.S = 1                                   # one "sample" per zero-length ray: p = o + 0 * z
        st = core.RenderState(eng, P, 1)
        zeros, ones = torch.zeros_like(p), torch.ones(P, device=p.device)
        r2 = (dynamic_r_query.reshape(-1).double() ** 2).float().contiguous() if dynamic_r_query is not None else None
        aff = self.exposure_affine(exposure_feat)
        logits = self.encode_exposure and exposure_feat is None
        core.render_forward(eng, cfg, st, p, zeros, ones, npc.knn, npc.cloud_pos(), npc_geo_feats, npc_col_feats, self.dec,
                            'color' if stage in ('color', 'mesh', 'color_only') else 'geometry', tracker=is_tracker, r2_ray=r2,
                            affine=aff.detach().contiguous() if aff is not None else None, color_logits=logits)
        point_mask = st.nbr_count >= cfg.min_nn
        S = self.cfg['rendering']['N_surface']
        ray_mask = point_mask.view(-1, pts_num).sum(1) >= int(S / 2 + 1) if P % pts_num == 0 else None
        return st.raw.clone(), ray_mask, point_mask

    __call__ = forward


# ============================================================================================ NeuralPointCloud
class NeuralPointCloud:
    """Tensor-resident neural point cloud: positions, geometry / colour feature tables, exact grid index."""

    def __init__(self, cfg, slam=None, args=None, eng=None, capacity=1 << 18):
        self.cfg = cfg
        self.eng = eng if eng is not None else core.Engine()
        pc = cfg['pointcloud']
        self.c_dim = cfg['model']['c_dim']
        self.nn_num, self.N_add = pc['nn_num'], pc['N_add']
        assert self.nn_num == 8 and self.c_dim == 32
        self.radius_add, self.radius_min, self.radius_query = pc['radius_add'], pc['radius_min'], pc['radius_query']
        self.radius_mesh = pc.get('radius_mesh', pc['radius_query'])
        self.near_end_surface, self.far_end_surface = pc['near_end_surface'], pc['far_end_surface']
        self.use_dynamic_radius = cfg['use_dynamic_radius']
        # storage format of the two feature tables: 'float32' (the reference), or opt-in 'float16' (BASELINE config 5: half the bytes
        # of a whole-map optimisation; every value computed from the tables and every gradient stays fp32, Adam steps in fp32 and
        # rounds the stored value to nearest - LK_FLAG_FEATS_F16)
        self.feat_dtype = {'float32': torch.float32, 'float16': torch.float16}[pc.get('feature_dtype', 'float32')]
        self._cell = max(pc['radius_query'], 1e-3)
        # feature initialisation draws on the device (Philox): no host RNG + upload per insertion
        self._gen = torch.Generator(device=self.eng.device).manual_seed(cfg.get('setup_seed', 1219))
        # loop closure (loop_closure.LoopCloser attaches itself): the closer and the segment id of every row, one int32 beside _pos.
        # Both stay None with the feature off - nothing is allocated and nothing is called
        self.closer, self._seg = None, None
        self._alloc(capacity)
        self.n = 0
        self._input_pos, self._input_rgb = [], []

    def _alloc(self, cap):
        e = self.eng
        self.capacity = int(cap)
        self._pos = e.zeros(cap, 3)
        self._geo, self._col = e.zeros(cap, 32, dtype=self.feat_dtype), e.zeros(cap, 32, dtype=self.feat_dtype)
        self.knn = core.KnnIndex(e, self.capacity, cell_size=self._cell)

    def _grow(self, need):
        if need <= self.capacity:
            return
        old = (self._pos, self._geo, self._col)
        self._alloc(max(need, 2 * self.capacity))
        for new, o in zip((self._pos, self._geo, self._col), old):
            new[:self.n] = o[:self.n]
        if self._seg is not None:
            seg = torch.zeros(self.capacity, dtype=torch.int32, device=self.eng.device)
            seg[:self.n] = self._seg[:self.n]
            self._seg = seg
        if self.n:
            self.knn.build(self._pos[:self.n])

    # ---- accessors with the reference's names (neural_point.py:1328-1546)
    def device(self):
        return self.eng.device

    def cloud_pos(self):
        return self._pos[:self.n]

    def get_cloud_pos(self, end=False):
        return self._pos[:self.n]

    def get_geo_feats(self, end=False):
        return self._geo[:self.n]

    def get_col_feats(self, end=False):
        return self._col[:self.n]

    def update_geo_feats(self, feats, indices=None, end=False):
        if indices is not None:
            self._geo[:self.n][torch.as_tensor(indices, device=self.eng.device).long()] = feats.detach().to(self.feat_dtype)
        elif feats.data_ptr() != self._geo.data_ptr():
            self._geo[:self.n] = feats.detach().to(self.feat_dtype)

    def update_col_feats(self, feats, indices=None, end=False):
        if indices is not None:
            self._col[:self.n][torch.as_tensor(indices, device=self.eng.device).long()] = feats.detach().to(self.feat_dtype)
        elif feats.data_ptr() != self._col.data_ptr():
            self._col[:self.n] = feats.detach().to(self.feat_dtype)

    def pts_num(self):
        return self.n

    def index_ntotal(self):
        return self.n

    def get_radius_query(self):
        return self.radius_query

    def input_pos(self):
        return torch.cat(self._input_pos) if self._input_pos else self.eng.zeros(0, 3)

    def input_rgb(self):
        return torch.cat(self._input_rgb) if self._input_rgb else self.eng.zeros(0, 3)

    # ---- search (neural_point.py:1659-1708)
    def find_neighbors_faiss(self, pos, step='add', retrain=False, is_pts_grad=False, dynamic_radius=None):
        assert step in ('add', 'query', 'mesh')
        radius = self.radius_query if step == 'query' else (self.radius_mesh if step == 'mesh' else
                                                            (self.radius_min if is_pts_grad else self.radius_add))
        pos = pos.reshape(-1, 3).float().contiguous()
        if dynamic_radius is not None and dynamic_radius.numel() == pos.shape[0]:
            r2 = (dynamic_radius.reshape(-1).double() ** 2).float().contiguous()
        else:
            r2 = float(np.float32(radius ** 2))
        D, I, cnt = self.knn.query(pos, r2)
        return D, I.long(), cnt

    def sample_near_pcl(self, rays_o, rays_d, near, far, num):
        """For rays without a depth reading: sample between the first two probe depths (of 25 between near and far) that
        have a cloud point within radius_query (neural_point.py:1734-1786).  Returns (z [n, num] f32, invalid [n] bool).
        The probes go through the device kNN; disabled in every reference config (sample_near_pcl: False)."""
        ro, rd = rays_o.reshape(-1, 3).float(), rays_d.reshape(-1, 3).float()
        n, intervals = rd.shape[0], 25
        far = float(far)
        zp = torch.linspace(near, far, steps=intervals, device=ro.device)
        pts = (ro[:, None, :] + rd[:, None, :] * zp[None, :, None]).reshape(-1, 3).contiguous()
        _, _, cnt = self.find_neighbors_faiss(pts, step='query')
        sup = (cnt.reshape(n, intervals) > 0).cpu().numpy()
        invalid = sup.sum(-1) < 2
        sect = np.linspace(near, far, intervals)
        z = np.tile(np.linspace(near, far, num), (n, 1))
        for r in np.nonzero(~invalid)[0]:
            c = np.nonzero(sup[r])[0]
            z[r] = np.linspace(sect[c[0]], sect[c[1]], num=num)
        return torch.from_numpy(z).float().to(ro.device), torch.from_numpy(invalid).to(ro.device)

    # ---- insertion (neural_point.py:1557-1631): radius de-dup against the existing cloud, N_add points per ray
    def add_neural_points(self, batch_rays_o, batch_rays_d, batch_gt_depth, batch_gt_color, train=False, is_pts_grad=False,
                          dynamic_radius=None, idx=None, gt_color=None, gt_depth=None, cur_c2w=None, gt_camera=None):
        if batch_rays_o.shape[0] == 0:
            return 0
        ro, rd, gd = batch_rays_o.float().contiguous(), batch_rays_d.float().contiguous(), batch_gt_depth.float().contiguous()
        radius = self.radius_min if is_pts_grad else self.radius_add
        if dynamic_radius is not None and dynamic_radius.numel() == gd.shape[0]:
            r2 = (dynamic_radius.reshape(-1).double() ** 2).float().contiguous()
        else:
            r2 = float(np.float32(radius ** 2))
        # radius test against the existing cloud, compaction and the N_add points per accepted ray: lk_add_points
        acc, pts = optim.add_points(self.eng, self.knn if self.n > 0 else None, ro, rd, gd, r2, self.near_end_surface,
                                    self.far_end_surface, self.N_add)
        accl = acc.long()
        self._input_pos.append(ro[accl] + rd[accl] * gd[accl, None])
        self._input_rgb.append(batch_gt_color[accl] * 255)
        n_acc = acc.shape[0]
        k = pts.shape[0]
        if k:
            self._grow(self.n + k)
            self._pos[self.n:self.n + k] = pts
            if self._seg is not None:
                self._seg[self.n:self.n + k] = self.closer.current_segment
            # neural_point.py:1608-1614: normal(0, 0.1) features for the new points
            self._geo[self.n:self.n + k] = (torch.randn(k, 32, generator=self._gen, device=self.eng.device) * 0.1).to(self.feat_dtype)
            self._col[self.n:self.n + k] = (torch.randn(k, 32, generator=self._gen, device=self.eng.device) * 0.1).to(self.feat_dtype)
            self.n += k
            self.knn.build(self._pos[:self.n])             # counting-sort rebuild on the device (no IVF re-training)
        return n_acc

    # ---- loop closure (neural_point.py:144-215, 585-990): the reference's names, forwarded to the closer
    def compute_correction(self, segments):
        if self.closer is None:
            raise RuntimeError("loop closure is off: set cfg['loop_closure']['enabled']")
        return self.closer.compute_correction(segments)

    def apply_correction(self, pose_graph, segments, estimate_c2w_list=None, keyframe_dict=None, n_frames=None):
        if self.closer is None:
            raise RuntimeError("loop closure is off: set cfg['loop_closure']['enabled']")
        return self.closer.apply(pose_graph, segments, estimate_c2w_list, keyframe_dict, n_frames)


# ============================================================================================ Renderer
class _RenderFn(torch.autograd.Function):
    """autograd bridge: forward = lk_render_fwd, backward = lk_render_bwd."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, geo_feats, col_feats, blob, affine, pack):
        eng, cfg, knn, pos, dec, gt_depth, stage, tracker, r2, logits, chunk, z_given = pack
        R = rays_o.shape[0]
        st = core.RenderState(eng, R, cfg.S, need_act=True)
        core.render_forward(eng, cfg, st, rays_o.detach().contiguous(), rays_d.detach().contiguous(), gt_depth, knn, pos,
                            geo_feats.detach(), col_feats.detach(), dec, stage, tracker=tracker, r2_ray=r2,
                            affine=affine.detach().contiguous() if affine is not None else None, color_logits=logits,
                            save_act=True, stats_chunk=chunk, z_given=z_given)
        ctx.pack, ctx.st = pack, st
        ctx.needs = (rays_o.requires_grad or rays_d.requires_grad, geo_feats.requires_grad or col_feats.requires_grad,
                     blob.requires_grad, affine is not None and affine.requires_grad)
        ctx.N = geo_feats.shape[0]
        ctx.feat_dtype = geo_feats.dtype
        ctx.mark_non_differentiable(st.valid_ray)
        return st.depth, st.var, st.color, st.valid_ray

    @staticmethod
    def backward(ctx, g_depth, g_var, g_color, _):
        eng, cfg, knn, pos, dec = ctx.pack[:5]
        rays, feats, weights, aff = ctx.needs
        R = ctx.st.R
        gs = core.GradState(eng, ctx.N, R, dec.n, feats=feats, weights=weights, rays=rays, affine=aff)
        z = lambda t, *s: eng.zeros(*s) if t is None else t.contiguous()
        core.render_backward(eng, ctx.st, gs, z(g_depth, R), z(g_color, R, 3), z(g_var, R))
        cast = (lambda t: t) if ctx.feat_dtype == torch.float32 else (lambda t: None if t is None else t.to(ctx.feat_dtype))   # half tables
        return (gs.g_rays_o, gs.g_rays_d, cast(gs.g_geo), cast(gs.g_col), gs.g_weights, gs.g_affine, None)


class Renderer:
    def __init__(self, cfg, args=None, slam=None, points_batch_size=500000, ray_batch_size=3000):
        self.cfg = cfg
        self.ray_batch_size, self.points_batch_size = ray_batch_size, points_batch_size
        self.N_surface = cfg['rendering']['N_surface']
        self.use_dynamic_radius = cfg['use_dynamic_radius']
        self.sigmoid_coefficient = cfg['rendering']['sigmoid_coef_mapper']     # set externally like the reference
        # off in every reference config (replica/tum/scannet.yaml): depth-less rays then sample where the cloud is (Renderer.py:152-160)
        self.sample_near_pcl = bool(cfg['rendering'].get('sample_near_pcl', False))
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy
        self.dist = getattr(slam, 'dist', None)       # parallel.DistContext or None: render_img shares its rays out over the ranks

    def render_batch_ray(self, npc, decoders, rays_d, rays_o, device, stage, gt_depth=None, npc_geo_feats=None,
                         npc_col_feats=None, is_tracker=False, cloud_pos=None, dynamic_r_query=None, exposure_feat=None,
                         _stats_chunk=None):
        """(depth [R], uncertainty [R], color [R,3], valid_ray_mask [R] bool) — Renderer.py:71-201."""
        eng = decoders.eng
        cfg = render_cfg_from(self.cfg, self.sigmoid_coefficient)
        R = rays_o.shape[0]
        if gt_depth is None:
            gt_depth = eng.zeros(R)
        gt_depth = gt_depth.reshape(-1).float().contiguous()
        geo = npc_geo_feats if npc_geo_feats is not None else npc.get_geo_feats()
        col = npc_col_feats if npc_col_feats is not None else npc.get_col_feats()
        pos = cloud_pos if cloud_pos is not None else npc.cloud_pos()
        r2 = (dynamic_r_query.reshape(-1).double() ** 2).float().contiguous() if (self.use_dynamic_radius and dynamic_r_query is not None) else None
        aff = decoders.exposure_affine(exposure_feat)
        logits = decoders.encode_exposure and exposure_feat is None
        blob = decoders.dec.blob
        z_given, not_near = None, None
        if self.sample_near_pcl and bool((gt_depth <= 0).any()):
            # Renderer.py:102-122, 152-160: far of the batch, then the probe of the cloud along the rays without a reading (host round
            # trips as in the reference: this path is off in every config); their rows of z go to the sampler (LK_FLAG_Z_GIVEN)
            far_bb = torch.minimum(5 * gt_depth.mean(), torch.max(gt_depth * 1.2))
            far = torch.clamp(far_bb, 0, torch.max(gt_depth * 1.2)) if float(gt_depth.max()) > 0 else far_bb
            zero = torch.nonzero(gt_depth <= 0).reshape(-1)
            z0, inv = npc.sample_near_pcl(rays_o[zero].detach(), rays_d[zero].detach(), cfg.near_end, float(far), cfg.S)
            z_given = eng.zeros(R, cfg.S)
            z_given[zero] = z0
            not_near = zero[inv]
        pack = (eng, cfg, npc.knn, pos.contiguous(), decoders.dec, gt_depth, stage, is_tracker, r2, logits, _stats_chunk, z_given)
        depth, var, color, valid = _RenderFn.apply(rays_o.float(), rays_d.float(), geo, col, blob, aff, pack)
        valid = valid.bool()
        if not_near is not None and not_near.numel():
            valid = valid.clone()
            valid[not_near] = False                       # valid_ray_mask & mask_rays_near_pcl (Renderer.py:194-195)
        return depth, var, color, valid

    def render_img(self, npc, decoders, c2w, device, stage, gt_depth=None, npc_geo_feats=None, npc_col_feats=None,
                   dynamic_r_query=None, cloud_pos=None, exposure_feat=None):
        """Whole image in ONE fused pass over all H*W rays (the reference loops over 3000-ray batches,
        Renderer.py:241-266); far_bb is still evaluated per ray_batch_size group."""
        with torch.no_grad():
            ro, rd = get_rays(self.H, self.W, self.fx, self.fy, self.cx, self.cy, c2w, device)
            ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
            gd = gt_depth.reshape(-1) if gt_depth is not None else None
            rq = dynamic_r_query.reshape(-1) if dynamic_r_query is not None else None
            n = ro.shape[0]
            dist = self.dist if (self.dist is not None and self.dist.world > 1) else None
            # multi-GPU: every rank renders ONE contiguous range of whole ray_batch_size groups, then the ranges are exchanged
            lo, hi = parallel.ray_range(n, dist.rank, dist.world, self.ray_batch_size) if dist is not None else (0, n)
            sl = slice(lo, hi)
            if hi > lo:
                d, u, c, _ = self.render_batch_ray(npc, decoders, rd[sl], ro[sl], device, stage, gt_depth=gd[sl] if gd is not None else None,
                                                   npc_geo_feats=npc_geo_feats, npc_col_feats=npc_col_feats, cloud_pos=cloud_pos,
                                                   dynamic_r_query=rq[sl] if rq is not None else None, exposure_feat=exposure_feat,
                                                   _stats_chunk=self.ray_batch_size)
            if dist is not None:
                full = [torch.zeros(n, device=ro.device), torch.zeros(n, device=ro.device), torch.zeros(n, 3, device=ro.device)]
                if hi > lo:
                    full[0][sl], full[1][sl], full[2][sl] = d, u, c
                d, u, c = dist.gather_ranges(full, lo, hi)
            return d.double().reshape(self.H, self.W), u.double().reshape(self.H, self.W), c.reshape(self.H, self.W, 3)


# ============================================================================================ Mapper
class Mapper:
    def __init__(self, cfg, args, slam):
        self.cfg, self.slam = cfg, slam
        self.eng = slam.eng
        m = cfg['mapping']
        self.npc, self.decoders, self.renderer = slam.npc, slam.shared_decoders, slam.renderer_map
        self.renderer.sigmoid_coefficient = cfg['rendering']['sigmoid_coef_mapper']
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy
        self.every_frame, self.keyframe_every = m['every_frame'], m['keyframe_every']
        self.mapping_pixels, self.pixels_adding = m['pixels'], m['pixels_adding']
        self.num_joint_iters, self.iters_first = m['iters'], m['iters_first']
        self.geo_iter_ratio, self.geo_iter_first, self.min_iter_ratio = m['geo_iter_ratio'], m['geo_iter_first'], m['min_iter_ratio']
        self.mapping_window_size, self.w_color_loss = m['mapping_window_size'], m['w_color_loss']
        self.frustum_feature_selection, self.frustum_edge = m['frustum_feature_selection'], m['frustum_edge']
        self.filter_before_add_points = m['filter_before_add_points']
        self.pixels_based_on_color_grad = m.get('pixels_based_on_color_grad', 0)
        self.color_refine, self.fix_color_decoder = m.get('color_refine', False), m.get('fix_color_decoder', False)
        self.fix_geo_decoder = m.get('fix_geo_decoder', True)       # False: the geometry decoder's matrices are trained too (Mapper.py:524-526)
        self.keyframe_selection_method = m.get('keyframe_selection_method', 'overlap')
        # bundle adjustment (Mapper.py:82-83, 957-962): off until the run has more than four keyframes, then as the config says
        self.BA, self.BA_cfg, self.BA_cam_lr, self.ckpt_freq = False, m.get('BA', False), m.get('BA_cam_lr', 0.0002), m.get('ckpt_freq', 500)
        self.keep_refine_settings = False       # the reference leaves the refinement settings on (its mapper exits right after)
        self.logger = None                      # slam.Logger, attached by the caller that wants checkpoints
        self.last_add_counts, self.last_frame_pts_add, self.last_num_joint_iters = [], 0, 0
        self.use_dynamic_radius = cfg['use_dynamic_radius']
        self.keyframe_list, self.keyframe_dict = [], []
        # SEGMENTS (the reference's map fragments, neural_point.py:1300-1326): loop closure registers them against each other when it is on
        # (self.closer below), and the end-of-sequence refinement optimises over ONE KEYFRAME PER SEGMENT (Mapper.py:386-396, neural_point.py:1424-1433) - so
        # the segmentation of the trajectory is kept: a segment starts at frame 0 and at every mapped frame whose tracked pose has left the
        # last segment's keyframe pose by more than segment_rel_trans metres or whose optical axis makes a cosine below segment_rot_cos
        # with it (segment_strategy 'rot_trans'; 'fixed': every fixed_segment_size frames).  `segments` is a plain list of
        # {idx, color, depth, est_c2w, r2_query, exposure_feat} records: a caller that runs its own segmentation may replace or extend it
        # before the last frame is mapped
        self.segments = []
        # loop closure (loop_closure.py; off unless cfg['loop_closure']['enabled']): when a segment opens, its candidate pairs are registered,
        # the segment pose graph is optimised and map, poses and keyframes are moved - where the reference calls apply_transformation
        self.closer = loop_closure.LoopCloser(cfg, self.npc, slam) if loop_closure.settings(cfg)['enabled'] else None
        # final mesh (tsdf.py; off unless cfg['meshing']['enabled'], and then imported at the end of run()): TSDF fusion of the mapped frames
        self.meshing = bool((cfg.get('meshing') or {}).get('enabled'))
        self.mesh_file = None
        if self.meshing and getattr(getattr(slam, 'dist', None), 'world', 1) > 1:
            raise NotImplementedError('meshing.enabled with world > 1: the fusion runs on one rank - mesh the checkpoint afterwards '
                                      '(tools/get_mesh_tsdf_fusion.py)')
        # rendering evaluation (render_eval.py; off unless cfg['rendering_eval']['enabled']): at the end of run() the mapped frames are
        # re-rendered and measured against the input (depth L1, PSNR, MS-SSIM), with the ATE of the trajectory, into eval/rendering.json
        self.rendering_eval = bool((cfg.get('rendering_eval') or {}).get('enabled'))
        self.eval_result = None
        if self.rendering_eval and getattr(getattr(slam, 'dist', None), 'world', 1) > 1:
            raise NotImplementedError('rendering_eval.enabled with world > 1: the evaluation runs on one rank - evaluate the checkpoint '
                                      'afterwards (tools/eval_rendering.py)')
        self.segment_strategy = m.get('segment_strategy', 'rot_trans')
        self.segment_rot_cos, self.segment_rel_trans = m.get('segment_rot_cos', 0.94), m.get('segment_rel_trans', 0.30)
        self.fixed_segment_size = m.get('fixed_segment_size', 50)
        # draws on the device, like the reference's select_uv (common.py:156-172): no host RNG + upload between GPU launches
        self.gen = torch.Generator(device=self.eng.device).manual_seed(cfg.get('setup_seed', 1219) + 7)
        # Multi-GPU (slam.dist, loopy_slam_amd/parallel.py): everything that changes the MAP or the window - insertion pixels, keyframe
        # selection, new feature rows - draws from `gen`, seeded alike on every rank (replicated work keeps the replicas identical); the
        # pixels of the joint iterations draw from `gen_rays`, seeded per rank: every rank renders its own mapping_pixels / world rays of
        # the shared iteration and the gradients are summed (the loss is a sum over rays, Mapper.py:693-720)
        dist = getattr(slam, 'dist', None)
        self.gen_rays = self.gen if dist is None else \
            torch.Generator(device=self.eng.device).manual_seed(cfg.get('setup_seed', 1219) + 7 + 1000 * (1 + dist.rank))
        self.prev_c2w = None
        self.last_log = None
        # the optimised exposure feature of every optimize_map call (Mapper.py:800, 827): checkpointed (Mapper.py:1028-1031) and read
        # back by the final refinement and the evaluation renders (Mapper.py:394, 1111)
        self.exposure_feat_all = [] if slam.encode_exposure else None

    def set_pipe(self, pipe):
        self.pipe = pipe

    # -- frustum feature selection (Mapper.py:165-217): project every point, bilinear depth lookup, z test
    def get_mask_from_c2w(self, c2w, depth, return_mask=False, pending=False):
        """Frustum feature selection (Mapper.py:165-217) on the device: lk_frustum_rows.  pending: the selection is enqueued and the result
        object's finish() waits for its count (optim._PendingRows)."""
        return optim.frustum_rows(self.eng, self.npc.cloud_pos(), c2w, depth.float().contiguous(), (self.fx, self.fy, self.cx, self.cy),
                                  self.H, self.W, self.frustum_edge, return_mask=return_mask, pending=pending)

    def filter_point_before_add(self, rays_o, rays_d, gt_depth, prev_c2w):
        pts = rays_o + rays_d * gt_depth[:, None]
        w2c = _inv_pose(prev_c2w, pts.device)
        cam = pts @ w2c[:3, :3].T + w2c[:3, 3]
        zc = cam[:, 2]
        z = zc + 1e-5
        u = (self.fx * -cam[:, 0] + self.cx * zc) / z
        v = (self.fy * cam[:, 1] + self.cy * zc) / z
        inside = (u < self.W) & (u > 0) & (v < self.H) & (v > 0)
        return ~inside

    def overlap_fractions(self, pts, est_c2ws):
        """Fraction of the points [n,3] that project inside every keyframe's image minus a 20-pixel edge, in front of the camera
        (Mapper.py:250-270) - all keyframes in one batched projection on the device (the reference loops over them on the host with
        a numpy inverse each).  As in the reference this projection does NOT mirror x (the flip is commented out there, unlike
        get_mask_from_c2w / filter_point_before_add) and tests z + 1e-5 < 0."""
        dev = self.eng.device
        w2c = _inv_pose(torch.stack([c.to(dev).float() for c in est_c2ws]), dev)                       # [K,4,4]
        cam = torch.einsum('kij,nj->kni', w2c[:, :3, :3], pts) + w2c[:, None, :3, 3]
        z = cam[..., 2] + 1e-5
        u = (self.fx * cam[..., 0] + self.cx * cam[..., 2]) / z
        v = (self.fy * cam[..., 1] + self.cy * cam[..., 2]) / z
        m = (u < self.W - 20) & (u > 20) & (v < self.H - 20) & (v > 20) & (z < 0)
        return m.float().mean(dim=1)

    def keyframe_selection_overlap(self, gt_color, gt_depth, c2w, keyframe_dict, k, N_samples=8, pixels=200):
        """Keyframes that see the current frame's points, random k of them (Mapper.py:219-282)."""
        dev = self.eng.device
        ro, rd, gd, _ = get_samples(0, self.H, 0, self.W, pixels, self.H, self.W, self.fx, self.fy, self.cx, self.cy, c2w,
                                    gt_depth, gt_color, dev, depth_filter=True, generator=self.gen)     # (the replicas of a multi-GPU run draw alike)
        t = torch.linspace(0., 1., N_samples, device=dev)
        z = gd[:, None] * 0.8 * (1 - t) + (gd[:, None] + 0.5) * t
        pts = (ro[:, None, :] + rd[:, None, :] * z[..., None]).reshape(-1, 3)
        if len(keyframe_dict) == 0:
            return []
        frac = self.overlap_fractions(pts, [kf['est_c2w'] for kf in keyframe_dict]).cpu().tolist()   # one transfer for all keyframes
        # sorted by overlap (stable, as Python's sorted on the reference's dicts), then a random k of those with any overlap
        order = sorted(range(len(frac)), key=lambda i: frac[i], reverse=True)
        scored = [i for i in order if frac[i] > 0.0]
        perm = torch.randperm(len(scored), generator=self.gen, device=self.eng.device).tolist()
        return [scored[i] for i in perm[:k]]

    # -- point insertion of a mapped frame (Mapper.py:421-482)
    def _pixel_rays(self, flat, cur_c2w, gt_depth, gt_color, r2_add_map):
        """Rays of flat image indices with a positive depth (get_samples(depth_filter=True), common.py:237-259)."""
        W = self.W
        i, j = (flat % W).float(), torch.div(flat, W, rounding_mode='floor').float()
        ro, rd = get_rays_from_uv(i, j, cur_c2w, self.H, W, self.fx, self.fy, self.cx, self.cy)
        gd = gt_depth.reshape(-1)[flat]
        keep = gd > 0
        dyn = torch.sqrt(r2_add_map.reshape(-1)[flat][keep]) if r2_add_map is not None else None
        return ro[keep], rd[keep], gd[keep], gt_color.reshape(-1, 3)[flat][keep], dyn

    def draw_add_pixels(self, idx, gt_depth, gt_color, grad_mag=None):
        """The pixel draws of one frame's insertion passes as flat image indices: 'main' (pixels_adding, scaled on the first
        frame by the median depth, Mapper.py:421-425), 'overlap' (1000, Mapper.py:443-446) and 'grad' - n of the 5n highest
        colour-gradient pixels without replacement, sorted (get_samples_with_pixel_grad, common.py:175-196, 262-298)."""
        H, W, dev = self.H, self.W, self.eng.device
        n_main = self.pixels_adding
        if idx == 0:
            n_main = int(torch.clamp(self.pixels_adding * ((gt_depth.median() / 2.5) ** 2), min=self.pixels_adding,
                                     max=self.pixels_adding * 3).int().item())
        draws = {'main': torch.randint(0, H * W, (n_main,), generator=self.gen, device=dev),
                 'overlap': torch.randint(0, H * W, (1000,), generator=self.gen, device=dev)}
        n = self.pixels_based_on_color_grad
        if n > 0:
            if grad_mag is None:
                grad_mag = frame_radius_maps(self.eng, self.cfg, gt_color)[0]
            pool = optim.top_grad_pixels(self.eng, grad_mag, 5 * n, (0, H, 0, W))
            pick = torch.randperm(int(pool.numel()), generator=self.gen, device=dev)[:n]
            draws['grad'] = torch.sort(pool[pick].long()).values
        return draws

    def add_points_for_frame(self, idx, gt_color, gt_depth, cur_c2w, r2_add_map=None, draws=None, grad_mag=None):
        """Mapper.py:421-482: the non-overlapping area first (surface points outside the previous view), then 1000 more
        samples for holes INSIDE it, then the high colour-gradient pixels with radius_min (is_pts_grad).  Returns
        (frame_pts_add, per-pass counts)."""
        npc = self.npc
        draws = draws if draws is not None else self.draw_add_pixels(idx, gt_depth, gt_color, grad_mag)
        counts = []
        ro, rd, gd, gc, dyn = self._pixel_rays(draws['main'].long(), cur_c2w, gt_depth, gt_color, r2_add_map)
        if self.filter_before_add_points and idx != 0 and self.prev_c2w is not None:
            out = self.filter_point_before_add(ro, rd, gd, self.prev_c2w)
            counts.append(npc.add_neural_points(ro[out], rd[out], gd[out], gc[out], dynamic_radius=dyn[out] if dyn is not None else None))
            ro, rd, gd, gc, dyn = self._pixel_rays(draws['overlap'].long(), cur_c2w, gt_depth, gt_color, r2_add_map)
            out = self.filter_point_before_add(ro, rd, gd, self.prev_c2w)
            counts.append(npc.add_neural_points(ro[~out], rd[~out], gd[~out], gc[~out], dynamic_radius=dyn[~out] if dyn is not None else None))
        else:
            counts.append(npc.add_neural_points(ro, rd, gd, gc, dynamic_radius=dyn))
        if self.pixels_based_on_color_grad > 0 and 'grad' in draws:
            ro, rd, gd, gc, dyn = self._pixel_rays(draws['grad'].long(), cur_c2w, gt_depth, gt_color, r2_add_map)
            counts.append(npc.add_neural_points(ro, rd, gd, gc, is_pts_grad=True, dynamic_radius=dyn))
        return int(sum(counts)), [int(c) for c in counts]

    # -- one optimize_map call (Mapper.py:347-807)
    def optimize_map(self, num_joint_iters, idx, cur_gt_color, cur_gt_depth, gt_cur_c2w, keyframe_dict, keyframe_list,
                     cur_c2w, color_refine=False, new_fragment=False):
        cfg, eng, npc = self.cfg, self.eng, self.npc
        H, W = self.H, self.W
        intr = (self.fx, self.fy, self.cx, self.cy)
        init = idx == 0
        # 1. keyframes of the window
        segments = self.keyframe_selection_method == 'segments'
        sel = []
        if len(keyframe_dict) > 0:
            if segments:
                # end-of-sequence refinement (Mapper.py:386-396): the window is one keyframe per SEGMENT - the frame that opened it, with
                # the pose it was mapped at - all of them (`optimize_frame = list(range(len(keyframe_dict)))`), plus the current frame
                keyframe_dict = self.segments if self.segments else keyframe_dict[:1]
                sel = list(range(len(keyframe_dict)))
            elif self.keyframe_selection_method == 'global':
                num = self.mapping_window_size - 2
                sel = list(range(max(0, len(keyframe_dict) - 1 - num), len(keyframe_dict) - 1))
            else:
                sel = self.keyframe_selection_overlap(cur_gt_color, cur_gt_depth, cur_c2w, keyframe_dict[:-1], self.mapping_window_size - 2)
            if len(keyframe_list) > 0 and not segments:
                sel = sel + [len(keyframe_dict) - 1]
        frames_d = [keyframe_dict[k]['depth'] for k in sel] + [cur_gt_depth]
        frames_c = [keyframe_dict[k]['color'] for k in sel] + [cur_gt_color]
        frames_p = [keyframe_dict[k]['est_c2w'] for k in sel] + [cur_c2w]
        self.last_window_idx = [int(keyframe_dict[k]['idx']) for k in sel] + [int(idx)]       # frame indices of this call's window (logging, tests)
        grad_mag = r2_add_map = r2_query_map = None
        if self.use_dynamic_radius:                 # per-pixel radii of the current frame (Mapper.py:854-872)
            grad_mag, r2_add_map, r2_query_map = frame_radius_maps(eng, cfg, cur_gt_color)
            self.cur_r2_query = r2_query_map
        frames_r = ([keyframe_dict[k]['r2_query'] for k in sel] + [r2_query_map]) if self.use_dynamic_radius else None
        exposure = None
        if self.slam.encode_exposure:               # per-keyframe exposure features + the current frame's (Mapper.py:494-496, 588-607)
            self.cur_exposure_feat = self.slam.exposure_feat.detach().clone().requires_grad_(True)
            exposure = (self.decoders.mlp_exposure, [keyframe_dict[k]['exposure_feat'] for k in sel] + [self.cur_exposure_feat])
        # 2. add neural points seen by the current frame (Mapper.py:421-482)
        frame_pts_add = 0
        if not color_refine:
            frame_pts_add, self.last_add_counts = self.add_points_for_frame(idx, cur_gt_color, cur_gt_depth, cur_c2w, r2_add_map,
                                                                           grad_mag=grad_mag)
        # 3. rows to optimise (Mapper.py:498-520): selected further down, AFTER the call's batch assembly has been enqueued - the selection
        # ends in a count read-back, and neither the gradient-table fills nor the assembly depend on it (MapOptimizer.prepare)
        # 4. iteration count (Mapper.py:572-574)
        if idx > 0 and not color_refine:
            num_joint_iters = int(np.clip(int(num_joint_iters * frame_pts_add / 300), int(self.min_iter_ratio * num_joint_iters),
                                          2 * num_joint_iters))
        self.last_num_joint_iters, self.last_frame_pts_add = num_joint_iters, frame_pts_add
        stage_cfg = cfg['mapping']['init' if init else 'stage']
        lrs = {s: (stage_cfg[s]['decoders_lr'], stage_cfg[s]['geometry_lr'], stage_cfg[s]['color_lr']) for s in ('geometry', 'color')}
        F = len(frames_d)
        pix = (self.mapping_pixels // 10) if segments else (self.mapping_pixels // F)       # Mapper.py:417-418
        dist = getattr(self.slam, 'dist', None)
        if dist is not None:                        # the reference's batch, split over the ranks
            pix = max(1, pix // dist.world)
        R = pix * F
        rcfg = render_cfg_from(cfg, cfg['rendering']['sigmoid_coef_mapper'])
        mo = steps.MapOptimizer(eng, rcfg, self.decoders.dec, npc.knn, npc.cloud_pos(), npc.get_geo_feats(), npc.get_col_feats(),
                                None, R, lrs, w_color=self.w_color_loss, dynamic_radius=self.use_dynamic_radius,
                                fix_color_decoder=self.fix_color_decoder, dist=getattr(self.slam, 'dist', None), exposure=exposure,
                                fix_geo_decoder=self.fix_geo_decoder)          # (its gradient tables are allocated zeroed)
        geo_iters = self.geo_iter_first if init else int(num_joint_iters * self.geo_iter_ratio)
        ba_cams = ba_train = None
        if self.BA:
            # Mapper.py:541-566: the window's poses as 7-vectors in a fourth Adam group; the oldest keyframe stays fixed against drift
            # (Mapper.py:401, 547-548).  lr = BA_cam_lr while (geo_iter_ratio + 0.2) n <= it <= (geo_iter_ratio + 0.3) n, else 0
            # (Mapper.py:602-607).  The loop then runs on the per-statement path (steps.MapOptimizer.enable_ba)
            oldest = min(sel) if (len(keyframe_list) > 0 and not segments and len(sel) > 0) else None
            ba_train = [oldest is None or k != oldest for k in sel] + [True]
            ba_cams = torch.stack([get_tensor_from_camera(p) for p in frames_p]).float().to(eng.device).contiguous()
            lo, hi = num_joint_iters * (self.geo_iter_ratio + 0.2), num_joint_iters * (self.geo_iter_ratio + 0.3)
            mo.enable_ba(ba_cams, ba_train, lambda it: self.BA_cam_lr if lo <= it <= hi else 0.0)
        stack = (torch.stack(frames_d).contiguous(), torch.stack(frames_c).contiguous(),
                 torch.stack([p.float().to(eng.device) for p in frames_p]).contiguous(),
                 torch.stack(frames_r).contiguous() if frames_r is not None else None)
        fid = torch.arange(F, dtype=torch.int32).repeat_interleave(pix).to(eng.device)
        rnd = torch.randint(0, H * W, (num_joint_iters, R), generator=self.gen_rays, dtype=torch.int32, device=eng.device)
        log = eng.zeros(num_joint_iters, 4)
        # stage 'geometry' while joint_iter <= geo_iters (Mapper.py:594-597)
        n_geo = min(num_joint_iters, geo_iters + 1)
        # order on the stream: the selection, its count on the way to the host, THEN the fills and the batch assembly of the call
        sel_rows = self.get_mask_from_c2w(cur_c2w, cur_gt_depth, return_mask=True, pending=True) if self.frustum_feature_selection else None
        mo.prepare(num_joint_iters, n_geo, stack, rnd, fid, (0, H, 0, W), intr, H, W, log)
        rows = row_mask = None
        if sel_rows is not None:
            rows, row_mask = sel_rows.finish()
        mo.new_frame(rows, row_mask, zero=False)            # the backward only scatters into the rows being optimised
        mo.run(num_joint_iters, n_geo, stack, rnd, fid, (0, H, 0, W), intr, H, W, log)
        mo.finish()
        if self.slam.encode_exposure:           # the optimised feature of this frame is what the tracker starts from (Mapper.py:799)
            self.slam.exposure_feat = self.cur_exposure_feat.detach().clone()
            self.exposure_feat_all.append(self.cur_exposure_feat.detach().cpu())          # Mapper.py:800
        self.last_log = log
        if ba_cams is not None:                 # put the optimised poses back (Mapper.py:782-797)
            bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=eng.device)
            new = [torch.cat([get_camera_from_tensor(c), bottom], 0) for c in ba_cams]
            for f, k in enumerate(sel):
                if ba_train[f]:
                    keyframe_dict[k]['est_c2w'] = new[f].to(keyframe_dict[k]['est_c2w']).clone()
            return new[-1].to(cur_c2w).clone()
        return None

    def new_segment(self, idx, cur_c2w):
        """Mapper.check_new_fragment (Mapper.py:338-345) / NeuralPointCloud.check_rot_trans (neural_point.py:1317-1326) with
        compute_rel_trans / compute_cos_rel_rot (common.py:759-777): does the mapped frame idx open a new segment?"""
        if not self.segments:
            return True
        if self.segment_strategy == 'fixed':
            return idx % self.fixed_segment_size == 0
        if self.segment_strategy != 'rot_trans':
            raise NotImplementedError(self.segment_strategy)
        last = self.segments[-1]['est_c2w'].detach().cpu().float()
        cur = cur_c2w.detach().cpu().float()
        rel_trans = float((cur[:3, 3] - last[:3, 3]).norm(2))
        cos = float(torch.dot(last[:3, 2], cur[:3, 2]))          # the optical axes R e_z of the two cameras
        return rel_trans > self.segment_rel_trans or cos < self.segment_rot_cos

    def map_frame(self, idx, gt_color, gt_depth, gt_c2w, cur_c2w=None):
        """One mapped frame: the body of Mapper.run's loop (Mapper.py:835-1037) minus I/O and visualisation."""
        slam, cfg = self.slam, self.cfg
        cur_c2w = cur_c2w if cur_c2w is not None else slam.estimate_c2w_list[idx].to(self.eng.device)
        init = idx == 0
        last = idx == slam.n_img - 1
        rows_before = self.npc.n
        color_refine = bool(last and self.color_refine and not init)
        num_joint_iters, outer = (self.iters_first if init else self.num_joint_iters), 1
        saved = None
        if not init:
            self.mapping_window_size = cfg['mapping']['mapping_window_size'] * (2 if slam.n_img > 4000 else 1)
            if color_refine:
                # end of the sequence (Mapper.py:884-897): every row of the map is trainable, only the features move (the colour
                # decoder is frozen), ten times the iterations in five calls over a doubled window
                saved = (self.mapping_window_size, self.geo_iter_ratio, self.fix_color_decoder, self.frustum_feature_selection,
                         self.keyframe_selection_method)
                outer = 5
                self.mapping_window_size *= 2
                self.geo_iter_ratio = 0.4
                num_joint_iters *= 10
                self.fix_color_decoder, self.frustum_feature_selection, self.keyframe_selection_method = True, False, 'segments'
        num_joint_iters //= outer
        for _ in range(outer):
            self.BA = bool(len(self.keyframe_list) > 4 and self.BA_cfg)          # start BA when having enough keyframes (Mapper.py:957-958)
            ret = self.optimize_map(num_joint_iters, idx, gt_color, gt_depth, gt_c2w, self.keyframe_dict, self.keyframe_list, cur_c2w,
                                    color_refine=color_refine)
            if self.BA:                         # Mapper.py:962-964
                cur_c2w = ret
                slam.estimate_c2w_list[idx] = cur_c2w.detach().cpu()
        if saved is not None and not self.keep_refine_settings:
            (self.mapping_window_size, self.geo_iter_ratio, self.fix_color_decoder, self.frustum_feature_selection,
             self.keyframe_selection_method) = saved
        # (no keyframe from a frame whose ground-truth pose is not finite - ScanNet has -inf poses, Mapper.py:982)
        if (idx % self.keyframe_every == 0 or idx == slam.n_img - 2) and idx not in self.keyframe_list and bool(torch.isfinite(gt_c2w).all()):
            self.keyframe_list.append(idx)
            self.keyframe_dict.append({'gt_c2w': gt_c2w, 'idx': idx, 'color': gt_color, 'depth': gt_depth, 'est_c2w': cur_c2w.clone(),
                                       'r2_query': getattr(self, 'cur_r2_query', None),
                                       'exposure_feat': self.cur_exposure_feat.detach() if self.slam.encode_exposure else None})
        if self.new_segment(idx, cur_c2w):
            self.segments.append({'idx': idx, 'color': gt_color, 'depth': gt_depth, 'est_c2w': cur_c2w.clone(), 'gt_c2w': gt_c2w,
                                  'r2_query': getattr(self, 'cur_r2_query', None),
                                  'exposure_feat': self.cur_exposure_feat.detach() if self.slam.encode_exposure else None})
            if self.closer is not None and self.closer.on_new_segment(self, rows_before) is not None:
                cur_c2w = self.segments[-1]['est_c2w'].clone()          # the corrected pose: the tracker starts the next frame from it
        elif self.closer is not None and self.closer.place is not None:
            self.closer.on_mapped_frame(gt_color, self.segments)        # place recognition: the segment's own score (compute_dbow_score)
        self.prev_c2w = cur_c2w.clone()         # Mapper.py:1001
        slam.mapping_idx[0] = idx
        return self.last_log

    def run(self, time_string=None, tracker=None, n_frames=None, callback=None):
        """Mapper.run (Mapper.py:808-1049) in the single-process form: the reference's mapper blocks on a pipe until the tracker
        has posed the next frame to map (frame 0, every `every_frame`-th, the last); here the loop itself asks the tracker
        (Tracker.track_frame) for every frame in between, in order, and maps when the reference's mapper would wake up."""
        slam = self.slam
        tracker = tracker if tracker is not None else slam.tracker
        n = n_frames or slam.n_img
        for i in range(n):
            idx, color, depth, c2w = slam.frame_reader[i]
            est = tracker.track_frame(idx, color, depth, c2w)
            if idx == 0 or idx % self.every_frame == 0 or idx == n - 1:
                self.map_frame(idx, color, depth, c2w, cur_c2w=est)
                if self.logger is not None and ((idx > 0 and idx % self.ckpt_freq == 0) or idx == n - 1):
                    self.logger.log(idx, self.keyframe_dict, self.keyframe_list, npc=self.npc,
                                    exposure_feat=self.exposure_feat_all, last_log=(idx == n - 1))
            if callback:
                callback(idx, est, c2w)
            if self.cfg.get('stop') and idx != 0 and idx % self.cfg['stop'] == 0:       # Tracker.py:423, Mapper.py:1048 (run.py --stop)
                n = idx + 1
                break
        records = None
        if self.rendering_eval:
            from . import render_eval
            records = render_eval.FrameRecords(self)
        if self.meshing:                        # Mapper.py:1080-1200: re-render the mapped frames, fuse them, write the mesh
            from . import tsdf
            self.mesh_file, _ = tsdf.mesh_run(self, n, on_frame=records)     # (a frame re-rendered for the mesh is measured there)
        if self.rendering_eval:                 # Mapper.py:1056-1160: ATE, depth L1, PSNR and MS-SSIM of the re-rendered frames
            self.eval_result = render_eval.eval_run(self, n, records=records)
        return slam.estimate_c2w_list[:n], slam.gt_c2w_list[:n]


def frame_radius_maps(eng, cfg, color):
    """(grad_mag, r2_add, r2_query) of one frame from the pointcloud config (Tracker.py:243-258, Mapper.py:854-872)."""
    pc = cfg['pointcloud']
    return optim.radius_maps(eng, color.float().contiguous(), pc['color_grad_threshold'], pc['radius_add_max'], pc['radius_add_min'],
                             pc['radius_query_ratio'])


# ============================================================================================ Tracker
class Tracker:
    def __init__(self, cfg, args, slam):
        self.cfg, self.slam = cfg, slam
        self.eng = slam.eng
        t = cfg['tracking']
        self.npc, self.decoders, self.renderer = slam.npc, slam.shared_decoders, slam.renderer
        self.renderer.sigmoid_coefficient = cfg['rendering']['sigmoid_coef_tracker']
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy
        self.cam_lr, self.num_cam_iters, self.tracking_pixels = t['lr'], t['iters'], t['pixels']
        self.separate_LR, self.w_color_loss = t['separate_LR'], t['w_color_loss']
        self.ignore_edge_W, self.ignore_edge_H = t['ignore_edge_W'], t['ignore_edge_H']
        self.use_color_in_tracking, self.const_speed_assumption = t['use_color_in_tracking'], t['const_speed_assumption']
        self.gt_camera = t.get('gt_camera', False)
        self.use_dynamic_radius = cfg['use_dynamic_radius']
        self.sample_with_color_grad, self.depth_limit = t.get('sample_with_color_grad', False), t.get('depth_limit', False)
        self.handle_dynamic = t.get('handle_dynamic', True)       # False: median-of-residual outlier mask (Tracker.py:177-179)
        self.gen = torch.Generator(device=self.eng.device).manual_seed(cfg.get('setup_seed', 1219) + 3)      # device draws (select_uv)
        self.last_log = None
        # tracking.visual_odometer (Tracker.py:92-97): off (absent / False) makes no object and adds no launch
        self.odometer = None
        if t.get('visual_odometer', False):
            self.odometer = odometry.VisualOdometer(self.eng, dict(H=self.H, W=self.W, fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy),
                                                    t['visual_odometer'])

    @property
    def odometry_fallbacks(self):
        """Frames whose odometry estimate was not usable and that started from the copied pose instead."""
        return 0 if self.odometer is None else self.odometer.fallbacks

    def set_pipe(self, pipe):
        self.pipe = pipe

    def update_para_from_mapping(self):
        pass            # one process, one copy of the map: nothing to clone (Tracker.py:199-212)

    def optimize_cam_in_batch(self, camera_tensor, gt_color, gt_depth, batch_size, optimizer=None, selected_index=None):
        """One pose iteration through the autograd bridge with a caller-supplied torch optimiser
        (reference signature, Tracker.py:102-197).  track_frame uses the fused loop instead."""
        dev = self.eng.device
        H, W = self.H, self.W
        c2w = get_camera_from_tensor(camera_tensor)
        ro, rd, gd, gc, i, j = get_samples(self.ignore_edge_H, H - self.ignore_edge_H, self.ignore_edge_W, W - self.ignore_edge_W,
                                           batch_size, H, W, self.fx, self.fy, self.cx, self.cy, c2w, gt_depth, gt_color, dev,
                                           depth_filter=True, return_index=True, depth_limit=5.0 if self.depth_limit else None)
        with torch.no_grad():
            inside = gd <= torch.minimum(10 * gd.median(), 1.2 * gd.max())
        ro, rd, gd, gc = ro[inside], rd[inside], gd[inside], gc[inside]
        depth, unc, color, _ = self.renderer.render_batch_ray(self.npc, self.decoders, rd, ro, dev, 'color', gt_depth=gd, is_tracker=True)
        unc = unc.detach()
        tmp = torch.abs(gd - depth) / torch.sqrt(unc + 1e-10)
        if self.handle_dynamic:
            mask = (tmp < 10 * tmp.mean()) & (gd > 0) & (~torch.isnan(depth)) & (~torch.isnan(unc))
        else:                                       # Tracker.py:177-179
            t2 = torch.abs(gd - depth)
            mask = (t2 < 10 * t2.median()) & (gd > 0) & (~torch.isnan(depth)) & (~torch.isnan(unc))
        geo_loss = torch.clamp(tmp, min=0.0, max=1e3)[mask].sum()
        color_loss = torch.abs(gc - color)[mask].sum()
        loss = geo_loss + (self.w_color_loss * color_loss if self.use_color_in_tracking else 0.0)
        if optimizer is not None:
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        return loss.item(), (color_loss / mask.shape[0]).item(), (geo_loss / mask.shape[0]).item()

    def track_frame(self, idx, gt_color, gt_depth, gt_c2w):
        """Pose of frame idx (Tracker.py:281-409)."""
        slam, eng = self.slam, self.eng
        if idx <= 1 or self.gt_camera:       # the first TWO frames keep the given pose (Tracker.py:297: `if idx <= 1 or self.gt_camera`)
            c2w = gt_c2w.clone()
            if self.odometer is not None:    # Tracker.py:291-295
                self.odometer.set_init_state(gt_color, gt_depth, gt_c2w)
        else:
            pre = slam.estimate_c2w_list[idx - 1].float()           # pose bookkeeping lives on the host (4x4 algebra)
            if self.const_speed_assumption and idx - 2 >= 0:
                delta = pre @ torch.linalg.inv(slam.estimate_c2w_list[idx - 2].float())
                init = delta @ pre
            elif self.odometer is not None and idx - 2 >= 0:        # Tracker.py:304-309
                # the previous frame's OPTIMISED pose is the base (Tracker.py:275-277, every frame here: one process, nothing to wait for)
                self.odometer.update_est_abs_pose(slam.estimate_c2w_list[idx - 1])
                init = self.odometer.estimate_pose(gt_color, gt_depth).float()
            else:
                init = pre
            cam = get_tensor_from_camera(init)
            gt_cam = get_tensor_from_camera(gt_c2w.detach().cpu())
            if float(torch.dot(cam[:4], gt_cam[:4])) < 0:           # same quaternion hemisphere as the ground truth (Tracker.py:330-331)
                cam[:4] *= -1
            cam = cam.to(eng.device)
            rcfg = render_cfg_from(self.cfg, self.cfg['rendering']['sigmoid_coef_tracker'])
            win = (self.ignore_edge_H, self.H - self.ignore_edge_H, self.ignore_edge_W, self.W - self.ignore_edge_W)
            n_px = self.tracking_pixels
            grad = r2_query = None
            if self.use_dynamic_radius or self.sample_with_color_grad:      # per-frame image pre-pass (Tracker.py:243-268)
                grad, _, r2q = frame_radius_maps(eng, self.cfg, gt_color)
                r2_query = r2q if self.use_dynamic_radius else None
            if self.sample_with_color_grad:
                # pool of the 15*n highest-gradient pixels inside the window with a valid depth; every iteration draws n
                # of them without replacement (common.py:198-234, Tracker.py:126-139) -> flat full-image pixel indices
                pool = optim.top_grad_pixels(eng, grad, 15 * n_px, win, gt_depth.float().contiguous(), self.depth_limit)
                n_px = min(n_px, int(pool.numel()))
                # n distinct positions per iteration = the n largest of a row of uniform draws, generated and selected on the
                # device that holds the pool (200 x 75 000 draws per frame for the TUM budget: ~100 ms on host threads)
                u = torch.rand(self.num_cam_iters, pool.numel(), generator=self.gen, device=eng.device)
                order = u.topk(n_px, dim=1).indices.to(eng.device)
                rnd = pool[order].contiguous()
                win_it = (0, self.H, 0, self.W)
            else:
                n = (win[1] - win[0]) * (win[3] - win[2])
                rnd = torch.randint(0, n, (self.num_cam_iters, n_px), generator=self.gen, dtype=torch.int32, device=eng.device)
                win_it = win
            track_depth = gt_depth
            if self.depth_limit and not self.sample_with_color_grad:
                # get_samples(depth_filter=True, depth_limit=5.0) (Tracker.py:142-146, common.py:249-252): draws whose depth reading is
                # 5 m or beyond are dropped like the ones without a reading - a zero reading IS "dropped" to the loop (absent ray)
                track_depth = torch.where(gt_depth < 5.0, gt_depth, torch.zeros_like(gt_depth))
            to = steps.TrackOptimizer(eng, rcfg, self.decoders.dec, self.npc.knn, self.npc.cloud_pos(), self.npc.get_geo_feats(),
                                      self.npc.get_col_feats(), n_px, self.cam_lr, separate_lr=self.separate_LR,
                                      w_color=self.w_color_loss, use_color=self.use_color_in_tracking,
                                      dynamic_radius=r2_query is not None, dist=getattr(slam, 'dist', None),
                                      handle_dynamic=self.handle_dynamic, shard_rays=bool(self.cfg['tracking'].get('shard_rays', False)))
            exposure = None
            if slam.encode_exposure:                # this frame's exposure feature starts from the shared one (Tracker.py:280-283)
                self.exposure_feat = slam.exposure_feat.detach().clone().requires_grad_(True)
                exposure = (self.decoders.mlp_exposure, self.exposure_feat)
            best, log = to.track(cam, track_depth, gt_color, self.num_cam_iters, win_it, (self.fx, self.fy, self.cx, self.cy), rnd,
                                 r2_map=r2_query, exposure=exposure)
            if slam.encode_exposure:
                slam.exposure_feat = self.exposure_feat.detach().clone()           # Tracker.py:412-414
            self.last_log = log
            c2w = torch.eye(4, device=eng.device)
            c2w[:3] = get_camera_from_tensor(best)
        slam.estimate_c2w_list[idx] = c2w.detach().cpu()
        slam.gt_c2w_list[idx] = gt_c2w.detach().cpu()
        slam.idx[0] = idx
        return c2w

    def run(self, time_string=None, mapper=None, n_frames=None, callback=None):
        """Tracker.run (Tracker.py:214-427) in the single-process form: the reference's tracker waits on a pipe for the mapper
        after frame 0 and after every `every_frame`-th frame; here the same interleaving is one loop (Mapper.run), entered from
        either side."""
        return (mapper if mapper is not None else self.slam.mapper).run(time_string, tracker=self, n_frames=n_frames, callback=callback)


# ============================================================================================ Point_SLAM
class SyntheticRoomDataset:
    """(idx, color [H,W,3], depth [H,W], c2w [4,4]) from loopy_slam_amd.synthetic."""

    def __init__(self, cfg, device, n_frames=None):
        self.cfg, self.device = cfg, device
        self.n_img = n_frames or cfg['data'].get('n_frames', 50)
        c = cfg['cam']
        self.intr = dict(H=c['H'], W=c['W'], fx=c['fx'], fy=c['fy'], cx=c['cx'], cy=c['cy'])
        self.crop_edge = c.get('crop_edge', 0) or 0
        # data.motion: 'loop' = the slow closed loop (3 mm, 0.2 degrees per frame: throughput runs), 'handheld' = 1-2 cm and 0.5-1.2 degrees
        # per frame with a changing velocity (synthetic.handheld_pose: the accuracy runs, where the tracker has to do something)
        self.motion = cfg['data'].get('motion', 'loop')
        self.scene = cfg['data'].get('scene', 'plain')         # 'furnished': boxes along the walls, finer relief and texture (synthetic.FURNITURE)

    def __len__(self):
        return self.n_img

    def __getitem__(self, idx):
        d, c, p = synthetic.render_frame(idx, intr=self.intr, device=self.device, holes=0.01, n_poses=2000, motion=self.motion, scene=self.scene)
        e = self.crop_edge
        if e > 0:       # the reference's readers crop the frames (src/utils/datasets.py), Point_SLAM.update_cam the intrinsics
            d, c = d[e:-e, e:-e].contiguous(), c[e:-e, e:-e].contiguous()
        return idx, c, d, p


class Point_SLAM:
    def __init__(self, cfg, args=None, share_npc=True, share_decoders=True, time_string=None, eng=None, dataset=None, dist=None):
        self.cfg, self.args = cfg, args
        self.eng = eng if eng is not None else core.Engine()
        self.dist = dist
        c = cfg['cam']
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = c['H'], c['W'], c['fx'], c['fy'], c['cx'], c['cy']
        self.update_cam()
        if 'stop' not in cfg:                   # run.py --stop n (Point_SLAM.py:70-73): both loops return after frame n
            cfg['stop'] = getattr(args, 'stop', None)
        self.shared_decoders = NICER(cfg, eng=self.eng)
        self.load_pretrain(cfg)                 # Point_SLAM.py:94
        # the frames: a reader handed in; else the reader of cfg['dataset'] when data.input_folder holds a sequence of its layout
        # (datasets.open_sequence; Point_SLAM.py:110); else the synthetic room
        self.frame_reader = dataset if dataset is not None else datasets.open_sequence(cfg, args, eng=self.eng)
        if self.frame_reader is None:
            self.frame_reader = SyntheticRoomDataset(cfg, self.eng.device)
        self.n_img = len(self.frame_reader)
        self.estimate_c2w_list = torch.zeros((self.n_img, 4, 4))
        self.gt_c2w_list = torch.zeros((self.n_img, 4, 4))
        self.idx = torch.zeros(1, dtype=torch.int32)
        self.mapping_idx = torch.zeros(1, dtype=torch.int32)
        # one shared exposure feature, cloned by the tracker for every frame and kept per keyframe by the mapper
        # (Point_SLAM.py:90-96; model.encode_exposure, ScanNet)
        self.encode_exposure = cfg['model']['encode_exposure']
        self.exposure_feat = torch.zeros(cfg['model']['exposure_dim'], device=self.eng.device) if self.encode_exposure else None
        self.npc = NeuralPointCloud(cfg, self, args, eng=self.eng)
        self.renderer = Renderer(cfg, args, self)
        self.renderer_map = Renderer(cfg, args, self)
        self.mapper = Mapper(cfg, args, self)
        self.tracker = Tracker(cfg, args, self)

    def load_pretrain(self, cfg, color=None):
        """The pretrained ConvONet checkpoint's middle-level decoder becomes the geometry decoder (Point_SLAM.py:177-209): of
        ckpt['model'] the keys that contain 'decoder' and not 'encoder'; 'decoder.coarse.<name>' -> geo_decoder.<name>
        (load_state_dict(strict=False): names the decoder does not have are ignored, a size mismatch raises), 'decoder.fine.*' is
        collected and unused as in the reference.  color: optional checkpoint of a run whose 'decoder_state_dict' holds
        'color_decoder.*' entries for the colour decoder (Point_SLAM.py:198-209).
        Every shipped config freezes the geometry decoder (mapping.fix_geo_decoder), so without this file the system runs on a
        random geometry prior: a missing file is reported loudly and the run continues on the random-init decoders (the reference
        would stop in torch.load; no pretrained file exists offline).  Returns the names loaded into the geometry decoder."""
        path = (cfg.get('pretrained_decoders') or {}).get('middle_fine')
        self.pretrained_loaded = []
        if not path or not os.path.exists(path):
            import warnings
            warnings.warn(f'pretrained_decoders.middle_fine = {path!r} not found: the geometry decoder keeps its random initialisation '
                          '(Point_SLAM.load_pretrain)')
            return self.pretrained_loaded
        ckpt = torch.load(path, map_location='cpu', weights_only=False)
        middle, fine = {}, {}
        for key, val in ckpt['model'].items():
            if ('decoder' in key) and ('encoder' not in key):
                if 'coarse' in key:
                    middle[key[8 + 7:]] = val           # strip 'decoder.' + 'coarse.'
                elif 'fine' in key:
                    fine[key[8 + 5:]] = val
        have = set(self.shared_decoders.geo_decoder.state_dict())
        self.shared_decoders.geo_decoder.load_state_dict(middle, strict=False)
        self.pretrained_loaded = sorted(k for k in middle if k in have)
        if color:
            dec = torch.load(color, map_location='cpu', weights_only=False)['decoder_state_dict']
            self.shared_decoders.color_decoder.load_state_dict({k[14:]: v for k, v in dec.items() if 'color' in k}, strict=False)
        return self.pretrained_loaded

    def update_cam(self):
        """crop_size rescales the intrinsics to the resized image, then crop_edge shifts the principal point and shrinks the image
        (Point_SLAM.py:155-175)."""
        crop_size = self.cfg['cam'].get('crop_size')
        if crop_size:
            sx, sy = crop_size[1] / self.W, crop_size[0] / self.H
            self.fx, self.fy, self.cx, self.cy = sx * self.fx, sy * self.fy, sx * self.cx, sy * self.cy
            self.W, self.H = crop_size[1], crop_size[0]
        e = self.cfg['cam'].get('crop_edge', 0) or 0
        if e > 0:
            self.H -= 2 * e
            self.W -= 2 * e
            self.cx -= e
            self.cy -= e

    def run(self, n_frames=None, callback=None):
        """Alternate tracking (every frame) and mapping (frame 0 and every `every_frame`-th), as the reference's
        two processes do through their pipe (Tracker.py:272-273,417-418; Mapper.py:836-842)."""
        return self.mapper.run(tracker=self.tracker, n_frames=n_frames, callback=callback)


# ============================================================================================ checkpoints
class Logger:
    """Checkpoints in the reference's format (src/utils/Logger.py:20-65): one `{idx:05d}.tar` with the same keys, so the
    reference's offline tools (eval_ate.py, get_mesh_tsdf_fusion.py, eval_recon.py) read our runs and `load` resumes
    theirs.  The map is tensor-resident here; tensors are saved on the CPU (the reference saves python lists for the
    positions - both load with `torch.tensor(...)`)."""

    def __init__(self, cfg, args, mapper, ckptsdir=None):
        self.mapper, self.slam = mapper, mapper.slam
        self.ckptsdir = ckptsdir or os.path.join(cfg['data'].get('output', 'output'), 'ckpts')
        self.decoders = mapper.decoders

    def log(self, idx, keyframe_dict, keyframe_list, selected_keyframes=None, npc=None, exposure_feat=None, last_log=False):
        npc = npc if npc is not None else self.mapper.npc
        os.makedirs(self.ckptsdir, exist_ok=True)
        path = os.path.join(self.ckptsdir, '{:05d}.tar'.format(idx))
        cpu = lambda t: t.detach().cpu() if torch.is_tensor(t) else t
        ck = {
            'cloud_pos': npc.get_cloud_pos(end=True).detach().cpu().tolist(),
            'pts_num': npc.pts_num(),
            'input_pos': npc.input_pos().detach().cpu().tolist(),
            'input_rgb': npc.input_rgb().detach().cpu().tolist(),
            'input_normal': [], 'input_normal_cartesian': [],
            'decoder_state_dict': {k: cpu(v) for k, v in self.decoders.state_dict().items()},
            'gt_c2w_list': self.slam.gt_c2w_list, 'estimate_c2w_list': self.slam.estimate_c2w_list,
            'keyframe_list': list(keyframe_list),
            'keyframe_dict': [{k: cpu(v) for k, v in kf.items()} for kf in keyframe_dict],
            'selected_keyframes': selected_keyframes if selected_keyframes is not None else {},
            'idx': idx,
            'fragments': self.mapper.closer.fragments(self.mapper.segments) if getattr(self.mapper, 'closer', None) is not None else [],
            'exposure_feat_all': torch.stack([cpu(e) for e in exposure_feat], dim=0) if exposure_feat else None,
        }
        if last_log:
            ck['geo_feats'] = cpu(npc.get_geo_feats(end=True)).float()         # the reference's tools read fp32 tables whatever the storage format
            ck['col_feats'] = cpu(npc.get_col_feats(end=True)).float()
        # the colour embedding matrix is not part of the reference's state_dict (decoder.py:32); keep it beside it
        ck['color_embedder_B'] = cpu(self.decoders.color_embedder_B()) if hasattr(self.decoders, 'color_embedder_B') else None
        torch.save(ck, path, _use_new_zipfile_serialization=False)
        return path

    @staticmethod
    def load(path, slam_obj):
        """Restore map, decoders, poses and keyframes of `slam_obj` from a checkpoint written by `log(last_log=True)`."""
        ck = torch.load(path, map_location='cpu', weights_only=False)
        eng, npc = slam_obj.eng, slam_obj.npc
        pos = torch.tensor(ck['cloud_pos'], dtype=torch.float32).reshape(-1, 3)
        n = pos.shape[0]
        npc._grow(n)
        npc._pos[:n] = pos.to(eng.device)
        if 'geo_feats' in ck:
            npc._geo[:n] = ck['geo_feats'].to(eng.device).to(npc.feat_dtype)
            npc._col[:n] = ck['col_feats'].to(eng.device).to(npc.feat_dtype)
        npc.n = n
        if n:
            npc.knn.build(npc._pos[:n])
        if ck.get('color_embedder_B') is not None and hasattr(slam_obj.shared_decoders, 'set_color_embedder_B'):
            slam_obj.shared_decoders.set_color_embedder_B(ck['color_embedder_B'])
        slam_obj.shared_decoders.load_state_dict(ck['decoder_state_dict'])
        slam_obj.gt_c2w_list[:] = ck['gt_c2w_list']
        slam_obj.estimate_c2w_list[:] = ck['estimate_c2w_list']
        slam_obj.mapper.keyframe_list = list(ck['keyframe_list'])
        kfs = []
        for kf in ck['keyframe_dict']:
            kf = {k: (v.to(eng.device) if torch.is_tensor(v) else v) for k, v in kf.items()}
            if 'r2_query' not in kf and kf.get('dynamic_r_query') is not None:
                # a checkpoint written by the reference: per-pixel RADIUS (float64); the kernels take its square in float32
                kf['r2_query'] = (kf['dynamic_r_query'].double() ** 2).float().contiguous()
            kfs.append(kf)
        slam_obj.mapper.keyframe_dict = kfs
        if slam_obj.encode_exposure:            # per-mapped-frame exposure features (Mapper.py:394, 1111; get_mesh_tsdf_fusion.py:44-46)
            xa = ck.get('exposure_feat_all')
            slam_obj.mapper.exposure_feat_all = [e.clone() for e in xa] if xa is not None else []
            if xa is not None and len(xa):
                slam_obj.exposure_feat = xa[-1].to(eng.device).clone()
        if 'geo_feats' not in ck and n:
            import warnings
            warnings.warn(f'{path}: no geo_feats / col_feats in this checkpoint (the reference only writes them with last_log): '
                          'the feature tables of the restored map are zero')
        return ck['idx']
