/* loopy_hip.h — C ABI of libloopyhip.so: the MI355X (gfx950) implementation of
 * Loopy-SLAM's per-frame neural-point render / optimise hot path.
 *
 * The reference (eriksandstroem/Loopy-SLAM) has no FFI; its seam for this path is the
 * Python API (Renderer.render_batch_ray, NICER.forward, NeuralPointCloud.find_neighbors_faiss,
 * torch.optim.Adam ...).  Each entry point below names the reference code it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless named host_*; the caller (PyTorch) owns all
 *    buffers; the library allocates only what an lk_knn_t handle owns;
 *  - every call returns 0 on success, <0 on error (lk_last_error() gives the message,
 *    thread-local); nothing throws across the ABI;
 *  - kernels are enqueued on `stream` (a hipStream_t; torch.cuda.current_stream().cuda_stream)
 *    and never synchronise the device; lk_render_bwd (and lk_render_fwd inside lk_map_frame) additionally fork part of their
 *    work onto ONE library-owned non-blocking stream, and lk_map_frame runs the neighbour search of its iterations ahead on a
 *    library-owned third stream; both are joined back into `stream` with events, so results are complete in stream
 *    order (see lk_set_serial to switch them off).  These streams and the per-point scratch of an lk_knn_t are shared state:
 *    concurrent calls from several host threads must be ordered by the caller;
 *  - fp32 everywhere; indices int32; R rays, S samples/ray (<= 8), P = R*S points in
 *    ray-major order (point r*S+s), k = 8 neighbours, C = 32 channels, N cloud points.
 */
#ifndef LOOPY_HIP_H
#define LOOPY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LK_ABI_VERSION 1
#define LK_K 8          /* pointcloud.nn_num   (configs/point_slam.yaml:136) */
#define LK_C 32         /* model.c_dim         (configs/point_slam.yaml:11)  */
#define LK_S_MAX 8      /* rendering.N_surface is 5 in every config          */

#define LK_OK 0
#define LK_ERR_ARG (-1)
#define LK_ERR_HIP (-2)
#define LK_ERR_STATE (-3)
#define LK_ERR_RANGE (-4)   /* an operand left the range of the split fp16 products (see lk_status_peek) */

typedef struct lk_knn_s* lk_knn_t;

int lk_version(void);
const char* lk_last_error(void);

/* ---------------------------------------------------------------- neighbour index
 * Replaces the FAISS-GPU IVF index of NeuralPointCloud (src/neural_point.py:67-72 create,
 * :1623-1627 train+add, :1659-1708 find_neighbors_faiss) by an exact uniform-grid search.
 * Contract (oracle/hotpath.py::knn_exact): d2 = (dx*dx+dy*dy)+dz*dz in fp32, candidates
 * d2 <= r2, the k=8 smallest by (d2, index) ascending, empty slots idx=-1 / d2=FLT_MAX,
 * count = #returned with d2 < r2.
 */
int lk_knn_create(float cell_size, int64_t capacity_points, int64_t max_cells, lk_knn_t* out);
int lk_knn_destroy(lk_knn_t h);
/* (Re)build the grid over pos[0..N).  Appending points = rebuilding with the larger N
 * (counting sort, O(N), device only, no host sync).  pos must stay alive and unchanged
 * until the next build (the grid keeps its own sorted copy; pos itself is not read by queries). */
int lk_knn_build(lk_knn_t h, const float* pos, int64_t N, void* stream);
int64_t lk_knn_size(lk_knn_t h);
/* Grow the indexed cloud by M points (they get the indices lk_knn_size() .. + M - 1): NeuralPointCloud.add_neural_points'
 * index.add (src/neural_point.py:1623-1627).  A uniform grid has no cheap in-place insert - this is lk_knn_build over
 * (points recovered from the grid's sorted copy | pos_new): O(N + M), device only, the handle keeps its own position buffer
 * from the first call on.  A caller that holds the grown position array anyway (NeuralPointCloud does) calls lk_knn_build. */
int lk_knn_append(lk_knn_t h, const float* pos_new, int64_t M, void* stream);
/* r2_per_query may be NULL (then r2_scalar is used for every query). */
int lk_knn_query(lk_knn_t h, const float* q, int64_t P, float r2_scalar, const float* r2_per_query,
                 float* out_d2 /*[P,8]*/, int32_t* out_idx /*[P,8]*/, int32_t* out_count /*[P]*/,
                 void* stream);

/* ---------------------------------------------------------------- decoder weights
 * NICER = MLP_geometry (hidden 32, relu) + MLP_color (hidden 128, softplus beta=100)
 * (src/conv_onet/models/decoder.py:106-288, 345-546).  The kernels read ONE packed fp32
 * blob; lk_weight_layout() describes it so the host can pack/unpack a state_dict.
 * Every matrix is stored [out][in_padded] (torch layout, input dim zero-padded to a
 * multiple of 8; the geometry skip layer's input is [e(93) pad 3 | h(32)]).
 */
typedef struct {
    char name[64];      /* reference state_dict key, e.g. "color_decoder.pts_linears.3.weight" */
    int64_t offset;     /* in floats, multiple of 64 */
    int32_t rows, cols; /* logical shape (cols = 1 for vectors) */
    int32_t ld;         /* padded row length in the blob */
    int32_t col_split;  /* if >0: logical cols [col_split..) start at padded col `col_shift` */
    int32_t col_shift;
} lk_weight_entry;
int lk_weight_layout(lk_weight_entry* out, int max_entries); /* returns #entries */
int64_t lk_weight_blob_floats(void);
/* The GEMM operands are streamed from a derived "fragment" copy of the blob (MFMA operand order, forward + transposed,
 * every weight as three bf16 pieces, the forward form also as two fp16 pieces; opaque to the caller: allocate lk_weight_frag_floats() floats, 16-byte aligned);
 * refresh it after every change of the master blob (optimiser step, load). */
int64_t lk_weight_frag_floats(void);
int lk_weights_repack(const float* blob, float* frag, void* stream);
/* The same, then `stream` is synchronised and the range check of the repack (LK_STATUS_WEIGHT_RANGE below) is reported: LK_ERR_RANGE with
 * the message in lk_last_error() when a matrix entry is non-finite or |w| >= 32768.  For the places where weights enter from outside
 * (checkpoint load, DecoderBlob.pack); the per-step repacks stay asynchronous and report through the sticky status word. */
int lk_weights_repack_checked(const float* blob, float* frag, void* stream);

/* ---------------------------------------------------------------- operand-range status (sticky)
 * The decoders' fp32 products run as split fp16 products on the 16-bit matrix pipe: exact to fp32 class for operands
 * below fp16's ceiling, SATURATING above it - the reference (src/conv_onet/models/decoder.py:513-546, plain fp32) has no such ceiling.
 * The library therefore keeps one status word (host-mapped memory, written by the kernels, read by the host without synchronisation):
 *   LK_STATUS_WEIGHT_RANGE  a repack (lk_weights_repack, the repack riders of lk_map_frame) met a matrix entry that is non-finite or
 *                           has |w| >= 32768;
 *   LK_STATUS_ACT_RANGE     a forward launched with LK_FLAG_CHECK_RANGE met an operand (interpolated feature, activation) that is
 *                           non-finite or has |x| >= 65504.
 * The word is STICKY: once a bit is set every lk_render_fwd / lk_render_bwd / lk_track_frame / lk_map_frame / lk_weights_repack call
 * fails with LK_ERR_RANGE (nothing is launched) until lk_status_clear().  A bit set by a launch that is still running shows at a later
 * call; lk_status_sync waits for `stream` first. */
#define LK_STATUS_WEIGHT_RANGE 1u
#define LK_STATUS_ACT_RANGE    2u
int lk_status_peek(uint32_t* bits);
int lk_status_sync(void* stream, uint32_t* bits);
int lk_status_clear(void);

/* ---------------------------------------------------------------- render forward / backward */
#define LK_FLAG_STAGE_COLOR   (1u << 0)  /* NICER stage 'color' (else 'geometry': rgb = 0)          */
#define LK_FLAG_TRACKER       (1u << 1)  /* is_tracker: gradient flows to the sample positions      */
#define LK_FLAG_REL_POS       (1u << 2)  /* model.encode_rel_pos_in_col                             */
#define LK_FLAG_COLOR_LOGITS  (1u << 3)  /* colour decoder returns pre-sigmoid logits (decoder.py:541-542) */
#define LK_FLAG_SAVE_ACT      (1u << 4)  /* forward keeps the activations lk_render_bwd needs        */
#define LK_FLAG_GRAD_FEATS    (1u << 5)  /* backward: d/d geo_feats, d/d col_feats                   */
#define LK_FLAG_GRAD_WEIGHTS  (1u << 6)  /* backward: d/d decoder blob                               */
#define LK_FLAG_GRAD_RAYS     (1u << 7)  /* backward: d/d rays_o, d/d rays_d (tracker / BA)          */
#define LK_FLAG_ALL_DEPTH_POS (1u << 8)  /* caller guarantees gt_depth > 0 for every ray            */
#define LK_FLAG_ZERO_ABSENT   (1u << 9)  /* rays with gt_depth <= 0 are ABSENT (filtered rays of a training batch kept for a
                                           * static shape: the losses ignore them): no far_bb statistics, their samples sit
                                           * between near_end and 0 */
#define LK_FLAG_MAPPER_LOSS   (1u << 10) /* lk_render_fwd also evaluates the mapper loss of the batch (Mapper.py:691-720, what
                                           * lk_loss_mapper computes) inside the composite kernel: reads loss_gt_color /
                                           * loss_w_color, writes d_depth, d_color and loss_out4 = [loss, geo, colour, #masked] */
#define LK_FLAG_UNIT_LOSS_GRADS (1u << 11) /* lk_render_bwd: the caller guarantees |d_color| <= ~1 (sum-type losses such as the mapper's
                                           * and the tracker's L1 colour terms; without ray gradients also |d_depth| <= ~1): the colour
                                           * decoder's backward may then run its products on fp16 pieces with a fixed 2^10 pre-scale
                                           * instead of bf16 pieces.  d_depth reaches the geometry decoder only, whose backward ignores
                                           * the flag */
#define LK_FLAG_Z_GIVEN       (1u << 12) /* lk_render_fwd: rays with gt_depth <= 0 take their S sample depths from `z` as the caller filled
                                         * it (rendering.sample_near_pcl, Renderer.py:152-160) instead of linspace(near_end, far_bb) */
#define LK_FLAG_FEATS_F16     (1u << 13) /* opt-in storage format: geo_feats / col_feats point at IEEE half tables [N,32] (64-byte rows; BASELINE
                                         * config 5 'fp16 features').  Everything computed from them, and their gradients, stays fp32 */
#define LK_FLAG_EMBED_GRADS_ONLY (1u << 14) /* lk_render_bwd, with LK_FLAG_GRAD_WEIGHTS: of the decoder blob only the Fourier matrices
                                           geo_decoder.embedder._B and (REL_POS) color_decoder.embedder_rel_pos._B receive gradients - the
                                           colour decoder's and the rel-pos MLP's matrices are frozen (Mapper.py:531-541 with
                                           fix_color_decoder, the end-of-sequence refinement): no weight-gradient rows are written and no
                                           weight-gradient reduction is launched; the rest of g_weights is left untouched */

#define LK_FLAG_CHECK_RANGE   (1u << 16) /* lk_render_fwd (debug): the decoder kernels test every operand they cut into fp16 pieces (interpolated
                                           features, activations) and set LK_STATUS_ACT_RANGE when one is non-finite or >= 65504 in magnitude */
#define LK_FLAG_GRAD_GEO_DECODER (1u << 15) /* lk_render_bwd, with LK_FLAG_GRAD_WEIGHTS: the geometry decoder's matrices and biases receive
                                           gradients too (mapping.fix_geo_decoder: False, Mapper.py:524-526; every reference config keeps
                                           them frozen and trains geo_decoder.embedder._B alone) - one more launch that redoes the 32-wide
                                           backward chain per sample in plain fp32 from the saved activations (lk_geo_wgrad.hip) */

typedef struct {
    /* ---- sizes */
    int32_t R, S;
    int32_t stats_chunk;        /* rays per far_bb group: R for a training batch, ray_batch_size (3000)
                                   for render_img (Renderer.py:102-121 is evaluated per batch) */
    uint32_t flags;
    /* ---- inputs */
    const float* rays_o;        /* [R,3] */
    const float* rays_d;        /* [R,3] */
    const float* gt_depth;      /* [R]   */
    const float* r2_ray;        /* [R] squared query radius per ray, or NULL -> r2_static */
    lk_knn_t knn;
    const float* pos;           /* [N,3] cloud positions in original order (rel-pos MLP, tracker gradients) */
    const float* geo_feats;     /* [N,32] */
    const float* col_feats;     /* [N,32] */
    const float* weights;       /* packed blob (master, plain [out][in_padded] matrices) */
    const float* weights_frag;  /* lk_weights_repack(weights) */
    const float* affine;        /* [12] exposure transform applied before the sigmoid, or NULL */
    const float* noise_geo;     /* [32] feature of samples without neighbours, or NULL (zeros) */
    const float* noise_col;     /* [32] */
    float near_surface, far_surface, near_end, coef, r2_static;
    int32_t min_nn;
    /* ---- outputs (Renderer.render_batch_ray: src/utils/Renderer.py:71-201) */
    float* depth;               /* [R]   */
    float* var;                 /* [R]   */
    float* color;               /* [R,3] */
    uint8_t* valid_ray;         /* [R]   */
    /* ---- state shared by forward and backward (caller allocated) */
    float* z;                   /* [R,S]   */
    int32_t* nbr_idx;           /* [P,8]   */
    float* nbr_w;               /* [P,8] normalised interpolation weights */
    int32_t* nbr_count;         /* [P]     */
    float* c_geo;               /* [P,32]  */
    float* c_col;               /* [P,32]  */
    float* raw;                 /* [P,4] rgb(or logits), occ */
    float* far_stats;           /* [ceil(R/stats_chunk)] */
    float* act;                 /* SAVE_ACT: lk_render_act_floats(R,S,flags) floats (16-byte aligned), else NULL.  lk_render_fwd leaves there what
                                   lk_render_bwd reads: of the geometry trunk its relu bits (8 words per sample, read by every backward) and its
                                   fp32 relu rows (read with LK_FLAG_GRAD_GEO_DECODER only; lk_track_frame and lk_map_frame without
                                   train_geo_decoder do not write them), of the colour trunk the derivative mask, h_i rows and embedding */
    /* ---- backward inputs */
    const float* d_depth;       /* [R]   */
    const float* d_var;         /* [R] or NULL */
    const float* d_color;       /* [R,3] */
    /* ---- backward outputs (ACCUMULATED into: caller zeroes) */
    float* g_geo_feats;         /* [N,32] */
    float* g_col_feats;         /* [N,32] */
    float* g_weights;           /* blob-shaped */
    float* g_rays_o;            /* [R,3] (overwritten) */
    float* g_rays_d;            /* [R,3] (overwritten) */
    float* g_affine;            /* [12] accumulated, or NULL */
    const uint8_t* grad_row_mask; /* [N] or NULL: feature-row gradients are produced only for rows with a non-zero byte
                                  * (the frustum rows being optimised, Mapper.py:498-512) - the others are never read */
    /* ---- backward scratch */
    float* bwd_scratch;         /* lk_render_bwd_scratch_floats(R,S,flags) floats - the layout depends on `flags`: size it with the
                                 * flags of the call that uses it */
    int64_t bwd_scratch_cap;    /* floats available at bwd_scratch; checked against the layout of the call (0 = unchecked) */
    /* ---- LK_FLAG_MAPPER_LOSS */
    const float* loss_gt_color;  /* [R,3] */
    float* loss_out4;            /* [4] */
    float loss_w_color;
} lk_render_desc;

int64_t lk_render_act_floats(int32_t R, int32_t S, uint32_t flags);
int64_t lk_render_bwd_scratch_floats(int32_t R, int32_t S, uint32_t flags);
/* Renderer.render_batch_ray + NICER.forward + raw2outputs_nerf_color
 * (Renderer.py:71-201, decoder.py:573-610, common.py:382-422). */
int lk_render_fwd(const lk_render_desc* d, void* stream);
/* autograd backward of the same graph (Mapper.py:722, Tracker.py:193). */
int lk_render_bwd(const lk_render_desc* d, void* stream);

/* ---------------------------------------------------------------- losses (fused with d/d outputs)
 * Mapper (src/Mapper.py:691-720, non-exposure branch): mask = gt>0 & valid_ray & !nan(depth);
 *   loss = sum|gt-depth| + w_color*sum|gt_color-color| (colour term only if use_color).
 * Tracker (src/Tracker.py:169-191): u = |gt-depth|/sqrt(var+1e-10); mask = u < 10*mean(u) & gt>0 & !nan;
 *   loss = sum clamp(u,0,1e3) + w_color*sum|gt_color-color|.
 *   lk_loss_tracker's use_color is a flag word: LK_TRACK_USE_COLOR (the colour term takes part in the loss and its gradient) and
 *   LK_TRACK_MEDIAN_MASK (tracking.handle_dynamic: False, Tracker.py:177-179: mask = |gt-depth| < 10*median(|gt-depth|) & gt>0 & !nan,
 *   torch.median = the lower middle value, NaN if any residual is NaN; the loss terms are unchanged).
 * out_loss[0..3] = {loss, geo_loss, color_loss, #masked rays}; d_depth/d_color are overwritten. */
#define LK_TRACK_USE_COLOR   1
#define LK_TRACK_MEDIAN_MASK 2
int lk_loss_mapper(int32_t R, const float* depth, const float* color, const uint8_t* valid_ray,
                   const float* gt_depth, const float* gt_color, float w_color, int32_t use_color,
                   float* d_depth, float* d_color, float* out_loss, void* stream);
int lk_loss_tracker(int32_t R, const float* depth, const float* var, const float* color,
                    const float* gt_depth, const float* gt_color, float w_color, int32_t use_color,
                    float* d_depth, float* d_color, float* out_loss, float* scratch /*[R+8]*/, void* stream);

/* ---------------------------------------------------------------- Adam
 * torch.optim.Adam (amsgrad=False, weight_decay=0) on up to LK_ADAM_MAX_SEG tensors in one launch
 * (Mapper.py:570,723; Tracker.py:352,194).  `step` is the 1-based step count of that tensor. */
#define LK_ADAM_MAX_SEG 16
typedef struct {
    float* p; float* g; float* m; float* v;   /* m, v: compact optimiser state of n floats */
    int64_t n;                                /* elements updated by this segment */
    float lr; int32_t step;
    const int32_t* row_index;                 /* optional: element i lives at p[row_index[i/row_len]*row_len + i%row_len]
                                                 (frustum-selected feature rows updated in place in the full table) */
    int32_t row_len;
    int32_t zero_grad;                        /* clear the consumed gradient entries */
    int32_t p_f16;                            /* p is an IEEE half array (LK_FLAG_FEATS_F16 tables): read as fp32, stepped, rounded to nearest */
    const uint8_t* row_flags;                 /* optional (row_index must be NULL, n a multiple of row_len): [n / row_len] bytes, only the rows
                                                 with a non-zero flag are stepped.  Exact whenever the skipped rows have a zero gradient and zero
                                                 moments (Adam leaves such an element bit for bit where it is): whole-map refinement over millions
                                                 of rows of which an optimize_map call touches a few per cent (lk_map_frame sets the flags) */
    int32_t g_compact;                        /* with row_index: g is indexed like m and v (element i), not like p - the gradient rows arrive
                                                 compact in row-list order (a data-parallel caller's all-reduced bucket); zero_grad is ignored */
} lk_adam_seg;
int lk_adam_step(const lk_adam_seg* host_segs, int32_t n_seg, float beta1, float beta2, float eps, void* stream);

/* Exposure encoding (model.encode_exposure, ScanNet): mlp_exposure = Linear(8,128) -> Softplus(100) -> Linear(128,12)
 * (src/conv_onet/models/decoder.py:534-540) evaluated for F exposure features at once (the keyframes of the mapping window,
 * Mapper.py:588-607, or the tracker's frame, Tracker.py:329-344): aff [F,12] = (3x3 rot | 3 trans), hid [F,128] kept for
 * the backward.  lk_exposure_bwd turns d loss / d aff into g = [W1 1024 | b1 128 | W2 1536 | b2 12 | feats F*8].
 * lk_loss_mapper_exposure is lk_loss_mapper of the colour stage with the per-keyframe affine on the rendered colour LOGITS
 * (Mapper.py:697-715): out d_logits and g_aff [F,12] besides d_depth and [loss, geo, colour, #masked]. */
#define LK_EXPOSURE_MAX_F 32
#define LK_EXPOSURE_GRAD_FLOATS (1024 + 128 + 1536 + 12 + LK_EXPOSURE_MAX_F * 8)
int lk_exposure_fwd(const float* feats, const float* W1, const float* b1, const float* W2, const float* b2, int32_t F,
                    float* aff, float* hid, void* stream);
int lk_exposure_bwd(const float* feats, const float* W1, const float* W2, const float* hid, const float* g_aff, int32_t F,
                    float* g, void* stream);
int lk_loss_mapper_exposure(int32_t R, const float* depth, const float* logits, const uint8_t* valid_ray, const float* gt_depth,
                            const float* gt_color, const int32_t* frame_id, const float* aff, int32_t F, float w_color,
                            float* d_depth, float* d_logits, float* out_loss, float* g_aff, void* stream);

/* Gradient exchange bucket of the ray-sharded data-parallel step (the all-reduce payload of Mapper.py:722-724's
 * step = decoder-gradient spans + the feature-gradient rows being optimised): segment i is `n` floats at `data`
 * (row_index NULL) or the rows data[row_index[k]] of a [*, row_len] table (n = rows * row_len); the bucket is the
 * concatenation of the segments.  unpack = 0: bucket <- segments, 1: segments <- bucket, 2: bucket <- segments and the copied source
 * elements are cleared (for lk_map_desc::grad_bucket: the step then reads the bucket and nothing is unpacked).  One launch either way. */
typedef struct lk_copy_seg {
    float* data;
    int64_t n;
    const int32_t* row_index;
    int32_t row_len;
} lk_copy_seg;
int lk_bucket_copy(const lk_copy_seg* host_segs, int32_t n_seg, float* bucket, int32_t unpack, void* stream);

/* ---------------------------------------------------------------- rays / pose / compaction
 * get_camera_from_tensor + get_rays_from_uv (src/common.py:301-343,104-120): cam = (qw,qx,qy,qz,tx,ty,tz). */
int lk_rays_from_pose(const float* cam7, const float* pix_i, const float* pix_j, int32_t R,
                      float fx, float fy, float cx, float cy, float* rays_o, float* rays_d, void* stream);
/* One launch for a multi-keyframe ray batch: get_samples/get_sample_uv/select_uv/get_rays_from_uv
 * (src/common.py:104-172,237-259; Mapper.py:625-665, Tracker.py:142-146).  Ray r reads frame frame_id[r]
 * (NULL: frame 0) of the stacked images at window pixel rnd[r] in [0, h*w) (row-major over the window
 * [H0,H0+h) x [W0,W0+w)); c2w_stack holds row-major [3|4][4] matrices, c2w_stride floats apart.
 * pix_i/pix_j/r2_ray/r2_map_stack/frame_id may be NULL. */
int lk_gather_rays(const float* depth_stack, const float* color_stack, const float* c2w_stack, int32_t c2w_stride,
                   const float* r2_map_stack, const int32_t* frame_id, const int32_t* rnd, int32_t R,
                   int32_t H, int32_t W, int32_t H0, int32_t W0, int32_t w, float fx, float fy, float cx, float cy,
                   float* rays_o, float* rays_d, float* gt_depth, float* gt_color, float* pix_i, float* pix_j,
                   float* r2_ray, void* stream);
/* d loss / d cam7 from d rays (overwrites g_cam7[7]). */
int lk_pose_bwd(const float* cam7, const float* pix_i, const float* pix_j, int32_t R,
                float fx, float fy, float cx, float cy, const float* g_rays_o, const float* g_rays_d,
                float* g_cam7, void* stream);
/* Stable stream compaction (wave ballot + prefix sum): out_index[0..count) = i with mask[i]!=0. */
int lk_compact(const uint8_t* mask, int32_t n, int32_t* out_index, int32_t* out_count, void* stream);
/* lk_compact for masks of millions of entries (many-workgroup count / scan / scatter; same result).  block_scratch:
 * ceil(n / 256) ints. */
int lk_compact_large(const uint8_t* mask, int32_t n, int32_t* out_index, int32_t* out_count, int32_t* block_scratch, void* stream);
/* Rows of the [N,32] feature tables a batch's neighbour lists refer to: flags[i] = 1 for every 0 <= nbr_idx[j] = i < N, j < n
 * (flags is cleared by the caller).  When the whole map is optimised (final refinement, Mapper.py:884-897; BASELINE config 5)
 * a ray-sharded multi-GPU step exchanges the gradient rows of the union of the ranks' flags only. */
int lk_touch_rows(const int32_t* nbr_idx, int64_t n, uint8_t* flags, int32_t N, void* stream);
/* ORs flags[0..n) into the index's per-row flags of the running optimize_map call (rows whose Adam state may be non-zero: lk_map_frame
 * with rows == NULL steps only these; it clears them at the call's first iteration and sets the rows its own batches touch).  A
 * data-parallel caller passes the MAX-reduced flags of lk_touch_rows: rows only another rank touched receive gradient through the exchange. */
int lk_knn_flag_rows(lk_knn_t knn, const uint8_t* flags, int64_t n, void* stream);
/* ---------------------------------------------------------------- map maintenance around the hot loop
 * Frustum row selection, Mapper.get_mask_from_c2w (src/Mapper.py:165-217): out_index[0..*out_count) = ascending indices
 * of the points of pos[N,3] that project inside the image of the pose (cropped by `edge` pixels, negative = enlarged)
 * and lie no more than 0.5 m behind the observed depth (bilinear lookup as cv2.remap INTER_LINEAR / constant 0 border;
 * zero lookups are replaced by the largest lookup).  w2c12_host = rows 0..2 of inv(c2w) (HOST pointer, 12 floats;
 * the projection itself runs in float64 like the reference's numpy code).  Scratch: float[N], uint8[N], uint32[1]. */
int lk_frustum_rows(const float* pos, int32_t N, const float* w2c12_host, const float* depth, int32_t H, int32_t W,
                    float fx, float fy, float cx, float cy, int32_t edge, float* scratch_depth, uint8_t* scratch_mask,
                    uint32_t* scratch_max, int32_t* out_index, int32_t* out_count, void* stream);
/* Point insertion, geometry part of NeuralPointCloud.add_neural_points (src/neural_point.py:1557-1631): a ray with
 * gt_depth > 0 is accepted iff NO point of the index `knn` (NULL or empty: accept all) lies at squared distance
 * < r2 (r2_per_ray[i] if given, else r2_static) from o + d*gt_depth; accepted ray j (ascending ray order) emits n_add
 * points o + d*z, z = linspace(near_surface*depth, far_surface*depth, n_add), at out_points[(j*n_add + q)*3].
 * out_ray_index[0..*out_count) = accepted rays; out_points must hold 3*n_add*n floats.  Rays of one call are not
 * de-duplicated against each other (as in the reference).  Feature rows of the new points are the caller's
 * (N(0, 0.1), neural_point.py:1614-1617), followed by lk_knn_build on the grown cloud. */
int lk_add_points(lk_knn_t knn, const float* rays_o, const float* rays_d, const float* gt_depth, int32_t n,
                  float r2_static, const float* r2_per_ray, float near_surface, float far_surface, int32_t n_add,
                  uint8_t* scratch_mask, int32_t* out_ray_index, int32_t* out_count, float* out_points, void* stream);
/* Per-frame image pre-passes (Tracker.py:243-268, Mapper.py:854-872, common.py:175-234).
 * lk_radius_maps: grad_mag[H,W] = |Sobel(rgb2gray(color))| (reflected borders), and the dynamic radii as SQUARED
 * float32 maps: r_add = lerp over [0, 0.01, thr] -> [max, max, min] of the clipped magnitude, r_query = ratio * r_add
 * (r2_add / r2_query may be NULL).
 * lk_top_grad_pixels: the K pixels of largest grad_mag over the whole image (ties at the cut in ascending flat index),
 * kept only inside the window [H0,H1) x [W0,W1) and where depth > 0 (depth may be NULL; depth_limit: also <= 5):
 * out_index[0..*out_count) ascending flat indices (out_index must hold K ints).  Images above 16 384 pixels use a library-owned
 * scratch, one per DEVICE (grown with a stream synchronisation when a larger image first arrives): on one device the calls must be
 * ordered - one stream, or streams ordered by events - like the calls on one lk_knn_t handle. */
int lk_radius_maps(const float* color, int32_t H, int32_t W, double color_grad_threshold, double radius_add_max,
                   double radius_add_min, double radius_query_ratio, float* grad_mag, float* r2_add, float* r2_query, void* stream);
int lk_top_grad_pixels(const float* grad_mag, int32_t H, int32_t W, int32_t K, int32_t H0, int32_t H1, int32_t W0, int32_t W1,
                       const float* depth, int32_t depth_limit, int32_t* out_index, int32_t* out_count, void* stream);
/* thr = min(10*median(depth), 1.2*max(depth)) over depth>0 (Tracker.py:153-155, Mapper.py:674-676);
 * mask[i] = depth[i] > 0 && depth[i] <= thr (mask may be NULL); depth_filtered[i] = mask ? depth : 0 (may be
 * NULL or alias depth): a ray with gt_depth 0 is "absent" for the losses, which keeps the batch shape static
 * (no host sync) while matching the reference's boolean-index filtering.  scratch: n uint32. */
int lk_inside_mask(const float* depth, int32_t n, uint8_t* mask, float* depth_filtered, float* out_thr,
                   uint32_t* scratch, void* stream);

/* Exposure encoding inside the per-frame loops (lk_track_frame / lk_map_frame): everything lk_exposure_fwd / _bwd and the Adam groups of
 * mlp_exposure and the exposure features need (Tracker.py:329-344; Mapper.py:524-570, 588-607), all caller-owned.  Per iteration the
 * loops run ONE small launch for it: backward of the MLP from g_aff, Adam on its tensors and on the trainable features, forward with
 * the stepped values for the next iteration, g_aff cleared. */
typedef struct {
    float* feats;               /* [F,8] exposure features (tracker: F = 1; mapper: the keyframes of the window, the current frame last) */
    float* W1; float* b1; float* W2; float* b2;      /* mlp_exposure: [128,8], [128], [12,128], [12] - stepped in place */
    int32_t F;                  /* 1 .. LK_EXPOSURE_MAX_F */
    float* aff;                 /* [F,12] */
    float* hid;                 /* [F,128] */
    float* g_aff;               /* [F,12] d loss / d aff of the iteration (accumulated by the loss / decoder kernels) */
    float* g;                   /* [LK_EXPOSURE_GRAD_FLOATS] layout of lk_exposure_bwd */
    float* adam;                /* [2][LK_EXPOSURE_GRAD_FLOATS] exp_avg | exp_avg_sq in the layout of g; zeroed by the caller (fresh optimiser) */
    float lr_mlp;               /* Adam rate of the four MLP tensors (tracker 1e-3; mapper: decoders_lr of stage 'color'); < 0: frozen */
    float lr_feat;              /* Adam rate of the trainable features (1e-3) */
    int32_t feat_first, feat_count;      /* features [feat_first, feat_first + feat_count) are Adam parameters (mapper: only the last) */
    float* bwd_scale;           /* [1] or NULL.  With it the colour decoder's backward and the weight-gradient reductions of the loops run on
                                   pre-scaled fp16 pieces as under LK_FLAG_UNIT_LOSS_GRADS although the loss gradient passes through the
                                   LEARNED affines: every forward of the MLP stores here the power of two that maps 3 max|A| into (0.5, 1]
                                   - the bound of |d out| relative to the plain colour loss - and the kernels apply it on top of their 2^10 */
} lk_exposure_desc;

/* ---------------------------------------------------------------- per-frame optimisation loops
 * The launch sequences of the reference's two inner loops as ONE call each, so that the host enqueues a frame's work in
 * microseconds instead of interpreting ~20 Python statements per iteration (at 1 500-ray tracking batches the Python loop
 * was slower than the GPU).  Static shapes, no host synchronisation inside; every buffer is the caller's.
 *
 * lk_track_frame: Tracker.run's loop body for one frame (src/Tracker.py:313-401) = iters x { pixel gather + rays of the
 * current pose + inside mask (Tracker.py:142-160), lk_render_fwd in tracker mode, tracker loss (Tracker.py:169-191),
 * lk_render_bwd w.r.t. the rays, pose gradient, Adam on (T | quaternion) (Tracker.py:317-352) }.  For R <= 8192 the small
 * steps run as three one-workgroup kernels (batch assembly; composite + loss + composite backward; ray / pose gradient +
 * Adam) - 9 launches per iteration instead of 16.
 * render: R, S, the map (knn, pos, tables, weights), scalars, and ALL per-call buffers of lk_render_fwd / lk_render_bwd
 * (rays_o, rays_d, gt_depth, r2_ray or NULL, outputs, state, act, d_depth, d_color, g_rays_o, g_rays_d, bwd_scratch sized
 * for flags | TRACKER | STAGE_COLOR | SAVE_ACT | GRAD_RAYS | ZERO_ABSENT); render.flags carries LK_FLAG_REL_POS only. */
typedef struct {
    lk_render_desc render;
    const float* depth_img;     /* [H,W]   */
    const float* color_img;     /* [H,W,3] */
    const float* r2_map;        /* [H,W] squared dynamic query radius per pixel, or NULL */
    int32_t H, W, H0, W0, w;    /* draw q of rnd -> pixel (row H0 + q / w, column W0 + q % w) */
    float fx, fy, cx, cy;
    const int32_t* rnd;         /* [iters][R] pixel draws (window pixels, or flat image indices with H0 = W0 = 0, w = W) */
    float* gt_color;            /* [R,3] */
    float* pix_i; float* pix_j; /* [R]   */
    float* thr;                 /* [1]   */
    uint32_t* scratch_u32;      /* [R]   */
    float* loss_scratch;        /* [R+8] */
    float* cam7;                /* [7] in: initial pose (qw,qx,qy,qz,tx,ty,tz); out: pose after the last iteration */
    float* g_cam7;              /* [7] */
    float* adam_mv;             /* [14] exp_avg | exp_avg_sq of the pose; zeroed by the call (fresh optimiser per frame) */
    float lr_T, lr_q;           /* separate_LR: cam_lr and 0.2 cam_lr (Tracker.py:317-333); otherwise both cam_lr */
    float w_color; int32_t use_color;   /* flag word as for lk_loss_tracker: LK_TRACK_USE_COLOR | LK_TRACK_MEDIAN_MASK */
    int32_t hist_post;          /* 0: hist[it] = pose BEFORE iteration it (separate_LR: the candidate is a detached copy);
                                   1: pose AFTER its update (one leaf tensor stepped in place, Tracker.py:375-377) */
    float* hist;                /* [iters][7] candidate poses */
    float* log;                 /* [iters][4] loss, geo, colour, #masked rays per iteration; complete when the call's work has
                                 * completed (a row may be written by the iteration AFTER its own: the pose step sums its terms) */
    int32_t iters;
    float* work;                /* lk_track_work_floats(R, S, iters) floats: with it (and R <= 8192) every iteration's pixels, colours,
                                   radii and inside mask are assembled by ONE launch up front and the small steps of an iteration run
                                   fused (4 launches per iteration instead of 16); gt_color / pix_i / pix_j / thr / scratch_u32 /
                                   loss_scratch and render.g_rays_o / g_rays_d are then not used and may be NULL.  NULL: the
                                   per-iteration launch sequence */
    const lk_exposure_desc* exposure;   /* model.encode_exposure (HOST pointer) or NULL: the frame's affine is applied per sample inside the
                                   colour decoder (decoder.py:534-540); feature and MLP are stepped every iteration (Tracker.py:329-344) */
} lk_track_desc;
int64_t lk_track_work_floats(int32_t R, int32_t S, int32_t iters);
int lk_track_frame(const lk_track_desc* d, void* stream);

/* lk_map_frame: the joint iterations [it_begin, it_end) of one Mapper.optimize_map call (src/Mapper.py:576-735) = per iteration { multi-keyframe ray gather, inside mask, lk_render_fwd with the fused mapper loss, lk_render_bwd,
 * Adam over {decoder spans, geometry rows, colour rows}, fragment repack in stage 'color' }.  Iteration it runs stage
 * 'geometry' iff it < n_geo_iters.  phases: 1 = forward/backward only, 2 = optimiser step only, 3 = both (a ray-sharded
 * multi-GPU caller all-reduces the gradients between phase 1 and phase 2 of every iteration).
 * render: as for lk_track_frame (flags: LK_FLAG_REL_POS, + LK_FLAG_UNIT_LOSS_GRADS if wanted; g_geo_feats, g_col_feats,
 * g_weights, grad_row_mask, bwd_scratch sized for STAGE_COLOR | SAVE_ACT | GRAD_FEATS | GRAD_WEIGHTS). */
#define LK_MAX_SPANS 8
typedef struct { int64_t offset, n; } lk_blob_span;       /* floats [offset, offset + n) of the weight blob */
typedef struct {
    lk_render_desc render;
    const float* depth_stack; const float* color_stack; const float* c2w_stack; int32_t c2w_stride;
    const float* r2_map_stack;  /* or NULL */
    const int32_t* frame_id;    /* [R] keyframe of every ray */
    const int32_t* rnd;         /* [iters][R] */
    int32_t H, W, H0, W0, w;
    float fx, fy, cx, cy;
    float* gt_color; float* thr; uint32_t* scratch_u32;
    float w_color;
    float* log;                 /* [iters][4] as lk_track_desc::log; the rows of a call's iterations are complete at the END of that
                                 * lk_map_frame call (one launch sums the per-tile terms the decoder backward left) */
    /* optimiser (a fresh Adam per optimize_map call, Mapper.py:570: the caller zeroes the state buffers) */
    float* weights_rw;          /* = render.weights, writable */
    float* weights_frag_rw;     /* = render.weights_frag, writable */
    float* geo_feats_rw; float* col_feats_rw;     /* = render.geo_feats / col_feats, writable */
    const int32_t* rows;        /* [n_rows] rows being optimised, or NULL = all N rows (then n_rows = N) */
    int64_t n_rows;
    float* adam_rows;           /* [4][n_rows*32]: exp_avg, exp_avg_sq of the geometry rows, then of the colour rows */
    lk_blob_span geo_dec[LK_MAX_SPANS]; int32_t n_geo_dec;   /* decoder spans stepped in both stages (embedder._B) */
    lk_blob_span col_dec[LK_MAX_SPANS]; int32_t n_col_dec;   /* decoder spans stepped in stage 'color' */
    float* adam_dec;            /* [2][lk_weight_blob_floats()]: exp_avg | exp_avg_sq, blob-shaped */
    float lr[2][3];             /* [stage: geometry, colour][decoders, geometry rows, colour rows] (configs mapping.stage.*) */
    int32_t iters, n_geo_iters;
    float* work;                /* lk_map_work_floats(R, S, iters) floats, or NULL: as lk_track_desc.work - the batches (pixels, rays, colours,
                                   radii, inside masks) of all `iters` iterations are assembled by one launch of the call that starts at
                                   it_begin = 0 (gt_color / thr / scratch_u32 and render.rays_o / rays_d / gt_depth are then unused) */
    const lk_exposure_desc* exposure;   /* model.encode_exposure (HOST pointer) or NULL: the 'color' iterations render colour LOGITS and the loss
                                   applies sigmoid(logits @ rot_f + trans_f) of the ray's keyframe f = frame_id (Mapper.py:697-715);
                                   needs `work`; bwd_scratch sized WITHOUT LK_FLAG_UNIT_LOSS_GRADS (d logits = w sigma' A is unbounded) */
    const float* grad_bucket;   /* phase-2 calls of a data-parallel caller (rows != NULL, no exposure): the all-reduced gradient bucket or NULL.  With
                                   it the step reads its gradients from the bucket itself - decoder span k of the geometry / colour list at float
                                   offset bucket_geo_dec[k] / bucket_col_dec[k], the optimised rows of the two tables compact (row-list order) at
                                   bucket_geo_rows / bucket_col_rows - and no unpack launch is needed; the caller packs with lk_bucket_copy mode 2
                                   (copy + clear the source: what the step's zero_grad would have done) */
    int64_t bucket_geo_dec[LK_MAX_SPANS], bucket_col_dec[LK_MAX_SPANS];
    int64_t bucket_geo_rows, bucket_col_rows;
    int32_t union_rows_flagged; /* rows == NULL, phase-split (data-parallel) callers: non-zero = between phase 1 and phase 2 of every iteration
                                   the caller ORs the union of the rows ALL ranks touched into the index's row flags (lk_knn_flag_rows); the
                                   step then visits the flagged rows only, as the single-process call does on its own (0: dense step) */
    int32_t it_offset;          /* a long optimize_map call may be issued as consecutive SEGMENTS, one descriptor each: this one covers the
                                   iterations it_offset .. it_offset + iters - 1 of the call (rnd, log and work are the segment's own; iters
                                   sizes them), n_geo_iters stays the call's GLOBAL count, the optimiser state (adam_rows, adam_dec) carries
                                   over and the step counts continue.  The work buffer then holds one segment's batches and neighbour
                                   lists instead of the whole call's (26 floats per sample and iteration).  0 for an unsegmented call */
    int32_t batches_ready;      /* non-zero: lk_map_prepare has already assembled this descriptor's batches (see there) */
    int32_t train_geo_decoder;  /* mapping.fix_geo_decoder: False (Mapper.py:524-526): the geometry decoder's own matrices and biases are parameters too - they are
                                   listed in geo_dec (all of the decoder's used tensors), every backward also forms their gradients
                                   (LK_FLAG_GRAD_GEO_DECODER: size render.bwd_scratch with that flag), and the matrix fragments are refreshed after the
                                   'geometry' steps as well */
    int32_t signal_rows;        /* phase-1 calls of a data-parallel caller: non-zero = the backward records a library-owned event on the launch stream
                                   right behind the feature-row gather - the point from which g_geo_feats / g_col_feats of the iteration are final,
                                   while the weight-gradient launch and the reduction of the decoder gradients are still to run.  lk_map_wait_rows
                                   makes another stream wait for it: the caller exchanges the row part of its gradient bucket there, beside the
                                   tail of the backward (loopy_slam_amd/parallel.py) */
} lk_map_desc;
int64_t lk_map_work_floats(int32_t R, int32_t S, int32_t iters);
/* The batch assembly of lk_map_frame's first call (pixels, rays, colours, radii, inside masks of all `iters` iterations: one launch) AHEAD of
 * that call: it reads the batch inputs of the descriptor only (stacks, frame_id, rnd, window, intrinsics, render.R / S / r2_ray, work, iters,
 * log, exposure) - not the row list, not the map.  A caller whose row list comes out of a device-side selection with a count read-back
 * (Mapper.get_mask_from_c2w -> lk_frustum_rows) enqueues this BEFORE the read-back, so that the device assembles batches while the host
 * waits and fills in the rest of the descriptor; the lk_map_frame call then carries batches_ready = 1. */
int lk_map_prepare(const lk_map_desc* d, void* stream);
/* float offset inside `work` of the neighbour lists lk_map_frame keeps per iteration: int32 [iters][R*S][8] (what a data-parallel
 * caller needs to agree on the touched rows of an iteration, loopy_slam_amd/parallel.py) */
int64_t lk_map_work_nbr_idx(int32_t R, int32_t S, int32_t iters);
/* One render / backward sequence per kNN handle at a time: the handle owns the row counters of the gradient sort (zero between calls: the
 * scan that consumes them clears them) and lk_map_frame's look-ahead search and sort run on a library-owned stream.  The call with
 * it_begin = 0 joins that stream before it touches `work`; after an ERROR return from lk_map_frame / lk_render_bwd the counters may be
 * stale - lk_knn_build (which clears them) before the handle renders a backward again. */
/* Phase-split callers (phases 1, then 2, per iteration): the phase-2 call of a 'color' iteration that is not the call's last leaves the
 * fragment repack to the phase-1 call of the NEXT iteration (it rides in that call's interpolation launch, as in the unsplit loop) - the
 * iterations of an optimize_map call must be issued in order, each phase 1 followed by its phase 2. */
int lk_map_frame(const lk_map_desc* d, int32_t it_begin, int32_t it_end, int32_t phases, void* stream);
/* Makes `stream` wait until the neighbour lists of iteration `it` (work + lk_map_work_nbr_idx) are written: lk_map_frame
 * searches ahead of its loop on a library-owned stream.  Valid after the phase-1 call of iteration it - 1 (or it) of the same
 * optimize_map call has returned. */
int lk_map_wait_lists(const lk_map_desc* d, int32_t it, void* stream);
/* `stream` waits until the feature-row gradients of the LAST phase-1 call issued with lk_map_desc::signal_rows are final.  The event is
 * recorded on that call's launch stream whatever the library's stream mode (with LK_SERIAL / lk_set_serial, or after a failed side-stream
 * creation, too: the waiter always gets a real dependency on the backward); a no-op only if no call has signalled yet. */
int lk_map_wait_rows(const lk_map_desc* d, void* stream);

/* ---------------------------------------------------------------- weight-gradient building block
 * dW[n][k] += sum_rows A'[row][n] * B[row][k], db[n] += sum_rows A'[row][n] (db may be NULL); row-major operands.
 * a_mode 0: A' = A;  1: A' = A * softplus100'(A2) with A2 the activation OUTPUT;  2: A' = A2[row] * A[row>>3]
 * (rel-pos: per-neighbour weight times the per-sample gradient).  This is what lk_render_bwd runs for every
 * decoder matrix (torch: grad of nn.Linear weights, decoder.py:265-288,480-546). */
int lk_wgrad_single(const float* A, int32_t lda, int32_t a_mode, const float* A2, int32_t lda2,
                    const float* B, int32_t ldb, int32_t N, int32_t K, int64_t rows,
                    float* dW, int32_t ldw, float* db, int32_t chunk, void* stream);

/* ---------------------------------------------------------------- loop closure: segment registration and map correction
 * The per-point work of the reference's loop closure (src/common.py: estimate_normals / pairwise_registration /
 * register_point_cloud_pair around Open3D; src/neural_point.py: apply_transformation).  Place recognition and the pose graph
 * are the caller's (loopy_slam_amd/loop_closure.py); these three calls are what touches every point.
 *
 * lk_normals: for every point i of the cloud pos[N,3] that `knn` was built over, the covariance of ALL indexed points with
 * d2 <= radius^2 (contract distance, the point itself included; Open3D's hybrid search would stop at the 50 nearest), and the unit
 * eigenvector of its smallest eigenvalue (fp32 Jacobi), flipped to face host_camera3 (HOST pointer, 3 floats).  Fewer than 3
 * neighbours: out_valid[i] = 0 and a zero normal.  The sums follow the grid's cell order, which one build fixes: repeated calls on one
 * build are bit-identical, a rebuilt index may differ in the last bits. */
int lk_normals(lk_knn_t knn, const float* pos, int64_t N, float radius, const float* host_camera3,
               float* out_normals /*[N,3]*/, uint8_t* out_valid /*[N]*/, void* stream);
/* lk_normals_nn: the same over the max_nn NEAREST neighbours within the radius (Open3D's hybrid search; a segment's fused surface cloud holds
 * on the order of a thousand vertices per 0.1-m ball, and the cap IS the support of a normal there).  For point i the candidates are all
 * indexed points with contract distance d2 = (dx dx + dy dy) + dz dz <= fl(radius * radius), the point itself included - lk_normals' set.
 * Of them the min(count, max_nn) smallest under the total order (d2, index) are selected: out_count[i] (or NULL) is that number,
 * out_nbr[i][0 .. max_nn) (or NULL) their indices in that order, padded with -1.  The covariance runs over the selection, the sums relative
 * to point i, in fp32, ADDED IN ASCENDING (d2, index) ORDER; then lk_normals' Jacobi, smallest eigenvector and flip towards host_camera3.
 * Fewer than 3 selected points: out_valid[i] = 0 and a zero normal.  Selection and sum order are fixed by the cloud alone, so equal inputs
 * give equal bits, also after the index is rebuilt (lk_normals cannot promise that).  No floating-point atomics.
 * LK_ERR_ARG: max_nn < 1, max_nn > LK_NORMALS_MAX_NN, radius <= 0, N != the size of the index.  N = 0 is a no-op. */
#define LK_NORMALS_MAX_NN 64
int lk_normals_nn(lk_knn_t knn, const float* pos, int64_t N, float radius, int32_t max_nn, const float* host_camera3,
                  float* out_normals /*[N,3]*/, uint8_t* out_valid /*[N]*/, int32_t* out_count /*[N] or NULL*/,
                  int32_t* out_nbr /*[N][max_nn] or NULL*/, void* stream);
/* One Gauss-Newton step's sums of point-to-plane ICP, or the sums of the correspondence information matrix.
 * Every source point p of src[P,3] is moved by the row-major 3 x 4 transform host_T12 (HOST pointer; three fused multiply-adds per
 * coordinate, s_x = fma(T00, p_x, fma(T01, p_y, fma(T02, p_z, T03))), so the identity reproduces p exactly); its correspondence is the
 * nearest point q of the index under the contract above with d2 <= fl(max_dist * max_dist), order (d2, index); out_corr[P] (or NULL)
 * receives its index, -1 if there is none.  tgt_pos[N,3] is the array the index was built over.
 *   LK_ICP_POINT_TO_PLANE: correspondences whose target normal is valid contribute r = n.(s - q), J = [s x n | n],
 *     w = (1 - (r/k)^2)^2 for |r| <= k else 0 (tukey_k <= 0: w = 1):
 *     out_sums[0..20] = upper triangle of sum w J^T J row by row, [21..26] = sum w J^T r, [27] = their count, [28] = sum d2,
 *     [29] = sum w r^2, [30..31] = 0.
 *   LK_ICP_INFORMATION: every correspondence contributes G = [-[q]x | I] (normals may be NULL):
 *     out_sums[0..20] = upper triangle of sum G^T G, [27] = count, [28] = sum d2, the rest 0.
 * out_sums: LK_ICP_SUMS doubles in DEVICE memory.  scratch: lk_icp_scratch_floats(P) floats (one row of fp32 partials per workgroup).
 * The reduction has a fixed order (lane -> wave -> workgroup row -> rows ascending in fp64, no atomics): equal inputs give equal bits. */
#define LK_ICP_POINT_TO_PLANE 0
#define LK_ICP_INFORMATION 1
#define LK_ICP_SUMS 32
int64_t lk_icp_scratch_floats(int64_t P);
int lk_icp_accumulate(lk_knn_t tgt, const float* tgt_pos, const float* tgt_normals, const uint8_t* tgt_valid, const float* src,
                      int64_t P, const float* host_T12, float max_dist, float tukey_k, int32_t mode, int32_t* out_corr,
                      float* scratch, int64_t scratch_floats, double* out_sums, void* stream);
/* In place on pos[N,3]: p <- R[s] p + t[s], s = seg_id[i], mats[n_seg][12] row-major 3 x 4 in device memory (three fused
 * multiply-adds per coordinate).  Rows whose matrix is exactly the identity, and rows with s outside [0, n_seg), keep their bits.
 * The neighbour index is stale afterwards: lk_knn_build. */
int lk_apply_correction(float* pos, int64_t N, const int32_t* seg_id, const float* mats, int32_t n_seg, void* stream);
/* In place on pos[N,3]: p <- R p + t with ONE row-major 3 x 4 matrix host_M12 (HOST pointer) for the whole array - a stored surface cloud
 * of a segment, which has no label per row.  lk_apply_correction's arithmetic (three fused multiply-adds per coordinate); a matrix that is
 * exactly the identity launches nothing, so the bits stay. */
int lk_rigid_map(float* pos, int64_t N, const float* host_M12, void* stream);

/* ---------------------------------------------------------------- loop closure: global start (FPFH + RANSAC)
 * What the reference's default "robust_icp" runs before its ICP (src/common.py: preprocess_point_cloud, execute_global_registration around
 * Open3D).  fp32 throughout, no floating-point atomics, every sum in an order fixed by the inputs: equal inputs and seed give equal bits.
 *
 * Voxel downsample.  lk_voxel_keys: key[i] = (kx << 42) | (ky << 21) | kz with k = clamp(floor((p - origin) / voxel), 0, LK_VOXEL_AXIS_MAX) per
 * axis, the subtraction and the division each rounded once (host_origin3: HOST pointer; the caller passes min - 0.5 voxel).  The caller sorts
 * the keys (stable) and passes the sorted keys to lk_voxel_heads (head[i] = 1 where a voxel's run begins), compacts the heads (lk_compact_large)
 * into `starts`, and lk_voxel_downsample writes one centroid per voxel, in ascending key order: the points order[starts[j]] .. of the run are
 * summed in that order relative to the first of them, divided by their number and added back to it. */
#define LK_VOXEL_AXIS_MAX 2097151
int lk_voxel_keys(const float* pos, int64_t N, const float* host_origin3, float voxel, int64_t* out_keys, void* stream);
int lk_voxel_heads(const int64_t* sorted_keys, int64_t N, uint8_t* out_head, void* stream);
int lk_voxel_downsample(const float* pos, int64_t N, const int64_t* order /*[N] point of each sorted key*/, const int32_t* starts /*[n_vox]*/,
                        int32_t n_vox, float* out_centroids /*[n_vox,3]*/, void* stream);
/* Re-orders the points inside every cell of a built index by ascending point index.  lk_knn_build leaves them in the order its counting
 * atomics landed; afterwards every walk over the index (lk_normals, lk_fpfh) meets the points in an order the cloud alone fixes, so its
 * floating-point sums have the same bits after every rebuild.  Query results do not change. */
int lk_knn_canonicalize(lk_knn_t knn, void* stream);
/* FPFH (Rusu et al. 2009) with Open3D's conventions over ALL indexed points k != i with contract d2 <= radius^2 and a valid normal (Open3D
 * stops at the 100 nearest).  Pair features of (p1 = point i, n1) and (p2 = neighbour, n2): e = p2 - p1, d = |e|, a1 = n1.e / d, a2 = n2.e / d;
 * if |n1.e| < |n2.e| (acos|a1| > acos|a2|; this one comparison in fp64 on the exact differences - ties are common: a neighbour along the
 * normal - and they flip the sign of f2) the roles swap: u = n2, m = n1, e = -e, f2 = -a2, else u = n1, m = n2, f2 = a1;
 * v = (e x u) / |e x u|, w = u x v, f1 = v.m, f0 = atan2(w.m, u.m); d = 0 or |e x u| = 0: f0 = f1 = f2 = 0.
 * Bins: clamp(floor(11 (f0 + pi) / (2 pi)), 0, 10), 11 + clamp(floor(11 (f1 + 1) / 2), 0, 10), 22 + clamp(floor(11 (f2 + 1) / 2), 0, 10);
 * out_spfh[i][bin] = (pairs in the bin) x (100 / number of neighbours).
 * out_fpfh[i][b] = scale[b / 11] x (sum over the neighbours with d2 > 0 of out_spfh[k][b] / d2) + out_spfh[i][b], scale = 100 / (the sum of
 * the block's 11 neighbour sums), 0 for a zero block.  The neighbour sums follow the canonical cell order (lk_knn_canonicalize).
 * A point with valid[i] = 0 gets zero rows and is nobody's neighbour. */
#define LK_FPFH_DIM 33
int lk_fpfh(lk_knn_t knn, const float* pos, const float* normals, const uint8_t* valid, int64_t N, float radius,
            float* out_spfh /*[N,33]*/, float* out_fpfh /*[N,33]*/, void* stream);
/* For every row i of A[Na,33]: out_idx[i] = the row j of B[Nb,33] with the smallest (d2, j), d2 = sum over the 33 columns ascending of
 * (A[i][c] - B[j][c])^2 (each term rounded, added one by one), out_d2[i] = that d2.  Rows with validB[j] = 0 are never chosen; a row with
 * validA[i] = 0, or without a candidate, gets -1 and 0.  The masks may be NULL (all valid). */
int lk_feature_match(const float* A, const uint8_t* validA, int64_t Na, const float* B, const uint8_t* validB, int64_t Nb,
                     int32_t* out_idx, float* out_d2, void* stream);
/* RANSAC over M correspondences corr[M][2] = (source point, target point); lk_ransac_gather copies their points into cs[M,3] / ct[M,3].
 * lk_ransac_hypotheses, trial t = trial0 + (0 .. n_trials): (r0, r1, r2, r3) = Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 * (t & 0xffffffff, t >> 32, 0, 0) - ten rounds of
 *     (c0, c1, c2, c3) <- (hi(0xCD9E8D57 c2) ^ c1 ^ k0, lo(0xCD9E8D57 c2), hi(0xD2511F53 c0) ^ c3 ^ k1, lo(0xD2511F53 c0)),
 *     then (k0, k1) += (0x9E3779B9, 0xBB67AE85)
 * - and the three correspondences are i_k = (r_k x M) >> 32, k = 0, 1, 2 (out_triples[n_trials,3], may be NULL).  The trial is dropped when two
 * indices are equal, when for one of the sides (0,1), (1,2), (2,0) |s_a - s_b| < edge_ratio |t_a - t_b| or the other way round, or when after
 * the rigid least-squares fit of the three pairs (Horn's unit quaternion by cyclic Jacobi, no scale, det = +1; this fit alone runs in fp64 and is rounded to fp32: a thin triangle loses
 * the rotation about its long side in fp32) one of the three points lies
 * more than dist_thr from its partner.  out_ok[n_trials] = 1 for a survivor, out_T[n_trials,12] its row-major 3 x 4 transform (zeros else).
 * lk_ransac_score: for hypothesis h < *n_survivors (device), transform out_T[survivors[h]]: out_count[h] = number of correspondences with
 * d2(T s, t) <= dist_thr^2 (the points moved by three fused multiply-adds per coordinate as in lk_icp_accumulate), out_sum_d2[h] = their d2
 * summed per lane of a 64-lane wave over j = lane, lane + 64, .. and then by an xor butterfly (1, 2, .., 32).
 * lk_ransac_best folds the batch into best[LK_RANSAC_BEST] (int32, device; set best[0] = -1 and the rest 0 before the first batch):
 * [0] count, [1] bits of sum d2, [2] / [3] trial low / high, [4..15] bits of the transform, [16] survivors so far.  Order: count descending,
 * sum d2 ascending, trial ascending. */
#define LK_RANSAC_BEST 20
int lk_ransac_gather(const float* src, const float* tgt, const int32_t* corr, int32_t M, float* out_cs, float* out_ct, void* stream);
int lk_ransac_hypotheses(const float* cs, const float* ct, int32_t M, uint64_t seed, uint64_t trial0, int32_t n_trials, float edge_ratio,
                         float dist_thr, int32_t* out_triples, uint8_t* out_ok, float* out_T, void* stream);
int lk_ransac_score(const float* cs, const float* ct, int32_t M, const float* T_all, const int32_t* survivors, const int32_t* n_survivors,
                    int32_t max_survivors, float dist_thr, int32_t* out_count, float* out_sum_d2, void* stream);
int lk_ransac_best(const int32_t* count, const float* sum_d2, const int32_t* survivors, const int32_t* n_survivors, const float* T_all,
                   uint64_t trial0, int32_t* best, void* stream);

/* ---------------------------------------------------------------- TSDF fusion and meshing
 * What the reference does with Open3D's ScalableTSDFVolume at the end of a run (src/tools/get_mesh_tsdf_fusion.py).  fp32 throughout, no
 * atomics: every voxel, cube and vertex has one owning thread, so equal inputs give equal bits.
 *
 * Volume.  A block is 16^3 voxels of edge `voxel`; block (bx, by, bz) = floor(p / (16 voxel)) per axis has the key
 * ((bx + 2^20) << 42) | ((by + 2^20) << 21) | (bz + 2^20) (the bit order of lk_voxel_keys).  Blocks live in slots in allocation order:
 * slot_keys[n_slots] holds their keys, planes[n_slots][5][4096] their tsdf, weight, r, g, b (r, g, b in 0 .. 255), a plane in [z][y][x] order;
 * a new slot is all zeros.  The centre of voxel i of block b along an axis is ((float)(16 b + i) + 0.5f) * voxel.
 *
 * Camera.  host_c2w16: HOST pointer, row-major 4 x 4 of the project's camera (x right, y up, looking down -z).  Both calls negate its columns 1
 * and 2 (the reference's flip into Open3D's axes) once on the host; lk_tsdf_integrate inverts the result in fp64 and rounds once.  Points are
 * moved by three fused multiply-adds per coordinate, as in lk_icp_accumulate.
 *
 * lk_tsdf_touch: every stride-th pixel (rows 0, stride, ..; columns likewise; sample s = (row / stride) * ceil(W / stride) + column / stride) with
 * 0 < depth < depth_trunc is back-projected, p = c2w ((px - cx) d / fx, (py - cy) d / fy, d), and out_keys[s][0..8) receives the keys of the blocks
 * that the box p +- sdf_trunc overlaps (floor((p - sdf_trunc) / (16 voxel)) .. floor((p + sdf_trunc) / (16 voxel)) per axis), -1 in the unused
 * places and for a pixel without depth.  2 sdf_trunc <= 16 voxel is required (at most 2 blocks per axis): LK_ERR_ARG otherwise.
 *
 * lk_tsdf_integrate: one workgroup per entry of touched_slots[n_touched] (distinct slots).  Per voxel: (x, y, z) = w2c centre; if z > 0:
 * u = x fx / z + cx + 0.5, v = y fy / z + cy + 0.5; if 0 <= u < W and 0 <= v < H: pixel ((int)u, (int)v) with depth d; if 0 < d < depth_trunc:
 * sdf = (d - z) sqrt(xx^2 + yy^2 + 1), xx = ((int)u - cx) / fx, yy = ((int)v - cy) / fy; if sdf > -sdf_trunc: t = min(1, sdf / sdf_trunc),
 * tsdf <- (tsdf w + t) / (w + 1), r, g, b likewise with floor(clip(c, 0, 1) 255) of color[H, W, 3], w <- w + 1.  Other voxels are not written. */
int lk_tsdf_touch(const float* depth, int32_t H, int32_t W, const float* host_c2w16, float fx, float fy, float cx, float cy, int32_t stride,
                  float depth_trunc, float sdf_trunc, float voxel, int64_t* out_keys /*[ceil(H/stride) ceil(W/stride), 8]*/, void* stream);
int lk_tsdf_integrate(float* planes, const int64_t* slot_keys, int32_t n_slots, const int32_t* touched_slots, int32_t n_touched,
                      const float* depth, const float* color, int32_t H, int32_t W, const float* host_c2w16, float fx, float fy, float cx,
                      float cy, float voxel, float sdf_trunc, float depth_trunc, void* stream);
/* Marching cubes over the blocks, indexed and welded by construction.  The caller sorts the keys: sorted_slots[n_blocks] is the slot of the
 * block at each position, nbr[n_blocks][8] the position of the block at offset o = dx | dy << 1 | dz << 2 (nbr[.][0] unused), -1 if absent.
 * The cube of voxel (i, j, k) has its corners c = dx | dy << 1 | dz << 2 at the voxel centres (i + dx, j + dy, k + dz); it is active iff all
 * eight exist with weight > 0; case bit c = (tsdf < 0).  Edge e = 4 axis + b1 + 2 b2 runs along `axis` from the corner whose other two offsets
 * are (b1, b2) in ascending axis order; its owner is (block position, voxel) of that lower corner plus the axis.
 * lk_mc_mark: out_case / out_ntri[n_blocks 4096] = case (0 if inactive) and triangle count of every cube; edge_flag[n_blocks 4096 3] (zeroed by
 *   the caller) gets a 1 at ((position 4096 + voxel) 3 + axis) of every cut edge of an active cube.
 * The caller compacts edge_flag (lk_compact_large) into vert_index[V]: vertex ids in (position, voxel, axis) order; and sums out_ntri into
 *   tri_end[n_blocks 4096] (inclusive).
 * lk_mc_vertices: vertex v on its edge at p0 + f0 / (f0 - f1) (p1 - p0), out_col the planes r, g, b interpolated alike and divided by 255.
 * lk_mc_triangles: out_tri[F, 3] = the vertex ids of every active cube's triangles (the generated table csrc/lk_mc_table.h; normals point from
 *   tsdf < 0 to tsdf >= 0), cube after cube in (position, voxel) order. */
int lk_mc_mark(const float* planes, const int32_t* sorted_slots, const int32_t* nbr, int32_t n_blocks, uint8_t* out_case, uint8_t* out_ntri,
               uint8_t* edge_flag, void* stream);
int lk_mc_vertices(const float* planes, const int64_t* slot_keys, const int32_t* sorted_slots, const int32_t* nbr, int32_t n_blocks,
                   const int32_t* vert_index, int32_t V, float voxel, float* out_pos /*[V,3]*/, float* out_col /*[V,3]*/, void* stream);
int lk_mc_triangles(const int32_t* sorted_slots, const int32_t* nbr, int32_t n_blocks, const uint8_t* cube_case, const int32_t* tri_end,
                    const int32_t* vert_index, int32_t V, int32_t* out_tri /*[F,3]*/, void* stream);

/* ---------------------------------------------------------------- reconstruction evaluation
 * What the reference runs on the host at the end of an experiment (src/tools/cull_mesh.py, src/tools/eval_recon.py around trimesh, Open3D and
 * scipy's cKDTree).  fp32 except the sampler's cumulative area table; the only atomic is the z-buffer's unsigned integer minimum: equal inputs
 * and an equal seed give equal bits.
 *
 * lk_nearest: for every query of queries[P,3] the nearest point of the index under the contract distance d2 = (dx dx + dy dy) + dz dz (each
 * operation rounded once), order (d2, index): out_d2[P] and out_idx[P].  max_dist = +infinity: the minimum over ALL indexed points, wherever the
 * query lies (the search box doubles from one cell edge until the hit lies inside the half-width searched or the box covers the grid).  Finite
 * max_dist: candidates are the points with d2 <= fl(max_dist * max_dist); a query without one gets index -1 and d2 = +infinity, as does every
 * query of an empty index. */
int lk_nearest(lk_knn_t knn, const float* queries, int64_t P, float max_dist, float* out_d2, int32_t* out_idx, void* stream);
/* lk_mesh_areas: out_area[f] = 0.5 sqrt((cx cx + cy cy) + cz cz), c = (v1 - v0) x (v2 - v0) with every difference, product and difference of
 * products rounded once; 0 for a face with an index outside [0, V) or a non-finite area.
 * lk_mesh_sample: sample s = 0 .. S of `seed`: (r0, r1, r2, r3) = Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 * (s, 0, 0, 0) (the rounds are written out at lk_ransac_hypotheses).  Face: the first f with cum_area[f] > ((r0 + 0.5) 2^-32)
 * cum_area[F - 1] in fp64, by bisection - cum_area[F] is the inclusive running sum of the areas in fp64, the caller's; it must end above 0;
 * a zero-area face is never chosen.  Point: u_k = fl(fl((float)r_k + 0.5) 2^-32), a = sqrt(u_1), b = u_2, barycentrics (w0, w1, w2) = (1 - a,
 * a (1 - b), a b), every operation rounded once; out_pos = fma(w0, v0, fma(w1, v1, w2 v2)) per coordinate.  out_face[S], out_bary[S,3]. */
int lk_mesh_areas(const float* verts, int64_t V, const int32_t* faces, int64_t F, float* out_area, void* stream);
int lk_mesh_sample(const float* verts, int64_t V, const int32_t* faces, int64_t F, const double* cum_area, uint64_t seed, int64_t S,
                   float* out_pos /*[S,3]*/, int32_t* out_face /*[S]*/, float* out_bary /*[S,3]*/, void* stream);
/* lk_mesh_cull: seen[i] = 1 if points[i] projects into the image of at least one of the n_poses cameras; bytes of unseen points are NOT written
 * (the caller zeroes them; a long trajectory goes through in chunks that OR into the same bytes).  w2c[n_poses][12]: DEVICE memory, row-major
 * 3 x 4 inverses of the project's camera-to-world matrices (x right, y up, looking down -z), inverted by the caller.  Per pose, with (x, y, z) =
 * w2c p by three fused multiply-adds per coordinate (lk_icp_accumulate) and the reference's signs: zz = z + 1e-5, u = (fx (-x) + cx z) / zz,
 * v = (fy y + cy z) / zz; seen iff 0 <= -zz and 0 < u < W and 0 < v < H. */
int lk_mesh_cull(const float* points, int64_t N, const float* w2c, int32_t n_poses, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                 uint8_t* seen, void* stream);
/* Depth image of a triangle mesh: depth[i][j] = the smallest z in [near, far] at which the line through the camera centre with direction
 * ((j - cx) / fx, (i - cy) / fy, 1) (camera axes x right, y down, z forward) meets a triangle, either face; 0 where it meets none.
 * host_w2c12: HOST pointer, row-major 3 x 4 world -> that camera.  Per triangle with camera-space corners a, b, c the pixel is inside iff its
 * direction d has d . (b x c), d . (c x a), d . (a x b) all >= 0 or all <= 0 - p x q evaluated as (p - q) x q with the corners of the edge in
 * ascending vertex order and negated for the reverse edge, so that two triangles sharing an edge agree on it bit for bit - and then
 * z = (n . a) / (n . d), n = (b - a) x (c - a).  Nothing is projected for the test, so a triangle crossing the camera plane needs no clipping.
 * lk_mesh_depth_setup fills depth with the empty pattern, writes the records out_rec[F][16] and, per triangle, the box of 8 x 8-pixel tiles
 * out_box[F][4] = (first tile column, first tile row, columns, rows) that holds its projection cut at z = near, and out_ntiles[F] = columns x
 * rows (0 for a triangle wholly nearer than near, beyond far, outside the image, or with a bad index).  The caller forms tile_end[F] = the
 * inclusive running sum of out_ntiles (T = its last entry, < 2^31).  lk_mesh_depth_raster gives every tile of that work list one 64-lane
 * wave - a triangle over the whole image is T waves, not one lane's loop - which takes an unsigned 32-bit atomic minimum on the bit pattern of
 * the (positive) depth per covered pixel, and then turns the empty pattern into 0. */
int lk_mesh_depth_setup(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* host_w2c12, int32_t H, int32_t W, float fx,
                        float fy, float cx, float cy, float near, float far, float* out_rec, int32_t* out_box, int32_t* out_ntiles,
                        float* out_depth /*[H,W]*/, void* stream);
int lk_mesh_depth_raster(const float* rec, const int32_t* box, const int32_t* tile_end, int64_t F, int64_t T, int32_t H, int32_t W, float fx,
                         float fy, float cx, float cy, float near, float far, float* depth /*[H,W]*/, void* stream);

/* ---------------------------------------------------------------- rendering evaluation
 * The image figures the reference reports for every re-rendered frame (src/Mapper.py:1120-1160): depth L1 and PSNR over the pixels with a
 * sensor depth, and MS-SSIM as pytorch_msssim.ms_ssim(X, Y, data_range=1.0, size_average=True) forms it.  The device produces sums and means;
 * the caller combines them (loopy_slam_amd/render_eval.py).  No floating-point atomic: per-workgroup partials and a fixed-order reduction, so
 * two calls on equal inputs give equal bits.  ws: lk_img_eval_ws_bytes(H, W) bytes, 8-byte aligned; its contents on entry do not matter.
 *
 * out_rec[LK_IMG_REC] (fp64, device):
 *   [0]  n_valid: the number of pixels with gt_depth > 0 (exact)
 *   [1]  sum over those pixels of |fl32(gt_depth - depth)|
 *   [2]  sum over those pixels and the three channels of fl32(gt_color - color)^2
 *        (the difference is one fp32 subtraction; widened to fp64 it is made absolute or squared - exact - and added in fp64)
 *   [3 + 6 l + c], [3 + 6 l + 3 + c]   level l = 0 .. 4, channel c = 0 .. 2: the mean of the SSIM map and of the contrast-structure map
 *        (with_msssim = 0: neither computed nor written)
 * Level l + 1 is the 2 x 2 average of level l with stride 2 and one line of zeros in FRONT of every odd-sized dimension, divisor always 4
 * (avg_pool2d(kernel_size=2, padding=size % 2)): size s becomes (s + 1) / 2.  Per level and channel, with G the 11-tap window
 * g[k] = exp(-(k - 5)^2 / (2 1.5^2)) / sum (formed in fp64, rounded to fp32) applied down the columns and then along the rows without
 * padding (an h x w level has (h - 10) x (w - 10) maps), C1 = 0.01^2, C2 = 0.03^2:
 *   mu1 = G(X), mu2 = G(Y), s1 = G(X X) - mu1^2, s2 = G(Y Y) - mu2^2, s12 = G(X Y) - mu1 mu2,
 *   cs = (2 s12 + C2) / (s1 + s2 + C2), ssim = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) cs
 * in fp32 with every operation rounded once and each window sum taken in tap order; the map sums are fp64.  MS-SSIM is defined for
 * min(H, W) > 160 only (the package's assertion): with_msssim != 0 on a smaller image is an error.  3 H W < 2^31. */
#define LK_IMG_REC 33
int lk_img_eval_ws_bytes(int32_t H, int32_t W, int64_t* out_bytes);
int lk_img_eval(const float* gt_color, const float* color /*[H][W][3], values in [0, 1]*/, const float* gt_depth, const float* depth /*[H][W]*/,
                int32_t H, int32_t W, int32_t with_msssim, void* ws, double* out_rec /*device, [LK_IMG_REC]*/, void* stream);

/* ---------------------------------------------------------------- place recognition
 * Which earlier segment does the newest keyframe look at?  The reference answers with OpenCV's ORB and a DBoW3 vocabulary tree
 * (src/neural_point.py:126-142, 619-644, 1076-1107); neither can be assumed, so the contract below is this library's own: an ORB-like binary
 * descriptor and a direct descriptor-matching score.  INTEGER ARITHMETIC FROM THE GREY IMAGE ONWARD: the kernels, the host emulator and the
 * referee (tests/place_referee.py) agree bit for bit.  No floating-point atomic; equal inputs give equal bits.
 *
 * Grey image.  color[H][W][3] fp32.  Per channel q = clamp((int)fmaf(c, 255.0f, 0.5f), 0, 255) - one fused multiply-add, truncated; a NaN gives 0 -
 * and grey = (1868 q_0 + 9617 q_1 + 4899 q_2 + 8192) >> 14.  Channel 0 takes the BLUE weight: the reference hands its RGB image to
 * cv2.COLOR_BGR2GRAY, and that is kept.
 * Pyramid.  n_levels levels (<= LK_PLACE_MAX_LEVELS), ratio 6/5: a level of n pixels along a side is followed by one of floor(5 n / 6).  Output
 * pixel i samples source coordinate (12 i + 1) / 10 per axis: t = 12 i + 1, i0 = min(t / 10, n - 1), i1 = min(i0 + 1, n - 1), f = t % 10, weights
 * (10 - f, f) in tenths; value = (sum over the four pixels of wy wx v + 50) / 100.  A level whose interior is empty after the
 * LK_PLACE_BORDER-pixel border has no keypoints and is no error.  Pixel i of level l sits at off[l] + i of every per-pixel array of the
 * workspace (levels one after another, rows of w[l] pixels).
 * Corners, per level, at the pixels with LK_PLACE_BORDER <= x < w - LK_PLACE_BORDER and the same in y.  FAST-9: with p the pixel and the
 * 16-pixel circle of radius 3 - (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3) as
 * (dx, dy) - a corner has 9 consecutive circle pixels (cyclically) all > p + 20 or all < p - 20.  Score: with the 3 x 3 Sobel derivatives
 * Ix = (v(x+1,y-1) + 2 v(x+1,y) + v(x+1,y+1)) - (the same at x-1), Iy = (v(x-1,y+1) + 2 v(x,y+1) + v(x+1,y+1)) - (the same at y-1) and
 * a = sum Ix^2, b = sum Ix Iy, c = sum Iy^2 over the 7 x 7 block centred on the corner: R = 25 (a c - b^2) - (a + c)^2 in int64, Harris with
 * k = 0.04 exactly.  A corner is a KEY if none of its 8 neighbours is a corner that precedes it in the total order (R descending, flat pixel
 * index ascending).
 * Selection (host).  Level l keeps its first quota[l] keys in that order: d_0 = n_features (1 - f) / (1 - f^n_levels), f = 5/6, d_{l+1} = d_l f
 * in fp64; quota[l] = floor(d_l + 0.5) for l < n_levels - 1 and the last level gets max(n_features - the sum of the others, 0) (ORB's rule).
 * Unused quota is not redistributed.  Output order: level ascending, then rank.
 * Orientation.  m10 = sum dx v, m01 = sum dy v over the level's grey pixels with dx^2 + dy^2 <= 225; the bin is the k in [0, LK_PLACE_BINS)
 * that maximises m10 C[k] + m01 S[k] (int64), lowest k on a tie, with C[k], S[k] = rint(2^14 cos / sin(12 degrees k)) as int32 - cos_sin[2][30],
 * the caller's.  No atan2.
 * Descriptor.  S = the level's grey image under the separable binomial [1 6 15 20 15 6 1] along x and then y, edge-clamped, kept as the
 * undivided uint32 sum.  Bit i of 256 = S(p + a_i) < S(p + b_i), word i / 32, position i % 32; (a_i, b_i) = pattern[bin][i] = (ax, ay, bx, by) int8.
 * The base pattern (bin 0): coordinate c = 0 .. 3 of test i is (u0 % 7) + (u1 % 7) + (u2 % 7) + (u3 % 7) - 12 with (u0 .. u3) = Philox4x32-10, key
 * (LK_PLACE_SEED, 0), counter (i, c, 0, 0) (the rounds are written out at lk_ransac_hypotheses).  Bin k: (x', y') = (rint(c x - s y),
 * rint(s x + c y)) with c, s = cos, sin of 12 degrees k in fp64, rounded once on the host (loopy_slam_amd/place.py: pattern_tables).  All
 * coordinates stay within 17 pixels, the disc within 15: inside the border.
 *
 * lk_place_ws_bytes: out_layout[8] = workspace bytes, total pixels P = off[n_levels], and the byte offsets of grey (uint8 [P]), S (uint32 [P]),
 * the scores (int64 [P], INT64_MIN for a pixel that is no corner), the key list (int32 [P]: flat pixels of the keys, ascending), its length (int32)
 * and the key mask (uint8 [P]).  The workspace is 8-byte aligned; its contents on entry do not matter.  H W <= LK_PLACE_MAX_PIXELS.
 * lk_place_detect: everything up to the key list, and out_level_counts[n_levels] (device) = the keys of each level.  The caller reads those back
 * - the one synchronisation of an image -, orders each level's keys by their scores (a stable sort of the negated scores: the list is ascending
 * in the pixel index already) and passes the chosen flat pixels as sel[N] to
 * lk_place_describe: out_kp[N][4] = (x, y, level, bin) in the level's own pixel grid, out_desc[N][8].  A pixel outside a level's border region is
 * not a keypoint of this library: its descriptor is zero.
 *
 * lk_place_match_score: query[n_query][8] against the segments db[S][F][8] of which the first counts[s] rows are in use (n_query <= F), both
 * directions in one launch: rows[S][2][F][3] int32 = (best, second, index) - direction 0 for every query row over the segment's rows, direction 1
 * for every row of the segment over the query rows.  best = the smallest Hamming distance, index = the lowest row that has it, second = the
 * smallest distance among the OTHER rows; LK_PLACE_NO_MATCH (257) where there is none (and index -1).  Rows beyond a set's size are not
 * written.  out_count[s] = the query rows i with index j >= 0 whose row j of direction 1 has index i (mutual), best <= max_hamming and
 * 5 best <= 4 second.  The caller's score is out_count / min(n_query, counts[s]), 0 if either is empty. */
#define LK_PLACE_MAX_LEVELS 16
#define LK_PLACE_MAX_PIXELS 16777216
#define LK_PLACE_BORDER 20
#define LK_PLACE_FAST_T 20
#define LK_PLACE_BINS 30
#define LK_PLACE_SEED 0x4F524221u
#define LK_PLACE_NO_MATCH 257
int lk_place_ws_bytes(int32_t H, int32_t W, int32_t n_levels, int64_t* out_layout /*[8]*/);
int lk_place_detect(const float* color, int32_t H, int32_t W, int32_t n_levels, void* ws, int32_t* out_level_counts, void* stream);
int lk_place_describe(const void* ws, int32_t H, int32_t W, int32_t n_levels, const int32_t* sel, int32_t N, const int32_t* cos_sin,
                      const int8_t* pattern, int32_t* out_kp, uint32_t* out_desc, void* stream);
int lk_place_match_score(const uint32_t* query, int32_t n_query, const uint32_t* db, const int32_t* counts, int32_t S, int32_t F,
                         int32_t max_hamming, int32_t* rows, int32_t* out_count, void* stream);

/* ---------------------------------------------------------------- visual odometry
 * The tracker's starting pose from the previous and the current RGB-D frame: the reference's tracking.visual_odometer
 * (src/utils/visual_odometer.py, src/Tracker.py:92-97, 275-309), a multi-scale hybrid (intensity + depth) odometry after
 * o3d.t.pipelines.odometry.  Open3D cannot be assumed: the contract is the arithmetic below, restated in NumPy by tests/odometry_referee.py,
 * with two deliberate departures: bilinear instead of nearest-pixel lookups in the target frame, and a correct pose
 * composition on the host.  NaN is the one "invalid" value throughout.  No floating-point atomic; equal inputs give equal bits.  fp32
 * operations are rounded once each and taken in the order written.
 *
 * Pyramid of one frame (lk_odom_prepare), n_levels <= LK_ODOM_MAX_LEVELS levels, level l + 1 of size (h_l / 2) x (w_l / 2) (integer division)
 * with all four intrinsics halved; the coarsest level must be 8 x 8 at least.  Level l holds LK_ODOM_PLANES planes of h_l w_l floats one after
 * another from float offset off[l]: I, Vx, Vy, D, Ix, Iy, Dx, Dy.
 *   Level 0: I = (0.299 r + 0.587 g) + 0.114 b; D = d where 0 < d <= max_depth, else NaN.
 *   Level l + 1, pixel (y, x), centre (2y, 2x) of level l, K = [1 4 6 4 1] / 16:
 *     I = sum_r K[r] (sum_k K[k] I_l[clamp(2y + r - 2)][clamp(2x + k - 2)]), both sums from index 0 up (rows filtered first, border replicated);
 *     D = NaN where the centre c is NaN, else (sum K[r] K[k] v) / (sum K[r] K[k]) over the 5 x 5 neighbours v that are in bounds, not NaN and
 *     have |v - c| <= depth_diff, r outer, k inner.
 *   Per level: Vx = ((x - cx) / fx) D, Vy = ((y - cy) / fy) D (the vertex map is (Vx, Vy, D)); with the border replicated,
 *     dx = (((p[y-1][x+1] + 2 p[y][x+1]) + p[y+1][x+1]) - ((p[y-1][x-1] + 2 p[y][x-1]) + p[y+1][x-1])) / 8 and dy likewise with rows and
 *     columns exchanged, for p = I (Ix, Iy) and p = D (Dx, Dy); a depth derivative is NaN if any of its nine taps is.
 *
 * Estimate (lk_odom_estimate).  T (fp64 [16], row-major 4 x 4, device, in / out) maps source-camera points to target-camera points in the pinhole
 * convention (x right, y down, z forward).  iters[n_levels] (host) are the iteration counts from the coarsest level to the finest (>= 0 each,
 * LK_ODOM_MAX_ITERS in all); every iteration runs, there is no early exit and no host synchronisation.  One iteration at level l, with
 * (R | t) = T rounded to fp32 and the level's intrinsics, for every source pixel whose D is not NaN, p = (Vx, Vy, D):
 *   X = ((R00 px + R01 py) + R02 pz) + t0 and Y, Z alike; Z > 0;  uf = (fx X) / Z + cx, vf = (fy Y) / Z + cy;
 *   u0 = floor(uf + 1/1024), a = clamp(uf - u0, 0, 1), v0 and b alike; 0 <= u0 < w_l - 1, 0 <= v0 < h_l - 1;
 *   bil(M) = (1 - b) ((1 - a) M[v0][u0] + a M[v0][u0+1]) + b ((1 - a) M[v0+1][u0] + a M[v0+1][u0+1]) in the TARGET pyramid;
 *   r_D = bil(D) - Z, (hx, hy) = bil(Dx), bil(Dy): all four taps of the three not NaN, and |r_D| <= outlier_trunc;
 *   r_I = bil(I) - I_source, (gx, gy) = bil(Ix), bil(Iy);  iz = 1 / Z;
 *   c0 = (gx fx) iz, c1 = (gy fy) iz, c2 = -((c0 X + c1 Y) iz), J_I = (-Z c1 + Y c2, Z c0 - X c2, -Y c0 + X c1, c0, c1, c2);
 *   J_D = the same form from (hx, hy), plus (-Y, X, 0, 0, 0, -1);
 *   w = 1 if |r| <= delta else delta / |r| (delta = huber_intensity, huber_depth); loss = r^2 / 2 or delta (|r| - delta / 2).
 * Sums over the valid pixels, per lane in fp32, then lanes, half-waves and workgroups in a fixed order (workgroups in fp64):
 *   A = sum w_I J_I J_I^T + w_D J_D J_D^T (upper triangle, rows first: 21), b = sum w_I r_I J_I + w_D r_D J_D (6), the loss, the count.
 * Then A x = -b by Cholesky in fp64.  If the count is < 6 or a pivot is <= 0 (or NaN), T stays as it is and the record's flag is 1.  Otherwise
 * T <- [exp(x0..2) | x3..5] T in fp64, exp by Rodrigues' formula.
 * out_log (device, fp64 [sum iters][LK_ODOM_REC], or NULL), one record per iteration in the order run:
 *   [0] level, [1] iteration, [2] valid count, [3] loss, [4..24] A, [25..30] b, [31] |x| (0 if flagged), [32] flag.
 *
 * lk_odom_ws_bytes: out_layout[4 + 2 LK_ODOM_MAX_LEVELS] = bytes of one pyramid, bytes of the estimate's scratch ws (8-byte aligned, contents on
 * entry do not matter), LK_ODOM_PLANES, n_levels, then off[l] (in floats) and h_l w_l for l < LK_ODOM_MAX_LEVELS (0 beyond n_levels). */
#define LK_ODOM_MAX_LEVELS 6
#define LK_ODOM_MAX_PIXELS 16777216
#define LK_ODOM_MAX_ITERS 100000
#define LK_ODOM_PLANES 8
#define LK_ODOM_REC 33
int lk_odom_ws_bytes(int32_t H, int32_t W, int32_t n_levels, int64_t* out_layout /*[16]*/);
int lk_odom_prepare(const float* color /*[H][W][3]*/, const float* depth /*[H][W]*/, int32_t H, int32_t W, int32_t n_levels, float fx, float fy,
                    float cx, float cy, float max_depth, float depth_diff, float* pyr, void* stream);
int lk_odom_estimate(const float* pyr_src, const float* pyr_tgt, int32_t H, int32_t W, int32_t n_levels, float fx, float fy, float cx, float cy,
                     const int32_t* iters /*host, [n_levels], coarse to fine*/, float outlier_trunc, float huber_intensity, float huber_depth,
                     double* T /*device, [16]*/, double* out_log, void* ws, void* stream);

/* ---------------------------------------------------------------- frame preparation
 * A decoded frame -> what the trackers and mappers consume: colour float [Ho][Wo][3] in R, G, B and depth float [Ho][Wo] (the CPU passes of
 * the reference's reader behind cv2.imread, src/utils/datasets.py:95-119; tests/datasets_referee.py states the same in NumPy
 * float64).  The stages, in the reference's order, each skipped when it is the identity:
 *   undistort   colour only, when `distortion` (HOST, [5] = k1 k2 p1 p2 k3) is given and not all zero.  Destination pixel (u, v), in double:
 *               x = (u - cx) / fx, y = (v - cy) / fy, r2 = x x + y y, rad = ((1 + k1 r2) + k2 r2 r2) + k3 (r2 r2) r2,
 *               x' = (x rad + ((2 p1) x) y) + p2 (r2 + (2 x) x), y' = (y rad + p1 (r2 + (2 y) y)) + ((2 p2) x) y, source = (fx x' + cx, fy y' + cy),
 *               rounded to 1/32 pixel (rint of 32 s, half to even); the integer part picks the 2 x 2 taps, the two 5-bit fractions a, b the
 *               integer weights 32 (32 - b)(32 - a), 32 (32 - b) a, 32 b (32 - a), 32 b a (they sum to 2^15); taps outside the image are 0;
 *               result (sum w p + 2^14) >> 15 as uint8, into `undist` (device, [Hc][Wc][3], caller-owned: nothing is allocated here).
 *   to float    colour float(c) / 255.0f, depth float(d) / png_depth_scale (fp32 divisions, correctly rounded).
 *   resize      colour to the depth size when (Hc, Wc) != (Hd, Wd): source = (dst + 0.5) in / out - 0.5 clamped to [0, in - 1], bilinear.
 *   crop_size   when crop_h, crop_w > 0: colour bilinear with source = dst (in - 1) / (out - 1); depth nearest, source =
 *               min(floor(dst * fp32(in / out)), in - 1) (fp32 product).
 *   crop_edge   rows and columns [e, size - e) of that: Ho = Hb - 2 e, Wo = Wb - 2 e with (Hb, Wb) = crop_size, else (Hd, Wd).
 * Source cells and fractions of both float resamplings are formed in integers (quotient and remainder), the fraction by one fp32 division;
 * a bilinear value is (1 - fy) ((1 - fx) p00 + fx p01) + fy ((1 - fx) p10 + fx p11) in fp32; with both on, every crop tap composes its four
 * resize taps on the fly (no intermediate float image).  At most two launches (the undistortion, then everything else), on `stream` only,
 * no host synchronisation, no allocation.  LK_ERR_ARG: a NULL buffer (`undist` only when the undistortion runs), a size outside
 * 1 .. LK_FRAME_MAX_DIM, flag bits other than the two below, crop_h / crop_w negative, only one of them 0, or one of them 1 (align_corners
 * has no scale for it), crop_edge < 0 or 2 crop_edge >= Hb or Wb, png_depth_scale not finite and > 0, fx or fy == 0 with a distortion. */
#define LK_FRAME_BGR 1u         /* colour bytes are B, G, R (cv2.imread); default R, G, B (Pillow) */
#define LK_FRAME_DEPTH_F32 2u   /* depth is float [Hd][Wd]; default uint16 */
#define LK_FRAME_MAX_DIM 16384
int lk_frame_prepare(const uint8_t* color /*[Hc][Wc][3]*/, int32_t Hc, int32_t Wc, const void* depth /*[Hd][Wd]*/, int32_t Hd, int32_t Wd,
                     uint32_t flags, float png_depth_scale, double fx, double fy, double cx, double cy, const double* distortion /*host [5] or NULL*/,
                     int32_t crop_h, int32_t crop_w, int32_t crop_edge, uint8_t* undist /*[Hc][Wc][3] or NULL*/, float* out_color /*[Ho][Wo][3]*/,
                     float* out_depth /*[Ho][Wo]*/, void* stream);

/* ---------------------------------------------------------------- measurement
 * Per-kernel GPU time with HIP events recorded on the launch stream around the selected kernels
 * (names: comma-separated, e.g. "k_decode_bwd", or "*").  lk_profile_end synchronises those events and writes
 * "name calls total_ms" lines into buf.  Used by bench.py for the roofline figure.  A name stands for the instantiations rocprofv3 lists
 * under it, with one split: the decoder backward of launches WITH ray gradients (the tracker's: other instantiations, bf16 pieces in the
 * geometry role) is timed as "k_decode_bwd_track", the mapper's as "k_decode_bwd". */
int lk_profile_begin(const char* names);
/* lk_render_bwd runs the decoder weight-gradient reductions on a second, library-owned HIP stream beside the rel-pos backward and
 * the feature scatter (fork / join with events on the caller's stream: the caller sees one ordered stream).  on != 0 keeps
 * everything on the caller's stream - per-kernel durations are then those of a kernel running alone (measurement; the
 * environment variable LK_SERIAL sets the initial state). */
int lk_set_serial(int32_t on);
/* Creates the library's side streams now (they are otherwise created at their first use).  Call right after choosing the device and BEFORE
 * anything that creates many streams of its own (torch.distributed process groups, RCCL): the runtime multiplexes streams onto a few hardware
 * queues in creation order, and a side stream that shares the launch stream's queue serialises the backward's fork. */
int lk_streams_init(void);
int lk_profile_end(char* buf, int cap);
/* Measurement: resident 256-thread workgroups per compute unit of the five MLP kernels, as the runtime computes them from the
 * registers and LDS of the loaded code objects (hipOccupancyMaxActiveBlocksPerMultiprocessor): out[0..4] = k_decode_fwd,
 * k_decode_bwd (mapper form), k_relpos_fwd, k_relpos_bwd_fused, k_wgrad.  Needs a device. */
int lk_debug_occupancy(int32_t out[5]);
/* Test hook: every weight-gradient launch forked onto the library's side stream is preceded there by a kernel that spins for `us`
 * microseconds (0 = off, the default) - a missing ordering between the side stream and the launch stream then fails deterministically
 * instead of by timing (tests/test_split_step_order.py).  Results must not depend on it. */
int lk_debug_side_delay(int32_t us);
/* Test hook, the general form (lk_debug_side_delay(us) is site LK_DELAY_WGRAD): one delay site per stream of the library.  A site that is
 * on puts the same spinning kernel (one wave) of `us` microseconds at every place listed for it; us = 0 switches the site off.  The three
 * side-stream sites make that stream LATE (a missing join shows as a read before the write), LK_DELAY_LAUNCH makes the caller's stream
 * late behind every fork, so the library's streams run AHEAD of it (a buffer reused too early shows as a write before the last read).
 * us outside 0 .. LK_DELAY_MAX_US and unknown sites are refused with LK_ERR_ARG and change nothing.  In one-stream mode (lk_set_serial)
 * no site launches anything; with every site off the launches of every call are exactly those without the hook.  Results must not
 * depend on any site (tests/test_stream_order.py holds whole calls to equal bits). */
#define LK_DELAY_WGRAD  0  /* weight-gradient stream, in front of the forked k_wgrad of a backward */
#define LK_DELAY_SORT   1  /* weight-gradient stream, in front of the forked counting sort of a standalone lk_render_bwd */
#define LK_DELAY_AHEAD  2  /* look-ahead stream of lk_map_frame, in front of every chunk's search and once more between its search and its sorts */
#define LK_DELAY_LAUNCH 3  /* the caller's stream, right behind every fork: the weight-gradient fork and the sort fork of a backward, and every
                              look-ahead chunk that lk_map_frame enqueues */
#define LK_DELAY_SITES  4
#define LK_DELAY_MAX_US 2000
int lk_debug_stream_delay(int32_t site, int32_t us);
/* Test hook: the fp16 two-piece cut of the forward kernels (hi = rtz_f16(x), lo = rtz_f16(x - hi)) over n values (n even, device
 * pointers): hi / lo [n/2] = the packed pieces of the pairs (x[2i], x[2i+1]) in the production form, hi_ref / lo_ref [n/2] = the same
 * from the convert-and-subtract form it replaced (tests/test_split_forms.py: the two must agree bit for bit). */
int lk_debug_split_forms(const float* x, int32_t n, uint32_t* hi, uint32_t* lo, uint32_t* hi_ref, uint32_t* lo_ref, void* stream);
/* Test hook: the geometry trunk's saved relu bits (8 words per sample behind the act regions).  x [P][160] = five layers of 32 relu outputs per
 * sample (device pointers throughout).  The production packer runs over x in the decoder forward's lane-to-sample mapping with tiles of
 * `tile_stride` samples (32, or (32 / S) S as the tracker's fused forward) and leaves words [P][8]; the production reader then walks tiles of 32
 * as the decoder backward does: dec [P][160] = 1 where it lets the gradient through, else 0; ref [P][160] = (x > 0.0f) from a plain kernel
 * (tests/test_geo_act_bits.py: the two must be equal everywhere). */
int lk_debug_geo_bits(const float* x, int32_t P, int32_t tile_stride, uint32_t* words, uint8_t* dec, uint8_t* ref, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LOOPY_HIP_H */
