/* foundationpose_amd - C ABI of the MI355X (gfx950) render-and-compare hot path.
 *
 * The reference (SavaRobotics/FoundationPose) has no FFI for this path: its boundary is a set of
 * Python call signatures backed by third-party CUDA libraries.  Each entry point
 * below names the reference interface it replaces (file:line relative to the reference repo).
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative FP_E* code otherwise; fp_last_error() gives
 *     the message of the last failure on the calling thread.
 *   - `d_*` pointers are DEVICE pointers owned by the caller; `h_*` pointers are host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Nothing synchronises
 *     the stream except where stated; all launch functions are hipGraph-capturable.
 *   - poses are row-major 4x4 float32 (ob_in_cam, OpenCV camera), K is row-major 3x3 float64.
 *   - "net tensor" = fp16 NHWC with C padded to 8: [n][160][160][8] = (r,g,b,x,y,z,0,0), the
 *     fused, network-ready form of the reference's (N,6,160,160) fp32 A/B tensors.
 */
#ifndef FOUNDATIONPOSE_AMD_H
#define FOUNDATIONPOSE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the declarations of this header are its ONLY dynamic symbols. */
#pragma GCC visibility push(default)

#define FP_OK 0
#define FP_EINVAL (-1)   /* bad argument / shape */
#define FP_EHIP (-2)     /* HIP runtime error */
#define FP_ENOMEM (-3)
#define FP_EKEY (-4)     /* state_dict key missing / wrong shape */

typedef struct fp_ctx fp_ctx;    /* per-device context: workspace arena (replaces dr.RasterizeCudaContext, src/estimater.py:102,168) */
typedef struct fp_mesh fp_mesh;  /* device-resident mesh_tensors (src/Utils.py:104-130) */
typedef struct fp_net fp_net;    /* folded + packed network weights (load_state_dict, predict_pose_refine.py:138-141 / predict_score.py:151-154) */

const char *fp_last_error(void);
int fp_version(void);

/* ---- context ------------------------------------------------------------------------------- */
int fp_ctx_create(int device, fp_ctx **out);
int fp_ctx_destroy(fp_ctx *ctx);
/* Pre-size the activation arena for batches of up to `max_hyp` hypotheses so that no allocation
 * happens inside a timed / captured region. */
int fp_ctx_reserve(fp_ctx *ctx, int max_hyp);
/* Counts the (re)allocations of the arena.  A captured hipGraph of the launch functions holds arena addresses: it stays valid
 * while this number does not change (reserve enough before capturing). */
int fp_ctx_arena_generation(const fp_ctx *ctx);

/* ---- mesh: make_mesh_tensors (src/Utils.py:104-130); host pointers, copied to the device ---- */
int fp_mesh_create(fp_ctx *ctx, const float *h_pos, int V, const int32_t *h_faces, int F, const float *h_vnormals,
                   const float *h_vertex_color /* V*3 in [0,1] or NULL */,
                   const float *h_uv /* n_uv*2, v already flipped, or NULL */, int n_uv, const int32_t *h_uv_idx /* F*3 */,
                   const float *h_tex /* texH*texW*3 in [0,1] */, int texH, int texW, fp_mesh **out);
int fp_mesh_destroy(fp_mesh *mesh);

/* ---- a9: compute_crop_window_tf_batch(method='box_3d') (src/Utils.py:577-621) + bbox2d_ori
 *      (predict_pose_refine.py:44-45).  d_tf: N*9, d_bbox2d: N*4 (umin,vmin,umax,vmax). -------- */
int fp_crop_window_tf(fp_ctx *ctx, const float *d_poses, int N, const double *K, double crop_ratio, double mesh_diameter,
                      int out_w, int out_h, float *d_tf, float *d_bbox2d, void *stream);

/* ---- a11: nvdiffrast_render (src/Utils.py:133-219): fp32 channels-last maps, rows top-down,
 *      background 0.  Any output pointer may be NULL.  d_bbox2d may be NULL (full frame). ------- */
int fp_render(fp_ctx *ctx, const fp_mesh *mesh, const float *d_poses, int N, const double *K, int H, int W,
              const float *d_bbox2d, int out_h, int out_w, int use_light, float w_ambient, float w_diffuse,
              float *d_color /* N*h*w*3 */, float *d_depth /* N*h*w */, float *d_normal /* N*h*w*3 */,
              float *d_xyz /* N*h*w*3 */, void *stream);

/* The same with the non-default arguments of nvdiffrast_render: light_dir / light_pos / light_color (src/Utils.py:200-211)
 * and projection_mat (src/Utils.py:159-161).  opts == NULL is fp_render with use_light = 0. */
typedef struct fp_render_opts {
  size_t struct_size;      /* = sizeof(fp_render_opts) of the header the CALLER was built against: fields beyond it are read as 0 / NULL,
                            * a size the library does not know is refused (FP_EINVAL) */
  int use_light;
  float w_ambient, w_diffuse;
  int light_mode;          /* 0: light_dir = (0,0,1) (the default); 1: light_vec = -light_dir; 2: light_vec = light_pos (light_dir=None) */
  float light_vec[3];
  int has_light_color;     /* 0: light_color=None (the diffuse term takes the surface colour) */
  float light_color[3];
  int has_projection;      /* 1: projection (row-major 4x4, the reference's projection_mat) replaces the matrix derived from K */
  double projection[16];
  float *d_rast;           /* optional device output N*h*w*4: dr.rasterize's (u, v, z/w, triangle_id + 1) per pixel (src/Utils.py:182), rows flipped like
                            * the other outputs; NULL: not written.  What the parity tests compare coverage and the winning face on. */
} fp_render_opts;
int fp_render_ex(fp_ctx *ctx, const fp_mesh *mesh, const float *d_poses, int N, const double *K, int H, int W,
                 const float *d_bbox2d, int out_h, int out_w, const fp_render_opts *opts,
                 float *d_color, float *d_depth, float *d_normal, float *d_xyz, void *stream);

/* ---- a10/a13/a18 side A fused: render + rgb scaling + xyz centring / normalising / invalidating
 *      (h5_dataset.py:92-99 | :151-156) straight into a net tensor.  invalid_thres = 0.001
 *      (refiner) or 0.1 (scorer). ------------------------------------------------------------- */
int fp_render_net(fp_ctx *ctx, const fp_mesh *mesh, const float *d_poses, int N, const double *K, int H, int W,
                  const float *d_bbox2d, int out_h, int out_w, double mesh_diameter, int normalize_xyz, float invalid_thres,
                  void *d_net_out /* fp16 N*h*w*8 */, void *stream);

/* ---- a12/a13/a14 side B fused: kornia.warp_perspective crops of the observed frame + the batch
 *      transform.  mode 0 = refiner (rgb bilinear + xyz_map nearest, predict_pose_refine.py:63,72;
 *      h5_dataset.py:101-112); mode 1 = scorer (rgb bilinear + depth nearest + the full-resolution
 *      depth->xyz round trip of h5_dataset.py:158-161, composed per pixel, never materialised).
 *      d_rgb: H*W*3 float [0,255]; d_geom: H*W*3 xyz_map (mode 0) or H*W depth (mode 1).
 *      out_fmt 0: fp32 planar N*6*h*w (the reference's cat([rgbB, xyz_mapB],1)); 1: fp16 net tensor. */
int fp_crop_observed(fp_ctx *ctx, const float *d_rgb, const float *d_geom, int H, int W, const double *K,
                     const float *d_tf, const float *d_poses, int N, int out_h, int out_w, int mode,
                     double mesh_diameter, int normalize_xyz, int out_fmt, void *d_out, void *stream);

/* ---- a12, the use_normal branch: kornia.warp_perspective(mode='nearest', align_corners=False, zeros padding) of a
 *      channel-last float image batch by the axis-aligned crop transforms (predict_pose_refine.py:74-76: normalAs from
 *      the rendered normals, normalBs from the frame's normal map).  d_src: src_batch x src_h x src_w x channels with
 *      src_batch == N, or 1 = one image for every transform (the reference's .expand(B,-1,-1,-1)); d_tf: N x 3x3;
 *      d_out: N x channels x out_h x out_w (planar, as the reference's BatchPoseData holds it). */
int fp_warp_nearest(fp_ctx *ctx, const float *d_src, int src_batch, int src_h, int src_w, int channels, const float *d_tf, int N,
                    int out_h, int out_w, float *d_out, void *stream);

/* ---- a6/a7/a8: depth pre-processing (src/Utils.py:304-438) ----------------------------------- */
int fp_erode_depth(fp_ctx *ctx, const float *d_depth, int H, int W, int radius, float depth_diff_thres, float ratio_thres,
                   float zfar, float *d_out, void *stream);
int fp_bilateral_filter_depth(fp_ctx *ctx, const float *d_depth, int H, int W, int radius, float zfar, float sigmaD,
                              float sigmaR, float *d_out, void *stream);
int fp_depth2xyzmap(fp_ctx *ctx, const float *d_depth, int H, int W, const double *K, float zfar, float *d_xyz, void *stream);
/* The depth prelude of a tracking frame (src/estimater.py:256-260: erode_depth -> bilateral_filter_depth -> depth2xyzmap_batch) in
   one launch; `radius` must be 2 (both filters, as the reference calls them).  d_depth_out (H,W) and d_xyz (H,W,3) are bit-identical
   to the three calls above chained; d_depth_out must not alias d_depth.  Optionally the frame's colours ride along: d_rgb_u8 (H,W,3)
   uint8 -> d_rgb_f32 (H,W,3) float (what fp_crop_observed and the fused passes read); both null: not done. */
int fp_depth_prefilter(fp_ctx *ctx, const float *d_depth, int H, int W, int radius, float depth_diff_thres, float ratio_thres,
                       float zfar_erode, float zfar_bilateral, float sigmaD, float sigmaR, const double *K, float zfar_xyz,
                       float *d_depth_out, float *d_xyz, const uint8_t *d_rgb_u8, float *d_rgb_f32, void *stream);
/* depth2xyzmap of the registration path (src/Utils.py:399-417): float64 arithmetic, one rounding to float32, depth < 0.001 -> 0. */
int fp_depth2xyzmap_f64(fp_ctx *ctx, const float *d_depth, int H, int W, const double *K, float *d_xyz, void *stream);
/* The reductions behind FoundationPose.guess_translation and the "valid too small" test of register()
 * (src/estimater.py:137-156,173-177) without a host copy of the depth image.  d_mask: H*W bytes, non-zero = object.
 * h_stats6 (host): cmin, cmax, rmin, rmax of mask > 0 (cmax = -1 if the mask is empty), count of mask > 0, count of usable
 * pixels (mask > 0 and depth >= min_depth); h_median (host): np.median of the usable depths (0 if none).  Synchronises. */
int fp_mask_depth_stats(fp_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int H, int W, float min_depth, int32_t *h_stats6,
                        float *h_median, void *stream);

/* ---- evaluation against ground truth ----------------------------------------------------------- */
#define FP_ERR_ADD 1
#define FP_ERR_ADDS 2
#define FP_ERR_ADD_SYM 4
/* Pose errors of n_poses poses against ground truth: add_err / adds_err (src/Utils.py:232-253), in one launch plus a small one that
 * adds the partial sums.  d_pts (n_pts,3) model points; d_pred (n_poses,4,4); d_gt (4,4) shared by every pose (gt_per_pose = 0) or
 * (n_poses,4,4) (gt_per_pose = 1); d_sym (n_sym,4,4) symmetry transforms in the frame of d_pts.  Only rows 0..2 of a matrix are read.
 * `which` ORs FP_ERR_*; each requested output (n_poses float32, device) receives, with p the model points and T p = R p + t:
 *   FP_ERR_ADD      d_add[b]     = mean_i |pred_b p_i - gt_b p_i|
 *   FP_ERR_ADDS     d_adds[b]    = mean_i min_j |gt_b p_i - pred_b p_j|     (each ground-truth point queries the predicted points)
 *   FP_ERR_ADD_SYM  d_add_sym[b] = min_k mean_i |pred_b p_i - gt_b S_k p_i|  (= ADD for the single transform S_0 = I)
 * ADD-S is exact brute force over all n_pts x n_pts pairs.  A pose's results are bit-identical whatever the batch it is in and its
 * index there (no float atomics).  Workspace comes from the context's arena; nothing synchronises.  FP_EINVAL: n_pts or n_poses < 1,
 * a null input, a requested output that is null, FP_ERR_ADD_SYM with n_sym < 1 or d_sym null, gt_per_pose not 0 / 1, unknown bits
 * in `which`.  which = 0 launches nothing. */
int fp_pose_errors(fp_ctx *ctx, const float *d_pts, int n_pts, const float *d_pred, const float *d_gt, int gt_per_pose, int n_poses,
                   const float *d_sym, int n_sym, int which, float *d_add, float *d_adds, float *d_add_sym, void *stream);

#define FP_BOP_MSSD 1
#define FP_BOP_MSPD 2
/* BOP pose errors of n_poses poses against ground truth: bop_toolkit pose_error.mssd and pose_error.mspd (BOP 2019 evaluation), in one
 * launch plus a small one that reduces the tile maxima.  d_pts, d_pred, d_gt, gt_per_pose, d_sym as for fp_pose_errors; d_sym may be
 * null with n_sym = 0 (the identity only).  K: host float64 3x3 intrinsics, required for FP_BOP_MSPD.  `which` ORs FP_BOP_*; each
 * requested output (n_poses float32, device) receives
 *   FP_BOP_MSSD  d_mssd[b] = min_k max_i |(pred_b - gt_b S_k) p_i|                     metres
 *   FP_BOP_MSPD  d_mspd[b] = min_k max_i |pi(pred_b p_i) - pi(gt_b S_k p_i)|           pixels, pi(x) = (fx x/z + cx, fy y/z + cy)
 * pred_b - gt_b S_k and gt_b S_k are formed in double and rounded once, so pred = gt gives exactly 0.  A point at z <= 0 under either
 * transform makes that k's MSPD maximum +inf.  A pose's results are bit-identical whatever the batch it is in.  Workspace comes from
 * the context's arena; nothing synchronises.  FP_EINVAL: a null ctx, d_pts, d_pred or d_gt, n_pts < 1, n_poses < 0, n_sym < 0,
 * n_sym > 0 with d_sym null, gt_per_pose not 0 / 1, unknown bits in `which`, a requested output that is null, FP_BOP_MSPD with K
 * null.  n_poses = 0 or which = 0 launches nothing. */
int fp_pose_errors_bop(fp_ctx *ctx, const float *d_pts, int n_pts, const float *d_pred, const float *d_gt, int gt_per_pose, int n_poses,
                       const float *d_sym, int n_sym, const double *K, int which, float *d_mssd, float *d_mspd, void *stream);

#define FP_VSD_MAX_TAUS 32
/* Visible surface discrepancy of n_poses poses: bop_toolkit pose_error.vsd with visib_mode = 'bop19' and the distances normalised by
 * the diameter.  d_depth_test: metres, 0 = missing, (H,W) shared by every pose (depth_per_pose = 0) or (n_poses,H,W) (= 1).  d_pred
 * (n_poses,4,4); d_gt (4,4) (gt_per_pose = 0, rendered once) or (n_poses,4,4) (= 1).  K: host float64 3x3.  The depth of every pose is
 * rendered full frame by this library's rasteriser (fp_render), into workspace from the context's arena, in chunks of poses.  Per pixel,
 * with u, v the integer pixel indices:
 *   dist(d) = sqrt(X*X + Y*Y + d*d),  X = ((u - cx) * d) * (1/fx),  Y = ((v - cy) * d) * (1/fy)      float64, not contracted
 *   Dt = dist(depth_test), Dg = dist(render(gt)), De = dist(render(pred))
 *   vis(Dm) = Dm > 0 && ((double)((float)Dm - (float)Dt) <= delta || Dt == 0)
 *   visib_gt = vis(Dg),  visib_est = vis(De) || (visib_gt && De > 0)
 *   cost_t = #{inter : |Dg - De| / diameter >= h_taus[t]},  e_t = (cost_t + |union| - |inter|) / |union|  (1 when |union| = 0)
 * d_err (n_poses, n_taus) float32 receives e; d_counts, if not null, (n_poses, 2 + n_taus) int32: |union|, |inter|, cost_0 ..
 * Nothing synchronises.  FP_EINVAL: a null ctx, mesh, d_depth_test, K, d_pred, d_gt, h_taus or d_err, n_taus outside
 * 1..FP_VSD_MAX_TAUS, H or W < 1, H * W > 2^30, diameter <= 0 (or NaN), depth_per_pose or gt_per_pose not 0 / 1, n_poses < 0.
 * n_poses = 0 launches nothing.  A frame the rasteriser cannot take (W above 6553, for one) is refused with FP_EINVAL as well. */
int fp_vsd(fp_ctx *ctx, const fp_mesh *mesh, const float *d_depth_test, int depth_per_pose, int H, int W, const double *K, const float *d_pred,
           const float *d_gt, int gt_per_pose, int n_poses, double diameter, double delta, const double *h_taus, int n_taus, float *d_err,
           int32_t *d_counts, void *stream);

#define FP_SCENE_MAX_INSTANCES 1024
#define FP_SCENE_OCC_DEPTH 1      /* the observed depth image occludes */
#define FP_SCENE_OCC_INSTANCES 2  /* the instances occlude one another (z-buffer over all of them) */
#define FP_SCENE_INFO_COLS 12     /* int32 columns of a d_info row: */
#define FP_SCENE_INFO_PX_COUNT_ALL 0
#define FP_SCENE_INFO_PX_COUNT_VALID 1
#define FP_SCENE_INFO_PX_COUNT_VISIB 2
#define FP_SCENE_INFO_PX_COUNT_IN_FRAME 3
#define FP_SCENE_INFO_BBOX_OBJ 4   /* x0, y0, x1, y1 */
#define FP_SCENE_INFO_BBOX_VISIB 8 /* x0, y0, x1, y1 */
/* From the poses of the n_inst object instances of a frame to which pixels each covers, which of them are visible and how much of the
 * object that is: what bop_toolkit's calc_gt_masks.py, calc_gt_info.py and visibility.estimate_visib_mask_gt compute on the CPU with an
 * OpenGL renderer, and a z-buffer composite of the instances.  meshes: host array of n_inst handles (repeats allowed); d_poses
 * (n_inst,4,4) device; K host float64 3x3.
 *   Canvas.  Every instance is rendered alone, depth only, by this library's rasteriser (fp_render) on a canvas of
 * (H + 2 pad_y) x (W + 2 pad_x) with K' = K except cx' = cx + pad_x, cy' = cy + pad_y (in double).  Image pixel (u, v) is canvas pixel
 * (u + pad_x, v + pad_y).  pad = 0 is the plain frame; calc_gt_info uses pad_x = W, pad_y = H, so that the part of an object outside the
 * frame counts in px_count_all.  Every output comes from this ONE render per instance (bop_toolkit renders twice, padded and not).
 *   Distance.  dist(d) at canvas pixel (u', v') as under fp_vsd with K' and the canvas indices, float64, not contracted.  Dm_i = dist of
 * instance i's render; Dt = dist(d_depth_test) inside the frame with FP_SCENE_OCC_DEPTH, else 0.
 *   Occluder.  FP_SCENE_OCC_DEPTH alone: Docc = Dt.  With FP_SCENE_OCC_INSTANCES: Dmin = the smallest positive Dm_i at the pixel (0 if
 * none) and Docc = Dmin, or with both bits the smaller positive one of Dt and Dmin (0 if neither is positive).
 *   Masks.  mask_i = Dm_i > 0.  mask_visib_i = Dm_i > 0 && ((double)((float)Dm_i - (float)Docc) <= delta || Docc == 0) inside the frame
 * (BOP's 'bop19' rule, the expression of fp_vsd) and false outside it: what lies outside the image is not visible in it, so
 * px_count_visib == count(mask_visib) always and visib_fract = px_count_visib / px_count_all is BOP's.  d_mask / d_mask_visib
 * (n_inst,H,W) uint8 receive 0 / 255 for the in-frame part.
 *   Composite.  d_owner (H,W) int32: the instance with the smallest positive render DEPTH at the pixel, the smallest index among equal
 * depths, -1 where none renders; d_depth (H,W): that depth in metres, 0 where none.  Neither looks at d_depth_test or `occluders`.
 *   Info.  d_info (n_inst, FP_SCENE_INFO_COLS) int32, columns FP_SCENE_INFO_*: px_count_all = |mask| over the whole canvas;
 * px_count_valid = mask pixels inside the frame with d_depth_test > 0 (0 when d_depth_test is null); px_count_visib = |mask_visib|;
 * px_count_in_frame; bbox_obj = x0, y0, x1, y1 inclusive, in IMAGE coordinates, of the mask over the whole canvas (negative or beyond
 * W-1 / H-1 with padding); bbox_visib the same of mask_visib.  An empty set has count 0 and a box of four -1: test the count, -1 is a
 * legal coordinate with padding.
 *   The instances are rendered in chunks whose depth layers fit 512 MB of the context's arena; the results do not depend on the
 * chunking.  With FP_SCENE_OCC_INSTANCES and more than one chunk a first pass over the chunks forms the running minimum and a second
 * one the masks: every instance is then rendered twice.  Without FP_SCENE_OCC_INSTANCES an instance's masks and info row are
 * bit-identical whatever else is in the call.  Counts and boxes are accumulated with integer atomics (add, min, max): deterministic.
 * Nothing synchronises; every output pointer may be null independently; n_inst = 0 launches nothing but clears d_owner (-1) and d_depth
 * (0) when given.  FP_EINVAL: a null ctx or K, null meshes (or one of its entries) or d_poses with n_inst > 0, n_inst outside
 * 0..FP_SCENE_MAX_INSTANCES, H or W < 1, a negative pad, `occluders` 0 or with unknown bits, FP_SCENE_OCC_DEPTH with d_depth_test null,
 * delta < 0 or NaN, a canvas the rasteriser refuses (wider than 6553 pixels, or more rows than 255 of its strips hold - a strip holds
 * about 15 000 pixels, so about 3.8 M canvas pixels: pad_x = W, pad_y = H fits frames up to 640 x 480; the message says to reduce the
 * pad when there is one), checked before anything is queued.  FP_ENOMEM: the arena cannot hold the call's workspace. */
int fp_scene_instances(fp_ctx *ctx, const fp_mesh *const *meshes, const float *d_poses, int n_inst, const double *K, int H, int W, int pad_x,
                       int pad_y, const float *d_depth_test, int occluders, double delta, uint8_t *d_mask, uint8_t *d_mask_visib,
                       int32_t *d_owner, float *d_depth, int32_t *d_info, void *stream);

#define FP_MESH_DIAMETER_MAX_POINTS (1 << 21)
/* Exact diameter of a point set: max over i < j of |p_i - p_j| over ALL pairs, in place of the reference's maximum over a random
 * sample of the points (compute_mesh_diameter, src/Utils.py:559-574, `np.random.choice`), whose value changes with numpy's seed once
 * a model has more points than the sample.  d_pts (n_pts,3) float32, device, finite.  d_out_diameter: 1 float32, device.  d_out_pair:
 * 2 int32, device, or null: the pair (i, j), i < j, that spans the diameter.  Upper-triangle pairs of 1024-point tiles, one workgroup
 * each; the squared distance is dx*dx + dy*dy + dz*dz in fp32 in that order and the square root is taken once, of the maximum.  The
 * result is deterministic and independent of the execution order: among pairs whose fp32 squared distances tie, the smallest (i, j) in
 * lexicographic order is returned.  No atomics; per-workgroup candidates go to the context's arena and a second launch folds them.
 * Nothing synchronises.  n_pts < 2 gives diameter 0 and pair (0, 0).  FP_EINVAL: a null ctx or d_out_diameter, d_pts null with
 * n_pts > 0, n_pts < 0 or above FP_MESH_DIAMETER_MAX_POINTS (2^21: 2.1 M tile pairs, 34 MB of arena). */
int fp_mesh_diameter(fp_ctx *ctx, const float *d_pts, int n_pts, float *d_out_diameter, int32_t *d_out_pair, void *stream);

#define FP_BOX_EXTENTS_MAX_POINTS (1 << 21)
#define FP_BOX_EXTENTS_MAX_FRAMES (1 << 24)
#define FP_BOX_EXTENTS_MAX_EVALS (1ll << 40)
#define FP_BOX_EXTENTS_TILE 1024          /* points of an LDS tile */
#define FP_BOX_EXTENTS_CAND 1024          /* candidates of a workgroup */
/* The boxes of n points in C candidate frames and the smallest of them: the search of a minimum-volume oriented box
 * (Utils.oriented_bounds), and the box of any cloud in given frames (Utils.box_extents).  d_points (n,3) float32; d_frames (C,3,3)
 * float32 row-major, the rows r_0, r_1, r_2 of a frame being its axes - normalised by the caller: the device takes no root and divides
 * nothing.  The rule per candidate c is the project's own, restated op for op by tests/oriented_bounds_oracle.py:
 *     q_k  = ((r_k0 * x) + (r_k1 * y)) + (r_k2 * z)             fp32, in that order, nothing contracted
 *     lo_k = min, hi_k = max of q_k over all points             fminf / fmaxf from +inf / -inf: a NaN projection is passed over
 *     vol  = ((hi_0 - lo_0) * (hi_1 - lo_1)) * (hi_2 - lo_2)    fp32
 * The winner is chosen by a total order: among the candidates with vol >= 0 (a NaN volume never wins, nor the negative one of a
 * candidate that saw no finite projection) the smaller volume first, then the lower index.  min and max do not depend on the order of
 * their operands, so every output is the same bits whatever the tiling, the launch shape, the batch a candidate sits in or the run.
 *   Outputs, device: d_best_index 1 int32 (-1 when no candidate is eligible; the three others are then NaN), d_best_lohi 6 float32
 * lo[3], hi[3], d_best_volume 1 float32.  Optional, null to skip: d_all_lohi (C,6) and d_all_volume (C).
 *   grid = (blocks of FP_BOX_EXTENTS_CAND candidates, slices of the points), a lane holding four frames and their bounds in registers
 * and a tile of FP_BOX_EXTENTS_TILE points in LDS; a second launch folds the slices and forms the volumes, a third folds the
 * per-workgroup winners.  No atomics, no arrival counters; the per-slice bounds go to the context's arena (24 bytes per candidate and
 * slice; more than one slice only below 2^20 candidates).  Nothing synchronises and nothing is allocated once the arena holds the call:
 * it sits in a captured graph.  FP_EINVAL, before anything is queued: a null ctx, d_points, d_frames, d_best_index, d_best_lohi or
 * d_best_volume; n < 1 or above FP_BOX_EXTENTS_MAX_POINTS; C < 1 or above FP_BOX_EXTENTS_MAX_FRAMES; n C above
 * FP_BOX_EXTENTS_MAX_EVALS (2^40 projections of a point on a frame, seconds of work: cut the candidates into several calls). */
int fp_box_extents(fp_ctx *ctx, const float *d_points, int n, const float *d_frames, int C, int32_t *d_best_index, float *d_best_lohi,
                   float *d_best_volume, float *d_all_lohi, float *d_all_volume, void *stream);

#define FP_MESH_SIMPLIFY_MAX_VERTICES (1 << 21)
#define FP_MESH_SIMPLIFY_MAX_FACES (1 << 23)
/* Vertex clustering: a mesh (or, with F = 0, a point cloud) reduced to one vertex per occupied cell of a grid of pitch `cell`.  The
 * rasteriser keeps a hypothesis' vertices in LDS up to 8192 vertices and its one-launch forms take up to 65 535 faces; fused and scanned
 * meshes are far larger, and this is the stage that takes them there.  Deterministic: the outputs are a function of the inputs alone,
 * bit for bit, whatever order the device runs in (tests/mesh_simplify_oracle.py restates the rule in numpy).
 *   Inputs, device: d_pos (V,3) float32, finite; d_faces (F,3) int32 with entries in 0 .. V-1, F may be 0; optional d_normals (V,3) float32
 * (components within +-2^11) and d_colors (V,3) uint8; cell > 0.  All arithmetic is IEEE without contraction.
 *   1. Origin.  o = the component-wise minimum of the positions (an exact float32 minimum).
 *   2. Cell of a vertex.  Per axis c = (int64) floorf((p - o) / cell), subtraction and division in float32.  dims = max c + 1 per axis;
 *      FP_EINVAL when a dim exceeds 2^21 (the message names a cell that fits).  key = (cz * ny + cy) * nx + cx in int64.
 *   3. Clusters.  The vertices of one key form a cluster.  Clusters are numbered by their lowest member vertex index, ascending.
 *      Vertices that no face references cluster like the others.
 *   4. Cluster attributes, exact and hence independent of the order of the sums.  Position: q = llrint(((double)p - (double)o) * 2^30)
 *      per axis (round half to even), S = sum of q over the members in int64, n = members; the result is
 *      (float)((double)o + (double)S / (double)n / 2^30).  Normal: the int64 sums of llrint((double)nrm * 2^30) per axis, converted to
 *      double (sx, sy, sz), divided by sqrt((sx*sx + sy*sy) + sz*sz) in double, cast to float; a zero sum gives (0,0,0).  Colour:
 *      (2 * sum c + n) / (2 n) per channel in integers.  A cluster of ONE member keeps that member's position, normal and colour bits:
 *      a cell below the smallest vertex spacing returns the input vertices bit for bit.
 *   5. Faces.  Each face is mapped to cluster ids.  A face with two equal ids is dropped.  Among faces with the same unordered id
 *      triple, whatever their orientation, only the lowest input face index survives.  Survivors keep their input order and their own
 *      vertex order.
 *   6. Vertices kept.  With F > 0 the clusters that no surviving face references are dropped and the others renumbered in cluster order.
 *      With F = 0 every cluster is kept: the per-cell centroid cloud.
 *   7. Vertex map.  d_out_vertex_map (V,) int32, optional: the output vertex of every input vertex, or -1.
 *   Consequences: an input vertex whose cluster survives lies within sqrt(3) * cell of its output vertex (plus 1e-6 of the bounding
 * box' extent for the float32 cell assignment); no output face is degenerate or repeats a vertex triple; with F > 0 every output vertex
 * is referenced.
 *   Two calls, as for the TSDF extraction.  fp_mesh_simplify_count builds the cluster and face tables in an allocation owned by the
 * context (about 50 bytes a vertex and 40 a face, kept until a larger mesh arrives or the context is destroyed), SYNCHRONISES the stream
 * and returns h_counts = {vertices, faces}.  The caller allocates d_out_pos (nv,3), d_out_normals and d_out_colors (nv,3; each optional,
 * and only with its input), d_out_faces (nf,3), and calls fp_mesh_simplify_write with the SAME d_pos, V, d_faces, F and cell; it
 * queues its kernels and does not synchronise.  The sums are 64-bit integer atomic adds; there is no floating-point atomic.
 *   FP_EINVAL: a null ctx or h_counts, V or F outside their limits, null d_pos or d_faces with a non-zero count, a cell that is not
 * positive and finite, positions that are not finite, a face index outside 0 .. V-1, a dim above 2^21, a bounding box whose extent times
 * 2^30 times V reaches 2^62 (the fixed point would overflow: extents in metres are far below it); for write: no count before it on this
 * context, another mesh (pointers or sizes) or cell than the last count had, n_vertices or n_faces other than its counts, a null
 * required output, an output attribute without its input.  FP_ENOMEM: the tables do not fit the device. */
int fp_mesh_simplify_count(fp_ctx *ctx, const float *d_pos, int V, const int32_t *d_faces, int F, float cell, int64_t *h_counts, void *stream);
int fp_mesh_simplify_write(fp_ctx *ctx, const float *d_pos, const float *d_normals, const uint8_t *d_colors, int V, const int32_t *d_faces, int F,
                           float cell, float *d_out_pos, float *d_out_normals, uint8_t *d_out_colors, int32_t *d_out_faces,
                           int32_t *d_out_vertex_map, int64_t n_vertices, int64_t n_faces, void *stream);

#define FP_MESH_COMPONENTS_MAX_VERTICES (1 << 21)
#define FP_MESH_COMPONENTS_MAX_FACES (1 << 23)
/* Connected components of a triangle list, a selection among them and the mesh of the selected ones: the clean-up that drops the
 * floating pieces fused depth noise leaves, and the debris of scanned models.  Deterministic: the outputs are a function of the inputs
 * alone, bit for bit, whatever order the device runs in (tests/mesh_components_oracle.py restates the rule in numpy / scipy).
 *   Inputs, device: d_faces (F,3) int32 with entries in 0 .. V-1, F may be 0; for write d_pos (V,3) float32 and optional d_normals (V,3)
 * float32 and d_colors (V,3) uint8.  No arithmetic is done on the attributes.
 *   1. Graph.  Its nodes are the V vertices; every face (a, b, c) joins a-b and b-c.  Two sheets that share only a vertex are one
 *      component.  A face with repeated indices is legal: it joins what it names and counts as a face.  A vertex that no face names is a
 *      component of its own with 0 faces.
 *   2. Label.  label[v] = the lowest vertex index of v's component.
 *   3. Numbering.  Components are numbered 0 .. C-1 by that lowest index, ascending (the rule fp_mesh_simplify uses for clusters; it is
 *      the label order of scipy's connected_components for an undirected graph).
 *   4. Per component: n_vertices and n_faces, int32.  A face belongs to the component of its FIRST vertex.
 *   5. Selection.  min_faces >= 1, min_fraction in [0, 1], largest_only 0 / 1.  M = the largest n_faces.  Component c is a candidate iff
 *      n_faces[c] >= 1 and n_faces[c] >= min_faces and (double)n_faces[c] >= (double)min_fraction * (double)M (one IEEE multiplication in
 *      double, no contraction).  Without largest_only every candidate is kept.  With it exactly one is: the candidate with the most faces,
 *      the lowest component number among equals (none when the component of M faces is itself no candidate).  min_faces = 1,
 *      min_fraction = 0, largest_only = 1 is "the component with the most faces".
 *   6. Output.  Kept vertices are exactly the members of kept components, in their input order; every one of them is referenced (a kept
 *      component has a face).  Kept faces are the faces of kept components, in their input order and with their own vertex order,
 *      re-indexed.  Positions, normals and colours are copied bit for bit.
 *   7. d_out_vertex_map (V,) int32, optional: the output vertex of every input vertex, or -1.  d_out_label (V,) int32, optional: rule 2.
 *      d_out_stats (C,2) int32, optional: {n_vertices, n_faces} by component number.
 *   Two calls, as for the simplification.  fp_mesh_components_count builds the decomposition in an allocation owned by the context (about
 * 28 bytes a vertex and 8 a face, kept until a larger mesh arrives or the context is destroyed), SYNCHRONISES the stream and returns
 * h_counts = {components C, kept components, kept vertices nv, kept faces nf}.  F = 0 gives {V, 0, 0, 0}; V = 0 gives zeros.  The caller
 * allocates d_out_pos (nv,3), d_out_normals and d_out_colors (nv,3; each optional, and only with its input), d_out_faces (nf,3), and calls
 * fp_mesh_components_write with the SAME d_faces, F and V; it queues its kernels and does not synchronise.
 *   How: a lock-free union-find over an int32 parent array, one thread per face; the larger root is hooked under the smaller one with a
 * compare-and-swap, so a root only ever decreases and the final root is the component's minimum whatever the order of the unions; one
 * flatten pass; exclusive scans for the three numberings; int32 atomic adds for the counts.  No kernel waits for another workgroup.
 *   FP_EINVAL: a null ctx or h_counts, V or F outside their limits, null d_faces with F > 0, faces without a vertex, min_faces < 1,
 * min_fraction outside [0, 1] or NaN, largest_only other than 0 / 1, a face index outside 0 .. V-1 (found on the device, never followed);
 * for write: no count before it on this context, another mesh (d_faces, F or V) than the last count had, n_vertices or n_faces other than
 * its counts, a null required output or a null d_pos with nv > 0, an output attribute without its input.  FP_ENOMEM: the state does not
 * fit the device. */
int fp_mesh_components_count(fp_ctx *ctx, const int32_t *d_faces, int F, int V, int min_faces, float min_fraction, int largest_only,
                             int64_t *h_counts /* {components, kept components, kept vertices, kept faces} */, void *stream);
int fp_mesh_components_write(fp_ctx *ctx, const float *d_pos, const float *d_normals, const uint8_t *d_colors, int V, const int32_t *d_faces, int F,
                             float *d_out_pos, float *d_out_normals, uint8_t *d_out_colors, int32_t *d_out_faces,
                             int32_t *d_out_vertex_map, int32_t *d_out_label, int32_t *d_out_stats,
                             int64_t n_vertices, int64_t n_faces, void *stream);

/* ---- networks -------------------------------------------------------------------------------- */
typedef struct {
  const char *name;    /* reference state_dict key, e.g. "encodeA.0.net.0.weight" */
  const float *data;   /* host fp32, contiguous */
  int ndim;
  int64_t shape[4];
} fp_tensor;

#define FP_NET_REFINE 0  /* RefineNet (learning/models/refine_network.py:27-93) */
#define FP_NET_SCORE 1   /* ScoreNetMultiPair (learning/models/score_network.py:28-90) */
/* Builds device weights from a reference-layout state_dict: BatchNorm (eval) folded into the
 * preceding conv, fp16 [Cout][tap][Cin] packing, attention / linear weights.  use_bn mirrors cfg.use_BN. */
int fp_net_create(fp_ctx *ctx, int kind, const fp_tensor *tensors, int n_tensors, int use_bn, fp_net **out);
int fp_net_destroy(fp_net *net);
int fp_net_rot_dim(const fp_net *net);   /* 3 (axis_angle) or 6 (6d), from rot_head.1.weight */

/* a15: RefineNet.forward.  d_net_in: fp16 net tensor [2N][160][160][8], A = first N images, B = last N. */
int fp_refine_forward(fp_ctx *ctx, const fp_net *net, const void *d_net_in, int N, float *d_trans /* N*3 */,
                      float *d_rot /* N*rot_dim */, void *stream);
/* The shared trunk alone (encodeA/encodeAB | encoderA/encoderAB + pos_embed: refine_network.py:79-88, score_network.py:66-72):
 * d_tokens receives the (N,400,512) fp16 token tensor both heads read.  Exported for the parity tests, which compare it with
 * the reference module's encodeAB output. */
int fp_net_tokens(fp_ctx *ctx, const fp_net *net, const void *d_net_in, int N, void *d_tokens /* fp16 N*400*512 */, void *stream);
/* a19: ScoreNetMultiPair.extract_feat -> d_feats N*512 fp32 */
int fp_score_features(fp_ctx *ctx, const fp_net *net, const void *d_net_in, int N, float *d_feats, void *stream);
/* a19/a20: att_cross + linear over `groups` objects of L hypotheses each (score_network.py:82-88),
 * logits groups*L; d_argmax (groups, may be NULL) = per-object argmax (predict_score.py:196). */
int fp_score_tail(fp_ctx *ctx, const fp_net *net, const float *d_feats, int groups, int L, float *d_logits,
                  int32_t *d_argmax, void *stream);

/* a16: pose update (predict_pose_refine.py:195-231 + so3_exp_map + egocentric_delta_pose_to_pose).
 * trans_rep_tanh: 1 -> tanh(trans)*trans_normalizer (normalize_xyz False), 0 -> raw.  rot_dim 3|6.
 * (fp_refine_cfg.trans_rep_tanh also takes 2 = trans_rep 'deepim', see fp_pose_update_deepim.) */
int fp_pose_update(fp_ctx *ctx, const float *d_poseA, const float *d_trans, const float *d_rot, int N, int rot_dim,
                   int trans_rep_tanh, const float *trans_normalizer3, float rot_normalizer, float trans_scale,
                   float *d_pose_out, void *stream);

/* a16, trans_rep='deepim' (predict_pose_refine.py:201-215): trans[:, :2] shifts the projected centre inside the crop (units of
 * input_resize), trans[:, 2] scales its depth; d_tf_to_crops N*9 are the crop transforms of the pass, K the intrinsics. */
int fp_pose_update_deepim(fp_ctx *ctx, const float *d_poseA, const float *d_trans, const float *d_rot, int N, int rot_dim,
                          const float *d_tf_to_crops, const double *K, float input_resize, float rot_normalizer, float trans_scale,
                          float *d_pose_out, void *stream);

/* a17: PoseRefinePredictor.predict inner loop (predict_pose_refine.py:182-234), `iteration` rounds of
 * crop-window -> render -> observed crop -> RefineNet -> pose update, entirely on the device.
 * d_poses is updated in place.  d_trans/d_rot (may be NULL) receive the last raw network outputs. */
typedef struct {
  double crop_ratio;
  int normalize_xyz;
  int trans_rep_tanh;
  float trans_normalizer[3];
  float rot_normalizer;
} fp_refine_cfg;
int fp_refine_predict(fp_ctx *ctx, const fp_net *net, const fp_mesh *mesh, const float *d_rgb, const float *d_xyz_map,
                      int H, int W, const double *K, double mesh_diameter, const fp_refine_cfg *cfg, float *d_poses, int N,
                      int iteration, float *d_trans, float *d_rot, void *stream);

/* Several objects (frames / meshes) in ONE pass: the render + crop stages run per object, the networks run once on the
 * concatenated hypotheses (they are object-agnostic).  This is BASELINE configs[3] (4 concurrent objects x 252) and what
 * a rank of the sharded multi-GPU job executes (its slice of every object).  d_poses / d_trans / d_rot / d_feats are the
 * concatenation over objects in order; objs[i].n hypotheses belong to object i. */
typedef struct {
  const fp_mesh *mesh;
  const float *d_rgb;      /* H*W*3 float [0,255] */
  const float *d_geom;     /* refine: xyz_map H*W*3; score: depth H*W */
  int H, W;
  const double *K;         /* host, 3x3 row-major */
  double mesh_diameter;
  int n;                   /* hypotheses of this object */
} fp_object_batch;
int fp_refine_predict_multi(fp_ctx *ctx, const fp_net *net, const fp_object_batch *objs, int n_obj, const fp_refine_cfg *cfg,
                            float *d_poses, int iteration, float *d_trans, float *d_rot, void *stream);
/* The same with flags.  FP_REFINE_SHARED_TRANSLATION: the caller states that, on entry, every hypothesis of an object has the SAME
 * translation - what FoundationPose.register builds (src/estimater.py:126-135,196-199: the rotation grid around ONE guessed centre).  The
 * crop window depends on the translation only (src/Utils.py:577-621), so in the first iteration the observed side (predict_pose_refine.py:63,72
 * and its half of RefineNet.encodeA, refine_network.py:74-78) is one crop per object: it is cropped and encoded once instead of once per
 * hypothesis, by the same kernels - the refined poses are those of fp_refine_predict_multi bit for bit.  A false statement gives the
 * hypotheses of an object the first one's observed crop in iteration 1. */
#define FP_REFINE_SHARED_TRANSLATION 1u
int fp_refine_predict_multi_flags(fp_ctx *ctx, const fp_net *net, const fp_object_batch *objs, int n_obj, const fp_refine_cfg *cfg,
                                  float *d_poses, int iteration, float *d_trans, float *d_rot, unsigned flags, void *stream);
int fp_score_predict_features_multi(fp_ctx *ctx, const fp_net *net, const fp_object_batch *objs, int n_obj, double crop_ratio,
                                    int normalize_xyz, const float *d_poses, float *d_feats, void *stream);

/* a18-a20: ScorePredictor.predict up to per-hypothesis features (shardable), then the tail. */
int fp_score_predict_features(fp_ctx *ctx, const fp_net *net, const fp_mesh *mesh, const float *d_rgb, const float *d_depth,
                              int H, int W, const double *K, double mesh_diameter, double crop_ratio, int normalize_xyz,
                              const float *d_poses, int N, float *d_feats, void *stream);

/* ---- FoundationPose.track_one (src/estimater.py:250-268) as ONE call: depth prelude (erode -> bilateral -> back-projection, :256-260),
 *      refinement of the previous pose IN PLACE (:263), pose @ get_tf_to_centered_mesh() (:268) - every launch hand-written, hipGraph-
 *      capturable, no host synchronisation.  n_hyp > 1 (BASELINE configs[4], a build extension): d_perturb[i] applied to the previous pose
 *      (R_i = dR_i R, t_i = t + dt_i), all refined, scored (logits + 100, predict_score.py:209); the winner becomes d_pose. ------------- */
typedef struct fp_track_args {
  size_t struct_size;              /* = sizeof(fp_track_args) */
  const fp_net *refine_net, *score_net /* NULL when n_hyp == 1 */;
  const fp_mesh *mesh;
  const void *d_rgb;               /* H*W*3: uint8 (rgb_is_u8) or float [0,255] */
  int rgb_is_u8;
  const float *d_depth;            /* H*W raw depth, metres */
  int H, W;
  const double *K;                 /* host, 3x3 row-major */
  double mesh_diameter;
  const fp_refine_cfg *refine_cfg;
  double score_crop_ratio;
  int score_normalize_xyz;
  int iteration;
  int n_hyp;
  const float *d_perturb;          /* n_hyp*16 rigid perturbations, the first the identity; NULL when n_hyp == 1 */
  float model_center[3];           /* get_tf_to_centered_mesh() = translation by -model_center (src/estimater.py:82-86) */
  float *d_pose;                   /* 16: in = the previous frame's pose (centred mesh), out = this frame's */
  float *d_pose_of_mesh;           /* 16 out: d_pose @ get_tf_to_centered_mesh(), what track_one returns; device memory, or pinned host memory
                                      (hipHostMalloc: the last launch writes it there and the caller only waits for the stream) */
  float *d_poses, *d_scores;       /* n_hyp > 1: the refined hypotheses (n_hyp*16) and their scores (n_hyp) */
  int32_t *d_best;                 /* n_hyp > 1: index of the winner */
  float *d_depth_f, *d_xyz, *d_rgb_f; /* workspace: filtered depth H*W, xyz_map H*W*3, float colours H*W*3 (uint8 frames only) */
} fp_track_args;
int fp_track_frame(fp_ctx *ctx, const fp_track_args *args, void *stream);

/* ---- track_one for several objects of ONE frame in one call: the depth prelude once, then per iteration one crop-window (first
 *      iteration), one render and one observed-crop launch over all objects (an object whose mesh the one-launch render cannot take
 *      gets a render launch of its own), ONE network pass over the n_obj images and one fused tail that refines each object's pose and,
 *      in the last iteration, writes it back to d_pose together with pose @ get_tf_to_centered_mesh().  One hypothesis per object, no
 *      scoring.  hipGraph-capturable, no host synchronisation; the arena must already hold the pass (fp_ctx_reserve(ctx, 64)).  Each
 *      object's result is fp_track_frame's for it alone except for the last bits of the network pass, whose kernel forms depend on the
 *      number of images; with one object it is fp_track_frame's bit for bit. ----------------------------------- */
#define FP_TRACK_MAX_OBJECTS 8
typedef struct {
  const fp_mesh *mesh;             /* objects may share a mesh (two instances of one part) */
  double mesh_diameter;
  float model_center[3];           /* get_tf_to_centered_mesh() = translation by -model_center */
  float *d_pose;                   /* 16: in = the previous pose (centred mesh), out = this frame's; device memory */
  float *d_pose_of_mesh;           /* 16 out: d_pose @ get_tf_to_centered_mesh(); device or pinned host memory */
} fp_track_object;
typedef struct {
  size_t struct_size;              /* = sizeof(fp_track_objects_args) */
  const fp_net *refine_net;
  const void *d_rgb;               /* H*W*3: uint8 (rgb_is_u8) or float [0,255] */
  int rgb_is_u8;
  const float *d_depth;            /* H*W raw depth, metres */
  int H, W;
  const double *K;                 /* host, 3x3 row-major */
  const fp_refine_cfg *refine_cfg;
  int iteration;
  int n_obj;                       /* 1 .. FP_TRACK_MAX_OBJECTS */
  const fp_track_object *objs;     /* host array of n_obj objects */
  float *d_depth_f, *d_xyz, *d_rgb_f; /* workspace, as in fp_track_args */
} fp_track_objects_args;
int fp_track_objects(fp_ctx *ctx, const fp_track_objects_args *args, void *stream);

/* ---- FoundationPose.register (src/estimater.py:159-240) for several objects of ONE frame in one call (a build extension; the reference
 *      registers one object per call).  The frame's depth prelude runs once (erode -> bilateral, :169-170, and the float64 back-projection
 *      of :198), the mask reductions of every object are one launch (fp_mask_depth_stats_objects), the hypothesis sets are built on the
 *      device (fp_register_hypotheses), then `iteration` refinement passes and one scoring pass run over the hypotheses of all objects
 *      (fp_refine_predict_multi_flags with FP_REFINE_SHARED_TRANSLATION, fp_score_predict_features_multi, one score tail per object), and
 *      one last launch ranks every object's hypotheses (fp_register_rank).  The objects are cut into network passes at object boundaries:
 *      a pass holds at most max_pass_hyp hypotheses (an object with more gets a pass of its own), and an object with 1 or 2 hypotheses
 *      always gets a pass of its own (the few-image kernel forms) - so every object's poses and scores are those of
 *      its own register() call.  Synchronises the stream ONCE, after the mask reductions (register() has the same wait): not capturable. */
typedef struct {
  const fp_mesh *mesh;             /* objects may share a mesh */
  double mesh_diameter;
  float model_center[3];           /* get_tf_to_centered_mesh() = translation by -model_center */
  const uint8_t *d_mask;           /* H*W bytes, non-zero = object; NULL when the frame comes with a label image */
  int32_t label;                   /* label image: the pixels equal to `label` are this object */
  const float *d_rot_grid;         /* n_hyp*16: the rotation grid (src/estimater.py:106-124); its length differs between objects */
  int n_hyp;
  /* device outputs, written only when the object is registered */
  float *d_poses;                  /* n_hyp*16: refined poses of the centred mesh, best first (self.poses) */
  float *d_scores;                 /* n_hyp: logits + 100, descending (self.scores); equal scores keep their hypothesis order */
  int64_t *d_order;                /* n_hyp: hypothesis index of every rank; d_order[0] = best_id */
  float *d_pose_of_mesh;           /* 16: d_poses[0] @ get_tf_to_centered_mesh(), what register() returns; device or pinned host memory */
  /* host outputs */
  int32_t stats[6];                /* cmin, cmax, rmin, rmax, n_mask, n_usable of the mask on the filtered depth (as fp_mask_depth_stats) */
  float median;                    /* np.median of the usable depths */
  int registered;                  /* 0: fewer than 4 usable pixels (src/estimater.py:173-177) - nothing ran for this object, the device outputs are
                                      untouched; the caller returns eye(4) with guess_translation (:184-189) */
  double guess_translation[3];     /* (inv(K) @ [uc, vc, 1]) * median, zeros for an empty mask or no usable pixel (src/estimater.py:137-156) */
} fp_register_object;
typedef struct {
  size_t struct_size;              /* = sizeof(fp_register_objects_args) */
  const fp_net *refine_net, *score_net;
  const void *d_rgb;               /* H*W*3: uint8 (rgb_is_u8) or float [0,255] */
  int rgb_is_u8;
  const float *d_depth;            /* H*W raw depth, metres */
  int H, W;
  const double *K;                 /* host, 3x3 row-major */
  const double *K_inv;             /* host, 3x3 row-major: np.linalg.inv(K) as the caller computes it */
  const fp_refine_cfg *refine_cfg;
  double score_crop_ratio;
  int score_normalize_xyz;
  int iteration;
  int n_obj;                       /* 1 .. FP_TRACK_MAX_OBJECTS */
  fp_register_object *objs;        /* host array of n_obj objects (its host outputs are written) */
  const int32_t *d_labels;         /* H*W label image, or NULL: every object brings its d_mask */
  int max_pass_hyp;                /* hypotheses per network pass; 0: FP_REGISTER_PASS_HYP */
  float *d_depth_f, *d_xyz, *d_rgb_f; /* workspace / outputs: filtered depth H*W, xyz_map H*W*3, float colours H*W*3 (uint8 frames only) */
} fp_register_objects_args;
#define FP_REGISTER_PASS_HYP 1008  /* 4 x 252: the largest network pass the library's tests cover */
#define FP_REGISTER_MIN_VALID 4    /* src/estimater.py:185 */
int fp_register_objects(fp_ctx *ctx, fp_register_objects_args *args, void *stream);
/* The pieces of fp_register_objects, one launch each.
 * fp_mask_depth_stats for n_obj objects (src/estimater.py:137-156,173-177 per object) in ONE launch and one copy to the host: object o is
 * d_masks[o] (host array of n_obj device pointers, H*W bytes each) or, with d_labels (H*W int32) not NULL, the pixels equal to labels[o]
 * (d_masks may then be NULL).  h_stats (n_obj, 6) and h_median (n_obj) equal fp_mask_depth_stats of each mask bit for bit.  Synchronises. */
int fp_mask_depth_stats_objects(fp_ctx *ctx, const float *d_depth, const uint8_t *const *d_masks, const int32_t *d_labels, const int32_t *labels,
                                int n_obj, int H, int W, float min_depth, int32_t *h_stats, float *h_median, void *stream);
/* generate_random_pose_hypo over guess_translation (src/estimater.py:126-156) for n_obj objects in one launch: d_poses receives, object
 * after object, d_rot_grids[o][i] with the translation (K_inv @ [(cmin+cmax)/2, (rmin+rmax)/2, 1]) * median in float64 (the dot product as
 * fma(k0, u, k1 * v) + k2), rounded once to float32.  h_stats (n_obj, 6) / h_median (n_obj): fp_mask_depth_stats_objects' results. */
int fp_register_hypotheses(fp_ctx *ctx, const float *const *d_rot_grids, const int *n_hyp, int n_obj, const int32_t *h_stats, const float *h_median,
                           const double *K_inv, float *d_poses, void *stream);
/* The ranking that ends register() (src/estimater.py:230-237) for n_obj objects in one launch: object o's n_hyp[o] poses / scores lie
 * behind one another in d_poses / d_scores; its d_poses_out[o] / d_scores_out[o] / d_order_out[o] receive them in stable descending order
 * of the score (equal scores: the lower hypothesis index first), d_pose_of_mesh[o] (device or pinned host) the best pose @
 * get_tf_to_centered_mesh() (model_centers: n_obj*3 host floats).  The pointer arrays are host arrays of device pointers. */
int fp_register_rank(fp_ctx *ctx, const float *d_poses, const float *d_scores, const int *n_hyp, int n_obj, const float *model_centers,
                     float *const *d_poses_out, float *const *d_scores_out, int64_t *const *d_order_out, float *const *d_pose_of_mesh, void *stream);

/* fp_score_tail with a feature row stride (feat_ld >= 512 floats: 528 reads the [feature | pose] rows below in place) and, optionally
 * (d_scores != NULL), scores = logits + score_offset from the same launch (ScorePredictor.predict: + 100, predict_score.py:209) */
int fp_score_tail_scores(fp_ctx *ctx, const fp_net *net, const float *d_feats, int feat_ld, int groups, int L, float score_offset, float *d_logits,
                         float *d_scores, int32_t *d_argmax, void *stream);
/* fp_score_predict_features_multi writing the hypothesis-parallel job's all-gather records directly: d_rows (sum n) x 528 floats =
 * [feature 512 | pose 16] per hypothesis (ONE all-gather of these rows precedes the cross-hypothesis tail) */
int fp_score_predict_rows_multi(fp_ctx *ctx, const fp_net *net, const fp_object_batch *objs, int n_obj, double crop_ratio,
                                int normalize_xyz, const float *d_poses, float *d_rows, void *stream);

/* ---- the picture the reference's demo ends with (main.py:67-71: draw_posed_3d_box and draw_xyz_axis, src/Utils.py:667-749, on the frame),
 *      for up to FP_DRAW_MAX_OBJECTS objects of one frame in two launches, plus the silhouettes of an owner map (fp_scene_instances' d_owner).
 *      The reference draws with cv2.line / cv2.arrowedLine (LINE_AA, Wu's lines); cv2 is not part of this build and the drawing rule below is
 *      the project's own, like the font of vis.py: the same segments between the same rounded endpoints, but cv2's anti-aliased fringe
 *      differs from it.
 *      Segments: per object in index order the 12 edges of the box - the edges along x over (y, z), those along y over (x, z), those along z
 *      over (x, y), each min before max (draw_posed_3d_box's order; bbox_min / bbox_max after a per-component min / max) - then the axes x, y,
 *      z from the origin, axis_scale long.  Endpoints: p_cam = (d_poses[o] @ offset) p in float64 (offset is rigid: its last row is taken as
 *      0 0 0 1); a segment wholly behind z = FP_DRAW_ZNEAR is dropped, one that crosses it is cut there; (u, v) = (K[0,:] . p / z,
 *      K[1,:] . p / z), each rounded to the nearest integer, ties to even (np.round, as the reference rounds); a segment with a rounded
 *      coordinate beyond +-2^20 is dropped whole.  Coverage of a pixel: d = the Euclidean distance in fp32 of its integer centre to the
 *      segment (a segment of length zero is a point), a = clamp(thickness / 2 + 0.5 - d, 0, 1) * opacity, c = c + a (colour - c) in fp32,
 *      segment after segment in the order above.  (The launch holds each segment as the part inside the frame grown by 64 pixels, cut in
 *      float64 - the pixels' distances are those to the whole segment; on frames up to 4096 pixels a side d is within 1e-3 of the exact one.)
 *      Before the segments, where d_owner[p] = o in 0 .. n_obj-1 (any other value is "none"): with FP_DRAW_FILL c = c + fill_alpha
 *      (fill_color_o - c); with FP_DRAW_CONTOUR, if a 4-neighbour of p inside the frame has another owner, c = box_color_o.  Each channel is
 *      rounded once at the end (rint, clamped to 0 .. 255); a pixel nothing touched keeps its byte.  Deterministic: no atomics, a pixel
 *      belongs to one thread.
 *      d_poses is read by the launches, not by the host: the call can sit behind fp_track_objects in one hipGraph, and a replay draws the
 *      poses the buffer holds then.  K, objs and the scalar arguments are read during the call (a captured graph keeps their values).
 *      Nothing synchronises.  Workspace: under 64 KB of the context's arena - the call leaves the arena generation alone when
 *      fp_ctx_reserve (or any larger call) has run before; call it before capturing.
 *      n_obj = 0 or flags = 0: d_img_in is copied to d_img_out when they differ, nothing else happens. */
#define FP_DRAW_MAX_OBJECTS 64
#define FP_DRAW_BOX 1       /* the 12 edges of bbox */
#define FP_DRAW_AXES 2      /* x, y, z axes from the origin, length axis_scale */
#define FP_DRAW_FILL 4      /* tint the pixels d_owner gives to an object */
#define FP_DRAW_CONTOUR 8   /* 1-pixel inner contour of d_owner's regions */
#define FP_DRAW_ZNEAR 0.01  /* metres: segments are clipped to z >= this before projection */
typedef struct {
  float bbox_min[3], bbox_max[3];  /* in the frame `offset` maps from */
  float offset[16];                /* row-major rigid 4x4, right-multiplied: drawn pose = d_poses[o] @ offset (main.py:67: inv(to_origin)); identity leaves the pose */
  float axis_scale;                /* metres (reference default 0.1) */
  uint8_t box_color[3], axis_color[9] /* x, y, z */, fill_color[3];   /* in the channel order of the image */
} fp_draw_object;
typedef struct {
  size_t struct_size;              /* = sizeof(fp_draw_args) */
  const uint8_t *d_img_in; uint8_t *d_img_out;   /* H*W*3; equal pointers = in place; any other overlap is refused */
  int H, W; const double *K;                     /* host 3x3; the first two rows are used in full (skew included) */
  const float *d_poses; int n_obj;               /* (n_obj,4,4) DEVICE: read by the launch, not by the host */
  const fp_draw_object *objs;                    /* host */
  int flags; float box_thickness /* 2 */, axis_thickness /* 3 */, opacity /* 1 - transparency */, fill_alpha;
  const int32_t *d_owner;                        /* H*W, fp_scene_instances' owner; required with FILL / CONTOUR */
} fp_draw_args;
int fp_draw_poses(fp_ctx *ctx, const fp_draw_args *args, void *stream);

/* ---- model-free set-up: posed RGB-D reference views fused into a truncated signed distance volume, and a coloured triangle mesh
 *      extracted from it by marching tetrahedra.  The reference trains a neural field for this (bundlesdf/run_nerf.py); this is a
 *      different, classical algorithm with the arithmetic below.  Everything is fp32, not contracted, every
 *      operation in the written order; / and sqrt are correctly rounded.
 *      Volume.  dims = (nx, ny, nz) sample points; point (i, j, k) has index i + nx (j + ny k) in every plane (i fastest) and lies at
 *      s = (ox + v (float)i, oy + v (float)j, oz + v (float)k), with o = (float)origin (object frame, metres) and v = voxel_size.  Six
 *      fp32 planes, zero after create and reset: tsdf T, weight W, r, g, b (0 .. 255), color_weight Wc.  The volume owns its device
 *      memory (planes and extraction scratch: 33 bytes a point, plus 8 per 1024 points), not the context's arena.
 *      fp_tsdf_create: FP_EINVAL for a null pointer, a dim < 2, nx ny nz above FP_TSDF_MAX_POINTS, voxel_size or trunc not > 0 (or not
 *      finite), a non-finite origin; FP_ENOMEM when an allocation fails (nothing is kept).
 *      Integrate.  One thread per sample point; the views are taken inside the thread in index order, so a call reads and writes the
 *      volume once.  d_depth (n_views,H,W) fp32 metres; d_rgb (n_views,H,W,3) uint8 or null; d_mask (n_views,H,W) uint8 or null; K host
 *      float64 3x3, of which fx = K[0], cx = K[2], fy = K[4], cy = K[5] are used, each cast to fp32 (no skew); cam_in_ob host float64
 *      (n_views,4,4), camera-to-object, rigid: its inverse is taken on the host in float64 as R = Rc^T and
 *      t_i = -((Rc[0][i] tc[0] + Rc[1][i] tc[1]) + Rc[2][i] tc[2]), then cast to fp32.  Per view, for the point s:
 *        q_a = ((R[a][0] s.x + R[a][1] s.y) + R[a][2] s.z) + t[a];                    skip the view unless q.z >= 0.001
 *        col = floor((fx (q.x / q.z) + cx) + 0.5), row = floor((fy (q.y / q.z) + cy) + 0.5);   skip unless 0 <= col < W and 0 <= row < H
 *        d = depth[row, col];               skip unless d >= 0.001 and d < zfar, and, with a mask, mask[row, col] != 0
 *        sdf = d - q.z;                     skip if sdf < -trunc
 *        tau = min(1, sdf / trunc);  T = (T W + tau) / (W + 1);  W = W + 1
 *        if rgb is given and sdf <= trunc:  c = (c Wc + (float)rgb[row, col, ch]) / (Wc + 1) for c = r, g, b;  Wc = Wc + 1
 *      ("unless" so that a NaN skips.)  Consequences: one call with n views is bit for bit n calls with one view each in the same order;
 *      a point belongs to one thread - no atomics, deterministic; nothing synchronises.  FP_EINVAL: a null ctx, vol, d_depth, K or
 *      cam_in_ob, n_views outside 0 .. FP_TSDF_MAX_VIEWS (0 does nothing), H or W < 1, fx or fy not > 0, zfar not > 0 (infinity is
 *      allowed), a view matrix that is not finite or whose last row is not 0 0 0 1.
 *      Surface (marching tetrahedra, Kuhn / Freudenthal split).  A point is observed when W >= min_weight and negative when T < 0.  It
 *      owns 7 edges, slot 0 .. 6, to the points at +x, +y, +z, +xy, +xz, +yz, +xyz (those inside the volume).  An edge (a, b) carries a
 *      vertex iff both ends are observed and exactly one is negative: u = T_a / (T_a - T_b), position s_a + (s_b - s_a) u per component,
 *      colour floor((c_a + (c_b - c_a) u) + 0.5) clamped to 0 .. 255, normal n = g_a + (g_b - g_a) u divided by sqrt((n.x n.x + n.y n.y)
 *      + n.z n.z) (left as it is when that is 0), where g is the gradient of T per axis: (T[+1] - T[-1]) 0.5 when both neighbours exist
 *      and are observed, T[+1] - T or T - T[-1] when one does, else 0.  Vertices are welded by construction: id = the number of
 *      vertices of all points with a smaller index (an exclusive scan) + the number of lower slots of the same point that carry one.
 *      The cube at (i, j, k), i < nx-1, j < ny-1, k < nz-1, is cut into 6 tetrahedra around its (0,0,0)-(1,1,1) diagonal: tetrahedron p
 *      has the corners 0, e_a, e_a + e_b, (1,1,1) for the p-th permutation (a, b, c) of (x, y, z) in lexicographic order, numbered
 *      0 .. 3.  It emits triangles only if its four corners are observed.  One corner L of the other sign than A < B < C: the triangle
 *      (LA, LB, LC) of the vertices on those edges; two negative N0 < N1 and two non-negative P0 < P1: the quad q = (N0P0, N0P1, N1P1,
 *      N1P0) as (q0, q1, q2), (q0, q2, q3).  The last two indices of every triangle are swapped where needed so that the normal
 *      (v1 - v0) x (v2 - v0) points from the negative to the non-negative side - outward.  (The 16-case table is derived from this
 *      rule when the volume is created.)  Faces are ordered by cube index, tetrahedron, triangle; vertices by point index, slot.  Both
 *      orders are independent of the execution order; no atomics.  The scan is reduce / scan of the block sums / add, recursive, with
 *      no waiting between workgroups.
 *      fp_tsdf_extract_count runs the flag and count pass and the scan, SYNCHRONISES the stream and returns h_counts = {vertices, faces}.
 *      fp_tsdf_extract_write fills d_vertices (n_vertices,3) fp32, d_normals (n_vertices,3) fp32 or null, d_colors (n_vertices,3) uint8
 *      or null, d_faces (n_faces,3) int32; nothing synchronises.  It returns FP_EINVAL when no count has happened since the last
 *      integrate or reset of the volume, when n_vertices / n_faces are not the counted ones, or when a required buffer is null
 *      (d_vertices with n_vertices > 0, d_faces with n_faces > 0).  min_weight must be > 0 (FP_EINVAL).
 *      fp_tsdf_read_plane copies plane FP_TSDF_PLANE_* into d_out (nx ny nz fp32, device) on the stream.
 *      Align (frame-to-model: one Gauss-Newton linearisation of the poses of n_views depth maps against the volume; the solver is the
 *      caller's - foundationpose_amd/reconstruct.py: TsdfVolume.align).  d_depth, d_mask, K and cam_in_ob as for integrate, but cam_in_ob
 *      is used as given, not inverted: Rc, tc = its rotation and translation cast to fp32.  One workgroup per (view, tile of 1024 pixels),
 *      pixel index row W + col.  Per view and pixel, in fp32, not contracted, in the written order:
 *        d = depth[row, col];               skip unless d >= 0.001 and d < zfar, and, with a mask, mask[row, col] != 0
 *        p = ((((float)col - cx) / fx) d, (((float)row - cy) / fy) d, d)
 *        x_a = ((Rc[a][0] p.x + Rc[a][1] p.y) + Rc[a][2] p.z) + tc[a]                  the pixel's point in the object frame
 *        g_a = (x_a - o_a) / v,  i_a = floor(g_a),  f_a = g_a - i_a;   skip unless 0 <= i_a <= n_a - 2 for a = x, y, z (the 8 corners
 *        (i + {0,1}) of the cell lie inside the volume), and unless W >= min_weight at all 8 corners
 *        T_c = T at corner c = dx + 2 dy + 4 dz.  x-differences d00 = T1 - T0, d10 = T3 - T2, d01 = T5 - T4, d11 = T7 - T6; x-lerps
 *        a00 = T0 + d00 f.x, a10 = T2 + d10 f.x, a01 = T4 + d01 f.x, a11 = T6 + d11 f.x; y-differences e0 = a10 - a00, e1 = a11 - a01;
 *        y-lerps b0 = a00 + e0 f.y, b1 = a01 + e1 f.y; dz = b1 - b0; the trilinear interpolant T = b0 + dz f.z
 *        skip unless |T| < 1                                                            (a truncated sample has no gradient)
 *        h0 = d00 + (d10 - d00) f.y, h1 = d01 + (d11 - d01) f.y;  s = trunc / v
 *        G = ((h0 + (h1 - h0) f.z) s, (e0 + (e1 - e0) f.z) s, dz s)                     the gradient of the same interpolant, per metre
 *        r = T trunc                                                                    the residual, metres
 *        J = (G.x, G.y, G.z, x.y G.z - x.z G.y, x.z G.x - x.x G.z, x.x G.y - x.y G.x)   dr / dxi of cam_in_ob <- exp(xi) cam_in_ob,
 *                                                                                       xi = (translation, rotation), object frame
 *      ("unless" so that a NaN skips.)  d_rows, when not null, (n_views,H,W,8) fp32 on the device, 16-byte aligned
 *      (it is written as float4; FP_EINVAL otherwise), gets (J0 .. J5, r, valid = 1) per
 *      pixel and eight zeros where the pixel was skipped: it exists so that the rule can be tested bit for bit.  h_sums, HOST
 *      (n_views, FP_TSDF_ALIGN_TERMS) float64: per view the 21 entries of the upper triangle of J^T J row by row ((0,0), (0,1) .. (0,5),
 *      (1,1) .. (5,5)), the 6 of J^T r, sum r r, the number of valid pixels.  Every term is formed in double from the fp32 values (a
 *      product of two fp32 numbers is exact in double) and added in double: over a lane's 4 pixels, over the wave by a butterfly, over
 *      the waves in order, and by a second launch over the tiles in order.  No atomics: a view's 29 numbers are bit-identical from run
 *      to run, in any batch and at any index of it.  fp_tsdf_align SYNCHRONISES the stream (the sums are copied to the host; the partial
 *      sums live in the context's arena for the duration of the call).  The volume is only read; one that was never integrated into
 *      skips every pixel (count 0).  FP_EINVAL: a null ctx, vol, d_depth, K, cam_in_ob or h_sums, n_views outside 0 ..
 *      FP_TSDF_MAX_VIEWS (0 writes nothing), H or W < 1, fx or fy not > 0, zfar not > 0 (infinity is allowed), min_weight not > 0, a
 *      view matrix that is not finite or whose last row is not 0 0 0 1. */
typedef struct fp_tsdf fp_tsdf;
#define FP_TSDF_MAX_POINTS (1 << 27)   /* 512^3 */
#define FP_TSDF_MAX_VIEWS 64           /* per fp_tsdf_integrate call: the view matrices travel as kernel arguments */
#define FP_TSDF_PLANE_TSDF 0
#define FP_TSDF_PLANE_WEIGHT 1
#define FP_TSDF_PLANE_R 2
#define FP_TSDF_PLANE_G 3
#define FP_TSDF_PLANE_B 4
#define FP_TSDF_PLANE_COLOR_WEIGHT 5
#define FP_TSDF_ALIGN_TERMS 29         /* doubles per view of fp_tsdf_align's h_sums */
int fp_tsdf_create(fp_ctx *ctx, const double *origin, float voxel_size, const int *dims, float trunc, fp_tsdf **out);
int fp_tsdf_destroy(fp_tsdf *vol);
int fp_tsdf_reset(fp_ctx *ctx, fp_tsdf *vol, void *stream);
int fp_tsdf_integrate(fp_ctx *ctx, fp_tsdf *vol, const float *d_depth, const uint8_t *d_rgb, const uint8_t *d_mask, int n_views, int H, int W,
                      const double *K, const double *cam_in_ob, float zfar, void *stream);
int fp_tsdf_extract_count(fp_ctx *ctx, fp_tsdf *vol, float min_weight, int64_t *h_counts, void *stream);
int fp_tsdf_extract_write(fp_ctx *ctx, fp_tsdf *vol, float *d_vertices, float *d_normals, uint8_t *d_colors, int32_t *d_faces,
                          int64_t n_vertices, int64_t n_faces, void *stream);
int fp_tsdf_read_plane(fp_ctx *ctx, const fp_tsdf *vol, int plane, float *d_out, void *stream);
int fp_tsdf_align(fp_ctx *ctx, const fp_tsdf *vol, const float *d_depth, const uint8_t *d_mask, int n_views, int H, int W, const double *K,
                  const double *cam_in_ob, float zfar, float min_weight, float *d_rows, double *h_sums, void *stream);

/* ---- posing reference views from depth alone: point-to-plane ICP between PAIRS of depth maps with projective association, linearised
 *      for all pairs in one launch (csrc/depth_icp.hip); the joint solve over all views is the caller's - foundationpose_amd/
 *      reconstruct.py: solve_joint_step, joint_refine_view_poses, estimate_view_poses.  No volume is needed and the basin is set by a
 *      distance gate, not by a voxel size.  Everything is fp32, not contracted, every operation in the written order; / and sqrtf are
 *      correctly rounded ("unless" so that a NaN skips).  tests/depth_icp_oracle.py restates both rules in numpy.
 *      d_depth (n_views,H,W) fp32 metres on the device, K (3,3) float64 HOST (fx, fy, cx, cy cast to fp32), pixel index row W + col.
 *      The back-projection of a depth d at (row, col) is that of fp_tsdf_align: p = ((((float)col - cx) / fx) d, (((float)row - cy) / fy) d, d).
 *      Normals.  fp_depth_normals writes d_normals (n_views,H,W,4) fp32, 16-byte aligned (it is written as float4; FP_EINVAL
 *      otherwise), one thread per pixel; nothing synchronises.  d_mask (n_views,H,W) uint8 or null.  Per pixel:
 *        ok(r,c): d >= 0.001 and d < zfar and, with a mask, mask != 0
 *        write (0,0,0,0) unless 1 <= r <= H-2 and 1 <= c <= W-2, ok at the pixel and at its four neighbours (r, c-1), (r, c+1), (r-1, c),
 *        (r+1, c), and |d_neighbour - d| <= max_jump for each of the four
 *        a = p(r,c+1) - p(r,c-1),  b = p(r+1,c) - p(r-1,c)
 *        m = b x a = (b.y a.z - b.z a.y, b.z a.x - b.x a.z, b.x a.y - b.y a.x)          each component a difference of two products
 *        l2 = (m.x m.x + m.y m.y) + m.z m.z;   write (0,0,0,0) unless l2 > 0
 *        n = m / sqrtf(l2);   write (n.x, n.y, n.z, 1)                                   n faces the camera: n.z < 0 on a fronto-parallel surface
 *      Normals come from one-pixel central differences of the maps the caller passes: smooth the maps first if they are noisy.
 *      Pairs.  fp_depth_pairs_align takes the depth maps, the normals of fp_depth_normals, cam_in_ob (n_views,4,4) float64 HOST
 *      (camera-to-object) and pairs (n_pairs,2) int32 HOST, directed (s, t): the pixels of view s are projected into view t.  Per view v,
 *      C_v = (Rc, tc) is cam_in_ob cast to fp32 and D_v = (Ri, ti) its inverse formed in double - Ri[a][i] = R[i][a],
 *      ti[a] = -((R[0][a] t[0] + R[1][a] t[1]) + R[2][a] t[2]) - and then cast to fp32.  One workgroup per (pair, tile of 1024 pixels of
 *      view s).  Per pair (s, t) and pixel (r, c) of view s:
 *        skip unless normals_s[r,c].w != 0
 *        p = the back-projection of depth_s[r,c];  ns = normals_s[r,c].xyz
 *        x_a = ((Rc_s[a][0] p.x + Rc_s[a][1] p.y) + Rc_s[a][2] p.z) + tc_s[a]            the point in the object frame
 *        y_a = ((Ri_t[a][0] x.x + Ri_t[a][1] x.y) + Ri_t[a][2] x.z) + ti_t[a]            the point in camera t
 *        skip unless y.z >= 0.001
 *        u = (fx y.x) / y.z + cx,  v = (fy y.y) / y.z + cy;   cf = floorf(u + 0.5f),  rf = floorf(v + 0.5f)
 *        skip unless 0 <= cf <= W-1 and 0 <= rf <= H-1 (compared as floats);   skip unless normals_t[rf,cf].w != 0
 *        q = the back-projection of depth_t[rf,cf] at (rf, cf);  n = normals_t[rf,cf].xyz;   e = y - q
 *        skip unless (e.x e.x + e.y e.y) + e.z e.z < dist_max dist_max
 *        w_a = (Rc_s[a][0] ns.x + Rc_s[a][1] ns.y) + Rc_s[a][2] ns.z;   g_a = (Ri_t[a][0] w.x + Ri_t[a][1] w.y) + Ri_t[a][2] w.z
 *        skip unless (g.x n.x + g.y n.y) + g.z n.z >= cos_min
 *        r = (n.x e.x + n.y e.y) + n.z e.z                                               the point-to-plane residual, metres
 *        no_a = (Rc_t[a][0] n.x + Rc_t[a][1] n.y) + Rc_t[a][2] n.z                        the target normal in the object frame
 *        J = (no.x, no.y, no.z, x.y no.z - x.z no.y, x.z no.x - x.x no.z, x.x no.y - x.y no.x)
 *      J is dr / dxi_s for cam_in_ob_s <- exp(xi_s) cam_in_ob_s, xi = (translation, rotation) in the object frame, at fixed association;
 *      dr / dxi_t is exactly -J (moving view t by xi moves the point in camera t as moving view s by -xi does), so ONE 6-vector serves
 *      both ends of the pair: the caller adds A = sum J J^T to the diagonal blocks of s and t and subtracts it from the two off-diagonal
 *      blocks, adds b = sum J r to the gradient of s and subtracts it from that of t.
 *      d_rows, when not null, (n_pairs,H,W,8) fp32 on the device, 16-byte aligned (FP_EINVAL otherwise), gets (J0 .. J5, r, 1) per pixel
 *      and eight zeros where the pixel was skipped.  h_sums, HOST (n_pairs, FP_DEPTH_ALIGN_TERMS) float64: per pair the 29 terms of
 *      fp_tsdf_align's h_sums in the same order (the upper triangle of J^T J row by row, J^T r, sum r r, the number of valid pixels),
 *      formed and added in double in the same way: over a lane's 4 pixels, over the wave by a butterfly, over the waves in order, and by
 *      a second launch over the tiles in order.  No atomics: a pair's 29 numbers are bit-identical from run to run, in any batch and at
 *      any index of it.  fp_depth_pairs_align SYNCHRONISES the stream (the partial sums and the pairs' matrices live in the context's
 *      arena for the duration of the call).  At most FP_DEPTH_ALIGN_MAX_PAIRS pairs per call (the partial sums of 256 pairs of 640 x 480
 *      pixels take 17 MB); the Python wrapper cuts longer lists into calls.  At most FP_TSDF_MAX_VIEWS views.
 *      Geometry only: a turntable of a rotationally symmetric object leaves the rotation about its axis unobservable (the photometric
 *      term below is for that).
 *      FP_EINVAL, each checked before ctx is looked into: a null ctx, d_depth, d_normals, K (both calls), cam_in_ob, h_sums, or pairs with
 *      n_pairs > 0; a misaligned d_normals or d_rows; n_views outside 0 .. FP_TSDF_MAX_VIEWS (fp_depth_normals: 0 writes nothing); n_pairs
 *      < 0 or above the cap (0 writes nothing); a pair index outside 0 .. n_views-1, or s == t; H or W < 1; a non-finite K or fx or fy
 *      not > 0; zfar not > 0 (infinity is allowed); max_jump not > 0; dist_max not > 0; cos_min outside [-1, 1]; a view matrix that is
 *      not finite or whose last row is not 0 0 0 1.
 *      Photometric term (optional; fp_view_intensity, fp_depth_pairs_align_photo): a grey-value residual on the SAME association, for
 *      surfaces whose geometry leaves a direction free (a turntable of a bottle, a face seen head-on) but whose texture does not.
 *      Same number format and ordering conventions as above.  tests/photo_icp_oracle.py restates both rules in numpy.
 *      Intensity map.  fp_view_intensity reads d_rgb (n_views,H,W,3) uint8 and the normals of fp_depth_normals and writes d_intensity
 *      (n_views,H,W,4) fp32, 16-byte aligned (d_normals too; FP_EINVAL otherwise), one thread per pixel; nothing synchronises.  Per pixel:
 *        I(r,c) = ((0.299f (float)R + 0.587f (float)G) + 0.114f (float)B) / 255.f
 *        write (0,0,0,0) unless normals[r,c].w != 0 and 1 <= r <= H-2 and 1 <= c <= W-2 (a normal of fp_depth_normals is never on the
 *        border; the condition keeps the neighbours inside the view for any other map)
 *        gx = (I(r,c+1) - I(r,c-1)) 0.5f,   gy = (I(r+1,c) - I(r-1,c)) 0.5f;   write (I(r,c), gx, gy, 1)
 *      Where the normal is there, the pixel and its four neighbours are masked, valid depth within max_jump of each other, so the
 *      gradient never crosses an occlusion edge.
 *      Photometric row.  fp_depth_pairs_align_photo is fp_depth_pairs_align with d_intensity and i_max; per pair (s, t) and pixel (r, c)
 *      of view s that passed EVERY condition of the rule above, with the same x, y, u, v (before rounding), cf, rf:
 *        a4 = intensity_s[r,c],  b4 = intensity_t[rf,cf];   skip unless a4.w != 0;   skip unless b4.w != 0
 *        du = u - cf,  dv = v - rf                                                      the projection's offset from the pixel centre
 *        r = ((b4.x + b4.y du) + b4.z dv) - a4.x                                        first-order sub-pixel value of view t minus view s
 *        skip unless fabsf(r) < i_max
 *        jx = (b4.y fx) / y.z,  jy = (b4.z fy) / y.z,  jz = -((jx y.x + jy y.y) / y.z)   d r / d y: the image gradient through the projection
 *        a_k = (Rc_t[k][0] jx + Rc_t[k][1] jy) + Rc_t[k][2] jz                           the same in the object frame
 *        J = (a.x, a.y, a.z, x.y a.z - x.z a.y, x.z a.x - x.x a.z, x.x a.y - x.y a.x)
 *      As for the geometric row J is dr / dxi_s and dr / dxi_t is exactly -J, at fixed association and fixed b4, du and dv taken as
 *      functions of y: y = C_t^-1 expm(-xi_t) x with x = expm(xi_s) C_s p, and r depends on the two poses through y only (a4 is a value
 *      of view s at a fixed pixel, b4 a record of view t at a fixed pixel), so moving view t by xi moves y as moving view s by -xi does.
 *      h_sums is (n_pairs, FP_PHOTO_ALIGN_TERMS = 58): terms 0 .. 28 are fp_depth_pairs_align's 29, bit-identical to that call's on the
 *      same inputs; terms 29 .. 57 are the same 29 quantities of the photometric rows (the number of valid photometric pixels last),
 *      formed and added in the same way.  The residual is in units of intensity (0 .. 1): the caller weighs it against metres
 *      (reconstruct.py: combine_sums).  d_rows, when not null, is (n_pairs,H,W,16): the 8 geometric floats, then (J0 .. J5, r, 1) of the
 *      photometric row or eight zeros.  i_max > 0 (infinity is allowed).  Every other check, limit and the synchronisation are those of
 *      fp_depth_pairs_align; d_intensity must not be null and must be 16-byte aligned.
 *      Limits: brightness constancy is assumed (a camera moving round a static object under fixed light; NOT an object turning under a
 *      fixed lamp, speculars or exposure changes); grey only; no image pyramid - the basin is half a texture wavelength; no blur - the
 *      caller may pre-filter the rgb. */
#define FP_DEPTH_ALIGN_TERMS 29        /* doubles per pair of fp_depth_pairs_align's h_sums */
#define FP_PHOTO_ALIGN_TERMS 58        /* doubles per pair of fp_depth_pairs_align_photo's h_sums */
#define FP_DEPTH_ALIGN_MAX_PAIRS 256   /* per fp_depth_pairs_align and fp_depth_pairs_align_photo call */
int fp_depth_normals(fp_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int n_views, int H, int W, const double *K, float zfar,
                     float max_jump, float *d_normals, void *stream);
int fp_depth_pairs_align(fp_ctx *ctx, const float *d_depth, const float *d_normals, int n_views, int H, int W, const double *K,
                         const double *cam_in_ob, const int32_t *pairs, int n_pairs, float dist_max, float cos_min, float *d_rows,
                         double *h_sums, void *stream);
int fp_view_intensity(fp_ctx *ctx, const uint8_t *d_rgb, const float *d_normals, int n_views, int H, int W, float *d_intensity, void *stream);
int fp_depth_pairs_align_photo(fp_ctx *ctx, const float *d_depth, const float *d_normals, const float *d_intensity, int n_views, int H, int W,
                               const double *K, const double *cam_in_ob, const int32_t *pairs, int n_pairs, float dist_max, float cos_min,
                               float i_max, float *d_rows, double *h_sums, void *stream);

/* ---- polishing object poses against depth: point-to-plane ICP between a MODEL at a pose and the depth of the frame it is seen in, with
 *      projective association, linearised for N poses in one launch, stepped on the device and looped without the host
 *      (csrc/pose_icp.hip).  The aligners above move cameras against other depth maps or a volume; this one moves an object pose onto
 *      the measured surface by geometry alone.  Number format and ordering conventions are those of fp_depth_pairs_align: fp32, not
 *      contracted, every operation in the written order, every condition written as "unless" so that a NaN skips, pixel index
 *      row W + col, back-projection q of a depth d at (row, col) = ((((float)col - cx) / fx) d, (((float)row - cy) / fy) d, d).
 *      tests/pose_icp_oracle.py restates everything below in numpy and Python floats.
 *      Linearisation.  fp_pose_depth_align takes, all on the device: d_xyz and d_normal (N,h,w,3) fp32 - the camera-space maps fp_render
 *      writes for the N poses, at full frame or through d_bbox2d crops, background 0 (any maps of that meaning will do: the rule looks at
 *      nothing else of the model); the observed d_depth (H,W) and its d_normals (H,W,4) of fp_depth_normals, 16-byte aligned - a mask
 *      enters there and nowhere else; d_poses (N,16) fp32 row-major, of which only the origin c = (pose[3], pose[7], pose[11]) is read.
 *      K (3,3) float64 HOST.  Both normal maps face the camera: n.z < 0 on a fronto-parallel surface (fp_render's normal is the outward
 *      vertex normal rotated into the camera frame; tests/test_gpu_pose_icp.py checks the sign on a sphere).  Per pose i and map pixel k:
 *        y = xyz[i,k];  nm = normal[i,k]
 *        skip unless y.z >= 0.001                                                        "rendered" counts the pixels that pass
 *        u = (fx y.x) / y.z + cx,  v = (fy y.y) / y.z + cy;   cf = floorf(u + 0.5f),  rf = floorf(v + 0.5f)
 *        skip unless 0 <= cf <= W-1 and 0 <= rf <= H-1 (compared as floats);   n4 = normals[rf,cf];   skip unless n4.w != 0
 *        q = the back-projection of depth[rf,cf] at (rf, cf);   n = n4.xyz;   e = y - q  "observed" counts the pixels that got here
 *        skip unless (e.x e.x + e.y e.y) + e.z e.z < dist_max dist_max
 *        skip unless (nm.x n.x + nm.y n.y) + nm.z n.z >= cos_min
 *        r = (n.x e.x + n.y e.y) + n.z e.z                                               the point-to-plane residual, metres
 *        x = y - c
 *        J = (n.x, n.y, n.z, x.y n.z - x.z n.y, x.z n.x - x.x n.z, x.x n.y - x.y n.x)
 *      J is dr / dxi for R <- exp([w]) R, t <- t + tau with xi = (tau, w) in the camera frame, at fixed association: a twist about the
 *      pose's own origin, not about the camera's.  With a mesh centred on its origin (estimater.py) that is the object's centre, which
 *      keeps tau and w decoupled.
 *      d_sums (N, FP_POSE_ALIGN_TERMS) float64 on the DEVICE: per pose the 29 terms of fp_tsdf_align's h_sums in the same order (the
 *      upper triangle of J^T J row by row, J^T r, sum r r, the number of valid pixels), formed and added as csrc/gn_sums.h states: one
 *      workgroup per (pose, tile of 1024 map pixels), 256 threads x 4 pixels, over a lane's pixels, over the wave by a butterfly, over
 *      the waves in order, and by a second launch over the tiles in order.  No atomics: a pose's 29 numbers are bit-identical from run
 *      to run, in any batch and at any index of it.  d_rows, when not null, (N,h,w,8) fp32 on the device, 16-byte aligned, gets
 *      (J0 .. J5, r, 1) per pixel and eight zeros where the pixel was skipped.  d_counts, when not null, (N,2) int32 on the device:
 *      the rendered and the observed pixels of each pose, exact (one pair per workgroup, added per pose by a small launch: no atomics).  h_sums, when not null, HOST (N,29): the call copies d_sums to it and
 *      SYNCHRONISES the stream.  When h_sums is null nothing synchronises and nothing is read on the host: the partial sums live in the
 *      context's arena (N tiles 232 bytes: 5.9 MB for 1024 maps of 160 x 160) and go back to it when the launches are queued, as the
 *      scratch of fp_render does - with the arena reserved beforehand (fp_ctx_reserve) the call can sit in a captured graph.  At most
 *      FP_POSE_ALIGN_MAX_POSES poses per call, maps of at most 2^24 pixels.
 *      Step.  fp_pose_gn_step is one thread per pose, on the device and in double: d_sums as above, d_poses (N,16) in and out, d_state
 *      N records of fp_pose_state (8-byte aligned; all-zero bytes are a fresh record).  Per pose, with s its 29 sums:
 *        nothing unless state.stopped == 0                                               a stopped pose is never touched again
 *        cnt = s[28].  Unless cnt >= min_pixels: stopped = FP_POSE_STOP_FEW_PIXELS; the pose goes back to prev_pose if steps > 0,
 *          otherwise prev_pose = pose, fit_count = cnt, fit_ms = s[27] / cnt (0 if cnt is 0)
 *        ms = s[27] / cnt.  If steps > 0 and ms > fit_ms: the pose goes back to prev_pose, stopped = FP_POSE_STOP_RESIDUAL_ROSE
 *          (mean squares are compared, not their roots)
 *        otherwise prev_pose = pose, fit_ms = ms, fit_count = cnt - the fit on record is always that of the pose the call returns -
 *          and, unless closing:
 *        A = the symmetric 6 x 6 of s[0 .. 20], b = s[21 .. 26];  lam = damping (((((A00 + A11) + A22) + A33) + A44) + A55)
 *        M = A with M_aa = A_aa + lam;  g_a = -b_a.  M = L D L^T without square roots, for j = 0 .. 5:
 *          d = M_jj, then for k = 0 .. j-1 in order d = d - (L_jk D_k) L_jk;  unless d > 0: stopped = FP_POSE_STOP_SINGULAR, the pose
 *          stays as it is;  D_j = d;  for a = j+1 .. 5: v = M_aj, then for k = 0 .. j-1 v = v - (L_ak D_k) L_jk;  L_aj = v / d
 *        z_a = g_a, then for k = 0 .. a-1 z_a = z_a - L_ak z_k                            (a = 0 .. 5)
 *        xi_a = z_a / D_a, then for k = a+1 .. 5 xi_a = xi_a - L_ka xi_k                  (a = 5 .. 0);   state.xi = xi = (tau, w)
 *        th = sqrt((w0 w0 + w1 w1) + w2 w2);  below 1e-4: ca = 1 - th th / 6, cb = 0.5 - th th / 24;  else ca = sin(th) / th,
 *          cb = (1 - cos(th)) / (th th);  Kx = [w];  K2_ab = (Kx_a0 Kx_0b + Kx_a1 Kx_1b) + Kx_a2 Kx_2b
 *        E_ab = ((a == b) + ca Kx_ab) + cb K2_ab;   R_ab <- (float)((E_a0 R_0b + E_a1 R_1b) + E_a2 R_2b);   t_a <- (float)(t_a + tau_a)
 *          with R, t the fp32 pose widened; the last row is left alone;  steps = steps + 1
 *      Nothing synchronises.  The host solve of the other aligners costs a synchronisation per iteration, which is wrong for 252
 *      hypotheses and impossible inside the hipGraph of a tracking frame.
 *      Loop.  fp_pose_polish enqueues iterations + 1 rounds on the stream: the crop windows of the poses (fp_crop_window_tf's launcher;
 *      crop = the maps' side, 0 = full-frame maps and no windows), fp_render's launcher for xyz and normals, the linearisation, the
 *      step - the first round starts every record of d_state afresh, whatever it held; the last has closing = 1.  No memset and no
 *      atomic is among the launches.  d_poses (N,16) in and out.  d_sums and d_counts are
 *      left as the last round wrote them (they are those of a pose that round may have taken back; the fit of the returned pose is in
 *      d_state).  It does not synchronise and reads nothing on the host; the maps, the partial sums and the rasteriser's scratch live in
 *      the arena as above.  It equals the same rounds issued through the public calls bit for bit.
 *      Defaults of the Python layer (Utils.polish_poses), this project's own choice, fixed by the experiment with the restatement on the
 *      CPU that DESIGN.md section 5 records: dist_max 0.010 m, cos_min 0.5, 8 iterations, damping 1e-9, min_pixels 100.
 *      Limits.  Geometry only: symmetric objects and flat faces slide along their free directions (state.xi and the sums show it; the
 *      damping only keeps the solve finite).  Projective association needs a start within dist_max of the surface.  Several map pixels
 *      can land on one observed pixel when the crop magnifies; each counts.  No occlusion reasoning beyond the two gates.  The fit
 *      numbers are reported, not judged.
 *      FP_EINVAL, each checked before ctx is looked into: a null ctx, d_xyz, d_normal, d_depth, d_normals, K, d_poses, d_sums (align);
 *      ctx, d_sums, d_poses, d_state (step); ctx, mesh, d_poses, K, d_depth, d_normals, d_state, d_sums (polish); a misaligned
 *      d_normals, d_rows or d_state; N < 0 or above the cap (0 writes nothing); h, w, H or W < 1; a non-finite K or fx or fy not > 0;
 *      dist_max not > 0; cos_min outside [-1, 1]; damping negative or not finite; min_pixels < 1; crop < 0; iterations outside
 *      0 .. FP_POSE_POLISH_MAX_ITERATIONS; with a crop, crop_ratio or mesh_diameter not > 0. */
#define FP_POSE_ALIGN_TERMS 29            /* doubles per pose of fp_pose_depth_align's d_sums */
#define FP_POSE_ALIGN_MAX_POSES 1024      /* per call of the three */
#define FP_POSE_POLISH_MAX_ITERATIONS 64
#define FP_POSE_STOP_FEW_PIXELS 1         /* fp_pose_state.stopped: too few valid pixels */
#define FP_POSE_STOP_RESIDUAL_ROSE 2      /* the mean square residual rose */
#define FP_POSE_STOP_SINGULAR 3           /* a pivot of the damped system was not > 0 */
typedef struct fp_pose_state {
  double fit_ms, fit_count;               /* mean square residual and valid pixels at prev_pose */
  double xi[6];                           /* the last step taken: (tau, w) */
  float prev_pose[16];                    /* the pose before the last step; the returned pose once stopped or closed */
  int32_t stopped;                        /* 0: active; else FP_POSE_STOP_* */
  int32_t steps;                          /* steps taken */
} fp_pose_state;
int fp_pose_depth_align(fp_ctx *ctx, const float *d_xyz, const float *d_normal, int N, int h, int w, const float *d_depth,
                        const float *d_normals, int H, int W, const double *K, const float *d_poses, float dist_max, float cos_min,
                        float *d_rows, double *d_sums, int32_t *d_counts, double *h_sums, void *stream);
int fp_pose_gn_step(fp_ctx *ctx, const double *d_sums, float *d_poses, fp_pose_state *d_state, int N, double damping, int min_pixels,
                    int closing, void *stream);
int fp_pose_polish(fp_ctx *ctx, const fp_mesh *mesh, float *d_poses, int N, const double *K, int H, int W, const float *d_depth,
                   const float *d_normals, int crop, double crop_ratio, double mesh_diameter, int iterations, float dist_max,
                   float cos_min, double damping, int min_pixels, fp_pose_state *d_state, double *d_sums, int32_t *d_counts,
                   void *stream);

/* ---- masks from depth: the objects standing on one supporting plane (csrc/segment.hip).  Find the plane (fp_plane_score over explicit
 *      three-pixel hypotheses, fp_plane_moments for the least-squares refit on the host), keep what stands above it, cut that into
 *      4-connected components (fp_depth_segment_count / _write).  Geometry only: no weights, no recognition; objects that touch without
 *      a depth step between them are one segment, and there is one plane.  The reference offers a mask-painting GUI instead
 *      (src/masking.py); this rule is the library's own.  tests/segment_oracle.py restates all of it in numpy.
 *      Everything is fp32, not contracted, every operation in the written order; / and sqrtf are correctly rounded.  d_depth
 *      (n_views,H,W) fp32 metres on the device, d_mask (n_views,H,W) uint8 or null, K (3,3) float64 HOST (fx, fy, cx, cy cast to fp32),
 *      one K and one size for all views, pixel index row W + col.  p(r,c) is the back-projection of fp_depth_normals:
 *        p = ((((float)col - cx) / fx) d, (((float)row - cy) / fy) d, d)
 *        ok(r,c): d >= 0.001 and d < zfar and, with a mask, mask != 0
 *      0 < zfar <= 1000 in all four calls, and at most FP_SEGMENT_MAX_PIXELS pixels (n_views H W) a call.  A view's results are
 *      bit-identical in any batch and at any index of it, and from run to run: counts and statistics are integer atomics, the moments
 *      are summed in a fixed order, nothing is a float atomic.
 *      Planes are (n.x, n.y, n.z, dd) with the camera (the origin) on the positive side: (n . p) + dd is the height of p above the plane.
 *      (a) fp_plane_score.  triplets (n_views,n_hyp,3) int32 HOST pixel indices, 0 <= n_hyp <= FP_PLANE_MAX_HYP.  Per view and
 *      hypothesis (i, j, k):
 *        count 0 and plane (0,0,0,0) unless i, j, k are in 0 .. H W - 1, pairwise different and ok
 *        u = p_j - p_i,  w = p_k - p_i;   m = u x w = (u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x)
 *        l2 = (m.x m.x + m.y m.y) + m.z m.z;   count 0 and plane (0,0,0,0) unless l2 > 0
 *        l = sqrtf(l2);  n = (m.x / l, m.y / l, m.z / l);   dd = -((n.x p_i.x + n.y p_i.y) + n.z p_i.z)
 *        if dd < 0: n = -n, dd = -dd
 *        count = the number of ok pixels with fabsf(((n.x p.x + n.y p.y) + n.z p.z) + dd) < tol, int32
 *      h_planes (n_views,n_hyp,4) fp32, h_counts (n_views,n_hyp) int32 and h_best (n_views) int32 are HOST arrays: h_best is the
 *      hypothesis with the largest count, the lowest index among equals, -1 when every count is 0 (or n_hyp is 0).  SYNCHRONISES.
 *      (b) fp_plane_moments.  planes (n_views,4) float64 HOST, cast to fp32.  h_sums (n_views, FP_PLANE_MOMENT_TERMS) float64 HOST:
 *      n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz over the ok pixels with fabsf(((n.x p.x + n.y p.y) + n.z p.z) + dd) < tol; x, y, z
 *      widened to double before the products; any other pixel adds +0.0 to every term.  Summation order (that of csrc/gn_sums.h): a
 *      workgroup of 256 threads owns a tile of 1024 pixels of one view (pixels past the view's last one add +0.0); lane tid adds pixels
 *      tile 1024 + q 256 + tid, q = 0 .. 3 in that order, from +0.0; over the 64 lanes of a wave a butterfly, partner distance 32, 16,
 *      .. 1, s = s + s[lane ^ o]; the four waves in order, red[0] + red[1] + ..; the tiles in order from 0.0.  SYNCHRONISES.
 *      (c) fp_depth_segment_count / fp_depth_segment_write, count-then-write as fp_mesh_components_*.  planes as in (b).  Per pixel:
 *        h = ((n.x p.x + n.y p.y) + n.z p.z) + dd;   foreground: ok and h >= h_min and h <= h_max
 *        two 4-neighbours a, b are joined when both are foreground and fabsf(d_a - d_b) <= max_jump (the gate of fp_depth_normals)
 *      A component is kept when it has at least min_pixels pixels; the kept components of a view are numbered 1, 2, .. by their lowest
 *      pixel index.  fp_depth_segment_count builds the decomposition in an allocation owned by the context (24 bytes a pixel, kept
 *      until a larger batch arrives or the context is destroyed), SYNCHRONISES and returns h_counts (n_views,2) int32 HOST: components,
 *      kept components.  The caller allocates d_labels (n_views,H,W) int32 and d_stats (sum of kept, FP_SEGMENT_STATS) int64 (may be
 *      null when nothing is kept) and calls fp_depth_segment_write with the SAME d_depth, n_views, H, W and n_kept = the sum of the kept
 *      counts; it queues its kernels and does not synchronise.  d_labels: the component's number where it is kept, else 0.  d_stats: the
 *      kept components of view 0 in label order, then those of view 1, ..; with q(x) = (long long)rintf(min(max(x 1048576.f, -2^34),
 *      2^34)), i.e. 2^-20 m fixed point (the clamp is never met by a camera with |col - cx| / fx of ordinary size: 2^34 is 16 km), a row is
 *        0 pixels;  1 rmin, 2 rmax, 3 cmin, 4 cmax;  5-7 sum of q(p.x), q(p.y), q(p.z);  8-10 min of the same;  11-13 max of the same;
 *        14 max of q(h);  15 the lowest pixel index
 *      How: the lock-free union-find of fp_mesh_components_count over the pixels - roots only decrease, hooks are by compare-and-swap,
 *      one flatten pass - started from the horizontal runs inside each wave; no kernel waits for another workgroup.
 *      FP_EINVAL, each checked before ctx is looked into (count, score, moments): a null ctx, d_depth, K, planes or host output; H or
 *      W < 1; n_views outside 0 .. FP_TSDF_MAX_VIEWS (0 writes nothing); more than FP_SEGMENT_MAX_PIXELS pixels; a non-finite K, or fx
 *      or fy not > 0; zfar outside (0, 1000]; tol or max_jump not > 0; h_max < h_min; min_pixels < 1; n_hyp outside 0 ..
 *      FP_PLANE_MAX_HYP, or null triplets, h_planes or h_counts with n_hyp > 0; a plane that is not finite or has a zero normal (as
 *      fp32); for write: no count before it on this context, other maps (d_depth, n_views, H, W) than the last count had, n_kept other
 *      than its sum, a null d_labels.  FP_ENOMEM: the state does not fit the device. */
#define FP_PLANE_MAX_HYP 1024          /* hypotheses per view of fp_plane_score */
#define FP_PLANE_MOMENT_TERMS 10       /* doubles per view of fp_plane_moments' h_sums */
#define FP_SEGMENT_STATS 16            /* int64 per kept component of fp_depth_segment_write's d_stats */
#define FP_SEGMENT_MAX_PIXELS (1 << 28) /* n_views H W of one call */
int fp_plane_score(fp_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int n_views, int H, int W, const double *K, float zfar,
                   const int32_t *triplets, int n_hyp, float tol, float *h_planes, int32_t *h_counts, int32_t *h_best, void *stream);
int fp_plane_moments(fp_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int n_views, int H, int W, const double *K, float zfar,
                     const double *planes, float tol, double *h_sums, void *stream);
int fp_depth_segment_count(fp_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int n_views, int H, int W, const double *K, float zfar,
                           const double *planes, float h_min, float h_max, float max_jump, int min_pixels, int32_t *h_counts, void *stream);
int fp_depth_segment_write(fp_ctx *ctx, const float *d_depth, int n_views, int H, int W, int32_t *d_labels, int64_t *d_stats, int64_t n_kept,
                           void *stream);

/* ---- depth from a rectified stereo pair: semi-global matching on census costs (csrc/stereo.hip).  The reference loads a depth image
 *      that its camera vendor's SDK computed (src/file_processing.py:99-138); this rule is the library's own, NOT
 *      OpenCV's StereoSGBM, and tests/stereo_oracle.py restates all of it in numpy.  The arithmetic is integer from the images to the
 *      winning disparity: every stage is bit-identical from run to run, in any batch and at any index of it.  The pair must already be
 *      rectified and undistorted: a point of left pixel (y, x) is looked for at right pixels (y, x - d), 0 <= d < D = max_disparity.
 *      d_left, d_right (n,H,W) uint8 with channels = 1, (n,H,W,3) uint8 RGB with channels = 3, on the device; n >= 1 pairs of one size,
 *      H, W >= 1; D a multiple of 64, 64 .. FP_STEREO_MAX_DISPARITY; n H W D <= FP_STEREO_MAX_CELLS and n <= 65535.
 *      1 Grey.  One channel is used as given; RGB becomes (77 R + 150 G + 29 B + 128) >> 8.
 *      2 Census, 9 wide x 7 high.  The 62 neighbours dy = -3 .. 3, dx = -4 .. 4 without the centre, scanned row-major (dy outer), the
 *        first neighbour in bit 61 of a uint64, the last in bit 0; coordinates clamped to the image; a bit is set when the neighbour is
 *        smaller than the centre.
 *      3 Cost.  C(y,x,d) = popcount(cl(y,x) ^ cr(y,x-d)) where x - d >= 0, else 64 (one above anything a comparison can give).
 *      4 Paths.  Bit b of `paths` selects the direction r = (dy, dx): 0 (0,+1), 1 (0,-1), 2 (+1,0), 3 (-1,0), 4 (+1,+1), 5 (+1,-1),
 *        6 (-1,+1), 7 (-1,-1) (this numbering is pinned here); 0xFF is all eight, 0x0F the four axis-aligned ones.  With q = p - r and
 *        m_q = min_k L_r(q,k):
 *          L_r(p,d) = C(p,d) + min(L_r(q,d), L_r(q,d-1) + P1, L_r(q,d+1) + P1, m_q + P2) - m_q
 *        L_r = C where q lies outside the image; d - 1 < 0 and d + 1 >= D are not considered.  L_r <= 64 + P2.  S = the sum of the
 *        selected L_r, uint16.  P1 and P2 are constants (no gradient-adaptive P2); the defaults 8 and 32 are this library's own choice.
 *      5 Winner.  d*(p) = the lowest d at which S(p, .) is minimal.
 *      6 Left-right check.  d_R(y,x) = the lowest d minimising S(y,x+d,d) over x + d < W.  A pixel is valid when x - d* >= 0 and
 *        |d_R(y,x-d*) - d*| <= lr_max and d* >= min_disparity; lr_max < 0 switches the middle test off.
 *      7 Sub-pixel (subpixel = 1).  With 0 < d* < D - 1, a, b, c = S(d*-1), S(d*), S(d*+1) as int and a - 2b + c > 0:
 *        disparity = (float)d* + (float)(a - c) / (float)(2 (a - 2b + c)), fp32, / correctly rounded; in every other case (float)d*.
 *      8 Outputs, either may be null.  d_disparity (n,H,W) fp32, -1 where the pixel is not valid.  d_depth (n,H,W) fp32 =
 *        fb / disparity with fb = (float)(fx * baseline), the product formed in double; 0 where the pixel is not valid, where the depth
 *        is above zfar (infinity: no limit) and where the disparity is not > 0 (possible only with min_disparity = 0; pinned here).
 *      dbg (may be null): device pointers, each may be null, that receive the stages: d_census_left / d_census_right (n,H,W) uint64,
 *      d_cost (n,H,W,D) uint8, d_sum (n,H,W,D) uint16, d_dstar / d_dright (n,H,W) int32.  C is formed only for this output: the
 *      aggregation computes its costs from the census images.
 *      Working memory is one allocation owned by the context (16 + 2 D bytes a pixel, + 2 with RGB; kept until a larger call arrives or
 *      the context is destroyed); a call writes everything it reads.  The call queues one chain of launches on `stream` and does not
 *      synchronise; after a first call of a size, a call of that size allocates nothing and can be captured into a graph.
 *      FP_EINVAL, each checked before ctx is looked into: a null ctx, d_left, d_right or opts; a struct_size the library does not know;
 *      n, H or W < 1; channels other than 1 or 3; max_disparity as above; too many cells; p1 < 0, p1 > p2 or 8 (64 + p2) > 65535;
 *      paths outside 1 .. 0xFF; min_disparity outside 0 .. D - 1; subpixel other than 0 or 1; with d_depth: fx baseline not positive
 *      and finite as fp32, zfar not > 0.  FP_ENOMEM: the working memory does not fit the device. */
#define FP_STEREO_MAX_DISPARITY 256
#define FP_STEREO_MAX_CELLS (1LL << 31) /* n H W max_disparity of one call */
typedef struct fp_stereo_opts {
  size_t struct_size;      /* = sizeof(fp_stereo_opts) */
  int max_disparity;       /* D */
  int p1, p2;
  unsigned paths;          /* one bit per direction */
  int lr_max;              /* < 0: no left-right check */
  int min_disparity;
  int subpixel;            /* 0 or 1 */
  double fx, baseline;     /* pixels, metres; read only with d_depth */
  float zfar;              /* metres; read only with d_depth */
} fp_stereo_opts;
typedef struct fp_stereo_debug {
  size_t struct_size;      /* = sizeof(fp_stereo_debug) */
  uint64_t *d_census_left, *d_census_right;
  uint8_t *d_cost;
  uint16_t *d_sum;
  int32_t *d_dstar, *d_dright;
} fp_stereo_debug;
int fp_stereo_sgm(fp_ctx *ctx, const uint8_t *d_left, const uint8_t *d_right, int n, int H, int W, int channels, const fp_stereo_opts *opts,
                  float *d_disparity, float *d_depth, const fp_stereo_debug *dbg, void *stream);

/* ---- warping images and depth maps through a camera model: undistortion and stereo rectification (csrc/rectify.hip), the stage in
 *      front of fp_stereo_sgm on a raw stereo pair and in front of every depth toolkit on a camera with lens distortion.  The reference
 *      has nothing in this place (its camera vendor's SDK delivers rectified images); the rule is the library's own (DESIGN.md section
 *      5), NOT OpenCV's remap, and tests/rectify_oracle.py restates all of it in numpy.  The plans are built on the host in float64
 *      (foundationpose_amd/rectify.py) and rounded to fp32 once.  The map is computed per pixel, no map is read from memory.
 *      A plan (fp_remap_plan) says for one image: k_new = fx, fy, cx, cy of the new (ideal pinhole) camera; rot = the rotation from the
 *      new frame to the raw frame, row-major; k_raw = fx, fy, cx, cy of the raw camera; dist = k1 k2 p1 p2 k3 k4 k5 k6 (OpenCV's order);
 *      r2_max (infinity: no limit); the size of the source (raw) and of the destination (new) image.
 *      1 Map, per destination pixel (col, row), fp32, each operation rounded once, in this order and with these parentheses:
 *          x = (col - cx_new) / fx_new, y = (row - cy_new) / fy_new                      (pinhole_ray_x / _y of csrc/view_geom.h)
 *          X = (rot[0] x + rot[1] y) + rot[2], Y = (rot[3] x + rot[4] y) + rot[5], Z = (rot[6] x + rot[7] y) + rot[8]   (mat3_row, z = 1)
 *          the pixel is invalid unless Z > 0;  xr = X / Z, yr = Y / Z;  r2 = xr xr + yr yr;  the pixel is invalid unless r2 < r2_max
 *          radial = (1 + r2 (k1 + r2 (k2 + r2 k3))) / (1 + r2 (k4 + r2 (k5 + r2 k6)))
 *          xy2 = 2 (xr yr)
 *          xd = (xr radial + p1 xy2) + p2 (r2 + 2 (xr xr)),  yd = (yr radial + p1 (r2 + 2 (yr yr))) + p2 xy2
 *          u = fx_raw xd + cx_raw,  v = fy_raw yd + cy_raw
 *      2 Colour mode (FP_REMAP_COLOUR): uint8, channels 1 or 3, bilinear with 1/256-pixel weights, integer from here on.
 *          fu = floor(u 256 + 0.5), fv = floor(v 256 + 0.5) in fp32; the pixel is valid when 0 <= fu <= 256 (W_src - 1) and
 *          0 <= fv <= 256 (H_src - 1), decided in float, so that a NaN or a huge value never reaches a cast: exactly the pixels whose
 *          taps of non-zero weight lie inside the source.  qu = (int)fu, u0 = qu >> 8, a = qu & 255, likewise qv, v0, b;
 *          out = ((256-a)(256-b) p(v0,u0) + a (256-b) p(v0,u0+1) + (256-a) b p(v0+1,u0) + a b p(v0+1,u0+1) + 32768) >> 16 per
 *          channel (a tap of weight 0 is not read outside the source).  Invalid pixels are 0 in every channel.  An identity plan
 *          (rot = 1, k_new = k_raw, dist = 0, equal sizes) reproduces its input on every pixel.
 *      3 Depth mode (FP_REMAP_DEPTH): float32 metres, channels = 1, the NEAREST source pixel cf = floor(u + 0.5), rf = floor(v + 0.5),
 *          valid when 0 <= cf <= W_src - 1 and 0 <= rf <= H_src - 1, decided in float.  out = d / Z with d the source depth and Z of
 *          step 1 (the depth along the new optical axis of the point at depth d along the raw one); 0 where the pixel is invalid or d
 *          is not a depth (d >= 0.001 and d < zfar fails, a NaN too).  Depth is never blended across an edge; with rot = 1, Z is
 *          exactly 1 and the depth is copied bit for bit.
 *      Batching: n images of one source size and one destination size, n_plans = 1 or 2, image i uses plan i mod n_plans.  With
 *      n_plans = 1 all images lie in d_src0 / d_dst0.  With n_plans = 2 (a stereo pair, or n / 2 pairs) the images of plan 0 lie in
 *      d_src0 (n / 2, H_src, W_src[, 3]) and those of plan 1 in d_src1, likewise d_dst0 / d_dst1: left and right are two device pointers
 *      and one launch, without a staging copy.  Optional outputs: d_valid0 / d_valid1 (.., H_dst, W_dst) uint8, 1 where the pixel is valid
 *      in the sense of step 2 or 3 (in depth mode whatever the source depth); dbg->d_map0 / d_map1 (.., H_dst, W_dst, 2) fp32, the (u, v)
 *      of step 1, both the quiet NaN 0x7fc00000 where step 1 declared the pixel invalid.
 *      One launch on `stream`, the plans travel as kernel arguments; no allocation, no synchronisation, no atomics: the call can be
 *      captured into a graph at once.
 *      FP_EINVAL, each checked before ctx is looked into: a null ctx, opts, d_src0 or d_dst0 (with n_plans = 2 also d_src1, d_dst1); a
 *      struct_size the library does not know; mode other than the two; channels other than 1 or 3 (depth: 1); n_plans other than 1 or
 *      2; n < 1 or no multiple of n_plans; a size < 1 or > FP_REMAP_MAX_SIDE; plans of different sizes; a plan value that is not finite
 *      (r2_max: not > 0), fx or fy not > 0; in depth mode zfar not > 0. */
#define FP_REMAP_COLOUR 0
#define FP_REMAP_DEPTH 1
#define FP_REMAP_MAX_SIDE 16384
typedef struct fp_remap_plan {
  float k_new[4];          /* fx, fy, cx, cy of the new camera */
  float rot[9];            /* new frame -> raw frame, row-major */
  float k_raw[4];          /* fx, fy, cx, cy of the raw camera */
  float dist[8];           /* k1 k2 p1 p2 k3 k4 k5 k6 */
  float r2_max;            /* rays with r2 >= r2_max are refused; infinity: none */
  int src_h, src_w, dst_h, dst_w;
} fp_remap_plan;
typedef struct fp_remap_opts {
  size_t struct_size;      /* = sizeof(fp_remap_opts) */
  int mode;                /* FP_REMAP_COLOUR or FP_REMAP_DEPTH */
  int channels;            /* 1 or 3 */
  int n_plans;             /* 1 or 2 */
  float zfar;              /* metres; read only in depth mode (infinity: no limit) */
  fp_remap_plan plan[2];
} fp_remap_opts;
typedef struct fp_remap_debug {
  size_t struct_size;      /* = sizeof(fp_remap_debug) */
  float *d_map0, *d_map1;
} fp_remap_debug;
int fp_remap(fp_ctx *ctx, const void *d_src0, const void *d_src1, int n, const fp_remap_opts *opts, void *d_dst0, void *d_dst1, uint8_t *d_valid0,
             uint8_t *d_valid1, const fp_remap_debug *dbg, void *stream);

/* ---- registering depth into another camera: the depth maps of V calibrated pinhole cameras reprojected into ONE target pinhole camera
 *      of another size, with a z-buffer (csrc/reproject.hip).  The stage between fp_remap and fp_depth_prefilter on an RGB-D sensor whose
 *      depth and colour come from two sensors (V = 1, the target is the colour camera), and the merge of a rig of depth cameras into one
 *      view (V > 1).  The reference has nothing in this place (its camera vendor's SDK delivers depth aligned to colour); the rule is the
 *      library's own and tests/depth_reproject_oracle.py restates all of it in numpy.  Lens distortion is not seen
 *      here: fp_remap removes it on either side.
 *      d_depth (n, V, Hs, Ws) fp32 metres: n frames of V views of one size.  Ks (V, 3, 3) and K_dst (3, 3) are host double camera
 *      matrices, T_dst_src (V, 4, 4) host double rigid transforms, row-major, from the frame of source camera s to the target frame
 *      (x_dst = R x_src + t; the last row is not used).  They are the same for every frame, are rounded to fp32 once (pinhole_of /
 *      rigid_of of csrc/view_geom.h) and travel as kernel arguments.
 *      The rule, fp32, each operation rounded once, in this order, with the functions of csrc/view_geom.h.  For view s, source pixel
 *      (c, r) with depth d:
 *        1 Source.  The pixel is skipped unless depth_ok(d, zfar): d >= 0.001 and d < zfar (a NaN fails).
 *        2 Centre.  p = pinhole_point(cam_s, c, r, d); q = (rigid_apply(T_s, 0, p), rigid_apply(T_s, 1, p), rigid_apply(T_s, 2, p)).
 *          Skipped unless depth_ok(q.z, zfar).  z_out = q.z.
 *        3 Footprint.  The corners pinhole_point(cam_s, c - 0.5, r - 0.5, d) and pinhole_point(cam_s, c + 0.5, r + 0.5, d) go through
 *          T_s the same way: q0, q1.  Skipped unless q0.z > 0 and q1.z > 0.  (uc, vc), (u0, v0), (u1, v1) = project_ratio(dst, .) of q,
 *          q0, q1.  Skipped unless all six are finite.
 *        4 Range.  xa = ceil(min(u0, u1)), xb = ceil(max(u0, u1)) - 1, pc = floor(uc + 0.5); x_lo = min(xa, pc), x_hi = max(xb, pc);
 *          likewise y_lo, y_hi, pr from the v: the target pixels whose centres lie in the source pixel's footprint [min, max), and always
 *          the centre's own pixel (pc, pr).  All in float; skipped unless the four values are finite, so nothing huge reaches a cast.
 *        5 Cap.  If (x_hi - x_lo) + 1 or (y_hi - y_lo) + 1 exceeds FP_REPROJECT_MAX_SPLAT, the range is (pc, pr) alone: a grazing
 *          surface or an absurd magnification.
 *        6 Clip.  x_lo = max(x_lo, 0), x_hi = min(x_hi, Wd - 1), likewise y with Hd; an empty range writes nothing.
 *        7 Write.  Every target pixel of the range takes the minimum of its 64-bit key and (bits of z_out << 32 | (s Hs + r) Ws + c):
 *          z_out is positive, so the order of its bits is the order of its value.  The nearest surface wins, among equal depths the
 *          lowest source index; the result does not depend on the order of the threads and is the same on every run and in any batch.
 *      d_depth_out (n, Hd, Wd) fp32: z_out of the winner, 0 where nothing arrived.  d_source (n, Hd, Wd) int32, optional: the winner's
 *      index (s Hs + r) Ws + c within its frame, -1 where nothing arrived.  With one view, cam_s = dst and T = 1 of one size every
 *      depth is copied bit for bit onto its own pixel.
 *      d_keys: n Hd Wd uint64 of working memory from the caller, 8-byte aligned; its contents before the call do not matter and are
 *      undefined after it.  One memset node and two launches on `stream`; no allocation, no synchronisation: the call can be captured
 *      into a graph at once.
 *      Depth is piecewise constant over a source pixel: nearest neighbour, nothing is interpolated across an edge.  A background can
 *      show through a foreground at the foreground's rim and where the magnification exceeds the cap; what no source sees stays 0.
 *      FP_EINVAL, each checked before ctx is looked into: a null ctx, d_depth, Ks, T_dst_src, K_dst, d_keys or d_depth_out; n outside
 *      1 .. FP_REPROJECT_MAX_FRAMES; V outside 1 .. FP_REPROJECT_MAX_VIEWS; a side < 1 or > FP_REMAP_MAX_SIDE; V Hs Ws > 2^31 - 1; an
 *      entry of a K or a T that is not finite (as a double or rounded to fp32); fx or fy not > 0; zfar not > 0 (infinity: no limit);
 *      d_keys not 8-byte aligned. */
#define FP_REPROJECT_MAX_VIEWS 8
#define FP_REPROJECT_MAX_SPLAT 8
#define FP_REPROJECT_MAX_FRAMES 65535
int fp_depth_reproject(fp_ctx *ctx, const float *d_depth, int n, int V, int Hs, int Ws, const double *Ks, const double *T_dst_src, const double *K_dst,
                       int Hd, int Wd, float zfar, uint64_t *d_keys, float *d_depth_out, int32_t *d_source, void *stream);

/* ---- finding an object in a depth frame without a mask: depth templates of the model matched at every pixel of an anchor lattice
 *      (csrc/detect.hip).  What register() needs in place of a mask is a centre (x, y, z); this gives a few, each with a rough rotation.
 *      The reference has nothing in this place (a person paints the mask); the rule is the library's own and
 *      tests/detect_oracle.py restates all of it in numpy.  Geometry only, nothing learned.
 *      d_depth (n_frames, H, W) fp32 metres.  K: host double 3x3; fx, fy, cx, cy are rounded to fp32 once (pinhole_of of csrc/view_geom.h).
 *      d_table (T, n_in + n_out, 4) fp32, 16-byte aligned: per template its n_in in-samples, then its n_out out-samples, each the offset
 *      (x, y, z, 0) in metres, camera axes, of a point from the object's centre: in-samples lie on the model's surface inside the
 *      silhouette, out-samples just outside the silhouette at the depth of its rim; the first `anchors` in-samples are the anchors
 *      (foundationpose_amd/detect.py builds the table).  ranges: host int32 (n_obj + 1), ranges[0] = 0, ascending: object o owns the
 *      templates ranges[o] .. ranges[o + 1] - 1, T = ranges[n_obj].
 *      The anchor lattice: pixel (r, c) = (r0 + i stride, c0 + j stride), i < Hs = ceil((H - r0) / stride), j < Ws = ceil((W - c0) / stride).
 *      The rule, fp32, each operation rounded once, in this order, / correctly rounded, every comparison written so that a NaN fails it.
 *      Per frame, object, anchor pixel (r, c), template t of the object's range (t_local = t - ranges[o]) and anchor a < anchors:
 *        d = D[r, c];                 no candidate unless d >= 0.001 and d < zfar
 *        A = in-sample a of t;        zc = d - A.z;      no candidate unless z_min <= zc and zc <= z_max
 *        Cx = ((((float)c - cx) / fx) * d) - A.x;        Cy = ((((float)r - cy) / fy) * d) - A.y
 *        per sample S:  X = Cx + S.x, Y = Cy + S.y, Z = zc + S.z;      the sample fails unless Z >= 0.001
 *                       u = (fx X) / Z + cx, v = (fy Y) / Z + cy;  cf = floorf(u + 0.5f), rf = floorf(v + 0.5f)      (project_icp)
 *                       the sample fails unless 0 <= cf <= W - 1 and 0 <= rf <= H - 1, compared as floats;      o = D[rf, cf]
 *           an in-sample passes when   o >= 0.001 and |o - Z| <= tol_in
 *           an out-sample passes when  not (o >= 0.001), or |o - Z| > tol_out      (no reading, or a depth step at the silhouette)
 *        score = n_in_pass * n_out_pass      the product: a plane fits every in-sample and no out-sample, free space the reverse
 *        key   = (score << 16) | (0xFFFF - (4 t_local + a))
 *      d_keys (n_frames, n_obj, Hs, Ws) uint32: the maximum key over the object's candidates at that anchor pixel - among equal scores
 *      the lowest (t, a) -, 0 where there is no candidate.  d_counts, optional, same shape: n_in_pass << 16 | n_out_pass of the winner, 0
 *      where there is none.  The centre of a candidate is (Cx, Cy, zc); foundationpose_amd/detect.py recomputes it in double.
 *      One thread owns an anchor pixel and carries the maximum in a register: no atomics, no allocation, no synchronisation, one launch
 *      that can be captured into a graph; a frame's map has the same bits in any batch and on every run.  Candidates that can no longer
 *      reach the maximum are left early; that prune is exact.  n_frames = 0 does nothing; T = 0 zeroes the maps.
 *      FP_EINVAL, each checked before ctx is looked into: a null ctx, d_depth, K, d_table, ranges or d_keys; n_frames outside 0 ..
 *      FP_TEMPLATE_MAX_FRAMES; H or W < 1 or > FP_REMAP_MAX_SIDE; stride < 1; r0 outside 0 .. H - 1 or c0 outside 0 .. W - 1; tol_in or
 *      tol_out not > 0; z_min > z_max (or a NaN); zfar not > 0; an entry of K that is not finite, fx or fy not > 0; n_in or n_out < 1,
 *      n_in n_out > 65535, n_in + n_out > FP_TEMPLATE_MAX_SAMPLES; anchors outside 1 .. FP_TEMPLATE_MAX_ANCHORS or > n_in; n_obj outside
 *      1 .. FP_TEMPLATE_MAX_OBJECTS; ranges[0] != 0, descending ranges, an object with more than 16384 templates (4 T <= 65536); d_table
 *      not 16-byte aligned.
 *      fp_template_match_info: *chunk_templates = the number of templates of n_samples = n_in + n_out samples each that the kernel stages
 *      at once (a host function; the tests put template counts around its multiples). */
#define FP_TEMPLATE_MAX_OBJECTS 64
#define FP_TEMPLATE_MAX_SAMPLES 1024
#define FP_TEMPLATE_MAX_ANCHORS 4
#define FP_TEMPLATE_MAX_FRAMES 65535
int fp_template_match(fp_ctx *ctx, const float *d_depth, int n_frames, int H, int W, const double *K, const float *d_table, const int32_t *ranges,
                      int n_obj, int n_in, int n_out, int anchors, int stride, int r0, int c0, float z_min, float z_max, float zfar, float tol_in,
                      float tol_out, uint32_t *d_keys, uint32_t *d_counts, void *stream);
int fp_template_match_info(int n_samples, int *chunk_templates);

/* ---- texture baking: the colours of posed RGB-D reference views gathered into a per-face texture atlas of a mesh - the last stage of
 *      the model-free set-up, after the simplification (fp_mesh_simplify_* refuses textured meshes: simplify first, then bake).  The
 *      reference does this in mesh_texture_from_train_images (bundlesdf/nerf_runner.py:1122) with a UV parametrisation and the equal
 *      mean of each triangle's best 4 views; the atlas and the weighting below are this library's own.
 *      Deterministic: one thread per texel, the views in index order inside it, no atomics; nothing synchronises.  Everything is fp32,
 *      not contracted, every operation in the written order; / and sqrt are correctly rounded (tests/texture_bake_oracle.py restates
 *      the rule in numpy).
 *      Atlas.  T = tex_size, a power of two, FP_TEXTURE_MIN_SIZE .. FP_TEXTURE_MAX_SIZE.  g = the smallest integer with g g >=
 *      ceil(F / 2); cells of c x c texels, c = floor(T / g), in row-major order: cell k has its first texel at column (k mod g) c, row
 *      floor(k / g) c, and holds face 2k (A) and face 2k + 1 (B).  c < 4 is refused.  With m = c - 3 and (i, j) = (column, row) of a
 *      texel inside its cell, A has its corners 0, 1, 2 at (0,0), (m,0), (0,m) and owns the texels with i + j <= c - 2; B has them at
 *      (c-1,c-1), (c-1-m,c-1), (c-1,c-1-m) and owns those with i + j >= c.  The anti-diagonal i + j = c - 1, the B half of a last odd
 *      cell and every texel outside the g x g cells belong to no face: colour 0, used -1.
 *      uv.  Face f has its own entries 3f, 3f + 1, 3f + 2 of d_uv (the uv_idx of fp_mesh_create is 0, 1, .. 3F - 1; the vertex count
 *      does not change), at the texel CENTRES of its corners: (((float)column + 0.5) / (float)T, ((float)row + 0.5) / (float)T) with
 *      atlas columns and rows, in the rasteriser's convention ("v already flipped" for fp_mesh_create): v T - 0.5 is the texture row,
 *      rows top-down.  Both values and 1 - v are exact in fp32, so the v -> 1 - v of an OBJ file or of make_mesh_tensors round-trips bit
 *      for bit.  Consequence: for a uv inside a face's uv triangle the rasteriser's bilinear fetch (x = u T - 0.5, floor, + 1) gives
 *      non-zero weight to texels of that face alone - on an edge of the triangle the far neighbour's weight is exactly 0 - so nothing
 *      bleeds between faces or wraps at the atlas border.  (The rasteriser interpolates uv itself in fp32; its rounding can put a uv a
 *      few ulp outside, where a foreign texel's weight is of that order: below 1e-5 of a colour step.)
 *      Point of an owned texel.  For A b1 = (float)i / (float)m, b2 = (float)j / (float)m; for B b1 = (float)(c-1-i) / (float)m,
 *      b2 = (float)(c-1-j) / (float)m; b0 = (1 - b1) - b2.  If b0 < 0 (a ring texel beyond the hypotenuse): s = b1 + b2, b0 = 0,
 *      b1 = b1 / s, b2 = b2 / s - the nearest edge region.  With P0, P1, P2 the face's vertices in its index order:
 *      p = (b0 P0 + b1 P1) + b2 P2 per component.  Normal: e = P1 - P0, h = P2 - P0, n = (e.y h.z - e.z h.y, e.z h.x - e.x h.z,
 *      e.x h.y - e.y h.x), divided by sqrt((n.x n.x + n.y n.y) + n.z n.z) (a degenerate face gives NaN: every view skips).
 *      Views.  d_rgb (n_views,H,W,3) uint8, d_depth (n_views,H,W) fp32 metres, d_mask (n_views,H,W) uint8 or null, K and cam_in_ob as
 *      for fp_tsdf_integrate (R, t: the float64 inverse cast to fp32).  Per view, in index order:
 *        q_a = ((R[a][0] p.x + R[a][1] p.y) + R[a][2] p.z) + t[a];                    skip the view unless q.z >= 0.001
 *        x = fx (q.x / q.z) + cx, y = fy (q.y / q.z) + cy (pixel centres at integers);  x0 = floor(x), y0 = floor(y)
 *        skip unless 0 <= x0 < W - 1 and 0 <= y0 < H - 1                                (the bilinear footprint lies inside the image)
 *        d = depth[floor(y + 0.5), floor(x + 0.5)];  skip unless d >= 0.001 and d < zfar, and, with a mask, mask there != 0
 *        skip unless |d - q.z| <= depth_tol                                             (occluded, or not on the observed surface)
 *        o_i = -((R[0][i] t[0] + R[1][i] t[1]) + R[2][i] t[2])                          (the camera centre, from the fp32 R, t)
 *        w = o - p;  cosang = ((n.x w.x + n.y w.y) + n.z w.z) / sqrt((w.x w.x + w.y w.y) + w.z w.z);   skip unless cosang >= cos_min
 *        sample, per channel: t00 = rgb[y0, x0], t10 = rgb[y0, x0 + 1], t01 = rgb[y0 + 1, x0], t11 = rgb[y0 + 1, x0 + 1] as float,
 *        wx = x - x0, wy = y - y0, ta = t00 + wx (t10 - t00), tb = t01 + wx (t11 - t01), colour = ta + wy (tb - ta)
 *      ("unless" so that a NaN skips.)  The top_n views with the largest cosang are kept, ordered by cosang descending; among equal
 *      values the lower view index comes first and wins the last place.  used = the number kept.  With used > 0:
 *      sw = sum of cosang, sc = sum of cosang colour, both added in that order starting from 0; the texel is sc / sw.  With used = 0:
 *      (b0 C0 + b1 C1) + b2 C2 of the face's vertex colours as float, or 128 without vertex colours.  Each channel is stored as
 *      floor(value + 0.5) clamped to 0 .. 255.
 *      Outputs, device: d_texture (T,T,3) uint8, rows top-down; d_uv (3F,2) fp32; d_used (T,T) int8 or null.  n_views = 0 bakes the
 *      vertex colours alone.  A face index outside 0 .. V-1 is found on the device and never followed: the face's texels are 128 with
 *      used 0, and no error is reported (the call does not synchronise).
 *      FP_EINVAL: a null ctx, d_pos, d_faces, K, cfg, d_texture or d_uv; null d_rgb, d_depth or cam_in_ob with n_views > 0; a
 *      struct_size the library does not know; V or F < 1, F above FP_TEXTURE_MAX_FACES; tex_size not a power of two in range; c < 4
 *      (the message names the tex_size that fits); top_n outside 1 .. FP_TEXTURE_MAX_TOP_N; n_views outside 0 .. FP_TSDF_MAX_VIEWS (the
 *      view matrices travel as kernel arguments); H or W < 2 with views; depth_tol < 0, cos_min outside (0, 1], zfar not > 0 (infinity
 *      is allowed), or one of them NaN; fx or fy not > 0; a view matrix that is not finite or whose last row is not 0 0 0 1.  All of
 *      it is checked on the host before anything is queued. */
#define FP_TEXTURE_MIN_SIZE 64
#define FP_TEXTURE_MAX_SIZE 4096
#define FP_TEXTURE_MAX_TOP_N 4         /* the reference's _CHOOSE_TOP_N */
#define FP_TEXTURE_MAX_FACES (1 << 21) /* 1024 x 1024 cells of 4 texels at tex_size 4096 */
typedef struct fp_texture_cfg {
  size_t struct_size;      /* = sizeof(fp_texture_cfg) */
  int tex_size, top_n;
  float depth_tol /* metres */, cos_min, zfar;
} fp_texture_cfg;
int fp_texture_bake(fp_ctx *ctx, const float *d_pos, int V, const int32_t *d_faces, int F, const uint8_t *d_vertex_colors,
                    const uint8_t *d_rgb, const float *d_depth, const uint8_t *d_mask, int n_views, int H, int W, const double *K,
                    const double *cam_in_ob, const fp_texture_cfg *cfg, uint8_t *d_texture, float *d_uv, int8_t *d_used, void *stream);

/* ---- distance between surfaces: the exact distance from points to a triangle mesh, a deterministic surface sampler and the
 *      statistics Chamfer, Hausdorff and F-score are made of (csrc/surface_distance.hip).  The reference has no such function; the
 *      nearest is the cKDTree query of adds_err (src/Utils.py:242-253), which is point to VERTEX and so depends on the tessellation.
 *      tests/surface_distance_oracle.py restates the rules below in float64 numpy. */
#define FP_SURFDIST_MAX_POINTS (1 << 24)
#define FP_SURFDIST_MAX_FACES (1 << 23)
#define FP_SURFDIST_MAX_TAUS 8
#define FP_SURFDIST_MAX_SAMPLES (1 << 22)
#define FP_SURFDIST_TILE 1024   /* queries of one workgroup */
#define FP_SURFDIST_CHUNK 256   /* face records of one LDS chunk */
/* Nearest triangle of a mesh for n query points, by brute force over ALL F faces.  d_points (n,3), d_pos (V,3) float32, d_faces (F,3)
 * int32, device.  d_dist (n) float32; d_face (n) int32 or null; d_closest (n,3) float32 or null: the nearest point on that face.
 *   Per face, once, in DOUBLE from the fp32 positions and rounded to fp32 once: ab = b - a, ac = c - a, e00 = ab.ab, e01 = ab.ac,
 * e11 = ac.ac, n = ab x ac, det = n.n, the unit normal nu = n / sqrt(det), and inv(x) = 1 / x where x > 0 and the fp32 value is finite,
 * else 0, of e00, e11 and ebc = bc.bc (bc = ac - ab).  (The cross product of a sliver cancels; in double its unit normal keeps full fp32
 * precision.)
 *   Per pair (point p, face a b c), fp32, nothing contracted, fma(x, y, z) where written; dot(u, w) = fma(u.x, w.x, fma(u.y, w.y,
 * u.z w.z)).  Everything is relative to a: ap = p - a, bp = ap - ab, cp = ap - ac, and the six dot products of the region
 * classification, each from its own difference vector so that nothing cancels against the size of the face: d1 = dot(ab, ap),
 * d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp); vc = fma(e00, d2, -(e01 d1)),
 * vb = fma(e11, d1, -(e01 d2)).  The closest point relative to a is q of the FIRST region that applies, of seven:
 *     vertex a   d1 <= 0 and d2 <= 0                                   q = 0
 *     vertex b   d3 >= 0 and d4 <= d3                                  q = ab
 *     edge ab    vc <= 0 and d1 >= 0 and d3 <= 0                       q = s ab, s = d1 inv(e00)
 *     vertex c   d6 >= 0 and d5 <= d6                                  q = ac
 *     edge ac    vb <= 0 and d2 >= 0 and d6 <= 0                       q = t ac, t = d2 inv(e11)
 *     edge bc    vb + vc >= det and d4 - d3 >= 0 and d5 - d6 >= 0      q = fma(w, bc, ab), bc = ac - ab in fp32,
 *                                                                      w = min(max(dot(bc, bp) inv(ebc), 0), 1)
 *     interior   otherwise                                             q = ap - h nu, h = dot(nu, ap): the foot of the perpendicular
 * (vertices and the edges ab, ac: q = fma(t, ac, s ab) per component with the (s, t) shown, 0 or 1 otherwise.)  (dx, dy, dz) = ap - q -
 * for the interior h nu itself - and d2 = fma(dx, dx, fma(dy, dy, dz dz)): the difference form of fp_pose_errors, so a point that is a
 * vertex of the face gives exactly 0.  closest = a + q.  Against float64 the distance is off by at most 1 x 2^-24 x (the diagonal of the
 * bounding box of points and mesh) on the shapes of tests/test_gpu_surface_distance.py, slivers included.
 *   Degenerate faces.  A face with det = 0 - its cross product is exactly zero: collinear or coincident vertices - (or with a det below
 * the smallest fp32 number) is the minimum over its three segments (a, ab), (a, ac), (b, bc) in that order, a later one replacing an
 * earlier one only when strictly smaller: with o the segment's origin and e its direction, u = p - o (for b: bp),
 * t = min(max(dot(u, e) inv(dot(e, e)), 0), 1), q = t e, d2 of u - q as above.  A segment of zero length has inv = 0: it is its end
 * point.  No NaN comes of it.
 *   Over the faces.  The smallest fp32 d2 wins; equal values go to the LOWEST face index; dist = sqrtf(d2).  The result of a point is a
 * function of that point and the mesh alone, bit for bit: it does not depend on the batch, the query's index, how the faces are divided
 * among the workgroups, or the run.  (Each workgroup folds its candidates into a 64-bit key, d2's bits << 32 | face, with an integer
 * atomicMin: non-negative fp32 bit patterns order as unsigned integers.  No float atomics.)
 *   Bad values.  A pair whose d2 is NaN or infinite is never selected: a face with a non-finite vertex is never selected, and a query
 * with a non-finite coordinate, like one for which no face is left, gets dist = NaN,
 * face = -1, closest = NaN.  A face index outside [0, V) is found on the device and that face is never followed or selected; no error
 * is reported (the call does not synchronise).
 *   Work: n F pair tests, about 0.4 M of them per microsecond on an MI355X (README.md) - no spatial cull.  The context's arena holds the n
 * keys (8 n bytes).  n = 0 succeeds and writes nothing.  FP_EINVAL: a null ctx, d_pos or d_faces; d_points or d_dist null with n > 0;
 * V < 1; F < 1 (F = 0 included) or above FP_SURFDIST_MAX_FACES; n < 0 or above FP_SURFDIST_MAX_POINTS. */
int fp_point_mesh_distance(fp_ctx *ctx, const float *d_points, int n, const float *d_pos, int V, const int32_t *d_faces, int F,
                           float *d_dist, int32_t *d_face, float *d_closest, void *stream);

#define FP_SURFDIST_STATS_COUNT 0        /* entries of d_stats: the number of finite entries of d_dist */
#define FP_SURFDIST_STATS_SUM 1          /* their sum */
#define FP_SURFDIST_STATS_SUM_SQ 2       /* the sum of their squares */
#define FP_SURFDIST_STATS_MAX 3          /* the largest (0 when there is none; distances are >= 0) */
#define FP_SURFDIST_STATS_NOT_FINITE 4   /* the number of entries that are NaN or infinite: they are left out of everything else */
#define FP_SURFDIST_STATS_TAU0 5         /* [5 + k]: the number of finite entries with (double)d <= h_taus[k] */
/* Statistics of n distances, as FP_SURFDIST_STATS_TAU0 + n_taus doubles in d_stats (device).  d_dist (n) float32, device; h_taus
 * (n_taus <= FP_SURFDIST_MAX_TAUS) float64, host, read before the call returns.  Every entry is widened to double first; the sums are
 * double sums of per-workgroup partials that a finishing launch adds in tile order - no float atomics - so the same input gives the same
 * bits on every run; the counts and the maximum are exact.  Nothing synchronises.  n = 0 gives zeros.  FP_EINVAL: a null ctx or d_stats,
 * d_dist null with n > 0, n outside 0 .. FP_SURFDIST_MAX_POINTS, n_taus outside 0 .. FP_SURFDIST_MAX_TAUS, h_taus null with n_taus > 0. */
int fp_distance_stats(fp_ctx *ctx, const float *d_dist, int n, const double *h_taus, int n_taus, double *d_stats, void *stream);

/* Distances of n surface samples to a mesh under T rigid transforms, and their statistics per transform: what a search for the mesh's
 * symmetries asks of the device (Utils.find_symmetries).  d_points (n,3) float32; d_tfs (T,3,4) float32, row-major [R|t] with rows
 * (r00 r01 r02 tx), (r10 r11 r12 ty), (r20 r21 r22 tz); d_pos (V,3) float32, d_faces (F,3) int32: device.  h_taus (n_taus <=
 * FP_SURFDIST_MAX_TAUS) float64, host, read before the call returns.
 *   The query (k, i) is q = R_k p_i + t_k in fp32, nothing contracted, the translation innermost:
 *     q.x = fma(r00, p.x, fma(r01, p.y, fma(r02, p.z, tx))), and q.y, q.z the same with rows 1 and 2.
 * Its distance is what fp_point_mesh_distance gives for the point q - the same pair rule, the smallest fp32 d2, equal values to the
 * lowest face, sqrtf - bit for bit a function of (q, mesh) alone: not of T, n, the tile the query lands in or how the faces are divided.
 * The bad-value rules are those of fp_point_mesh_distance (a non-finite q, or no face left: dist = NaN).
 *   d_stats (T, FP_SURFDIST_STATS_TAU0 + n_taus) float64, device: row k holds the entries of fp_distance_stats over the n distances of
 * transform k.  The queries are flattened to g = k n + i and tiled by FP_SURFDIST_TILE - a tile may hold parts of several transforms -
 * and the sums are double sums of per-workgroup partials, one per (tile, transform), that a finishing launch adds in tile order: no
 * float atomics, the same input gives the same bits on every run.  The counts and the maximum are exact.
 *   d_q (T n,3) float32 or null: the transformed points; d_dist (T n) float32 or null: their distances.  (Feeding d_q to
 * fp_point_mesh_distance gives d_dist again, bit for bit: tests/test_gpu_symmetry.py.)
 *   Work: T n F pair tests at the rate of fp_point_mesh_distance - no spatial cull - plus one pass over the T n keys; the arena holds
 * the keys (8 T n bytes) and the partials.  Nothing synchronises.  n = 0 gives zeros.  FP_EINVAL: T < 1; n < 0; T n above
 * FP_SURFDIST_MAX_POINTS; a null ctx, d_tfs, d_pos, d_faces or d_stats; d_points null with n > 0; V < 1; F < 1 or above
 * FP_SURFDIST_MAX_FACES; n_taus outside 0 .. FP_SURFDIST_MAX_TAUS; h_taus null with n_taus > 0. */
int fp_symmetry_residuals(fp_ctx *ctx, const float *d_points, int n, const float *d_tfs, int T, const float *d_pos, int V,
                          const int32_t *d_faces, int F, const double *h_taus, int n_taus, double *d_stats, float *d_q, float *d_dist,
                          void *stream);

/* Rigid alignment of a point set to a mesh: one Gauss-Newton linearisation of ICP against the EXACT nearest triangle for N poses at
 * once (fp_points_mesh_align) and the loop of it with fp_pose_gn_step behind it (fp_points_mesh_polish).  The reference has no such
 * step.  tests/mesh_align_oracle.py restates the rows in fp32 numpy, operation for operation.
 *   d_points (n,3) float32: the source points, in the source's frame.  d_poses (N,4,4) float32 row-major, "target from source"; the
 * first 12 floats of a pose are the (3,4) record [R|t] of fp_symmetry_residuals, read in place (a transform stride of 16 floats).
 * d_pos (V,3), d_faces (F,3): the target.  d_keys: N n 64-bit words of the caller's, 8-byte aligned, scratch.
 *   Search.  The query of (pose k, point i) is y = R_k p_i + t_k by fp_symmetry_residuals' rule; d_keys is set to all ones - by a small
 * launch, not a memset node: the call is made to sit in a captured graph, and no captured path of the library holds one - and the
 * search kernel of fp_point_mesh_distance runs over the N n queries.  dist, face and closest of a query are bit for bit what
 * fp_point_mesh_distance returns for the point y.
 *   Rows.  Per query, fp32, nothing contracted, every operation written out:
 *     c = closest, nu = the record's unit normal of the winning face (zeros for a degenerate face), t = (pose[3], pose[7], pose[11])
 *     e = y - c;  X = y - t
 *     valid = a face was found and dist <= dist_max (the fp32 value written to d_dist: NaN fails)
 *     FP_MESH_ALIGN_PLANE, one row:  valid = valid and the winning face is not degenerate
 *       r = (nu.x e.x + nu.y e.y) + nu.z e.z;   J = (nu.x, nu.y, nu.z, X.y nu.z - X.z nu.y, X.z nu.x - X.x nu.z, X.x nu.y - X.y nu.x)
 *     FP_MESH_ALIGN_POINT, three rows, a = 0, 1, 2 in that order:  r = e[a];  J as above with nu = the unit vector of axis a
 *   The face normal, not the direction e / |e|: e vanishes at the solution, so its direction is noise exactly where the last steps are
 * taken, and off an edge or a vertex it is not the normal of any plane of the model.
 *   J is dr / dxi for R <- exp([w]) R, t <- t + tau, xi = (tau, w) in the target's frame, about the pose's own translation: the twist
 * fp_pose_gn_step applies.  An invalid point is a zero row.  d_sums (N,29) float64, device: the terms of fp_pose_depth_align in the
 * same order, formed and added as csrc/gn_sums.h states - one workgroup per (pose, tile of 1024 points), 256 threads x 4 points, a
 * lane's rows in point order and within a point in axis order, the butterfly, the waves, then the tiles by a second launch.  In POINT
 * mode only the row of axis 0 carries the count: term 28 counts points and term 27 is the sum of e.e, the squared distances.  No float
 * atomics (the one integer atomicMin per (query, face slice) is the search's): a pose's 29 numbers are bit-identical from run to run,
 * in any batch and at any index of it.
 *   Optional outputs, device, each may be null: d_q (N,n,3) the queries; d_dist (N,n); d_face (N,n) int32; d_closest (N,n,3); d_normal
 * (N,n,3) nu (zeros where no face was found); d_rows (N,n,R,8), R = 1 (PLANE) or 3 (POINT), 16-byte aligned: (J0 .. J5, r, flag) per row,
 * flag = 1 on the row that carries the count (POINT: the row of axis 0) and 0 on the other two; eight zeros for an invalid point.  h_sums, when not null, HOST (N,29): the call copies d_sums there and SYNCHRONISES; without it
 * nothing synchronises.  The arena holds the partial sums only (N tiles 232 bytes).
 *   Loop.  fp_points_mesh_polish takes n_stages <= FP_MESH_ALIGN_MAX_STAGES records (mode, dist_max, iterations) from the host.  Every
 * stage first sets the N records of d_state to zero bytes (a pose that stopped because its residual rose has converged at that
 * stage's gate and is taken up again by the next), then enqueues `iterations` rounds of (the keys set to all ones, the search, the
 * rows and their fold, fp_pose_gn_step with min_points in the place of min_pixels).  After the last stage one closing round at that
 * stage's mode and gate, closing = 1: d_state holds the fit of the returned poses and describes the last stage alone.  Nothing
 * synchronises and nothing is read on the host; with the arena reserved the call sits in a captured graph and replays bit for bit.  It
 * equals the same launches issued through the public calls.
 *   Work: N n F pair tests per round at the rate of fp_point_mesh_distance - no spatial cull.  Rigid only, no scale.  Align the PARTIAL
 * surface to the COMPLETE one: every source point looks for a partner, so source points without a counterpart pull.
 *   FP_EINVAL, each checked before ctx is looked into: a null ctx, d_poses, d_pos, d_faces, d_keys or d_sums (polish: d_state, h_stages);
 * d_points null with n > 0; N outside 0 .. FP_POSE_ALIGN_MAX_POSES; n < 0; N n above FP_SURFDIST_MAX_POINTS; V < 1; F outside
 * 1 .. FP_SURFDIST_MAX_FACES; a mode that is neither of the two; dist_max not > 0; d_keys or d_state not 8-byte, d_rows not 16-byte
 * aligned; n_stages outside 1 .. FP_MESH_ALIGN_MAX_STAGES; iterations of a stage outside 0 .. FP_POSE_POLISH_MAX_ITERATIONS; damping
 * negative or not finite; min_points < 1.  N = 0 writes nothing; n = 0 writes zero sums. */
#define FP_MESH_ALIGN_PLANE 0             /* point to plane: one row per point */
#define FP_MESH_ALIGN_POINT 1             /* point to point: three rows per point */
#define FP_MESH_ALIGN_MAX_STAGES 8
typedef struct fp_mesh_align_stage {
  int32_t mode;                           /* FP_MESH_ALIGN_* */
  float dist_max;                         /* the gate, in the mesh's unit */
  int32_t iterations;
} fp_mesh_align_stage;
int fp_points_mesh_align(fp_ctx *ctx, const float *d_points, int n, const float *d_poses, int N, const float *d_pos, int V,
                         const int32_t *d_faces, int F, int mode, float dist_max, uint64_t *d_keys, float *d_q, float *d_dist,
                         int32_t *d_face, float *d_closest, float *d_normal, float *d_rows, double *d_sums, double *h_sums, void *stream);
int fp_points_mesh_polish(fp_ctx *ctx, const float *d_points, int n, float *d_poses, int N, const float *d_pos, int V,
                          const int32_t *d_faces, int F, const fp_mesh_align_stage *h_stages, int n_stages, double damping, int min_points,
                          fp_pose_state *d_state, double *d_sums, uint64_t *d_keys, void *stream);

/* n points on the surface of a mesh, area-weighted, stratified along the face order, a function of (mesh, n, seed) alone.
 *   Face choice, exact.  area_f = 0.5 |ab x ac| in double from the fp32 positions (edge differences, cross product and square root in
 * double; 0 for a face with an index outside [0, V) or a non-finite area), A = their double sum, area_q[f] = rint(area_f / A 2^40) as
 * int64: units of 2^-40 A, so the integer total A_q is 2^40 to within F / 2, and integer prefix sums are exact in any order.  Sample i
 * of n targets t_i = ((2 i + 1) A_q) div (2 n) in unsigned 64-bit integers and lands on the first face whose INCLUSIVE prefix sum of
 * area_q exceeds t_i: every face gets its share n area_q[f] / A_q of the samples to within one.
 *   Barycentrics.  h = lowbias32 (Chris Wellons' 32-bit integer hash: x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b,
 * x ^= x >> 16, in uint32); ku = h(h(seed) + 2 i) >> 8, kv = h(h(seed) + 2 i + 1) >> 8 (uint32 sums); u, v = (k + 0.5) / 2^24,
 * reflected when u + v > 1, which is done exactly on the integers: if ku + kv >= 2^24 then ku = 2^24 - 1 - ku, kv = 2^24 - 1 - kv.
 * u and v are (k + 0.5) 2^-24 in double rounded to fp32 once; p = fma(v, c - a, fma(u, b - a, a)) per component in fp32.
 *   Outputs, device: d_points (n,3) float32; d_face (n) int32 or null; d_bary (n,2) float32 (u, v) or null; d_area_q (F) int64 or null
 * (written for n = 0 too).  SYNCHRONISES the stream once, to read A: FP_EINVAL for a mesh whose total area is zero or not finite,
 * and for a null ctx, d_pos or d_faces, d_points null with n > 0, V or F < 1, F above FP_SURFDIST_MAX_FACES, n outside
 * 0 .. FP_SURFDIST_MAX_SAMPLES. */
int fp_mesh_sample_surface(fp_ctx *ctx, const float *d_pos, int V, const int32_t *d_faces, int F, int n, uint32_t seed, float *d_points,
                           int32_t *d_face, float *d_bary, int64_t *d_area_q, void *stream);

/* ---- building blocks exported for parity tests and profiling ---------------------------------- */
/* fp16 NHWC implicit-GEMM convolution on MFMA: out = act(conv(in, w) + bias [+ res]).  w_packed is
 * [Cout][Kpad] fp16 with k = (ky*KW+kx)*Cin + ci, Kpad = roundup(KH*KW*Cin, 32), zero padded. */
int fp_conv2d_f16(fp_ctx *ctx, const void *d_in, int Nimg, int H, int W, int Cin, const void *d_w_packed, const float *d_bias,
                  int Cout, int KH, int KW, int stride, int pad, const void *d_res, int relu, void *d_out, int out_f32,
                  void *stream);

/* The band-in-LDS form of the C -> C (C = 128 | 256) 3x3 stride-1 / pad-1 convolutions on 40x40 maps (csrc/conv_s1b.hip; the
 * ResnetBasicBlock convolutions of encodeA and of encodeAB's first stage, learning/models/network_modules.py:73-111): what the networks
 * run for batches of more than 40 hypotheses (more than one round of the general kernel's tiles).  Same operands as fp_conv2d_f16 (w_packed [C][9 C]); bit-identical to the general 3x3 stride-1
 * kernel behind fp_conv2d_f16. */
int fp_conv3x3_band_f16(fp_ctx *ctx, const void *d_in, int Nimg, int C, const void *d_w_packed, const float *d_bias, const void *d_res,
                        int relu, void *d_out, void *stream);
/* The front end of encodeA / encoderA in one launch (csrc/front.hip): a1 = ConvBNReLU_3x3s2(ConvBNReLU_7x7s2(x)), the first two layers
 * of the trunk (learning/models/refine_network.py:37-38, score_network.py:36-37), with the stem's output kept in LDS.  x [Nimg][160][160][8]
 * fp16 NHWC (channels 6, 7 zero); w0_packed [64][416], w1_packed [128][576] fp16 and the folded biases as fp_conv2d_f16 takes them;
 * a1 [Nimg][40][40][128] fp16.  d_a0 (optional, may be null): [Nimg][80][80][64] fp16, receives the stem's output as the kernel's tiles
 * hold it.  Bit-identical to fp_conv2d_f16 on the two layers in turn, at any image count. */
int fp_front_end_f16(fp_ctx *ctx, const void *d_x, int Nimg, const void *d_w0_packed, const float *d_b0, const void *d_w1_packed,
                     const float *d_b1, void *d_a1, void *d_a0, void *stream);
/* fused multi-head self-attention core, 4 heads x 128: qk [M][1024] fp16 (q|k), vt [B][4][128][416] fp16 -> out [M][512] fp16.
 * vt is V transposed, token t of a hypothesis in column (t & ~15) | ((t>>2 & 1) << 3) | ((t>>3 & 1) << 2) | (t & 3)
 * (tokens of a group of 16 in the order 0-3, 8-11, 4-7, 12-15); columns of tokens >= T must hold zeros. */
int fp_attention_f16(fp_ctx *ctx, const void *d_qk, const void *d_vt, int B, int T, void *d_out, void *stream);

/* One nn.Linear(512, 512) on M tokens with the epilogue the transformer heads fuse behind it (csrc/tok_gemm.hip;
 * nn.TransformerEncoderLayer / nn.MultiheadAttention, refine_network.py:56-70, score_network.py:53-54):
 *   epilogue 0: out = [relu](x W^T + b), fp16 [M][512]
 *            1: the same values as the transposed V image [M/tokens][4][128][416] (layout: fp_attention_f16)
 *            2: out = LayerNorm(res + x W^T + b) * gamma + beta, fp16 [M][512] (statistics and residual in fp32)
 *            3: sums over groups of 16 tokens of the normalised rows (before gamma / beta), fp32 [M/16][512]
 *            4 / 5: epilogues 0 / 1 through the kernel the networks' in-projections run (csrc/tok_qkv.hip: a resident 128-token
 *               tile, every column block in one launch); bit-identical to 0 / 1
 *            6 / 7: epilogues 0 / 1 through the few-image form of that kernel (one or two hypotheses: 32-token tiles, K in four
 *               quarters added in order - its own fp32 summation order)
 * h_weight (512x512 row-major) / h_bias / h_gamma / h_beta are host fp32; synchronises the stream. */
int fp_token_linear_f16(fp_ctx *ctx, const void *d_in, int M, const float *h_weight, const float *h_bias, int epilogue, int relu,
                        const void *d_res, const float *h_gamma, const float *h_beta, int tokens, void *d_out, void *stream);

/* Building block: the part of one nn.TransformerEncoderLayer behind its attention core as the RefineNet heads run it, in one launch
 * (refine_network.py:56-70,88-91): x1 = LayerNorm1(tok + att W_out^T + b_out); ff = relu(x1 W1^T + b1); y = LayerNorm2(x1 + ff W2^T + b2)
 * WITHOUT its gamma / beta; d_gsum [M/16][512] fp32 = sums of y over groups of 16 tokens (the token mean, gamma2 / beta2 and the
 * output Linear follow in fp_refine_forward).  d_att / d_tok fp16 [M][512], M a multiple of 16; weights host fp32 row-major
 * (512x512) / (512); synchronises the stream. */
int fp_head_mlp_f16(fp_ctx *ctx, const void *d_att, const void *d_tok, int M, const float *h_w_out, const float *h_b_out,
                    const float *h_gamma1, const float *h_beta1, const float *h_w1, const float *h_b1, const float *h_w2,
                    const float *h_b2, float *d_gsum, void *stream);

/* mycpp.cluster_poses (mycpp/src/app/pybind_api.cpp:24-68); host function, float32 row-major 4x4.
 * h_out must hold n_in*16 floats; returns the number of kept poses (>=1) or a negative error. */
int fp_cluster_poses(float angle_diff_deg, float dist_diff_m, const float *h_poses_in, int n_in, const float *h_symmetry_tfs,
                     int n_sym, float *h_out);

/* timing helper: device time of a kernel class ("conv3x3_halo", "conv3x3_s2", "conv7x7", "linear", "attention", "render", "scene_pass", "draw", "draw_setup") over
 * the launches since the last reset, measured with (pooled) HIP events on the launch stream.  on = 0: off; 1: events around the
 * dominant class only (the 3x3 stride-1 convolutions: what a timed benchmark run carries); 2: around every class. */
int fp_prof_enable(fp_ctx *ctx, int on);
int fp_prof_read(fp_ctx *ctx, const char *kernel_class, double *total_ms, int64_t *launches, double *flops);
/* time during which at least one launch of the class was executing (union of the launch spans; = total_ms unless launches of the
 * class overlap on two streams): FLOPs / busy time is the rate the chip sustains on the class */
int fp_prof_read_busy(fp_ctx *ctx, const char *kernel_class, double *busy_ms);
int fp_prof_reset(fp_ctx *ctx);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif
