"""ctypes binding of libfoundationpose_amd.so (C-ABI: include/foundationpose_amd.h).

There is no CPU fallback: if the HIP library has not been built, importing an op raises with the
build command.  torch is used only for device memory and the current HIP stream.
"""
import ctypes
import os
import weakref
from ctypes import POINTER, Structure, byref, c_char_p, c_double, c_float, c_int, c_int64, c_uint, c_void_p

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libfoundationpose_amd.so')
_lib = None

FP_REFINE_SHARED_TRANSLATION = 1      # include/foundationpose_amd.h
FP_NET_REFINE, FP_NET_SCORE = 0, 1
FP_EINVAL = -1
FP_ERR_ADD, FP_ERR_ADDS, FP_ERR_ADD_SYM = 1, 2, 4      # fp_pose_errors' `which` bits
FP_BOP_MSSD, FP_BOP_MSPD = 1, 2                       # fp_pose_errors_bop's `which` bits
FP_VSD_MAX_TAUS = 32
FP_MESH_DIAMETER_MAX_POINTS = 1 << 21                     # fp_mesh_diameter's largest n_pts
FP_BOX_EXTENTS_MAX_POINTS, FP_BOX_EXTENTS_MAX_FRAMES, FP_BOX_EXTENTS_MAX_EVALS = 1 << 21, 1 << 24, 1 << 40      # fp_box_extents
FP_BOX_EXTENTS_TILE, FP_BOX_EXTENTS_CAND = 1024, 1024    # points of its LDS tile, candidates of its workgroup
FP_MESH_SIMPLIFY_MAX_VERTICES, FP_MESH_SIMPLIFY_MAX_FACES = 1 << 21, 1 << 23      # fp_mesh_simplify_count
FP_MESH_COMPONENTS_MAX_VERTICES, FP_MESH_COMPONENTS_MAX_FACES = 1 << 21, 1 << 23  # fp_mesh_components_count
FP_SCENE_MAX_INSTANCES = 1024                             # fp_scene_instances
FP_SCENE_OCC_DEPTH, FP_SCENE_OCC_INSTANCES = 1, 2         # its `occluders` bits
FP_SCENE_INFO_COLS = 12                                   # int32 columns of a d_info row:
FP_SCENE_INFO_PX_COUNT_ALL, FP_SCENE_INFO_PX_COUNT_VALID, FP_SCENE_INFO_PX_COUNT_VISIB, FP_SCENE_INFO_PX_COUNT_IN_FRAME = 0, 1, 2, 3
FP_SCENE_INFO_BBOX_OBJ, FP_SCENE_INFO_BBOX_VISIB = 4, 8   # x0, y0, x1, y1 each
SCENE_DEPTH_BUDGET = 512 << 20                            # bytes of depth layers per render chunk of fp_scene_instances (api.hip)


class FpTensor(Structure):
  _fields_ = [('name', c_char_p), ('data', c_void_p), ('ndim', c_int), ('shape', c_int64 * 4)]


class FpRefineCfg(Structure):
  _fields_ = [('crop_ratio', c_double), ('normalize_xyz', c_int), ('trans_rep_tanh', c_int),
              ('trans_normalizer', c_float * 3), ('rot_normalizer', c_float)]


class FpRenderOpts(Structure):
  """fp_render_opts (include/foundationpose_amd.h): the non-default arguments of nvdiffrast_render."""
  _fields_ = [('struct_size', ctypes.c_size_t), ('use_light', c_int), ('w_ambient', c_float), ('w_diffuse', c_float), ('light_mode', c_int), ('light_vec', c_float * 3),
              ('has_light_color', c_int), ('light_color', c_float * 3), ('has_projection', c_int), ('projection', c_double * 16), ('d_rast', c_void_p)]


class FpTrackArgs(Structure):
  """fp_track_args (include/foundationpose_amd.h): one tracking frame, every launch of it."""
  _fields_ = [('struct_size', ctypes.c_size_t), ('refine_net', c_void_p), ('score_net', c_void_p), ('mesh', c_void_p), ('d_rgb', c_void_p),
              ('rgb_is_u8', c_int), ('d_depth', c_void_p), ('H', c_int), ('W', c_int), ('K', c_void_p), ('mesh_diameter', c_double),
              ('refine_cfg', c_void_p), ('score_crop_ratio', c_double), ('score_normalize_xyz', c_int), ('iteration', c_int), ('n_hyp', c_int),
              ('d_perturb', c_void_p), ('model_center', c_float * 3), ('d_pose', c_void_p), ('d_pose_of_mesh', c_void_p), ('d_poses', c_void_p),
              ('d_scores', c_void_p), ('d_best', c_void_p), ('d_depth_f', c_void_p), ('d_xyz', c_void_p), ('d_rgb_f', c_void_p)]


FP_TRACK_MAX_OBJECTS = 8             # include/foundationpose_amd.h


class FpTrackObject(Structure):
  """fp_track_object (include/foundationpose_amd.h): one object of a multi-object tracking frame."""
  _fields_ = [('mesh', c_void_p), ('mesh_diameter', c_double), ('model_center', c_float * 3), ('d_pose', c_void_p), ('d_pose_of_mesh', c_void_p)]


class FpTrackObjectsArgs(Structure):
  """fp_track_objects_args (include/foundationpose_amd.h): track_one for several objects of one frame, every launch of it."""
  _fields_ = [('struct_size', ctypes.c_size_t), ('refine_net', c_void_p), ('d_rgb', c_void_p), ('rgb_is_u8', c_int), ('d_depth', c_void_p),
              ('H', c_int), ('W', c_int), ('K', c_void_p), ('refine_cfg', c_void_p), ('iteration', c_int), ('n_obj', c_int), ('objs', c_void_p),
              ('d_depth_f', c_void_p), ('d_xyz', c_void_p), ('d_rgb_f', c_void_p)]


FP_REGISTER_PASS_HYP, FP_REGISTER_MIN_VALID = 1008, 4      # include/foundationpose_amd.h


class FpRegisterObject(Structure):
  """fp_register_object (include/foundationpose_amd.h): one object of a multi-object registration, its device and host outputs."""
  _fields_ = [('mesh', c_void_p), ('mesh_diameter', c_double), ('model_center', c_float * 3), ('d_mask', c_void_p), ('label', ctypes.c_int32),
              ('d_rot_grid', c_void_p), ('n_hyp', c_int), ('d_poses', c_void_p), ('d_scores', c_void_p), ('d_order', c_void_p),
              ('d_pose_of_mesh', c_void_p), ('stats', ctypes.c_int32 * 6), ('median', c_float), ('registered', c_int),
              ('guess_translation', c_double * 3)]


class FpRegisterObjectsArgs(Structure):
  """fp_register_objects_args (include/foundationpose_amd.h): register() for several objects of one frame, every launch of it."""
  _fields_ = [('struct_size', ctypes.c_size_t), ('refine_net', c_void_p), ('score_net', c_void_p), ('d_rgb', c_void_p), ('rgb_is_u8', c_int),
              ('d_depth', c_void_p), ('H', c_int), ('W', c_int), ('K', c_void_p), ('K_inv', c_void_p), ('refine_cfg', c_void_p),
              ('score_crop_ratio', c_double), ('score_normalize_xyz', c_int), ('iteration', c_int), ('n_obj', c_int), ('objs', c_void_p),
              ('d_labels', c_void_p), ('max_pass_hyp', c_int), ('d_depth_f', c_void_p), ('d_xyz', c_void_p), ('d_rgb_f', c_void_p)]


FP_DRAW_MAX_OBJECTS = 64             # include/foundationpose_amd.h: fp_draw_poses
FP_DRAW_BOX, FP_DRAW_AXES, FP_DRAW_FILL, FP_DRAW_CONTOUR = 1, 2, 4, 8
FP_DRAW_ZNEAR = 0.01


class FpDrawObject(Structure):
  """fp_draw_object (include/foundationpose_amd.h): the box, the axes and the colours of one object of fp_draw_poses."""
  _fields_ = [('bbox_min', c_float * 3), ('bbox_max', c_float * 3), ('offset', c_float * 16), ('axis_scale', c_float),
              ('box_color', ctypes.c_uint8 * 3), ('axis_color', ctypes.c_uint8 * 9), ('fill_color', ctypes.c_uint8 * 3)]


class FpDrawArgs(Structure):
  """fp_draw_args (include/foundationpose_amd.h): one fp_draw_poses call."""
  _fields_ = [('struct_size', ctypes.c_size_t), ('d_img_in', c_void_p), ('d_img_out', c_void_p), ('H', c_int), ('W', c_int), ('K', c_void_p),
              ('d_poses', c_void_p), ('n_obj', c_int), ('objs', c_void_p), ('flags', c_int), ('box_thickness', c_float),
              ('axis_thickness', c_float), ('opacity', c_float), ('fill_alpha', c_float), ('d_owner', c_void_p)]


FP_TSDF_MAX_POINTS, FP_TSDF_MAX_VIEWS = 1 << 27, 64      # include/foundationpose_amd.h: fp_tsdf_create, fp_tsdf_integrate
FP_TSDF_PLANES = ('tsdf', 'weight', 'r', 'g', 'b', 'color_weight')      # FP_TSDF_PLANE_*
FP_TSDF_ALIGN_TERMS = 29                                                  # fp_tsdf_align: doubles per view of h_sums
FP_DEPTH_ALIGN_TERMS, FP_DEPTH_ALIGN_MAX_PAIRS = 29, 256                  # fp_depth_pairs_align: doubles per pair of h_sums, pairs per call
FP_PHOTO_ALIGN_TERMS = 58                                                 # fp_depth_pairs_align_photo: doubles per pair of h_sums
FP_POSE_ALIGN_TERMS, FP_POSE_ALIGN_MAX_POSES, FP_POSE_POLISH_MAX_ITERATIONS = 29, 1024, 64     # fp_pose_depth_align, fp_pose_gn_step, fp_pose_polish
FP_POSE_STOP_FEW_PIXELS, FP_POSE_STOP_RESIDUAL_ROSE, FP_POSE_STOP_SINGULAR = 1, 2, 3      # fp_pose_state.stopped
FP_POSE_STOP_REASONS = {1: 'too few valid pixels', 2: 'residual rose', 3: 'singular'}
# fp_pose_state as a numpy record (136 bytes); all-zero bytes are a fresh record
POSE_STATE_DTYPE = np.dtype([('fit_ms', '<f8'), ('fit_count', '<f8'), ('xi', '<f8', (6,)), ('prev_pose', '<f4', (16,)), ('stopped', '<i4'), ('steps', '<i4')])
FP_PLANE_MAX_HYP, FP_PLANE_MOMENT_TERMS = 1024, 10                        # fp_plane_score, fp_plane_moments
FP_SEGMENT_STATS, FP_SEGMENT_MAX_PIXELS = 16, 1 << 28                     # fp_depth_segment_write: int64 per kept component; pixels per call


FP_TEXTURE_MIN_SIZE, FP_TEXTURE_MAX_SIZE, FP_TEXTURE_MAX_TOP_N, FP_TEXTURE_MAX_FACES = 64, 4096, 4, 1 << 21      # fp_texture_bake


# fp_point_mesh_distance, fp_distance_stats, fp_mesh_sample_surface, fp_symmetry_residuals
FP_SURFDIST_MAX_POINTS, FP_SURFDIST_MAX_FACES, FP_SURFDIST_MAX_TAUS, FP_SURFDIST_MAX_SAMPLES = 1 << 24, 1 << 23, 8, 1 << 22
FP_SURFDIST_TILE, FP_SURFDIST_CHUNK = 1024, 256          # queries of a workgroup, face records of an LDS chunk
FP_SURFDIST_STATS_COUNT, FP_SURFDIST_STATS_SUM, FP_SURFDIST_STATS_SUM_SQ, FP_SURFDIST_STATS_MAX, FP_SURFDIST_STATS_NOT_FINITE = 0, 1, 2, 3, 4
FP_SURFDIST_STATS_TAU0 = 5                               # d_stats[5 + k]: the count of d <= taus[k]
# fp_points_mesh_align, fp_points_mesh_polish
FP_MESH_ALIGN_PLANE, FP_MESH_ALIGN_POINT, FP_MESH_ALIGN_MAX_STAGES = 0, 1, 8
FP_MESH_ALIGN_MODES = {'plane': FP_MESH_ALIGN_PLANE, 'point': FP_MESH_ALIGN_POINT}
MESH_ALIGN_STAGE_DTYPE = np.dtype([('mode', '<i4'), ('dist_max', '<f4'), ('iterations', '<i4')])      # fp_mesh_align_stage (12 bytes)


class FpTextureCfg(Structure):
  """fp_texture_cfg (include/foundationpose_amd.h)."""
  _fields_ = [('struct_size', ctypes.c_size_t), ('tex_size', c_int), ('top_n', c_int), ('depth_tol', c_float), ('cos_min', c_float), ('zfar', c_float)]


FP_STEREO_MAX_DISPARITY, FP_STEREO_MAX_CELLS = 256, 1 << 31                # fp_stereo_sgm


class FpStereoOpts(Structure):
  """fp_stereo_opts (include/foundationpose_amd.h)."""
  _fields_ = [('struct_size', ctypes.c_size_t), ('max_disparity', c_int), ('p1', c_int), ('p2', c_int), ('paths', c_uint), ('lr_max', c_int),
              ('min_disparity', c_int), ('subpixel', c_int), ('fx', c_double), ('baseline', c_double), ('zfar', c_float)]


class FpStereoDebug(Structure):
  """fp_stereo_debug: device pointers (or None) that receive the stages of fp_stereo_sgm."""
  _fields_ = [('struct_size', ctypes.c_size_t), ('d_census_left', c_void_p), ('d_census_right', c_void_p), ('d_cost', c_void_p), ('d_sum', c_void_p),
              ('d_dstar', c_void_p), ('d_dright', c_void_p)]


FP_REMAP_COLOUR, FP_REMAP_DEPTH, FP_REMAP_MAX_SIDE = 0, 1, 16384             # fp_remap


class FpRemapPlan(Structure):
  """fp_remap_plan (include/foundationpose_amd.h)."""
  _fields_ = [('k_new', c_float * 4), ('rot', c_float * 9), ('k_raw', c_float * 4), ('dist', c_float * 8), ('r2_max', c_float), ('src_h', c_int),
              ('src_w', c_int), ('dst_h', c_int), ('dst_w', c_int)]


class FpRemapOpts(Structure):
  """fp_remap_opts."""
  _fields_ = [('struct_size', ctypes.c_size_t), ('mode', c_int), ('channels', c_int), ('n_plans', c_int), ('zfar', c_float), ('plan', FpRemapPlan * 2)]


class FpRemapDebug(Structure):
  """fp_remap_debug: device pointers (or None) that receive the (u, v) map of fp_remap."""
  _fields_ = [('struct_size', ctypes.c_size_t), ('d_map0', c_void_p), ('d_map1', c_void_p)]


FP_REPROJECT_MAX_VIEWS, FP_REPROJECT_MAX_SPLAT, FP_REPROJECT_MAX_FRAMES = 8, 8, 65535      # fp_depth_reproject


FP_TEMPLATE_MAX_OBJECTS, FP_TEMPLATE_MAX_SAMPLES, FP_TEMPLATE_MAX_ANCHORS, FP_TEMPLATE_MAX_FRAMES = 64, 1024, 4, 65535      # fp_template_match


class FpObjectBatch(Structure):
  _fields_ = [('mesh', c_void_p), ('d_rgb', c_void_p), ('d_geom', c_void_p), ('H', c_int), ('W', c_int), ('K', c_void_p),
              ('mesh_diameter', c_double), ('n', c_int)]


class FoundationPoseAmdError(RuntimeError):
  pass


_PROTOS = {
  'fp_last_error': (c_char_p, []),
  'fp_version': (c_int, []),
  'fp_ctx_create': (c_int, [c_int, POINTER(c_void_p)]),
  'fp_ctx_destroy': (c_int, [c_void_p]),
  'fp_ctx_reserve': (c_int, [c_void_p, c_int]),
  'fp_ctx_arena_generation': (c_int, [c_void_p]),
  'fp_mesh_create': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, POINTER(c_void_p)]),
  'fp_mesh_destroy': (c_int, [c_void_p]),
  'fp_crop_window_tf': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_double, c_double, c_int, c_int, c_void_p, c_void_p, c_void_p]),
  'fp_render': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_render_ex': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int, POINTER(FpRenderOpts), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_render_net': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_double, c_int, c_float, c_void_p, c_void_p]),
  'fp_crop_observed': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_double, c_int, c_int, c_void_p, c_void_p]),
  'fp_warp_nearest': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
  'fp_erode_depth': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_float, c_void_p, c_void_p]),
  'fp_bilateral_filter_depth': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_float, c_void_p, c_void_p]),
  'fp_depth2xyzmap': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_void_p, c_void_p]),
  'fp_depth_prefilter': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_float, c_float, c_float, c_float, c_void_p, c_float,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_depth2xyzmap_f64': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
  'fp_mask_depth_stats': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
  'fp_pose_errors': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_pose_errors_bop': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
  'fp_vsd': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_double, c_double, c_void_p, c_int,
                     c_void_p, c_void_p, c_void_p]),
  'fp_mesh_diameter': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
  'fp_box_extents': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_mesh_simplify_count': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_float, c_void_p, c_void_p]),
  'fp_mesh_simplify_write': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_int64, c_int64, c_void_p]),
  'fp_mesh_components_count': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p]),
  'fp_mesh_components_write': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
  'fp_scene_instances': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_double, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_draw_poses': (c_int, [c_void_p, POINTER(FpDrawArgs), c_void_p]),
  'fp_tsdf_create': (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_float, POINTER(c_void_p)]),
  'fp_tsdf_destroy': (c_int, [c_void_p]),
  'fp_tsdf_reset': (c_int, [c_void_p, c_void_p, c_void_p]),
  'fp_tsdf_integrate': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p]),
  'fp_tsdf_extract_count': (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
  'fp_tsdf_extract_write': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
  'fp_tsdf_read_plane': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
  'fp_tsdf_align': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p]),
  'fp_depth_normals': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_float, c_void_p, c_void_p]),
  'fp_depth_pairs_align': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_float, c_float, c_void_p,
                                   c_void_p, c_void_p]),
  'fp_view_intensity': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
  'fp_depth_pairs_align_photo': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_float, c_float,
                                         c_float, c_void_p, c_void_p, c_void_p]),
  'fp_pose_depth_align': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_float, c_float,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_pose_gn_step': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_double, c_int, c_int, c_void_p]),
  'fp_pose_polish': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_double, c_double, c_int, c_float,
                             c_float, c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_plane_score': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_int, c_float, c_void_p, c_void_p,
                             c_void_p, c_void_p]),
  'fp_plane_moments': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_float, c_void_p, c_void_p]),
  'fp_depth_segment_count': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_float, c_float, c_float,
                                     c_int, c_void_p, c_void_p]),
  'fp_depth_segment_write': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
  'fp_stereo_sgm': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(FpStereoOpts), c_void_p, c_void_p, POINTER(FpStereoDebug),
                            c_void_p]),
  'fp_remap': (c_int, [c_void_p, c_void_p, c_void_p, c_int, POINTER(FpRemapOpts), c_void_p, c_void_p, c_void_p, c_void_p, POINTER(FpRemapDebug),
                       c_void_p]),
  'fp_depth_reproject': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p,
                                 c_void_p, c_void_p]),
  'fp_template_match': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                c_float, c_float, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
  'fp_template_match_info': (c_int, [c_int, POINTER(c_int)]),
  'fp_texture_bake': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                              POINTER(FpTextureCfg), c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_point_mesh_distance': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_distance_stats': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
  'fp_symmetry_residuals': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                    c_void_p, c_void_p]),
  'fp_points_mesh_align': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_points_mesh_polish': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_double, c_int,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_mesh_sample_surface': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_uint, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_net_create': (c_int, [c_void_p, c_int, POINTER(FpTensor), c_int, c_int, POINTER(c_void_p)]),
  'fp_net_destroy': (c_int, [c_void_p]),
  'fp_net_rot_dim': (c_int, [c_void_p]),
  'fp_refine_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
  'fp_net_tokens': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
  'fp_score_features': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
  'fp_score_tail': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
  'fp_score_tail_scores': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_score_predict_rows_multi': (c_int, [c_void_p, c_void_p, POINTER(FpObjectBatch), c_int, c_double, c_int, c_void_p, c_void_p, c_void_p]),
  'fp_track_frame': (c_int, [c_void_p, POINTER(FpTrackArgs), c_void_p]),
  'fp_track_objects': (c_int, [c_void_p, POINTER(FpTrackObjectsArgs), c_void_p]),
  'fp_register_objects': (c_int, [c_void_p, POINTER(FpRegisterObjectsArgs), c_void_p]),
  'fp_mask_depth_stats_objects': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
  'fp_register_hypotheses': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_register_rank': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_pose_update': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_float, c_void_p, c_void_p]),
  'fp_pose_update_deepim': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_float, c_float, c_float, c_void_p, c_void_p]),
  'fp_refine_predict': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_double, POINTER(FpRefineCfg), c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
  'fp_refine_predict_multi': (c_int, [c_void_p, c_void_p, POINTER(FpObjectBatch), c_int, POINTER(FpRefineCfg), c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
  'fp_refine_predict_multi_flags': (c_int, [c_void_p, c_void_p, POINTER(FpObjectBatch), c_int, POINTER(FpRefineCfg), c_void_p, c_int, c_void_p, c_void_p, c_uint, c_void_p]),
  'fp_score_predict_features_multi': (c_int, [c_void_p, c_void_p, POINTER(FpObjectBatch), c_int, c_double, c_int, c_void_p, c_void_p, c_void_p]),
  'fp_score_predict_features': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_double, c_double, c_int, c_void_p, c_int, c_void_p, c_void_p]),
  'fp_conv3x3_band_f16': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
  'fp_front_end_f16': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
  'fp_conv2d_f16': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
  'fp_token_linear_f16': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
  'fp_head_mlp_f16': (c_int, [c_void_p, c_void_p, c_void_p, c_int] + [c_void_p] * 8 + [c_void_p, c_void_p]),
  'fp_attention_f16': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
  'fp_cluster_poses': (c_int, [c_float, c_float, c_void_p, c_int, c_void_p, c_int, c_void_p]),
  'fp_prof_enable': (c_int, [c_void_p, c_int]),
  'fp_prof_read': (c_int, [c_void_p, c_char_p, POINTER(c_double), POINTER(c_int64), POINTER(c_double)]),
  'fp_prof_read_busy': (c_int, [c_void_p, c_char_p, POINTER(c_double)]),
  'fp_prof_reset': (c_int, [c_void_p]),
}


def exported_symbols():
  """Names declared in include/foundationpose_amd.h (kept in step by tests/test_abi.py)."""
  return sorted(_PROTOS)


def lib():
  global _lib
  if _lib is None:
    if not os.path.exists(LIB_PATH):
      raise FoundationPoseAmdError(
        f'{LIB_PATH} is missing: build the HIP library first (python -c "import __graft_entry__ as g; g.build()" '
        f'or make -C foundationpose_amd/csrc).  foundationpose_amd has no CPU fallback.')
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _PROTOS.items():
      fn = getattr(L, name)
      fn.restype = res
      fn.argtypes = args
    _lib = L
  return _lib


def check(rc):
  if rc != 0:
    msg = lib().fp_last_error()
    raise FoundationPoseAmdError(f'libfoundationpose_amd error {rc}: {msg.decode() if msg else "?"}')


def ptr(t):
  """Device (or host) address of a contiguous torch tensor / numpy array; None -> NULL."""
  if t is None:
    return None
  if torch.is_tensor(t):
    assert t.is_contiguous(), 'tensor must be contiguous'
    return c_void_p(t.data_ptr())
  assert t.flags['C_CONTIGUOUS']
  return c_void_p(t.ctypes.data)


def stream_ptr(device=None):
  return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def k_ptr(K):
  """3x3 intrinsics as a float64 host array (kept alive by the caller)."""
  if torch.is_tensor(K):
    K = K.detach().cpu().numpy()
  Kd = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(3, 3))
  return Kd, c_void_p(Kd.ctypes.data)


def center3(model_center):
  """A model centre rounded to float32, as the `model_center` field of the per-object structures takes it."""
  return (c_float * 3)(*np.asarray(model_center, dtype=np.float32).reshape(3))


class Context:
  """Per-device fp_ctx (workspace arena + profiling).  The opaque handle the reference calls
  `glctx` (dr.RasterizeCudaContext, src/estimater.py:102,168; main.py:42)."""
  _by_device = {}

  def __init__(self, device_index):
    self.device_index = device_index
    h = c_void_p()
    check(lib().fp_ctx_create(device_index, byref(h)))
    self.handle = h

  @classmethod
  def get(cls, device=None):
    if device is None:
      idx = torch.cuda.current_device()
    else:
      d = torch.device(device)
      idx = d.index if d.index is not None else torch.cuda.current_device()
    if idx not in cls._by_device:
      if not torch.cuda.is_available():
        raise FoundationPoseAmdError('no HIP device visible: foundationpose_amd needs an MI355X (no CPU fallback)')
      cls._by_device[idx] = Context(idx)
    return cls._by_device[idx]

  def reserve(self, max_hyp):
    check(lib().fp_ctx_reserve(self.handle, int(max_hyp)))

  def arena_generation(self):
    return int(lib().fp_ctx_arena_generation(self.handle))

  def prof_enable(self, on=True):
    """False / 0: off; 1: events around the dominant kernel class only; True / 2: around every class."""
    check(lib().fp_prof_enable(self.handle, 2 if on is True else int(on)))

  def prof_reset(self):
    check(lib().fp_prof_reset(self.handle))

  def prof_read(self, cls_name):
    ms, n, fl = c_double(), c_int64(), c_double()
    check(lib().fp_prof_read(self.handle, cls_name.encode(), byref(ms), byref(n), byref(fl)))
    busy = c_double()
    check(lib().fp_prof_read_busy(self.handle, cls_name.encode(), byref(busy)))
    return dict(total_ms=ms.value, launches=n.value, flops=fl.value, busy_ms=busy.value)


class DeviceMesh:
  """fp_mesh built from a reference-layout mesh_tensors dict (src/Utils.py:104-130)."""

  def __init__(self, ctx, mesh_tensors):
    f32 = lambda t: np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32))
    i32 = lambda t: np.ascontiguousarray(t.detach().cpu().numpy().astype(np.int32))
    pos, faces, vn = f32(mesh_tensors['pos']), i32(mesh_tensors['faces']), f32(mesh_tensors['vnormals'])
    h = c_void_p()
    if 'tex' in mesh_tensors:
      tex = f32(mesh_tensors['tex']).reshape(mesh_tensors['tex'].shape[-3], mesh_tensors['tex'].shape[-2], 3)
      uv, uvi = f32(mesh_tensors['uv']), i32(mesh_tensors['uv_idx'])
      check(lib().fp_mesh_create(ctx.handle, ptr(pos), len(pos), ptr(faces), len(faces), ptr(vn), None, ptr(uv), len(uv), ptr(uvi),
                                 ptr(tex), tex.shape[0], tex.shape[1], byref(h)))
    else:
      vc = f32(mesh_tensors['vertex_color'])
      check(lib().fp_mesh_create(ctx.handle, ptr(pos), len(pos), ptr(faces), len(faces), ptr(vn), ptr(vc), None, 0, None, None, 0, 0,
                                 byref(h)))
    self.handle = h
    self.ctx = ctx

  def __del__(self):
    try:
      if self.handle:
        lib().fp_mesh_destroy(self.handle)
        self.handle = None
    except Exception:
      pass


_mesh_cache = {}      # id(mesh_tensors['pos']) -> [(device, pos version, signature, DeviceMesh), ...]; dropped when that tensor dies


def _mesh_signature(mesh_tensors):
  """Identity + in-place version of every tensor of the dict.  The entries hold the tensors themselves (strong references,
  except `pos`, whose death drops the entry), so an `id` cannot be recycled while its entry is alive."""
  return tuple((k, v, v._version) for k, v in sorted(mesh_tensors.items()) if torch.is_tensor(v) and k != 'pos')


def device_mesh(ctx, mesh_tensors):
  """The fp_mesh of a reference-layout mesh_tensors dict, uploaded once per (device, set of tensor objects).  The cache is
  keyed on the `pos` tensor OBJECT (its entry is dropped when the tensor dies - a dict built inside one call is not retained) and
  checked against the identity and in-place version counter of every other tensor, so a re-coloured, re-textured or edited
  mesh of the same size is uploaded again instead of being mistaken for the previous one at the same address."""
  pos = mesh_tensors['pos']
  sig = _mesh_signature(mesh_tensors)
  entries = _mesh_cache.get(id(pos))
  if entries is None:
    entries = _mesh_cache[id(pos)] = []
    weakref.finalize(pos, _mesh_cache.pop, id(pos), None)
  for e in entries:
    if e[0] == ctx.device_index and e[1] == pos._version and len(e[2]) == len(sig) and \
       all(a[0] == b[0] and a[1] is b[1] and a[2] == b[2] for a, b in zip(e[2], sig)):
      return e[3]
  m = DeviceMesh(ctx, mesh_tensors)
  entries[:] = [e for e in entries if e[0] != ctx.device_index][-3:]      # one live variant per device and pos object (+ a few devices)
  entries.append((ctx.device_index, pos._version, sig, m))
  return m


def object_batches(ctx, objects, geom_key):
  """list of dicts (rgb, <geom_key>, K, mesh_tensors, mesh_diameter, ob_in_cams) -> (FpObjectBatch array, concatenated
  poses (N,4,4) on the device, keep-alive list).  geom_key = 'xyz_map' (refiner) or 'depth' (scorer)."""
  dev = torch.device('cuda', ctx.device_index)
  arr = (FpObjectBatch * len(objects))()
  keep, poses = [], []
  for i, ob in enumerate(objects):
    rgb = torch.as_tensor(ob['rgb'], device=dev, dtype=torch.float).contiguous()
    geom = torch.as_tensor(ob[geom_key], device=dev, dtype=torch.float).contiguous()
    Kd, _ = k_ptr(ob['K'])
    dm = device_mesh(ctx, ob['mesh_tensors'])
    p = torch.as_tensor(ob['ob_in_cams'], device=dev, dtype=torch.float).reshape(-1, 4, 4)
    keep += [rgb, geom, Kd, dm]
    poses.append(p)
    arr[i].mesh, arr[i].d_rgb, arr[i].d_geom = dm.handle, rgb.data_ptr(), geom.data_ptr()
    arr[i].H, arr[i].W = rgb.shape[0], rgb.shape[1]
    arr[i].K = Kd.ctypes.data
    arr[i].mesh_diameter = float(ob['mesh_diameter'])
    arr[i].n = len(p)
  return arr, torch.cat(poses, 0).contiguous().clone(), keep


class DeviceNet:
  """fp_net built from a reference-layout state_dict (torch tensors).  The float32 host copies of the parameters are kept, so
  the network can be rebuilt on another device (`to`, the counterpart of nn.Module.to in src/estimater.py:97-100)."""

  def __init__(self, ctx, kind, state_dict, use_bn=True):
    self._host = [(k.encode(), np.ascontiguousarray(v.detach().cpu().float().numpy())) for k, v in state_dict.items()
                  if torch.is_tensor(v) and v.dtype.is_floating_point]
    self.kind = kind
    self.use_bn = bool(use_bn)
    self.handle = None
    self._create(ctx)

  def _create(self, ctx):
    arr = (FpTensor * len(self._host))()
    for n, (kb, a) in enumerate(self._host):
      arr[n].name = kb
      arr[n].data = a.ctypes.data
      arr[n].ndim = a.ndim
      for i in range(min(a.ndim, 4)):
        arr[n].shape[i] = a.shape[i]
    h = c_void_p()
    check(lib().fp_net_create(ctx.handle, self.kind, arr, len(self._host), 1 if self.use_bn else 0, byref(h)))
    self.handle = h
    self.ctx = ctx
    self.rot_dim = lib().fp_net_rot_dim(h) if self.kind == FP_NET_REFINE else 0

  def to(self, device):
    """Move the packed weights to `device` (a torch device / string): a no-op on the same device, otherwise the fp_net is
    rebuilt there from the host copies and the old one freed.  Returns self, like nn.Module.to."""
    ctx = Context.get(device)
    if ctx.device_index != self.ctx.device_index:
      old = self.handle
      self._create(ctx)
      lib().fp_net_destroy(old)
    return self

  def __del__(self):
    try:
      if self.handle:
        lib().fp_net_destroy(self.handle)
        self.handle = None
    except Exception:
      pass
