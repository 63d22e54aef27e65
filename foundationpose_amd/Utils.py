"""Host-side mirror of the hot-path subset of the reference's `src/Utils.py`, backed by the HIP library.

Same names, argument meaning and error behaviour as the reference functions cited in each
docstring; tensors live on the HIP device ('cuda' in torch-ROCm).  The rasteriser context is
`RasterizeContext` (the reference's `dr.RasterizeCudaContext`).
"""
import logging
import math
import os
import random

import ctypes
import numpy as np
import torch

from . import _lib
from ._lib import check, k_ptr, lib, ptr, stream_ptr
from .mesh_tensors import make_mesh_tensors  # noqa: F401  (src/Utils.py:104-130)
from .segment import assign_segments, fit_plane, segment_on_plane  # noqa: F401  (masks from depth; a build extension)
from .stereo import stereo_depth, stereo_disparity  # noqa: F401  (depth from a rectified stereo pair; a build extension)
from .rectify import (distort_points, monotonic_r2_max, rectify_pair, rectify_stereo, remap_image, undistort_frame,  # noqa: F401
                      undistort_plan, undistort_points)      # raw stereo pairs and distorted cameras; a build extension
from .reproject import align_frame, gather_by_source, reproject_depth, rgbd_rig  # noqa: F401  (depth and colour from two sensors; a build extension)
from .detect import TemplateSet, build_templates, detect, match_templates, templates_from_depths  # noqa: F401  (objects without a mask; a build extension)
from .pose_icp import align_poses_step, polish_poses, pose_gn_step  # noqa: F401  (polishing poses against depth; a build extension)
from .mesh_align import align_points_step, align_to_mesh, transform_mesh  # noqa: F401  (a mesh or a point cloud onto a model; a build extension)
from .bounds import box_extents, oriented_bounds  # noqa: F401  (the minimum-volume box of a model, main.py:38-39; a build extension)
from .vis import cv_draw_text, depth_to_vis, make_grid_image  # noqa: F401  (src/Utils.py:630-653, 456-478, 293-300)

glcam_in_cvcam = np.array([[1, 0, 0, 0],
                           [0, -1, 0, 0],
                           [0, 0, -1, 0],
                           [0, 0, 0, 1]]).astype(float)


def set_logging_format(level=logging.INFO):
  """src/Utils.py:94-99"""
  logging.basicConfig(level=level, format='[%(funcName)s()] %(message)s')


def set_seed(random_seed):
  """src/Utils.py:222-229"""
  np.random.seed(random_seed)
  random.seed(random_seed)
  torch.manual_seed(random_seed)
  if torch.cuda.is_available():
    torch.cuda.manual_seed_all(random_seed)


class RasterizeContext:
  """Opaque, reusable per-device handle; replaces dr.RasterizeCudaContext(device)
  (main.py:42; src/estimater.py:102,168; src/Utils.py:147)."""

  def __init__(self, device='cuda'):
    self.device = torch.device(device)
    self.ctx = _lib.Context.get(self.device)


RasterizeCudaContext = RasterizeContext   # the reference's spelling


def _ctx_of(glctx, device=None):
  if glctx is None:
    return _lib.Context.get(device)
  if isinstance(glctx, RasterizeContext):
    return glctx.ctx
  if isinstance(glctx, _lib.Context):
    return glctx
  raise TypeError(f'glctx must be a foundationpose_amd RasterizeContext, got {type(glctx)}')


def nvdiffrast_render(K=None, H=None, W=None, ob_in_cams=None, glctx=None, context='cuda', get_normal=False, mesh_tensors=None,
                      mesh=None, projection_mat=None, bbox2d=None, output_size=None, use_light=False, light_color=None,
                      light_dir=np.array([0, 0, 1]), light_pos=np.array([0, 0, 0]), w_ambient=0.8, w_diffuse=0.5, extra={}):
  """src/Utils.py:133-219.  Returns (color (N,h,w,3), depth (N,h,w), normal_map (N,h,w,3)|None);
  extra['xyz_map'] (N,h,w,3).  Rendered by the hand-written HIP rasteriser (csrc/raster.hip)."""
  if glctx is None:
    if context == 'gl' or context == 'cuda':
      glctx = RasterizeContext()
      logging.info("created context")
    else:
      raise NotImplementedError
  if mesh_tensors is None:
    mesh_tensors = make_mesh_tensors(mesh)
  ctx = _ctx_of(glctx)
  dev = torch.device('cuda', ctx.device_index)
  poses = torch.as_tensor(ob_in_cams, dtype=torch.float, device=dev).reshape(-1, 4, 4).contiguous()
  N = len(poses)
  if output_size is None:
    output_size = np.asarray([H, W])
  h, w = int(output_size[0]), int(output_size[1])
  bb = None
  if bbox2d is not None:
    bb = torch.as_tensor(bbox2d, dtype=torch.float, device=dev).reshape(-1, 4).contiguous()
    assert len(bb) == N
  if use_light:
    get_normal = True
  dm = _lib.device_mesh(ctx, mesh_tensors)
  color = torch.empty((N, h, w, 3), dtype=torch.float, device=dev)
  depth = torch.empty((N, h, w), dtype=torch.float, device=dev)
  xyz = torch.empty((N, h, w, 3), dtype=torch.float, device=dev)
  normal = torch.empty((N, h, w, 3), dtype=torch.float, device=dev) if get_normal else None
  default_light = light_color is None and light_dir is not None and np.array_equal(np.asarray(light_dir, dtype=float).reshape(-1), [0, 0, 1])
  # extra={'rast': ...} asks for dr.rasterize's own output as well (u, v, z/w, triangle id + 1 per pixel: src/Utils.py:182's rast_out, rows
  # flipped like the images) - the reference keeps it internal; the parity tests compare coverage and the winning face on it
  rast = torch.empty((N, h, w, 4), dtype=torch.float, device=dev) if 'rast' in extra else None
  if projection_mat is None and (default_light or not use_light) and rast is None:
    Kd, Kp = k_ptr(K)
    check(lib().fp_render(ctx.handle, dm.handle, ptr(poses), N, Kp, int(H), int(W), ptr(bb), h, w, 1 if use_light else 0,
                          float(w_ambient), float(w_diffuse), ptr(color), ptr(depth), ptr(normal), ptr(xyz), stream_ptr(dev)))
  else:
    # light_dir / light_pos / light_color / projection_mat (src/Utils.py:159-161,200-211) travel in fp_render_opts
    o = _lib.FpRenderOpts()
    o.struct_size = ctypes.sizeof(o)
    o.use_light, o.w_ambient, o.w_diffuse = (1 if use_light else 0), float(w_ambient), float(w_diffuse)
    if default_light:
      o.light_mode = 0
    elif light_dir is not None:
      o.light_mode = 1
      o.light_vec[:] = [-float(x) for x in np.asarray(light_dir, dtype=np.float32).reshape(3)]      # light_dir_neg
    else:
      o.light_mode = 2
      o.light_vec[:] = [float(x) for x in np.asarray(light_pos, dtype=np.float32).reshape(3)]
    if light_color is not None:
      o.has_light_color = 1
      o.light_color[:] = [float(x) for x in np.asarray(torch.as_tensor(light_color).cpu(), dtype=np.float32).reshape(3)]
    if projection_mat is not None:
      pm = np.asarray(torch.as_tensor(projection_mat).cpu(), dtype=np.float64).reshape(-1, 4, 4)
      if len(pm) != 1:
        raise NotImplementedError('one projection_mat per call (the reference broadcasts a single matrix in every in-repo call)')
      o.has_projection = 1
      o.projection[:] = [float(x) for x in pm[0].reshape(16)]
    Kp = None
    if K is not None:
      Kd, Kp = k_ptr(K)
    o.d_rast = ptr(rast)
    check(lib().fp_render_ex(ctx.handle, dm.handle, ptr(poses), N, Kp, int(H), int(W), ptr(bb), h, w, ctypes.byref(o), ptr(color), ptr(depth),
                             ptr(normal), ptr(xyz), stream_ptr(dev)))
  extra['xyz_map'] = xyz
  if rast is not None:
    extra['rast'] = rast
  return color, depth, normal


def erode_depth(depth, radius=2, depth_diff_thres=0.001, ratio_thres=0.8, zfar=100, device='cuda'):
  """src/Utils.py:387-395 (numpy in -> numpy out, tensor in -> tensor out)."""
  d = torch.as_tensor(depth, dtype=torch.float, device=device).contiguous()
  ctx = _lib.Context.get(d.device)
  out = torch.empty_like(d)
  check(lib().fp_erode_depth(ctx.handle, ptr(d), d.shape[0], d.shape[1], int(radius), float(depth_diff_thres), float(ratio_thres),
                             float(zfar), ptr(out), stream_ptr(d.device)))
  if isinstance(depth, np.ndarray):
    out = out.data.cpu().numpy()
  return out


def bilateral_filter_depth(depth, radius=2, zfar=100, sigmaD=2, sigmaR=100000, device='cuda'):
  """src/Utils.py:345-356"""
  d = torch.as_tensor(depth, dtype=torch.float, device=device).contiguous()
  ctx = _lib.Context.get(d.device)
  out = torch.empty_like(d)
  check(lib().fp_bilateral_filter_depth(ctx.handle, ptr(d), d.shape[0], d.shape[1], int(radius), float(zfar), float(sigmaD),
                                        float(sigmaR), ptr(out), stream_ptr(d.device)))
  if isinstance(depth, np.ndarray):
    out = out.data.cpu().numpy()
  return out


def depth_prefilter(depth, K, radius=2, depth_diff_thres=0.001, ratio_thres=0.8, zfar=100, sigmaD=2, sigmaR=100000, zfar_xyz=np.inf, rgb_u8=None):
  """The depth prelude of a tracking frame (src/estimater.py:256-260) in one launch (a build extension; not in the reference):
  bilateral_filter_depth(erode_depth(depth, radius), radius) and depth2xyzmap_batch of the result with the float32 camera matrix.
  Returns (depth (H,W), xyz_map (H,W,3)) on the device, bit-identical to the three calls chained; with `rgb_u8` (H,W,3) uint8 on the
  device also its float copy (rgb_u8.to(torch.float)) as a third value, from the same launch."""
  d = torch.as_tensor(depth, dtype=torch.float, device='cuda').contiguous()
  ctx = _lib.Context.get(d.device)
  H, W = d.shape
  out = torch.empty_like(d)
  xyz = torch.empty((H, W, 3), dtype=torch.float, device=d.device)
  Kd, Kp = k_ptr(np.asarray(K.detach().cpu().numpy() if torch.is_tensor(K) else K, dtype=np.float32))
  zf = float(zfar_xyz) if np.isfinite(zfar_xyz) else 3.0e38
  rgb_f = None
  if rgb_u8 is not None:
    if not (torch.is_tensor(rgb_u8) and rgb_u8.is_cuda and rgb_u8.dtype == torch.uint8 and tuple(rgb_u8.shape) == (H, W, 3) and rgb_u8.is_contiguous()):
      raise ValueError('depth_prefilter: rgb_u8 must be a contiguous (H,W,3) uint8 tensor on the device')
    rgb_f = torch.empty((H, W, 3), dtype=torch.float, device=d.device)
  check(lib().fp_depth_prefilter(ctx.handle, ptr(d), H, W, int(radius), float(depth_diff_thres), float(ratio_thres), float(zfar), float(zfar),
                                 float(sigmaD), float(sigmaR), Kp, zf, ptr(out), ptr(xyz), ptr(rgb_u8), ptr(rgb_f), stream_ptr(d.device)))
  return (out, xyz) if rgb_u8 is None else (out, xyz, rgb_f)


def depth2xyzmap(depth, K, uvs=None):
  """src/Utils.py:399-417: back-projection in float64 arithmetic, one rounding to float32, depth < 1 mm -> 0.
  Both input kinds run fp_depth2xyzmap_f64 on the device; a numpy image comes back as numpy (H,W,3) float32 like the
  reference's, a device tensor stays on the device.  `uvs` (n,2) keeps only the listed (rounded) pixels, zeros elsewhere."""
  as_numpy = not torch.is_tensor(depth)
  d = torch.as_tensor(np.ascontiguousarray(depth) if as_numpy else depth, device='cuda').to(torch.float).contiguous()
  ctx = _lib.Context.get(d.device)
  H, W = d.shape[:2]
  xyz = torch.empty((H, W, 3), dtype=torch.float, device=d.device)
  Kd, Kp = k_ptr(K)
  check(lib().fp_depth2xyzmap_f64(ctx.handle, ptr(d), H, W, Kp, ptr(xyz), stream_ptr(d.device)))
  if uvs is not None:
    px = torch.as_tensor(np.asarray(uvs).round().astype(np.int64), device=d.device)
    keep = torch.zeros((H, W, 1), dtype=torch.bool, device=d.device)
    keep[px[:, 1], px[:, 0]] = True
    xyz = xyz * keep
  return xyz.cpu().numpy() if as_numpy else xyz


def mask_depth_stats(depth, mask, min_depth=0.001):
  """Reductions of guess_translation / register()'s validity test on the device (src/estimater.py:137-156,173-177):
  dict(cmin, cmax, rmin, rmax, n_mask, n_usable, median) for a device depth image and a mask (anything non-zero = object)."""
  d = torch.as_tensor(depth, dtype=torch.float, device='cuda').contiguous()
  m = torch.as_tensor(np.ascontiguousarray(mask) if isinstance(mask, np.ndarray) else mask, device=d.device)
  m = (m != 0).to(torch.uint8).contiguous()
  assert m.shape == d.shape, 'mask and depth shapes differ'
  ctx = _lib.Context.get(d.device)
  st = (ctypes.c_int32 * 6)()
  med = ctypes.c_float()
  check(lib().fp_mask_depth_stats(ctx.handle, ptr(d), ptr(m), d.shape[0], d.shape[1], float(min_depth), st, ctypes.byref(med),
                                  stream_ptr(d.device)))
  return dict(cmin=st[0], cmax=st[1], rmin=st[2], rmax=st[3], n_mask=st[4], n_usable=st[5], median=np.float32(med.value))


def mask_depth_stats_objects(depth, masks, min_depth=0.001, labels=None):
  """mask_depth_stats of several objects in ONE launch and one copy to the host (fp_mask_depth_stats_objects): `masks` is a sequence of
  (H,W) masks (anything non-zero = object) or, with `labels` = [id_0, ...], one (H,W) integer label image (pixel == id_o: object o).
  Returns one dict(cmin, cmax, rmin, rmax, n_mask, n_usable, median) per object, each equal to mask_depth_stats of that mask."""
  d = torch.as_tensor(depth, dtype=torch.float, device='cuda').contiguous()
  dev_of = lambda m: torch.as_tensor(np.ascontiguousarray(m) if isinstance(m, np.ndarray) else m, device=d.device)
  H, W = d.shape
  if labels is not None:
    img = dev_of(masks).to(torch.int32).contiguous()
    assert img.shape == d.shape, 'label image and depth shapes differ'
    n = len(labels)
    ids = (ctypes.c_int32 * n)(*[int(x) for x in labels])
    mptr, lptr, keep = None, ptr(img), img
  else:
    keep = [(dev_of(m) != 0).to(torch.uint8).contiguous() for m in masks]
    assert all(m.shape == d.shape for m in keep), 'mask and depth shapes differ'
    n = len(keep)
    ids = None
    mptr, lptr = (ctypes.c_void_p * n)(*[m.data_ptr() for m in keep]), None
  ctx = _lib.Context.get(d.device)
  st = (ctypes.c_int32 * (6 * n))()
  med = (ctypes.c_float * n)()
  check(lib().fp_mask_depth_stats_objects(ctx.handle, ptr(d), mptr, lptr, ids, n, H, W, float(min_depth), st, med, stream_ptr(d.device)))
  return [dict(cmin=st[6 * o], cmax=st[6 * o + 1], rmin=st[6 * o + 2], rmax=st[6 * o + 3], n_mask=st[6 * o + 4], n_usable=st[6 * o + 5],
               median=np.float32(med[o])) for o in range(n)]


def depth2xyzmap_batch(depths, Ks, zfar):
  """src/Utils.py:420-438: (B,H,W) device tensor + (B,3,3) -> (B,H,W,3), float32 on the device."""
  depths = torch.as_tensor(depths, dtype=torch.float, device='cuda').contiguous()
  ctx = _lib.Context.get(depths.device)
  B, H, W = depths.shape
  out = torch.empty((B, H, W, 3), dtype=torch.float, device=depths.device)
  Ks = torch.as_tensor(Ks).reshape(-1, 3, 3)
  zf = float(zfar) if np.isfinite(zfar) else 3.0e38
  for b in range(B):
    Kd, Kp = k_ptr(Ks[b if len(Ks) > 1 else 0])
    check(lib().fp_depth2xyzmap(ctx.handle, ptr(depths[b]), H, W, Kp, zf, ptr(out[b]), stream_ptr(depths.device)))
  return out


def compute_crop_window_tf_batch(pts=None, H=None, W=None, poses=None, K=None, crop_ratio=1.2, out_size=None, rgb=None, uvs=None,
                                 method='min_box', mesh_diameter=None):
  """src/Utils.py:577-621.  Only method='box_3d' exists in the reference's hot path; anything else
  raises RuntimeError exactly as the reference does."""
  if method != 'box_3d':
    raise RuntimeError
  poses = torch.as_tensor(poses, dtype=torch.float, device='cuda').reshape(-1, 4, 4).contiguous()
  ctx = _lib.Context.get(poses.device)
  tf = torch.empty((len(poses), 3, 3), dtype=torch.float, device=poses.device)
  Kd, Kp = k_ptr(K)
  check(lib().fp_crop_window_tf(ctx.handle, ptr(poses), len(poses), Kp, float(crop_ratio), float(mesh_diameter), int(out_size[0]),
                                int(out_size[1]), ptr(tf), None, stream_ptr(poses.device)))
  return tf


def projection_matrix_from_intrinsics(K, height, width, znear, zfar, window_coords='y_down'):
  """src/Utils.py:752-802"""
  depth = float(zfar - znear)
  q = -(zfar + znear) / depth
  qn = -2 * (zfar * znear) / depth
  w, h = width, height
  if window_coords == 'y_up':
    r1 = [0, -2 * K[1, 1] / h, (-2 * K[1, 2] + h) / h, 0]
  elif window_coords == 'y_down':
    r1 = [0, 2 * K[1, 1] / h, (2 * K[1, 2] - h) / h, 0]
  else:
    raise NotImplementedError
  return np.array([[2 * K[0, 0] / w, -2 * K[0, 1] / w, (-2 * K[0, 2] + w) / w, 0], r1, [0, 0, q, qn], [0, 0, -1, 0]])


def to_homo_torch(pts):
  """src/Utils.py:520-526: append w = 1."""
  return torch.nn.functional.pad(pts.to(torch.float), (0, 1), value=1.0)


def _apply_linear(vecs, mats, offset=None):
  """Row-vector form of the reference's broadcasting rule (src/Utils.py:529-546): a stack of B transforms whose B is not
  the number of vectors maps EVERY vector (result (B,N,3)); B equal to the vector count maps them one to one."""
  one_to_one = mats.ndim >= 3 and mats.shape[-3] == vecs.shape[-2]
  if one_to_one:
    out = (vecs[..., None, :] @ mats.swapaxes(-1, -2))[..., 0, :]
    return out if offset is None else out + offset
  out = vecs @ mats.swapaxes(-1, -2)
  return out if offset is None else out + offset[..., None, :]


def transform_pts(pts, tf):
  """src/Utils.py:529-536: R p + t."""
  return _apply_linear(pts, tf[..., :-1, :-1], tf[..., :-1, -1])


def transform_dirs(dirs, tf):
  """src/Utils.py:539-546: R d."""
  return _apply_linear(dirs, tf[..., :3, :3])


def pose_to_egocentric_delta_pose(A_in_cam, B_in_cam):
  """src/Utils.py:838-844: the inverse of egocentric_delta_pose_to_pose -> (trans_delta (B,3), rot_mat_delta (B,3,3))."""
  return B_in_cam[:, :3, 3] - A_in_cam[:, :3, 3], B_in_cam[:, :3, :3] @ A_in_cam[:, :3, :3].transpose(1, 2)


def egocentric_delta_pose_to_pose(A_in_cam, trans_delta, rot_mat_delta):
  """src/Utils.py:848-855: t' = t + dt, R' = dR R (the camera-frame update of the refiner)."""
  n = len(A_in_cam)
  top = torch.cat([rot_mat_delta @ A_in_cam[:, :3, :3], (A_in_cam[:, :3, 3] + trans_delta)[..., None]], dim=-1)
  bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float, device=A_in_cam.device).expand(n, 1, 4)
  return torch.cat([top.to(torch.float), bottom], dim=1)


def compute_mesh_diameter(model_pts=None, mesh=None, n_sample=1000):
  """src/Utils.py:559-574 (model_pts branch; the O(n^2) distance matrix is evaluated in blocks)."""
  if mesh is not None:
    import scipy.linalg
    u, s, vh = scipy.linalg.svd(mesh.vertices, full_matrices=False)
    pts = u @ s
    return float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)))
  model_pts = np.asarray(model_pts)
  if n_sample is None:
    pts = model_pts
  else:
    ids = np.random.choice(len(model_pts), size=min(n_sample, len(model_pts)), replace=False)
    pts = model_pts[ids]
  best = 0.0
  for s0 in range(0, len(pts), 1024):
    best = max(best, float(np.linalg.norm(pts[None] - pts[s0:s0 + 1024, None], axis=-1).max()))
  return best


def mesh_diameter(model_pts=None, mesh=None, mesh_tensors=None, return_pair=False):
  """The exact diameter of a model on the device (fp_mesh_diameter): the largest distance between two of its points, over ALL pairs.

  It replaces the random sub-sample of compute_mesh_diameter (src/Utils.py:559-574) where a value that does not depend on numpy's
  seed is wanted, e.g. against BOP's thresholds, which are defined on the exact diameter of models_info.json.  The points are
  model_pts (N,3), else mesh.vertices, else mesh_tensors['pos']; numpy or torch, rounded to float32.  Returns a python float, and with
  return_pair=True also the pair (i, j), i < j, that spans it - among tied pairs the smallest (i, j).  Fewer than two points give 0.0
  and (0, 0).  The value is read back, so this call synchronises."""
  if model_pts is None:
    if mesh is not None:
      model_pts = np.asarray(mesh.vertices)
    elif mesh_tensors is not None:
      model_pts = mesh_tensors['pos']
    else:
      raise ValueError('mesh_diameter needs model_pts, mesh or mesh_tensors')
  dev = _device_of(model_pts)
  pts = torch.as_tensor(model_pts).to(device=dev, dtype=torch.float).reshape(-1, 3).contiguous()
  out = torch.empty(1, dtype=torch.float, device=dev)
  pair = torch.empty(2, dtype=torch.int32, device=dev)
  ctx = _lib.Context.get(dev)
  check(lib().fp_mesh_diameter(ctx.handle, ptr(pts) if len(pts) else None, len(pts), ptr(out), ptr(pair), stream_ptr(dev)))
  d = float(out.item())
  if return_pair:
    i, j = pair.tolist()
    return d, (int(i), int(j))
  return d


def _mesh_parts(mesh, stored_normals=False):
  """(vertices, faces, normals, colors, visual) of a mesh object or of a tuple (vertices, faces[, normals[, colors]]).  stored_normals:
  a synthetic.SimpleMesh that was given no normals yields None instead of computing them on the host."""
  if isinstance(mesh, (tuple, list)):
    parts = list(mesh) + [None] * (4 - len(mesh))
    return parts[0], parts[1], parts[2], parts[3], None
  visual = getattr(mesh, 'visual', None)
  normals = mesh._vn if stored_normals and hasattr(mesh, '_vn') else getattr(mesh, 'vertex_normals', None)
  return mesh.vertices, mesh.faces, normals, getattr(visual, 'vertex_colors', None), visual


def _faces_on(faces, dev):
  return torch.zeros((0, 3), dtype=torch.int32, device=dev) if faces is None else \
      torch.as_tensor(faces).to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()


def _mesh_arrays_on(pos, faces, normals, colors):
  """The arrays of simplify_mesh_arrays / clean_mesh_arrays on the device of `pos` as float32 / int32 / uint8, checked: (dev, pos, faces,
  normals | None, colors | None)."""
  dev = _device_of(pos)
  pos = torch.as_tensor(pos).to(device=dev, dtype=torch.float).reshape(-1, 3).contiguous()
  V = len(pos)
  faces = _faces_on(faces, dev)
  if normals is not None:
    normals = torch.as_tensor(normals).to(device=dev, dtype=torch.float).reshape(-1, 3).contiguous()
  if colors is not None:
    colors = torch.as_tensor(colors).to(device=dev)
    if colors.dtype != torch.uint8 or colors.dim() != 2 or colors.shape[1] != 3:
      raise ValueError(f'colors must be (V,3) uint8, got {colors.dtype} {tuple(colors.shape)}')
    colors = colors.contiguous()
  for name, a in (('normals', normals), ('colors', colors)):
    if a is not None and len(a) != V:
      raise ValueError(f'{len(a)} {name} for {V} vertices')
  return dev, pos, faces, normals, colors


def _rgb_u8_on(colors, dev, who):
  """Vertex colours of a mesh object, RGB or RGBA uint8, as a (V,3) device tensor."""
  colors = torch.as_tensor(colors).to(device=dev)
  if colors.dtype != torch.uint8:
    raise ValueError(f'{who}: vertex colours must be uint8, got {colors.dtype}')
  return colors.reshape(len(colors), -1)[:, :3].contiguous()


def _mesh_outputs(dev, V, nv, nf, normals, colors, want_map):
  """The output tensors of a mesh *_write call for nv vertices and nf faces: (pos, normals | None, colors | None, faces, vertex_map | None)."""
  o_pos = torch.empty((nv, 3), dtype=torch.float, device=dev)
  o_nrm = None if normals is None else torch.empty((nv, 3), dtype=torch.float, device=dev)
  o_col = None if colors is None else torch.empty((nv, 3), dtype=torch.uint8, device=dev)
  o_faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
  vmap = torch.empty((V,), dtype=torch.int32, device=dev) if want_map else None
  return o_pos, o_nrm, o_col, o_faces, vmap


def _mesh_output_ptrs(out):
  """Their addresses as the *_write calls take them: NULL for an absent or empty tensor."""
  return tuple(ptr(t) if t is not None and len(t) else None for t in out)


def simplify_mesh_arrays(pos, faces, cell, normals=None, colors=None, return_map=False):
  """fp_mesh_simplify_count + fp_mesh_simplify_write on arrays: pos (V,3), faces (F,3) or None (a point cloud), normals (V,3) or None,
  colors (V,3) uint8 or None; numpy or torch, taken to the device as float32 / int32 / uint8.  Returns the device tensors (pos, normals |
  None, colors | None, faces, vertex_map | None).  The count is read back, so this call synchronises."""
  dev, pos, faces, normals, colors = _mesh_arrays_on(pos, faces, normals, colors)
  ctx = _lib.Context.get(dev)
  V, F = len(pos), len(faces)
  nv, nf = _simplify_count(ctx, dev, pos, faces, cell)
  out = _mesh_outputs(dev, V, nv, nf, normals, colors, return_map)
  check(lib().fp_mesh_simplify_write(ctx.handle, ptr(pos) if V else None, ptr(normals), ptr(colors), V, ptr(faces) if F else None, F, float(cell),
                                     *_mesh_output_ptrs(out), nv, nf, stream_ptr(dev)))
  return out


def _simplify_count(ctx, dev, pos, faces, cell):
  counts = (ctypes.c_int64 * 2)()
  check(lib().fp_mesh_simplify_count(ctx.handle, ptr(pos) if len(pos) else None, len(pos), ptr(faces) if len(faces) else None, len(faces),
                                     float(cell), counts, stream_ptr(dev)))
  return int(counts[0]), int(counts[1])


SIMPLIFY_SEARCH_STEPS = 20


def simplify_mesh(mesh, cell=None, max_vertices=None, return_map=False):
  """Vertex-clustering simplification on the device (fp_mesh_simplify_*; the rule is stated in include/foundationpose_amd.h): one vertex
  per occupied cell of a grid of pitch `cell`, degenerate and repeated faces dropped.  Deterministic, bit for bit.

  mesh: anything with `vertices`, `faces` and optionally `vertex_normals` and `visual.vertex_colors` (trimesh.Trimesh, synthetic.SimpleMesh),
  or a tuple (vertices, faces[, normals[, colors]]) of numpy arrays or device tensors; faces None or empty: a point cloud.  Exactly one of
  `cell` (metres) and `max_vertices` is given.  max_vertices runs a fixed bisection on the cell: lo = 0, hi = the largest extent of
  the bounding box (float64); 20 times mid = (lo + hi) / 2, and hi = mid when the count at float32(mid) is at most max_vertices, else
  lo = mid; the result is the mesh at float32(hi).  A mesh that already has at most max_vertices vertices comes back as a copy, cell 0.
  The rasteriser's fast forms take up to 8192 vertices and 65 535 faces: max_vertices=8192 puts a fused or scanned mesh onto them.

  Returns (synthetic.SimpleMesh, info) - info: cell, vertices_in, faces_in, vertices, faces, evaluations (count calls) - and, with
  return_map=True, the (V,) int32 map from input vertex to output vertex (-1: dropped).  A UV-textured mesh is refused (ValueError):
  texture coordinates are not transferred.  The alpha of RGBA colours is set to 255."""
  from .synthetic import SimpleMesh
  if (cell is None) == (max_vertices is None):
    raise ValueError('simplify_mesh: give exactly one of cell and max_vertices')
  visual = None if isinstance(mesh, (tuple, list)) else getattr(mesh, 'visual', None)
  if getattr(visual, 'vertex_colors', None) is None and getattr(visual, 'uv', None) is not None:
    raise ValueError('simplify_mesh: the mesh is UV-textured; texture coordinates are not transferred - bake vertex colours first')
  verts, f_in, normals_in, colors, _ = _mesh_parts(mesh)
  if colors is not None:
    colors = _rgb_u8_on(colors, _device_of(verts), 'simplify_mesh')
  dev, pos, faces, normals, colors = _mesh_arrays_on(verts, f_in, normals_in, colors)
  V, F = len(pos), len(faces)
  info = dict(cell=0.0, vertices_in=V, faces_in=F, vertices=V, faces=F, evaluations=0)

  def as_mesh(p, n, c, f):
    rgba = None if c is None else np.concatenate([c.cpu().numpy(), np.full((len(c), 1), 255, dtype=np.uint8)], 1)
    return SimpleMesh(p.cpu().numpy(), f.cpu().numpy(), vertex_normals=None if n is None else n.cpu().numpy(), vertex_colors=rgba)

  if max_vertices is not None:
    max_vertices = int(max_vertices)
    if max_vertices < 8:
      raise ValueError(f'simplify_mesh: max_vertices {max_vertices} (at least 8: a cell of the whole extent still leaves up to 8 clusters)')
    if V <= max_vertices:      # the arrays as they came, copied to the host: no rounding to float32
      host = lambda x: None if x is None else np.array(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
      rgba = None if colors is None else np.concatenate([colors.cpu().numpy(), np.full((V, 1), 255, dtype=np.uint8)], 1)
      out = SimpleMesh(host(verts), np.zeros((0, 3), dtype=np.int64) if f_in is None else host(f_in), vertex_normals=host(normals_in), vertex_colors=rgba)
      vmap = np.arange(V, dtype=np.int32)
      return (out, info, vmap) if return_map else (out, info)
    ctx = _lib.Context.get(dev)
    lo, hi = 0.0, float((pos.max(0).values.double() - pos.min(0).values.double()).max().item())
    for _ in range(SIMPLIFY_SEARCH_STEPS):
      mid = (lo + hi) / 2
      nv, _ = _simplify_count(ctx, dev, pos, faces, np.float32(mid))
      info['evaluations'] += 1
      if nv <= max_vertices:
        hi = mid
      else:
        lo = mid
    cell = hi
  cell = float(np.float32(cell))
  p, n, c, f, vmap = simplify_mesh_arrays(pos, faces, cell, normals=normals, colors=colors, return_map=return_map)
  info.update(cell=cell, vertices=len(p), faces=len(f), evaluations=info['evaluations'] + 1)
  out = as_mesh(p, n, c, f)
  return (out, info, vmap.cpu().numpy()) if return_map else (out, info)


def _components_count(ctx, dev, faces, V, keep, min_faces, min_fraction):
  if keep not in ('largest', 'all'):
    raise ValueError(f"keep must be 'largest' or 'all', got {keep!r}")
  counts = (ctypes.c_int64 * 4)()
  check(lib().fp_mesh_components_count(ctx.handle, ptr(faces) if len(faces) else None, len(faces), V, int(min_faces), float(min_fraction),
                                       1 if keep == 'largest' else 0, counts, stream_ptr(dev)))
  return tuple(int(c) for c in counts)


def mesh_components(mesh):
  """The connected components of a mesh on the device (fp_mesh_components_*; the rule is stated in include/foundationpose_amd.h): every
  face (a, b, c) joins a-b and b-c.  mesh: anything with `vertices` and `faces`, or a tuple (vertices, faces, ...) of numpy arrays or
  device tensors.  Returns the device tensors (labels (V,) int32 - the lowest vertex index of every vertex' component - and stats (C,2)
  int32 - {n_vertices, n_faces} of the components, numbered by that lowest index).  The count is read back: this call synchronises."""
  verts, faces = _mesh_parts(mesh)[:2]
  dev = _device_of(verts)
  ctx = _lib.Context.get(dev)
  V = len(verts)
  faces = _faces_on(faces, dev)
  # a selection that keeps nothing (no int32 face count reaches min_faces = 2^31 - 1 with F below it): the write then needs no mesh buffers
  C, _, nv, nf = _components_count(ctx, dev, faces, V, 'all', 2 ** 31 - 1, 0.0)
  labels = torch.empty((V,), dtype=torch.int32, device=dev)
  stats = torch.empty((C, 2), dtype=torch.int32, device=dev)
  F = len(faces)
  check(lib().fp_mesh_components_write(ctx.handle, None, None, None, V, ptr(faces) if F else None, F, None, None, None, None, None,
                                       ptr(labels) if V else None, ptr(stats) if C else None, nv, nf, stream_ptr(dev)))
  return labels, stats


def _clean_arrays(pos, faces, normals, colors, keep, min_faces, min_fraction, want_map, want_stats):
  dev, pos, faces, normals, colors = _mesh_arrays_on(pos, faces, normals, colors)
  ctx = _lib.Context.get(dev)
  V, F = len(pos), len(faces)
  C, kept, nv, nf = _components_count(ctx, dev, faces, V, keep, min_faces, min_fraction)
  out = _mesh_outputs(dev, V, nv, nf, normals, colors, want_map)
  labels = torch.empty((V,), dtype=torch.int32, device=dev) if want_stats else None
  stats = torch.empty((C, 2), dtype=torch.int32, device=dev) if want_stats else None
  check(lib().fp_mesh_components_write(ctx.handle, ptr(pos) if V else None, ptr(normals), ptr(colors), V, ptr(faces) if F else None, F,
                                       *_mesh_output_ptrs(out), ptr(labels) if V and want_stats else None,
                                       ptr(stats) if C and want_stats else None, nv, nf, stream_ptr(dev)))
  info = dict(components=C, kept_components=kept, vertices_in=V, faces_in=F, vertices=nv, faces=nf)
  return (*out, labels, stats, info)


def clean_mesh_arrays(pos, faces, normals=None, colors=None, keep='largest', min_faces=1, min_fraction=0.0, return_map=False):
  """fp_mesh_components_count + fp_mesh_components_write on arrays: the mesh of the kept connected components.  pos (V,3), faces (F,3),
  normals (V,3) or None, colors (V,3) uint8 or None; numpy or torch, taken to the device as float32 / int32 / uint8.  A component is kept
  when it has at least min_faces faces and at least min_fraction of the largest component's; keep='largest' then keeps only the one
  with the most faces (the lowest-numbered of equals), keep='all' every such component.  Vertices and faces keep their order; attributes
  are copied bit for bit.  Returns the device tensors (pos, normals | None, colors | None, faces, vertex_map | None).  The count is read
  back, so this call synchronises."""
  return _clean_arrays(pos, faces, normals, colors, keep, min_faces, min_fraction, return_map, False)[:5]


def clean_mesh(mesh, keep='largest', min_faces=1, min_fraction=0.0, return_map=False):
  """Drops the small connected components of a mesh on the device (fp_mesh_components_*; the rule is stated in
  include/foundationpose_amd.h): fused depth noise and scanned models carry floating debris.  mesh: as for simplify_mesh.  keep, min_faces,
  min_fraction: as for clean_mesh_arrays - the default keeps the single component with the most faces; keep='all', min_fraction=0.2
  keeps every part with at least a fifth of the largest one's faces, which is how a lid or a second jaw survives.

  Returns (synthetic.SimpleMesh, info) - info: components, kept_components, vertices_in, faces_in, vertices, faces and component_faces,
  the face counts of the kept components in component order - and, with return_map=True, the (V,) int32 map from input vertex to
  output vertex (-1: dropped).  A UV-textured mesh keeps its texture: nothing is blended, so `uv` is gathered with the vertex map and
  the image is passed through (synthetic.TextureVisual).  The alpha of RGBA colours is set to 255.  A SimpleMesh that was given no normals
  gets none either: the result computes its own when asked, as the input would."""
  from .synthetic import SimpleMesh, TextureVisual
  verts, faces, normals, colors, visual = _mesh_parts(mesh, stored_normals=True)
  uv = None if colors is not None else getattr(visual, 'uv', None)
  if getattr(visual, 'uv_idx', None) is not None:
    raise ValueError('clean_mesh: the mesh carries a per-face texture atlas (visual.uv_idx); its uv entries do not follow the vertices - '
                     'clean the mesh first, then bake_texture')
  if colors is not None:
    colors = _rgb_u8_on(colors, _device_of(verts), 'clean_mesh')
  p, n, c, f, vmap, labels, stats, info = _clean_arrays(verts, faces, normals, colors, keep, min_faces, min_fraction, True, True)
  roots = torch.nonzero(labels == torch.arange(len(labels), dtype=torch.int32, device=labels.device))[:, 0]      # component k has the label roots[k]
  info['component_faces'] = [int(x) for x in stats[vmap[roots] >= 0, 1].tolist()]
  vmap = vmap.cpu().numpy()
  host = lambda t: None if t is None else t.cpu().numpy()
  if uv is not None:
    image = getattr(visual, 'image', None)
    if image is None and getattr(visual, 'material', None) is not None:
      image = visual.material.image
    out = SimpleMesh(host(p), host(f), vertex_normals=host(n), visual=TextureVisual(np.asarray(uv)[vmap >= 0], image))
  else:
    rgba = None if c is None else np.concatenate([host(c), np.full((len(c), 1), 255, dtype=np.uint8)], 1)
    out = SimpleMesh(host(p), host(f), vertex_normals=host(n), vertex_colors=rgba)
  return (out, info, vmap) if return_map else (out, info)


TEXTURE_COS_MIN = math.cos(math.radians(75.0))


def texture_cell(tex_size, n_faces):
  """The edge, in texels, of a cell of fp_texture_bake's atlas: floor(tex_size / g), g = the smallest integer with g g >= ceil(F / 2)."""
  g = math.isqrt(max((int(n_faces) + 1) // 2, 1) - 1) + 1
  return int(tex_size) // g


def texture_size_for(n_faces, min_cell=8):
  """The smallest power of two in fp_texture_bake's range whose cells have at least `min_cell` texels on an edge, or None."""
  T = _lib.FP_TEXTURE_MIN_SIZE
  while T <= _lib.FP_TEXTURE_MAX_SIZE:
    if texture_cell(T, n_faces) >= min_cell:
      return T
    T *= 2
  return None


def bake_texture_arrays(pos, faces, rgbs, depths, K, cam_in_obs, tex_size, colors=None, masks=None, top_n=4, depth_tol=0.005,
                        cos_min=TEXTURE_COS_MIN, zfar=np.inf, want_used=True):
  """fp_texture_bake on arrays (the rule is stated in include/foundationpose_amd.h): pos (V,3), faces (F,3), colors (V,3) uint8 or None,
  rgbs (n,H,W,3) uint8, depths (n,H,W) metres, masks (n,H,W) or None, cam_in_obs (n,4,4) camera-to-object; numpy or torch.  Returns the
  device tensors (texture (T,T,3) uint8, uv (3F,2) float32 in the rasteriser's convention, used (T,T) int8 | None).  Nothing
  synchronises.  At most FP_TSDF_MAX_VIEWS (64) views a call: the colour of a texel is chosen among all views at once, so more cannot
  be cut into calls (ValueError)."""
  dev, pos, faces, _, colors = _mesh_arrays_on(pos, faces, None, colors)
  V, F, T = len(pos), len(faces), int(tex_size)
  if V < 1 or F < 1:
    raise ValueError(f'bake_texture: {V} vertices, {F} faces: nothing to texture')
  if T < _lib.FP_TEXTURE_MIN_SIZE or T > _lib.FP_TEXTURE_MAX_SIZE or T & (T - 1):
    raise ValueError(f'bake_texture: tex_size {T} must be a power of two, {_lib.FP_TEXTURE_MIN_SIZE} .. {_lib.FP_TEXTURE_MAX_SIZE}')
  if texture_cell(T, F) < 4:
    fit = texture_size_for(F, 4)
    raise ValueError(f'bake_texture: {F} faces leave cells of {texture_cell(T, F)} texels at tex_size {T} (at least 4); ' +
                     (f'tex_size {fit} fits' if fit else f'no tex_size up to {_lib.FP_TEXTURE_MAX_SIZE} fits: simplify the mesh first'))
  if not 1 <= int(top_n) <= _lib.FP_TEXTURE_MAX_TOP_N:
    raise ValueError(f'bake_texture: top_n {top_n} (1 .. {_lib.FP_TEXTURE_MAX_TOP_N})')
  poses = np.ascontiguousarray(np.asarray(torch.as_tensor(cam_in_obs).cpu(), dtype=np.float64).reshape(-1, 4, 4))
  n = len(poses)
  if n > _lib.FP_TSDF_MAX_VIEWS:
    raise ValueError(f'bake_texture: {n} views, at most {_lib.FP_TSDF_MAX_VIEWS} in one bake (every texel chooses among all views at once); '
                     f'pass a subset')
  H = W = 0
  if n:
    rgbs = torch.as_tensor(rgbs, device=dev)
    if rgbs.dim() != 4 or rgbs.dtype != torch.uint8 or rgbs.shape[0] != n or rgbs.shape[3] != 3:
      raise ValueError(f'bake_texture: rgbs must be uint8 of shape ({n},H,W,3), got {rgbs.dtype} {tuple(rgbs.shape)}')
    rgbs = rgbs.contiguous()
    H, W = int(rgbs.shape[1]), int(rgbs.shape[2])
    depths = torch.as_tensor(depths, device=dev).to(torch.float).contiguous()
    if tuple(depths.shape) != (n, H, W):
      raise ValueError(f'bake_texture: depths must have the shape {(n, H, W)}, got {tuple(depths.shape)}')
    if masks is not None:
      masks = torch.as_tensor(masks, device=dev)
      if tuple(masks.shape) != (n, H, W):
        raise ValueError(f'bake_texture: masks must have the shape {(n, H, W)}, got {tuple(masks.shape)}')
      masks = (masks != 0).to(torch.uint8).contiguous()
  else:
    rgbs = depths = masks = None
  ctx = _lib.Context.get(dev)
  Kd, Kp = k_ptr(K)
  cfg = _lib.FpTextureCfg(struct_size=ctypes.sizeof(_lib.FpTextureCfg), tex_size=T, top_n=int(top_n), depth_tol=float(depth_tol),
                          cos_min=float(cos_min), zfar=float(zfar) if np.isfinite(zfar) else float('inf'))
  tex = torch.empty((T, T, 3), dtype=torch.uint8, device=dev)
  uv = torch.empty((3 * F, 2), dtype=torch.float, device=dev)
  used = torch.empty((T, T), dtype=torch.int8, device=dev) if want_used else None
  check(lib().fp_texture_bake(ctx.handle, ptr(pos), V, ptr(faces), F, ptr(colors), ptr(rgbs), ptr(depths), ptr(masks), n, H, W, Kp,
                              ptr(poses) if n else None, ctypes.byref(cfg), ptr(tex), ptr(uv), ptr(used), stream_ptr(dev)))
  return tex, uv, used


def bake_texture(mesh, views, tex_size=None, top_n=4, depth_tol=0.005, cos_min=TEXTURE_COS_MIN, return_info=False, min_cell=8, zfar=np.inf):
  """A texture atlas for `mesh` from posed RGB-D reference views, on the device (fp_texture_bake; the rule is stated in
  include/foundationpose_amd.h).  Every face gets its own patch of the atlas and its own three uv entries, so the vertices, faces and
  normals come back unchanged; every texel is the cosang-weighted mean of the bilinear colour samples of the `top_n` views that see
  its surface point most frontally (visible: the view's depth there agrees within depth_tol metres; cosang >= cos_min, default cos 75
  degrees), and a texel no view sees takes the mesh's interpolated vertex colours (grey without any).

  mesh: anything with `vertices`, `faces` and optionally `vertex_normals` and `visual.vertex_colors`.  Simplify first (simplify_mesh
  refuses textured meshes).  views: the dict reconstruct_object takes - rgbs (required), depths, K, cam_in_obs, optional masks - or a
  folder in the reference's layout; at most 64 views.  tex_size: a power of two, 64 .. 4096; None: the smallest whose cells have
  at least min_cell texels on an edge.  Returns a synthetic.SimpleMesh whose visual is TextureVisual(uv, image, uv_idx): `uv` (3F,2)
  float32 in the OBJ / trimesh convention (v up: make_mesh_tensors flips it back, bit for bit), `image` (T,T,3) uint8, `uv_idx`
  (F,3) = arange(3F).  With return_info=True also info: tex_size, cell (texels on a cell's edge), coverage (the share of owned texels
  that at least one view coloured), views."""
  from .synthetic import SimpleMesh, TextureVisual
  if isinstance(views, (str, os.PathLike)):
    from .reconstruct import load_reference_views
    views = load_reference_views(views)
  if views.get('rgbs') is None:
    raise ValueError('bake_texture: the views have no rgbs')
  verts, faces, normals, colors, _ = _mesh_parts(mesh, stored_normals=True)
  F = len(faces)
  f_host = np.asarray(torch.as_tensor(faces).cpu()).reshape(-1, 3)
  if F and (f_host.min() < 0 or f_host.max() >= len(verts)):
    raise ValueError(f'bake_texture: a face indexes a vertex outside 0 .. {len(verts) - 1}')
  if tex_size is None:
    tex_size = texture_size_for(F, min_cell)
    if tex_size is None:
      raise ValueError(f'bake_texture: {F} faces do not fit cells of {min_cell} texels at tex_size {_lib.FP_TEXTURE_MAX_SIZE}; '
                       f'simplify the mesh first or lower min_cell (at least 4)')
  if colors is not None:
    colors = _rgb_u8_on(colors, _device_of(verts), 'bake_texture')
  tex, uv, used = bake_texture_arrays(verts, faces, views['rgbs'], views['depths'], views['K'], views['cam_in_obs'], tex_size, colors=colors,
                                      masks=views.get('masks'), top_n=top_n, depth_tol=depth_tol, cos_min=cos_min, zfar=zfar)
  uv = uv.cpu().numpy()
  uv[:, 1] = np.float32(1) - uv[:, 1]       # exact: texel centres of a power-of-two atlas
  host = lambda x: None if x is None else np.array(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
  out = SimpleMesh(host(verts), f_host.copy(), vertex_normals=host(normals),
                   visual=TextureVisual(uv, tex.cpu().numpy(), uv_idx=np.arange(3 * F, dtype=np.int64).reshape(F, 3)))
  if not return_info:
    return out
  owned = used >= 0
  info = dict(tex_size=int(tex_size), cell=texture_cell(tex_size, F), views=len(views['cam_in_obs']),
              coverage=float((used >= 1).sum().item()) / max(1, int(owned.sum().item())))
  return out, info


def _icosphere_vertices(subdivisions):
  """Unit icosphere: the 12 icosahedron vertices followed, per subdivision, by the normalised
  midpoints of the unique edges (sorted by vertex pair).  trimesh.creation.icosphere
  (src/Utils.py:485-489) is not available offline; its vertex order is unpinned."""
  t = (1.0 + 5.0 ** 0.5) / 2.0
  v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
  f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]])
  v /= np.linalg.norm(v, axis=1, keepdims=True)
  for _ in range(subdivisions):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0), axis=1)
    uniq, inv = np.unique(e, axis=0, return_inverse=True)
    mid = v[uniq].mean(axis=1)
    mid /= np.linalg.norm(mid, axis=1, keepdims=True)
    inv = inv.reshape(3, -1).T + len(v)
    f = np.concatenate([np.stack([f[:, 0], inv[:, 0], inv[:, 2]], 1), np.stack([f[:, 1], inv[:, 1], inv[:, 0]], 1),
                        np.stack([f[:, 2], inv[:, 2], inv[:, 1]], 1), np.stack([inv[:, 0], inv[:, 1], inv[:, 2]], 1)], 0)
    v = np.concatenate([v, mid], 0)
  return v


def sample_views_icosphere(n_views, subdivisions=None, radius=1):
  """src/Utils.py:483-507"""
  if subdivisions is not None:
    verts = _icosphere_vertices(subdivisions) * radius
  else:
    subdivision = 1
    while 1:
      verts = _icosphere_vertices(subdivision) * radius
      if verts.shape[0] >= n_views:
        break
      subdivision += 1
  return _look_at_origin(verts)


def _look_at_origin(eyes):
  """Camera frames at `eyes` looking at the origin (src/Utils.py:491-507): z towards the origin, x = up x z with up = +z
  of the object (x = +x of the object where that product vanishes, i.e. at the poles), y = z x x."""
  eyes = np.asarray(eyes, dtype=np.float64)
  fwd = -eyes / np.linalg.norm(eyes, axis=1, keepdims=True)
  right = np.cross(np.broadcast_to([0.0, 0.0, 1.0], fwd.shape), fwd)
  right[~right.any(axis=1)] = (1.0, 0.0, 0.0)
  right /= np.linalg.norm(right, axis=1, keepdims=True)
  down = np.cross(fwd, right)
  down /= np.linalg.norm(down, axis=1, keepdims=True)
  frames = np.zeros((len(eyes), 4, 4))
  frames[:, :3, :] = np.stack([right, down, fwd, eyes], axis=2)
  frames[:, 3, 3] = 1.0
  return frames


def euler_matrix(ai, aj, ak):
  """transformations.euler_matrix(..., axes='sxyz') restricted to what src/estimater.py:113 uses:
  R = Rz(ak) Ry(aj) Rx(ai)."""
  ci, si, cj, sj, ck, sk = math.cos(ai), math.sin(ai), math.cos(aj), math.sin(aj), math.cos(ak), math.sin(ak)
  M = np.eye(4)
  M[:3, :3] = np.array([[cj * ck, sj * si * ck - ci * sk, sj * ci * ck + si * sk],
                        [cj * sk, sj * si * sk + ci * ck, sj * ci * sk - si * ck],
                        [-sj, cj * si, cj * ci]])
  return M


def cluster_poses(angle_diff, dist_diff, poses_in, symmetry_tfs):
  """mycpp.cluster_poses (mycpp/src/app/pybind_api.cpp:24-68) - native host code in the HIP library."""
  pin = np.ascontiguousarray(np.asarray(poses_in, dtype=np.float32).reshape(-1, 4, 4))
  sym = np.ascontiguousarray(np.asarray(symmetry_tfs, dtype=np.float32).reshape(-1, 4, 4))
  logging.info(f'num original candidates = {len(pin)}')      # the reference's C++ prints these two lines to stdout
  out = np.zeros_like(pin)
  n = lib().fp_cluster_poses(float(angle_diff), float(dist_diff), ptr(pin), len(pin), ptr(sym), len(sym), ptr(out))
  if n < 0:
    check(n)
  logging.info(f'num of pose after clustering: {n}')
  return [out[i] for i in range(n)]


# ---------------------------------------------------------------------------------------------- evaluation against ground truth
_POSE_METRICS = {'add': _lib.FP_ERR_ADD, 'adds': _lib.FP_ERR_ADDS, 'add_sym': _lib.FP_ERR_ADD_SYM}


def pose_errors(poses, gt, model_pts, symmetry_tfs=None, metrics=('add', 'adds')):
  """ADD / ADD-S / symmetric ADD of a batch of poses on the device (fp_pose_errors; src/Utils.py:232-253).

  poses (B,4,4) object-to-camera; gt (4,4) shared by every pose or (B,4,4), one per pose (a tracked sequence against its
  ground truth in one call); model_pts (N,3); symmetry_tfs (K,4,4) in the frame of model_pts (None: the identity only).  numpy or
  torch inputs.  Returns {metric: (B,) float32 device tensor} for each name of `metrics`, in metres:
    'add'     mean_i |pred p_i - gt p_i|
    'adds'    mean_i min_j |gt p_i - pred p_j|   (each ground-truth point queries the predicted points, as adds_err does)
    'add_sym' min_k mean_i |pred p_i - gt S_k p_i|
  ADD-S is an exact brute force over all N x N point pairs.  The results are written on the current stream; nothing synchronises."""
  unknown = [m for m in metrics if m not in _POSE_METRICS]
  if unknown:
    raise ValueError(f'unknown metric(s) {unknown}: choose from {sorted(_POSE_METRICS)}')
  which = 0
  for m in metrics:
    which |= _POSE_METRICS[m]
  dev = poses.device if torch.is_tensor(poses) and poses.is_cuda else torch.device('cuda', torch.cuda.current_device())
  f32 = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.float).contiguous()
  P, G, pts = f32(poses).reshape(-1, 4, 4), f32(gt), f32(model_pts).reshape(-1, 3)
  B = len(P)
  if G.shape == (4, 4):
    gt_per_pose = 0
  elif G.shape == (B, 4, 4):
    gt_per_pose = 1
  else:
    raise ValueError(f'gt must be (4,4) or ({B},4,4), got {tuple(G.shape)}')
  sym = None
  if 'add_sym' in metrics:
    sym = f32(np.eye(4)[None] if symmetry_tfs is None else symmetry_tfs).reshape(-1, 4, 4)
  out = {m: torch.empty(B, dtype=torch.float, device=dev) for m in metrics}
  ctx = _lib.Context.get(dev)
  check(lib().fp_pose_errors(ctx.handle, ptr(pts), len(pts), ptr(P), ptr(G), gt_per_pose, B, ptr(sym), 0 if sym is None else len(sym), which,
                             ptr(out.get('add')), ptr(out.get('adds')), ptr(out.get('add_sym')), stream_ptr(dev)))
  return out


def add_err(pred, gt, model_pts, symetry_tfs=np.eye(4)[None]):
  """src/Utils.py:232-240: mean_i |pred p_i - gt p_i| as a Python float.  Like the reference, `symetry_tfs` is accepted and
  IGNORED; the symmetric form is pose_errors(..., symmetry_tfs=..., metrics=('add_sym',))."""
  return float(pose_errors(torch.as_tensor(pred).reshape(1, 4, 4), gt, model_pts, metrics=('add',))['add'][0])


def adds_err(pred, gt, model_pts):
  """src/Utils.py:242-253: mean over the ground-truth points of the distance to the nearest predicted point, as a Python float
  (exact brute force on the device instead of the reference's cKDTree)."""
  return float(pose_errors(torch.as_tensor(pred).reshape(1, 4, 4), gt, model_pts, metrics=('adds',))['adds'][0])


def compute_auc_sklearn(errs, max_val=0.1, step=0.001):
  """src/Utils.py:255-267 on the host: the fraction of errors <= x on the grid 0, step, .., max_val (the curve stays at 1 from the
  first x where every error is covered, as the reference's early `break` leaves it), integrated by the trapezoid rule - what
  sklearn.metrics.auc computes for an increasing x - over max_val."""
  errs = np.sort(np.array(errs))
  X = np.arange(0, max_val + step, step)
  Y = np.ones(len(X))
  for i, x in enumerate(X):
    y = (errs <= x).sum() / len(errs)
    Y[i] = y
    if y >= 1:
      break
  return float((np.diff(X) * (Y[1:] + Y[:-1]) / 2.0).sum() / (max_val * 1))


# ---------------------------------------------------------------------------------------------- BOP errors and average recall
BOP19_VSD_TAUS = np.arange(0.05, 0.51, 0.05)               # misfit tolerances of VSD, as fractions of the object diameter
BOP19_VSD_DELTA = 0.015                                     # VSD visibility tolerance: BOP's 15 mm, in metres
BOP19_VSD_THETAS = np.arange(0.05, 0.51, 0.05)              # correctness thresholds of e_VSD
BOP19_MSSD_THETAS = np.arange(0.05, 0.51, 0.05)             # x the object diameter
BOP19_MSPD_THETAS = np.arange(5, 51, 5)                     # pixels, x image_width / 640
_BOP_METRICS = {'mssd': _lib.FP_BOP_MSSD, 'mspd': _lib.FP_BOP_MSPD}


def _pose_batch(poses, gt, dev):
  f32 = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.float).contiguous()
  P, G = f32(poses).reshape(-1, 4, 4), f32(gt)
  B = len(P)
  if G.shape == (4, 4):
    return P, G, 0
  if G.shape == (B, 4, 4):
    return P, G, 1
  raise ValueError(f'gt must be (4,4) or ({B},4,4), got {tuple(G.shape)}')


def _device_of(x):
  return x.device if torch.is_tensor(x) and x.is_cuda else torch.device('cuda', torch.cuda.current_device())


def bop_pose_errors(poses, gt, model_pts, K=None, symmetry_tfs=None, metrics=('mssd', 'mspd')):
  """MSSD / MSPD of a batch of poses on the device (fp_pose_errors_bop; bop_toolkit pose_error.mssd / mspd).

  poses (B,4,4) object-to-camera; gt (4,4) shared by every pose or (B,4,4), one per pose; model_pts (N,3); K (3,3) intrinsics, needed
  for 'mspd'; symmetry_tfs (S,4,4) in the frame of model_pts, e.g. symmetry_tfs_from_info(models_info[obj_id]) (None: the identity
  only).  numpy or torch inputs.  Returns {metric: (B,) float32 device tensor}:
    'mssd'  min_k max_i |pred p_i - gt S_k p_i|                    metres
    'mspd'  min_k max_i |pi(pred p_i) - pi(gt S_k p_i)|            pixels; +inf when a point lies at z <= 0 under either pose
  The results are written on the current stream; nothing synchronises."""
  unknown = [m for m in metrics if m not in _BOP_METRICS]
  if unknown:
    raise ValueError(f'unknown metric(s) {unknown}: choose from {sorted(_BOP_METRICS)}')
  if 'mspd' in metrics and K is None:
    raise ValueError("'mspd' needs the intrinsics K")
  which = 0
  for m in metrics:
    which |= _BOP_METRICS[m]
  dev = _device_of(poses)
  P, G, gt_per_pose = _pose_batch(poses, gt, dev)
  pts = torch.as_tensor(model_pts).to(device=dev, dtype=torch.float).reshape(-1, 3).contiguous()
  sym = None if symmetry_tfs is None else torch.as_tensor(symmetry_tfs).to(device=dev, dtype=torch.float).reshape(-1, 4, 4).contiguous()
  Kd, Kp = k_ptr(K) if K is not None else (None, None)
  B = len(P)
  out = {m: torch.empty(B, dtype=torch.float, device=dev) for m in metrics}
  ctx = _lib.Context.get(dev)
  check(lib().fp_pose_errors_bop(ctx.handle, ptr(pts), len(pts), ptr(P), ptr(G), gt_per_pose, B, ptr(sym), 0 if sym is None else len(sym),
                                 Kp, which, ptr(out.get('mssd')), ptr(out.get('mspd')), stream_ptr(dev)))
  return out


def vsd_errors(poses, gt, depth_test, K, mesh=None, mesh_tensors=None, glctx=None, diameter=None, delta=BOP19_VSD_DELTA,
               taus=BOP19_VSD_TAUS, return_counts=False):
  """Visible surface discrepancy of a batch of poses on the device (fp_vsd; bop_toolkit pose_error.vsd with visib_mode='bop19' and
  normalized_by_diameter=True), defined on this library's depth renders (nvdiffrast_render).

  poses (B,4,4); gt (4,4) shared by every pose (rendered once) or (B,4,4); depth_test (H,W) in metres, 0 = missing, shared by every
  pose, or (B,H,W), one frame per pose (a tracked sequence in one call); K (3,3).  The mesh is given as for nvdiffrast_render, in the
  frame the poses refer to (for the poses of register() / track_one(), the original mesh).  diameter=None: compute_mesh_diameter of
  its vertices.  Returns e (B, len(taus)) float32 on the device, and with return_counts=True also (B, 2 + len(taus)) int32 counts:
  |union|, |inter| and the cost of every tau.  Nothing synchronises."""
  if mesh_tensors is None:
    if mesh is None:
      raise ValueError('vsd_errors needs mesh or mesh_tensors')
    mesh_tensors = make_mesh_tensors(mesh)
  if diameter is None:
    verts = np.asarray(mesh.vertices) if mesh is not None else mesh_tensors['pos'].detach().cpu().numpy()
    diameter = compute_mesh_diameter(model_pts=verts, n_sample=10000)
  ctx = _ctx_of(glctx, _device_of(poses))
  dev = torch.device('cuda', ctx.device_index)
  P, G, gt_per_pose = _pose_batch(poses, gt, dev)
  B = len(P)
  D = torch.as_tensor(depth_test).to(device=dev, dtype=torch.float).contiguous()
  if D.dim() == 2:
    depth_per_pose = 0
  elif D.dim() == 3 and len(D) == B:
    depth_per_pose = 1
  else:
    raise ValueError(f'depth_test must be (H,W) or ({B},H,W), got {tuple(D.shape)}')
  H, W = D.shape[-2:]
  t = np.ascontiguousarray(np.asarray(taus, dtype=np.float64).reshape(-1))
  Kd, Kp = k_ptr(K)
  err = torch.empty((B, len(t)), dtype=torch.float, device=dev)
  counts = torch.empty((B, 2 + len(t)), dtype=torch.int32, device=dev) if return_counts else None
  dm = _lib.device_mesh(ctx, mesh_tensors)
  check(lib().fp_vsd(ctx.handle, dm.handle, ptr(D), depth_per_pose, int(H), int(W), Kp, ptr(P), ptr(G), gt_per_pose, B, float(diameter),
                     float(delta), ptr(t), len(t), ptr(err), ptr(counts), stream_ptr(dev)))
  return (err, counts) if return_counts else err


def _host(x):
  return None if x is None else np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float64)


def bop_average_recall(e_vsd=None, e_mssd=None, e_mspd=None, diameter=None, image_width=640, n_targets=None):
  """BOP 2019 average recall on the host (bop_toolkit eval_bop19: the recall of every threshold, averaged).

  e_vsd (n, T) VSD errors of n estimates at T taus; e_mssd (n,) metres; e_mspd (n,) pixels - one estimate per target.  diameter: a
  scalar or one value per estimate (needed for MSSD).  n_targets: the number of targets, estimated or not (default n); the targets
  without an estimate count as misses.  An estimate is correct when e < theta:
    AR_VSD   the mean over every (tau, theta) pair, theta in BOP19_VSD_THETAS
    AR_MSSD  the mean over theta in BOP19_MSSD_THETAS * diameter
    AR_MSPD  the mean over theta in BOP19_MSPD_THETAS * image_width / 640
  Returns a dict with the AR_* of the errors given, and AR, the mean of the three, when all three are given."""
  e_vsd, e_mssd, e_mspd = _host(e_vsd), _host(e_mssd), _host(e_mspd)
  n = next((len(e) for e in (e_vsd, e_mssd, e_mspd) if e is not None), None)
  if n is None:
    raise ValueError('bop_average_recall needs at least one of e_vsd, e_mssd, e_mspd')
  for e in (e_vsd, e_mssd, e_mspd):
    if e is not None and len(e) != n:
      raise ValueError('the error arrays must hold one entry per estimate each')
  n_targets = n if n_targets is None else int(n_targets)
  if n_targets < n or n_targets < 1:
    raise ValueError(f'n_targets {n_targets} must be >= the number of estimates {n} and >= 1')
  recall = lambda e, th: float((e < th).sum()) / n_targets
  out = {}
  if e_vsd is not None:
    e_vsd = e_vsd.reshape(n, -1)
    out['AR_VSD'] = float(np.mean([recall(e_vsd[:, t], th) for t in range(e_vsd.shape[1]) for th in BOP19_VSD_THETAS]))
  if e_mssd is not None:
    if diameter is None:
      raise ValueError('AR_MSSD needs the object diameter')
    d = np.broadcast_to(np.asarray(diameter, dtype=np.float64), (n,))
    out['AR_MSSD'] = float(np.mean([recall(e_mssd, th * d) for th in BOP19_MSSD_THETAS]))
  if e_mspd is not None:
    r = image_width / 640.0
    out['AR_MSPD'] = float(np.mean([recall(e_mspd, th * r) for th in BOP19_MSPD_THETAS]))
  if len(out) == 3:
    out['AR'] = (out['AR_VSD'] + out['AR_MSSD'] + out['AR_MSPD']) / 3.0
  return out


def symmetry_tfs_from_info(info, rot_angle_discrete=5):
  """The symmetry transforms of a BOP models_info entry as (S,4,4) float64, with the signature and results of the reference's helper
  (src/Utils.py:806-835), quirks included:
    - the identity comes first, then every 'symmetries_discrete' matrix with its translation scaled from mm to m (x 0.001);
    - of 'symmetries_continuous' only the first entry is read: its axis is the first of x, y, z with a positive component, and the
      rotations about it by 0, rot_angle_discrete, .. degrees (below 360) follow, each with the entry's 'offset' as its translation,
      NOT scaled - so the identity appears twice for an offset of 0, and an axis about z gives 1 + 360 / rot_angle_discrete transforms;
    - an axis with no positive component gives the single rotation by 0 degrees with that offset.
  The rotations are euler_matrix(angle about x, about y, about z)."""
  tfs = [np.eye(4)]
  if 'symmetries_discrete' in info:
    for T in np.array(info['symmetries_discrete'], dtype=np.float64).reshape(-1, 4, 4):
      T[:3, 3] = T[:3, 3] * 0.001
      tfs.append(T)
  if 'symmetries_continuous' in info:
    cont = info['symmetries_continuous'][0]
    positive = np.flatnonzero(np.asarray(cont['axis'], dtype=np.float64).reshape(3) > 0)
    degrees = np.arange(0, 360, rot_angle_discrete) if len(positive) else np.zeros(1)
    for deg in degrees:
      euler = [0.0, 0.0, 0.0]
      euler[positive[0] if len(positive) else 0] = deg / 180.0 * np.pi
      T = euler_matrix(*euler)
      T[:3, 3] = cont['offset']
      tfs.append(T)
  return np.stack(tfs)


# ---------------------------------------------------------------------------------------------- masks and visibility from poses
SCENE_INFO_KEYS = ('px_count_all', 'px_count_valid', 'px_count_visib', 'visib_fract', 'bbox_obj', 'bbox_visib')     # scene_gt_info.json's
_SCENE_OCCLUDERS = {'depth': _lib.FP_SCENE_OCC_DEPTH, 'instances': _lib.FP_SCENE_OCC_INSTANCES,
                    'both': _lib.FP_SCENE_OCC_DEPTH | _lib.FP_SCENE_OCC_INSTANCES}
_SCENE_WANT = ('mask', 'mask_visib', 'owner', 'depth', 'info')


def scene_info_rows(rows):
  """fp_scene_instances' int rows (n, FP_SCENE_INFO_COLS) -> one dict per instance with scene_gt_info.json's keys (bop_toolkit
  calc_gt_info.py): px_count_all, px_count_valid, px_count_visib, visib_fract = px_count_visib / px_count_all in float64 (0.0 for an
  object that renders nowhere), bbox_obj and bbox_visib as [x, y, w, h] with w = x1 - x0 + 1 ([-1, -1, -1, -1] for an empty set: told by
  the COUNT, a corner at -1 is legal on a padded canvas), and px_count_in_frame.  Host only: Python ints and floats, ready for json."""
  rows = np.asarray(rows)
  if rows.ndim != 2 or rows.shape[1] != _lib.FP_SCENE_INFO_COLS:
    raise ValueError(f'scene_info_rows takes (n, {_lib.FP_SCENE_INFO_COLS}) integer rows, got {rows.shape}')

  def box(r, c, count):
    if count == 0:
      return [-1, -1, -1, -1]
    x0, y0, x1, y1 = (int(x) for x in r[c:c + 4])
    return [x0, y0, x1 - x0 + 1, y1 - y0 + 1]
  out = []
  for r in rows:
    n_all, n_valid = int(r[_lib.FP_SCENE_INFO_PX_COUNT_ALL]), int(r[_lib.FP_SCENE_INFO_PX_COUNT_VALID])
    n_visib, n_in = int(r[_lib.FP_SCENE_INFO_PX_COUNT_VISIB]), int(r[_lib.FP_SCENE_INFO_PX_COUNT_IN_FRAME])
    out.append(dict(px_count_all=n_all, px_count_valid=n_valid, px_count_visib=n_visib,
                    visib_fract=float(np.float64(n_visib) / np.float64(n_all)) if n_all > 0 else 0.0,
                    bbox_obj=box(r, _lib.FP_SCENE_INFO_BBOX_OBJ, n_all), bbox_visib=box(r, _lib.FP_SCENE_INFO_BBOX_VISIB, n_visib),
                    px_count_in_frame=n_in))
  return out


def _scene_pad(pad, H, W):
  """`pad` of scene_instances as (pad_x, pad_y): an int, an (x, y) pair, or 'bop' = (W, H), calc_gt_info's canvas of three frames a side."""
  if isinstance(pad, str):
    if pad != 'bop':
      raise ValueError(f"pad must be an int, an (x, y) pair or 'bop', got {pad!r}")
    return int(W), int(H)
  if np.ndim(pad) == 0:
    return int(pad), int(pad)
  px, py = pad
  return int(px), int(py)


def _scene_occluders(occluders, has_depth):
  """`occluders` of scene_instances as FP_SCENE_OCC_* bits: None = 'depth' if a depth image is given, plus 'instances'; a name, a
  sequence of names, or the bits themselves."""
  if occluders is None:
    return _lib.FP_SCENE_OCC_INSTANCES | (_lib.FP_SCENE_OCC_DEPTH if has_depth else 0)
  if isinstance(occluders, (int, np.integer)):
    return int(occluders)
  names = [occluders] if isinstance(occluders, str) else list(occluders)
  unknown = [o for o in names if o not in _SCENE_OCCLUDERS]
  if unknown:
    raise ValueError(f'unknown occluder(s) {unknown}: choose from {sorted(_SCENE_OCCLUDERS)}')
  bits = 0
  for o in names:
    bits |= _SCENE_OCCLUDERS[o]
  return bits


def scene_instances(K, H, W, meshes, poses, depth=None, occluders=None, delta=BOP19_VSD_DELTA, pad=0,
                    want=('mask', 'mask_visib', 'owner', 'depth', 'info'), glctx=None):
  """Which pixels every object instance of a frame covers, which of them are visible, and how much of the object that is, from the
  instances' poses (fp_scene_instances; bop_toolkit calc_gt_masks.py / calc_gt_info.py, visibility rule 'bop19'), on the device.

  meshes: one mesh or mesh_tensors dict per instance, or a single one shared by all, in the frame the poses refer to; poses (n,4,4);
  depth (H,W) metres, 0 = missing, or None.  occluders: 'depth' (the depth image hides what lies more than delta behind it),
  'instances' (the instances hide one another), 'both' (or a sequence of names), or None = both when a depth image is given, else 'instances'.  pad: pixels of
  canvas around the frame, an int, an (x, y) pair or 'bop' (= (W, H), bop_toolkit's): the part of an object outside the image then
  counts in px_count_all and bbox_obj.  The canvas must fit the rasteriser: at most 6553 pixels wide and 255 of its strips high (a
  strip holds about 15 000 pixels), about 3.8 M pixels - 'bop' fits frames up to 640 x 480; give a smaller pad for larger ones.  Returns a dict with the entries named in `want`:
    'mask', 'mask_visib'  (n,H,W) uint8 device tensors, 0 / 255 as the BOP mask files hold them (`> 0` for bool)
    'owner'               (H,W) int32: the instance in front at the pixel (the smaller index at equal depth), -1 where none renders
    'depth'               (H,W) float32: the depth of that instance, 0 where none
    'info'                a list of n dicts (scene_info_rows); this entry alone waits for the device.
  A visible pixel lies inside the image, so px_count_visib == (mask_visib[i] > 0).sum() and visib_fract is BOP's."""
  unknown = [w for w in want if w not in _SCENE_WANT]
  if unknown:
    raise ValueError(f'unknown output(s) {unknown}: choose from {list(_SCENE_WANT)}')
  H, W = int(H), int(W)
  ctx = _ctx_of(glctx, _device_of(poses))
  dev = torch.device('cuda', ctx.device_index)
  P = torch.as_tensor(poses).to(device=dev, dtype=torch.float).reshape(-1, 4, 4).contiguous()
  n = len(P)
  if isinstance(meshes, dict) or not isinstance(meshes, (list, tuple)):
    meshes = [meshes] * n
  if len(meshes) == 1 and n != 1:
    meshes = list(meshes) * n
  if len(meshes) != n:
    raise ValueError(f'{len(meshes)} meshes for {n} poses: give one per instance, or one for all')
  tensors = {}                                      # one upload per mesh object, however many instances share it
  for m in meshes:
    if id(m) not in tensors:
      tensors[id(m)] = _lib.device_mesh(ctx, m if isinstance(m, dict) else make_mesh_tensors(m))
  handles = (ctypes.c_void_p * max(n, 1))(*[tensors[id(m)].handle for m in meshes])
  D = None
  if depth is not None:
    D = torch.as_tensor(depth).to(device=dev, dtype=torch.float).contiguous()
    if tuple(D.shape) != (H, W):
      raise ValueError(f'depth is {tuple(D.shape)}, the frame {(H, W)}')
  bits = _scene_occluders(occluders, D is not None)
  pad_x, pad_y = _scene_pad(pad, H, W)
  new = lambda name, shape, dtype: torch.empty(shape, dtype=dtype, device=dev) if name in want else None
  mask, visib = new('mask', (n, H, W), torch.uint8), new('mask_visib', (n, H, W), torch.uint8)
  owner, dcomp = new('owner', (H, W), torch.int32), new('depth', (H, W), torch.float)
  rows = new('info', (n, _lib.FP_SCENE_INFO_COLS), torch.int32)
  Kd, Kp = k_ptr(K)
  check(lib().fp_scene_instances(ctx.handle, handles, ptr(P), n, Kp, H, W, pad_x, pad_y, ptr(D), bits, float(delta), ptr(mask), ptr(visib),
                                 ptr(owner), ptr(dcomp), ptr(rows), stream_ptr(dev)))
  out = {}
  if mask is not None:
    out['mask'] = mask
  if visib is not None:
    out['mask_visib'] = visib
  if owner is not None:
    out['owner'] = owner
  if dcomp is not None:
    out['depth'] = dcomp
  if rows is not None:
    out['info'] = scene_info_rows(rows.cpu().numpy())
  return out


# ---- drawing poses on the frame (src/Utils.py:667-749, main.py:67-71) ----------------------------------------------------------------
DRAW_PALETTE = np.array([[0, 255, 0], [255, 128, 0], [0, 160, 255], [255, 0, 255], [255, 255, 0], [0, 255, 255], [160, 96, 255], [255, 255, 255]],
                        dtype=np.uint8)      # RGB; object o takes entry o % 8


def project_3d_to_2d(pt, K, ob_in_cam):
  """src/Utils.py:667-672 on the host: the pixel of the homogeneous object point `pt` (4,), rounded as np.round does (ties to even)."""
  cam = np.asarray(ob_in_cam) @ np.asarray(pt).reshape(4, 1)
  uvw = (np.asarray(K) @ cam[:3]).reshape(-1)
  uvw = uvw / uvw[2]
  return uvw[:2].round().astype(int)


def model_box(mesh_or_pts, oriented=False):
  """(to_origin (4,4), bbox (2,3)) of a model in the shape main.py:38-39 builds: bbox = [-extents / 2, extents / 2] and to_origin moves the
  model into it, so that a pose of the model is drawn with `pose @ inv(to_origin)`.  By default this is the AXIS-ALIGNED box about the
  middle of the vertices' extent.  oriented=True takes the minimum-volume box that the reference asks of trimesh, from
  Utils.oriented_bounds (the candidate class, the convention of axes and signs and the limits are stated there; the search runs on
  the device and hull and frame building take a few tenths of a second on an 8 000-vertex model, so cache the pair)."""
  if oriented:
    to_origin, extents = oriented_bounds(mesh_or_pts)
    return to_origin, np.stack([-extents / 2, extents / 2], axis=0)
  pts = np.asarray(getattr(mesh_or_pts, 'vertices', mesh_or_pts), dtype=np.float64).reshape(-1, 3)
  lo, hi = pts.min(axis=0), pts.max(axis=0)
  to_origin = np.eye(4)
  to_origin[:3, 3] = -(lo + hi) / 2
  extents = hi - lo
  return to_origin, np.stack([-extents / 2, extents / 2], axis=0)


def _per_object(x, n, shape, name):
  """`x` as (n, *shape) float64: one entry for all objects, or one each"""
  x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float64)
  if x.shape == tuple(shape):
    x = np.broadcast_to(x, (n,) + tuple(shape))
  if x.shape != (n,) + tuple(shape):
    raise ValueError(f'{name} is {x.shape}: give {tuple(shape)} for all objects or {(n,) + tuple(shape)}')
  return x


def draw_poses(img, K, poses, bboxes=None, offsets=None, owner=None, box=True, axes=True, fill_alpha=0.0, contour=False, axis_scale=0.1,
               box_thickness=2, axis_thickness=3, transparency=0, colors=None, is_input_rgb=True, out=None, glctx=None):
  """The boxes and axes of n posed objects, and optionally their silhouettes, drawn on a frame in one call (fp_draw_poses; the drawing
  rule is in include/foundationpose_amd.h - the project's own anti-aliased capsules, not cv2's Wu lines).

  img (H,W,3) uint8, a numpy array or a device tensor: the result is of the same kind - a new image, or `out` (which may be `img`
  itself: in place).  poses (n,4,4), numpy or a tensor; a float32 device tensor is read where it lies.  bboxes (2,3) or (n,2,3) min / max
  corners (None: no boxes); offsets (4,4) or (n,4,4), right-multiplied on the poses (main.py:67: inv(to_origin); None: identity).
  owner (H,W) int32: scene_instances' owner map; fill_alpha > 0 tints every object's pixels with its colour, contour=True outlines its
  region.  colors: (3,) or (n,3) for box, fill and contour, in the image's channel order; None takes DRAW_PALETTE.  The x, y, z axes are
  red, green and blue in the order is_input_rgb says.  transparency as draw_xyz_axis': the lines are blended with 1 - transparency."""
  is_np = not torch.is_tensor(img)
  ctx = _ctx_of(glctx, None if is_np else img.device)
  dev = torch.device('cuda', ctx.device_index)
  src = torch.as_tensor(np.ascontiguousarray(img) if is_np else img).to(dev).contiguous()
  if src.dtype != torch.uint8 or src.ndim != 3 or src.shape[2] != 3:
    raise ValueError(f'img must be (H,W,3) uint8, got {tuple(src.shape)} {src.dtype}')
  H, W = int(src.shape[0]), int(src.shape[1])
  P = torch.as_tensor(poses).to(device=dev, dtype=torch.float).reshape(-1, 4, 4).contiguous()
  n = len(P)
  if n > _lib.FP_DRAW_MAX_OBJECTS:
    raise ValueError(f'{n} poses: one call draws at most {_lib.FP_DRAW_MAX_OBJECTS} objects')
  flags = (_lib.FP_DRAW_BOX if box and bboxes is not None else 0) | (_lib.FP_DRAW_AXES if axes else 0)
  if fill_alpha > 0 or contour:
    if owner is None:
      raise ValueError('fill_alpha > 0 and contour=True need the owner map (scene_instances(...)["owner"])')
    flags |= (_lib.FP_DRAW_FILL if fill_alpha > 0 else 0) | (_lib.FP_DRAW_CONTOUR if contour else 0)
  own = None
  if flags & (_lib.FP_DRAW_FILL | _lib.FP_DRAW_CONTOUR):
    own = torch.as_tensor(owner).to(device=dev, dtype=torch.int32).contiguous()
    if tuple(own.shape) != (H, W):
      raise ValueError(f'owner is {tuple(own.shape)}, the frame {(H, W)}')
  boxes = _per_object(bboxes if bboxes is not None else np.zeros((2, 3)), n, (2, 3), 'bboxes')
  offs = _per_object(offsets if offsets is not None else np.eye(4), n, (4, 4), 'offsets')
  cols = DRAW_PALETTE[np.arange(n) % len(DRAW_PALETTE)][:, ::1 if is_input_rgb else -1] if colors is None else _per_object(colors, n, (3,), 'colors')
  axis_cols = np.eye(3, dtype=np.uint8)[:, ::1 if is_input_rgb else -1] * 255
  objs = (_lib.FpDrawObject * max(n, 1))()
  for o in range(n):
    objs[o].bbox_min[:], objs[o].bbox_max[:] = [float(v) for v in boxes[o, 0]], [float(v) for v in boxes[o, 1]]
    objs[o].offset[:] = [float(v) for v in offs[o].reshape(-1)]
    objs[o].axis_scale = float(axis_scale)
    objs[o].box_color[:] = objs[o].fill_color[:] = [int(v) for v in cols[o]]
    objs[o].axis_color[:] = [int(v) for v in axis_cols.reshape(-1)]
  if out is None:
    dst = torch.empty_like(src)
  elif is_np:
    if not isinstance(out, np.ndarray) or out.shape != (H, W, 3) or out.dtype != np.uint8:
      raise ValueError('out must be a (H,W,3) uint8 numpy array like img')
    dst = src                                        # (the upload is a scratch copy: drawn in place, copied back below)
  else:
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3) or out.device != dev or not out.is_contiguous():
      raise ValueError('out must be a contiguous (H,W,3) uint8 tensor on the device of img')
    dst = out
    if out is img and src is not img:                # a non-contiguous img cannot be drawn in place
      raise ValueError('in-place drawing needs a contiguous img')
  Kd, Kp = k_ptr(K)
  a = _lib.FpDrawArgs()
  a.struct_size = ctypes.sizeof(a)
  a.d_img_in, a.d_img_out, a.H, a.W, a.K = src.data_ptr(), dst.data_ptr(), H, W, Kd.ctypes.data
  a.d_poses, a.n_obj, a.objs, a.flags = (P.data_ptr() if n else None), n, ctypes.addressof(objs), flags
  a.box_thickness, a.axis_thickness, a.opacity, a.fill_alpha = float(box_thickness), float(axis_thickness), 1.0 - float(transparency), float(fill_alpha)
  a.d_owner = own.data_ptr() if own is not None else None
  check(lib().fp_draw_poses(ctx.handle, ctypes.byref(a), stream_ptr(dev)))
  if not is_np:
    return dst
  res = dst.cpu().numpy()
  if out is None:
    return res
  out[...] = res
  return out


def draw_xyz_axis(color, ob_in_cam, scale=0.1, K=np.eye(3), thickness=3, transparency=0, is_input_rgb=False):
  """src/Utils.py:675-710: the x, y, z axes of a pose, `scale` metres long, in red, green and blue on a COPY of the image `color` (BGR
  unless is_input_rgb)."""
  return draw_poses(color, K, np.asarray(ob_in_cam, dtype=np.float64).reshape(1, 4, 4), box=False, axes=True, axis_scale=scale, axis_thickness=thickness,
                    transparency=transparency, is_input_rgb=is_input_rgb)


def draw_posed_3d_box(K, img, ob_in_cam, bbox, line_color=(0, 255, 0), linewidth=2):
  """src/Utils.py:713-749: the 12 edges of `bbox` (2,3) at the pose, drawn INTO `img` (a numpy array or a device tensor), which is also
  returned, as cv2.line does - main.py:68-69 relies on it."""
  return draw_poses(img, K, np.asarray(ob_in_cam, dtype=np.float64).reshape(1, 4, 4), bboxes=np.asarray(bbox, dtype=np.float64).reshape(2, 3), box=True,
                    axes=False, box_thickness=linewidth, colors=np.asarray(line_color, dtype=np.float64), out=img)


# ---- distance between surfaces (fp_point_mesh_distance, fp_mesh_sample_surface, fp_distance_stats) -----------------------------------
def _surface_on(mesh, vertices, faces, dev, what):
  """(pos float32 (V,3), faces int32 (F,3)) on `dev` of mesh (an object with .vertices / .faces, or a (vertices, faces) tuple) or of the
  two arrays.  Face arrays that live on the host are validated up front; device faces are checked by the kernels (a face with an index
  outside [0, V) is never followed)."""
  if mesh is not None:
    vertices, faces = _mesh_parts(mesh)[:2]
  if vertices is None or faces is None:
    raise ValueError(f'{what} needs a mesh, or vertices and faces')
  pos = torch.as_tensor(vertices).to(device=dev, dtype=torch.float).reshape(-1, 3).contiguous()
  if not (torch.is_tensor(faces) and faces.is_cuda):
    f = np.asarray(faces.cpu() if torch.is_tensor(faces) else faces)
    if f.size and (not np.issubdtype(f.dtype, np.integer) or f.min() < 0 or f.max() >= len(pos)):
      raise ValueError(f'{what}: faces must be integers in [0, {len(pos)})')
  fc = _faces_on(faces, dev)
  if len(pos) < 1 or len(fc) < 1:
    raise ValueError(f'{what}: the mesh has {len(pos)} vertices and {len(fc)} faces (at least one of each)')
  if len(fc) > _lib.FP_SURFDIST_MAX_FACES:
    raise ValueError(f'{what}: {len(fc)} faces (at most {_lib.FP_SURFDIST_MAX_FACES})')
  return pos, fc


def _point_mesh_distance_on(pts, pos, fc, want_face=False, want_closest=False):
  dev, n = pts.device, len(pts)
  dist = torch.empty(n, dtype=torch.float, device=dev)
  face = torch.empty(n, dtype=torch.int32, device=dev) if want_face else None
  closest = torch.empty((n, 3), dtype=torch.float, device=dev) if want_closest else None
  check(lib().fp_point_mesh_distance(_lib.Context.get(dev).handle, ptr(pts) if n else None, n, ptr(pos), len(pos), ptr(fc), len(fc),
                                     ptr(dist) if n else None, ptr(face) if n else None, ptr(closest) if n else None, stream_ptr(dev)))
  return dist, face, closest


def point_mesh_distance(points, mesh=None, vertices=None, faces=None, return_face=False, return_closest=False):
  """The exact distance from every point to the surface of a triangle mesh on the device (fp_point_mesh_distance): the minimum over ALL
  faces of the point-to-triangle distance, in fp32 - not the distance to the nearest vertex or sample, which depends on the tessellation.

  points (N,3); the mesh as `mesh` (an object with .vertices and .faces, or a (vertices, faces) tuple) or as `vertices` (V,3) and `faces`
  (F,3).  numpy in -> numpy out, device tensor in -> device tensor out.  Returns dist (N,) float32 and, as asked, face (N,) int32 (the
  nearest face; among faces at equal distance the lowest index) and closest (N,3) float32 (the nearest point on it).  A point with a
  non-finite coordinate gets NaN, -1, NaN.  Brute force, N x F pair tests; with device tensors nothing
  synchronises."""
  dev = _device_of(points)
  pts = torch.as_tensor(points).to(device=dev, dtype=torch.float).reshape(-1, 3).contiguous()
  if len(pts) > _lib.FP_SURFDIST_MAX_POINTS:
    raise ValueError(f'point_mesh_distance: {len(pts)} points (at most {_lib.FP_SURFDIST_MAX_POINTS})')
  pos, fc = _surface_on(mesh, vertices, faces, dev, 'point_mesh_distance')
  out = _point_mesh_distance_on(pts, pos, fc, return_face, return_closest)
  out = [o for o in out if o is not None]
  if not (torch.is_tensor(points) and points.is_cuda):
    out = [o.cpu().numpy() for o in out]
  return out[0] if len(out) == 1 else tuple(out)


def _sample_surface_on(pos, fc, n, seed, want_face=False, want_bary=False, want_area_q=False):
  dev = pos.device
  if not 0 <= n <= _lib.FP_SURFDIST_MAX_SAMPLES:
    raise ValueError(f'sample_surface: n {n} (0 .. {_lib.FP_SURFDIST_MAX_SAMPLES})')
  pts = torch.empty((n, 3), dtype=torch.float, device=dev)
  face = torch.empty(n, dtype=torch.int32, device=dev) if want_face else None
  bary = torch.empty((n, 2), dtype=torch.float, device=dev) if want_bary else None
  area_q = torch.empty(len(fc), dtype=torch.int64, device=dev) if want_area_q else None
  check(lib().fp_mesh_sample_surface(_lib.Context.get(dev).handle, ptr(pos), len(pos), ptr(fc), len(fc), n, int(seed) & 0xffffffff,
                                     ptr(pts) if n else None, ptr(face) if n else None, ptr(bary) if n else None, ptr(area_q), stream_ptr(dev)))
  return pts, face, bary, area_q


def sample_surface(mesh, n, seed=0, return_face=False, return_info=False):
  """n points on the surface of a mesh, on the device (fp_mesh_sample_surface): area-weighted and stratified along the face order (every
  face gets its area share of the samples to within one), a function of (mesh, n, seed) alone - the same bits on every run.

  mesh: an object with .vertices and .faces, or a (vertices, faces) tuple, numpy or torch.  Returns points (n,3) float32 on the device of
  the vertices (the current device for numpy) and, as asked, face (n,) int32 and info = {'bary': (n,2) float32 (u, v) with
  p = a + u (b - a) + v (c - a), 'area_q': (F,) int64, the device's table of face areas in units of 2^-40 of the total}.  A mesh
  without area raises.  The call synchronises once (the library reads the total area)."""
  vertices = _mesh_parts(mesh)[0]
  dev = _device_of(vertices)
  pos, fc = _surface_on(mesh, None, None, dev, 'sample_surface')
  pts, face, bary, area_q = _sample_surface_on(pos, fc, int(n), seed, return_face, return_info, return_info)
  out = [pts] + ([face] if return_face else []) + ([dict(bary=bary, area_q=area_q)] if return_info else [])
  return out[0] if len(out) == 1 else tuple(out)


def _distance_stats_on(dist, taus):
  """d_stats of fp_distance_stats as a device tensor of FP_SURFDIST_STATS_TAU0 + len(taus) doubles; nothing synchronises"""
  dev = dist.device
  th = np.ascontiguousarray(np.asarray(taus, dtype=np.float64).reshape(-1))
  if len(th) > _lib.FP_SURFDIST_MAX_TAUS:
    raise ValueError(f'at most {_lib.FP_SURFDIST_MAX_TAUS} thresholds ({len(th)} given)')
  stats = torch.empty(_lib.FP_SURFDIST_STATS_TAU0 + len(th), dtype=torch.float64, device=dev)
  check(lib().fp_distance_stats(_lib.Context.get(dev).handle, ptr(dist) if len(dist) else None, len(dist), ptr(th) if len(th) else None, len(th),
                                ptr(stats), stream_ptr(dev)))
  return stats


def distance_stats(dist, taus=()):
  """Statistics of a distance array on the device (fp_distance_stats), deterministic (no float atomics): {'n': finite entries,
  'not_finite': the others (left out of everything), 'sum', 'sum_sq', 'max', 'within': [count of d <= tau per tau]}.  Synchronises."""
  d = torch.as_tensor(dist).to(device=_device_of(dist), dtype=torch.float).reshape(-1).contiguous()
  s = _distance_stats_on(d, taus).cpu().numpy()
  L = _lib
  return dict(n=int(s[L.FP_SURFDIST_STATS_COUNT]), not_finite=int(s[L.FP_SURFDIST_STATS_NOT_FINITE]), sum=float(s[L.FP_SURFDIST_STATS_SUM]),
              sum_sq=float(s[L.FP_SURFDIST_STATS_SUM_SQ]), max=float(s[L.FP_SURFDIST_STATS_MAX]),
              within=[int(x) for x in s[L.FP_SURFDIST_STATS_TAU0:]])


def mesh_distance(mesh_a, mesh_b, n_samples=100_000, seed=0, taus=(0.001, 0.002, 0.005), use_vertices=True, align=False):
  """How far apart two meshes are, measured on the device: Chamfer and Hausdorff distance and precision / recall / F-score.

  The points of A are its vertices (use_vertices) plus n_samples surface samples (sample_surface, seeded); each is measured against B's
  TRIANGLES with point_mesh_distance - exact point-to-surface distances, independent of B's tessellation - and the same from B to A.
  Returns a dict:
    'a_to_b', 'b_to_a'   {'n', 'mean', 'rms', 'max'} of the distances of that direction (n: the points with a finite distance)
    'chamfer'            a_to_b.mean + b_to_a.mean: the SUM of the two mean UNSQUARED distances, in the meshes' unit.  (Conventions
                         differ: some report the mean of the two, or sums of squared distances; convert with the four numbers above.)
    'hausdorff'          the larger of the two maxima (over the measured points, so a lower bound of the true value that tightens with
                         n_samples)
    'taus'               the thresholds, and per threshold:
    'precision'          the share of A's points within tau of B;  'recall': the share of B's points within tau of A
    'fscore'             their harmonic mean, 0 when both are 0
  With A a reconstruction and B the CAD model this is the usual reporting of model-free results.  Meshes: objects with .vertices and
  .faces or (vertices, faces) tuples.  The statistics are deterministic sums (fp_distance_stats) and are read back together at the end;
  sampling a mesh synchronises once more per mesh (the library reads its total area).

  align: False measures the meshes as they lie.  True first lays A onto B with align_to_mesh(mesh_a, mesh_b) - for meshes of one object
  in two frames, such as a reconstruction with estimated poses against its CAD model; A should be the partial surface, B the complete
  one - and a (4,4) array is used as that transform, `B from A`.  The result then also holds 'a_to_b_transform' (4,4) float64 and, for
  True, 'align_info' (align_to_mesh's: look at 'ambiguous')."""
  n_samples = int(n_samples)
  if n_samples < 0 or (n_samples == 0 and not use_vertices):
    raise ValueError('mesh_distance: nothing to measure (n_samples = 0 and use_vertices = False)')
  if align is not False and align is not None:
    if align is True:
      T, align_info = align_to_mesh(mesh_a, mesh_b, seed=seed)
      extra = dict(a_to_b_transform=T, align_info=align_info)
    else:
      T = np.asarray(align.cpu() if torch.is_tensor(align) else align, dtype=np.float64).reshape(4, 4)
      extra = dict(a_to_b_transform=T)
    va, fa = _mesh_parts(mesh_a)[:2]
    va = np.asarray(va.cpu() if torch.is_tensor(va) else va, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]
    return dict(mesh_distance((va, fa), mesh_b, n_samples=n_samples, seed=seed, taus=taus, use_vertices=use_vertices), **extra)
  dev = _device_of(_mesh_parts(mesh_a)[0])
  surf = [_surface_on(m, None, None, dev, 'mesh_distance') for m in (mesh_a, mesh_b)]
  pts = []
  for k, (pos, fc) in enumerate(surf):
    parts = [pos] if use_vertices else []
    if n_samples:
      parts.append(_sample_surface_on(pos, fc, n_samples, seed)[0])
    pts.append(parts[0] if len(parts) == 1 else torch.cat(parts))
  taus = [float(t) for t in taus]
  stats = torch.stack([_distance_stats_on(_point_mesh_distance_on(pts[k], *surf[1 - k])[0], taus) for k in (0, 1)]).cpu().numpy()
  L = _lib

  def side(s):
    n = s[L.FP_SURFDIST_STATS_COUNT]
    return dict(n=int(n), mean=float(s[L.FP_SURFDIST_STATS_SUM] / n) if n else float('nan'),
                rms=float(math.sqrt(s[L.FP_SURFDIST_STATS_SUM_SQ] / n)) if n else float('nan'), max=float(s[L.FP_SURFDIST_STATS_MAX]))

  def share(s, k):
    return float(s[L.FP_SURFDIST_STATS_TAU0 + k] / s[L.FP_SURFDIST_STATS_COUNT]) if s[L.FP_SURFDIST_STATS_COUNT] else 0.0

  ab, ba = side(stats[0]), side(stats[1])
  precision = [share(stats[0], k) for k in range(len(taus))]
  recall = [share(stats[1], k) for k in range(len(taus))]
  fscore = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(precision, recall)]
  return dict(a_to_b=ab, b_to_a=ba, chamfer=ab['mean'] + ba['mean'], hausdorff=max(ab['max'], ba['max']), taus=taus, precision=precision,
              recall=recall, fscore=fscore)


# ---- symmetries of a model (fp_symmetry_residuals; the search itself is foundationpose_amd/symmetry.py, host float64) ------------------
def _symmetry_residuals_on(pts, tfs, pos, fc, taus=(), want_q=False, want_dist=False):
  """d_stats of fp_symmetry_residuals as a device tensor (T, FP_SURFDIST_STATS_TAU0 + len(taus)) float64, and d_q, d_dist as asked;
  pts (n,3) float32, tfs (T,3,4) float32, on the device of the mesh.  Nothing synchronises."""
  dev, n, T = pos.device, len(pts), len(tfs)
  th = np.ascontiguousarray(np.asarray(taus, dtype=np.float64).reshape(-1))
  if len(th) > _lib.FP_SURFDIST_MAX_TAUS:
    raise ValueError(f'at most {_lib.FP_SURFDIST_MAX_TAUS} thresholds ({len(th)} given)')
  if T < 1 or T * n > _lib.FP_SURFDIST_MAX_POINTS:
    raise ValueError(f'symmetry_residuals: {T} transforms of {n} points (at least one transform, at most {_lib.FP_SURFDIST_MAX_POINTS} queries)')
  stats = torch.empty((T, _lib.FP_SURFDIST_STATS_TAU0 + len(th)), dtype=torch.float64, device=dev)
  q = torch.empty((T * n, 3), dtype=torch.float, device=dev) if want_q else None
  dist = torch.empty(T * n, dtype=torch.float, device=dev) if want_dist else None
  check(lib().fp_symmetry_residuals(_lib.Context.get(dev).handle, ptr(pts) if n else None, n, ptr(tfs), T, ptr(pos), len(pos), ptr(fc), len(fc),
                                    ptr(th) if len(th) else None, len(th), ptr(stats), ptr(q) if n else None, ptr(dist) if n else None,
                                    stream_ptr(dev)))
  return stats, q, dist


def _tfs_f32_on(tfs, dev):
  """(S,4,4) transforms -> (S,3,4) float32 [R|t] on dev: float64 on the host, rounded to fp32 once"""
  t = np.asarray(tfs.cpu() if torch.is_tensor(tfs) else tfs, dtype=np.float64).reshape(-1, 4, 4)
  return torch.as_tensor(np.ascontiguousarray(t[:, :3, :].astype(np.float32)), device=dev)


def _stats_dict(s):
  L = _lib
  n = s[:, L.FP_SURFDIST_STATS_COUNT]
  with np.errstate(invalid='ignore', divide='ignore'):
    mean = np.where(n > 0, s[:, L.FP_SURFDIST_STATS_SUM] / n, np.nan)
    rms = np.where(n > 0, np.sqrt(s[:, L.FP_SURFDIST_STATS_SUM_SQ] / n), np.nan)
  return dict(n=n.astype(np.int64), not_finite=s[:, L.FP_SURFDIST_STATS_NOT_FINITE].astype(np.int64), max=s[:, L.FP_SURFDIST_STATS_MAX].copy(),
              mean=mean, rms=rms, within=s[:, L.FP_SURFDIST_STATS_TAU0:].astype(np.int64))


def symmetry_residuals(mesh=None, vertices=None, faces=None, tfs=None, n_samples=4096, seed=0, taus=()):
  """How far a mesh is from itself under each of S rigid transforms, on the device (fp_symmetry_residuals): n_samples surface samples
  (sample_surface: a function of the mesh, n_samples and seed alone) are moved by every transform and measured against the mesh's
  triangles, exactly (point_mesh_distance's rule), in one launch; only the statistics come back.

  The mesh as `mesh` (.vertices / .faces or a (vertices, faces) tuple) or as vertices and faces; tfs (S,4,4), taken as float64 and
  rounded to fp32 once.  Returns a dict of numpy arrays over the transforms: 'max', 'mean', 'rms' (float64; NaN where no distance is
  finite), 'n' and 'not_finite' (counts), 'within' (S, len(taus)): the number of samples within each tau.  A symmetry of the mesh has
  max about 0 (fp32 rounding); what a value means otherwise is up to the caller.  Synchronises (the sampler once, the read-back once)."""
  if tfs is None:
    raise ValueError('symmetry_residuals needs tfs')
  v = _mesh_parts(mesh)[0] if mesh is not None else vertices
  dev = _device_of(v)
  pos, fc = _surface_on(mesh, vertices, faces, dev, 'symmetry_residuals')
  pts = _sample_surface_on(pos, fc, int(n_samples), seed)[0]
  stats = _symmetry_residuals_on(pts, _tfs_f32_on(tfs, dev), pos, fc, taus)[0]
  return _stats_dict(stats.cpu().numpy())


SYMMETRY_TOL_FRACTION = 0.02       # find_symmetries' default tol as a share of the exact diameter: this project's choice


def find_symmetries(mesh, tol=None, max_order=12, angle_step_deg=1.0, n_samples=4096, n_coarse=512, seed=0, rot_angle_discrete=5,
                    max_group=128):
  """The rotational symmetries of a mesh: what a hand-edited models_info.json supplies for a CAD model, found for any mesh - a
  reconstructed one included.  Proper rotations only (a reflection is not a pose).  The search runs on the host in float64
  (foundationpose_amd/symmetry.py); every residual it looks at comes from the device (fp_symmetry_residuals): the largest distance from
  the mesh's surface samples, moved by a candidate, to the mesh's triangles.  A transform is ACCEPTED when that maximum is <= tol.

  Pivot and axes: the area-weighted centroid and covariance of the surface, in closed form per triangle.  Every rotational symmetry fixes
  the centroid and commutes with the covariance, so an axis of order >= 3 is an eigenvector and a 2-fold axis is an eigenvector or lies
  in the plane of two equal eigenvalues.  Candidates, for each of the three eigenvectors a (so no eigenvalue gap is thresholded):
  rotations about a by 2 pi m / k, k = 2 .. max_order (order k stands only when EVERY multiple of 2 pi / k passes); rotations about a by
  every multiple of angle_step_deg - if ALL pass, a is a
  continuous axis; 2-fold rotations about the axes of the plane perpendicular to a, on a grid of angle_step_deg, every local minimum of
  the mean residual refined by halving to angle_step_deg / 64.  All candidates are scored on n_coarse samples in one call, the survivors
  verified on n_samples in a second, the accepted set closed under composition (elements closer than half a step are one; elements that
  differ by a rotation about a continuous axis are one), and every element the closure adds is verified too.  More than max_group
  discrete elements raise ValueError.

  tol: in the mesh's unit; None is SYMMETRY_TOL_FRACTION = 0.02 x mesh_diameter (exact) - this project's own choice, wide enough for the
  noise of a 2 mm fusion on a hand-sized object; a CAD model takes a much smaller one.

  Returns a dict:
    'symmetry_tfs'           (S,4,4) float64 in the mesh's frame, what FoundationPose(symmetry_tfs=), pose_errors and bop_pose_errors
                             take: the identity first, every transform fixing the centroid; a continuous axis is sampled every
                             rot_angle_discrete degrees and multiplied with the discrete elements
    'symmetries_discrete'    models_info.json's form: each discrete element but the identity as its 4x4 matrix, row-major, 16 numbers,
                             the translation in MILLIMETRES (the mesh is in metres)
    'symmetries_continuous'  [{'axis': the unit axis, 'offset': a point on it (the centroid) in millimetres}] or []
    'centroid', 'eigenvalues' (ascending), 'axes' (rows: the eigenvectors)
    'max', 'mean'            (S,) the residuals of every element of symmetry_tfs on n_samples samples
    'n_candidates', 'tol', 'closed' (False: the closure produced an element that did not verify and was left out),
    'continuous_axes'        the eigenvectors about which every rotation passed (more than one: a sphere; the first is used)
  When all three eigenvalues are nearly equal (a cube, a sphere) the principal axes are arbitrary and the result may be INCOMPLETE: what
  is returned verifies - it is never wrong, only possibly partial - and 'eigenvalues' shows the case.  The same mesh and arguments give
  the same bits on every run.  Synchronises several times (cold path)."""
  from . import symmetry as _sym
  vertices, faces = _mesh_parts(mesh)[:2]
  dev = _device_of(vertices)
  pos, fc = _surface_on(mesh, None, None, dev, 'find_symmetries')
  if tol is None:
    tol = SYMMETRY_TOL_FRACTION * mesh_diameter(model_pts=pos)
  tol = float(tol)
  if not tol >= 0:
    raise ValueError(f'find_symmetries: tol {tol}')
  samples = {}

  def residuals(tfs, n):
    if n not in samples:
      samples[n] = _sample_surface_on(pos, fc, int(n), seed)[0]
    tfs = np.asarray(tfs, dtype=np.float64).reshape(-1, 4, 4)
    per_call = max(1, _lib.FP_SURFDIST_MAX_POINTS // max(int(n), 1))
    parts = [_symmetry_residuals_on(samples[n], _tfs_f32_on(tfs[s0:s0 + per_call], dev), pos, fc)[0] for s0 in range(0, len(tfs), per_call)]
    d = _stats_dict(torch.cat(parts).cpu().numpy())
    bad = d['not_finite'] > 0
    return np.where(bad, np.inf, d['max']), np.where(bad, np.inf, d['mean'])

  v = pos.cpu().numpy().astype(np.float64)
  return _sym.find_symmetries(v, fc.cpu().numpy(), residuals, tol, max_order=max_order, angle_step_deg=angle_step_deg, n_samples=n_samples,
                              n_coarse=n_coarse, rot_angle_discrete=rot_angle_discrete, max_group=max_group)
