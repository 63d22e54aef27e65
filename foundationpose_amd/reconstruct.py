"""Model-free set-up: a handful of posed RGB-D reference views of an object, with masks, fused into a mesh that goes where a CAD model
goes - make_mesh_tensors and FoundationPose(model_pts, model_normals, mesh=...).

The reference trains a neural object field for this (bundlesdf/run_nerf.py: run_one_ob -> model/model.obj).  This module reads the same
folder layout and does something else: the depth maps are fused into a truncated signed distance volume and a
coloured triangle mesh is extracted by marching tetrahedra, both on the GPU (csrc/tsdf.hip; the arithmetic is stated in
include/foundationpose_amd.h).  The poses of the reference views can be refined first (refine_view_poses, reconstruct_object(...,
refine_poses=True)): each view's depth map is aligned rigidly to the geometry fused so far, frame-to-model Gauss-Newton on the volume
(fp_tsdf_align builds the normal equations on the GPU, the 6x6 solves run on the host).  They can also be refined jointly, or estimated
when the folder has none, from depth alone: point-to-plane ICP between pairs of depth maps, linearised for all pairs in one launch
(fp_depth_pairs_align, csrc/depth_icp.hip) and solved for all views at once on the host (joint_refine_view_poses, estimate_view_poses).
Joint geometric alignment; still no photometric term and no view-dependent appearance.
"""
import ctypes
import glob
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .synthetic import SimpleMesh

MAX_POINTS, MAX_VIEWS = _lib.FP_TSDF_MAX_POINTS, _lib.FP_TSDF_MAX_VIEWS


def _device(device):
  d = torch.device(device)
  return torch.device('cuda', d.index if d.index is not None else torch.cuda.current_device())


class TsdfVolume:
  """fp_tsdf: sample point (i, j, k) lies at origin + voxel_size * (i, j, k) in the object frame (metres); dims = (nx, ny, nz)."""

  def __init__(self, origin, voxel_size, dims, trunc=None, device='cuda'):
    self.device = _device(device)
    self.ctx = _lib.Context.get(self.device)
    self.origin = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))
    self.voxel_size = float(voxel_size)
    self.trunc = 4.0 * self.voxel_size if trunc is None else float(trunc)
    self.dims = tuple(int(d) for d in dims)
    dims_c = (ctypes.c_int * 3)(*self.dims)
    h = ctypes.c_void_p()
    check(lib().fp_tsdf_create(self.ctx.handle, ptr(self.origin), self.voxel_size, dims_c, self.trunc, ctypes.byref(h)))
    self.handle = h

  def __del__(self):
    try:
      if self.handle:
        lib().fp_tsdf_destroy(self.handle)
        self.handle = None
    except Exception:
      pass

  def reset(self):
    check(lib().fp_tsdf_reset(self.ctx.handle, self.handle, stream_ptr(self.device)))

  def integrate(self, depths, K, cam_in_obs, rgbs=None, masks=None, zfar=np.inf):
    """depths (n,H,W) metres; cam_in_obs (n,4,4) camera-to-object; rgbs (n,H,W,3) uint8; masks (n,H,W), non-zero = object.  numpy
    arrays or device tensors.  More than MAX_VIEWS views are cut into calls: the result is the same bits (the header's promise)."""
    depths = torch.as_tensor(depths, device=self.device).to(torch.float).contiguous()
    if depths.dim() == 2:
      depths = depths[None]
    n, H, W = depths.shape
    poses = np.ascontiguousarray(np.asarray(torch.as_tensor(cam_in_obs).cpu(), dtype=np.float64).reshape(-1, 4, 4))
    if len(poses) != n:
      raise ValueError(f'{n} depth maps, {len(poses)} poses')
    if rgbs is not None:
      rgbs = torch.as_tensor(rgbs, device=self.device)
      if rgbs.dtype != torch.uint8 or tuple(rgbs.shape) != (n, H, W, 3):
        raise ValueError(f'rgbs must be uint8 of shape {(n, H, W, 3)}, got {rgbs.dtype} {tuple(rgbs.shape)}')
      rgbs = rgbs.contiguous()
    if masks is not None:
      masks = torch.as_tensor(masks, device=self.device)
      if tuple(masks.shape) != (n, H, W):
        raise ValueError(f'masks must have the shape {(n, H, W)}, got {tuple(masks.shape)}')
      masks = (masks != 0).to(torch.uint8).contiguous()
    Kd, Kp = _lib.k_ptr(K)
    zf = float(zfar) if np.isfinite(zfar) else float('inf')
    for a in range(0, n, MAX_VIEWS):
      b = min(a + MAX_VIEWS, n)
      check(lib().fp_tsdf_integrate(self.ctx.handle, self.handle, ptr(depths[a:b]), None if rgbs is None else ptr(rgbs[a:b]),
                                    None if masks is None else ptr(masks[a:b]), b - a, H, W, Kp, ptr(poses[a:b]), zf, stream_ptr(self.device)))

  def _views(self, depths, cam_in_obs, masks):
    depths = torch.as_tensor(depths, device=self.device).to(torch.float).contiguous()
    if depths.dim() == 2:
      depths = depths[None]
    n, H, W = depths.shape
    poses = np.ascontiguousarray(np.asarray(torch.as_tensor(cam_in_obs).cpu(), dtype=np.float64).reshape(-1, 4, 4))
    if len(poses) != n:
      raise ValueError(f'{n} depth maps, {len(poses)} poses')
    if masks is not None:
      masks = torch.as_tensor(masks, device=self.device)
      if tuple(masks.shape) != (n, H, W):
        raise ValueError(f'masks must have the shape {(n, H, W)}, got {tuple(masks.shape)}')
      masks = (masks != 0).to(torch.uint8).contiguous()
    return depths, poses, masks

  def align_step(self, depths, K, cam_in_obs, masks=None, zfar=np.inf, min_weight=1, rows=False):
    """One linearisation of every view's pose against the volume (fp_tsdf_align; arguments as for integrate): the (n,29) float64 array
    of the header - per view the upper triangle of J^T J, J^T r, sum r^2, the number of valid pixels - and, with rows=True, the
    (n,H,W,8) float32 device tensor of the per-pixel rows.  Synchronises.  More than MAX_VIEWS views are cut into calls (a view's
    numbers do not depend on the batch it is in)."""
    depths, poses, masks = self._views(depths, cam_in_obs, masks)
    n, H, W = depths.shape
    Kd, Kp = _lib.k_ptr(K)
    zf = float(zfar) if np.isfinite(zfar) else float('inf')
    sums = np.zeros((n, _lib.FP_TSDF_ALIGN_TERMS), dtype=np.float64)
    out = torch.empty((n, H, W, 8), dtype=torch.float, device=self.device) if rows else None
    for a in range(0, n, MAX_VIEWS):
      b = min(a + MAX_VIEWS, n)
      part = np.zeros((b - a, _lib.FP_TSDF_ALIGN_TERMS), dtype=np.float64)
      check(lib().fp_tsdf_align(self.ctx.handle, self.handle, ptr(depths[a:b]), None if masks is None else ptr(masks[a:b]), b - a, H, W, Kp,
                                ptr(poses[a:b]), zf, float(min_weight), None if out is None else ptr(out[a:b]), ptr(part),
                                stream_ptr(self.device)))
      sums[a:b] = part
    return (sums, out) if rows else sums

  def align(self, depths, K, cam_in_obs, masks=None, iterations=10, min_pixels=100, damping=1e-9, max_step=None, zfar=np.inf, min_weight=1):
    """Frame-to-model alignment of n views to the volume: Gauss-Newton on the host in float64 over the sums of align_step - per view
    (A + damping trace(A) I) xi = -b, pose <- expm_se3(xi) @ pose - with ALL views advanced by one fp_tsdf_align call per iteration
    (`iterations` steps and one closing evaluation).  A view with fewer than min_pixels valid pixels, or whose RMS residual rose, goes
    back to the pose it had before its last step and stops.  max_step = (metres, radians) scales a step down to that translation and
    rotation.  Returns (cam_in_obs (n,4,4) float64, info) with info['valid'] and info['rms'] (evaluations, n), info['stopped'] {view:
    reason} and info['after_first'], the poses after the first step."""
    depths, poses, masks = self._views(depths, cam_in_obs, masks)
    poses = poses.copy()
    n = len(poses)
    prev_pose, prev_rms = poses.copy(), np.full(n, np.inf)
    active = np.ones(n, dtype=bool)
    info = dict(valid=[], rms=[], stopped={}, after_first=None)
    for it in range(iterations + 1):
      if not active.any():
        break
      s = self.align_step(depths, K, poses, masks=masks, zfar=zfar, min_weight=min_weight)
      cnt = s[:, 28]
      rms = np.sqrt(s[:, 27] / np.maximum(cnt, 1))
      info['valid'].append(cnt.copy())
      info['rms'].append(rms.copy())
      for v in range(n):
        if not active[v]:
          continue
        if cnt[v] < min_pixels:
          poses[v], active[v], info['stopped'][v] = prev_pose[v], False, 'too few valid pixels'
        elif rms[v] > prev_rms[v]:
          poses[v], active[v], info['stopped'][v] = prev_pose[v], False, 'residual rose'
        elif it < iterations:
          prev_pose[v], prev_rms[v] = poses[v], rms[v]
          xi = solve_step(s[v], damping)
          if max_step is not None:
            xi = xi * min(1.0, max_step[0] / max(np.linalg.norm(xi[:3]), 1e-300), max_step[1] / max(np.linalg.norm(xi[3:]), 1e-300))
          poses[v] = expm_se3(xi) @ poses[v]
      if it == 0:
        info['after_first'] = poses.copy()
    info['valid'], info['rms'] = np.array(info['valid']).reshape(-1, n), np.array(info['rms']).reshape(-1, n)
    return poses, info

  def plane(self, name):
    """A copy of one plane as a (nz, ny, nx) float32 device tensor: 'tsdf', 'weight', 'r', 'g', 'b' or 'color_weight'."""
    nx, ny, nz = self.dims
    out = torch.empty((nz, ny, nx), dtype=torch.float, device=self.device)
    check(lib().fp_tsdf_read_plane(self.ctx.handle, self.handle, _lib.FP_TSDF_PLANES.index(name), ptr(out), stream_ptr(self.device)))
    return out

  tsdf = property(lambda self: self.plane('tsdf'))
  weight = property(lambda self: self.plane('weight'))

  def extract_arrays(self, min_weight=1, normals=True, colors=True):
    """(vertices (V,3) float32, normals (V,3) float32 | None, colors (V,3) uint8 | None, faces (F,3) int32) on the device."""
    counts = (ctypes.c_int64 * 2)()
    check(lib().fp_tsdf_extract_count(self.ctx.handle, self.handle, float(min_weight), counts, stream_ptr(self.device)))
    nv, nf = int(counts[0]), int(counts[1])
    v = torch.empty((nv, 3), dtype=torch.float, device=self.device)
    nr = torch.empty((nv, 3), dtype=torch.float, device=self.device) if normals else None
    c = torch.empty((nv, 3), dtype=torch.uint8, device=self.device) if colors else None
    f = torch.empty((nf, 3), dtype=torch.int32, device=self.device)
    check(lib().fp_tsdf_extract_write(self.ctx.handle, self.handle, ptr(v), ptr(nr), ptr(c), ptr(f), nv, nf, stream_ptr(self.device)))
    return v, nr, c, f

  def extract_mesh(self, min_weight=1):
    """The surface as a synthetic.SimpleMesh with vertex normals and vertex colours (RGBA uint8, alpha 255)."""
    v, nr, c, f = self.extract_arrays(min_weight)
    rgba = np.concatenate([c.cpu().numpy(), np.full((len(c), 1), 255, dtype=np.uint8)], 1)
    return SimpleMesh(v.cpu().numpy(), f.cpu().numpy(), vertex_normals=nr.cpu().numpy(), vertex_colors=rgba)


def expm_se3(xi):
  """exp of the twist xi = (u, w) - translation part, rotation vector - as a 4x4 float64 matrix: R = I + A [w] + B [w]^2,
  t = (I + B [w] + C [w]^2) u with A = sin th / th, B = (1 - cos th) / th^2, C = (th - sin th) / th^3 (their series below 1e-4 rad)."""
  xi = np.asarray(xi, dtype=np.float64).reshape(6)
  u, w = xi[:3], xi[3:]
  th = float(np.linalg.norm(w))
  Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
  if th < 1e-4:
    A, B, C = 1 - th * th / 6, 0.5 - th * th / 24, 1 / 6 - th * th / 120
  else:
    A, B, C = np.sin(th) / th, (1 - np.cos(th)) / (th * th), (th - np.sin(th)) / th ** 3
  m = np.eye(4)
  m[:3, :3] = np.eye(3) + A * Kx + B * (Kx @ Kx)
  m[:3, 3] = (np.eye(3) + B * Kx + C * (Kx @ Kx)) @ u
  return m


def solve_step(sums, damping=1e-9):
  """The Gauss-Newton step of one view from its 29 sums: (A + damping trace(A) I) xi = -b."""
  A = np.zeros((6, 6))
  e = 0
  for i in range(6):
    for j in range(i, 6):
      A[i, j] = A[j, i] = sums[e]
      e += 1
  return np.linalg.solve(A + damping * np.trace(A) * np.eye(6), -np.asarray(sums[21:27]))


def volume_from_views(depths, masks, K, cam_in_obs, voxel_size, margin=None, device='cuda'):
  """The volume that holds what the views see of the object: the masked valid pixels are back-projected (Utils.depth2xyzmap), taken to
  the object frame, and their bounding box grown by `margin` (default 5 voxels).  Returns (origin (3,) float64, dims (3,) int).  Raises
  ValueError when no pixel is valid or when dims would exceed the library's maximum - the message names a voxel size that fits."""
  from .Utils import depth2xyzmap
  dev = _device(device)
  margin = 5.0 * voxel_size if margin is None else float(margin)
  depths = torch.as_tensor(depths, device=dev).to(torch.float)
  poses = torch.as_tensor(np.asarray(torch.as_tensor(cam_in_obs).cpu(), dtype=np.float64).reshape(-1, 4, 4), device=dev)
  lo = torch.full((3,), float('inf'), dtype=torch.float64, device=dev)
  hi = -lo
  for v in range(len(depths)):
    xyz = depth2xyzmap(depths[v].contiguous(), K)
    keep = xyz[..., 2] >= 0.001
    if masks is not None:
      keep &= torch.as_tensor(masks[v], device=dev) != 0
    pts = xyz[keep].to(torch.float64)
    if len(pts) == 0:
      continue
    pts = pts @ poses[v, :3, :3].T + poses[v, :3, 3]
    lo, hi = torch.minimum(lo, pts.min(0).values), torch.maximum(hi, pts.max(0).values)
  lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
  if not np.isfinite(lo).all():
    raise ValueError('volume_from_views: no valid masked depth pixel in any view')
  origin = lo - margin
  dims = np.ceil((hi - lo + 2 * margin) / voxel_size).astype(np.int64) + 1
  dims = np.maximum(dims, 2)
  if int(np.prod(dims)) > MAX_POINTS:
    fit = voxel_size * (float(np.prod(dims.astype(np.float64))) / MAX_POINTS) ** (1.0 / 3.0) * 1.05
    raise ValueError(f'volume_from_views: {dims[0]} x {dims[1]} x {dims[2]} sample points at voxel_size {voxel_size:g} exceed the maximum of '
                     f'{MAX_POINTS}; voxel_size {fit:.3g} would fit')
  return origin, dims


def load_reference_views(dir, depth_dir=None, mask_dir='mask', poses=True, masks=True):
  """The reference's folder of reference views (bundlesdf/run_nerf.py: run_one_ob): rgb/NAME.png; depth as 16-bit PNG in millimetres
  under `depth_dir` (default: depth_enhanced/ when it exists, else depth/), read as value / 1e3 in float64 and cast to float32;
  `mask_dir`/NAME.png (non-zero = object); cam_in_ob/NAME.txt (4x4, camera-to-object); K.txt.  Returns a dict: rgbs (n,H,W,3) uint8,
  depths (n,H,W) float32 metres, masks (n,H,W) uint8, K (3,3), cam_in_obs (n,4,4) float64, names.  poses=False does not read cam_in_ob/
  (a folder that is still to be posed: estimate_view_poses) and returns no cam_in_obs.  masks=False likewise does not read `mask_dir`
  (a folder that is still to be segmented: segment_views) and returns no masks."""
  from PIL import Image
  want_masks = masks
  files = sorted(glob.glob(os.path.join(dir, 'rgb', '*.png')))
  if not files:
    raise FileNotFoundError(f'no rgb/*.png under {dir}')
  if depth_dir is None:
    depth_dir = 'depth_enhanced' if os.path.isdir(os.path.join(dir, 'depth_enhanced')) else 'depth'
  names = [os.path.splitext(os.path.basename(f))[0] for f in files]
  rgbs, depths, masks, cams = [], [], [], []
  for name, f in zip(names, files):
    rgbs.append(np.asarray(Image.open(f).convert('RGB'), dtype=np.uint8))
    d = np.asarray(Image.open(os.path.join(dir, depth_dir, name + '.png')))
    if d.ndim != 2:
      raise ValueError(f'{depth_dir}/{name}.png is not a single-channel depth image')
    depths.append((d.astype(np.float64) / 1e3).astype(np.float32))
    if want_masks:
      m = np.asarray(Image.open(os.path.join(dir, mask_dir, name + '.png')))
      masks.append(((m if m.ndim == 2 else m.max(-1)) > 0).astype(np.uint8))
    if poses:
      cams.append(np.loadtxt(os.path.join(dir, 'cam_in_ob', name + '.txt')).reshape(4, 4))
  out = dict(rgbs=np.stack(rgbs), depths=np.stack(depths))
  if want_masks:
    out['masks'] = np.stack(masks)
  out.update(K=np.loadtxt(os.path.join(dir, 'K.txt')).reshape(3, 3), names=names)
  if poses:
    out['cam_in_obs'] = np.stack(cams)
  return out


def largest_component(faces, n_vertices):
  """Boolean (F,) mask of the faces of the connected component with the most faces (components of the vertex graph, scipy)."""
  from scipy.sparse import coo_matrix
  from scipy.sparse.csgraph import connected_components
  f = np.asarray(faces, dtype=np.int64)
  if len(f) == 0:
    return np.zeros(0, dtype=bool)
  rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
  g = coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(n_vertices, n_vertices))
  _, label = connected_components(g, directed=False)
  face_label = label[f[:, 0]]
  return face_label == np.bincount(face_label).argmax()


def _eroded_depths(views, depth_filter, dev):
  """The depth maps the ALIGNMENT runs on: erode_depth only (pixels at depth discontinuities dropped, none invented); raw without filter."""
  from .Utils import erode_depth
  depths = torch.as_tensor(views['depths'], device=dev).to(torch.float)
  if depth_filter:
    depths = torch.stack([erode_depth(d.contiguous(), radius=2, device=dev) for d in depths])
  return depths


def _fusion_depths(eroded, depth_filter, dev):
  """The depth maps the FUSION runs on: bilateral_filter_depth over the eroded maps, as the estimator does with an observed frame."""
  from .Utils import bilateral_filter_depth
  if depth_filter:
    return torch.stack([bilateral_filter_depth(d.contiguous(), radius=2, device=dev) for d in eroded])
  return eroded


def refine_view_poses(views, voxel_size=0.002, anchor=0, order='greedy', rounds=0, depth_filter=True, trunc=None, margin=None, iterations=10,
                      min_pixels=100, damping=1e-9, max_step=None, device='cuda'):
  """Rigid per-view refinement of the reference views' poses against the geometry they fuse into.  `views` as for reconstruct_object.
  The anchor view fixes the gauge and is never moved.  The volume holds all views at their given poses, grown by `margin` (default:
  5 voxels + 1 cm, for poses that are off by millimetres and a degree or two).  The anchor is integrated; then, until every view is
  fused: the view whose optical axis makes the smallest angle with that of any fused view (order='greedy'; 'index': the lowest index;
  or a sequence of view indices) is aligned to the volume as it stands (TsdfVolume.align) and integrated at its refined pose.
  Two things differ from the fusion of reconstruct_object, both measured.  `trunc` is 2 voxels by default, not 4:
  a point within the truncation distance BEHIND a surface that the model has seen from elsewhere (the side face next to an edge)
  carries a residual that is an artefact of the projective distance, so the band is kept as narrow as the interpolation allows; it must
  stay above the pose error to be recovered.  depth_filter runs erode_depth only, which drops pixels at depth discontinuities; the
  bilateral filter also fills the eroded silhouette from the neighbours, and a model of few views fused from such maps pulls the
  alignment off.  rounds > 0 appends whole-model rounds: everything is fused again at the current poses and all views but the anchor are
  aligned in one batched call.  A view that cannot be aligned (too few valid pixels) is integrated at its given pose and named in
  info['stopped']; the call does not raise for that.  Returns (cam_in_obs (n,4,4) float64, info: order, stopped {view: reason}, valid
  and rms per view at its last evaluation)."""
  if isinstance(views, (str, os.PathLike)):
    views = load_reference_views(views)
  dev = _device(device)
  return _refine_on(_eroded_depths(views, depth_filter, dev), views, voxel_size, anchor, order, rounds, trunc, margin,
                    dict(iterations=iterations, min_pixels=min_pixels, damping=damping, max_step=max_step), dev)


def _refine_on(depths, views, voxel_size, anchor, order, rounds, trunc, margin, kw, dev):
  """refine_view_poses on depth maps that are already prepared for the alignment (device tensor (n,H,W)); kw: TsdfVolume.align's."""
  trunc = 2.0 * voxel_size if trunc is None else float(trunc)
  masks, K = views.get('masks'), views['K']
  poses = np.array(np.asarray(torch.as_tensor(views['cam_in_obs']).cpu(), dtype=np.float64).reshape(-1, 4, 4))
  n = len(poses)
  if not 0 <= anchor < n:
    raise ValueError(f'anchor {anchor} of {n} views')
  margin = 5.0 * voxel_size + 0.01 if margin is None else float(margin)
  origin, dims = volume_from_views(depths, masks, K, poses, voxel_size, margin=margin, device=dev)
  vol = TsdfVolume(origin, voxel_size, dims, trunc=trunc, device=dev)
  one = lambda a, v: None if a is None else a[v:v + 1]
  vol.integrate(depths[anchor:anchor + 1], K, poses[anchor:anchor + 1], masks=one(masks, anchor))
  fused, left = [anchor], [v for v in range(n) if v != anchor]
  if not isinstance(order, str):
    left = [int(v) for v in order if int(v) != anchor]
    if sorted(left) != [v for v in range(n) if v != anchor]:
      raise ValueError('order must name every view but the anchor once')
  elif order not in ('greedy', 'index'):
    raise ValueError(f"order must be 'greedy', 'index' or a sequence of view indices, got {order!r}")
  info = dict(order=[anchor], stopped={}, valid=np.zeros(n), rms=np.zeros(n))
  while left:
    v = left[0]
    if order == 'greedy':
      cos = [max(float(poses[c, :3, 2] @ poses[u, :3, 2]) for u in fused) for c in left]
      v = left[int(np.argmax(cos))]          # the first of equals: the lowest index
    got, inf = vol.align(depths[v:v + 1], K, poses[v:v + 1], masks=one(masks, v), **kw)
    poses[v] = got[0]
    if 0 in inf['stopped']:
      info['stopped'][v] = inf['stopped'][0]
    info['valid'][v], info['rms'][v] = inf['valid'][-1, 0], inf['rms'][-1, 0]
    vol.integrate(depths[v:v + 1], K, poses[v:v + 1], masks=one(masks, v))
    left.remove(v)
    fused.append(v)
    info['order'].append(v)
  others = [v for v in range(n) if v != anchor]
  for _ in range(rounds if others else 0):
    vol.reset()
    vol.integrate(depths, K, poses, masks=masks)
    got, inf = vol.align(depths[others], K, poses[others], masks=None if masks is None else torch.as_tensor(masks)[others], **kw)
    poses[others] = got
    for k, v in enumerate(others):
      if k in inf['stopped']:
        info['stopped'][v] = inf['stopped'][k]
      info['valid'][v], info['rms'][v] = inf['valid'][-1, k], inf['rms'][-1, k]
  return poses, info


# ---- posing views from depth alone: pairwise point-to-plane ICP, solved jointly (csrc/depth_icp.hip) ----------------------------------
DEFAULT_STAGES = ((0.020, 0.5, 6), (0.010, 0.5, 6), (0.005, 0.7, 8))            # (dist_max metres, cos_min, steps) of joint_refine_view_poses
ODOMETRY_STAGES = ((0.030, 0.3, 8), (0.015, 0.5, 6), (0.0075, 0.7, 6))          # estimate_view_poses: a new view against the views before it
ESTIMATE_JOINT_STAGES = ((0.010, 0.5, 8), (0.005, 0.7, 8))                      # estimate_view_poses: the joint pass behind the odometry
MAX_PAIRS = _lib.FP_DEPTH_ALIGN_MAX_PAIRS
PHOTO_WEIGHT = 0.03      # photometric=True: metres per unit of intensity (0 .. 1)
I_MAX = 0.2              # a photometric residual of this size or more is not used


def _host_poses(cam_in_obs):
  return np.ascontiguousarray(np.asarray(torch.as_tensor(cam_in_obs).cpu(), dtype=np.float64).reshape(-1, 4, 4))


def depth_normals(depths, K, masks=None, zfar=np.inf, max_jump=0.01, device='cuda'):
  """fp_depth_normals: (n,H,W,4) float32 device tensor - per pixel the unit normal facing the camera and 1, or four zeros where the pixel,
  one of its four neighbours or the depth step to one of them (max_jump, metres) rules a normal out.  depths (n,H,W) metres, masks
  (n,H,W) non-zero = object; numpy arrays or device tensors.  Nothing synchronises."""
  dev = depths.device if torch.is_tensor(depths) and depths.is_cuda else _device(device)
  depths = torch.as_tensor(depths, device=dev).to(torch.float).contiguous()
  if depths.dim() == 2:
    depths = depths[None]
  n, H, W = depths.shape
  if masks is not None:
    masks = torch.as_tensor(masks, device=dev)
    if tuple(masks.shape) != (n, H, W):
      raise ValueError(f'masks must have the shape {(n, H, W)}, got {tuple(masks.shape)}')
    masks = (masks != 0).to(torch.uint8).contiguous()
  Kd, Kp = _lib.k_ptr(K)
  out = torch.empty((n, H, W, 4), dtype=torch.float, device=dev)
  zf = float(zfar) if np.isfinite(zfar) else float('inf')
  for a in range(0, n, MAX_VIEWS):      # views are independent: more than MAX_VIEWS are cut into calls
    b = min(a + MAX_VIEWS, n)
    check(lib().fp_depth_normals(_lib.Context.get(dev).handle, ptr(depths[a:b]), None if masks is None else ptr(masks[a:b]), b - a, H, W, Kp, zf,
                                 float(max_jump), ptr(out[a:b]), stream_ptr(dev)))
  return out


def view_intensity(rgbs, normals):
  """fp_view_intensity: (n,H,W,4) float32 device tensor on the device of `normals` (n,H,W,4, of depth_normals) - per pixel the grey value
  ((0.299 R + 0.587 G) + 0.114 B) / 255 of rgbs (n,H,W,3) uint8, its central differences along the row and the column and 1, or four
  zeros where the view has no normal: there the pixel and its four neighbours are masked valid depth without a jump, so the differences
  never reach across an occlusion edge.  Nothing synchronises."""
  dev = normals.device
  normals = normals.contiguous()
  n, H, W = normals.shape[:3]
  rgbs = torch.as_tensor(rgbs, device=dev)
  if rgbs.dim() == 3:
    rgbs = rgbs[None]
  if tuple(rgbs.shape) != (n, H, W, 3) or rgbs.dtype != torch.uint8:
    raise ValueError(f'rgbs must be uint8 of shape {(n, H, W, 3)}, got {rgbs.dtype} {tuple(rgbs.shape)}')
  if tuple(normals.shape) != (n, H, W, 4) or normals.dtype != torch.float:
    raise ValueError(f'normals must be float32 of shape {(n, H, W, 4)}, got {normals.dtype} {tuple(normals.shape)}')
  rgbs = rgbs.contiguous()
  out = torch.empty((n, H, W, 4), dtype=torch.float, device=dev)
  for a in range(0, n, MAX_VIEWS):      # views are independent: more than MAX_VIEWS are cut into calls
    b = min(a + MAX_VIEWS, n)
    check(lib().fp_view_intensity(_lib.Context.get(dev).handle, ptr(rgbs[a:b]), ptr(normals[a:b]), b - a, H, W, ptr(out[a:b]), stream_ptr(dev)))
  return out


def align_pairs_step(depths, normals, K, cam_in_obs, pairs, dist_max, cos_min, rows=False, intensity=None, i_max=I_MAX):
  """One linearisation of point-to-plane ICP for every directed pair (s, t) of `pairs` (fp_depth_pairs_align): the pixels of view s
  are projected into view t.  depths (n,H,W) and normals (n,H,W,4, of depth_normals) are device tensors.  Returns the (P,29) float64
  array of the header - per pair the upper triangle of J^T J, J^T r, sum r^2, the number of valid pixels - and, with rows=True, the
  (P,H,W,8) float32 device tensor of the per-pixel rows.  Synchronises.  More than MAX_PAIRS pairs are cut into calls (a pair's numbers
  do not depend on the batch it is in).  With `intensity` (n,H,W,4, of view_intensity) the photometric rows ride on the same association
  (fp_depth_pairs_align_photo; residuals of i_max or more are not used): (P,58) - the 29 geometric numbers, bit for bit those of the call
  without `intensity`, then the same 29 of the photometric rows - and rows of 16 floats."""
  dev = normals.device
  depths = torch.as_tensor(depths, device=dev).to(torch.float).contiguous()
  normals = normals.contiguous()
  n, H, W = depths.shape
  if tuple(normals.shape) != (n, H, W, 4) or normals.dtype != torch.float:
    raise ValueError(f'normals must be float32 of shape {(n, H, W, 4)}, got {normals.dtype} {tuple(normals.shape)}')
  poses = _host_poses(cam_in_obs)
  if len(poses) != n:
    raise ValueError(f'{n} depth maps, {len(poses)} poses')
  pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
  P = len(pairs)
  Kd, Kp = _lib.k_ptr(K)
  ctx = _lib.Context.get(dev)
  if intensity is not None:
    intensity = intensity.contiguous()
    if tuple(intensity.shape) != (n, H, W, 4) or intensity.dtype != torch.float or intensity.device != dev:
      raise ValueError(f'intensity must be float32 of shape {(n, H, W, 4)} on {dev}, got {intensity.dtype} {tuple(intensity.shape)} on {intensity.device}')
  terms, width = (_lib.FP_DEPTH_ALIGN_TERMS, 8) if intensity is None else (_lib.FP_PHOTO_ALIGN_TERMS, 16)
  sums = np.zeros((P, terms), dtype=np.float64)
  out = torch.empty((P, H, W, width), dtype=torch.float, device=dev) if rows else None
  for a in range(0, P, MAX_PAIRS):
    b = min(a + MAX_PAIRS, P)
    part = np.zeros((b - a, terms), dtype=np.float64)
    batch, rows_ptr = ptr(np.ascontiguousarray(pairs[a:b])), None if out is None else ptr(out[a:b])
    if intensity is None:
      check(lib().fp_depth_pairs_align(ctx.handle, ptr(depths), ptr(normals), n, H, W, Kp, ptr(poses), batch, b - a, float(dist_max), float(cos_min),
                                       rows_ptr, ptr(part), stream_ptr(dev)))
    else:
      check(lib().fp_depth_pairs_align_photo(ctx.handle, ptr(depths), ptr(normals), ptr(intensity), n, H, W, Kp, ptr(poses), batch, b - a,
                                             float(dist_max), float(cos_min), float(i_max), rows_ptr, ptr(part), stream_ptr(dev)))
    sums[a:b] = part
  return (sums, out) if rows else sums


def combine_sums(sums58, photo_weight):
  """(P,29) for solve_joint_step from the (P,58) of align_pairs_step(intensity=..): terms 0 .. 27 (J^T J, J^T r, sum r^2) are the geometric
  ones + photo_weight^2 x the photometric ones - the photometric residual, in units of intensity, counts as photo_weight metres per unit -
  and term 28 is the geometric count.  photo_weight = 0 returns the geometric 29 bit for bit."""
  sums58 = np.asarray(sums58, dtype=np.float64).reshape(-1, _lib.FP_PHOTO_ALIGN_TERMS)
  out = sums58[:, :29].copy()
  out[:, :28] = sums58[:, :28] + (float(photo_weight) * float(photo_weight)) * sums58[:, 29:57]
  return out


def _photo_weight(photometric):
  """None for photometric=False or None, PHOTO_WEIGHT for True, else the weight itself (a positive finite number)"""
  if photometric is None or photometric is False:
    return None
  if photometric is True:
    return PHOTO_WEIGHT
  w = float(photometric)
  if not (np.isfinite(w) and w > 0):
    raise ValueError(f'photometric must be False, True or a positive weight in metres per unit of intensity, got {photometric!r}')
  return w


def _view_intensity_of(views, normals, weight):
  """the intensity maps of `views` for a photometric weight, or None without one"""
  if weight is None:
    return None
  if views.get('rgbs') is None:
    raise ValueError('photometric: the views have no rgbs')
  return view_intensity(views['rgbs'], normals)


def _pair_blocks(sums, pairs, n_views):
  """H (n,n,6,6), g (n,6) and the valid count per view: pair (s,t) adds its A to the diagonal blocks of s and t and subtracts it from the
  blocks (s,t) and (t,s), adds its b to g[s] and subtracts it from g[t] - dr/dxi_t is -J (include/foundationpose_amd.h)."""
  Hm, g, cnt = np.zeros((n_views, n_views, 6, 6)), np.zeros((n_views, 6)), np.zeros(n_views)
  iu = np.triu_indices(6)
  for k, (s, t) in enumerate(np.asarray(pairs, dtype=np.int64).reshape(-1, 2)):
    A = np.zeros((6, 6))
    A[iu] = sums[k][:21]
    A = A + np.triu(A, 1).T
    b = np.asarray(sums[k][21:27], dtype=np.float64)
    Hm[s, s] += A
    Hm[t, t] += A
    Hm[s, t] -= A
    Hm[t, s] -= A
    g[s] += b
    g[t] -= b
    cnt[s] += sums[k][28]
    cnt[t] += sums[k][28]
  return Hm, g, cnt


def solve_joint_step(sums, pairs, n_views, fixed, damping=1e-9):
  """The joint Gauss-Newton step of all views from the (P,29) sums of align_pairs_step: the 6n x 6n system of _pair_blocks with the rows
  and columns of the `fixed` views removed and damping x trace of each diagonal block added to that block, solved in float64.  A free
  view without a valid residual is taken out as well and keeps its pose.  Returns (twists (n,6) - cam_in_ob <- expm_se3(xi) cam_in_ob,
  zero for fixed and dropped views -, dropped: the list of those views)."""
  Hm, g, cnt = _pair_blocks(sums, pairs, n_views)
  fixed = set(int(v) for v in fixed)
  dropped = [v for v in range(n_views) if v not in fixed and cnt[v] == 0]
  free = [v for v in range(n_views) if v not in fixed and cnt[v] > 0]
  xi = np.zeros((n_views, 6))
  if not free:
    return xi, dropped
  M = np.zeros((6 * len(free), 6 * len(free)))
  for a, u in enumerate(free):
    for b, v in enumerate(free):
      M[6 * a:6 * a + 6, 6 * b:6 * b + 6] = Hm[u, v]
    M[6 * a:6 * a + 6, 6 * a:6 * a + 6] += damping * np.trace(Hm[u, u]) * np.eye(6)
  sol = np.linalg.solve(M, -np.concatenate([g[v] for v in free]))
  for a, v in enumerate(free):
    xi[v] = sol[6 * a:6 * a + 6]
  return xi, dropped


def choose_pairs(cam_in_obs, neighbours=4, max_angle_deg=100):
  """Directed pairs (s, t): for every view s the `neighbours` views whose optical axes make the smallest angle with its own, among those
  within max_angle_deg; ties go to the lowest index."""
  poses = _host_poses(cam_in_obs)
  cos = poses[:, :3, 2] @ poses[:, :3, 2].T
  lim = np.cos(np.deg2rad(max_angle_deg))
  out = []
  for s in range(len(poses)):
    cand = [t for t in range(len(poses)) if t != s and cos[s, t] >= lim]
    cand.sort(key=lambda t: -cos[s, t])            # stable: the lowest index among equals
    out += [(s, t) for t in cand[:neighbours]]
  return out


def _joint_on(depths, normals, K, poses, fixed, pairs, stages, neighbours, max_angle_deg, damping, intensity=None, weight=None, i_max=I_MAX):
  """The loop of joint_refine_view_poses on prepared device tensors; `fixed`: the views that are not moved.  With `intensity` and
  `weight` every evaluation takes the 58 sums and the solver gets combine_sums of them."""
  poses = poses.copy()
  n = len(poses)
  info = dict(rms=[], valid=[], photo_rms=[], photo_valid=[], pairs=[], stopped={}, after_first=None, eig_ratio=np.full(n, np.nan))
  pr = [] if pairs is None else [tuple(int(i) for i in p) for p in pairs]
  gate = (stages[-1][0], stages[-1][1]) if len(stages) else (DEFAULT_STAGES[-1][0], DEFAULT_STAGES[-1][1])

  def evaluate():
    sm = align_pairs_step(depths, normals, K, poses, pr, *gate, intensity=intensity, i_max=i_max)
    cnt = float(sm[:, 28].sum())
    info['valid'].append(cnt)
    info['rms'].append(float(np.sqrt(sm[:, 27].sum() / max(cnt, 1.0))))
    if intensity is None:
      return sm
    cnt = float(sm[:, 57].sum())
    info['photo_valid'].append(cnt)
    info['photo_rms'].append(float(np.sqrt(sm[:, 56].sum() / max(cnt, 1.0))))
    return combine_sums(sm, weight)
  for dist_max, cos_min, steps in stages:
    if pairs is None:
      pr = choose_pairs(poses, neighbours, max_angle_deg)
    gate = (dist_max, cos_min)
    info['pairs'].append(list(pr))
    for _ in range(int(steps)):
      xi, dropped = solve_joint_step(evaluate(), pr, n, fixed, damping)
      for v in dropped:
        info['stopped'][v] = 'no valid residual'
      for v in range(n):
        if xi[v].any():
          poses[v] = expm_se3(xi[v]) @ poses[v]
      if info['after_first'] is None:
        info['after_first'] = poses.copy()
  Hm, _, _ = _pair_blocks(evaluate(), pr, n)
  for v in range(n):
    w = np.linalg.eigvalsh(Hm[v, v])
    if w[-1] > 0:
      info['eig_ratio'][v] = w[0] / w[-1]
  for k in ('rms', 'valid', 'photo_rms', 'photo_valid'):
    info[k] = np.array(info[k])
  return poses, info


def _check_view_count(n):
  if n > MAX_VIEWS:
    raise ValueError(f'{n} views: the pairwise alignment takes at most {MAX_VIEWS} per call')


def joint_refine_view_poses(views, anchor=0, pairs=None, stages=DEFAULT_STAGES, neighbours=4, max_angle_deg=100, depth_filter=True, max_jump=0.01,
                            damping=1e-9, device='cuda', photometric=False, i_max=I_MAX):
  """Joint refinement of the reference views' poses from depth alone, or from depth and grey value (photometric, below).  `views` as for reconstruct_object (at most 64).  Every view is
  linked to its `neighbours` nearest views by optical axis (choose_pairs; or `pairs`, a list of directed (s, t)); per stage (dist_max
  metres, cos_min, steps) the pairs are chosen from the current poses and `steps` joint Gauss-Newton steps are taken - each one
  fp_depth_pairs_align launch sequence over all pairs (point-to-plane residuals of view s's pixels against the surface view t sees at
  their projection, gated by distance and by the angle between the two normals) and one solve of the 6n x 6n system on the host - and
  one closing evaluation ends the call.  The anchor fixes the gauge and keeps its bits.  The basin is the first stage's gate
  (centimetres), not a voxel size; no volume is built.  Depths are prepared as for refine_view_poses (erode_depth only); normals are
  one-pixel central differences of those maps, skipped where a neighbour is more than max_jump away.  Geometry only: on a rotationally
  symmetric object the rotation about its axis is unobservable.  Returns (cam_in_obs (n,4,4) float64, info): rms and valid (one entry
  per evaluation, over all pairs), pairs (per stage), stopped {view: reason} - a free view without a valid residual keeps its pose -,
  after_first (the poses after the first step) and eig_ratio (per view the smallest over the largest eigenvalue of its 6x6 diagonal
  block at the closing evaluation: a value orders of magnitude below the others marks a weakly constrained view).
  photometric (default False: every result as without the argument) adds a grey-value residual on the same association to every pair
  (fp_depth_pairs_align_photo): the value of view t at the pixel's projection, corrected to first order for the sub-pixel offset, minus
  the value of view s at the pixel.  True weighs a unit of intensity (0 .. 1) as PHOTO_WEIGHT = 0.03 metres; a float is that weight.
  Residuals of i_max (0.2) or more are not used.  Both defaults are this library's own choice, from a CPU experiment on a textured
  sphere and a textured orbit, not the reference's.  It determines what the geometry leaves free - the rotation
  of a turntable of a bottle or a can, the sliding of a face seen head-on - where the surface has texture.  The views need rgbs
  (ValueError otherwise).  Brightness constancy is assumed: a camera moving round a static object under fixed light is served; an
  object turning under a fixed lamp, speculars and exposure changes are not.  Grey only; no image pyramid - the basin is half a texture
  wavelength -; no blur: pre-filter rgbs if they are noisy.  info then also holds photo_rms (in units of intensity) and photo_valid, one
  entry per evaluation (empty without the term), and eig_ratio comes from the combined system."""
  if isinstance(views, (str, os.PathLike)):
    views = load_reference_views(views)
  dev = _device(device)
  weight = _photo_weight(photometric)
  poses = _host_poses(views['cam_in_obs']).copy()
  n = len(poses)
  _check_view_count(n)
  if not 0 <= anchor < n:
    raise ValueError(f'anchor {anchor} of {n} views')
  depths = _eroded_depths(views, depth_filter, dev).contiguous()
  normals = depth_normals(depths, views['K'], views.get('masks'), max_jump=max_jump, device=dev)
  return _joint_on(depths, normals, views['K'], poses, [anchor], pairs, stages, neighbours, max_angle_deg, damping,
                   _view_intensity_of(views, normals, weight), weight, i_max)


def _centroid_pose(depth, mask, K, dev):
  """Identity rotation and the translation that puts the centroid of the view's valid masked points at the object's origin."""
  from .Utils import depth2xyzmap
  xyz = depth2xyzmap(depth.contiguous(), K)
  keep = xyz[..., 2] >= 0.001
  if mask is not None:
    keep &= torch.as_tensor(mask, device=dev) != 0
  pts = xyz[keep].to(torch.float64)
  if len(pts) == 0:
    raise ValueError('estimate_view_poses: the first view has no valid masked depth pixel')
  m = np.eye(4)
  m[:3, 3] = -pts.mean(0).cpu().numpy()
  return m


def estimate_view_poses(views, first_pose=None, window=2, stages=ODOMETRY_STAGES, joint=True, joint_stages=ESTIMATE_JOINT_STAGES, neighbours=4,
                        max_angle_deg=60, depth_filter=True, max_jump=0.01, damping=1e-9, device='cuda', photometric=False, i_max=I_MAX):
  """Poses for views that have none: a masked RGB-D sequence in which neighbouring frames overlap (`views` without cam_in_obs; a folder
  is read with load_reference_views(poses=False); at most 64 views).  View 0 gets first_pose, or the identity rotation with the
  translation that puts the centroid of its valid masked points at the origin - the object frame is then view 0's camera frame moved
  to the object.  View k starts at view k-1's pose and is solved alone against views k-window .. k-1 (pairs in both directions, those
  views fixed) over `stages`; then, with joint=True, the joint pass of joint_refine_view_poses runs over all views (joint_stages,
  neighbours, max_angle_deg; view 0 fixed), which closes loops that the odometry leaves open by less than its first gate.  A frame-to-
  frame step beyond the odometry's first gate (3 cm) is lost and not recovered.  photometric and i_max are those of
  joint_refine_view_poses and act in the odometry and in the joint pass: without them the odometry loses track where the geometry
  leaves a direction free, and the joint pass does not bring it back.  Returns (cam_in_obs (n,4,4) float64, info: odometry -
  the poses before the joint pass -, joint - that pass's info or None)."""
  if isinstance(views, (str, os.PathLike)):
    views = load_reference_views(views, poses=False)
  dev = _device(device)
  depths = _eroded_depths(views, depth_filter, dev).contiguous()
  n = len(depths)
  _check_view_count(n)
  masks, K = views.get('masks'), views['K']
  normals = depth_normals(depths, K, masks, max_jump=max_jump, device=dev)
  weight = _photo_weight(photometric)
  photo = (_view_intensity_of(views, normals, weight), weight, i_max)
  first = _centroid_pose(depths[0], None if masks is None else masks[0], K, dev) if first_pose is None else _host_poses(first_pose)[0]
  poses = np.stack([first] * n)
  for k in range(1, n):
    poses[k] = poses[k - 1]
    refs = list(range(max(0, k - int(window)), k))
    pr = [(k, j) for j in refs] + [(j, k) for j in refs]
    poses, _ = _joint_on(depths, normals, K, poses, [v for v in range(n) if v != k], pr, stages, neighbours, max_angle_deg, damping, *photo)
  info = dict(odometry=poses.copy(), joint=None)
  if joint:
    poses, info['joint'] = _joint_on(depths, normals, K, poses, [0], None, joint_stages, neighbours, max_angle_deg, damping, *photo)
  return poses, info


def segment_views(views, keep='central', device='cuda', **kw):
  """Fills views['masks'] from the depth maps alone, for an object standing on a plane (a turntable, a table top): (views, info).  One
  batched call of each kernel per 64 views: Utils.fit_plane on every view (unless plane= is given), then Utils.segment_on_plane; keywords
  go to the latter (h_min, h_max, max_jump, min_pixels, zfar, tol, n_hyp, seed, refits, plane).  Of a view's kept segments ONE becomes its
  mask: keep='central' the one whose centroid projects nearest to the principal point (K[0,2], K[1,2]), keep='largest' the one with the
  most pixels; ties go to the lowest label.  A view without a kept segment gets an empty mask and is named in info['empty'].  views: a
  dict with depths (n,H,W) and K (load_reference_views(dir, masks=False)); it is updated in place and returned.  info: label (n,) the
  chosen label or 0, planes (n,4), stats (the per-view dicts of segment_on_plane), empty (the indices of views without a mask).  The
  limits of segment_on_plane hold: whatever touches the object without a depth step (a hand, a fixture) is part of its segment."""
  from .segment import segment_on_plane
  if keep not in ('central', 'largest'):
    raise ValueError(f"keep must be 'central' or 'largest', got {keep!r}")
  depths = views['depths']
  K = np.asarray(views['K'].detach().cpu() if torch.is_tensor(views['K']) else views['K'], dtype=np.float64).reshape(3, 3)
  if torch.is_tensor(depths) and depths.is_cuda:
    dev = depths.device
  else:
    dev, depths = _device(device), np.asarray(depths)
  if depths.ndim != 3:
    raise ValueError(f'views["depths"] must be (n,H,W), got {tuple(depths.shape)}')
  labels, stats = segment_on_plane(torch.as_tensor(depths, device=dev), K, **kw)
  chosen = np.zeros((len(stats),), np.int32)
  for v, st in enumerate(stats):
    if len(st['label']) == 0:
      continue
    if keep == 'largest':
      score = -st['n_pixels'].astype(np.float64)
    else:
      c = st['centroid']
      score = (K[0, 0] * c[:, 0] / c[:, 2]) ** 2 + (K[1, 1] * c[:, 1] / c[:, 2]) ** 2      # squared pixel distance from the principal point
    chosen[v] = st['label'][int(np.argmin(score))]      # argmin takes the first of equals: the lowest label
  pick = torch.as_tensor(chosen, device=dev).reshape(-1, 1, 1)
  masks = ((labels == pick) & (pick > 0)).to(torch.uint8)
  views['masks'] = masks if torch.is_tensor(views['depths']) and views['depths'].is_cuda else masks.cpu().numpy()
  info = dict(label=chosen, planes=np.stack([st['plane'] for st in stats]), stats=stats, empty=np.nonzero(chosen == 0)[0].tolist())
  return views, info


def reconstruct_object(views, voxel_size=0.002, trunc=None, min_weight=1, depth_filter=True, margin=None, device='cuda', refine_poses=False,
                       max_vertices=None, simplify_cell=None, components='largest', texture=None, symmetries=None, estimate_poses=False,
                       photometric=False, segment=False, align_to=None):
  """_reconstruct_mesh (which documents every other argument) and, with `symmetries`, the rotational symmetries of the finished mesh:
  symmetries=True runs Utils.find_symmetries with its defaults, a dict gives its keyword arguments (tol, max_order, ..), and the call
  then returns (mesh, info) - info['symmetry_tfs'] is what FoundationPose(symmetry_tfs=) takes, and bop.write_models_info writes the
  rest to models_info.json.  The default (None or False) returns the mesh alone, as before.
  segment (False, True or a dict of segment_views' keyword arguments) is for views WITHOUT masks, of an object standing on a plane:
  segment_views makes them from the depth maps first; a folder is then read without mask/.  Views that have masks keep them.
  align_to (default None: the mesh in the frame the poses define) is a mesh of the same object, e.g. its CAD model: the finished mesh is
  laid onto it with Utils.align_to_mesh (a dict {'mesh': .., and align_to_mesh's keyword arguments} sets them) and returned in THAT
  mesh's frame, and the call returns (mesh, info) with info['model_from_reconstruction'] (4,4) float64 - cam_in_ob of a view in the
  model's frame is that matrix times the view's pose - and info['align'], align_to_mesh's info: with estimate_poses the object frame is
  otherwise `view 0's camera moved to the object`, which no ground truth is given in.  Symmetries, if asked for, are found after it."""
  if segment is not False and segment is not None:
    if isinstance(views, (str, os.PathLike)):
      views = load_reference_views(views, poses=not estimate_poses, masks=False)
    if views.get('masks') is None:
      views = segment_views(dict(views), device=device, **(segment if isinstance(segment, dict) else {}))[0]
  mesh = _reconstruct_mesh(views, voxel_size=voxel_size, trunc=trunc, min_weight=min_weight, depth_filter=depth_filter, margin=margin,
                           device=device, refine_poses=refine_poses, max_vertices=max_vertices, simplify_cell=simplify_cell,
                           components=components, texture=texture, estimate_poses=estimate_poses, photometric=photometric)
  info = {}
  if align_to is not None:
    from .Utils import align_to_mesh, transform_mesh
    kw = dict(align_to) if isinstance(align_to, dict) else dict(mesh=align_to)
    with torch.cuda.device(_device(device)):
      T, ainfo = align_to_mesh(mesh, kw.pop('mesh'), **kw)
    mesh = transform_mesh(mesh, T)
    info.update(model_from_reconstruction=T, align=ainfo)
  if symmetries is None or symmetries is False:
    return (mesh, info) if align_to is not None else mesh
  from .Utils import find_symmetries
  with torch.cuda.device(_device(device)):
    return mesh, dict(find_symmetries(mesh, **(symmetries if isinstance(symmetries, dict) else {})), **info)


def _reconstruct_mesh(views, voxel_size=0.002, trunc=None, min_weight=1, depth_filter=True, margin=None, device='cuda', refine_poses=False,
                      max_vertices=None, simplify_cell=None, components='largest', texture=None, estimate_poses=False, photometric=False):
  """Reference views -> mesh (synthetic.SimpleMesh with vertex normals and colours).  `views`: a folder in the reference's layout
  (load_reference_views) or a dict with depths, masks, K, cam_in_obs and optionally rgbs.  depth_filter runs erode_depth and
  bilateral_filter_depth on every view first, as the estimator does with an observed frame.  The fusion and the extraction run on the
  GPU; afterwards every connected component except the one with the most faces is dropped, also on the GPU (Utils.clean_mesh_arrays:
  fp_mesh_components_*, the rule of include/foundationpose_amd.h) and the vertices are re-indexed in their old order - fused depth noise
  leaves small floating pieces.  components='largest' is that rule; a dict of clean_mesh's keyword arguments selects another one, e.g.
  dict(keep='all', min_fraction=0.2) keeps every part with at least a fifth of the largest one's faces (a lid, a second jaw) and
  dict(keep='all', min_faces=50) every part of 50 faces or more.  The mesh stays on the device from the extraction through the clean-up
  and the simplification and is copied to the host once; only a mesh above the component limits (2^21 vertices, 2^23 faces) takes the
  host path (largest_component, scipy), which knows the 'largest' rule alone.  refine_poses=True
  runs the procedure of refine_view_poses first (view 0 is the anchor) and fuses with the poses it returns; the default fuses with the
  poses as given.  The refinement aligns on the eroded maps, before the bilateral filter, in a volume of its own: `trunc` and `margin`
  here are the fusion's and are NOT passed on to it (its band is 2 voxels, its margin 5 voxels + 1 cm); give refine_poses a dict of
  refine_view_poses' keyword arguments (anchor, order, rounds, trunc, margin, iterations, min_pixels, damping, max_step) to set them.
  refine_poses='joint' runs joint_refine_view_poses instead (pairwise ICP on the eroded maps, all views solved together, view 0 the
  anchor, its defaults).  estimate_poses=True (or a dict of estimate_view_poses' first_pose, window, stages, joint, joint_stages,
  neighbours, max_angle_deg, max_jump, damping) is for views WITHOUT cam_in_obs: the poses come from estimate_view_poses on the eroded
  maps, and refine_poses, if given, then runs on them.  A folder is then read without cam_in_ob/.
  photometric (False, True or a weight: joint_refine_view_poses) goes to whichever of refine_poses='joint' and estimate_poses runs, to
  both if both do; the views need rgbs.  ValueError if neither runs and with refine_poses=True (or a dict): the TSDF procedure has no
  such term.
  max_vertices or simplify_cell (one of them; default neither: the mesh as extracted) reduces the mesh by vertex clustering after the
  largest-component step (Utils.simplify_mesh): the rasteriser keeps a hypothesis' vertices on chip up to 8192 vertices, and a 2 mm fusion
  of a hand-sized object has tens of times that.
  texture (default None: vertex colours, the mesh as before) bakes a texture atlas last (Utils.bake_texture: fp_texture_bake), after
  the clean-up and the simplification - a simplified mesh has one colour per 2.5 - 3 mm of surface, the views have a pixel per
  millimetre - with the poses the fusion used (the refined ones under refine_poses), the depth maps the fusion used and the rgb as
  given.  True: the smallest atlas with cells of 8 texels; an int: tex_size; a dict of bake_texture's tex_size, top_n, depth_tol,
  cos_min, min_cell.  depth_tol defaults to 2 voxels here.  The views need rgbs, at most 64 of them."""
  if max_vertices is not None and simplify_cell is not None:
    raise ValueError('reconstruct_object: give max_vertices or simplify_cell, not both')
  if _photo_weight(photometric) is not None:
    if not isinstance(refine_poses, str) and refine_poses:
      raise ValueError("reconstruct_object: photometric goes with refine_poses='joint' or estimate_poses; refine_view_poses (refine_poses=True or a "
                       'dict) aligns to the fused volume and has no photometric term')
    if not estimate_poses and refine_poses != 'joint':
      raise ValueError("reconstruct_object: photometric needs refine_poses='joint' or estimate_poses to act on")
  if isinstance(views, (str, os.PathLike)):
    views = load_reference_views(views, poses=not estimate_poses)
  bake = None
  if texture is not None and texture is not False:
    bake = dict(tex_size=None, top_n=4, depth_tol=2.0 * voxel_size, min_cell=8)
    if isinstance(texture, dict):
      if set(texture) - (set(bake) | {'cos_min'}):
        raise TypeError(f'texture: unknown keys {sorted(set(texture) - (set(bake) | {"cos_min"}))}')
      bake.update(texture)
    elif texture is not True:
      bake['tex_size'] = int(texture)
    if views.get('rgbs') is None:
      raise ValueError('reconstruct_object: texture needs the views\' rgbs')
  dev = _device(device)
  eroded = _eroded_depths(views, depth_filter, dev)
  if estimate_poses:
    kw = dict(first_pose=None, window=2, stages=ODOMETRY_STAGES, joint=True, joint_stages=ESTIMATE_JOINT_STAGES, neighbours=4, max_angle_deg=60,
              max_jump=0.01, damping=1e-9)
    given = dict(estimate_poses) if isinstance(estimate_poses, dict) else {}
    if set(given) - set(kw):
      raise TypeError(f'estimate_poses: unknown keys {sorted(set(given) - set(kw))}')
    kw.update(given)
    got, _ = estimate_view_poses(dict(views, depths=eroded), depth_filter=False, device=dev, photometric=photometric, **kw)
    views = dict(views, cam_in_obs=got)
  cam_in_obs = views['cam_in_obs']
  if isinstance(refine_poses, str):
    if refine_poses != 'joint':
      raise ValueError(f"refine_poses must be False, True, 'joint' or a dict of refine_view_poses' keyword arguments, got {refine_poses!r}")
    cam_in_obs, _ = joint_refine_view_poses(dict(views, depths=eroded), depth_filter=False, device=dev, photometric=photometric)
  elif refine_poses:
    kw = dict(anchor=0, order='greedy', rounds=0, trunc=None, margin=None, iterations=10, min_pixels=100, damping=1e-9, max_step=None)
    given = dict(refine_poses) if isinstance(refine_poses, dict) else {}
    if set(given) - set(kw):
      raise TypeError(f'refine_poses: unknown keys {sorted(set(given) - set(kw))}')
    kw.update(given)
    solver = {k: kw.pop(k) for k in ('iterations', 'min_pixels', 'damping', 'max_step')}
    cam_in_obs, _ = _refine_on(eroded, views, voxel_size, kw['anchor'], kw['order'], kw['rounds'], kw['trunc'], kw['margin'], solver, dev)
  depths = _fusion_depths(eroded, depth_filter, dev)
  origin, dims = volume_from_views(depths, views.get('masks'), views['K'], cam_in_obs, voxel_size, margin=margin, device=dev)
  vol = TsdfVolume(origin, voxel_size, dims, trunc=trunc, device=dev)
  vol.integrate(depths, views['K'], cam_in_obs, rgbs=views.get('rgbs'), masks=views.get('masks'))
  rule = dict(keep='largest', min_faces=1, min_fraction=0.0)
  if isinstance(components, dict):
    if set(components) - set(rule):
      raise TypeError(f'components: unknown keys {sorted(set(components) - set(rule))}')
    rule.update(components)
  elif components != 'largest':
    raise ValueError(f"components must be 'largest' or a dict of keep, min_faces, min_fraction, got {components!r}")
  v, nr, c, f = vol.extract_arrays(min_weight)
  if len(v) > _lib.FP_MESH_COMPONENTS_MAX_VERTICES or len(f) > _lib.FP_MESH_COMPONENTS_MAX_FACES:
    if rule != dict(keep='largest', min_faces=1, min_fraction=0.0):
      raise ValueError(f'reconstruct_object: {len(v)} vertices and {len(f)} faces exceed the limits of the component clean-up on the device; '
                       f"only components='largest' is available there (a larger voxel_size gives a smaller mesh)")
    return _textured(_finish_on_host(v, nr, c, f, dev, max_vertices, simplify_cell), bake, views, depths, cam_in_obs, dev)
  from .Utils import clean_mesh_arrays, simplify_mesh
  with torch.cuda.device(dev):
    if len(f):                   # without a face there is nothing to tell apart: the vertices as extracted
      kv, kn, kc, kf, _ = clean_mesh_arrays(v, f, normals=nr, colors=c, **rule)
      if len(kf) != len(f):      # (every face kept: the mesh as extracted)
        v, nr, c, f = kv, kn, kc, kf
    if max_vertices is not None or simplify_cell is not None:
      return _textured(simplify_mesh((v, f, nr, c), cell=simplify_cell, max_vertices=max_vertices)[0], bake, views, depths, cam_in_obs, dev)
  rgba = np.concatenate([c.cpu().numpy(), np.full((len(c), 1), 255, dtype=np.uint8)], 1)
  return _textured(SimpleMesh(v.cpu().numpy(), f.cpu().numpy(), vertex_normals=nr.cpu().numpy(), vertex_colors=rgba), bake, views, depths,
                   cam_in_obs, dev)


def _textured(mesh, bake, views, depths, cam_in_obs, dev):
  """The last stage of reconstruct_object: `mesh` as it is without `bake`, else with the atlas baked from the fusion's views."""
  if bake is None or len(mesh.faces) == 0:
    return mesh
  from .Utils import bake_texture
  with torch.cuda.device(dev):
    return bake_texture(mesh, dict(rgbs=views['rgbs'], depths=depths, masks=views.get('masks'), K=views['K'], cam_in_obs=cam_in_obs), **bake)


def _finish_on_host(v, nr, c, f, dev, max_vertices, simplify_cell):
  """The tail of reconstruct_object for a mesh above the limits of fp_mesh_components_count: the largest component by scipy."""
  rgba = np.concatenate([c.cpu().numpy(), np.full((len(c), 1), 255, dtype=np.uint8)], 1)
  mesh = SimpleMesh(v.cpu().numpy(), f.cpu().numpy(), vertex_normals=nr.cpu().numpy(), vertex_colors=rgba)
  keep = largest_component(mesh.faces, len(mesh.vertices))
  if len(keep) and not keep.all():
    faces = mesh.faces[keep]
    used = np.zeros(len(mesh.vertices), dtype=bool)
    used[faces.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    mesh = SimpleMesh(mesh.vertices[used], new_id[faces], vertex_normals=mesh.vertex_normals[used], vertex_colors=mesh.visual.vertex_colors[used])
  if max_vertices is not None or simplify_cell is not None:
    from .Utils import simplify_mesh
    with torch.cuda.device(dev):
      mesh, _ = simplify_mesh(mesh, cell=simplify_cell, max_vertices=max_vertices)
  return mesh
