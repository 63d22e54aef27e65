"""Model-free set-up: a handful of posed RGB-D reference views of an object, with masks, fused into a mesh that goes where a CAD model
goes - make_mesh_tensors and FoundationPose(model_pts, model_normals, mesh=...).

The reference trains a neural object field for this (bundlesdf/run_nerf.py: run_one_ob -> model/model.obj).  This module reads the same
folder layout and does something else: the depth maps are fused into a truncated signed distance volume and a
coloured triangle mesh is extracted by marching tetrahedra, both on the GPU (csrc/tsdf.hip; the arithmetic is stated in
include/foundationpose_amd.h).  It does not optimise the poses of the reference views and has no view-dependent appearance.
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


def load_reference_views(dir, depth_dir=None, mask_dir='mask'):
  """The reference's folder of reference views (bundlesdf/run_nerf.py: run_one_ob): rgb/NAME.png; depth as 16-bit PNG in millimetres
  under `depth_dir` (default: depth_enhanced/ when it exists, else depth/), read as value / 1e3 in float64 and cast to float32;
  `mask_dir`/NAME.png (non-zero = object); cam_in_ob/NAME.txt (4x4, camera-to-object); K.txt.  Returns a dict: rgbs (n,H,W,3) uint8,
  depths (n,H,W) float32 metres, masks (n,H,W) uint8, K (3,3), cam_in_obs (n,4,4) float64, names."""
  from PIL import Image
  files = sorted(glob.glob(os.path.join(dir, 'rgb', '*.png')))
  if not files:
    raise FileNotFoundError(f'no rgb/*.png under {dir}')
  if depth_dir is None:
    depth_dir = 'depth_enhanced' if os.path.isdir(os.path.join(dir, 'depth_enhanced')) else 'depth'
  names = [os.path.splitext(os.path.basename(f))[0] for f in files]
  rgbs, depths, masks, poses = [], [], [], []
  for name, f in zip(names, files):
    rgbs.append(np.asarray(Image.open(f).convert('RGB'), dtype=np.uint8))
    d = np.asarray(Image.open(os.path.join(dir, depth_dir, name + '.png')))
    if d.ndim != 2:
      raise ValueError(f'{depth_dir}/{name}.png is not a single-channel depth image')
    depths.append((d.astype(np.float64) / 1e3).astype(np.float32))
    m = np.asarray(Image.open(os.path.join(dir, mask_dir, name + '.png')))
    masks.append(((m if m.ndim == 2 else m.max(-1)) > 0).astype(np.uint8))
    poses.append(np.loadtxt(os.path.join(dir, 'cam_in_ob', name + '.txt')).reshape(4, 4))
  return dict(rgbs=np.stack(rgbs), depths=np.stack(depths), masks=np.stack(masks), K=np.loadtxt(os.path.join(dir, 'K.txt')).reshape(3, 3),
              cam_in_obs=np.stack(poses), names=names)


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


def reconstruct_object(views, voxel_size=0.002, trunc=None, min_weight=1, depth_filter=True, margin=None, device='cuda'):
  """Reference views -> mesh (synthetic.SimpleMesh with vertex normals and colours).  `views`: a folder in the reference's layout
  (load_reference_views) or a dict with depths, masks, K, cam_in_obs and optionally rgbs.  depth_filter runs erode_depth and
  bilateral_filter_depth on every view first, as the estimator does with an observed frame.  The fusion and the extraction run on the
  GPU; afterwards every connected component except the one with the most faces is dropped ON THE HOST (scipy connected_components over
  the faces) and the vertices are re-indexed in their old order - fused depth noise leaves small floating pieces."""
  from .Utils import bilateral_filter_depth, erode_depth
  if isinstance(views, (str, os.PathLike)):
    views = load_reference_views(views)
  dev = _device(device)
  depths = torch.as_tensor(views['depths'], device=dev).to(torch.float)
  if depth_filter:
    depths = torch.stack([bilateral_filter_depth(erode_depth(d.contiguous(), radius=2, device=dev), radius=2, device=dev) for d in depths])
  origin, dims = volume_from_views(depths, views.get('masks'), views['K'], views['cam_in_obs'], voxel_size, margin=margin, device=dev)
  vol = TsdfVolume(origin, voxel_size, dims, trunc=trunc, device=dev)
  vol.integrate(depths, views['K'], views['cam_in_obs'], rgbs=views.get('rgbs'), masks=views.get('masks'))
  mesh = vol.extract_mesh(min_weight)
  keep = largest_component(mesh.faces, len(mesh.vertices))
  if len(keep) and not keep.all():
    faces = mesh.faces[keep]
    used = np.zeros(len(mesh.vertices), dtype=bool)
    used[faces.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    mesh = SimpleMesh(mesh.vertices[used], new_id[faces], vertex_normals=mesh.vertex_normals[used], vertex_colors=mesh.visual.vertex_colors[used])
  return mesh
