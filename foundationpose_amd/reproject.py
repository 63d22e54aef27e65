"""Depth and colour from two sensors: the depth map of an RGB-D camera registered into its colour camera, and the depth maps of a rig of
calibrated depth cameras merged into one view - a forward warp with a z-buffer on the device (fp_depth_reproject, csrc/reproject.hip; the
rule is stated in include/foundationpose_amd.h and restated in numpy by tests/depth_reproject_oracle.py).

    rig = rgbd_rig(K_depth, dist_depth, K_colour, dist_colour, T_colour_depth, size_depth, size_colour)      # mesh_io.load_rgbd_calibration reads a file
    rgb, depth = align_frame(raw_rgb, raw_depth, rig)                  # what register / track_one / TsdfVolume take, with rig.K
    depth, source = reproject_depth(depths, Ks, T_dst_src, K_dst, size_dst, return_source=True)      # the primitive: V views into one camera
    labels = gather_by_source(label_image_of_the_depth_camera, source)      # anything per source pixel onto the target grid

The reference has nothing in this place (its camera vendor's SDK delivers depth aligned to colour); the rule is the library's own.
**Limits: a calibration is needed, nothing is estimated from images; depth is piecewise constant over a source pixel - nearest neighbour,
nothing is interpolated across an edge; a background surface can show through a foreground one at the foreground's rim and where the
magnification exceeds 8 target pixels a source pixel; what the depth sensor does not see stays 0 (a second view fills it only when there
is one); colour is not resampled into the depth camera - `source` and gather_by_source carry labels and masks the other way.**  Sizes are
(H, W) everywhere.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .rectify import _k4, _on_device, _size, dist8, remap_image, undistort_plan
from .stereo import _finish


def _transforms(T, V):
  T = np.asarray(T.detach().cpu() if torch.is_tensor(T) else T, dtype=np.float64)
  if T.shape == (4, 4) and V == 1:
    T = T[None]
  if T.shape != (V, 4, 4):
    raise ValueError(f'T_dst_src must be ({V}, 4, 4), one transform per view, got {T.shape}')
  if not np.isfinite(T).all():
    raise ValueError('T_dst_src must be finite')
  return np.ascontiguousarray(T)


def reproject_depth(depths, Ks, T_dst_src, K_dst, size_dst, zfar=np.inf, return_source=False, device='cuda'):
  """The depth maps of V calibrated pinhole cameras seen from ONE target pinhole camera: float32 metres (H_dst, W_dst), the nearest surface
  per pixel, 0 where nothing arrived.  depths: float32 metres (V, H, W), or (n, V, H, W) for a batch of frames of the same rig; Ks: (V, 3,
  3) (one 3x3 with V = 1); T_dst_src: (V, 4, 4), x_dst = T x_src, metres; K_dst, size_dst: the target camera; zfar: source and target
  depths of zfar and more count as none.  return_source adds the int32 map of the winner's index (s H + row) W + col, -1 where nothing
  arrived: (depth, source).  numpy in gives numpy out, a device tensor in gives device tensors out without a host copy or a
  synchronisation.  The same bits on every run and in any batch.  At most 8 views; lens distortion is not seen here (remap_image removes
  it on either side, align_frame does both)."""
  on_device = _on_device(depths)
  dev = depths.device if on_device else torch.device(device)
  t = torch.as_tensor(depths)
  if t.dtype != torch.float32:
    raise ValueError(f'depths must be float32, got {t.dtype}')
  if t.dim() not in (3, 4):
    raise ValueError(f'depths must be (V, H, W) or (n, V, H, W), got {tuple(t.shape)}')
  batch = t.dim() == 4
  t = t if batch else t[None]
  n, V, Hs, Ws = t.shape
  if not 1 <= V <= _lib.FP_REPROJECT_MAX_VIEWS:
    raise ValueError(f'{V} views (1 .. {_lib.FP_REPROJECT_MAX_VIEWS})')
  if n < 1:
    raise ValueError('an empty batch')
  _size((Hs, Ws), 'the size of depths')
  Hd, Wd = _size(size_dst, 'size_dst')
  Ks = np.asarray(Ks.detach().cpu() if torch.is_tensor(Ks) else Ks, dtype=np.float64)
  Ks = Ks[None] if Ks.shape == (3, 3) and V == 1 else Ks
  if Ks.shape != (V, 3, 3):
    raise ValueError(f'Ks must be ({V}, 3, 3), one camera per view, got {Ks.shape}')
  Ks = np.ascontiguousarray(np.stack([_k4(K, f'Ks[{i}]') for i, K in enumerate(Ks)]))
  Kd = np.ascontiguousarray(_k4(K_dst, 'K_dst'))
  Ts = _transforms(T_dst_src, V)
  if not float(zfar) > 0:
    raise ValueError(f'zfar must be > 0, got {zfar}')
  t = t.to(dev).contiguous()
  keys = torch.empty((n, Hd, Wd), dtype=torch.int64, device=dev)      # the working memory of the call: 8 bytes a target pixel
  out = torch.empty((n, Hd, Wd), dtype=torch.float32, device=dev)
  source = torch.empty((n, Hd, Wd), dtype=torch.int32, device=dev) if return_source else None
  check(lib().fp_depth_reproject(_lib.Context.get(dev).handle, ptr(t), n, V, Hs, Ws, ptr(Ks), ptr(Ts), ptr(Kd), Hd, Wd, float(zfar), ptr(keys),
                                 ptr(out), ptr(source), stream_ptr(dev)))
  out = _finish(out, batch, on_device)
  return (out, _finish(source, batch, on_device)) if return_source else out


class RgbdRig:
  """What rgbd_rig returns: K (3x3 float64), the pinhole camera of the aligned frame, and its size (H, W); colour_plan, depth_plan
  (rectify.RemapPlan, None for a sensor without distortion); K_depth, the pinhole camera of the (undistorted) depth image, and size_depth;
  T_colour_depth (4x4 float64, metres: x_colour = T x_depth)."""

  def __init__(self, K, size, colour_plan, depth_plan, K_depth, size_depth, T_colour_depth):
    self.K, self.size, self.colour_plan, self.depth_plan = K, size, colour_plan, depth_plan
    self.K_depth, self.size_depth, self.T_colour_depth = K_depth, size_depth, T_colour_depth


def rgbd_rig(K_depth, dist_depth, K_colour, dist_colour, T_colour_depth, size_depth, size_colour):
  """The record of an RGB-D sensor whose depth and colour come from two sensors.  K_*, dist_*: each sensor's camera matrix and distortion
  coefficients (k1 k2 p1 p2 [k3 [k4 k5 k6]]; None, empty or all zeros: none, and that sensor gets no plan and no warp); T_colour_depth:
  4x4, x_colour = T x_depth, metres; the sizes are (H, W).  The aligned frame has the colour camera's pinhole: rig.K =
  undistort_plan(K_colour, dist_colour, size_colour).K_new (which is K_colour), rig.size = size_colour."""
  Kd, Kc = _k4(K_depth, 'K_depth').copy(), _k4(K_colour, 'K_colour').copy()
  size_depth, size_colour = _size(size_depth, 'size_depth'), _size(size_colour, 'size_colour')
  T = np.asarray(T_colour_depth.detach().cpu() if torch.is_tensor(T_colour_depth) else T_colour_depth, dtype=np.float64)
  if T.shape != (4, 4) or not np.isfinite(T).all():
    raise ValueError('T_colour_depth must be a finite 4x4 matrix')
  R = T[:3, :3]
  if np.abs(R @ R.T - np.eye(3)).max() > 1e-6 or np.linalg.det(R) < 0 or (T[3] != [0, 0, 0, 1]).any():
    raise ValueError('T_colour_depth is not a rigid transform (a rotation, a translation and the last row 0 0 0 1)')
  colour_plan = undistort_plan(Kc, dist_colour, size_colour) if dist8(dist_colour).any() else None
  depth_plan = undistort_plan(Kd, dist_depth, size_depth) if dist8(dist_depth).any() else None
  return RgbdRig(Kc if colour_plan is None else colour_plan.K_new.copy(), size_colour, colour_plan, depth_plan,
                 Kd if depth_plan is None else depth_plan.K_new.copy(), size_depth, T.copy())


def align_frame(rgb, depth, rig, zfar=np.inf, return_source=False, device='cuda'):
  """An RGB-D frame of a two-sensor camera brought onto one pixel grid, the pinhole camera rig.K of size rig.size: (rgb', depth') for
  register, track_one, TsdfVolume and the aligners.  The colour image goes through remap_image(mode='colour') when its sensor has
  distortion and is returned as it is otherwise; the depth map goes through remap_image(mode='depth') when its sensor has distortion and
  then through reproject_depth into rig.K - all on the current stream.  Either input may be None (and comes back as None); a batch
  (n,H,W[,3]) / (n,H,W) is taken.  return_source adds the winner map of reproject_depth (indices into the depth image):
  (rgb', depth', source)."""
  out_rgb = rgb
  if rgb is not None and rig.colour_plan is not None:
    out_rgb = remap_image(rgb, rig.colour_plan, 'colour', device=device)
  out_depth = source = None
  if depth is not None:
    d = depth if rig.depth_plan is None else remap_image(depth, rig.depth_plan, 'depth', zfar=zfar, device=device)
    t = torch.as_tensor(d)
    if t.dim() not in (2, 3) or tuple(t.shape[-2:]) != tuple(rig.size_depth):
      raise ValueError(f'depth must be (H,W) or (n,H,W) of the rig\'s depth size {rig.size_depth}, got {tuple(t.shape)}')
    views = d[None] if t.dim() == 2 else d[:, None]      # one view a frame
    res = reproject_depth(views, rig.K_depth[None], rig.T_colour_depth[None], rig.K, rig.size, zfar=zfar, return_source=return_source, device=device)
    out_depth, source = res if return_source else (res, None)
  return (out_rgb, out_depth, source) if return_source else (out_rgb, out_depth)


def gather_by_source(values, source, fill=0):
  """Anything per source pixel carried onto the target grid with the winner map of reproject_depth: values (V, H, W) or (V, H, W, C) -
  (H, W) is taken as one view - indexed by source (H_dst, W_dst), `fill` where source is -1.  A batch: values (n, V, H, W[, C]) with
  source (n, H_dst, W_dst).  Examples: a label image or a mask of the depth camera, the colour of an auxiliary camera (one view with
  channels: values[None]).  Plain torch / numpy indexing, no kernel; a torch source gives a torch result on its device."""
  on_torch = torch.is_tensor(source)
  v = torch.as_tensor(values, device=source.device) if on_torch else np.asarray(values)
  src = source if on_torch else np.asarray(source)
  batch = src.ndim == 3
  if src.ndim not in (2, 3):
    raise ValueError(f'source must be (H_dst, W_dst) or (n, H_dst, W_dst), got {tuple(src.shape)}')
  nd = v.ndim - (1 if batch else 0)      # 2: (H, W); 3: (V, H, W); 4: (V, H, W, C)
  if nd not in (2, 3, 4):
    raise ValueError(f'values must be ([n,] V, H, W[, C]) or ([n,] H, W), got {tuple(v.shape)}')
  chan = tuple(v.shape[-1:]) if nd == 4 else ()
  src = src if batch else src[None]
  n, Hd, Wd = src.shape
  flat = v.reshape((n, -1) + chan)
  if on_torch:
    idx = src.long().clamp(min=0).reshape(n, -1)
    out = torch.stack([flat[i][idx[i]] for i in range(n)]).reshape((n, Hd, Wd) + chan)
    out = torch.where((src >= 0).reshape((n, Hd, Wd) + (1,) * len(chan)), out, torch.as_tensor(fill, dtype=out.dtype, device=out.device))
  else:
    idx = np.maximum(src.astype(np.int64), 0).reshape(n, -1)
    out = np.stack([flat[i][idx[i]] for i in range(n)]).reshape((n, Hd, Wd) + chan)
    out = np.where((src >= 0).reshape((n, Hd, Wd) + (1,) * len(chan)), out, np.asarray(fill, dtype=out.dtype))
  return out if batch else out[0]
