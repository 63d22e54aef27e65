"""Raw stereo pairs and distorted cameras: a lens-distortion camera model and a stereo rectification rule on the host in float64, and the
warp through them on the device (fp_remap, csrc/rectify.hip; the rule is stated in include/foundationpose_amd.h and restated in numpy by
tests/rectify_oracle.py).

    rect = rectify_stereo(K1, dist1, K2, dist2, R, T, (H, W))          # x2 = R x1 + T; mesh_io.load_stereo_calibration reads a file
    left, right = rectify_pair(raw_left, raw_right, rect)              # what stereo_disparity takes
    depth = stereo_depth(raw_left, raw_right, rectify=rect)            # warp + matching in one chain of launches, metres in rect.K_new
    plan = undistort_plan(K, dist, (H, W))
    rgb, depth = undistort_frame(raw_rgb, raw_depth, plan)             # what register / track_one / TsdfVolume take, with plan.K_new

The reference has nothing in this place (its camera vendor's SDK delivers rectified, undistorted images) and OpenCV is not a dependency:
the rules are the library's own.  **Limits: a calibration is needed, nothing is estimated from images; Brown-Conrady / rational model only
(k1 k2 p1 p2 k3 k4 k5 k6: no fisheye, no thin-prism terms); K_new keeps the focal length, so strongly distorted corners fall outside the
new image or find no source - `valid` reports them, there is no automatic zoom; depth maps are warped nearest-neighbour; the bilinear
weights of the colour warp are quantised to 1/256 pixel.**  Sizes are (H, W) everywhere.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .stereo import _finish

# monotonic_r2_max: the scan of r = i R2_SCAN_STEP, i = 1 .. R2_SCAN_STEPS (r <= 8: a field of view of 166 degrees), then R2_BISECTIONS halvings
R2_SCAN_STEP, R2_SCAN_STEPS, R2_BISECTIONS = 1.0 / 1024.0, 8 * 1024, 60


def dist8(dist):
  """The coefficients as 8 float64 (k1, k2, p1, p2, k3, k4, k5, k6): OpenCV's order; lengths 0, 4, 5 and 8 are taken, missing ones are 0."""
  d = np.zeros(0) if dist is None else np.asarray(dist, dtype=np.float64).reshape(-1)
  if d.size not in (0, 4, 5, 8):
    raise ValueError(f'distortion coefficients: {d.size} values (0, 4, 5 or 8: k1 k2 p1 p2 [k3 [k4 k5 k6]])')
  if not np.isfinite(d).all():
    raise ValueError('distortion coefficients must be finite')
  out = np.zeros(8)
  out[:d.size] = d
  return out


def _k4(K, what='K'):
  K = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float64)
  if K.shape != (3, 3):
    raise ValueError(f'{what} must be 3x3, got {K.shape}')
  if not (np.isfinite(K).all() and K[0, 0] > 0 and K[1, 1] > 0):
    raise ValueError(f'{what}: fx and fy must be positive and every entry finite')
  return K


def _size(size, what='size'):
  s = tuple(int(v) for v in np.asarray(size).reshape(-1))
  if len(s) != 2 or min(s) < 1 or max(s) > _lib.FP_REMAP_MAX_SIDE:
    raise ValueError(f'{what} must be (H, W) with 1 <= H, W <= {_lib.FP_REMAP_MAX_SIDE}, got {size}')
  return s


def distort_normalised(xy, dist):
  """(..., 2) normalised rays (x/z, y/z) -> their distorted normalised coordinates (xd, yd), float64, the model of fp_remap step 1."""
  k1, k2, p1, p2, k3, k4, k5, k6 = dist8(dist)
  xy = np.asarray(xy, dtype=np.float64)
  x, y = xy[..., 0], xy[..., 1]
  r2 = x * x + y * y
  radial = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
  xy2 = 2 * (x * y)
  xd = (x * radial + p1 * xy2) + p2 * (r2 + 2 * (x * x))
  yd = (y * radial + p1 * (r2 + 2 * (y * y))) + p2 * xy2
  return np.stack([xd, yd], -1)


def distort_points(xy, K, dist):
  """(..., 2) normalised rays -> (..., 2) pixels (u, v) of the raw camera: u = fx xd + cx, v = fy yd + cy.  Host float64."""
  K = _k4(K)
  d = distort_normalised(xy, dist)
  return np.stack([K[0, 0] * d[..., 0] + K[0, 2], K[1, 1] * d[..., 1] + K[1, 2]], -1)


def undistort_points(uv, K, dist, iterations=20):
  """(..., 2) pixels of the raw camera -> (..., 2) normalised rays: the inverse of distort_points by `iterations` steps (a fixed count,
  no stopping test) of the fixed-point rule x <- (xd - tangential(x)) / radial(x) started at x = xd.  Host float64; it converges inside
  monotonic_r2_max for the moderate distortions of real lenses (1e-12 after 20 steps at k1 = -0.2, r = 0.6) and is not meant for rays
  near the fold."""
  K = _k4(K)
  k1, k2, p1, p2, k3, k4, k5, k6 = dist8(dist)
  uv = np.asarray(uv, dtype=np.float64)
  xd, yd = (uv[..., 0] - K[0, 2]) / K[0, 0], (uv[..., 1] - K[1, 2]) / K[1, 1]
  x, y = xd.copy(), yd.copy()
  for _ in range(int(iterations)):
    r2 = x * x + y * y
    radial = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
    xy2 = 2 * (x * y)
    tx, ty = p1 * xy2 + p2 * (r2 + 2 * (x * x)), p1 * (r2 + 2 * (y * y)) + p2 * xy2
    x, y = (xd - tx) / radial, (yd - ty) / radial
  return np.stack([x, y], -1)


def _radial_slope(r, d):
  """d(r radial(r^2)) / dr in float64; -inf where the denominator of the rational model is not positive."""
  k1, k2, _, _, k3, k4, k5, k6 = d
  r2 = r * r
  num, den = 1 + r2 * (k1 + r2 * (k2 + r2 * k3)), 1 + r2 * (k4 + r2 * (k5 + r2 * k6))
  if den <= 0:
    return -np.inf
  dnum, dden = k1 + r2 * (2 * k2 + r2 * 3 * k3), k4 + r2 * (2 * k5 + r2 * 3 * k6)      # d / d(r2)
  return num / den + 2 * r2 * (dnum * den - num * dden) / (den * den)


def monotonic_r2_max(dist):
  """The smallest r2 > 0 at which d(r radial(r2)) / dr stops being positive (or the rational denominator stops being positive), inf when
  there is none up to r = 8.  Beyond it the polynomial folds rays from outside the field of view back into the image (a barrel k1 < 0
  always does, at r2 = -1 / (3 k1) when it is alone); the plans carry the value and the kernel refuses such rays.  The scan is fixed:
  r = i / 1024 for i = 1 .. 8192 in float64, the first i with a slope <= 0, then 60 bisections between i - 1 and i; the upper end is
  returned, squared."""
  d = dist8(dist)
  if not d[[0, 1, 4, 5, 6, 7]].any():
    return np.inf
  for i in range(1, R2_SCAN_STEPS + 1):
    if _radial_slope(i * R2_SCAN_STEP, d) <= 0:
      lo, hi = (i - 1) * R2_SCAN_STEP, i * R2_SCAN_STEP
      for _ in range(R2_BISECTIONS):
        mid = 0.5 * (lo + hi)
        if _radial_slope(mid, d) <= 0:
          hi = mid
        else:
          lo = mid
      return hi * hi
  return np.inf


class RemapPlan:
  """What fp_remap needs for one image, rounded to fp32 once (the way pinhole_of / rigid_of of csrc/view_geom.h do it): k_new, k_raw
  (fx, fy, cx, cy), rot (9, the rotation from the new frame to the raw frame, row-major), dist (8), r2_max, src_size and dst_size (H, W).
  K_new (3x3 float64) is the camera matrix of the warped image: what register, track_one, TsdfVolume and stereo_depth take with it."""

  def __init__(self, K_new, rot, K_raw, dist, src_size, dst_size):
    self.K_new, self.K_raw = _k4(K_new, 'K_new').copy(), _k4(K_raw).copy()
    rot = np.asarray(rot, dtype=np.float64)
    if rot.shape != (3, 3) or not np.isfinite(rot).all():
      raise ValueError('the rotation must be a finite 3x3 matrix')
    self.rotation = rot.copy()
    d = dist8(dist)
    self.k_new = np.array([self.K_new[0, 0], self.K_new[1, 1], self.K_new[0, 2], self.K_new[1, 2]], np.float32)
    self.k_raw = np.array([self.K_raw[0, 0], self.K_raw[1, 1], self.K_raw[0, 2], self.K_raw[1, 2]], np.float32)
    self.rot = rot.reshape(9).astype(np.float32)
    self.dist = d.astype(np.float32)
    self.r2_max = np.float32(monotonic_r2_max(d))
    self.src_size, self.dst_size = _size(src_size, 'size'), _size(dst_size, 'size_new')
    self._struct = None

  def as_struct(self):
    """The plan as fp_remap takes it (built once: a plan is not meant to be changed after it is made)."""
    if self._struct is None:
      self._struct = self._make_struct()
    return self._struct

  def _make_struct(self):
    return _lib.FpRemapPlan((ctypes.c_float * 4)(*self.k_new), (ctypes.c_float * 9)(*self.rot), (ctypes.c_float * 4)(*self.k_raw),
                            (ctypes.c_float * 8)(*self.dist), float(self.r2_max), self.src_size[0], self.src_size[1], self.dst_size[0], self.dst_size[1])


class StereoRectification:
  """What rectify_stereo returns: K_new (3x3, the same for both cameras), size_new (H, W), baseline (metres, in the unit of T), R1, R2 (the
  rotations from the raw left / right camera frame to the rectified one) and the two plans `left`, `right` (also `plans`)."""

  def __init__(self, K_new, size_new, baseline, R1, R2, left, right):
    self.K_new, self.size_new, self.baseline, self.R1, self.R2, self.left, self.right = K_new, size_new, baseline, R1, R2, left, right
    self.plans = (left, right)


def undistort_plan(K, dist, size, K_new=None, size_new=None):
  """The plan that removes the lens distortion of one camera: the identity rotation, K_new = K and size_new = size unless given."""
  return RemapPlan(K if K_new is None else K_new, np.eye(3), K, dist, size, size if size_new is None else size_new)


def _unit(v):
  return v / np.linalg.norm(v)


def rectify_stereo(K1, dist1, K2, dist2, R, T, size, K_new=None, size_new=None):
  """The rectification of a calibrated pair, closed-form and symmetric in the two cameras.  Convention: a point x1 of the left camera frame
  is x2 = R x1 + T in the right one; size (H, W) of both raw images.  The right centre in the left frame is c2 = -R^T T (c2.x <= 0 is
  refused: the second camera must be the right one); e1 = c2 / |c2|, zmean = normalise((0,0,1) + R^T (0,0,1)), e2 = normalise(zmean x e1),
  e3 = e1 x e2; R_rect has the rows e1, e2, e3; R1 = R_rect, R2 = R_rect R^T.  K_new by default: fx = fy = (fy1 + fy2) / 2, cx =
  (cx1 + cx2) / 2, cy = (cy1 + cy2) / 2, the same for both cameras, so a point at infinity has disparity 0 and depth = fx baseline /
  disparity with baseline = |c2|.  All in float64; the plans are rounded to fp32 once."""
  K1, K2 = _k4(K1, 'K1'), _k4(K2, 'K2')
  R = np.asarray(R, dtype=np.float64)
  T = np.asarray(T, dtype=np.float64).reshape(-1)
  if R.shape != (3, 3) or T.shape != (3,) or not (np.isfinite(R).all() and np.isfinite(T).all()):
    raise ValueError('R must be a finite 3x3 matrix and T a finite 3-vector')
  if np.abs(R @ R.T - np.eye(3)).max() > 1e-6 or np.linalg.det(R) < 0:
    raise ValueError('R is not a rotation')
  size = _size(size)
  c2 = -R.T @ T
  if not c2[0] > 0:
    raise ValueError(f'the second camera lies at x = {c2[0]:g} in the frame of the first (c2.x <= 0): it must be the right one - swap the cameras')
  baseline = float(np.linalg.norm(c2))
  e1 = c2 / baseline
  zmean = _unit(np.array([0.0, 0.0, 1.0]) + R.T @ np.array([0.0, 0.0, 1.0]))
  e2 = _unit(np.cross(zmean, e1))
  e3 = np.cross(e1, e2)
  R1 = np.stack([e1, e2, e3])
  R2 = R1 @ R.T
  if K_new is None:
    f = 0.5 * (K1[1, 1] + K2[1, 1])
    K_new = np.array([[f, 0.0, 0.5 * (K1[0, 2] + K2[0, 2])], [0.0, f, 0.5 * (K1[1, 2] + K2[1, 2])], [0.0, 0.0, 1.0]])
  K_new = _k4(K_new, 'K_new').copy()
  size_new = size if size_new is None else _size(size_new, 'size_new')
  left = RemapPlan(K_new, R1.T, K1, dist1, size, size_new)
  right = RemapPlan(K_new, R2.T, K2, dist2, size, size_new)
  return StereoRectification(K_new, size_new, baseline, R1, R2, left, right)


# ---- the device warp ----

def _images_on(img, mode, dev, name='img'):
  """(contiguous device tensor (n,H,W[,3]), channels, batch) of one image or a batch as stereo_disparity takes them."""
  t = torch.as_tensor(img)
  want = torch.uint8 if mode == 'colour' else torch.float32
  if t.dtype != want:
    raise ValueError(f'{name} must be {want} in {mode} mode, got {t.dtype}')
  t = t.to(dev).contiguous()
  if t.dim() == 2:
    channels, batch = 1, False
  elif t.dim() == 3 and t.shape[2] == 3 and mode == 'colour':
    channels, batch = 3, False
  elif t.dim() == 3:
    channels, batch = 1, True
  elif t.dim() == 4 and t.shape[3] == 3 and mode == 'colour':
    channels, batch = 3, True
  else:
    raise ValueError(f'{name} must be (H,W), (H,W,3), (n,H,W) or (n,H,W,3) (a depth map: (H,W) or (n,H,W)), got {tuple(t.shape)}')
  return (t if batch else t[None]), channels, batch


def remap(srcs, plans, mode='colour', zfar=np.inf, want_valid=False, want_map=False):
  """One fp_remap call: srcs a list of 1 or 2 contiguous device tensors (n,H,W[,3]) of one shape, plans as many RemapPlans.  Returns
  (outs, valids or None, maps or None), lists of device tensors.  One launch on the current stream; does not synchronise."""
  if mode not in ('colour', 'depth'):
    raise ValueError(f"mode must be 'colour' or 'depth', got {mode!r}")
  sides = len(srcs)
  if sides not in (1, 2) or len(plans) != sides:
    raise ValueError('one image with one plan, or two with two')
  s0 = srcs[0]
  channels = 3 if (s0.dim() == 4) else 1
  for s, p in zip(srcs, plans):
    if s.shape != s0.shape or s.device != s0.device:
      raise ValueError(f'the images differ in shape or device: {tuple(s0.shape)} and {tuple(s.shape)}')
    if tuple(s.shape[1:3]) != p.src_size:
      raise ValueError(f'an image of {tuple(s.shape[1:3])} does not fit a plan made for size {p.src_size}')
    if p.dst_size != plans[0].dst_size:
      raise ValueError(f'the plans differ in size_new: {plans[0].dst_size} and {p.dst_size}')
  dev, m = s0.device, s0.shape[0]
  Hd, Wd = plans[0].dst_size
  shape = (m, Hd, Wd) + ((3,) if channels == 3 else ())
  outs = [torch.empty(shape, dtype=s0.dtype, device=dev) for _ in range(sides)]
  valids = [torch.empty((m, Hd, Wd), dtype=torch.uint8, device=dev) for _ in range(sides)] if want_valid else None
  maps = [torch.empty((m, Hd, Wd, 2), dtype=torch.float32, device=dev) for _ in range(sides)] if want_map else None
  o = _lib.FpRemapOpts(struct_size=ctypes.sizeof(_lib.FpRemapOpts), mode=_lib.FP_REMAP_DEPTH if mode == 'depth' else _lib.FP_REMAP_COLOUR,
                       channels=channels, n_plans=sides, zfar=float(zfar))
  for i, p in enumerate(plans):
    o.plan[i] = p.as_struct()
  dbg = None
  if maps is not None:
    dbg = _lib.FpRemapDebug(struct_size=ctypes.sizeof(_lib.FpRemapDebug), d_map0=maps[0].data_ptr(), d_map1=maps[1].data_ptr() if sides == 2 else None)
  second = lambda xs: ptr(xs[1]) if xs is not None and sides == 2 else None
  check(lib().fp_remap(_lib.Context.get(dev).handle, ptr(srcs[0]), second(srcs), m * sides, ctypes.byref(o), ptr(outs[0]), second(outs),
                       ptr(valids[0]) if valids is not None else None, second(valids), ctypes.byref(dbg) if dbg is not None else None,
                       stream_ptr(dev)))
  return outs, valids, maps


def _on_device(img):
  return torch.is_tensor(img) and img.is_cuda


def remap_image(img, plan, mode='colour', zfar=np.inf, return_valid=False, return_debug=False, device='cuda'):
  """One image (or a batch of one size) through one plan: the primitive under rectify_pair and undistort_frame.  mode 'colour': uint8
  (H,W), (H,W,3), (n,H,W) or (n,H,W,3), bilinear with 1/256-pixel weights, 0 where there is no source; mode 'depth': float32 metres (H,W)
  or (n,H,W), nearest neighbour, scaled to the depth along the new optical axis, 0 where there is no source or no depth (zfar: larger
  source depths count as none).  numpy in gives numpy out, a device tensor in gives device tensors out without a host copy or a
  synchronisation.  return_valid adds the uint8 mask of the pixels that found a source, return_debug the float32 (..., 2) map (u, v):
  the result is then a tuple (image[, valid][, map])."""
  on_device = _on_device(img)
  dev = img.device if on_device else torch.device(device)
  t, _, batch = _images_on(img, mode, dev)
  outs, valids, maps = remap([t], [plan], mode, zfar, return_valid, return_debug)
  res = [_finish(outs[0], batch, on_device)]
  if return_valid:
    res.append(_finish(valids[0], batch, on_device))
  if return_debug:
    res.append(_finish(maps[0], batch, on_device))
  return res[0] if len(res) == 1 else tuple(res)


def rectify_pair(left, right, rect, return_valid=False, return_debug=False, device='cuda'):
  """The raw pair warped into the rectified cameras of `rect` (rectify_stereo): (left, right), in ONE launch for both images - or for a
  batch of pairs - without a staging copy.  Shapes as stereo_disparity takes them; numpy in gives numpy out, device tensors in give
  device tensors out without a host copy or a synchronisation.  return_valid adds (valid_left, valid_right), uint8, return_debug
  (map_left, map_right), float32 (..., 2): (left, right[, valids][, maps])."""
  on_device = _on_device(left)
  dev = left.device if on_device else torch.device(device)
  l, ch_l, batch = _images_on(left, 'colour', dev, 'left')
  r, ch_r, _ = _images_on(right, 'colour', dev, 'right')
  if l.shape != r.shape:
    raise ValueError(f'left {tuple(l.shape)} and right {tuple(r.shape)} differ in shape')
  outs, valids, maps = remap([l, r], [rect.left, rect.right], 'colour', want_valid=return_valid, want_map=return_debug)
  res = [_finish(outs[0], batch, on_device), _finish(outs[1], batch, on_device)]
  if return_valid:
    res.append(tuple(_finish(v, batch, on_device) for v in valids))
  if return_debug:
    res.append(tuple(_finish(m, batch, on_device) for m in maps))
  return tuple(res)


def undistort_frame(rgb, depth, plan, zfar=np.inf, device='cuda'):
  """An RGB-D frame of a camera with lens distortion warped into the ideal pinhole camera plan.K_new: (rgb, depth) for register, track_one,
  TsdfVolume and the aligners, which all assume such a camera.  Either input may be None (and comes back as None); the colour image goes
  through colour mode, the depth map through depth mode (nearest neighbour: depth is never blended across an edge)."""
  out_rgb = None if rgb is None else remap_image(rgb, plan, 'colour', device=device)
  out_depth = None if depth is None else remap_image(depth, plan, 'depth', zfar=zfar, device=device)
  return out_rgb, out_depth
