"""numpy restatement of the alignment rule of include/foundationpose_amd.h (fp_tsdf_align): the per-pixel row in np.float32, operation for
operation in the stated order; the sums of the rows' double products by math.fsum (exactly rounded, so they are the reference for any
summation order); the Gauss-Newton loop of TsdfVolume.align and the sequential procedure of refine_view_poses in float64.  It imports
nothing from foundationpose_amd and takes the volume, the camera helpers and the analytic sphere from tests/tsdf_oracle.py.

Also here, because the host and the GPU tests share them: an asymmetric analytic scene of three spheres and the displacement measure."""
import math

import numpy as np

from tests import tsdf_oracle as O

F = np.float32
TERMS = 29
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]      # the upper triangle of J^T J, row by row


# ---- the per-pixel rule -------------------------------------------------------------------------------------------------------------
def rows(vol, depth, K, cam_in_ob, mask=None, zfar=np.inf, min_weight=1, reasons=False):
  """(H,W,8) float32: J0 .. J5, r, valid per pixel of one view against the tests.tsdf_oracle.Volume `vol`; zeros where skipped.  With
  reasons=True also a dict of boolean maps of the pixels each condition skipped (in the rule's order, each among those still alive)."""
  depth = np.asarray(depth, dtype=F)
  H, W = depth.shape
  K = np.asarray(K, dtype=np.float64)
  fx, fy, cx, cy = F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2])
  m = np.asarray(cam_in_ob, dtype=np.float64)
  Rc, tc = m[:3, :3].astype(F), m[:3, 3].astype(F)
  T, Wt = vol.planes['tsdf'], vol.planes['weight']
  nx, ny, nz = vol.dims
  o, v, trunc = vol.origin, vol.vs, vol.trunc
  why = {}
  with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
    col, row = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    d = depth
    ok = (d >= F(0.001)) & (d < F(zfar))
    why['depth'] = ~ok
    if mask is not None:
      why['mask'] = ok & ~(np.asarray(mask) != 0)
      ok = ok & (np.asarray(mask) != 0)
    p = [((col - cx) / fx) * d, ((row - cy) / fy) * d, d]
    x = [((Rc[a, 0] * p[0] + Rc[a, 1] * p[1]) + Rc[a, 2] * p[2]) + tc[a] for a in range(3)]
    g = [(x[a] - o[a]) / v for a in range(3)]
    fl = [np.floor(ga) for ga in g]
    f = [g[a] - fl[a] for a in range(3)]
    inside = np.ones_like(ok)
    for a, n in enumerate((nx, ny, nz)):
      inside &= (fl[a] >= F(0)) & (fl[a] <= F(n - 2))
    why['outside'] = ok & ~inside
    ok = ok & inside
    i, j, k = (np.where(ok, fl[a], 0).astype(np.int64) for a in range(3))
    Tc = [T[k + (c >> 2), j + ((c >> 1) & 1), i + (c & 1)] for c in range(8)]
    Wc = [Wt[k + (c >> 2), j + ((c >> 1) & 1), i + (c & 1)] for c in range(8)]
    seen = np.ones_like(ok)
    for c in range(8):
      seen &= Wc[c] >= F(min_weight)
    why['unobserved'] = ok & ~seen
    ok = ok & seen
    d00, d10, d01, d11 = Tc[1] - Tc[0], Tc[3] - Tc[2], Tc[5] - Tc[4], Tc[7] - Tc[6]
    a00, a10, a01, a11 = Tc[0] + d00 * f[0], Tc[2] + d10 * f[0], Tc[4] + d01 * f[0], Tc[6] + d11 * f[0]
    e0, e1 = a10 - a00, a11 - a01
    b0, b1 = a00 + e0 * f[1], a01 + e1 * f[1]
    dz = b1 - b0
    Ti = b0 + dz * f[2]
    why['truncated'] = ok & ~(np.abs(Ti) < F(1))
    ok = ok & (np.abs(Ti) < F(1))
    h0, h1 = d00 + (d10 - d00) * f[1], d01 + (d11 - d01) * f[1]
    s = trunc / v
    G = [(h0 + (h1 - h0) * f[2]) * s, (e0 + (e1 - e0) * f[2]) * s, dz * s]
    r = Ti * trunc
    J = [G[0], G[1], G[2], x[1] * G[2] - x[2] * G[1], x[2] * G[0] - x[0] * G[2], x[0] * G[1] - x[1] * G[0]]
    out = np.stack(J + [r, np.ones_like(r)], -1)
  assert out.dtype == F and s.dtype == F and all(a.dtype == F for a in f)
  out = np.where(ok[..., None], out, F(0)).astype(F)
  return (out, why) if reasons else out


def terms(rw):
  """(n_pixels, 29) float64: every pixel's contribution to the 29 sums - the products of the fp32 values, exact in double"""
  rw = np.asarray(rw, dtype=np.float64).reshape(-1, 8)
  J, r = rw[:, :6], rw[:, 6]
  return np.stack([J[:, i] * J[:, j] for i, j in PAIRS] + [J[:, i] * r for i in range(6)] + [r * r, rw[:, 7]], 1)


def sums(rw):
  """(29,) float64 by math.fsum; also sum |terms| per entry (the scale of the bound on any other summation order)"""
  t = terms(rw)
  return np.array([math.fsum(t[:, e]) for e in range(TERMS)]), np.array([math.fsum(np.abs(t[:, e])) for e in range(TERMS)])


def step_sums(vol, depths, K, cam_in_obs, masks=None, zfar=np.inf, min_weight=1):
  """(n,29): what fp_tsdf_align returns in h_sums, exactly rounded"""
  return np.stack([sums(rows(vol, depths[v], K, cam_in_obs[v], None if masks is None else masks[v], zfar, min_weight))[0]
                   for v in range(len(depths))])


def residual64(vol, depth, K, cam_in_ob, pix):
  """r (metres) in float64 at the pixels `pix` (m,2: row, col) of one view: the same trilinear interpolant of the volume's fp32 samples,
  every operation in double - smooth in the pose inside a cell, so that a finite difference of it checks the analytic J"""
  K = np.asarray(K, dtype=np.float64)
  row, col = pix[:, 0].astype(np.float64), pix[:, 1].astype(np.float64)
  d = np.asarray(depth, dtype=np.float64)[pix[:, 0], pix[:, 1]]
  p = np.stack([(col - K[0, 2]) / K[0, 0] * d, (row - K[1, 2]) / K[1, 1] * d, d], 1)
  x = p @ cam_in_ob[:3, :3].T + cam_in_ob[:3, 3]
  g = (x - vol.origin.astype(np.float64)) / float(vol.vs)
  i = np.floor(g).astype(np.int64)
  f = g - i
  T = vol.planes['tsdf'].astype(np.float64)
  c = lambda dx, dy, dz: T[i[:, 2] + dz, i[:, 1] + dy, i[:, 0] + dx]
  lx = lambda dy, dz: c(0, dy, dz) + (c(1, dy, dz) - c(0, dy, dz)) * f[:, 0]
  ly = lambda dz: lx(0, dz) + (lx(1, dz) - lx(0, dz)) * f[:, 1]
  return (ly(0) + (ly(1) - ly(0)) * f[:, 2]) * float(vol.trunc), f


# ---- Gauss-Newton -----------------------------------------------------------------------------------------------------------------
def expm_se3(xi):
  """exp of the twist xi = (translation part u, rotation vector w) as a 4x4 matrix, closed form (Rodrigues), series below 1e-4 rad"""
  xi = np.asarray(xi, dtype=np.float64)
  u, w = xi[:3], xi[3:]
  th = float(np.linalg.norm(w))
  Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
  if th < 1e-4:
    A, B, C = 1 - th * th / 6, 0.5 - th * th / 24, 1 / 6 - th * th / 120
  else:
    A, B, C = math.sin(th) / th, (1 - math.cos(th)) / (th * th), (th - math.sin(th)) / (th ** 3)
  m = np.eye(4)
  m[:3, :3] = np.eye(3) + A * Kx + B * (Kx @ Kx)
  m[:3, 3] = (np.eye(3) + B * Kx + C * (Kx @ Kx)) @ u
  return m


def solve_step(s, damping=1e-9):
  """xi of one view from its 29 sums: (A + damping trace(A) I) xi = -b"""
  A = np.zeros((6, 6))
  for e, (i, j) in enumerate(PAIRS):
    A[i, j] = A[j, i] = s[e]
  b = s[21:27]
  return np.linalg.solve(A + damping * np.trace(A) * np.eye(6), -b)


def gauss_newton(step_fn, cam_in_obs, iterations=10, min_pixels=100, damping=1e-9):
  """The loop of TsdfVolume.align over `step_fn(poses) -> (n,29)`: `iterations` steps and one closing evaluation.  A view with fewer than
  min_pixels valid pixels, or whose RMS residual rose, goes back to the pose it had before its last step and stops.
  Returns (poses (n,4,4), info: valid and rms (evaluations, n), stopped {view: reason}, poses_after_first)."""
  poses = np.array(cam_in_obs, dtype=np.float64).reshape(-1, 4, 4).copy()
  n = len(poses)
  prev_pose, prev_rms = poses.copy(), np.full(n, np.inf)
  active = np.ones(n, dtype=bool)
  info = dict(valid=[], rms=[], stopped={}, after_first=None)
  for it in range(iterations + 1):
    if not active.any():
      break
    s = step_fn(poses)
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
        poses[v] = expm_se3(solve_step(s[v], damping)) @ poses[v]
    if it == 0:
      info['after_first'] = poses.copy()
  info['valid'], info['rms'] = np.array(info['valid']), np.array(info['rms'])
  return poses, info


def align(vol, depths, K, cam_in_obs, masks=None, iterations=10, min_pixels=100, damping=1e-9):
  return gauss_newton(lambda p: step_sums(vol, depths, K, p, masks), cam_in_obs, iterations, min_pixels, damping)


def greedy_next(axes, fused, left):
  """the view of `left` whose optical axis makes the smallest angle with that of any fused view (the lowest index among equals)"""
  best, best_cos = None, -2.0
  for v in left:
    c = max(float(axes[v] @ axes[u]) for u in fused)
    if c > best_cos:
      best, best_cos = v, c
  return best


def volume_for(depths, masks, K, cam_in_obs, voxel_size, margin):
  """origin and dims as reconstruct.volume_from_views states them: the bounding box of the masked valid pixels' points, grown by margin"""
  K = np.asarray(K, dtype=np.float64)
  lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
  for v in range(len(depths)):
    d = np.asarray(depths[v], dtype=np.float64)
    H, W = d.shape
    us, vs_ = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    keep = (d >= 0.001) & (np.asarray(masks[v]) != 0)
    pts = np.stack([(us - K[0, 2]) / K[0, 0] * d, (vs_ - K[1, 2]) / K[1, 1] * d, d], -1)[keep]
    pts = pts @ cam_in_obs[v][:3, :3].T + cam_in_obs[v][:3, 3]
    lo, hi = np.minimum(lo, pts.min(0)), np.maximum(hi, pts.max(0))
  return lo - margin, np.maximum(np.ceil((hi - lo + 2 * margin) / voxel_size).astype(np.int64) + 1, 2)


def refine_view_poses(depths, masks, K, cam_in_obs, voxel_size, margin, anchor=0, iterations=10, min_pixels=100, trunc=None):
  """The sequential procedure of reconstruct.refine_view_poses (order='greedy', rounds=0, no depth filter, trunc = 2 voxels
  by default) on the restatement."""
  poses = np.array(cam_in_obs, dtype=np.float64).copy()
  origin, dims = volume_for(depths, masks, K, poses, voxel_size, margin)
  vol = O.Volume(origin, voxel_size, dims, trunc=2 * voxel_size if trunc is None else trunc)
  vol.integrate(depths[anchor:anchor + 1], K, poses[anchor:anchor + 1], masks=masks[anchor:anchor + 1])
  fused, left, order, stopped = [anchor], [v for v in range(len(poses)) if v != anchor], [anchor], {}
  while left:
    v = greedy_next([p[:3, 2] for p in poses], fused, left)
    got, info = align(vol, depths[v:v + 1], K, poses[v:v + 1], masks[v:v + 1], iterations, min_pixels)
    poses[v] = got[0]
    if 0 in info['stopped']:
      stopped[v] = info['stopped'][0]
    vol.integrate(depths[v:v + 1], K, poses[v:v + 1], masks=masks[v:v + 1])
    left.remove(v)
    fused.append(v)
    order.append(v)
  return poses, dict(order=order, stopped=stopped)


# ---- the scene and the measure --------------------------------------------------------------------------------------------------------
SPHERES = ((0.034, (0.018, 0.012, -0.010)), (0.024, (-0.036, 0.016, 0.020)), (0.017, (0.004, -0.040, 0.022)))      # radius, centre (metres)


def scene_depth(cam_in_ob, K, H, W):
  """z-depth (H,W) float32 of the three spheres, the nearest hit per pixel; 0 where every ray misses"""
  d = np.stack([O.sphere_depth(cam_in_ob, K, H, W, r, c) for r, c in SPHERES])
  far = np.where(d > 0, d, np.inf).min(0)
  return np.where(np.isfinite(far), far, 0).astype(F)


def scene_views(n, H, W, focal, dist=0.4):
  """n Fibonacci views of the scene from `dist`: (K, cam_in_obs (n,4,4), depths (n,H,W), masks (n,H,W) uint8)"""
  K = np.array([[focal, 0, W / 2 - 0.5], [0, focal, H / 2 - 0.5], [0, 0, 1.0]])
  poses = np.stack([O.look_at(e) for e in O.fibonacci_eyes(n, dist)])
  depths = np.stack([scene_depth(p, K, H, W) for p in poses])
  return K, poses, depths, (depths > 0).astype(np.uint8)


def perturb(pose, trans, rot_deg, rs):
  """exp(xi) pose with a seeded twist: a translation part of length `trans` (metres) and a rotation of rot_deg degrees about random axes"""
  u, w = rs.randn(3), rs.randn(3)
  xi = np.concatenate([u / np.linalg.norm(u) * trans, w / np.linalg.norm(w) * np.deg2rad(rot_deg)])
  return expm_se3(xi) @ pose


BALL = np.random.RandomState(11).randn(2000, 3)
BALL = BALL / np.linalg.norm(BALL, axis=1, keepdims=True) * 0.05 * np.random.RandomState(12).rand(2000, 1) ** (1 / 3)


def displacement(pose, truth):
  """mean distance (metres) over 2000 seeded points of a 5 cm ball at the object's origin between where `pose` and `truth` put them:
  both are camera-to-object, so the error transform pose truth^-1 acts in the object frame"""
  E = np.asarray(pose, dtype=np.float64) @ np.linalg.inv(np.asarray(truth, dtype=np.float64))
  return float(np.linalg.norm(BALL @ E[:3, :3].T + E[:3, 3] - BALL, axis=1).mean())


# ---- the end-to-end case of refine_view_poses ---------------------------------------------------------------------------------------------
# refine_view_poses(...) of this file on refine_case(), displacement per view in mm (tests/test_tsdf_align_host.py holds it to this record)
RECORDED_BEFORE_MM = (0.0, 4.061, 4.084, 4.052, 4.074, 4.063, 4.072, 4.071, 4.050, 4.050)
RECORDED_AFTER_MM = (0.0, 0.111, 0.278, 0.133, 0.249, 0.246, 0.174, 0.245, 2.738, 0.253)
RECORDED_MEAN_MM = 0.492


def refine_case():
  """10 views of 96 x 72, view 0 true, the others perturbed by 4 mm / 1.5 degrees (seeded): (K, truth, depths, masks, given); 3 mm voxels"""
  K, truth, depths, masks = scene_views(10, 72, 96, 220.0)
  rs = np.random.RandomState(21)
  given = truth.copy()
  for v in range(1, 10):
    given[v] = perturb(truth[v], 0.004, 1.5, rs)
  return K, truth, depths, masks, given
