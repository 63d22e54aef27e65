"""numpy restatement of the photometric rules of include/foundationpose_amd.h (fp_view_intensity, fp_depth_pairs_align_photo): the intensity
map and the 16-float row of a pair in np.float32, operation for operation in the stated order, with the reason each pixel's photometric
row was skipped; the 58 sums by math.fsum; the weighting of the two halves; the two procedures of tests/depth_icp_oracle.py with the
weight.  It imports nothing from foundationpose_amd.  The geometric half of a row, the joint solver, the pair choice and the scenes come
from tests/depth_icp_oracle.py, tests/tsdf_align_oracle.py and tests/tsdf_oracle.py.

Also here, because the host and the GPU tests share them: the analytic texture, the textured cases and the recorded results."""
import math

import numpy as np

from tests import depth_icp_oracle as D
from tests import tsdf_align_oracle as A
from tests import tsdf_oracle as O

F = np.float32
TERMS = 58
PHOTO_WEIGHT = 0.03      # metres per unit of intensity
I_MAX = 0.2


# ---- the per-pixel rules --------------------------------------------------------------------------------------------------------------
def grey(rgb):
  """I = ((0.299 R + 0.587 G) + 0.114 B) / 255 in float32"""
  c = np.asarray(rgb).astype(F)
  out = ((F(0.299) * c[..., 0] + F(0.587) * c[..., 1]) + F(0.114) * c[..., 2]) / F(255)
  assert out.dtype == F
  return out


def intensity(rgb, nrm4):
  """(H,W,4) float32 of one view: (I, gx, gy, 1) where the normal map has w != 0 off the border, four zeros elsewhere"""
  I = grey(rgb)
  H, W = I.shape
  sh = lambda a, dr, dc: np.roll(a, (-dr, -dc), (0, 1))       # a[r + dr, c + dc]; the wrap-around lands on border pixels only
  gx = (sh(I, 0, 1) - sh(I, 0, -1)) * F(0.5)
  gy = (sh(I, 1, 0) - sh(I, -1, 0)) * F(0.5)
  keep = np.asarray(nrm4)[..., 3] != 0
  keep[0], keep[-1], keep[:, 0], keep[:, -1] = False, False, False, False
  out = np.stack([I, gx, gy, np.ones_like(I)], -1)
  assert out.dtype == F
  return np.where(keep[..., None], out, F(0)).astype(F)


SKIPS = ('intensity_source', 'intensity_target', 'i_max')


def pair_rows(depths, nrm, inten, K, cam_in_obs, s, t, dist_max, cos_min, i_max, reasons=False):
  """(H,W,16) float32: the 8 floats of depth_icp_oracle.pair_rows, then J0 .. J5, r, valid of the photometric row per pixel of view s
  against view t; zeros where skipped.  With reasons=True also a dict of boolean maps of the pixels each condition of SKIPS skipped,
  each among the geometrically valid pixels still alive, and 'assoc' and 'offset': the target pixel (row, col) and (du, dv)."""
  H, W = depths[s].shape
  geo, gwhy = D.pair_rows(depths, nrm, K, cam_in_obs, s, t, dist_max, cos_min, reasons=True)
  fx, fy, cx, cy = D._intrinsics(K)
  Rc, tc, _, _ = D.view_matrices(cam_in_obs[s])
  Rct, _, Ri, ti = D.view_matrices(cam_in_obs[t])
  out = np.zeros((H, W, 16), dtype=F)
  out[..., :8] = geo
  rr, cc = np.nonzero(geo[..., 7] != 0)                 # the photometric row exists only where the geometric one does
  ri, ci = gwhy['assoc'][rr, cc, 0], gwhy['assoc'][rr, cc, 1]
  with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
    d = np.asarray(depths[s], dtype=F)[rr, cc]
    p = [((cc.astype(F) - cx) / fx) * d, ((rr.astype(F) - cy) / fy) * d, d]
    x = [((Rc[a, 0] * p[0] + Rc[a, 1] * p[1]) + Rc[a, 2] * p[2]) + tc[a] for a in range(3)]
    y = [((Ri[a, 0] * x[0] + Ri[a, 1] * x[1]) + Ri[a, 2] * x[2]) + ti[a] for a in range(3)]
    u, v = (fx * y[0]) / y[2] + cx, (fy * y[1]) / y[2] + cy
    cf, rf = np.floor(u + F(0.5)), np.floor(v + F(0.5))
    assert np.array_equal(cf.astype(np.int64), ci) and np.array_equal(rf.astype(np.int64), ri)
    a4 = np.asarray(inten[s], dtype=F)[rr, cc]
    b4 = np.asarray(inten[t], dtype=F)[ri, ci]
    dead = {'intensity_source': ~(a4[:, 3] != 0)}
    ok = a4[:, 3] != 0
    dead['intensity_target'] = ok & ~(b4[:, 3] != 0)
    ok = ok & (b4[:, 3] != 0)
    du, dv = u - cf, v - rf
    r = ((b4[:, 0] + b4[:, 1] * du) + b4[:, 2] * dv) - a4[:, 0]
    small = np.abs(r) < F(i_max)
    dead['i_max'] = ok & ~small
    ok = ok & small
    jx, jy = (b4[:, 1] * fx) / y[2], (b4[:, 2] * fy) / y[2]
    jz = -((jx * y[0] + jy * y[1]) / y[2])
    a = [(Rct[k, 0] * jx + Rct[k, 1] * jy) + Rct[k, 2] * jz for k in range(3)]
    J = [a[0], a[1], a[2], x[1] * a[2] - x[2] * a[1], x[2] * a[0] - x[0] * a[2], x[0] * a[1] - x[1] * a[0]]
    got = np.stack(J + [r, np.ones_like(r)], -1)
  assert got.dtype == F and du.dtype == F and jz.dtype == F
  out[rr, cc, 8:] = np.where(ok[:, None], got, F(0))
  if not reasons:
    return out
  why = {}
  for k, m in dead.items():
    why[k] = np.zeros((H, W), dtype=bool)
    why[k][rr, cc] = m
  why['assoc'] = gwhy['assoc']
  why['offset'] = np.zeros((H, W, 2), dtype=F)
  why['offset'][rr, cc] = np.stack([du, dv], 1)
  return out, why


def sums(rw16):
  """(58,) float64 by math.fsum and sum |terms| per entry: the geometric 29 and the photometric 29"""
  rw16 = np.asarray(rw16).reshape(-1, 16)
  (g, gs), (p, ps) = D.sums(rw16[:, :8]), D.sums(rw16[:, 8:])
  return np.concatenate([g, p]), np.concatenate([gs, ps])


def step_sums(depths, nrm, inten, K, cam_in_obs, pairs, dist_max, cos_min, i_max):
  """(P,58): what fp_depth_pairs_align_photo returns in h_sums, exactly rounded"""
  out = np.zeros((len(pairs), TERMS))
  for k, (s, t) in enumerate(pairs):
    out[k] = sums(pair_rows(depths, nrm, inten, K, cam_in_obs, int(s), int(t), dist_max, cos_min, i_max))[0]
  return out


def combine(sm58, weight):
  """(P,29) for the joint solver: terms 0 .. 27 are geometric + weight^2 x photometric, term 28 is the geometric count"""
  sm58 = np.asarray(sm58, dtype=np.float64).reshape(-1, TERMS)
  out = sm58[:, :29].copy()
  out[:, :28] = sm58[:, :28] + (float(weight) * float(weight)) * sm58[:, 29:57]
  return out


def residual64(depths, K, cam_in_obs, s, t, pix, target_pix, a4, b4):
  """the photometric r in float64 of the pixels `pix` (m,2: row, col) of view s against FIXED target pixels and FIXED intensity records
  (a4 of view s, b4 of view t, (m,4)): every operation in double, smooth in both poses, so that a finite difference of it checks the
  analytic J and -J"""
  K = np.asarray(K, dtype=np.float64)
  d = np.asarray(depths[s], dtype=np.float64)[pix[:, 0], pix[:, 1]]
  p = np.stack([(pix[:, 1] - K[0, 2]) / K[0, 0], (pix[:, 0] - K[1, 2]) / K[1, 1], np.ones(len(pix))], 1) * d[:, None]
  x = p @ cam_in_obs[s][:3, :3].T + cam_in_obs[s][:3, 3]
  Dt = np.linalg.inv(cam_in_obs[t])
  y = x @ Dt[:3, :3].T + Dt[:3, 3]
  u, v = K[0, 0] * y[:, 0] / y[:, 2] + K[0, 2], K[1, 1] * y[:, 1] / y[:, 2] + K[1, 2]
  a4, b4 = np.asarray(a4, dtype=np.float64), np.asarray(b4, dtype=np.float64)
  return b4[:, 0] + b4[:, 1] * (u - target_pix[:, 1]) + b4[:, 2] * (v - target_pix[:, 0]) - a4[:, 0]


# ---- the procedures with the weight ---------------------------------------------------------------------------------------------------
def joint_refine(depths, masks, rgbs, K, cam_in_obs, weight=PHOTO_WEIGHT, i_max=I_MAX, fixed=(0,), pairs=None, stages=D.DEFAULT_STAGES, neighbours=4,
                 max_angle_deg=100, max_jump=0.01, damping=1e-9, nrm=None, inten=None):
  """depth_icp_oracle.joint_refine with the photometric term: every evaluation takes the 58 sums and solves on combine(sums, weight).
  weight = 0 is the geometric procedure (0 x photometric adds +0.0: the same numbers).  info gains photo_rms and photo_valid."""
  poses = np.array(cam_in_obs, dtype=np.float64).reshape(-1, 4, 4).copy()
  n = len(poses)
  if nrm is None:
    nrm = [D.normals(depths[v], K, None if masks is None else masks[v], max_jump=max_jump) for v in range(n)]
  if inten is None:
    inten = [intensity(rgbs[v], nrm[v]) for v in range(n)]
  info = dict(rms=[], valid=[], photo_rms=[], photo_valid=[], pairs=[], stopped={}, after_first=None, eig_ratio=None)
  pr, gate = [], (stages[-1][0], stages[-1][1]) if stages else (0.005, 0.7)

  def evaluate():
    sm = step_sums(depths, nrm, inten, K, poses, pr, gate[0], gate[1], i_max)
    cnt, pcnt = (sm[:, 28].sum(), sm[:, 57].sum()) if len(sm) else (0.0, 0.0)
    info['valid'].append(cnt)
    info['rms'].append(math.sqrt(sm[:, 27].sum() / max(cnt, 1)) if len(sm) else 0.0)
    info['photo_valid'].append(pcnt)
    info['photo_rms'].append(math.sqrt(sm[:, 56].sum() / max(pcnt, 1)) if len(sm) else 0.0)
    return combine(sm, weight)
  for dist_max, cos_min, steps in stages:
    pr = [tuple(p) for p in pairs] if pairs is not None else D.choose_pairs(poses, neighbours, max_angle_deg)
    gate = (dist_max, cos_min)
    info['pairs'].append(pr)
    for _ in range(steps):
      xi, dropped = D.solve_joint_step(evaluate(), pr, n, fixed, damping)
      for v in dropped:
        info['stopped'][v] = 'no valid residual'
      for v in range(n):
        if xi[v].any():
          poses[v] = A.expm_se3(xi[v]) @ poses[v]
      if info['after_first'] is None:
        info['after_first'] = poses.copy()
  if pairs is not None and not stages:
    pr = [tuple(p) for p in pairs]
  info['eig_ratio'] = D.eig_ratios(evaluate(), pr, n)
  return poses, info


def estimate(depths, masks, rgbs, K, weight=PHOTO_WEIGHT, i_max=I_MAX, first_pose=None, window=2, stages=D.ODOMETRY_STAGES, joint=True,
             joint_stages=D.ESTIMATE_JOINT_STAGES, neighbours=4, max_angle_deg=60, max_jump=0.01, damping=1e-9):
  """depth_icp_oracle.estimate with the photometric term in the odometry and in the joint pass"""
  n = len(depths)
  nrm = [D.normals(depths[v], K, None if masks is None else masks[v], max_jump=max_jump) for v in range(n)]
  inten = [intensity(rgbs[v], nrm[v]) for v in range(n)]
  first = D.centroid_pose(depths[0], None if masks is None else masks[0], K) if first_pose is None else np.asarray(first_pose, dtype=np.float64)
  poses = np.stack([first] * n)
  for k in range(1, n):
    poses[k] = poses[k - 1]
    refs = list(range(max(0, k - window), k))
    pr = [(k, j) for j in refs] + [(j, k) for j in refs]
    poses, _ = joint_refine(depths, masks, rgbs, K, poses, weight, i_max, fixed=[v for v in range(n) if v != k], pairs=pr, stages=stages,
                            damping=damping, nrm=nrm, inten=inten)
  info = dict(odometry=poses.copy(), joint=None)
  if joint:
    poses, info['joint'] = joint_refine(depths, masks, rgbs, K, poses, weight, i_max, fixed=(0,), stages=joint_stages, neighbours=neighbours,
                                        max_angle_deg=max_angle_deg, damping=damping, nrm=nrm, inten=inten)
  return poses, info


# ---- the texture and the cases --------------------------------------------------------------------------------------------------------
def texture(x):
  """the analytic grey value (0.1 .. 0.9) of the object point x (..,3), metres"""
  x = np.asarray(x, dtype=np.float64)
  return 0.5 + 0.2 * np.sin(70 * x[..., 0] + 1) * np.cos(55 * x[..., 1]) + 0.2 * np.sin(60 * x[..., 2] + 45 * x[..., 0])


def textured_rgbs(depths, K, truth):
  """(n,H,W,3) uint8: every valid depth pixel's point at the TRUE pose painted with texture(), quantised to 8 bits, grey; 0 elsewhere"""
  K = np.asarray(K, dtype=np.float64)
  out = []
  for dm, pose in zip(depths, truth):
    d = np.asarray(dm, dtype=np.float64)
    H, W = d.shape
    us, vs_ = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    p = np.stack([(us - K[0, 2]) / K[0, 0] * d, (vs_ - K[1, 2]) / K[1, 1] * d, d], -1)
    x = p @ np.asarray(pose)[:3, :3].T + np.asarray(pose)[:3, 3]
    g = np.where(d > 0, np.round(texture(x) * 255), 0).astype(np.uint8)
    out.append(np.stack([g, g, g], -1))
  return np.stack(out)


def row_case(*size):
  """depth_icp_oracle.row_case() with the texture: (K, truth, depths, masks, query, pairs, rgbs)"""
  K, truth, depths, masks, query, pairs = D.row_case(*size)
  return K, truth, depths, masks, query, pairs, textured_rgbs(depths, K, truth)


def tiny_case(**kw):
  """depth_icp_oracle.tiny_case() with the texture"""
  K, truth, depths, masks, query, pairs = D.tiny_case(**kw)
  return K, truth, depths, masks, query, pairs, textured_rgbs(depths, K, truth)


ROW_I_MAX = 0.05                # of the row case: tight, so that it skips pixels
ROW_INTENSITY_MAX_JUMP = 0.002  # the row case takes its intensity maps from normals of a tighter max_jump than the alignment's (0.01), so
                                # that pixels with a normal but without an intensity record exist at both ends of a pair
RAGGED = (29, 37, 75.0)         # H, W, focal of the ragged row case: 1073 pixels, a last tile of 49


def row_intensity(depths, masks, rgbs, K, max_jump=ROW_INTENSITY_MAX_JUMP):
  """the intensity maps of the row case; masks may be None"""
  return [intensity(rgbs[v], D.normals(depths[v], K, None if masks is None else masks[v], max_jump=max_jump)) for v in range(len(depths))]


SPHERE_RADIUS = 0.06


def sphere_case():
  """One sphere of 6 cm at the origin - every rotation about its centre leaves the depth maps as they are - with the texture: 8 views of
  96 x 72 from 0.4 m, 25 degrees apart in azimuth at elevations of 10, -5, 15, 0, -10, 5, -15 and 8 degrees; view 0 true, the others
  perturbed by 4 mm / 1.5 degrees (seeded).  Returns (K, truth, depths, masks, given, rgbs)."""
  H, W, focal = 72, 96, 220.0
  K = np.array([[focal, 0, W / 2 - 0.5], [0, focal, H / 2 - 0.5], [0, 0, 1.0]])
  az, el = np.deg2rad(25.0) * np.arange(8), np.deg2rad([10.0, -5.0, 15.0, 0.0, -10.0, 5.0, -15.0, 8.0])
  eyes = 0.4 * np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
  truth = np.stack([O.look_at(e) for e in eyes])
  depths = np.stack([O.sphere_depth(p, K, H, W, SPHERE_RADIUS) for p in truth]).astype(F)
  rs = np.random.RandomState(21)
  given = truth.copy()
  for v in range(1, 8):
    given[v] = A.perturb(truth[v], 0.004, 1.5, rs)
  return K, truth, depths, (depths > 0).astype(np.uint8), given, textured_rgbs(depths, K, truth)


def orbit_case():
  """depth_icp_oracle.orbit_case() with the texture on the three spheres: (K, truth, depths, masks, rgbs)"""
  K, truth, depths, masks = D.orbit_case()
  return K, truth, depths, masks, textured_rgbs(depths, K, truth)


def rotation_deg(pose, truth):
  """the angle of the rotation between two poses, degrees"""
  E = np.asarray(pose, dtype=np.float64)[:3, :3] @ np.asarray(truth, dtype=np.float64)[:3, :3].T
  return float(np.degrees(np.arccos(np.clip((np.trace(E) - 1) / 2, -1, 1))))


# joint_refine(...) of this file on sphere_case() with DEFAULT_STAGES: mean and max displacement of views 1 .. 7 in mm and the largest
# rotation error in degrees, with PHOTO_WEIGHT and with weight 0 (tests/test_photo_icp_host.py holds it to this record)
RECORDED_SPHERE_PHOTO = (0.048, 0.068, 0.048)
RECORDED_SPHERE_GEOMETRY = (6.086, 8.970, 17.521)
RECORDED_SPHERE_GEOMETRY_MIN_ROTATION_DEG = 2.780      # the smallest rotation error of views 1 .. 7 without the term; 1.5 at the start
# estimate(...) of this file on orbit_case() with first_pose = truth[0] and PHOTO_WEIGHT: mean and max displacement of frames 1 .. 23 in mm
RECORDED_ORBIT_PHOTO_ODOMETRY_MM = (0.086, 0.124)
RECORDED_ORBIT_PHOTO_FINAL_MM = (0.052, 0.080)
