"""A plain reference of the per-hypothesis pose arithmetic (csrc/pose_math.h) and of the ranking and hypothesis kernels of a registration
(csrc/register.hip), written from the definitions: numpy + fractions, no torch, no GPU.

  crop_window        compute_crop_window_tf_batch(method='box_3d') and the window's corners in the frame, in float32 ONE OPERATION AT A TIME
                     (np.float32 scalars, left to right): the operation rounds to integers, so a float64 evaluation is no reference for it.
                     `int / tensor` is torch's reciprocal() * int, hence 1 / (right - left) * out_w.  Rounding is np.rint (half to even,
                     what torch.round does).
  pose_update64      the pose update in float64: translation raw / tanh * normalizer / deepim (np.linalg.inv), rotation by Rodrigues'
                     formula with the clamp max(|v|^2, 1e-4) or 6d Gram-Schmidt with the clamps max(|.|, 1e-12), then R_delta @ R_A and
                     t_A + t_delta * scale.
  rank               the stable descending order with NaN first, as a Python sort on a key.
  hypotheses         rotation grid rows with the translation inv(K) @ [uc, vc, 1] * median in float64, rounded once to float32.
  pose_of_mesh_*     pose @ translation(-center): the two float32 evaluation orders the code states, exact (Fractions) between roundings.

MUTANTS names deliberately WRONG variants of these (the `mutant` argument of each function); tests/test_pose_ref_host.py shows which named
case tells each of them from the right one at the tolerance tests/test_gpu_pose_arith.py uses.  Nothing is random at import: every
generator seeds its own numpy Generator."""
import functools
import math
from fractions import Fraction

import numpy as np

f32 = np.float32

MUTANTS = ('round_half_away', 'swap_ow_oh', 'u_extent_only', 'skew_ignored', 'so3_eps_1e-6', 'so3_no_clamp', 'swap_tn0_tn1',
           'delta_on_the_right', 'so3_no_transpose', 'd6_no_second_clamp', 'inverse_transposed_cofactor', 'rank_unstable',
           'rank_plus_zero_above_minus_zero', 'rank_nan_last')


# ------------------------------------------------------------------------------------------------------------------------------------------
# crop window (float32, step by step)
# ------------------------------------------------------------------------------------------------------------------------------------------
def _round_half_away(x):
  return f32(math.copysign(math.floor(abs(float(x)) + 0.5), float(x))) if np.isfinite(x) else x


def crop_window(poses, K, ratio, out_size, diameter, mutant=None):
  """poses (N,4,4) float32, K 3x3 (float64, used as float32), out_size = (width, height) -> tf (N,3,3), bbox (N,4) = the frame coordinates
  of the crop's pixels (0, 0) and (width - 1, height - 1), both float32."""
  poses = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)
  k = np.asarray(K, dtype=np.float64).astype(np.float32)
  ow, oh = f32(out_size[0]), f32(out_size[1])
  if mutant == 'swap_ow_oh':
    ow, oh = oh, ow
  radius = f32(float(diameter) * float(ratio) / 2)
  zero = f32(0)
  offsets = [(zero, zero), (radius, zero), (-radius, zero), (zero, radius), (zero, -radius)]
  rnd = _round_half_away if mutant == 'round_half_away' else np.rint
  k01 = zero if mutant == 'skew_ignored' else k[0, 1]
  tf, bbox = np.zeros((len(poses), 3, 3), dtype=np.float32), np.zeros((len(poses), 4), dtype=np.float32)
  with np.errstate(all='ignore'):
    for b, p in enumerate(poses):
      us, vs = [], []
      for ox, oy in offsets:
        x, y, z = p[0, 3] + ox, p[1, 3] + oy, p[2, 3] + zero
        pu = (k[0, 0] * x + k01 * y) + k[0, 2] * z
        pv = (k[1, 0] * x + k[1, 1] * y) + k[1, 2] * z
        pw = (k[2, 0] * x + k[2, 1] * y) + k[2, 2] * z
        us.append(pu / pw), vs.append(pv / pw)
      rad = zero
      for u, v in zip(us, vs):
        rad = max(rad, abs(u - us[0]))
        if mutant != 'u_extent_only':
          rad = max(rad, abs(v - vs[0]))
      left, right = rnd(us[0] - rad), rnd(us[0] + rad)
      top, bottom = rnd(vs[0] - rad), rnd(vs[0] + rad)
      sx, sy = (f32(1) / (right - left)) * ow, (f32(1) / (bottom - top)) * oh
      t02, t12 = sx * (-left), sy * (-top)
      tf[b] = [[sx, 0, t02], [0, sy, t12], [0, 0, 1]]
      # the inverse of an axis-aligned affine map, entry by entry, then (x, y, 1) . row, left to right (the middle entry of a row is 0)
      i00, i11, i02, i12 = f32(1) / sx, f32(1) / sy, -(t02 / sx), -(t12 / sy)
      bbox[b] = [i02, i12, i00 * (ow - f32(1)) + i02, i11 * (oh - f32(1)) + i12]
      for val in (sx, sy, t02, t12, i02):
        assert type(val) is np.float32
  return tf, bbox


def window_borders(poses, K, ratio, diameter):
  """The UNROUNDED (left, right, top, bottom) of every window as exact Fractions of the float32 values crop_window rounds (for the
  host check that a case's borders are exact halves)."""
  poses = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)
  k = np.asarray(K, dtype=np.float64).astype(np.float32)
  radius = f32(float(diameter) * float(ratio) / 2)
  out = []
  for p in poses:
    pts = [(p[0, 3] + ox, p[1, 3] + oy, p[2, 3]) for ox, oy in ((0, 0), (radius, 0), (-radius, 0), (0, radius), (0, -radius))]
    us = [((k[0, 0] * x + k[0, 1] * y) + k[0, 2] * z) / ((k[2, 0] * x + k[2, 1] * y) + k[2, 2] * z) for x, y, z in pts]
    vs = [((k[1, 0] * x + k[1, 1] * y) + k[1, 2] * z) / ((k[2, 0] * x + k[2, 1] * y) + k[2, 2] * z) for x, y, z in pts]
    rad = max(max(abs(u - us[0]) for u in us), max(abs(v - vs[0]) for v in vs))
    out.append(tuple(Fraction(float(v)) for v in (us[0] - rad, us[0] + rad, vs[0] - rad, vs[0] + rad)))
  return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# pose update (float64)
# ------------------------------------------------------------------------------------------------------------------------------------------
def _inv3(m, mutant=None):
  if mutant != 'inverse_transposed_cofactor':
    return np.linalg.inv(m)
  inv = np.linalg.inv(m).copy()
  inv[0, 1], inv[1, 0] = inv[1, 0], inv[0, 1]          # one cofactor taken from the transposed position
  return inv


def so3_exp(v, eps=1e-4, clamp=True):
  """Rodrigues: I + sin(t)/t [v]x + (1 - cos t)/t^2 [v]x^2 with t^2 = max(|v|^2, eps) (pytorch3d's so3_exp_map)"""
  n2 = float(v @ v)
  if clamp:
    n2 = max(n2, eps)
  with np.errstate(all='ignore'):
    t = np.sqrt(n2)
    kx = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=np.float64)
    return np.eye(3) + np.float64(np.sin(t)) / t * kx + (1 - np.float64(np.cos(t))) / (t * t) * (kx @ kx)


def rotation_6d(d6, second_clamp=True):
  """Gram-Schmidt of (a1, a2); rows b1, b2, b1 x b2 (pytorch3d's rotation_6d_to_matrix, F.normalize's eps = 1e-12)"""
  a1, a2 = d6[:3], d6[3:]
  with np.errstate(all='ignore'):
    b1 = a1 / max(np.sqrt(a1 @ a1), 1e-12)
    b2 = a2 - (b1 @ a2) * b1
    n2 = np.sqrt(b2 @ b2)
    b2 = b2 / (max(n2, 1e-12) if second_clamp else n2)
  return np.stack([b1, b2, np.cross(b1, b2)])


def pose_update64(poseA, trans, rot, mode, tn=(1, 1, 1), rot_normalizer=1.0, trans_scale=1.0, tf=None, K=None, resize=None, mutant=None):
  """poseA (N,4,4), trans (N,3), rot (N,3) axis-angle or (N,6): float32 inputs, every scalar the float32 value the library receives.
  mode: 'raw' (t_delta = trans), 'tanh' (tanh(trans) * tn) or 'deepim' (trans = shift of the projected centre in the crop, in units of
  `resize`, and the depth ratio; tf (N,3,3) the crop transforms, K the intrinsics).  Returns (N,4,4) float64."""
  A = np.asarray(poseA)
  A = (A if A.dtype == np.float64 else A.astype(np.float32)).astype(np.float64).reshape(-1, 4, 4)      # (a float64 pose: a chained reference)
  trans, rot = np.asarray(trans, dtype=np.float32).astype(np.float64), np.asarray(rot, dtype=np.float32).astype(np.float64)
  tn = np.asarray(tn, dtype=np.float32).astype(np.float64)
  if mutant == 'swap_tn0_tn1':
    tn = tn[[1, 0, 2]]
  rn, scale = float(f32(rot_normalizer)), float(f32(trans_scale))
  out = np.tile(np.eye(4), (len(A), 1, 1))
  for b in range(len(A)):
    R_A, t_A = A[b, :3, :3], A[b, :3, 3]
    if mode == 'raw':
      td = trans[b]
    elif mode == 'tanh':
      td = np.tanh(trans[b]) * tn
    elif mode == 'deepim':
      Kb = np.asarray(K, dtype=np.float64).astype(np.float32).astype(np.float64)
      tfb = np.asarray(tf, dtype=np.float32).astype(np.float64).reshape(-1, 3, 3)[b]
      z_pred = trans[b, 2] * t_A[2]
      uvw = Kb @ t_A
      uv_crop = (tfb @ (uvw / uvw[2]))[:2] + trans[b, :2] * float(f32(resize))
      tfi = _inv3(tfb, mutant)
      uv = tfi[:2, :2] @ uv_crop + tfi[:2, 2]
      td = np.linalg.inv(Kb) @ np.array([uv[0], uv[1], 1.0]) * z_pred - t_A
    else:
      raise ValueError(mode)
    if rot.shape[1] == 3:
      v = np.tanh(rot[b]) * rn
      E = so3_exp(v, eps=1e-6 if mutant == 'so3_eps_1e-6' else 1e-4, clamp=mutant != 'so3_no_clamp')
      R_d = E if mutant == 'so3_no_transpose' else E.T
    else:
      R_d = rotation_6d(rot[b], second_clamp=mutant != 'd6_no_second_clamp').T
    out[b, :3, :3] = R_A @ R_d if mutant == 'delta_on_the_right' else R_d @ R_A
    out[b, :3, 3] = t_A + td * scale
  return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# ranking, hypotheses, pose of the mesh
# ------------------------------------------------------------------------------------------------------------------------------------------
def rank(scores, mutant=None):
  """The stable descending order: NaN (of either sign, any payload) first, then by value, -0.0 == +0.0, equal keys in index order."""
  s = [float(v) for v in np.asarray(scores, dtype=np.float32)]

  def key(i):
    v = s[i]
    if math.isnan(v):
      return (2, 0.0, 0) if mutant == 'rank_nan_last' else (0, 0.0, 0)
    sign = 0
    if mutant == 'rank_plus_zero_above_minus_zero' and v == 0:
      sign = 1 if math.copysign(1.0, v) < 0 else 0
    return (1, -v, sign)
  order = sorted(range(len(s)), key=key)             # Python's sort is stable
  if mutant == 'rank_unstable':                      # equal keys in DESCENDING index order
    order = sorted(range(len(s)), key=lambda i: key(i) + (-i,))
  return np.asarray(order, dtype=np.int64)


def hypotheses(rot_grids, stats, medians, K, K_inv=None):
  """rot_grids: list of (n_o,4,4) float32; stats: (n_obj, 6) ints (cmin, cmax, rmin, rmax, n_mask, n_usable); medians (n_obj,) float32.
  Returns the (sum n_o, 4, 4) float32 hypotheses, object after object."""
  Ki = np.linalg.inv(np.asarray(K, dtype=np.float64)) if K_inv is None else np.asarray(K_inv, dtype=np.float64)
  out = []
  for g, st, med in zip(rot_grids, stats, medians):
    uc, vc = (int(st[0]) + int(st[1])) / 2.0, (int(st[2]) + int(st[3])) / 2.0
    center = (Ki @ np.asarray([uc, vc, 1.0]).reshape(3, 1)) * np.float64(f32(med))
    h = np.array(g, dtype=np.float32).reshape(-1, 4, 4)
    h[:, :3, 3] = center.reshape(3).astype(np.float32)
    out.append(h)
  return np.concatenate(out, 0)


def round_f32(x):
  """the float32 nearest to the Fraction x, ties to even (finite, normal range)"""
  c = f32(float(x))
  cands = [c, np.nextafter(c, f32(-np.inf)), np.nextafter(c, f32(np.inf))]
  dist = [abs(Fraction(float(v)) - x) for v in cands]
  best = min(dist)
  win = [v for v, d in zip(cands, dist) if d == best]
  if len(win) > 1:
    win = [v for v in win if (int(np.asarray(v).view(np.uint32)) & 1) == 0]
  return win[0]


def _pose_of_mesh(pose, center, fma):
  p = np.asarray(pose, dtype=np.float32).reshape(4, 4)
  cn = [Fraction(float(-f32(c))) for c in np.asarray(center, dtype=np.float32)]
  out = p.copy()
  F = lambda v: Fraction(float(v))
  for r in range(4):
    if fma:      # fma(p2, c2, fma(p1, c1, p0 * c0)) + p3: one rounding per fused step
      t = round_f32(F(p[r, 0]) * cn[0])
      t = round_f32(F(p[r, 1]) * cn[1] + F(t))
      t = round_f32(F(p[r, 2]) * cn[2] + F(t))
    else:        # ((p0 * c0 + p1 * c1) + p2 * c2) + p3: every product and every sum rounded
      t = round_f32(F(round_f32(F(p[r, 0]) * cn[0])) + F(round_f32(F(p[r, 1]) * cn[1])))
      t = round_f32(F(t) + F(round_f32(F(p[r, 2]) * cn[2])))
    out[r, 3] = round_f32(F(t) + F(p[r, 3]))
  return out


def pose_of_mesh_fma(pose, center):
  """pose @ translation(-center), column 3 as a chain of fused multiply-adds from the left (the ranking kernel)"""
  return _pose_of_mesh(pose, center, True)


def pose_of_mesh_plain(pose, center):
  """the same with separate multiplies and adds, left to right (pose_of_mesh_one: the tracker and the score tail)"""
  return _pose_of_mesh(pose, center, False)


# ------------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------------
K_HALF = np.array([[512.0, 0, 320.0], [0, 512.0, 240.0], [0, 0, 1.0]])
K_SCENE = np.array([[615.3, 0.0, 321.7], [0.0, 614.1, 238.2], [0.0, 0.0, 1.0]])


def _poses_at(ts, seed=0):
  rng = np.random.default_rng(seed)
  P = np.tile(np.eye(4, dtype=np.float32), (len(ts), 1, 1))
  for b in range(len(ts)):
    P[b, :3, :3] = random_rotation(rng)
  P[:, :3, 3] = np.asarray(ts, dtype=np.float32)
  return P


def random_rotation(rng):
  q, r = np.linalg.qr(rng.standard_normal((3, 3)))
  q = q * np.sign(np.diag(r))
  if np.linalg.det(q) < 0:
    q[:, 0] = -q[:, 0]
  return q.astype(np.float32)


def _scene_ts(n, seed):
  rng = np.random.default_rng(seed)
  return np.c_[rng.uniform(-0.2, 0.2, n), rng.uniform(-0.15, 0.15, n), rng.uniform(0.4, 1.5, n)]


def _crop_cases():
  c = {}
  # centre (320 + 512 tx, 240 + 512 ty), rad = 512 * (2k/1024) / 2 = k/2: k odd puts all four borders on x.5.  tx, ty multiples of 1/512
  # shift the centre by integers: odd and even integer parts, on both axes
  ks = (127, 63, 1, 255, 5, 127, 127, 31)
  shifts = ((0, 0), (1, 0), (0, 1), (3, 2), (-7, -4), (-64, 1), (2, -3), (100, 101))
  c['half_ties'] = [dict(poses=_poses_at([(sx / 512.0, sy / 512.0, 1.0)]), K=K_HALF, ratio=1.0, out_size=(160, 160), diameter=2 * k / 1024.0)
                    for k, (sx, sy) in zip(ks, shifts)]
  c['wide_160x96'] = [dict(poses=_poses_at(_scene_ts(63, 1), 1), K=K_SCENE, ratio=1.2, out_size=(160, 96), diameter=0.191)]
  c['tall_96x160'] = [dict(poses=_poses_at(_scene_ts(65, 2), 2), K=K_SCENE, ratio=1.2, out_size=(96, 160), diameter=0.191)]
  c['fy_2fx'] = [dict(poses=_poses_at(_scene_ts(64, 3), 3), K=np.array([[300.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1.0]]), ratio=1.2,
                      out_size=(160, 160), diameter=0.191)]
  c['fx_2fy'] = [dict(poses=_poses_at(_scene_ts(130, 4), 4), K=np.array([[600.0, 0, 320.0], [0, 300.0, 240.0], [0, 0, 1.0]]), ratio=1.2,
                      out_size=(160, 160), diameter=0.191)]
  # |u3 - u0| = k01 * radius / tz against fx * radius / tz: the skew term is the largest of the ten extents
  c['large_skew'] = [dict(poses=_poses_at(_scene_ts(37, 5), 5), K=np.array([[500.0, 900.0, 320.0], [0, 450.0, 240.0], [0, 0, 1.0]]), ratio=1.2,
                          out_size=(160, 160), diameter=0.191)]
  # partly off the image (centre near a corner), wholly off it (centre far outside), negative coordinates
  c['off_image'] = [dict(poses=_poses_at([(-0.31, -0.23, 0.6), (0.33, 0.24, 0.62), (-1.5, 0.1, 0.7), (0.2, 2.5, 0.9), (-0.4, -0.6, 0.45)], 6),
                         K=K_SCENE, ratio=1.2, out_size=(160, 160), diameter=0.191)]
  # so far away that the radius is below half a pixel: right == left and bottom == top, 1 / 0
  c['collapsed'] = [dict(poses=_poses_at([(0.0, 0.0, 4000.0), (10.0, -20.0, 3000.0), (0.3, 0.2, 2500.0)], 7), K=K_SCENE, ratio=1.2,
                         out_size=(160, 160), diameter=0.191)]
  # tz barely above the radius 0.1146: a window of more than a thousand pixels
  c['tz_near_radius'] = [dict(poses=_poses_at([(0.0, 0.0, 0.115), (0.05, -0.02, 0.1147), (-0.1, 0.1, 0.12)], 8), K=K_SCENE, ratio=1.2,
                              out_size=(160, 160), diameter=0.191)]
  c['n1'] = [dict(poses=_poses_at(_scene_ts(1, 9), 9), K=K_SCENE, ratio=1.1, out_size=(160, 160), diameter=0.3)]
  return c


ROT_NORMALIZER = float(f32(0.3490658503988659))      # 20 degrees
TN_DISTINCT = (0.01, 0.03, 0.07)
TINY_NORMS = (1e-6, 1e-3, 0.00999, 0.01, 0.0101, 0.02)
TINY_DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, -1), (1, 1, 1), (0.3, -0.5, 0.8))
K_FULL = np.array([[1066.778, 3.5, 312.9869], [1.25, 1067.487, 241.3109], [0.0, 0.0, 1.0]])      # skew and a non-zero K[1,0]


def _pose_inputs(n, seed, rot_dim, rot_sigma=0.7):
  rng = np.random.default_rng(seed)
  A = _poses_at(rng.standard_normal((n, 3)) * 0.3, seed)
  trans = (rng.standard_normal((n, 3)) * 0.5).astype(np.float32)
  rot = (rng.standard_normal((n, rot_dim)) * rot_sigma).astype(np.float32)
  return A, trans, rot


def _update_cases():
  c = {}
  # tiny rotations: the pre-tanh input that gives |tanh(rot) * rot_normalizer| = the named norm, and a zero row
  rows = [np.zeros(3)]
  for nrm in TINY_NORMS:
    for d in TINY_DIRS:
      d = np.asarray(d, dtype=np.float64)
      rows.append(np.arctanh(d / np.linalg.norm(d) * nrm / ROT_NORMALIZER))
  A, trans, _ = _pose_inputs(len(rows), 10, 3)
  c['so3_tiny'] = dict(poseA=A, trans=trans, rot=np.asarray(rows, dtype=np.float32), mode='raw', trans_scale=f32(0.191 / 2))
  # saturated tanh on every sign pattern, rotation and translation, with three different translation normalizers
  signs = np.array([[(1 if (i >> k) & 1 else -1) for k in range(3)] for i in range(8)], dtype=np.float32)
  A, _, _ = _pose_inputs(8, 11, 3)
  c['saturated'] = dict(poseA=A, trans=signs * f32(20), rot=signs[::-1] * f32(20), mode='tanh', tn=TN_DISTINCT)
  A, trans, rot = _pose_inputs(65, 12, 3)
  c['tanh_tn_n65'] = dict(poseA=A, trans=trans, rot=rot, mode='tanh', tn=TN_DISTINCT)
  A, trans, rot = _pose_inputs(64, 13, 3)
  c['raw_n64_inplace'] = dict(poseA=A, trans=trans, rot=rot, mode='raw', trans_scale=f32(0.191 / 2), inplace=True)
  A, trans, rot = _pose_inputs(1, 14, 3)
  c['raw_n1'] = dict(poseA=A, trans=trans, rot=rot, mode='raw', trans_scale=f32(0.191 / 2))
  # 6d: well-conditioned rows, the same scaled by 1e-3 and 1e3
  A, trans, rot = _pose_inputs(63, 15, 6)
  rot[21:42] *= f32(1e-3)
  rot[42:] *= f32(1e3)
  c['d6_regular_n63'] = dict(poseA=A, trans=trans, rot=rot, mode='raw', trans_scale=f32(0.191 / 2))
  A, trans, rot = _pose_inputs(5, 16, 6)
  c['d6_inplace'] = dict(poseA=A, trans=trans, rot=rot, mode='tanh', tn=TN_DISTINCT, inplace=True)
  # 6d, degenerate: no float64 answer means anything here (b2 or b1 is 0 / clamp); compared with the float32 oracle alone.  The parallel
  # pairs lie on an axis: b2 is then exactly 0 (a generic parallel pair leaves rounding noise, whose normalisation is arbitrary)
  A, trans, _ = _pose_inputs(4, 17, 6)
  rot = np.array([[0, 0, 0, 0.3, -0.5, 0.8], [0.4, 0.1, -0.7, 0, 0, 0], [2, 0, 0, 6, 0, 0], [0, 0, -0.5, 0, 0, -1.5]], dtype=np.float32)
  c['d6_degenerate'] = dict(poseA=A, trans=trans, rot=rot, mode='raw', degenerate=True)
  # 6d, a2 = a1 + 1e-7 e: b2 is a few float32 ulps of a1 long, above the clamp - a float32 evaluation keeps no digit of it, and e32 says so
  A, trans, _ = _pose_inputs(3, 18, 6)
  a1 = np.array([[0.4, 0.1, -0.7], [1.0, 2.0, 2.0], [-0.3, 0.9, 0.2]], dtype=np.float32)
  e = np.eye(3, dtype=np.float32)[[1, 0, 2]]
  c['d6_near_parallel'] = dict(poseA=A, trans=trans, rot=np.concatenate([a1, a1 + f32(1e-7) * e], 1).astype(np.float32), mode='raw')
  # deepim: K with skew and K[1,0], tf with rotation and shear (no zero entry in the affine part), resize != 160
  rng = np.random.default_rng(19)
  n = 37
  A = _poses_at(np.c_[rng.uniform(-0.15, 0.15, n), rng.uniform(-0.1, 0.1, n), rng.uniform(0.4, 1.5, n)], 19)
  trans = np.c_[rng.standard_normal((n, 2)) * 0.05, 1 + rng.standard_normal(n) * 0.03].astype(np.float32)
  rot = (rng.standard_normal((n, 3)) * 0.7).astype(np.float32)
  tf = np.zeros((n, 3, 3), dtype=np.float32)
  for b in range(n):
    a, sh, s = rng.uniform(0.2, 0.9), rng.uniform(0.1, 0.4), rng.uniform(0.4, 1.6)
    rotm = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    tf[b, :2, :2] = s * rotm @ np.array([[1.0, sh], [0.0, 1.0 + sh]])
    tf[b, :2, 2] = rng.uniform(-200, -20, 2)
    tf[b, 2, 2] = 1
  c['deepim_full'] = dict(poseA=A, trans=trans, rot=rot, mode='deepim', tf=tf, K=K_FULL, resize=128.0, trans_scale=1.0)
  c['deepim_full_6d'] = dict(poseA=A, trans=trans, rot=(rng.standard_normal((n, 6)) * 0.7).astype(np.float32), mode='deepim', tf=tf, K=K_FULL,
                             resize=128.0, trans_scale=f32(0.191 / 2))
  for v in c.values():
    v.setdefault('tn', (1.0, 1.0, 1.0)), v.setdefault('trans_scale', f32(1.0)), v.setdefault('rot_normalizer', ROT_NORMALIZER)
  return c


CHAIN_DEPTH = 5


def chain_inputs():
  """5 chained updates (the tracker's depth) of 33 poses with seeded deltas: the start poses and the (trans, rot) of every step"""
  A, _, _ = _pose_inputs(33, 20, 3)
  rng = np.random.default_rng(21)
  steps = [((rng.standard_normal((33, 3)) * 0.3).astype(np.float32), (rng.standard_normal((33, 3)) * 0.7).astype(np.float32)) for _ in range(CHAIN_DEPTH)]
  return A, steps


CHAIN_SCALE = f32(0.191 / 2)


@functools.lru_cache(maxsize=None)
def chain_ref():
  """(float64 chain - every step continues from the float64 pose of the step before -, float32 oracle chain, e32, bound)"""
  A, steps = chain_inputs()
  c = dict(mode='raw', tn=(1.0, 1.0, 1.0), rot_normalizer=ROT_NORMALIZER, trans_scale=CHAIN_SCALE, rot=steps[0][1])
  ref, ora = A.astype(np.float64), A
  for trans, rot in steps:
    ref = pose_update64(ref, trans, rot, 'raw', c['tn'], c['rot_normalizer'], c['trans_scale'])
    ora = oracle_update(c, poseA=ora, trans=trans, rot=rot)
  e32 = float(np.abs(ora - ref).max())
  return ref, ora, e32, max(4 * e32, 2 * ulp32(np.abs(ref).max()))


def _bits(vals):
  return np.asarray(vals, dtype=np.uint32).view(np.float32)


def _rank_cases():
  c = {}
  rng = np.random.default_rng(30)
  nan_mix = _bits([0x7fc00000, 0xffc00000, 0x7fc00001, 0xff800001, 0x7fffffff])       # both signs, payloads, a signalling pattern
  c['issue_example'] = np.array([0., -0., 1., np.nan, np.inf, -0., 0., -np.inf, 1., np.nan], dtype=np.float32)
  c['n1'] = np.array([3.5], dtype=np.float32)
  c['n1_nan'] = _bits([0xffc00000])
  c['n2_tie'] = np.array([2.0, 2.0], dtype=np.float32)
  c['all_equal_255'] = np.full(255, 101.25, dtype=np.float32)
  runs = np.repeat(rng.permutation(32).astype(np.float32), 8)
  c['tie_runs_256'] = runs[rng.permutation(256)]
  c['increasing_257'] = (np.arange(257, dtype=np.float32) - 100) / f32(8)
  c['decreasing_300'] = (100 - np.arange(300, dtype=np.float32)) / f32(8)
  s = (rng.standard_normal(300) * 3 + 100).astype(np.float32)
  s[rng.permutation(300)[:40]] = s[7]                                            # one run of 40 ties spread over the array
  s[[3, 150, 299]] = [np.inf, -np.inf, np.inf]
  s[[0, 17, 256, 257, 298]] = nan_mix
  c['mixed_300'] = s
  z = np.zeros(64, dtype=np.float32)
  z[rng.permutation(64)[:30]] = -0.0
  c['signed_zeros_64'] = z
  d = _bits(rng.integers(1, 0x007fffff, 40)).copy()                              # denormals, of both signs, with zeros of both signs and ties
  d[::3] = -d[::3]
  d[[5, 6, 20]] = d[4]
  d[[9, 30]] = [0.0, -0.0]
  c['denormals_40'] = d
  c['negative_65'] = -np.abs(rng.standard_normal(65).astype(np.float32)).round(1) - f32(1)      # ties from the rounding
  return c


def _hypothesis_cases():
  rng = np.random.default_rng(40)
  grids = []
  for n in (63, 1, 0, 64, 65):                       # the empty object in the middle; 63 / 64 / 65 around the 64-thread block
    g = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    for b in range(n):
      g[b, :3, :3] = random_rotation(rng)
    grids.append(g)
  # odd cmin + cmax and odd rmin + rmax (half-pixel centres), even ones, a one-pixel box
  stats = np.array([[100, 203, 50, 121, 900, 800], [7, 8, 300, 301, 4, 4], [0, 0, 0, 0, 0, 0], [320, 320, 240, 240, 1, 1], [11, 600, 3, 470, 5000, 4000]],
                   dtype=np.int32)
  medians = np.array([0.7312, 1.25, 0.0, 0.0, 0.4567], dtype=np.float32)      # object 3: median 0 with hypotheses
  K = np.array([[615.3, 41.0, 321.7], [0.0, 614.1, 238.2], [0.0, 0.0, 1.0]])  # skewed: K^-1[0,1] != 0
  return dict(skewed=dict(rot_grids=grids, stats=stats, medians=medians, K=K))


@functools.lru_cache(maxsize=None)
def cases():
  """dict(crop=..., update=..., rank=..., hypotheses=...): the named inputs, built once; treat as read-only"""
  return dict(crop=_crop_cases(), update=_update_cases(), rank=_rank_cases(), hypotheses=_hypothesis_cases())


N_CASES = dict(crop=10, update=11, rank=12, hypotheses=1)


def update_case_ref(c, mutant=None):
  return pose_update64(c['poseA'], c['trans'], c['rot'], c['mode'], c['tn'], c['rot_normalizer'], c['trans_scale'], c.get('tf'), c.get('K'),
                       c.get('resize'), mutant=mutant)


def oracle_update(c, poseA=None, trans=None, rot=None):
  """oracle/predict.py:pose_update (float32, torch) on a case -> (N,4,4) float32 numpy"""
  import torch
  from oracle import predict as OP
  scale = float(c['trans_scale'])
  norm = scale != 1.0
  cfg = dict(OP.DEFAULT_REFINE_CFG, rot_rep='axis_angle' if c['rot'].shape[1] == 3 else '6d', rot_normalizer=c['rot_normalizer'])
  if c['mode'] == 'deepim':
    cfg.update(trans_rep='deepim', normalize_xyz=norm, input_resize=(int(c['resize']), int(c['resize'])))
  elif c['mode'] == 'tanh':
    assert not norm
    cfg.update(trans_rep='tracknet', normalize_xyz=False, trans_normalizer=[float(f32(t)) for t in c['tn']])
  else:
    cfg.update(trans_rep='tracknet' if norm else 'none', normalize_xyz=norm)
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
  with np.errstate(all='ignore'):
    out, _, _ = OP.pose_update(cfg, t(c['poseA'] if poseA is None else poseA), t(c['trans'] if trans is None else trans),
                               t(c['rot'] if rot is None else rot), 2.0 * scale,
                               tf_to_crops=None if c.get('tf') is None else t(c['tf']), Ks=c.get('K'))
  return out.numpy()


def ulp32(x):
  return float(np.spacing(f32(abs(x))))


def update_bound(c, ref64=None, ora=None):
  """(e32, bound) of a case: e32 = max |float32 oracle - float64 reference|, bound = max(4 e32, 2 ulp of the largest output)"""
  ref64 = update_case_ref(c) if ref64 is None else ref64
  ora = oracle_update(c) if ora is None else ora
  e32 = float(np.abs(ora.astype(np.float64) - ref64).max())
  return e32, max(4 * e32, 2 * ulp32(np.abs(ref64).max()))


ROTATION_TOL = 16 * 2.0 ** -23       # 16 float32 ulp of 1


def rotation_defect(out, poseA):
  """max of |R_out^T R_out - R_A^T R_A| and |det R_out - det R_A|: zero for an exactly orthogonal delta, whatever rounding R_A carries"""
  Ro, Ra = np.asarray(out, dtype=np.float64)[:, :3, :3], np.asarray(poseA, dtype=np.float32).astype(np.float64)[:, :3, :3]
  gram = np.abs(np.swapaxes(Ro, 1, 2) @ Ro - np.swapaxes(Ra, 1, 2) @ Ra).max()
  return max(float(gram), float(np.abs(np.linalg.det(Ro) - np.linalg.det(Ra)).max()))
