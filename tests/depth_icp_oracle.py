"""numpy restatement of the two rules of include/foundationpose_amd.h for posing views from depth alone (fp_depth_normals,
fp_depth_pairs_align): the per-pixel normal and the per-pixel row of a pair in np.float32, operation for operation in the stated order,
with the reason each pixel was skipped; the sums of the rows' double products by math.fsum (exactly rounded, so they are the reference
for any summation order); the joint Gauss-Newton solver and the two procedures (joint refinement, pose estimation of an unposed
sequence) in float64.  It imports nothing from foundationpose_amd; the twist exponential, the three-sphere scene and the displacement
measure come from tests/tsdf_align_oracle.py, the camera helpers from tests/tsdf_oracle.py.

Also here, because the host and the GPU tests share them: the unposed orbit and the recorded results of both procedures."""
import math

import numpy as np

from tests import tsdf_align_oracle as A
from tests import tsdf_oracle as O

F = np.float32
TERMS = 29
DEFAULT_STAGES = ((0.020, 0.5, 6), (0.010, 0.5, 6), (0.005, 0.7, 8))             # dist_max (metres), cos_min, steps
ODOMETRY_STAGES = ((0.030, 0.3, 8), (0.015, 0.5, 6), (0.0075, 0.7, 6))
ESTIMATE_JOINT_STAGES = ((0.010, 0.5, 8), (0.005, 0.7, 8))


# ---- the per-pixel rules --------------------------------------------------------------------------------------------------------------
def _intrinsics(K):
  K = np.asarray(K, dtype=np.float64)
  return F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2])


def normals(depth, K, mask=None, zfar=np.inf, max_jump=0.01, reasons=False):
  """(H,W,4) float32: the unit normal facing the camera and 1, or four zeros; with reasons=True also a dict of boolean maps of the
  pixels each condition skipped (in the rule's order, each among those still alive)."""
  d = np.asarray(depth, dtype=F)
  H, W = d.shape
  fx, fy, cx, cy = _intrinsics(K)
  why = {}
  with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
    col, row = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    ok = (d >= F(0.001)) & (d < F(zfar))
    if mask is not None:
      ok = ok & (np.asarray(mask) != 0)
    inner = np.zeros((H, W), dtype=bool)
    inner[1:H - 1, 1:W - 1] = True
    why['border'] = ~inner
    sh = lambda a, dr, dc: np.roll(a, (-dr, -dc), (0, 1))       # a[r + dr, c + dc]; the wrap-around lands on border pixels only
    nb = ((0, -1), (0, 1), (-1, 0), (1, 0))
    all_ok = ok.copy()
    for dr, dc in nb:
      all_ok &= sh(ok, dr, dc)
    why['invalid'] = inner & ~all_ok
    alive = inner & all_ok
    flat = np.ones((H, W), dtype=bool)
    for dr, dc in nb:
      flat &= np.abs(sh(d, dr, dc) - d) <= F(max_jump)
    why['jump'] = alive & ~flat
    alive = alive & flat
    p = [((col - cx) / fx) * d, ((row - cy) / fy) * d, d]
    a = [sh(p[k], 0, 1) - sh(p[k], 0, -1) for k in range(3)]
    b = [sh(p[k], 1, 0) - sh(p[k], -1, 0) for k in range(3)]
    m = [b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]]
    l2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
    why['degenerate'] = alive & ~(l2 > F(0))
    alive = alive & (l2 > F(0))
    l = np.sqrt(l2)
    out = np.stack([m[0] / l, m[1] / l, m[2] / l, np.ones_like(l)], -1)
  assert out.dtype == F
  out = np.where(alive[..., None], out, F(0)).astype(F)
  return (out, why) if reasons else out


def view_matrices(cam_in_ob):
  """C = (Rc, tc): cam_in_ob cast to fp32; D = (Ri, ti): its inverse formed in double in the header's order, then cast"""
  m = np.asarray(cam_in_ob, dtype=np.float64)
  R, t = m[:3, :3], m[:3, 3]
  ti = np.array([-((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2]) for a in range(3)])
  return R.astype(F), t.astype(F), R.T.astype(F), ti.astype(F)


SKIPS = ('source', 'behind', 'outside', 'target', 'distance', 'angle')


def pair_rows(depths, nrm, K, cam_in_obs, s, t, dist_max, cos_min, reasons=False):
  """(H,W,8) float32: J0 .. J5, r, valid per pixel of view s against view t; zeros where skipped.  With reasons=True also a dict of
  boolean maps of the pixels each condition of SKIPS skipped (in the rule's order, each among those still alive) and, under 'assoc', the
  (H,W,2) int64 map of the target pixel (row, col) of every pixel that got as far as having one."""
  H, W = depths[s].shape
  fx, fy, cx, cy = _intrinsics(K)
  Rc, tc, _, _ = view_matrices(cam_in_obs[s])
  Rct, _, Ri, ti = view_matrices(cam_in_obs[t])
  ns4 = np.asarray(nrm[s], dtype=F)
  src = ns4[..., 3] != 0
  why = {'source': ~src}
  rr, cc = np.nonzero(src)                            # only the pixels with a source normal go on: the others write zeros
  out = np.zeros((H, W, 8), dtype=F)
  with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
    d = np.asarray(depths[s], dtype=F)[rr, cc]
    ns = [ns4[rr, cc, k] for k in range(3)]
    p = [((cc.astype(F) - cx) / fx) * d, ((rr.astype(F) - cy) / fy) * d, d]
    x = [((Rc[a, 0] * p[0] + Rc[a, 1] * p[1]) + Rc[a, 2] * p[2]) + tc[a] for a in range(3)]
    y = [((Ri[a, 0] * x[0] + Ri[a, 1] * x[1]) + Ri[a, 2] * x[2]) + ti[a] for a in range(3)]
    ok = y[2] >= F(0.001)
    dead = {'behind': ~ok}
    u, v = (fx * y[0]) / y[2] + cx, (fy * y[1]) / y[2] + cy
    cf, rf = np.floor(u + F(0.5)), np.floor(v + F(0.5))
    inside = (cf >= F(0)) & (cf <= F(W - 1)) & (rf >= F(0)) & (rf <= F(H - 1))
    dead['outside'] = ok & ~inside
    ok = ok & inside
    ci, ri = np.where(ok, cf, 0).astype(np.int64), np.where(ok, rf, 0).astype(np.int64)
    nt4 = np.asarray(nrm[t], dtype=F)[ri, ci]
    dt = np.asarray(depths[t], dtype=F)[ri, ci]
    dead['target'] = ok & ~(nt4[:, 3] != 0)
    ok = ok & (nt4[:, 3] != 0)
    q = [((cf - cx) / fx) * dt, ((rf - cy) / fy) * dt, dt]
    e = [y[a] - q[a] for a in range(3)]
    near = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] < F(dist_max) * F(dist_max)
    dead['distance'] = ok & ~near
    ok = ok & near
    n = [nt4[:, k] for k in range(3)]
    w = [(Rc[a, 0] * ns[0] + Rc[a, 1] * ns[1]) + Rc[a, 2] * ns[2] for a in range(3)]
    g = [(Ri[a, 0] * w[0] + Ri[a, 1] * w[1]) + Ri[a, 2] * w[2] for a in range(3)]
    facing = (g[0] * n[0] + g[1] * n[1]) + g[2] * n[2] >= F(cos_min)
    dead['angle'] = ok & ~facing
    ok = ok & facing
    r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
    no = [(Rct[a, 0] * n[0] + Rct[a, 1] * n[1]) + Rct[a, 2] * n[2] for a in range(3)]
    J = [no[0], no[1], no[2], x[1] * no[2] - x[2] * no[1], x[2] * no[0] - x[0] * no[2], x[0] * no[1] - x[1] * no[0]]
    got = np.stack(J + [r, np.ones_like(r)], -1)
  assert got.dtype == F and u.dtype == F and all(a.dtype == F for a in e)
  out[rr, cc] = np.where(ok[:, None], got, F(0))
  if not reasons:
    return out
  for k, m in dead.items():
    why[k] = np.zeros((H, W), dtype=bool)
    why[k][rr, cc] = m
  why['assoc'] = np.zeros((H, W, 2), dtype=np.int64)
  why['assoc'][rr, cc] = np.stack([ri, ci], 1)
  return out, why


def sums(rw):
  """(29,) float64 by math.fsum and sum |terms| per entry; skipped pixels hold zeros and are left out (they add nothing)"""
  rw = np.asarray(rw).reshape(-1, 8)
  t = A.terms(rw[rw[:, 7] != 0])
  return (np.array([math.fsum(t[:, e].tolist()) for e in range(TERMS)]), np.array([math.fsum(np.abs(t[:, e]).tolist()) for e in range(TERMS)]))


def step_sums(depths, nrm, K, cam_in_obs, pairs, dist_max, cos_min):
  """(P,29): what fp_depth_pairs_align returns in h_sums, exactly rounded"""
  out = np.zeros((len(pairs), TERMS))
  for k, (s, t) in enumerate(pairs):
    out[k] = sums(pair_rows(depths, nrm, K, cam_in_obs, int(s), int(t), dist_max, cos_min))[0]
  return out


def residual64(depths, K, cam_in_obs, s, t, pix, target_pix, n_t):
  """r in float64 of the pixels `pix` (m,2: row, col) of view s against FIXED target pixels and normals of view t: every operation in
  double, smooth in both poses, so that a finite difference of it checks the analytic J and -J"""
  K = np.asarray(K, dtype=np.float64)
  bp = lambda dm, px: np.stack([(px[:, 1] - K[0, 2]) / K[0, 0], (px[:, 0] - K[1, 2]) / K[1, 1], np.ones(len(px))], 1) * \
      np.asarray(dm, dtype=np.float64)[px[:, 0], px[:, 1]][:, None]
  x = bp(depths[s], pix) @ cam_in_obs[s][:3, :3].T + cam_in_obs[s][:3, 3]
  Dt = np.linalg.inv(cam_in_obs[t])
  y = x @ Dt[:3, :3].T + Dt[:3, 3]
  return ((y - bp(depths[t], target_pix)) * n_t).sum(1)


# ---- the joint solver -------------------------------------------------------------------------------------------------------------------
def blocks(s):
  """A (6,6) and b (6,) of one pair from its 29 sums"""
  Am = np.zeros((6, 6))
  for e, (i, j) in enumerate(A.PAIRS):
    Am[i, j] = Am[j, i] = s[e]
  return Am, np.asarray(s[21:27], dtype=np.float64)


def assemble(sm, pairs, n_views):
  """H (n,n,6,6) and g (n,6): pair (s,t) adds A to the diagonal blocks of s and t, subtracts it from the blocks (s,t) and (t,s), adds b
  to g[s] and subtracts it from g[t] (dr/dxi_t = -J)"""
  Hm, g = np.zeros((n_views, n_views, 6, 6)), np.zeros((n_views, 6))
  for k, (s, t) in enumerate(pairs):
    Am, b = blocks(sm[k])
    Hm[s, s] += Am
    Hm[t, t] += Am
    Hm[s, t] -= Am
    Hm[t, s] -= Am
    g[s] += b
    g[t] -= b
  return Hm, g


def solve_joint_step(sm, pairs, n_views, fixed, damping=1e-9):
  """The joint Gauss-Newton step: (twists (n,6) - zero for fixed and dropped views, dropped: the free views without a valid residual)"""
  Hm, g = assemble(sm, pairs, n_views)
  cnt = np.zeros(n_views)
  for k, (s, t) in enumerate(pairs):
    cnt[s] += sm[k][28]
    cnt[t] += sm[k][28]
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


def eig_ratios(sm, pairs, n_views):
  """per view the smallest over the largest eigenvalue of its diagonal block (nan without a residual): small = weakly constrained"""
  Hm, _ = assemble(sm, pairs, n_views)
  out = np.full(n_views, np.nan)
  for v in range(n_views):
    w = np.linalg.eigvalsh(Hm[v, v])
    if w[-1] > 0:
      out[v] = w[0] / w[-1]
  return out


def choose_pairs(cam_in_obs, neighbours=4, max_angle_deg=100):
  """directed pairs (s,t): for every view s the `neighbours` views whose optical axes make the smallest angle with its own, among those
  within max_angle_deg; ties go to the lowest index (a stable sort)"""
  axes = np.stack([np.asarray(p, dtype=np.float64)[:3, 2] for p in cam_in_obs])
  cos = axes @ axes.T
  lim = math.cos(math.radians(max_angle_deg))
  out = []
  for s in range(len(axes)):
    cand = [t for t in range(len(axes)) if t != s and cos[s, t] >= lim]
    cand.sort(key=lambda t: -cos[s, t])
    out += [(s, t) for t in cand[:neighbours]]
  return out


def joint_refine(depths, masks, K, cam_in_obs, fixed=(0,), pairs=None, stages=DEFAULT_STAGES, neighbours=4, max_angle_deg=100, max_jump=0.01,
                 damping=1e-9, nrm=None):
  """The procedure of reconstruct.joint_refine_view_poses (no depth filter): per stage, pairs from the current poses unless given, then
  `steps` joint steps; one closing evaluation.  Returns (poses, info: rms and valid per evaluation, pairs per stage, stopped,
  after_first, eig_ratio of the closing evaluation)."""
  poses = np.array(cam_in_obs, dtype=np.float64).reshape(-1, 4, 4).copy()
  n = len(poses)
  if nrm is None:
    nrm = [normals(depths[v], K, None if masks is None else masks[v], max_jump=max_jump) for v in range(n)]
  info = dict(rms=[], valid=[], pairs=[], stopped={}, after_first=None, eig_ratio=None)
  pr, gate = [], (stages[-1][0], stages[-1][1]) if stages else (0.005, 0.7)

  def evaluate():
    sm = step_sums(depths, nrm, K, poses, pr, *gate)
    cnt = sm[:, 28].sum() if len(sm) else 0.0
    info['valid'].append(cnt)
    info['rms'].append(math.sqrt(sm[:, 27].sum() / max(cnt, 1)) if len(sm) else 0.0)
    return sm
  for dist_max, cos_min, steps in stages:
    pr = [tuple(p) for p in pairs] if pairs is not None else choose_pairs(poses, neighbours, max_angle_deg)
    gate = (dist_max, cos_min)
    info['pairs'].append(pr)
    for _ in range(steps):
      xi, dropped = solve_joint_step(evaluate(), pr, n, fixed, damping)
      for v in dropped:
        info['stopped'][v] = 'no valid residual'
      for v in range(n):
        if xi[v].any():
          poses[v] = A.expm_se3(xi[v]) @ poses[v]
      if info['after_first'] is None:
        info['after_first'] = poses.copy()
  if pairs is not None and not stages:
    pr = [tuple(p) for p in pairs]
  info['eig_ratio'] = eig_ratios(evaluate(), pr, n)
  return poses, info


def centroid_pose(depth, mask, K):
  """identity rotation and the translation that puts the centroid of the valid masked points at the object's origin"""
  K = np.asarray(K, dtype=np.float64)
  d = np.asarray(depth, dtype=np.float64)
  H, W = d.shape
  us, vs_ = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
  keep = d >= 0.001
  if mask is not None:
    keep &= np.asarray(mask) != 0
  pts = np.stack([(us - K[0, 2]) / K[0, 0] * d, (vs_ - K[1, 2]) / K[1, 1] * d, d], -1)[keep]
  m = np.eye(4)
  m[:3, 3] = -pts.mean(0)
  return m


def estimate(depths, masks, K, first_pose=None, window=2, stages=ODOMETRY_STAGES, joint=True, joint_stages=ESTIMATE_JOINT_STAGES, neighbours=4,
             max_angle_deg=60, max_jump=0.01, damping=1e-9):
  """The procedure of reconstruct.estimate_view_poses (no depth filter): view 0 at first_pose (or centroid_pose), view k from view k-1's
  pose against views k-window .. k-1 (pairs in both directions, those views fixed), then the joint pass with view 0 fixed.
  Returns (poses, info: odometry poses, joint info)."""
  n = len(depths)
  nrm = [normals(depths[v], K, None if masks is None else masks[v], max_jump=max_jump) for v in range(n)]
  first = centroid_pose(depths[0], None if masks is None else masks[0], K) if first_pose is None else np.asarray(first_pose, dtype=np.float64)
  poses = np.stack([first] * n)
  for k in range(1, n):
    poses[k] = poses[k - 1]
    refs = list(range(max(0, k - window), k))
    pr = [(k, j) for j in refs] + [(j, k) for j in refs]
    poses, _ = joint_refine(depths, masks, K, poses, fixed=[v for v in range(n) if v != k], pairs=pr, stages=stages, damping=damping, nrm=nrm)
  info = dict(odometry=poses.copy(), joint=None)
  if joint:
    poses, info['joint'] = joint_refine(depths, masks, K, poses, fixed=(0,), stages=joint_stages, neighbours=neighbours,
                                        max_angle_deg=max_angle_deg, damping=damping, nrm=nrm)
  return poses, info


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def mean_mm(poses, truth, views):
  return float(np.mean([A.displacement(poses[v], truth[v]) for v in views])) * 1e3


def row_case(H=48, W=64, focal=130.0, K=None):
  """5 views of W x H of the three spheres on an arc, 20 degrees apart in azimuth at elevations of 10, -5, 15, 0 and -10 degrees (so
  that neighbours see much of the same surface), masks that cut a part of every view, poses perturbed by a seeded 3 mm / 1 degree, and
  a sixth entry: view 4's depth map again at a pose pushed 0.41 m along its optical axis, into the scene - its partners' points lie
  partly behind it and partly outside its image.  Pairs in both directions.  K, when given, replaces the centred camera of `focal`.
  Returns (K, truth, depths, masks, query, pairs)."""
  K = np.array([[focal, 0, W / 2 - 0.5], [0, focal, H / 2 - 0.5], [0, 0, 1.0]]) if K is None else K
  az, el = np.deg2rad([0.0, 20.0, 40.0, 60.0, 80.0]), np.deg2rad([10.0, -5.0, 15.0, 0.0, -10.0])
  eyes = 0.4 * np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
  truth = np.stack([O.look_at(e) for e in eyes])
  depths = np.stack([A.scene_depth(p, K, H, W) for p in truth])
  masks = (depths > 0).astype(np.uint8)
  masks[0, :H // 6], masks[1, :, :W // 3], masks[2, :, W - W // 3:], masks[3, H // 2 + H // 8:], masks[4, :H // 5] = 0, 0, 0, 0, 0
  rs = np.random.RandomState(7)
  query = np.stack([A.perturb(p, 0.003, 1.0, rs) for p in truth])
  pushed = query[4].copy()
  pushed[:3, 3] += 0.41 * pushed[:3, 2]
  truth, depths, masks, query = (np.concatenate([a, b[None]]) for a, b in ((truth, truth[4]), (depths, depths[4]), (masks, masks[4]), (query, pushed)))
  pairs = [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2), (3, 4), (4, 3), (0, 2), (2, 0), (4, 1), (1, 4), (3, 5), (5, 3), (1, 5), (5, 1)]
  return K, truth, depths, masks, query, pairs


def tiny_case(H=5, W=7, focal=130.0, K=None):
  """6 views of W x H (35 pixels: less than one wave of a tile) of the middle of the scene, all within a seeded 1 mm / 0.3 degrees of
  view 0 of the row case, so that the few pixels of a view land inside its partner; no mask cuts, the queries another 0.3 mm / 0.1
  degrees off, the pairs of the row case.  K as in row_case.  Returns what row_case returns."""
  K = np.array([[focal, 0, W / 2 - 0.5], [0, focal, H / 2 - 0.5], [0, 0, 1.0]]) if K is None else K
  rs = np.random.RandomState(5)
  first = O.look_at(0.4 * np.array([np.cos(np.deg2rad(10.0)), 0.0, np.sin(np.deg2rad(10.0))]))
  truth = np.stack([first] + [A.perturb(first, 0.001, 0.3, rs) for _ in range(5)])
  depths = np.stack([A.scene_depth(p, K, H, W) for p in truth])
  masks = (depths > 0).astype(np.uint8)
  query = np.stack([A.perturb(p, 0.0003, 0.1, rs) for p in truth])
  return K, truth, depths, masks, query, row_case(H, W, focal)[5]


ROW_GATE = (0.008, 0.98)     # dist_max, cos_min of the row case: tight, so that both gates skip pixels (248 and 223 over the 16 pairs)


def orbit_case():
  """24 frames of 96 x 72 around the three spheres, 15 degrees apart in azimuth, the elevation wobbling by +-15 degrees (three periods
  per turn), 0.4 m away, depth rounded to millimetres as a 16-bit PNG holds it: (K, truth, depths, masks)"""
  H, W, focal, n = 72, 96, 220.0, 24
  K = np.array([[focal, 0, W / 2 - 0.5], [0, focal, H / 2 - 0.5], [0, 0, 1.0]])
  az = np.deg2rad(15.0) * np.arange(n)
  el = np.deg2rad(15.0) * np.sin(3 * az)
  eyes = 0.4 * np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
  truth = np.stack([O.look_at(e) for e in eyes])
  depths = np.stack([A.scene_depth(p, K, H, W) for p in truth])
  depths = (np.round(depths.astype(np.float64) * 1e3) / 1e3).astype(F)
  return K, truth, depths, (depths > 0).astype(np.uint8)


# joint_refine(...) of this file on tsdf_align_oracle.refine_case() with DEFAULT_STAGES, displacement per view in mm
# (tests/test_depth_icp_host.py holds it to this record)
RECORDED_JOINT_AFTER_MM = (0.0, 0.038, 0.036, 0.038, 0.056, 0.044, 0.056, 0.061, 1.526, 0.068)
RECORDED_JOINT_MEAN_MM = 0.214
# estimate(...) of this file on orbit_case() with first_pose = truth[0]: mean and max displacement of frames 1 .. 23 in mm
RECORDED_ORBIT_ODOMETRY_MM = (25.123, 33.133)
RECORDED_ORBIT_FINAL_MM = (24.654, 32.648)
