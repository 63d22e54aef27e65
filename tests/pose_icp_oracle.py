"""numpy restatement of the rules of include/foundationpose_amd.h for polishing object poses against depth (fp_pose_depth_align,
fp_pose_gn_step, fp_pose_polish): the per-pixel row in np.float32, operation for operation in the stated order, with the reason each
pixel was skipped and the two pixel counts; the 29 sums in the device's order through tests/gn_sums_oracle.py; the step - gates, LDL^T,
pose update - in Python floats in the stated order; the loop over any source of model maps.  It imports nothing from foundationpose_amd;
the observed normals come from tests/depth_icp_oracle.py, the twist exponential and the three analytic spheres from
tests/tsdf_align_oracle.py, the camera helpers from tests/tsdf_oracle.py.

Also here, because the host and the GPU tests share them: the analytic model maps of the three spheres at a pose (no renderer is needed on
the CPU), the cases, and residual64."""
import math

import numpy as np

from tests import depth_icp_oracle as D
from tests import gn_sums_oracle as G
from tests import tsdf_align_oracle as A
from tests import tsdf_oracle as O

F = np.float32
TERMS = 29
PAIRS = A.PAIRS
SKIPS = ('background', 'outside', 'unobserved', 'distance', 'angle')      # the rule's five conditions, in its order
STOP = {0: None, 1: 'too few valid pixels', 2: 'residual rose', 3: 'singular'}
# the defaults of Utils.polish_poses (the header states them)
DEFAULT_DIST_MAX, DEFAULT_COS_MIN, DEFAULT_ITERATIONS, DEFAULT_DAMPING, DEFAULT_MIN_PIXELS = 0.010, 0.5, 8, 1e-9, 100


# ---- the per-pixel rule ---------------------------------------------------------------------------------------------------------------
def rows(xyz, normal, depth, normals4, pose, K, dist_max, cos_min, reasons=False):
  """(h,w,8) float32: J0 .. J5, r, valid per map pixel of one pose; zeros where skipped; and (rendered, observed).  With reasons=True
  also a dict of boolean maps of the pixels each condition of SKIPS skipped (in the rule's order, each among those still alive) and,
  under 'assoc', the (h,w,2) int64 frame pixel (row, col) of every map pixel that got as far as having one."""
  xyz, normal = np.asarray(xyz, dtype=F), np.asarray(normal, dtype=F)
  h, w = xyz.shape[:2]
  depth, normals4 = np.asarray(depth, dtype=F), np.asarray(normals4, dtype=F)
  H, W = depth.shape
  fx, fy, cx, cy = D._intrinsics(K)
  c = np.asarray(pose, dtype=F).reshape(4, 4)[:3, 3]
  with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
    y = [xyz[..., a] for a in range(3)]
    nm = [normal[..., a] for a in range(3)]
    ok = y[2] >= F(0.001)
    why = {'background': ~ok}
    rendered = int(ok.sum())
    u, v = (fx * y[0]) / y[2] + cx, (fy * y[1]) / y[2] + cy
    cf, rf = np.floor(u + F(0.5)), np.floor(v + F(0.5))
    inside = (cf >= F(0)) & (cf <= F(W - 1)) & (rf >= F(0)) & (rf <= F(H - 1))
    why['outside'] = ok & ~inside
    ok = ok & inside
    ci, ri = np.where(ok, cf, 0).astype(np.int64), np.where(ok, rf, 0).astype(np.int64)
    n4 = normals4[ri, ci]
    dt = depth[ri, ci]
    why['unobserved'] = ok & ~(n4[..., 3] != 0)
    ok = ok & (n4[..., 3] != 0)
    observed = int(ok.sum())
    q = [((cf - cx) / fx) * dt, ((rf - cy) / fy) * dt, dt]
    e = [y[a] - q[a] for a in range(3)]
    near = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] < F(dist_max) * F(dist_max)
    why['distance'] = ok & ~near
    ok = ok & near
    n = [n4[..., a] for a in range(3)]
    facing = (nm[0] * n[0] + nm[1] * n[1]) + nm[2] * n[2] >= F(cos_min)
    why['angle'] = ok & ~facing
    ok = ok & facing
    r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
    x = [y[a] - c[a] for a in range(3)]
    J = [n[0], n[1], n[2], x[1] * n[2] - x[2] * n[1], x[2] * n[0] - x[0] * n[2], x[0] * n[1] - x[1] * n[0]]
    got = np.stack(J + [r, np.ones_like(r)], -1)
  assert got.dtype == F and u.dtype == F and all(a.dtype == F for a in e)
  out = np.where(ok[..., None], got, F(0)).astype(F)
  if not reasons:
    return out, (rendered, observed)
  why['assoc'] = np.stack([ri, ci], -1)
  return out, (rendered, observed), why


def device_sums(rw):
  """the 29 sums of one pose's rows in the device's order: 256 threads x 4 pixels"""
  return G.device_sums(np.asarray(rw, dtype=F).reshape(-1, 8), 256, 4)


def residual64(y, n, q, c, xi):
  """r in float64 of model points y (m,3) of a pose with origin c, moved by the twist xi = (tau, w) about that origin - R <- exp([w]) R,
  t <- t + tau -, against FIXED observed points q and normals n: smooth in xi, so that a finite difference of it checks the analytic J"""
  y, n, q, c = (np.asarray(a, dtype=np.float64) for a in (y, n, q, c))
  E = A.expm_se3(np.concatenate([np.zeros(3), np.asarray(xi[3:], dtype=np.float64)]))[:3, :3]
  moved = (y - c) @ E.T + c + np.asarray(xi[:3], dtype=np.float64)
  return ((moved - q) * n).sum(1)


# ---- the step -------------------------------------------------------------------------------------------------------------------------
def ldl_solve(s, damping):
  """xi (6 Python floats) of (A + damping trace(A) I) xi = -b by LDL^T in the header's order, or None where a pivot is not > 0"""
  s = [float(v) for v in s]
  M = [[0.0] * 6 for _ in range(6)]
  for e, (i, j) in enumerate(PAIRS):
    M[i][j] = M[j][i] = s[e]
  lam = damping * (((((M[0][0] + M[1][1]) + M[2][2]) + M[3][3]) + M[4][4]) + M[5][5])
  g = [0.0] * 6
  for a in range(6):
    M[a][a] = M[a][a] + lam
    g[a] = -s[21 + a]
  L, Dg = [[0.0] * 6 for _ in range(6)], [0.0] * 6
  for j in range(6):
    d = M[j][j]
    for k in range(j):
      d = d - (L[j][k] * Dg[k]) * L[j][k]
    if not d > 0.0:
      return None
    Dg[j] = d
    for a in range(j + 1, 6):
      v = M[a][j]
      for k in range(j):
        v = v - (L[a][k] * Dg[k]) * L[j][k]
      L[a][j] = v / d
  z, xi = [0.0] * 6, [0.0] * 6
  for a in range(6):
    v = g[a]
    for k in range(a):
      v = v - L[a][k] * z[k]
    z[a] = v
  for a in range(5, -1, -1):
    v = z[a] / Dg[a]
    for k in range(a + 1, 6):
      v = v - L[k][a] * xi[k]
    xi[a] = v
  return xi


def moved_pose(pose, xi):
  """(4,4) float32: R <- (I + ca [w] + cb [w]^2) R, t <- t + tau, formed in double from the fp32 pose in the header's order, then cast"""
  P = [[float(v) for v in row] for row in np.asarray(pose, dtype=F).reshape(4, 4)]
  w0, w1, w2 = xi[3], xi[4], xi[5]
  th = math.sqrt((w0 * w0 + w1 * w1) + w2 * w2)
  if th < 1e-4:
    ca, cb = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
  else:
    ca, cb = math.sin(th) / th, (1.0 - math.cos(th)) / (th * th)
  Kx = [[0.0, -w2, w1], [w2, 0.0, -w0], [-w1, w0, 0.0]]
  out = np.asarray(pose, dtype=F).reshape(4, 4).copy()
  for a in range(3):
    E = []
    for b in range(3):
      k2 = (Kx[a][0] * Kx[0][b] + Kx[a][1] * Kx[1][b]) + Kx[a][2] * Kx[2][b]
      E.append(((1.0 if a == b else 0.0) + ca * Kx[a][b]) + cb * k2)
    for b in range(3):
      out[a, b] = F((E[0] * P[0][b] + E[1] * P[1][b]) + E[2] * P[2][b])
    out[a, 3] = F(P[a][3] + xi[a])
  return out


def fresh_state(n):
  return [dict(fit_ms=0.0, fit_count=0.0, xi=[0.0] * 6, prev_pose=np.zeros((4, 4), dtype=F), stopped=0, steps=0) for _ in range(n)]


def gn_step(sums, poses, state, damping, min_pixels, closing):
  """fp_pose_gn_step on (n,29) sums, (n,4,4) float32 poses and the list of records of fresh_state: poses and state are changed in place"""
  for i, st in enumerate(state):
    if st['stopped'] != 0:
      continue
    s = [float(v) for v in sums[i]]
    cnt = s[28]
    if not cnt >= min_pixels:
      if st['steps'] > 0:
        poses[i] = st['prev_pose']
      else:
        st['prev_pose'], st['fit_count'], st['fit_ms'] = poses[i].copy(), cnt, (s[27] / cnt if cnt > 0 else 0.0)
      st['stopped'] = 1
      continue
    ms = s[27] / cnt
    if st['steps'] > 0 and ms > st['fit_ms']:
      poses[i] = st['prev_pose']
      st['stopped'] = 2
      continue
    st['prev_pose'], st['fit_ms'], st['fit_count'] = poses[i].copy(), ms, cnt
    if closing:
      continue
    xi = ldl_solve(s, damping)
    if xi is None:
      st['stopped'] = 3
      continue
    st['xi'] = list(xi)
    poses[i] = moved_pose(poses[i], xi)
    st['steps'] += 1


def polish(maps_fn, poses, depth, normals4, K, iterations=DEFAULT_ITERATIONS, dist_max=DEFAULT_DIST_MAX, cos_min=DEFAULT_COS_MIN,
           damping=DEFAULT_DAMPING, min_pixels=DEFAULT_MIN_PIXELS, exact_sums=False):
  """fp_pose_polish: iterations + 1 rounds of maps_fn(pose (4,4) float32) -> (xyz, normal), the rows, the sums (the device's order; with
  exact_sums math.fsum, which is faster to compute and differs in the last bits only) and the step, the last round closing.  Returns
  (poses (n,4,4) float32, state, counts (n,2) of the last round)."""
  poses = np.array(poses, dtype=F).reshape(-1, 4, 4).copy()
  state = fresh_state(len(poses))
  counts = np.zeros((len(poses), 2), dtype=np.int64)
  for it in range(iterations + 1):
    sums = np.zeros((len(poses), TERMS))
    for i in range(len(poses)):
      xyz, nrm = maps_fn(poses[i])
      rw, counts[i] = rows(xyz, nrm, depth, normals4, poses[i], K, dist_max, cos_min)
      sums[i] = D.sums(rw)[0] if exact_sums else device_sums(rw)
    gn_step(sums, poses, state, damping, min_pixels, it == iterations)
  return poses, state, counts


# ---- the analytic model: the three spheres of tsdf_align_oracle at an object pose ------------------------------------------------------------
def sphere_maps(ob_in_cam, K, h, w):
  """(xyz (h,w,3), normal (h,w,3)) float32 in the camera frame of the three spheres posed by ob_in_cam (4,4), as a renderer with the
  camera K and h x w pixels would write them: the ray through every pixel centre, the nearest hit, the outward normal there; zeros where
  every ray misses.  Solved in float64."""
  K = np.asarray(K, dtype=np.float64)
  T = np.asarray(ob_in_cam, dtype=np.float64).reshape(4, 4)
  us, vs = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
  d = np.stack([(us - K[0, 2]) / K[0, 0], (vs - K[1, 2]) / K[1, 1], np.ones_like(us)], -1)
  best = np.full((h, w), np.inf)
  xyz, nrm = np.zeros((h, w, 3)), np.zeros((h, w, 3))
  with np.errstate(invalid='ignore'):
    for radius, centre in A.SPHERES:
      c = T[:3, :3] @ np.asarray(centre, dtype=np.float64) + T[:3, 3]
      a = (d * d).sum(-1)
      b = d @ c
      disc = b * b - a * (c @ c - radius * radius)
      z = (b - np.sqrt(np.where(disc > 0, disc, 0))) / a
      hit = (disc > 0) & (z > 0) & (z < best)
      p = d * z[..., None]
      best = np.where(hit, z, best)
      xyz = np.where(hit[..., None], p, xyz)
      nrm = np.where(hit[..., None], (p - c) / radius, nrm)
  return xyz.astype(F), nrm.astype(F)


def sphere_frame(truth, K, H, W):
  """the observed frame of the spheres at the pose `truth`: (depth (H,W) float32, normals (H,W,4) of the restated fp_depth_normals)"""
  depth = sphere_maps(truth, K, H, W)[0][..., 2].copy()
  return depth, D.normals(depth, K, (depth > 0).astype(np.uint8))


def object_poses(n, dist=0.4):
  """n object-in-camera poses (n,4,4) float64 of the sphere scene: the inverses of Fibonacci look-at cameras"""
  return np.stack([np.linalg.inv(O.look_at(e)) for e in O.fibonacci_eyes(n, dist)])


def perturbed(truth, trans, rot_deg, rs):
  """`truth` moved by a seeded twist about its own origin: a rotation of rot_deg degrees and a translation of `trans` metres"""
  u, w = rs.randn(3), rs.randn(3)
  out = np.array(truth, dtype=np.float64)
  out[:3, :3] = A.expm_se3(np.concatenate([np.zeros(3), w / np.linalg.norm(w) * np.deg2rad(rot_deg)]))[:3, :3] @ out[:3, :3]
  out[:3, 3] += u / np.linalg.norm(u) * trans
  return out


def displacement(pose, truth):
  """mean distance (metres) over tsdf_align_oracle's 2000 seeded points of a 5 cm ball at the object's origin between where the two
  object-in-camera poses put them"""
  a, b = np.asarray(pose, dtype=np.float64), np.asarray(truth, dtype=np.float64)
  return float(np.linalg.norm((A.BALL @ a[:3, :3].T + a[:3, 3]) - (A.BALL @ b[:3, :3].T + b[:3, 3]), axis=1).mean())


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
ROW_GATE = (0.004, 0.96)      # dist_max, cos_min of the row case: tight enough that both gates skip pixels at 4 mm / 1.5 degrees


def frame_camera(H, W, focal, shift=0.0):
  return np.array([[focal, 0, W / 2 - 0.5 + shift * W], [0, focal, H / 2 - 0.5], [0, 0, 1.0]])


def row_case(n=7, H=48, W=64, h=40, w=41, seed=6, K=None):
  """n poses of the spheres against ONE observed frame of H x W: the spheres at `truth`, seen off-centre so that the frame's right border
  cuts them.  Poses 0 .. n-1 are `truth` perturbed by 4 mm / 1.5 degrees (seeded), rendered analytically into maps of h x w through a
  camera that zooms on the object as a crop does (several map pixels land on one frame pixel) - except that pose 1's map is all
  background, pose 2 is pushed wholly outside the frame and pose 4 (when n > 4) holds a NaN and has NaN maps.  K, when given, replaces
  the frame's camera.  Returns dict(K, depth, normals, poses (n,4,4) float32, xyz, normal, truth)."""
  K = frame_camera(H, W, 1.35 * W, shift=0.42) if K is None else K
  truth = object_poses(3)[1]
  depth, nrm4 = sphere_frame(truth, K, H, W)
  rs = np.random.RandomState(seed)
  Km = frame_camera(h, w, 3.0 * w)
  poses, xyz, nrm = [], [], []
  for i in range(n):
    p = perturbed(truth, 0.004, 1.5, rs)
    if i == 2:
      p[:3, 3] += np.array([0.3, 0.0, 0.0])                              # far to the right: every point projects outside the frame
    p32 = p.astype(F)
    a, b = sphere_maps(p32, Km if i != 2 else frame_camera(h, w, 3.0 * w, shift=-2.2), h, w)
    if i == 1:
      a, b = np.zeros_like(a), np.zeros_like(b)
    if i == 4:
      p32 = p32.copy()
      p32[1, 3] = np.nan
      a, b = np.full_like(a, np.nan), np.full_like(b, np.nan)
    poses.append(p32), xyz.append(a), nrm.append(b)
  return dict(K=K, depth=depth, normals=nrm4, poses=np.stack(poses), xyz=np.stack(xyz), normal=np.stack(nrm), truth=truth)


def loop_case(n=6, H=72, W=96, focal=220.0, trans=0.004, rot_deg=1.5, seed=31):
  """n independent problems for the loop, each with its own truth: views of the spheres from n Fibonacci directions, every pose
  perturbed by trans / rot_deg (seeded).  Returns (K, truths (n,4,4), frames [(depth, normals)], given (n,4,4) float32)."""
  K = frame_camera(H, W, focal)
  truths = object_poses(n)
  rs = np.random.RandomState(seed)
  frames = [sphere_frame(t, K, H, W) for t in truths]
  given = np.stack([perturbed(t, trans, rot_deg, rs) for t in truths]).astype(F)
  return K, truths, frames, given


# ---- the end-to-end case on a mesh ------------------------------------------------------------------------------------------------------
MESH_K = np.array([[266.7, 0.0, 79.5], [0.0, 266.9, 59.5], [0.0, 0.0, 1.0]])      # a 160 x 120 frame
MESH_CROP = 64
# mean ADD after / before of the restated loop on mesh_case() with the ORACLE's rasteriser on the CPU (tests/test_pose_icp_host.py holds
# the restatement to this record; tests/test_gpu_pose_icp.py holds the library to twice the first)
RECORDED_MESH_RATIO = {'near': 0.3718, 'far': 0.1489}


def mesh_case(seed=41):
  """The mustard mesh of tests/util.scene seen in a 160 x 120 frame: (K, truth (4,4), near (8,4,4), far (8,4,4)) - `near` are 8 poses
  4 mm / 1.5 degrees off the truth, `far` 8 poses 1 cm / 5 degrees off (the tracking set's sigma), seeded; float64."""
  rs = np.random.RandomState(seed)
  q, _ = np.linalg.qr(rs.randn(3, 3))
  truth = np.eye(4)
  truth[:3, :3] = q * np.sign(np.linalg.det(q))
  truth[:3, 3] = (0.01, -0.01, 0.6)
  near = np.stack([perturbed(truth, 0.004, 1.5, rs) for _ in range(8)])
  far = np.stack([perturbed(truth, 0.010, 5.0, rs) for _ in range(8)])
  return MESH_K, truth, near, far


def add_error(pose, truth, vertices):
  """ADD: the mean distance between the model's vertices under the two poses"""
  a, b, v = np.asarray(pose, dtype=np.float64), np.asarray(truth, dtype=np.float64), np.asarray(vertices, dtype=np.float64)
  return float(np.linalg.norm((v @ a[:3, :3].T + a[:3, 3]) - (v @ b[:3, :3].T + b[:3, 3]), axis=1).mean())


def millimetres(depth):
  """a depth map rounded to whole millimetres, as a sensor delivers it"""
  return (np.round(np.asarray(depth, dtype=np.float64) * 1000.0) / 1000.0).astype(F)
