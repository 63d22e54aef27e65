"""CPU: tests/mesh_align_oracle.py - the restatement of fp_points_mesh_align / fp_points_mesh_polish that the GPU tests hold the kernels
to - checked on its own: the analytic J of both modes against finite differences of the residual under the step's own pose update, the
24 starts as a group, the float64 loop on the asymmetric two-box mesh (the values recorded here are the bounds of
tests/test_gpu_mesh_align.py), and the argument checks of the two calls that need no GPU."""
import ctypes

import numpy as np
import pytest

from tests import mesh_align_oracle as M
from tests import pose_icp_oracle as P
from tests import surface_distance_oracle as SD


@pytest.mark.parametrize('mode', ['plane', 'point'])
def test_J_is_the_derivative_of_the_residual_under_the_step(mode):
  """J of a row against the central difference of its residual when the pose moves by pose_icp_oracle.moved_pose's rule (R <- exp([w]) R,
  t <- t + tau, in double) at FIXED association: closest point and normal are held, as the linearisation holds them."""
  v, f = M.two_box_mesh(fine=False)
  rs = np.random.RandomState(3)
  pts = SD.sample_surface(v, f, 64, 1)[0] + rs.normal(scale=0.003, size=(64, 3))
  pose = M.random_rigid(rs, 40.0, 0.2)
  src = (pts - pose[:3, 3]) @ pose[:3, :3]                          # pose^-1 pts
  normals = M.face_normals(v, f)
  rw, _ = M.linearise64(src, pose, v, f, normals, mode, 1.0)
  q = src @ pose[:3, :3].T + pose[:3, 3]
  _, face, closest = SD.point_mesh_distance(q, v, f)
  assert (rw[:, 0, 7] == 1).all()

  def residual(xi):
    # moved_pose in float64 (its fp32 cast would swamp the difference): E R, t + tau
    w = np.asarray(xi[3:])
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    E = np.eye(3) + (np.sin(th) / th if th > 0 else 1.0) * K + ((1 - np.cos(th)) / th ** 2 if th > 0 else 0.5) * (K @ K)
    y = src @ (E @ pose[:3, :3]).T + pose[:3, 3] + np.asarray(xi[:3])
    e = y - closest
    return (e * normals[face]).sum(1)[:, None] if mode == 'plane' else e

  h = 1e-6
  for a in range(6):
    xi = np.zeros(6)
    xi[a] = h
    fd = (residual(xi) - residual(-xi)) / (2 * h)                    # (n, R)
    np.testing.assert_allclose(rw[:, :, a], fd, rtol=0, atol=1e-8)
  np.testing.assert_allclose(rw[:, :, 6], residual(np.zeros(6)), rtol=0, atol=1e-15)
  # the fp32 pose update agrees with that float64 rule to fp32 rounding
  xi = [0.001, -0.002, 0.0005, 0.01, -0.02, 0.015]
  moved = P.moved_pose(pose.astype(np.float32), xi)
  assert np.abs(moved[:3, 3] - (pose[:3, 3] + xi[:3])).max() < 1e-7


def test_rows_mask_what_the_rule_leaves_out():
  """a NaN distance, a distance beyond the gate and a zero normal (plane) are zero rows; the point rows carry one count a point; -0.0
  never appears where a row is masked"""
  q = np.array([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [np.nan, 0, 0]], np.float32)
  closest = np.array([[0.1, 0.2, 0.29], [0.1, 0.2, 0.1], [0.1, 0.2, 0.29], [np.nan] * 3], np.float32)
  dist = np.array([0.01, 0.2, 0.01, np.nan], np.float32)
  normal = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 0]], np.float32)
  pl = M.rows(q, dist, closest, normal, np.eye(4), 'plane', 0.05)
  assert pl.shape == (4, 1, 8) and pl[0, 0, 7] == 1 and not pl[1:].any() and not np.signbit(pl[1:]).any()
  pt = M.rows(q, dist, closest, normal, np.eye(4), 'point', 0.05)
  assert pt.shape == (4, 3, 8) and (pt[[0, 2], 0, 7] == 1).all() and not pt[:, 1:, 7].any() and not pt[[1, 3]].any()
  s = M.device_sums(pt)
  assert s[28] == 2 and abs(s[27] - 2 * float(np.float32(0.3) - np.float32(0.29)) ** 2) < 1e-12
  assert M.device_sums(pl)[28] == 1


def test_device_sums_of_three_rows_a_point_follow_the_lane_order():
  """the restated order against a direct loop over (tile, lane, q, axis) on a ragged two-tile case"""
  rs = np.random.RandomState(0)
  rw = rs.normal(size=(1500, 3, 8)).astype(np.float32)
  rw[..., 7] = 0
  rw[:, 0, 7] = 1
  got = M.device_sums(rw)
  x = np.zeros((2048, 3, 8), np.float32)
  x[:1500] = rw
  x = x.astype(np.float64)
  want = np.zeros(29)
  for tile in range(2):
    lanes = np.zeros((256, 29))
    for q in range(4):
      for ax in range(3):
        r = x[tile * 1024 + q * 256 + np.arange(256), ax]
        J, res = r[:, :6], r[:, 6]
        terms = [J[:, i] * J[:, j] for i in range(6) for j in range(i, 6)] + [J[:, i] * res for i in range(6)] + [res * res, (r[:, 7] != 0) * 1.0]
        lanes = lanes + np.stack(terms, 1)
    waves = lanes.reshape(4, 64, 29)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
      waves = waves + waves[:, lane ^ o]
    slot = waves[0, 0]
    for w in range(1, 4):
      slot = slot + waves[w, 0]
    want = want + slot
  assert np.array_equal(got, want) and got[28] == 1500


def test_the_24_starts_are_the_rotation_group_of_the_cube():
  g = M.cube_rotations()
  assert g.shape == (24, 3, 3) and np.array_equal(g[0], np.eye(3))
  assert np.allclose(np.linalg.det(g), 1.0) and all(np.array_equal(r @ r.T, np.eye(3)) for r in g)
  keys = {tuple(r.reshape(-1).astype(int)) for r in g}
  assert len(keys) == 24                                              # distinct
  assert all(tuple((a @ b).reshape(-1).astype(int)) in keys for a in g for b in g)      # closed under composition
  from foundationpose_amd import mesh_align as MA
  assert np.array_equal(MA.cube_rotations(), g)
  # the product's starts are the restated ones
  v, f = M.two_box_mesh()
  from foundationpose_amd import symmetry as S
  _, c, cov = S.surface_moments(v, f)
  ct, at, _ = M.principal_frame_of_mesh(v, f)
  assert np.allclose(c, ct) and np.allclose(S.principal_axes(cov)[1], at)
  st = MA.axes_starts(c + 0.1, at[[1, 2, 0]], c, at)
  assert np.allclose(st, M.axes_starts(c + 0.1, at[[1, 2, 0]], c, at)) and np.allclose(np.linalg.det(st[:, :3, :3]), 1.0)
  assert np.allclose(np.einsum('kij,j->ki', st[:, :3, :3], c + 0.1) + st[:, :3, 3], c)      # every start lays centroid on centroid


def test_the_two_box_mesh_has_no_symmetry_to_hide_behind():
  v, f = M.two_box_mesh()
  assert len(f) == 504
  _, _, w = M.principal_frame_of_mesh(v, f)
  assert w[1] / w[0] > 1.3 and w[2] / w[1] > 1.3                      # distinct eigenvalues: the principal axes are well defined
  c, fc = M.two_box_mesh(fine=False)
  assert len(fc) == 24 and np.allclose(M.principal_frame_of_mesh(c, fc)[0], M.principal_frame_of_mesh(v, f)[0])


@pytest.mark.parametrize('name', ['near', 'far'])
def test_oracle_loop_recovers_an_offset(name):
  """4 mm / 1.5 degrees and 1 cm / 5 degrees on the two-box mesh, 1024 noisy samples (sigma 0.5 mm), the default stages.  The mean
  displacement of the vertices ends at M.RECORDED[name] - 0.116 mm, the noise's share - from 4.3 mm and 11.4 mm.  Run on the coarse
  tessellation of the same surface: the exact distance does not depend on it (checked on the fine one when the values were recorded)."""
  trans, rot = M.OFFSETS[name]
  v, f, src, truth, start = M.offset_case(trans, rot, fine=False)
  vf = M.two_box_mesh()[0]
  before = M.displacement(start, truth, vf)
  poses, state = M.polish64(src, v, f, start[None], M.default_stages(M.exact_diameter(vf)))
  after = M.displacement(poses[0], truth, vf)
  print(f'{name}: displacement {before * 1e3:.3f} mm -> {after * 1e3:.4f} mm; rms {state[0]["fit_ms"] ** 0.5 * 1e3:.4f} mm; stopped {state[0]["stopped"]}')
  assert before > 0.8 * trans and after < 0.05 * before
  assert abs(after - M.RECORDED[name]) < 1e-6                         # the recorded value is this run's


def test_oracle_loop_from_the_24_axes_starts_recovers_an_arbitrary_rotation_without_the_bottom():
  """the `no bottom` source - 512 noisy samples of every face that does not face -z - under a seeded rotation of 60 to 180 degrees: the
  start of lowest ungated mean squared distance is the right one, and nothing else comes close"""
  v, f, src, truth = M.no_bottom_case(fine=False)
  vf = M.two_box_mesh()[0]
  cs, as_, _ = M.principal_frame_of_points(src)
  ct, at, _ = M.principal_frame_of_mesh(v, f)
  starts = M.axes_starts(cs, as_, ct, at)
  poses, _ = M.polish64(src, v, f, starts.astype(np.float32), M.default_stages(M.exact_diameter(vf)))
  ms = np.array([M.mean_square_distance(src, p, v, f) for p in poses])
  k = M.choose(ms)
  disp = M.displacement(poses[k], truth, vf)
  print(f'chosen {k}: displacement {disp * 1e3:.4f} mm (start {M.displacement(starts[k], truth, vf) * 1e3:.2f} mm); rms mm {np.round(np.sqrt(ms) * 1e3, 2)}')
  assert M.rotation_angle_deg(np.eye(3), truth[:3, :3]) > 59
  assert abs(disp - M.RECORDED['no_bottom']) < 1e-6
  assert np.sort(ms)[1] > 100 * ms[k]                                 # no second candidate


@pytest.fixture(scope='module')
def built():
  import __graft_entry__ as g
  g.build()
  from foundationpose_amd import _lib
  return _lib


def test_argument_checks_need_no_gpu(built):
  L, EINVAL = built.lib(), built.FP_EINVAL
  assert built.MESH_ALIGN_STAGE_DTYPE.itemsize == 12 and built.FP_MESH_ALIGN_MODES == M.MODES
  fake = ctypes.c_void_p(64)                     # never dereferenced: the null and range checks come first
  nan = float('nan')

  def align(ctx=fake, pts=fake, n=8, poses=fake, N=1, pos=fake, V=3, faces=fake, F=1, mode=0, dist=0.01, keys=fake, rows=None, sums=fake):
    return L.fp_points_mesh_align(ctx, pts, n, poses, N, pos, V, faces, F, mode, dist, keys, None, None, None, None, None, rows, sums, None, None)
  for kw in (dict(ctx=None), dict(poses=None), dict(pos=None), dict(faces=None), dict(keys=None), dict(sums=None), dict(pts=None)):
    assert align(**kw) == EINVAL and b'null' in L.fp_last_error(), kw
  for kw in (dict(N=-1), dict(N=built.FP_POSE_ALIGN_MAX_POSES + 1), dict(n=-1), dict(N=1024, n=(1 << 14) + 1), dict(V=0), dict(F=0),
             dict(F=built.FP_SURFDIST_MAX_FACES + 1), dict(mode=2), dict(mode=-1), dict(dist=0.0), dict(dist=-1.0), dict(dist=nan)):
    assert align(**kw) == EINVAL, kw
  assert align(keys=ctypes.c_void_p(68)) == EINVAL and b'aligned' in L.fp_last_error()
  assert align(rows=ctypes.c_void_p(72)) == EINVAL and b'aligned' in L.fp_last_error()
  assert align(N=0) == 0                         # nothing to do: returns before anything is touched

  def stages(*s):
    a = np.zeros(len(s), built.MESH_ALIGN_STAGE_DTYPE)
    for k, x in enumerate(s):
      a[k] = x
    return a
  ok = stages((1, 0.05, 3), (0, 0.01, 3))

  def polish(ctx=fake, pts=fake, n=8, poses=fake, N=1, pos=fake, V=3, faces=fake, F=1, st=ok, n_st=None, damping=1e-9, min_points=100, state=fake,
             sums=fake, keys=fake):
    return L.fp_points_mesh_polish(ctx, pts, n, poses, N, pos, V, faces, F, None if st is None else st.ctypes.data, len(st) if n_st is None else n_st,
                                   damping, min_points, state, sums, keys, None)
  for kw in (dict(ctx=None), dict(poses=None), dict(pos=None), dict(faces=None), dict(keys=None), dict(sums=None), dict(state=None),
             dict(st=None, n_st=1), dict(pts=None)):
    assert polish(**kw) == EINVAL and b'null' in L.fp_last_error(), kw
  for kw in (dict(N=-1), dict(N=1025), dict(n=-1), dict(V=0), dict(F=0), dict(n_st=0), dict(n_st=9), dict(st=stages((2, 0.1, 1))),
             dict(st=stages((0, 0.0, 1))), dict(st=stages((0, 0.1, -1))), dict(st=stages((0, 0.1, built.FP_POSE_POLISH_MAX_ITERATIONS + 1))),
             dict(damping=-1.0), dict(damping=nan), dict(min_points=0)):
    assert polish(**kw) == EINVAL, kw
  assert polish(state=ctypes.c_void_p(68)) == EINVAL and b'aligned' in L.fp_last_error()
  assert polish(keys=ctypes.c_void_p(68)) == EINVAL and b'aligned' in L.fp_last_error()
  assert polish(N=0) == 0
