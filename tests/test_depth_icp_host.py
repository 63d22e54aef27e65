"""CPU: the numpy restatement of pairwise depth ICP (tests/depth_icp_oracle.py) against its own records and against analytic truth - the
three ray-cast spheres seen from known poses -, the joint solver of foundationpose_amd/reconstruct.py on an exactly quadratic problem,
and the argument checks of fp_depth_normals and fp_depth_pairs_align that need no GPU.  The GPU tests (tests/test_gpu_depth_icp.py)
hold the kernels to this restatement bit for bit, so what is shown here about the rules holds for them."""
import ctypes

import numpy as np
import pytest

from tests import depth_icp_oracle as D
from tests import tsdf_align_oracle as A


@pytest.fixture(scope='module')
def row_case():
  K, truth, depths, masks, query, pairs = D.row_case()
  nrm = [D.normals(depths[v], K, masks[v]) for v in range(len(depths))]
  out = [D.pair_rows(depths, nrm, K, query, s, t, *D.ROW_GATE, reasons=True) for s, t in pairs]
  return dict(K=K, truth=truth, depths=depths, masks=masks, query=query, pairs=pairs, nrm=nrm, rows=[o[0] for o in out], why=[o[1] for o in out])


def test_every_skip_reason_occurs_in_the_row_case(row_case):
  """A condition on the case the GPU rows are compared on: each of the rule's six conditions skips at least one pixel, most pairs keep
  hundreds of valid ones, and the normals of its views skip pixels at the border, next to an invalid neighbour and at a depth jump."""
  total = {k: sum(int(w[k].sum()) for w in row_case['why']) for k in D.SKIPS}
  valid = [int(r[..., 7].sum()) for r in row_case['rows']]
  print(f'skipped {total}; valid per pair {valid}')
  assert all(total[k] > 0 for k in D.SKIPS), total
  assert sum(v >= 150 for v in valid) >= 12 and sum(v == 0 for v in valid) >= 1
  seen = {}
  for v in range(5):
    _, why = D.normals(row_case['depths'][v], row_case['K'], row_case['masks'][v], reasons=True)
    for k, m in why.items():
      seen[k] = seen.get(k, 0) + int(m.sum())
  print(f'normals skipped {seen}')
  assert seen['border'] > 0 and seen['invalid'] > 0 and seen['jump'] > 0


def test_normals_face_the_camera_and_match_the_spheres(row_case):
  """unit length, n.z < 0, and within 3 degrees of the analytic normal of the sphere the pixel's point lies on, where the surface is
  tilted by less than 37 degrees (|n.z| > 0.8).  A pixel is h = 3.1 mm wide at 0.4 m; on a sphere of radius R tilted by th the two
  neighbours are an arc of a = h / (R cos th) away on either side, not quite symmetrically, and the secant through them is off the
  tangent by about a^2 tan th / 2: for R = 17 mm and th = 37 degrees, a = 0.23 and the error 0.019 rad = 1.1 degrees."""
  K, truth, depths = row_case['K'], row_case['truth'], row_case['depths']
  n4 = D.normals(depths[0], K)
  ok = n4[..., 3] != 0
  n = n4[ok][:, :3].astype(np.float64)
  assert ok.sum() > 400 and np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6 and (n[:, 2] < 0).all()
  rr, cc = np.nonzero(ok)
  d = depths[0][rr, cc].astype(np.float64)
  p = np.stack([(cc - K[0, 2]) / K[0, 0] * d, (rr - K[1, 2]) / K[1, 1] * d, d], 1)
  x = p @ truth[0][:3, :3].T + truth[0][:3, 3]
  centres = np.array([c for _, c in A.SPHERES])
  radii = np.array([r for r, _ in A.SPHERES])
  which = np.abs(np.linalg.norm(x[:, None] - centres[None], axis=2) - radii[None]).argmin(1)
  want = (x - centres[which]) / radii[which][:, None]
  got = n @ truth[0][:3, :3].T
  cos = (want * got).sum(1)[np.abs(n[:, 2]) > 0.8]
  print(f'{len(cos)} pixels: smallest cosine to the analytic normal {cos.min():.5f}')
  assert len(cos) > 200 and cos.min() > np.cos(np.deg2rad(3.0))


def test_analytic_jacobian_is_the_derivative_of_the_residual(row_case):
  """J of a pixel against the central difference of the float64 residual at FIXED association under exp(eps e_k) applied to view s, and
  -J under the same twist applied to view t.  eps = 1e-6.  Tolerance 1e-5: the residual is linear in the translation and the difference
  quotient's own error is 1e-16 x 0.5 m / 2e-6 = 3e-11; J is fp32 - the normal's components carry 2^-24, the matrices are cast to fp32
  (6e-8), the point's coordinates carry up to 4 roundings of 2^-24 x 0.5 m, and the rotation entries are products with |x| < 0.5:
  below 1e-6 in all.  A wrong sign, axis or frame is an error of order 0.1 - 1."""
  K, depths, query = row_case['K'], row_case['depths'], row_case['query']
  k = row_case['pairs'].index((0, 1))
  rw, why = row_case['rows'][k], row_case['why'][k]
  pix = np.argwhere(rw[..., 7] > 0)
  assert len(pix) >= 200
  tp = why['assoc'][pix[:, 0], pix[:, 1]]
  n_t = row_case['nrm'][1][tp[:, 0], tp[:, 1], :3].astype(np.float64)
  r0 = D.residual64(depths, K, query, 0, 1, pix, tp, n_t)
  assert np.abs(r0 - rw[pix[:, 0], pix[:, 1], 6]).max() < 1e-6
  J = rw[pix[:, 0], pix[:, 1], :6].astype(np.float64)
  worst_s = worst_t = 0.0
  for view, sign in ((0, 1.0), (1, -1.0)):
    for a in range(6):
      eps = 1e-6 * np.eye(6)[a]
      moved = lambda e: [A.expm_se3(e) @ q if v == view else q for v, q in enumerate(query)]
      fd = (D.residual64(depths, K, moved(eps), 0, 1, pix, tp, n_t) - D.residual64(depths, K, moved(-eps), 0, 1, pix, tp, n_t)) / 2e-6
      err = np.abs(fd - sign * J[:, a]).max()
      worst_s, worst_t = (max(worst_s, err), worst_t) if view == 0 else (worst_s, max(worst_t, err))
  print(f'{len(pix)} pixels: max |J - d r / d xi_s| {worst_s:.3e}, max |-J - d r / d xi_t| {worst_t:.3e}')
  assert worst_s < 1e-5 and worst_t < 1e-5
  assert np.abs(np.linalg.norm(J[:, :3], axis=1) - 1).max() < 1e-5      # the translation part is a unit normal


def test_joint_refinement_reproduces_its_record():
  """joint_refine of the restatement (fp32 rule, DEFAULT_STAGES, pairs = 4 nearest by optical axis) on tsdf_align_oracle.refine_case():
  mean displacement of views 1 .. 9 from 4.064 mm to 0.214 mm - the same as the float64 experiment - against 0.492 mm of the recorded
  sequential TSDF procedure.  View 8, which sees the spheres nearly in line, ends at 1.526 mm (TSDF: 2.738 mm) and has by far the
  smallest eigenvalue ratio; the others end at 0.036 - 0.068 mm."""
  K, truth, depths, masks, given = A.refine_case()
  got, info = D.joint_refine(depths, masks, K, given)
  after = np.array([A.displacement(got[v], truth[v]) for v in range(10)]) * 1e3
  print(f'after {np.round(after, 3)} mean {after[1:].mean():.3f} mm; rms {np.round(1e3 * np.array(info["rms"]), 3)}; eig ratio {info["eig_ratio"]}')
  assert np.abs(after - D.RECORDED_JOINT_AFTER_MM).max() < 1e-3 and abs(after[1:].mean() - D.RECORDED_JOINT_MEAN_MM) < 1e-3
  assert np.array_equal(got[0], given[0]) and info['stopped'] == {}
  assert D.RECORDED_JOINT_MEAN_MM < A.RECORDED_MEAN_MM
  assert len(info['rms']) == 21 and info['rms'][-1] < 0.05 * info['rms'][0]
  assert np.nanargmin(info['eig_ratio']) == 8 and info['eig_ratio'][8] < 0.1 * np.delete(info['eig_ratio'], 8).min()


def test_orbit_reproduces_its_record():
  """estimate of the restatement on orbit_case() with first_pose = truth[0].  The odometry holds frames 1 .. 4 to 0.06 mm, loses 16 mm
  at frame 5 (azimuth 75 degrees, where the spheres line up) and more up to frame 10, and carries 33 mm to the end: mean 25.123 mm.
  The joint pass cannot close a gap that is three times its first gate (10 mm): mean 24.654 mm, below the odometry's, which is all
  that is asserted of it.  (The issue's float64 experiment lost 15 mm once and closed the loop to 0.059 mm; its orbit is not
  reproduced by this one - DESIGN.md section 5.)"""
  K, truth, depths, masks = D.orbit_case()
  got, info = D.estimate(depths, masks, K, first_pose=truth[0])
  odo = np.array([A.displacement(info['odometry'][v], truth[v]) for v in range(24)]) * 1e3
  fin = np.array([A.displacement(got[v], truth[v]) for v in range(24)]) * 1e3
  print(f'odometry {np.round(odo, 3)} mean {odo[1:].mean():.3f}; final {np.round(fin, 3)} mean {fin[1:].mean():.3f}')
  assert abs(odo[1:].mean() - D.RECORDED_ORBIT_ODOMETRY_MM[0]) < 1e-2 and abs(odo.max() - D.RECORDED_ORBIT_ODOMETRY_MM[1]) < 1e-2
  assert abs(fin[1:].mean() - D.RECORDED_ORBIT_FINAL_MM[0]) < 1e-2 and abs(fin.max() - D.RECORDED_ORBIT_FINAL_MM[1]) < 1e-2
  assert D.RECORDED_ORBIT_FINAL_MM[0] < D.RECORDED_ORBIT_ODOMETRY_MM[0]
  assert np.array_equal(got[0], truth[0]) and odo[1:5].max() < 0.1


def test_choose_pairs_takes_the_nearest_axes():
  K, truth, depths, masks, given = A.refine_case()
  pr = D.choose_pairs(truth, 4, 100)
  assert len(pr) == len(set(pr)) and all(s != t for s, t in pr)
  axes = truth[:, :3, 2]
  for s in range(10):
    mine = [t for a, t in pr if a == s]
    cos = axes @ axes[s]
    rest = [t for t in range(10) if t != s and t not in mine]
    assert 1 <= len(mine) <= 4 and all(cos[t] >= np.cos(np.deg2rad(100)) for t in mine)
    assert all(cos[t] <= min(cos[m] for m in mine) or cos[t] < np.cos(np.deg2rad(100)) for t in rest)
  assert D.choose_pairs(truth, 2, 1.0) == []                                   # nothing within a degree
  same = np.stack([truth[0]] * 4)
  assert [t for s, t in D.choose_pairs(same, 2, 100) if s == 3] == [0, 1]      # ties: the lowest index


@pytest.fixture(scope='module')
def built():
  import __graft_entry__ as g
  g.build()
  from foundationpose_amd import _lib
  return _lib


def _quadratic_problem():
  """5 views: 0 fixed, 1 .. 3 with known twists, 4 without a residual.  Pair (s,t): rows J with r = -J (xi_s - xi_t), so that the
  linearised residual r + J (xi_s - xi_t) vanishes at the known twists; the 29 sums in float64."""
  rs = np.random.RandomState(9)
  truth = np.zeros((5, 6))
  truth[1:4] = rs.randn(3, 6) * 0.01
  pairs = [(0, 1), (1, 0), (1, 2), (2, 3), (3, 1), (3, 0), (4, 0), (2, 4)]
  sm = np.zeros((len(pairs), 29))
  for k, (s, t) in enumerate(pairs):
    if 4 in (s, t):
      continue
    J = rs.randn(40, 6)
    r = -J @ (truth[s] - truth[t])
    JtJ = J.T @ J
    sm[k] = np.concatenate([[JtJ[i, j] for i, j in A.PAIRS], J.T @ r, [r @ r, 40.0]])
  return truth, pairs, sm


def test_solve_joint_step_recovers_known_twists(built):
  from foundationpose_amd import reconstruct as R
  truth, pairs, sm = _quadratic_problem()
  for solve in (R.solve_joint_step, D.solve_joint_step):
    xi, dropped = solve(sm, pairs, 5, [0], damping=0.0)
    assert dropped == [4] and (xi[0] == 0).all() and (xi[4] == 0).all()
    assert np.abs(xi - truth).max() < 1e-12
    xi, dropped = solve(sm, pairs, 5, [0, 2], damping=0.0)                      # view 2 held at zero: no longer the minimum of the others
    assert (xi[2] == 0).all() and (xi[0] == 0).all() and dropped == [4] and np.abs(xi[1] - truth[1]).max() > 1e-4
    xi, _ = solve(sm, pairs, 5, [0])
    assert 0 < np.abs(xi - truth).max() < 1e-6                                   # the default damping moves the answer by 1e-9 of it
    xi, dropped = solve(sm, pairs, 5, [0, 1, 2, 3, 4])
    assert (xi == 0).all() and dropped == []
  a, b = R.solve_joint_step(sm, pairs, 5, [0])[0], D.solve_joint_step(sm, pairs, 5, [0])[0]
  assert np.allclose(a, b, rtol=1e-10, atol=1e-15)
  K, truth_p, depths, masks, given = A.refine_case()
  assert R.choose_pairs(given, 4, 100) == D.choose_pairs(given, 4, 100)
  assert R.DEFAULT_STAGES == D.DEFAULT_STAGES and R.ODOMETRY_STAGES == D.ODOMETRY_STAGES and R.ESTIMATE_JOINT_STAGES == D.ESTIMATE_JOINT_STAGES


def test_argument_checks_need_no_gpu(built):
  L, EINVAL = built.lib(), built.FP_EINVAL
  dbl = lambda *a: (ctypes.c_double * len(a))(*a)
  K = dbl(100, 0, 4, 0, 100, 4, 0, 0, 1)
  fake = ctypes.c_void_p(64)                     # never dereferenced: the null and range checks come first
  # fp_depth_normals
  call = lambda ctx=fake, depth=fake, n=1, Hh=8, Ww=8, Kk=K, zfar=1.0, jump=0.01, out=fake: \
      L.fp_depth_normals(ctx, depth, None, n, Hh, Ww, Kk, zfar, jump, out, None)
  for kw in (dict(ctx=None), dict(depth=None), dict(Kk=None), dict(out=None)):
    assert call(**kw) == EINVAL and b'null' in L.fp_last_error(), kw
  for kw in (dict(n=-1), dict(n=built.FP_TSDF_MAX_VIEWS + 1), dict(Hh=0), dict(Ww=0), dict(zfar=0.0), dict(zfar=float('nan')), dict(jump=0.0),
             dict(jump=float('nan')), dict(jump=-1.0), dict(Kk=dbl(0, 0, 4, 0, 100, 4, 0, 0, 1)), dict(Kk=dbl(100, 0, 4, 0, -1, 4, 0, 0, 1)),
             dict(Kk=dbl(100, 0, float('nan'), 0, 100, 4, 0, 0, 1)), dict(Kk=dbl(float('inf'), 0, 4, 0, 100, 4, 0, 0, 1))):
    assert call(**kw) == EINVAL, kw
  assert call(out=ctypes.c_void_p(68)) == EINVAL and b'aligned' in L.fp_last_error()
  assert call(n=0) == 0                          # nothing to do: returns before anything is touched
  # fp_depth_pairs_align
  poses = np.ascontiguousarray(np.stack([np.eye(4)] * 3))
  pp = lambda a: ctypes.c_void_p(a.ctypes.data)
  pr = np.array([[0, 1], [2, 0]], dtype=np.int32)
  sums = np.zeros((2, 29))

  def call2(ctx=fake, depth=fake, nrm=fake, n=3, Hh=8, Ww=8, Kk=K, p=poses, pairs=pr, P=2, dist=0.01, cos=0.5, rows=None, out=sums):
    return L.fp_depth_pairs_align(ctx, depth, nrm, n, Hh, Ww, Kk, None if p is None else pp(p), None if pairs is None else pp(pairs), P, dist, cos, rows,
                                  None if out is None else pp(out), None)
  for kw in (dict(ctx=None), dict(depth=None), dict(nrm=None), dict(Kk=None), dict(p=None), dict(out=None), dict(pairs=None)):
    assert call2(**kw) == EINVAL and b'null' in L.fp_last_error(), kw
  for kw in (dict(n=-1), dict(n=built.FP_TSDF_MAX_VIEWS + 1), dict(P=-1), dict(P=built.FP_DEPTH_ALIGN_MAX_PAIRS + 1), dict(Hh=0), dict(Ww=-2),
             dict(dist=0.0), dict(dist=float('nan')), dict(cos=1.5), dict(cos=-1.01), dict(cos=float('nan')),
             dict(Kk=dbl(0, 0, 4, 0, 100, 4, 0, 0, 1)), dict(Kk=dbl(100, 0, 4, 0, float('nan'), 4, 0, 0, 1)),
             dict(pairs=np.array([[0, 3], [1, 0]], dtype=np.int32)), dict(pairs=np.array([[0, 1], [-1, 0]], dtype=np.int32)),
             dict(pairs=np.array([[0, 1], [2, 2]], dtype=np.int32)), dict(n=2)):
    assert call2(**kw) == EINVAL, kw
  assert call2(pairs=np.array([[1, 1], [0, 1]], dtype=np.int32)) == EINVAL and b'itself' in L.fp_last_error()
  bad = poses.copy()
  bad[1, 3, 3] = 2
  assert call2(p=bad) == EINVAL and b'last row' in L.fp_last_error()
  bad = poses.copy()
  bad[2, 1, 2] = np.inf
  assert call2(p=bad) == EINVAL and b'finite' in L.fp_last_error()
  assert call2(nrm=ctypes.c_void_p(72)) == EINVAL and b'aligned' in L.fp_last_error()
  assert call2(rows=ctypes.c_void_p(68)) == EINVAL and b'aligned' in L.fp_last_error()
  before = sums.copy()
  assert call2(P=0) == 0 and call2(P=0, pairs=None) == 0 and np.array_equal(sums, before)      # zero pairs: nothing is touched
  assert built.FP_DEPTH_ALIGN_TERMS == 29 and built.FP_DEPTH_ALIGN_MAX_PAIRS == 256
