"""CPU: the numpy restatement of polishing poses against depth (tests/pose_icp_oracle.py) against analytic truth - the three ray-cast
spheres, model maps and observed depth from the same formula - and the argument checks of fp_pose_depth_align, fp_pose_gn_step and
fp_pose_polish that need no GPU.  The GPU tests (tests/test_gpu_pose_icp.py) hold the kernels to this restatement bit for bit, so what
is shown here about the rules holds for them."""
import ctypes

import numpy as np
import pytest

from tests import pose_icp_oracle as P


@pytest.fixture(scope='module')
def row_case():
  c = P.row_case()
  out = [P.rows(c['xyz'][i], c['normal'][i], c['depth'], c['normals'], c['poses'][i], c['K'], *P.ROW_GATE, reasons=True) for i in range(len(c['poses']))]
  c.update(rows=[o[0] for o in out], counts=[o[1] for o in out], why=[o[2] for o in out])
  return c


def test_every_skip_reason_occurs_in_the_row_case(row_case):
  """A condition on the case the GPU rows are compared on: each of the rule's five conditions skips at least one pixel, most poses keep
  150 valid pixels or more, and the three special poses (background map, outside the frame, NaN) keep none."""
  total = {k: sum(int(w[k].sum()) for w in row_case['why']) for k in P.SKIPS}
  valid = [int(r[..., 7].sum()) for r in row_case['rows']]
  print(f'skipped {total}; valid per pose {valid}; (rendered, observed) {row_case["counts"]}')
  assert all(total[k] > 0 for k in P.SKIPS), total
  assert sum(v >= 150 for v in valid) > len(valid) / 2 and [valid[i] for i in (1, 2, 4)] == [0, 0, 0]
  assert row_case['counts'][1] == (0, 0) and row_case['counts'][2][0] > 0 and row_case['counts'][2][1] == 0 and row_case['counts'][4] == (0, 0)
  for i, r in enumerate(row_case['rows']):
    assert row_case['counts'][i][0] >= row_case['counts'][i][1] >= valid[i]
    assert not np.isnan(r).any()


def test_model_normals_face_the_camera(row_case):
  """both normal maps of the rule face the camera: n.z < 0 wherever there is one"""
  nm = row_case['normal'][0]
  assert (nm[row_case['xyz'][0][..., 2] > 0][:, 2] < 0).all()
  n4 = row_case['normals']
  assert (n4[n4[..., 3] != 0][:, 2] < 0).all()


def test_analytic_jacobian_is_the_derivative_of_the_residual(row_case):
  """J of a pixel against the central difference of the float64 residual at FIXED association under the twist eps e_k about the pose's
  origin.  eps = 1e-6.  Tolerance 1e-6: the residual is linear in the translation and even terms of the rotation's series cancel in a
  central difference, which leaves eps^2 |x| / 6 < 1e-13; the quotient's own rounding is 1e-16 x 0.5 m / 2e-6 = 3e-11.  J is fp32:
  x = y - c carries one rounding of 2^-24 x 0.5 m = 3e-8, each product with |n| <= 1 and the difference of two of them another 2^-24 x
  0.1: below 1e-7 in all.  A wrong sign, axis or origin (the camera's instead of the pose's: |c| = 0.4 m) is an error of order 0.1 - 1."""
  i = 0
  rw, why = row_case['rows'][i], row_case['why'][i]
  pix = np.argwhere(rw[..., 7] > 0)
  assert len(pix) >= 150
  K = np.asarray(row_case['K'], dtype=np.float64)
  y = row_case['xyz'][i][pix[:, 0], pix[:, 1]].astype(np.float64)
  tp = why['assoc'][pix[:, 0], pix[:, 1]]
  n = row_case['normals'][tp[:, 0], tp[:, 1], :3].astype(np.float64)
  d = row_case['depth'][tp[:, 0], tp[:, 1]].astype(np.float64)
  q = np.stack([(tp[:, 1] - K[0, 2]) / K[0, 0] * d, (tp[:, 0] - K[1, 2]) / K[1, 1] * d, d], 1)
  c = row_case['poses'][i][:3, 3].astype(np.float64)
  r0 = P.residual64(y, n, q, c, np.zeros(6))
  assert np.abs(r0 - rw[pix[:, 0], pix[:, 1], 6]).max() < 1e-6
  J = rw[pix[:, 0], pix[:, 1], :6].astype(np.float64)
  worst = 0.0
  for a in range(6):
    eps = 1e-6 * np.eye(6)[a]
    fd = (P.residual64(y, n, q, c, eps) - P.residual64(y, n, q, c, -eps)) / 2e-6
    worst = max(worst, np.abs(fd - J[:, a]).max())
  print(f'{len(pix)} pixels: max |J - d r / d xi| {worst:.3e}')
  assert worst < 1e-6
  assert np.abs(np.linalg.norm(J[:, :3], axis=1) - 1).max() < 1e-5      # the translation part is a unit normal


def test_ldl_step_solves_the_damped_system():
  """the restated LDL^T against numpy's solver on a random positive definite system, and its refusal of a singular one"""
  rs = np.random.RandomState(3)
  Jm, r = rs.randn(50, 6), rs.randn(50) * 1e-3
  Am, b = Jm.T @ Jm, Jm.T @ r
  s = np.concatenate([[Am[i, j] for i, j in P.PAIRS], b, [r @ r, 50.0]])
  xi = np.array(P.ldl_solve(s, 1e-9))
  want = np.linalg.solve(Am + 1e-9 * np.trace(Am) * np.eye(6), -b)
  assert np.abs(xi - want).max() < 1e-12 * np.abs(want).max() * np.linalg.cond(Am)
  flat = Jm.copy()
  flat[:, 5] = 0                                                          # nothing constrains the last coordinate
  Af = flat.T @ flat
  sf = np.concatenate([[Af[i, j] for i, j in P.PAIRS], flat.T @ r, [r @ r, 50.0]])
  assert P.ldl_solve(sf, 0.0) is None and P.ldl_solve(sf, 1e-9) is not None      # the damping only keeps the solve finite


def test_loop_brings_every_pose_closer():
  """The restated loop with the defaults on loop_case(): 6 views of the spheres, each pose 4 mm / 1.5 degrees off.  Model maps and
  observed depth come from the same ray-caster, so the fit can close to the fp32 rounding of the rule; every pose must end closer."""
  K, truths, frames, given = P.loop_case()
  H, W = frames[0][0].shape
  before, after, stopped = [], [], []
  for i in range(len(given)):
    got, st, _ = P.polish(lambda p: P.sphere_maps(p, K, H, W), given[i:i + 1], frames[i][0], frames[i][1], K, exact_sums=True)
    before.append(P.displacement(given[i], truths[i]) * 1e3)
    after.append(P.displacement(got[0], truths[i]) * 1e3)
    stopped.append(P.STOP[st[0]['stopped']])
  print(f'displacement mm before {np.round(before, 3)} after {np.round(after, 4)} stopped {stopped}')
  assert all(a < b for a, b in zip(after, before)) and np.mean(after) < 0.05 * np.mean(before)


def test_mesh_case_reproduces_its_record():
  """The CPU experiment behind the defaults and behind the bound of tests/test_gpu_pose_icp.py: the restated loop with the defaults on
  mesh_case() - the mustard mesh through the ORACLE's rasteriser, the observed depth rounded to millimetres, crop 64.  Mean ADD over the
  model's vertices: 4.19 -> 1.56 mm for the 8 poses 4 mm / 1.5 degrees off (ratio 0.3718), 10.59 -> 1.58 mm for the 8 poses 1 cm / 5 degrees
  off (ratio 0.1489); every pose ends closer, all within 0.13 mm of one another: the bottle is nearly a body of revolution, and what is
  left is the slide about its axis that geometry alone cannot hold."""
  from oracle import geometry as G
  from oracle.render import nvdiffrast_render as render
  from tests import util
  sc = util.scene()
  mt, diam, V = sc['mt'], float(sc['diameter']), sc['mesh'].vertices
  K, truth, near, far = P.mesh_case()
  depth = P.millimetres(render(K=K, H=120, W=160, ob_in_cams=truth[None].astype(np.float32), mesh_tensors=mt)[1][0].numpy())
  n4 = P.D.normals(depth, K, (depth > 0).astype(np.uint8))

  def maps(p):
    tf = G.compute_crop_window_tf_batch(p[None], K, 1.2, (P.MESH_CROP, P.MESH_CROP), diam)
    ex = {}
    nm = render(K=K, H=120, W=160, ob_in_cams=p[None], mesh_tensors=mt, get_normal=True, bbox2d=G.crop_bbox2d_ori(tf, (P.MESH_CROP, P.MESH_CROP)),
                output_size=(P.MESH_CROP, P.MESH_CROP), extra=ex)[2]
    return ex['xyz_map'][0].numpy(), nm[0].numpy()
  for name, given in (('near', near.astype(np.float32)), ('far', far.astype(np.float32))):
    got, st, _ = P.polish(maps, given, depth, n4, K, exact_sums=True)
    before = np.array([P.add_error(g, truth, V) for g in given]) * 1e3
    after = np.array([P.add_error(g, truth, V) for g in got]) * 1e3
    print(f'{name}: ADD mm before {np.round(before, 2)} after {np.round(after, 2)} ratio {after.mean() / before.mean():.4f} '
          f'stopped {[P.STOP[s["stopped"]] for s in st]} valid {[int(s["fit_count"]) for s in st]}')
    assert (after < before).all() and abs(after.mean() / before.mean() - P.RECORDED_MESH_RATIO[name]) < 2e-3


@pytest.fixture(scope='module')
def built():
  import __graft_entry__ as g
  g.build()
  from foundationpose_amd import _lib
  return _lib


def test_state_record_matches_the_header(built):
  assert built.POSE_STATE_DTYPE.itemsize == 136 and built.FP_POSE_ALIGN_TERMS == 29 and built.FP_POSE_ALIGN_MAX_POSES == 1024
  assert built.FP_POSE_STOP_REASONS == {k: v for k, v in P.STOP.items() if k}


def test_argument_checks_need_no_gpu(built):
  L, EINVAL = built.lib(), built.FP_EINVAL
  dbl = lambda *a: (ctypes.c_double * len(a))(*a)
  K = dbl(100, 0, 4, 0, 100, 4, 0, 0, 1)
  fake = ctypes.c_void_p(64)                     # never dereferenced: the null and range checks come first
  bad_K = (dbl(0, 0, 4, 0, 100, 4, 0, 0, 1), dbl(100, 0, 4, 0, -1, 4, 0, 0, 1), dbl(100, 0, float('nan'), 0, 100, 4, 0, 0, 1),
           dbl(float('inf'), 0, 4, 0, 100, 4, 0, 0, 1))
  nan = float('nan')

  # fp_pose_depth_align
  def align(ctx=fake, xyz=fake, nm=fake, n=1, h=8, w=8, depth=fake, nrm=fake, Hh=8, Ww=8, Kk=K, poses=fake, dist=0.01, cos=0.5, rows=None, sums=fake,
            counts=None, out=None):
    return L.fp_pose_depth_align(ctx, xyz, nm, n, h, w, depth, nrm, Hh, Ww, Kk, poses, dist, cos, rows, sums, counts, out, None)
  for kw in (dict(ctx=None), dict(xyz=None), dict(nm=None), dict(depth=None), dict(nrm=None), dict(Kk=None), dict(poses=None), dict(sums=None)):
    assert align(**kw) == EINVAL and b'null' in L.fp_last_error(), kw
  for kw in [dict(n=-1), dict(n=built.FP_POSE_ALIGN_MAX_POSES + 1), dict(h=0), dict(w=-1), dict(Hh=0), dict(Ww=0), dict(dist=0.0), dict(dist=nan),
             dict(dist=-1.0), dict(cos=1.5), dict(cos=-1.01), dict(cos=nan), dict(h=1 << 13, w=(1 << 11) + 1)] + [dict(Kk=k) for k in bad_K]:
    assert align(**kw) == EINVAL, kw
  assert align(nrm=ctypes.c_void_p(72)) == EINVAL and b'aligned' in L.fp_last_error()
  assert align(rows=ctypes.c_void_p(68)) == EINVAL and b'aligned' in L.fp_last_error()
  assert align(n=0) == 0                         # nothing to do: returns before anything is touched

  # fp_pose_gn_step
  def step(ctx=fake, sums=fake, poses=fake, state=fake, n=1, damping=1e-9, min_pixels=100, closing=0):
    return L.fp_pose_gn_step(ctx, sums, poses, state, n, damping, min_pixels, closing, None)
  for kw in (dict(ctx=None), dict(sums=None), dict(poses=None), dict(state=None)):
    assert step(**kw) == EINVAL and b'null' in L.fp_last_error(), kw
  for kw in (dict(n=-1), dict(n=built.FP_POSE_ALIGN_MAX_POSES + 1), dict(damping=-1e-9), dict(damping=nan), dict(damping=float('inf')),
             dict(min_pixels=0)):
    assert step(**kw) == EINVAL, kw
  assert step(state=ctypes.c_void_p(68)) == EINVAL and b'aligned' in L.fp_last_error()
  assert step(n=0) == 0

  # fp_pose_polish
  def polish(ctx=fake, mesh=fake, poses=fake, n=1, Kk=K, Hh=8, Ww=8, depth=fake, nrm=fake, crop=16, ratio=1.2, diam=0.1, it=4, dist=0.01, cos=0.5,
             damping=1e-9, min_pixels=100, state=fake, sums=fake, counts=None):
    return L.fp_pose_polish(ctx, mesh, poses, n, Kk, Hh, Ww, depth, nrm, crop, ratio, diam, it, dist, cos, damping, min_pixels, state, sums, counts, None)
  for kw in (dict(ctx=None), dict(mesh=None), dict(poses=None), dict(Kk=None), dict(depth=None), dict(nrm=None), dict(state=None), dict(sums=None)):
    assert polish(**kw) == EINVAL and b'null' in L.fp_last_error(), kw
  for kw in [dict(n=-1), dict(n=built.FP_POSE_ALIGN_MAX_POSES + 1), dict(Hh=0), dict(Ww=0), dict(crop=-1), dict(ratio=0.0), dict(ratio=nan),
             dict(diam=0.0), dict(diam=float('inf')), dict(it=-1), dict(it=built.FP_POSE_POLISH_MAX_ITERATIONS + 1), dict(dist=0.0), dict(cos=2.0),
             dict(damping=-1.0), dict(min_pixels=0)] + [dict(Kk=k) for k in bad_K]:
    assert polish(**kw) == EINVAL, kw
  assert polish(nrm=ctypes.c_void_p(72)) == EINVAL and b'aligned' in L.fp_last_error()
  assert polish(state=ctypes.c_void_p(68)) == EINVAL and b'aligned' in L.fp_last_error()
  assert polish(n=0) == 0 and polish(n=0, crop=0) == 0
