"""CPU: the numpy restatement of the photometric term of pairwise depth ICP (tests/photo_icp_oracle.py) against finite differences, against
its own records and against analytic truth - a textured sphere, whose depth maps leave every rotation about its centre free, and the
textured orbit of the three spheres -, the weighting of foundationpose_amd/reconstruct.py, and the argument checks of fp_view_intensity
and fp_depth_pairs_align_photo that need no GPU.  The GPU tests (tests/test_gpu_photo_icp.py) hold the kernels to this restatement bit
for bit, so what is shown here about the rules holds for them."""
import ctypes

import numpy as np
import pytest

from tests import depth_icp_oracle as D
from tests import photo_icp_oracle as P
from tests import tsdf_align_oracle as A


@pytest.fixture(scope='module')
def row_case():
  K, truth, depths, masks, query, pairs, rgbs = P.row_case()
  nrm = [D.normals(depths[v], K, masks[v]) for v in range(len(depths))]
  inten = P.row_intensity(depths, masks, rgbs, K)
  out = [P.pair_rows(depths, nrm, inten, K, query, s, t, *D.ROW_GATE, P.ROW_I_MAX, reasons=True) for s, t in pairs]
  return dict(K=K, truth=truth, depths=depths, masks=masks, query=query, pairs=pairs, rgbs=rgbs, nrm=nrm, inten=inten, rows=[o[0] for o in out],
              why=[o[1] for o in out])


def test_every_new_skip_reason_occurs_in_the_row_case(row_case):
  """A condition on the case the GPU rows are compared on.  An intensity record made from the alignment's own normals is there wherever
  a geometric row is valid, so the row case takes its intensity maps from normals of a tighter max_jump (2 mm against 10 mm): then
  pixels with a normal and without a record exist in the source and in the target.  i_max = 0.05 skips pixels too, and most pairs keep
  60 or more photometric rows.  The geometric half of every row is the geometric restatement's."""
  total = {k: sum(int(w[k].sum()) for w in row_case['why']) for k in P.SKIPS}
  valid = [int(r[..., 15].sum()) for r in row_case['rows']]
  geo = [int(r[..., 7].sum()) for r in row_case['rows']]
  print(f'skipped {total}; photometric rows per pair {valid}; geometric {geo}')
  assert all(total[k] > 0 for k in P.SKIPS), total
  assert sum(v >= 60 for v in valid) >= 10 and sum(v == 0 for v in valid) >= 1
  assert all(v <= g for v, g in zip(valid, geo))
  for (s, t), rw in zip(row_case['pairs'], row_case['rows']):
    assert np.array_equal(rw[..., :8], D.pair_rows(row_case['depths'], row_case['nrm'], row_case['K'], row_case['query'], s, t, *D.ROW_GATE))
    assert (rw[..., 8:][rw[..., 15] == 0] == 0).all()
  for v in range(6):
    rec, n4 = row_case['inten'][v], row_case['nrm'][v]
    assert 100 < rec[..., 3].sum() < n4[..., 3].sum() and (rec[n4[..., 3] == 0] == 0).all()


def test_intensity_map_is_the_grey_value_and_its_central_differences(row_case):
  """against float64 on an image of three different channels: the weights, the order of the channels and the two directions"""
  rs = np.random.RandomState(3)
  rgb = rs.randint(0, 256, size=(48, 64, 3)).astype(np.uint8)
  n4 = row_case['nrm'][0]
  got = P.intensity(rgb, n4)
  I = (0.299 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2]) / 255.0
  rr, cc = np.nonzero(n4[..., 3])
  assert len(rr) > 400 and (got[..., 3] == (n4[..., 3] != 0)).all()
  assert np.abs(got[rr, cc, 0] - I[rr, cc]).max() < 3e-7
  assert np.abs(got[rr, cc, 1] - (I[rr, cc + 1] - I[rr, cc - 1]) / 2).max() < 3e-7
  assert np.abs(got[rr, cc, 2] - (I[rr + 1, cc] - I[rr - 1, cc]) / 2).max() < 3e-7
  assert (got[n4[..., 3] == 0] == 0).all()
  edge = np.ones_like(n4)                                # a map that claims normals on the border: the border stays empty
  assert P.intensity(rgb, edge)[..., 3].sum() == 46 * 62


def test_analytic_jacobian_is_the_derivative_of_the_photometric_residual(row_case):
  """J of a pixel against the central difference of the float64 residual at FIXED association and FIXED intensity records under
  exp(eps e_k) applied to view s, and -J under the same twist applied to view t.  eps = 1e-6.
  Tolerance, per pixel: 1e-5 |a| + 1e-9, |a| the length of J's translation part (the image gradient carried into the object frame;
  up to 20 per metre here: a gradient of 0.05 per pixel x fx / y.z = 130 / 0.4).  Relative part: J is fp32 - the poses are cast to fp32
  (6e-8 relative), y carries up to 4 roundings of 2^-24 x 0.5 m against y.z = 0.4 m (1.5e-7), jx, jy and jz carry 2 to 5 roundings of
  2^-24 (3e-7), the rotation 3 more and the cross product 2 with |x| < 0.5: below 1e-6 |a| in all, so 1e-5 leaves a factor of ten.
  Absolute part: the difference quotient's own round-off is 1e-16 x |r terms| (1) / 2e-6 = 5e-11, and its truncation eps^2 / 6 x the
  third derivative of u along y.z, 6 fx / y.z^4 x gradient = 1.5e3, is 2.5e-10.  A wrong sign, axis or frame is an error of order |a|."""
  K, depths, query = row_case['K'], row_case['depths'], row_case['query']
  k = row_case['pairs'].index((0, 1))
  rw, why = row_case['rows'][k], row_case['why'][k]
  pix = np.argwhere(rw[..., 15] > 0)
  assert len(pix) >= 60
  tp = why['assoc'][pix[:, 0], pix[:, 1]]
  a4, b4 = row_case['inten'][0][pix[:, 0], pix[:, 1]], row_case['inten'][1][tp[:, 0], tp[:, 1]]
  r0 = P.residual64(depths, K, query, 0, 1, pix, tp, a4, b4)
  assert np.abs(r0 - rw[pix[:, 0], pix[:, 1], 14]).max() < 1e-5
  J = rw[pix[:, 0], pix[:, 1], 8:14].astype(np.float64)
  tol = 1e-5 * np.linalg.norm(J[:, :3], axis=1) + 1e-9
  assert np.linalg.norm(J[:, :3], axis=1).max() > 1.0
  worst = {0: 0.0, 1: 0.0}
  for view, sign in ((0, 1.0), (1, -1.0)):
    for a in range(6):
      eps = 1e-6 * np.eye(6)[a]
      moved = lambda e: [A.expm_se3(e) @ q if v == view else q for v, q in enumerate(query)]
      fd = (P.residual64(depths, K, moved(eps), 0, 1, pix, tp, a4, b4) - P.residual64(depths, K, moved(-eps), 0, 1, pix, tp, a4, b4)) / 2e-6
      worst[view] = max(worst[view], (np.abs(fd - sign * J[:, a]) / tol).max())
  print(f'{len(pix)} pixels, |a| up to {np.linalg.norm(J[:, :3], axis=1).max():.2f}: max |J - d r / d xi_s| / tolerance {worst[0]:.3e}, '
        f'max |-J - d r / d xi_t| / tolerance {worst[1]:.3e}')
  assert worst[0] < 1 and worst[1] < 1


def test_textured_sphere_reproduces_its_record():
  """joint_refine of the restatement (fp32 rules, DEFAULT_STAGES, weight 0.03, i_max 0.2) on sphere_case(): 8 views of one textured
  sphere, views 1 .. 7 off by 4 mm / 1.5 degrees.  Mean displacement of views 1 .. 7 from 4.06 mm to 0.048 mm (largest 0.068 mm,
  largest rotation error 0.048 degrees) - the figures of the issue's float64 experiment.  Cap: 0.5 mm."""
  K, truth, depths, masks, given, rgbs = P.sphere_case()
  got, info = P.joint_refine(depths, masks, rgbs, K, given)
  disp = np.array([A.displacement(got[v], truth[v]) for v in range(8)]) * 1e3
  rot = np.array([P.rotation_deg(got[v], truth[v]) for v in range(8)])
  print(f'displacement {np.round(disp, 3)} mean {disp[1:].mean():.3f} mm; rotation {np.round(rot, 3)} degrees; photometric rms '
        f'{info["photo_rms"][0]:.4f} -> {info["photo_rms"][-1]:.4f} over {info["photo_valid"][-1]:.0f} pixels')
  assert np.array_equal(got[0], given[0]) and info['stopped'] == {}
  assert disp[1:].mean() <= 0.5
  assert abs(disp[1:].mean() - P.RECORDED_SPHERE_PHOTO[0]) < 1e-3 and abs(disp.max() - P.RECORDED_SPHERE_PHOTO[1]) < 1e-3
  assert abs(rot.max() - P.RECORDED_SPHERE_PHOTO[2]) < 1e-3
  assert len(info['photo_rms']) == 21 and info['photo_rms'][-1] < 0.1 * info['photo_rms'][0]


def test_sphere_without_the_term_drifts():
  """The same input with weight 0 - the geometric procedure, which is checked: the poses are depth_icp_oracle.joint_refine's bit for bit.
  The translation is recovered and the rotation drifts: every one of views 1 .. 7 ends with a rotation error above the 1.5 degrees it
  started with (2.78 degrees at the least, 17.5 at the most), mean displacement 6.09 mm from 4.06 mm.  The system's condition number
  is 5e6 (eigenvalue ratios of 3e-7 per view), so this drift is data, not round-off."""
  K, truth, depths, masks, given, rgbs = P.sphere_case()
  got, info = P.joint_refine(depths, masks, rgbs, K, given, weight=0.0)
  assert np.array_equal(got, D.joint_refine(depths, masks, K, given)[0])
  disp = np.array([A.displacement(got[v], truth[v]) for v in range(8)]) * 1e3
  rot = np.array([P.rotation_deg(got[v], truth[v]) for v in range(8)])
  start = np.array([P.rotation_deg(given[v], truth[v]) for v in range(8)])
  print(f'displacement {np.round(disp, 3)} mean {disp[1:].mean():.3f} mm; rotation {np.round(rot, 3)} degrees from {np.round(start, 3)}')
  assert np.abs(start[1:] - 1.5).max() < 1e-6
  assert (rot[1:] > 1.5).all()
  assert abs(rot[1:].min() - P.RECORDED_SPHERE_GEOMETRY_MIN_ROTATION_DEG) < 1e-2
  assert abs(disp[1:].mean() - P.RECORDED_SPHERE_GEOMETRY[0]) < 1e-2 and abs(rot.max() - P.RECORDED_SPHERE_GEOMETRY[2]) < 1e-2
  assert np.nanmax(info['eig_ratio']) < 1e-6


def test_textured_orbit_reproduces_its_record():
  """estimate of the restatement on orbit_case() with the texture, first_pose = truth[0], weight 0.03: the odometry holds every frame
  (mean 0.086 mm, largest 0.124 mm) and the joint pass ends at mean 0.052 mm (largest 0.080 mm), where the geometric procedure loses
  16 mm at frame 5 and ends at 24.654 mm (tests/test_depth_icp_host.py).  Cap: 1 mm."""
  K, truth, depths, masks, rgbs = P.orbit_case()
  got, info = P.estimate(depths, masks, rgbs, K, first_pose=truth[0])
  odo = np.array([A.displacement(info['odometry'][v], truth[v]) for v in range(24)]) * 1e3
  fin = np.array([A.displacement(got[v], truth[v]) for v in range(24)]) * 1e3
  print(f'odometry {np.round(odo, 3)} mean {odo[1:].mean():.3f}; final {np.round(fin, 3)} mean {fin[1:].mean():.3f}')
  assert fin[1:].mean() <= 1.0
  assert abs(odo[1:].mean() - P.RECORDED_ORBIT_PHOTO_ODOMETRY_MM[0]) < 1e-3 and abs(odo.max() - P.RECORDED_ORBIT_PHOTO_ODOMETRY_MM[1]) < 1e-3
  assert abs(fin[1:].mean() - P.RECORDED_ORBIT_PHOTO_FINAL_MM[0]) < 1e-3 and abs(fin.max() - P.RECORDED_ORBIT_PHOTO_FINAL_MM[1]) < 1e-3
  assert P.RECORDED_ORBIT_PHOTO_FINAL_MM[0] < 0.01 * D.RECORDED_ORBIT_FINAL_MM[0]
  assert np.array_equal(got[0], truth[0])


@pytest.fixture(scope='module')
def built():
  import __graft_entry__ as g
  g.build()
  from foundationpose_amd import _lib
  return _lib


def test_combine_sums_and_constants(built):
  from foundationpose_amd import reconstruct as R
  rs = np.random.RandomState(5)
  sm = rs.randn(7, 58)
  sm[:, 28], sm[:, 57] = rs.randint(0, 900, 7), rs.randint(0, 900, 7)
  zero = R.combine_sums(sm, 0.0)
  assert zero.shape == (7, 29) and np.array_equal(zero.view(np.uint64), np.ascontiguousarray(sm[:, :29]).view(np.uint64))      # bit for bit
  got = R.combine_sums(sm, 0.03)
  assert np.array_equal(got, P.combine(sm, 0.03)) and np.array_equal(got[:, 28], sm[:, 28])
  assert np.allclose(got[:, :28], sm[:, :28] + 9e-4 * sm[:, 29:57], rtol=1e-14, atol=0)
  assert R.combine_sums(np.zeros((0, 58)), 0.03).shape == (0, 29)
  assert R.PHOTO_WEIGHT == P.PHOTO_WEIGHT == 0.03 and R.I_MAX == P.I_MAX == 0.2
  assert R.DEFAULT_STAGES == D.DEFAULT_STAGES and R.ODOMETRY_STAGES == D.ODOMETRY_STAGES and R.ESTIMATE_JOINT_STAGES == D.ESTIMATE_JOINT_STAGES
  assert R._photo_weight(False) is None and R._photo_weight(None) is None and R._photo_weight(True) == 0.03 and R._photo_weight(0.1) == 0.1
  for bad in (0.0, -1.0, float('nan'), float('inf')):
    with pytest.raises(ValueError):
      R._photo_weight(bad)


def test_argument_checks_need_no_gpu(built):
  L, EINVAL = built.lib(), built.FP_EINVAL
  dbl = lambda *a: (ctypes.c_double * len(a))(*a)
  K = dbl(100, 0, 4, 0, 100, 4, 0, 0, 1)
  fake = ctypes.c_void_p(64)                     # never dereferenced: the null and range checks come first
  # fp_view_intensity
  call = lambda ctx=fake, rgb=fake, nrm=fake, n=1, Hh=8, Ww=8, out=fake: L.fp_view_intensity(ctx, rgb, nrm, n, Hh, Ww, out, None)
  for kw in (dict(ctx=None), dict(rgb=None), dict(nrm=None), dict(out=None)):
    assert call(**kw) == EINVAL and b'null' in L.fp_last_error(), kw
  for kw in (dict(n=-1), dict(n=built.FP_TSDF_MAX_VIEWS + 1), dict(Hh=0), dict(Ww=0), dict(Ww=-3)):
    assert call(**kw) == EINVAL, kw
  assert call(out=ctypes.c_void_p(68)) == EINVAL and b'aligned' in L.fp_last_error()
  assert call(nrm=ctypes.c_void_p(72)) == EINVAL and b'aligned' in L.fp_last_error()
  assert call(n=0) == 0 and call(n=0, rgb=ctypes.c_void_p(3)) == 0      # nothing to do: returns before anything is touched; rgb is bytes, any address
  # fp_depth_pairs_align_photo
  poses = np.ascontiguousarray(np.stack([np.eye(4)] * 3))
  pp = lambda a: ctypes.c_void_p(a.ctypes.data)
  pr = np.array([[0, 1], [2, 0]], dtype=np.int32)
  sums = np.zeros((2, 58))

  def call2(ctx=fake, depth=fake, nrm=fake, inten=fake, n=3, Hh=8, Ww=8, Kk=K, p=poses, pairs=pr, P=2, dist=0.01, cos=0.5, imax=0.2, rows=None, out=sums):
    return L.fp_depth_pairs_align_photo(ctx, depth, nrm, inten, n, Hh, Ww, Kk, None if p is None else pp(p), None if pairs is None else pp(pairs), P,
                                        dist, cos, imax, rows, None if out is None else pp(out), None)
  for kw in (dict(ctx=None), dict(depth=None), dict(nrm=None), dict(inten=None), dict(Kk=None), dict(p=None), dict(out=None), dict(pairs=None)):
    assert call2(**kw) == EINVAL and b'null' in L.fp_last_error(), kw
  assert b'fp_depth_pairs_align_photo' in L.fp_last_error()
  for kw in (dict(n=-1), dict(n=built.FP_TSDF_MAX_VIEWS + 1), dict(P=-1), dict(P=built.FP_DEPTH_ALIGN_MAX_PAIRS + 1), dict(Hh=0), dict(Ww=-2),
             dict(dist=0.0), dict(dist=float('nan')), dict(cos=1.5), dict(cos=-1.01), dict(cos=float('nan')),
             dict(imax=0.0), dict(imax=-0.1), dict(imax=float('nan')),
             dict(Kk=dbl(0, 0, 4, 0, 100, 4, 0, 0, 1)), dict(Kk=dbl(100, 0, 4, 0, float('nan'), 4, 0, 0, 1)),
             dict(pairs=np.array([[0, 3], [1, 0]], dtype=np.int32)), dict(pairs=np.array([[0, 1], [-1, 0]], dtype=np.int32)),
             dict(pairs=np.array([[0, 1], [2, 2]], dtype=np.int32)), dict(n=2)):
    assert call2(**kw) == EINVAL, kw
  assert call2(imax=0.0) == EINVAL and b'i_max' in L.fp_last_error()
  assert call2(pairs=np.array([[1, 1], [0, 1]], dtype=np.int32)) == EINVAL and b'itself' in L.fp_last_error()
  bad = poses.copy()
  bad[1, 3, 3] = 2
  assert call2(p=bad) == EINVAL and b'last row' in L.fp_last_error()
  bad = poses.copy()
  bad[2, 1, 2] = np.inf
  assert call2(p=bad) == EINVAL and b'finite' in L.fp_last_error()
  assert call2(nrm=ctypes.c_void_p(72)) == EINVAL and b'aligned' in L.fp_last_error()
  assert call2(inten=ctypes.c_void_p(72)) == EINVAL and b'd_intensity' in L.fp_last_error()
  assert call2(rows=ctypes.c_void_p(68)) == EINVAL and b'aligned' in L.fp_last_error()
  before = sums.copy()
  for imax in (0.2, float('inf')):                                                               # zero pairs: nothing is touched; +inf is a value
    assert call2(P=0, imax=imax) == 0 and call2(P=0, pairs=None, imax=imax) == 0 and np.array_equal(sums, before)
  assert built.FP_PHOTO_ALIGN_TERMS == 58 and built.FP_PHOTO_ALIGN_TERMS == 2 * built.FP_DEPTH_ALIGN_TERMS
  # the geometric entry point names itself as before and does not ask for an intensity map
  assert L.fp_depth_pairs_align(fake, fake, fake, 3, 8, 8, K, pp(poses), pp(pr), 2, 0.0, 0.5, None, pp(sums), None) == EINVAL
  assert L.fp_last_error().startswith(b'fp_depth_pairs_align: dist_max')
