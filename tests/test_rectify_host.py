"""CPU: raw stereo pairs and distorted cameras - the float64 camera model and rectification rule of foundationpose_amd/rectify.py, the
numpy restatement tests/rectify_oracle.py pinned against them and against hand-made cases, the calibration-file reader, the pipeline
stages with a stubbed kernel call, the refusals of fp_remap that need no GPU, and the figures of the end-to-end scene that the GPU test
asserts as well."""
import ctypes

import numpy as np
import pytest

from foundationpose_amd import Utils as U
from foundationpose_amd import mesh_io, rectify
from tests import rectify_oracle as O


def product_plan(a):
  return rectify.RemapPlan(*a)


def assert_plan_equals_oracle(p, o):
  for k in ('k_new', 'rot', 'k_raw', 'dist'):
    assert getattr(p, k).dtype == np.float32 and (getattr(p, k).view(np.uint32) == o[k].view(np.uint32)).all(), k
  assert np.float32(p.r2_max) == o['r2_max'] and p.src_size == o['src'] and p.dst_size == o['dst']


def scene_calibration():
  Q, c2 = O.rodrigues(np.deg2rad(3.0) * np.array([0.6, -0.64, 0.48])), np.array([0.12, 0.004, -0.003])
  K1 = np.array([[500.0, 0, 320.5], [0, 503.0, 239.0], [0, 0, 1]])
  K2 = np.array([[497.0, 0, 318.0], [0, 499.0, 243.5], [0, 0, 1]])
  return K1, K2, Q.T, -Q.T @ c2, c2


def test_rectification_makes_rows_equal_and_disparity_metric():
  """R1, R2 are rotations; a 3-D point seen through (K_new, R1) and through (K_new, R2 after R, T) lands in the same row to float64
  round-off, and the columns differ by f baseline / z_rect."""
  K1, K2, R, T, c2 = scene_calibration()
  rect = U.rectify_stereo(K1, [], K2, [], R, T, (480, 640))
  for Rr in (rect.R1, rect.R2):
    assert np.abs(Rr @ Rr.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Rr) - 1) < 1e-14
  assert rect.baseline == pytest.approx(np.linalg.norm(c2), rel=1e-15) and rect.size_new == (480, 640)
  f = rect.K_new[0, 0]
  assert f == rect.K_new[1, 1] == (503.0 + 499.0) / 2 and rect.K_new[0, 2] == (320.5 + 318.0) / 2 and rect.K_new[1, 2] == (239.0 + 243.5) / 2
  X1 = np.random.default_rng(0).uniform([-1, -1, 0.5], [1, 1, 4], (1000, 3))
  a = (rect.R1 @ X1.T).T
  b = (rect.R2 @ (R @ X1.T + T[:, None])).T
  pa, pb = (rect.K_new @ (a / a[:, 2:]).T).T, (rect.K_new @ (b / b[:, 2:]).T).T
  assert np.abs(a[:, 2] - b[:, 2]).max() < 1e-13      # one z_rect for both cameras
  assert np.abs(pa[:, 1] - pb[:, 1]).max() < 1e-10
  assert np.abs((pa[:, 0] - pb[:, 0]) - f * rect.baseline / a[:, 2]).max() < 1e-10
  # the oracle's restatement gives the same record and the same plans
  o = O.rectify_stereo(K1, [], K2, [], R, T, (480, 640))
  assert np.abs(o['R1'] - rect.R1).max() < 1e-15 and np.abs(o['R2'] - rect.R2).max() < 1e-15 and o['baseline'] == pytest.approx(rect.baseline, rel=1e-15)
  assert_plan_equals_oracle(rect.left, o['left'])
  assert_plan_equals_oracle(rect.right, o['right'])
  assert np.abs(rect.left.rotation - rect.R1.T).max() == 0 and np.abs(rect.right.rotation - rect.R2.T).max() == 0


def test_every_test_plan_equals_the_oracle_plan():
  for src, dst in O.SIZES:
    args, plans = O.case_arguments(src, dst), O.case_plans(src, dst)
    for name in ('mild', 'barrel', 'rational'):
      assert_plan_equals_oracle(product_plan(args[name]), plans[name])
    rect = U.rectify_stereo(*args['rectification'])
    assert_plan_equals_oracle(rect.left, plans['rect_left'])
    assert_plan_equals_oracle(rect.right, plans['rect_right'])
  p = U.undistort_plan(np.diag([100.0, 100.0, 1.0]), [0.1, 0, 0, 0], (5, 7))
  assert (p.rot == np.eye(3, dtype=np.float32).reshape(9)).all() and (p.k_new == p.k_raw).all() and p.dst_size == (5, 7)
  assert (p.dist == np.array([0.1, 0, 0, 0, 0, 0, 0, 0], np.float32)).all()


def test_distort_then_undistort_returns_the_ray():
  K = np.array([[500.0, 0, 320], [0, 510.0, 240], [0, 0, 1]])
  xy = np.random.default_rng(1).uniform(-0.6, 0.6, (500, 2))
  for dist in ([], [-0.2, 0.05, 1e-3, -2e-3], [-0.2, 0.05, 1e-3, -2e-3, 0.01], [0.1, -0.02, 2e-4, 1e-4, 0.003, 0.05, -0.01, 0.002]):
    uv = U.distort_points(xy, K, dist)
    assert np.abs(U.undistort_points(uv, K, dist) - xy).max() < 1e-12, dist
    assert np.abs(O.distort64(xy, K, dist) - uv).max() < 1e-10      # the oracle's model is the same one
    assert np.abs(O.undistort64(uv, K, dist) - xy).max() < 1e-12
  assert np.abs(U.distort_points(xy, K, []) - (xy * [500.0, 510.0] + [320, 240])).max() < 1e-12
  # by hand: x = 0.5, y = 0: r2 = 0.25, radial = 1 - 0.05 = 0.95, tangential p2 (r2 + 2 x^2) = 0.01 * 0.75
  assert U.distort_points([[0.5, 0.0]], np.eye(3), [-0.2, 0, 0, 0.01])[0].tolist() == pytest.approx([0.5 * 0.95 + 0.0075, 0.0], abs=1e-15)


def test_map_equals_float64_distortion_of_the_rotated_ray():
  """The oracle's fp32 map against distort_points of the rotated ray in float64, over every test plan.  Measured here: the largest
  difference over the test plans is 3.55e-5 px (at 64 x 200; 4.8e-4 px at 1920 x 1200, where the coordinates are ten times larger);
  allowed: 4 x 3.55e-5 = 1.42e-4 px, far below the 1/512 px at which a bilinear weight changes."""
  worst = 0.0
  for src, dst in O.SIZES:
    args, plans = O.case_arguments(src, dst), O.case_plans(src, dst)
    rect = U.rectify_stereo(*args['rectification'])
    product = dict(rect_left=rect.left, rect_right=rect.right, **{k: product_plan(args[k]) for k in ('mild', 'barrel', 'rational')})
    for name, o in plans.items():
      u, v, Z, ray = O.pixel_map(o)
      p = product[name]
      Hd, Wd = p.dst_size
      row, col = np.meshgrid(np.arange(Hd, dtype=np.float64), np.arange(Wd, dtype=np.float64), indexing='ij')
      d = np.stack([(col - p.K_new[0, 2]) / p.K_new[0, 0], (row - p.K_new[1, 2]) / p.K_new[1, 1], np.ones_like(col)], -1) @ p.rotation.T
      want = U.distort_points(d[..., :2] / d[..., 2:], p.K_raw, o['dist64'])
      assert ray.any() and (d[..., 2][ray] > 0).all()
      worst = max(worst, np.abs(u[ray] - want[..., 0][ray]).max(), np.abs(v[ray] - want[..., 1][ray]).max())
      assert np.isnan(u[~ray]).all() and np.isnan(v[~ray]).all()
  print(f'largest |fp32 map - float64 map| over the test plans: {worst:.3e} px')
  assert worst <= 4 * 3.55e-5


def test_monotonic_r2_max():
  assert U.monotonic_r2_max([-0.4, 0, 0, 0]) == pytest.approx(1 / 1.2, rel=1e-12)      # 1 + 3 k1 r2 = 0
  assert U.monotonic_r2_max([]) == np.inf and U.monotonic_r2_max([0, 0, 0, 0, 0]) == np.inf
  assert U.monotonic_r2_max([0, 0, 0.01, -0.02]) == np.inf      # tangential terms alone do not fold
  assert U.monotonic_r2_max([0.1, 0.01, 0, 0, 0.001]) == np.inf      # a pincushion never folds
  # 1 + 3 k1 s + 5 k2 s^2 = 0 with k1 = -0.3, k2 = 0.05: s = (0.9 - sqrt(0.81 - 1)) / 0.5 has no real root -> the slope stays positive
  assert U.monotonic_r2_max([-0.3, 0.05, 0, 0]) == np.inf
  s = U.monotonic_r2_max([-0.3, 0.02, 0, 0])      # 0.1 s^2 - 0.9 s + 1 = 0: s = (0.9 - sqrt(0.41)) / 0.2
  assert s == pytest.approx((0.9 - np.sqrt(0.41)) / 0.2, rel=1e-12)
  assert U.monotonic_r2_max([0, 0, 0, 0, 0, -1.0, 0, 0]) <= 1.0      # the rational denominator reaches 0 at r2 = 1
  for dist in ([-0.4, 0, 0, 0], [-0.3, 0.02, 0, 0], [0.1, -0.02, 0, 0, 0.003, 0.05, -0.01, 0.002]):
    assert O.r2_max(dist) == pytest.approx(U.monotonic_r2_max(dist), rel=1e-12)
  # beyond the bound the barrel folds: the image radius grows up to it and falls behind it
  g = lambda r: U.distort_points([[r, 0.0]], np.eye(3), [-0.4, 0, 0, 0])[0, 0]
  top = np.sqrt(1 / 1.2)
  assert g(top - 0.05) < g(top - 0.01) < g(top) > g(top + 0.01) > g(top + 0.05)


def test_identity_and_integer_shift_in_the_oracle():
  """With the 1/256 rule an identity plan reproduces its input on every pixel, and an integer principal-point offset is an integer shift."""
  img = np.random.default_rng(2).integers(0, 256, (37, 53, 3)).astype(np.uint8)
  K = np.array([[47.7, 0, 26.2], [0, 48.6, 18.9], [0, 0, 1]])
  out = O.remap_colour(img, O.undistort_plan(K, [], (37, 53)))
  assert (out['out'] == img).all() and out['valid'].all()
  Ks = K.copy()
  Ks[0, 2] += 5
  Ks[1, 2] -= 3      # new pixel (col, row) shows raw pixel (col - 5, row + 3)
  out = O.remap_colour(img, O.undistort_plan(K, [], (37, 53), K_new=Ks))
  assert (out['out'][:34, 5:] == img[3:, :48]).all() and out['valid'][:34, 5:].all()
  assert not out['valid'][34:].any() and not out['valid'][:, :5].any() and not out['out'][34:].any() and not out['out'][:, :5].any()


def test_blend_and_depth_rule_by_hand():
  img = np.array([[10, 20], [110, 220]], np.uint8)
  K = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]])
  Kn = np.array([[1.0, 0, -0.25], [0, 1.0, -0.5], [0, 0, 1]])      # new pixel (0, 0) shows raw (0.25, 0.5)
  out = O.remap_colour(img, O.undistort_plan(K, [], (2, 2), K_new=Kn, size_new=(1, 2)))
  a, b = 64, 128
  want = ((256 - a) * (256 - b) * 10 + a * (256 - b) * 20 + (256 - a) * b * 110 + a * b * 220 + 32768) >> 16
  assert out['out'].tolist() == [[want, 0]] and out['valid'].tolist() == [[1, 0]] and want == 75      # 3.75 + 2.5 + 41.25 + 27.5
  depth = np.array([[1.0, 2.0], [np.nan, 0.0]], np.float32)
  d = O.remap_depth(depth, O.undistort_plan(K, [], (2, 2), K_new=Kn, size_new=(1, 2)))
  assert d['out'].tolist() == [[0.0, 0.0]] and d['valid'].tolist() == [[1, 1]]      # (0.25, 0.5), (1.25, 0.5) round to raw (0, 1), (1, 1): a NaN and a 0, no depth
  d = O.remap_depth(depth, O.undistort_plan(K, [], (2, 2)), zfar=1.5)
  assert d['out'].tolist() == [[1.0, 0.0], [0.0, 0.0]] and d['valid'].all()


SECTIONED = """
[LEFT_CAM_FHD1200]
fx=1067.51
fy=1067.9
cx=960.5
cy=600.25
k1=-0.0512
k2=0.021
p1=1.2e-05
k3=-0.004

[RIGHT_CAM_FHD1200]
fx=1066.1
fy=1066.3
cx=970.5
cy=590.75
k1=-0.049
p2=-3e-05

[LEFT_CAM_2K]
fx=1900.5
fy=1901.25
cx=1100
cy=620

[RIGHT_CAM_2K]
fx=1899
fy=1899.5
cx=1105
cy=615

[STEREO]
Baseline=119.905
TY=-0.0127
TZ=0.25
CV_2K=0.011
CV_FHD1200=0.012
RX_FHD1200=-0.001
RZ_FHD1200=0.0005
"""


def test_stereo_calibration_file(tmp_path):
  p = tmp_path / 'camera.conf'
  p.write_text(SECTIONED)
  c = mesh_io.load_stereo_calibration(str(p))
  assert sorted(c) == ['K1', 'K2', 'R', 'T', 'dist1', 'dist2']
  assert c['K1'].tolist() == [[1067.51, 0, 960.5], [0, 1067.9, 600.25], [0, 0, 1]] and c['K2'][0, 2] == 970.5
  assert c['dist1'].tolist() == [-0.0512, 0.021, 1.2e-05, 0.0, -0.004] and c['dist2'].tolist() == [-0.049, 0.0, 0.0, -3e-05, 0.0]
  Q = O.rodrigues([-0.001, 0.012, 0.0005])
  centre = np.array([119.905, -0.0127, 0.25]) * 0.001
  assert np.abs(c['R'] - Q.T).max() < 1e-15 and np.abs(-c['R'].T @ c['T'] - centre).max() < 1e-15      # c2 = -R^T T is the stated centre
  rect = U.rectify_stereo(c['K1'], c['dist1'], c['K2'], c['dist2'], c['R'], c['T'], (1200, 1920))
  assert rect.baseline == pytest.approx(np.linalg.norm(centre), rel=1e-14)
  c2k = mesh_io.load_stereo_calibration(str(p), left_section='LEFT_CAM_2K', scale=1.0)      # absent RX / RZ and coefficients are 0
  assert np.abs(c2k['R'] - O.rodrigues([0, 0.011, 0]).T).max() < 1e-15 and not c2k['dist1'].any() and c2k['K2'][0, 0] == 1899
  assert np.abs(-c2k['R'].T @ c2k['T'] - [119.905, -0.0127, 0.25]).max() < 1e-12
  mixed = mesh_io.load_stereo_calibration(str(p), 'LEFT_CAM_FHD1200', right_section='RIGHT_CAM_2K')
  assert mixed['K2'][0, 0] == 1899
  with pytest.raises(ValueError, match='LEFT_CAM_VGA'):
    mesh_io.load_stereo_calibration(str(p), left_section='LEFT_CAM_VGA')
  with pytest.raises(ValueError, match='RIGHT_CAM_HD'):
    mesh_io.load_stereo_calibration(str(p), right_section='RIGHT_CAM_HD')
  with pytest.raises(ValueError, match='right_section'):
    mesh_io.load_stereo_calibration(str(p), left_section='CAM_A')
  (tmp_path / 'nobase.conf').write_text(SECTIONED.replace('Baseline=119.905\n', ''))
  with pytest.raises(ValueError, match='Baseline='):
    mesh_io.load_stereo_calibration(str(tmp_path / 'nobase.conf'))
  (tmp_path / 'cam_K.txt').write_text('500 0 320 0 500 240 0 0 1')
  with pytest.raises(ValueError, match='sectioned'):
    mesh_io.load_stereo_calibration(str(tmp_path / 'cam_K.txt'))
  assert 'ASSUMPTION' in mesh_io.load_stereo_calibration.__doc__
  # the readers that were there read the same file as before
  assert mesh_io.load_intrinsics(str(p))[0, 0] == 1067.51 and mesh_io.load_stereo_baseline(str(p)) == pytest.approx(0.119905, rel=1e-15)


def test_refusals_on_the_host():
  K1, K2, R, T, _ = scene_calibration()
  with pytest.raises(ValueError, match='right one'):
    U.rectify_stereo(K2, [], K1, [], R.T, -R.T @ T, (480, 640))      # the cameras swapped: c2.x < 0
  with pytest.raises(ValueError, match='right one'):
    U.rectify_stereo(K1, [], K2, [], np.eye(3), [0.0, -0.1, 0.0], (480, 640))      # c2.x = 0
  with pytest.raises(ValueError, match='not a rotation'):
    U.rectify_stereo(K1, [], K2, [], 1.1 * np.eye(3), T, (480, 640))
  for n in (1, 2, 3, 6, 7, 9, 12):
    with pytest.raises(ValueError, match='0, 4, 5 or 8'):
      U.undistort_plan(K1, np.zeros(n), (480, 640))
    with pytest.raises(ValueError, match='0, 4, 5 or 8'):
      U.distort_points([[0.0, 0.0]], K1, np.zeros(n))
  with pytest.raises(ValueError, match='finite'):
    U.undistort_plan(K1, [np.nan, 0, 0, 0], (480, 640))
  for size in ((480,), (0, 640), (480, 640, 3), (480, 1 << 15)):
    with pytest.raises(ValueError, match='H, W'):
      U.undistort_plan(K1, [], size)
  with pytest.raises(ValueError, match='3x3'):
    U.undistort_plan(np.eye(4), [], (480, 640))
  with pytest.raises(ValueError, match='positive'):
    U.undistort_plan(np.diag([0.0, 1.0, 1.0]), [], (480, 640))
  # mismatched sizes are refused before anything touches the device
  import torch
  plan = U.undistort_plan(K1, [], (480, 640))
  with pytest.raises(ValueError, match='does not fit a plan'):
    rectify.remap([torch.zeros((1, 48, 64), dtype=torch.uint8)], [plan])
  with pytest.raises(ValueError, match='differ in shape'):
    rectify.remap([torch.zeros((1, 480, 640), dtype=torch.uint8), torch.zeros((1, 480, 641), dtype=torch.uint8)], [plan, plan])
  with pytest.raises(ValueError, match='size_new'):
    rectify.remap([torch.zeros((1, 480, 640), dtype=torch.uint8)] * 2, [plan, U.undistort_plan(K1, [], (480, 640), size_new=(48, 64))])
  with pytest.raises(ValueError, match='uint8'):
    U.remap_image(np.zeros((480, 640), np.float32), plan, device='cpu')
  with pytest.raises(ValueError, match='float32'):
    U.remap_image(np.zeros((480, 640), np.uint8), plan, mode='depth', device='cpu')
  with pytest.raises(ValueError, match='required'):
    U.stereo_depth(np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8))


@pytest.fixture(scope='module')
def built():
  import __graft_entry__ as g
  g.build()
  from foundationpose_amd import _lib
  return _lib


def test_argument_checks_need_no_gpu(built):
  L = built.lib()
  fake = ctypes.c_void_p(64)      # never dereferenced: every check of a value comes first
  good = U.undistort_plan(np.array([[50.0, 0, 8], [0, 50.0, 6], [0, 0, 1]]), [-0.1, 0, 0, 0], (12, 16))

  def call(ctx=fake, src0=fake, src1=fake, n=2, opts=True, dst0=fake, dst1=fake, dbg_size=None, opts_size=None, plan1=None, **kw):
    o = built.FpRemapOpts(struct_size=ctypes.sizeof(built.FpRemapOpts), mode=built.FP_REMAP_COLOUR, channels=1, n_plans=2, zfar=float('inf'))
    o.plan[0], o.plan[1] = good.as_struct(), good.as_struct()
    for k, v in (plan1 or {}).items():
      if isinstance(v, tuple):
        getattr(o.plan[1], k)[v[0]] = v[1]
      else:
        setattr(o.plan[1], k, v)
    for k, v in kw.items():
      setattr(o, k, v)
    if opts_size is not None:
      o.struct_size = opts_size
    d = ctypes.byref(built.FpRemapDebug(struct_size=dbg_size)) if dbg_size is not None else None
    return L.fp_remap(ctx, src0, src1, n, ctypes.byref(o) if opts else None, dst0, dst1, None, None, d, None)

  bad = [dict(ctx=None), dict(src0=None), dict(dst0=None), dict(src1=None), dict(dst1=None), dict(opts=False), dict(opts_size=0),
         dict(opts_size=ctypes.sizeof(built.FpRemapOpts) - 4), dict(dbg_size=8), dict(mode=2), dict(mode=-1), dict(channels=2), dict(channels=0),
         dict(channels=3, mode=built.FP_REMAP_DEPTH), dict(n_plans=0), dict(n_plans=3), dict(n=0), dict(n=3), dict(n=-2),
         dict(plan1=dict(src_h=0)), dict(plan1=dict(dst_w=1 << 15)), dict(plan1=dict(src_w=17)), dict(plan1=dict(dst_h=13)),
         dict(plan1=dict(k_new=(0, float('nan')))), dict(plan1=dict(rot=(4, float('inf')))), dict(plan1=dict(dist=(7, float('nan')))),
         dict(plan1=dict(k_raw=(1, 0.0))), dict(plan1=dict(k_new=(0, -5.0))), dict(plan1=dict(r2_max=0.0)), dict(plan1=dict(r2_max=float('nan'))),
         dict(mode=built.FP_REMAP_DEPTH, zfar=0.0), dict(mode=built.FP_REMAP_DEPTH, zfar=float('nan'))]
  for kw in bad:
    assert call(**kw) == built.FP_EINVAL, kw
    assert L.fp_last_error()
  assert call(plan1=dict(src_w=17)) == built.FP_EINVAL and b'differ in size' in L.fp_last_error()
  assert call(n=3) == built.FP_EINVAL and b'multiple of n_plans' in L.fp_last_error()
  assert ctypes.sizeof(built.FpRemapPlan) == 30 * 4 and ctypes.sizeof(built.FpRemapOpts) == 8 + 16 + 2 * 120


def test_pipeline_stages_with_a_stubbed_kernel_call(monkeypatch):
  from foundationpose_amd.pipeline import Pipeline, PipelineData, StereoDepth, StereoRectify, Undistort
  K1, K2, R, T, _ = scene_calibration()
  rect = U.rectify_stereo(K1, [-0.1, 0, 0, 0], K2, [], R, T, (4, 6))
  calls = []

  def fake_rectify_pair(left, right, r, **kw):
    calls.append(('rectify_pair', r))
    return 'L:' + left, 'R:' + right

  def fake_undistort_frame(rgb, depth, plan, zfar=np.inf, **kw):
    calls.append(('undistort_frame', plan, zfar))
    return (None if rgb is None else 'U:' + rgb), (None if depth is None else 'U:' + depth)

  def fake_stereo_depth(left, right, K, baseline, **kw):
    calls.append(('stereo_depth', left, right, np.asarray(K).copy(), baseline, kw))
    return 'depth'

  monkeypatch.setattr(rectify, 'rectify_pair', fake_rectify_pair)
  monkeypatch.setattr(rectify, 'undistort_frame', fake_undistort_frame)
  from foundationpose_amd import stereo
  monkeypatch.setattr(stereo, 'stereo_depth', fake_stereo_depth)
  assert PipelineData().baseline is None
  data = Pipeline('raw stereo').add_processor(StereoRectify(rect)).add_processor(StereoDepth(max_disparity=64)).run(PipelineData(rgb='l', right='r'))
  assert not data.errors and data.rgb == 'L:l' and data.right == 'R:r' and data.depth == 'depth'
  assert (data.K == rect.K_new).all() and data.K is not rect.K_new and data.baseline == rect.baseline
  assert [c[0] for c in calls] == ['rectify_pair', 'stereo_depth'] and calls[0][1] is rect
  _, left, right, K, baseline, kw = calls[1]
  assert (left, right, baseline, kw) == ('L:l', 'R:r', rect.baseline, dict(max_disparity=64)) and (K == rect.K_new).all()
  # a frame that is no pair is left alone; a baseline given to StereoDepth wins; none at all is refused
  del calls[:]
  mono = PipelineData(rgb='l', K='K as it was')
  assert StereoRectify(rect).process(mono) is mono and mono.rgb == 'l' and mono.K == 'K as it was' and mono.baseline is None and not calls
  StereoDepth(0.5, K=np.eye(3)).process(PipelineData(rgb='l', right='r', baseline=0.1))
  assert calls[0][4] == 0.5
  with pytest.raises(ValueError, match='baseline'):
    StereoDepth(K=np.eye(3)).process(PipelineData(rgb='l', right='r'))
  # Undistort: whichever of rgb / depth is there, and K
  del calls[:]
  plan = U.undistort_plan(K1, [-0.1, 0.01, 0, 0], (4, 6))
  data = Undistort(plan, zfar=3.0).process(PipelineData(rgb='rgb', depth='d', K=K1))
  assert (data.rgb, data.depth) == ('U:rgb', 'U:d') and (data.K == plan.K_new).all() and calls == [('undistort_frame', plan, 3.0)]
  data = Undistort(plan).process(PipelineData(rgb='rgb'))
  assert data.rgb == 'U:rgb' and data.depth is None


def test_end_to_end_figures_of_the_analytic_scene():
  """The plane z = 0.8 + 0.1 x with a random-dot texture seen by two raw cameras (distorted, the right one rotated by 1.9 degrees and
  4 mm off in y), 48 x 176, 64 disparities, through rectify_oracle + stereo_oracle - bit-equal to the device path, so these are the
  device's numbers (tests/test_gpu_rectify.py asserts that).  Measured: with rectify= 0.9009 of the pixels with x >= 64 are valid and
  the median |disparity - f b / z_rect| over them is 0.139 px; the same raw pair without it: 0.432 valid, median error 16.0 px.
  Asserted with a margin: >= 0.85 and <= 0.20 px with; without, at most 0.60 valid and an error of at least 2 px (ten times the bound
  of the rectified run)."""
  e = O.end_to_end(O.raw_plane_scene())
  print({k: round(e[k], 4) for k in ('valid_share', 'median_error', 'raw_valid_share', 'raw_median_error')})
  assert e['valid_share'] >= 0.85 and e['median_error'] <= 0.20
  assert e['raw_valid_share'] <= 0.60 and e['raw_median_error'] >= 2.0
