"""CPU: the numpy restatement of the masks-from-depth rules (tests/segment_oracle.py) against things independent of it, the host-side
assignment rule, load_reference_views(masks=False), and the argument checks of the four C entry points, which need no GPU."""
import ctypes
import os

import numpy as np
import pytest
import scipy.ndimage

from tests import segment_oracle as O


def same_partition(a, b):
  """Two label images describe the same components (0 = background in both), up to renumbering."""
  if not np.array_equal(a > 0, b > 0):
    return False
  pairs = set(zip(a[a > 0].tolist(), b[b > 0].tolist()))
  return len(pairs) == len(set(p[0] for p in pairs)) == len(set(p[1] for p in pairs))


@pytest.mark.parametrize('angle', [35, 60])
def test_oracle_components_are_scipy_ndimage_label_without_the_depth_gate(angle):
  sc = O.analytic_table(angle)
  fg = O.foreground(sc['depth'], sc['K'], sc['plane'], 0.008, 0.5)
  lab, rows, n_comp = O.segment(sc['depth'], sc['K'], sc['plane'], h_min=0.008, max_jump=np.inf, min_pixels=1)
  ref, n_ref = scipy.ndimage.label(fg)      # the default structure is the 4-neighbourhood
  assert n_comp == n_ref == lab.max() and n_ref >= 3
  assert same_partition(lab, ref)
  # numbered by the lowest pixel index, and the integer statistics agree with the label image
  first = [int(np.flatnonzero(lab.ravel() == k)[0]) for k in range(1, lab.max() + 1)]
  assert first == sorted(first) and first == rows[:, 15].tolist()
  assert rows[:, 0].tolist() == [int((lab == k).sum()) for k in range(1, lab.max() + 1)]


def test_oracle_serpentine_is_one_component():
  H, W = 37, 53
  d = np.full((H, W), 1.0, np.float32)
  d[0::2, :] = 0.5
  for k, r in enumerate(range(1, H, 2)):
    d[r, W - 1 if k % 2 == 0 else 0] = 0.5
  K = np.array([[50.0, 0, 26], [0, 50.0, 18], [0, 0, 1]])
  lab, rows, n = O.segment(d, K, [0, 0, -1, 1], h_min=0.25, h_max=0.75, max_jump=0.01, min_pixels=1)
  assert n == 1 and lab.max() == 1 and np.array_equal(lab > 0, d == 0.5)
  assert scipy.ndimage.label(d == 0.5)[1] == 1
  assert rows[0, 14] == 1 << 19 and rows[0, 0] == (d == 0.5).sum()      # height exactly 0.5 m


def test_oracle_plane_through_three_lattice_points_is_the_analytic_plane():
  # fx = fy = 64, cx = cy = 0 and depth 2: the points are (col / 32, row / 32, 2), exact in fp32
  K = np.array([[64.0, 0, 0], [0, 64.0, 0], [0, 0, 1]])
  d = np.full((8, 8), 2.0, np.float32)
  for trip in ([0, 1, 8], [0, 8, 1], [63, 5, 40]):      # both orientations of the triplet give the camera-facing normal
    planes, counts, best = O.plane_score(d, K, [trip], 0.001)
    assert np.array_equal(planes[0], np.array([0, 0, -1, 2], np.float32)) and counts[0] == 64 and best == 0
  # a tilted plane z = 1 + x / 2 through lattice points with exact coordinates: d = 1, 2 at x = 0, 2 (col 0 at d = 1, col 64 at d = 2)
  d = np.zeros((2, 65), np.float32)
  d[0, 0], d[1, 0], d[0, 64] = 1.0, 1.0, 2.0
  planes, counts, best = O.plane_score(d, K, [[0, 65, 64]], 0.001)
  n = np.array([1.0, 0, -2.0]) / np.sqrt(5.0)      # z - x / 2 - 1 = 0, oriented so that the origin is on the positive side
  assert np.allclose(planes[0, :3], n, atol=1e-7, rtol=0) and abs(planes[0, 3] - 2 / np.sqrt(5.0)) < 1e-7 and counts[0] == 3


def test_oracle_moments_are_the_plain_sums():
  sc = O.analytic_table(35)
  s = O.plane_moments(sc['depth'], sc['K'], sc['plane'], 0.004)
  x, y, z = (a.astype(np.float64) for a in O.points(sc['depth'], sc['K']))
  inl = O.ok_map(sc['depth']) & (np.abs(O.height(sc['plane'], *O.points(sc['depth'], sc['K']))) < np.float32(0.004))
  ref = [inl.sum(), x[inl].sum(), y[inl].sum(), z[inl].sum(), (x * x)[inl].sum(), (x * y)[inl].sum(), (x * z)[inl].sum(), (y * y)[inl].sum(),
         (y * z)[inl].sum(), (z * z)[inl].sum()]
  # 6912 terms of magnitude below 1: any order agrees to 6912 x 2^-53 < 1e-12 absolute
  assert s[0] == ref[0] and np.allclose(s, ref, rtol=0, atol=1e-12 * max(1.0, ref[0]))
  plane, w = O.plane_from_moments(s)
  assert np.arccos(min(1.0, plane[:3] @ sc['plane'][:3])) < 1e-4 and abs(plane[3] - sc['plane'][3]) < 1e-5


def stats_of(extents):
  return dict(label=np.arange(1, len(extents) + 1, dtype=np.int32), extent=np.asarray(extents, dtype=np.float64))


def test_assign_segments_tie_goes_to_the_lower_object_then_the_lower_label():
  from foundationpose_amd.segment import assign_segments
  # both objects are equally far from both segments: object 0 takes label 1, object 1 the other one
  labels, cost = assign_segments(stats_of([0.10, 0.10]), [0.10, 0.10])
  assert labels == [1, 2] and cost.shape == (2, 2) and (cost == 0).all()
  labels, cost = assign_segments(stats_of([0.30, 0.10, 0.20]), [0.21, 0.11])
  assert labels == [3, 2] and np.allclose(cost, [[0.09, 0.11, 0.01], [0.19, 0.01, 0.09]])


def test_assign_segments_object_without_a_segment_and_spare_segments():
  from foundationpose_amd.segment import assign_segments
  labels, cost = assign_segments(stats_of([0.2]), [0.1, 0.2, 0.5])
  assert labels == [-1, 1, -2] and cost.shape == (3, 1)      # negative labels match no pixel and stay pairwise different
  labels, cost = assign_segments(stats_of([]), [0.1])
  assert labels == [-1] and cost.shape == (1, 0)
  labels, cost = assign_segments(stats_of([0.05, 0.5, 0.21, 0.1]), [0.2, 0.1])      # more segments than objects: the nearest two
  assert labels == [3, 4]
  with pytest.raises(ValueError):
    assign_segments(stats_of([0.1]), [0.1], prefer='colour')


def test_load_reference_views_without_masks(tmp_path):
  from PIL import Image
  from foundationpose_amd.reconstruct import load_reference_views
  for sub in ('rgb', 'depth'):
    os.makedirs(tmp_path / sub)
  rs = np.random.RandomState(0)
  for name in ('000', '001'):
    Image.fromarray(rs.randint(0, 255, (6, 8, 3)).astype(np.uint8)).save(tmp_path / 'rgb' / f'{name}.png')
    Image.fromarray(rs.randint(300, 900, (6, 8)).astype(np.uint16)).save(tmp_path / 'depth' / f'{name}.png')
  np.savetxt(tmp_path / 'K.txt', np.array([[90.0, 0, 4], [0, 90, 3], [0, 0, 1]]))
  views = load_reference_views(str(tmp_path), poses=False, masks=False)
  assert 'masks' not in views and 'cam_in_obs' not in views
  assert views['depths'].shape == (2, 6, 8) and views['depths'].dtype == np.float32 and views['names'] == ['000', '001']
  with pytest.raises(FileNotFoundError):      # the default still reads mask/
    load_reference_views(str(tmp_path), poses=False)


@pytest.fixture(scope='module')
def built():
  import __graft_entry__ as g
  g.build()
  from foundationpose_amd import _lib
  return _lib


def test_argument_checks_need_no_gpu(built):
  L = built.lib()
  EINVAL = built.FP_EINVAL
  fake = ctypes.c_void_p(64)                     # never dereferenced: the null and range checks come first
  pp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
  K = np.array([[90.0, 0, 4], [0, 90.0, 3], [0, 0, 1]])
  plane = np.array([[0.0, 0, -1, 1]])
  trip = np.zeros((1, 4, 3), np.int32)
  hp, hc, hb = np.zeros((1, 4, 4), np.float32), np.zeros((1, 4), np.int32), np.zeros((1,), np.int32)
  sums, counts = np.zeros((1, 10)), np.zeros((1, 2), np.int32)

  def score(ctx=fake, depth=fake, n=1, H=6, W=8, Kk=K, zfar=100.0, t=trip, nh=4, tol=0.005, planes=hp, cnt=hc, best=hb):
    return L.fp_plane_score(ctx, depth, None, n, H, W, pp(Kk), zfar, pp(t), nh, tol, pp(planes), pp(cnt), pp(best), None)

  def moments(ctx=fake, depth=fake, n=1, H=6, W=8, Kk=K, zfar=100.0, p=plane, tol=0.005, out=sums):
    return L.fp_plane_moments(ctx, depth, None, n, H, W, pp(Kk), zfar, pp(p), tol, pp(out), None)

  def count(ctx=fake, depth=fake, n=1, H=6, W=8, Kk=K, zfar=100.0, p=plane, h_min=0.01, h_max=0.5, jump=0.01, min_pixels=1, out=counts):
    return L.fp_depth_segment_count(ctx, depth, None, n, H, W, pp(Kk), zfar, pp(p), h_min, h_max, jump, min_pixels, pp(out), None)

  bad_K = K.copy()
  bad_K[0, 0] = 0
  nan_K = K.copy()
  nan_K[1, 2] = np.nan
  shared = [dict(ctx=None), dict(depth=None), dict(Kk=None), dict(H=0), dict(W=0), dict(n=-1), dict(n=65), dict(Kk=bad_K), dict(Kk=nan_K),
            dict(zfar=0.0), dict(zfar=1000.5), dict(zfar=float('nan')), dict(zfar=float('inf')), dict(H=1 << 15, W=1 << 14)]
  for fn, own in ((score, [dict(tol=0.0), dict(tol=float('nan')), dict(nh=-1), dict(nh=1025), dict(t=None), dict(planes=None), dict(cnt=None),
                           dict(best=None)]),
                  (moments, [dict(tol=0.0), dict(p=None), dict(out=None), dict(p=np.array([[0.0, 0, 0, 1]])), dict(p=np.array([[0.0, np.inf, 1, 1]])),
                             dict(p=np.array([[0.0, 1e-60, 0, 1]]))]),
                  (count, [dict(jump=0.0), dict(jump=float('nan')), dict(h_min=0.5, h_max=0.4), dict(h_min=float('nan')), dict(min_pixels=0),
                           dict(p=None), dict(out=None), dict(p=np.array([[0.0, 0, 0, 1]])), dict(p=np.array([[np.nan, 0, 1, 1]]))])):
    for kw in shared + own:
      assert fn(**kw) == EINVAL, (fn.__name__, kw)
      assert L.fp_last_error()
  assert L.fp_depth_segment_write(None, fake, 1, 6, 8, fake, fake, 0, None) == EINVAL
