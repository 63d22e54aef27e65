"""CPU: the host side of Utils.oriented_bounds (foundationpose_amd/bounds.py) - the candidate builder, the convention of the result,
degenerate input and the untouched default of model_box.  The device call is replaced by the numpy restatement of fp_box_extents
(tests/oriented_bounds_oracle.py: `evaluate=O.winner_f32`); the float64 yardstick is the oracle's rotating calipers per hull normal,
which shares no code with bounds.py."""
import numpy as np
import pytest

from tests import oriented_bounds_oracle as O

REL = 1e-9


def _sets():
  from foundationpose_amd import synthetic as S
  small = S.make_mustard_mesh(seed=0, n_theta=24, n_z=20)
  return {'box': O.rotated_box(), 'cloud': O.gaussian_cloud(), 'mustard_small': np.asarray(small.vertices, dtype=np.float64) @ O.rotvec_matrix(O.ROTVEC).T}


def _min_volume(cand):
  return min(O.box_volume_f64(cand['points'], f) for f in cand['frames'])


def test_rotated_box_is_recovered():
  """0.05 x 0.12 x 0.2 m with 500 interior points, turned by rotvec (0.3, -0.7, 0.5) and shifted: the axis-aligned box is 6.6 times too
  large, the PCA frame 17 % - the search recovers the box."""
  from foundationpose_amd import bounds as B
  pts = O.rotated_box()
  to_origin, extents, info = B.oriented_bounds(pts, return_info=True, evaluate=O.winner_f32)
  print(f'extents {extents!r} volume {info["volume"]!r} aabb {info["aabb_volume"]:.6e} pca {info["pca_volume"]:.6e} candidates {info["n_candidates"]}')
  np.testing.assert_allclose(extents, O.BOX, rtol=REL, atol=0)
  assert abs(info['volume'] - 1.2e-3) <= REL * 1.2e-3
  assert info['hull_vertices'] == 8 and info['rank'] == 3
  assert info['aabb_volume'] > 6.5 * info['volume'] and info['pca_volume'] > 1.15 * info['volume']
  # the fp32 evaluation of the oracle alone, on the builder's candidates: the winner's float64 volume is the box's
  cand = B.hull_candidates(pts)
  w = O.box_extents_f32(cand['points'], cand['frames'])
  assert abs(O.box_volume_f64(cand['points'], cand['frames'][w['index']]) - 1.2e-3) <= REL * 1.2e-3
  assert abs(float(w['volume']) - 1.2e-3) <= 1e-5 * 1.2e-3           # and its fp32 volume is that to fp32's precision


@pytest.mark.parametrize('name', ['box', 'cloud'])
def test_silhouette_pairs_hold_the_minimum_of_the_full_class(name):
  from foundationpose_amd import bounds as B
  pts = _sets()[name]
  sil, full = B.hull_candidates(pts), B.hull_candidates(pts, silhouette=False)
  assert len(sil['frames']) <= len(full['frames'])
  v_sil, v_full = _min_volume(sil), _min_volume(full)
  v_cal, rows, n_normals = O.calipers_min_volume(pts)
  v_brute = O.calipers_min_volume(pts, brute=True)[0]
  print(f'{name}: {len(sil["frames"])} silhouette pairs of {len(full["frames"])}, {n_normals} normals; silhouette {v_sil!r} full {v_full!r} '
        f'calipers {v_cal!r} brute {v_brute!r}')
  assert n_normals == len(sil['normals'])
  assert abs(v_sil - v_full) <= REL * v_full
  assert abs(v_sil - v_cal) <= REL * v_cal
  assert abs(v_cal - v_brute) <= REL * v_cal                          # the calipers agree with trying every edge against every vertex
  assert abs(O.box_volume_f64(pts, rows) - v_cal) <= REL * v_cal     # and their frame has that volume over ALL points
  frames = sil['frames']
  np.testing.assert_allclose(frames @ frames.transpose(0, 2, 1), np.broadcast_to(np.eye(3), frames.shape), atol=1e-12)
  np.testing.assert_allclose(np.linalg.det(frames), 1.0, atol=1e-12)


def _sign_rule(R):
  return all(R[k, np.argmax(np.abs(R[k]))] > 0 for k in (0, 1))


@pytest.mark.parametrize('name', ['box', 'cloud', 'mustard_small'])
def test_convention_of_the_result(name):
  from foundationpose_amd import bounds as B
  pts = _sets()[name]
  to_origin, extents, info = B.oriented_bounds(pts, return_info=True, evaluate=O.winner_f32)
  R = to_origin[:3, :3]
  assert to_origin.dtype == np.float64 and extents.dtype == np.float64 and to_origin.shape == (4, 4) and extents.shape == (3,)
  assert abs(np.linalg.det(R) - 1) <= 1e-12 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
  np.testing.assert_array_equal(to_origin[3], [0, 0, 0, 1])
  assert (np.diff(extents) >= 0).all()
  assert _sign_rule(R)
  np.testing.assert_allclose(R[2], np.cross(R[0], R[1]), atol=1e-15)
  q = pts @ R.T + to_origin[:3, 3]
  assert (np.abs(q) <= extents / 2 * (1 + 1e-12)).all()
  assert (q.max(axis=0) >= extents / 2 * (1 - 1e-12)).all() and (q.min(axis=0) <= -extents / 2 * (1 - 1e-12)).all()      # and it is tight
  assert info['volume'] <= info['aabb_volume'] * (1 + REL) and info['volume'] <= info['pca_volume'] * (1 + REL)
  # ordered=False keeps the rows u, m x u, m: row 2 is the winning hull normal up to the sign the rule gives it
  to2, ext2, info2 = B.oriented_bounds(pts, ordered=False, return_info=True, evaluate=O.winner_f32)
  assert abs(abs(to2[2, :3] @ info2['normal']) - 1) <= 1e-12 and _sign_rule(to2[:3, :3]) and abs(np.linalg.det(to2[:3, :3]) - 1) <= 1e-12
  np.testing.assert_allclose(np.sort(ext2), extents, rtol=1e-12)
  i, j = info2['edge']
  e = (pts[j] - pts[i]) / np.linalg.norm(pts[j] - pts[i])
  assert abs(to2[1, :3] @ e) <= 1e-9                                  # the edge lies in the plane of rows u and m
  # a mesh object and its vertices give the same
  class Mesh:
    vertices = pts
  np.testing.assert_array_equal(B.oriented_bounds(Mesh(), evaluate=O.winner_f32)[0], to_origin)


def test_ties_of_extents_keep_the_builders_order():
  """A cube: three equal extents.  The stable sort leaves the rows in the order u, m x u, m."""
  from foundationpose_amd import bounds as B
  cube = np.array([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], dtype=np.float64) * 0.25
  a, ea = B.oriented_bounds(cube, ordered=True, evaluate=O.winner_f32)
  b, eb = B.oriented_bounds(cube, ordered=False, evaluate=O.winner_f32)
  np.testing.assert_array_equal(ea, [0.25, 0.25, 0.25])
  np.testing.assert_array_equal(a, b)
  np.testing.assert_allclose(a[:3, 3], -a[:3, :3] @ np.full(3, 0.125), atol=1e-15)


def test_degenerate_input():
  from foundationpose_amd import bounds as B
  Rm = O.rotvec_matrix(O.ROTVEC)
  never = lambda *a: pytest.fail('degenerate input is handled on the host alone')
  # planar: a 0.3 x 0.1 rectangle with points inside, turned and shifted
  rs = np.random.RandomState(3)
  flat = np.concatenate([np.array([[0, 0, 0], [0.3, 0, 0], [0.3, 0.1, 0], [0, 0.1, 0]]), np.c_[rs.rand(200, 2) * [0.3, 0.1], np.zeros(200)]])
  pts = flat @ Rm.T + O.SHIFT
  to_origin, extents, info = B.oriented_bounds(pts, return_info=True, evaluate=never)
  assert info['rank'] == 2 and extents[0] == 0.0 and info['volume'] == 0.0
  np.testing.assert_allclose(extents[1:], [0.1, 0.3], rtol=REL)
  assert abs(abs(to_origin[0, :3] @ Rm[:, 2]) - 1) <= 1e-12          # the zero extent lies along the plane's normal
  assert abs(np.linalg.det(to_origin[:3, :3]) - 1) <= 1e-12
  q = pts @ to_origin[:3, :3].T + to_origin[:3, 3]
  assert (np.abs(q) <= extents / 2 * (1 + 1e-12) + 1e-15).all()
  # exactly planar in its own axes, unordered: rows u, m x u, m with m the normal
  to2, ext2 = B.oriented_bounds(flat, ordered=False, evaluate=never)
  assert ext2[2] == 0.0 and abs(abs(to2[2, 2]) - 1) <= 1e-12 and sorted(np.round(ext2[:2], 12)) == [0.1, 0.3]
  # collinear
  line = (np.linspace(-0.2, 0.5, 17)[:, None] * np.array([[1.0, 2.0, -2.0]]) / 3) + O.SHIFT
  to_origin, extents, info = B.oriented_bounds(line, return_info=True, evaluate=never)
  assert info['rank'] == 1 and extents[0] == 0.0 and extents[1] == 0.0 and abs(extents[2] - 0.7) <= REL
  assert abs(np.linalg.det(to_origin[:3, :3]) - 1) <= 1e-12
  assert abs(abs(to_origin[2, :3] @ np.array([1.0, 2.0, -2.0]) / 3) - 1) <= 1e-12
  q = line @ to_origin[:3, :3].T + to_origin[:3, 3]
  assert np.abs(q[:, :2]).max() <= 1e-12 and abs(np.abs(q[:, 2]).max() - 0.35) <= 1e-12
  # two points are a line as well
  assert abs(B.oriented_bounds(line[[0, -1]], evaluate=never)[1][2] - 0.7) <= REL
  # one point, and copies of one point
  for one in (O.SHIFT[None], np.tile(O.SHIFT, (5, 1))):
    to_origin, extents, info = B.oriented_bounds(one, return_info=True, evaluate=never)
    assert info['rank'] == 0
    np.testing.assert_array_equal(extents, [0, 0, 0])
    np.testing.assert_array_equal(to_origin[:3, :3], np.eye(3))
    np.testing.assert_array_equal(to_origin[:3, 3], -O.SHIFT)
  # no point, and points that are not finite
  with pytest.raises(ValueError):
    B.oriented_bounds(np.zeros((0, 3)), evaluate=never)
  with pytest.raises(ValueError):
    B.oriented_bounds(np.array([[0.0, np.nan, 0.0]]), evaluate=never)


def test_model_box_default_is_unchanged_and_takes_the_keyword():
  import inspect
  from foundationpose_amd import Utils as U, synthetic as S
  from foundationpose_amd import bounds as B
  mesh = S.make_mustard_mesh(seed=0)
  v = np.asarray(mesh.vertices, dtype=np.float64)
  lo, hi = v.min(axis=0), v.max(axis=0)
  want_t = np.eye(4)
  want_t[:3, 3] = -(lo + hi) / 2
  want_b = np.stack([-(hi - lo) / 2, (hi - lo) / 2])
  for got in (U.model_box(mesh), U.model_box(mesh, oriented=False), U.model_box(v)):
    np.testing.assert_array_equal(got[0], want_t)
    np.testing.assert_array_equal(got[1], want_b)
  assert inspect.signature(U.model_box).parameters['oriented'].default is False
  assert U.oriented_bounds is B.oriented_bounds and U.box_extents is B.box_extents
  from foundationpose_amd.estimater import FoundationPose
  from foundationpose_amd.pipeline import FoundationPoseEstimator
  from foundationpose_amd.tracking import MultiObjectTracker
  assert inspect.signature(FoundationPose.model_box).parameters['oriented'].default is False
  assert inspect.signature(FoundationPoseEstimator.__init__).parameters['box'].default == 'aabb'
  assert inspect.signature(MultiObjectTracker.draw).parameters['oriented'].default is False
  with pytest.raises(ValueError):
    FoundationPoseEstimator(mesh=mesh, K=np.eye(3), box='obb')


def test_oracle_total_order():
  """The numpy restatement itself: ties go to the lowest index, a NaN volume and a candidate without a finite projection never win."""
  cube = np.array([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], dtype=np.float32)
  eye = np.eye(3, dtype=np.float32)
  big = np.float32(2) * eye
  nan = np.full((3, 3), np.nan, dtype=np.float32)
  r = O.box_extents_f32(cube, np.stack([nan, big, eye, eye]))
  assert r['index'] == 2 and r['volume'] == 1.0 and r['all_volume'][0] == -np.inf and r['all_volume'][1] == 8.0
  np.testing.assert_array_equal(r['all_lohi'][2], [0, 0, 0, 1, 1, 1])
  np.testing.assert_array_equal(r['all_lohi'][0], [np.inf] * 3 + [-np.inf] * 3)
  assert O.box_extents_f32(cube, nan[None])['index'] == -1
  far = O.box_extents_f32(np.array([[3e38, 0, 0]], dtype=np.float32), np.stack([big, eye]))      # inf - inf: a NaN volume
  assert np.isnan(far['all_volume'][0]) and far['index'] == 1 and far['volume'] == 0.0
  pts = np.array([[np.nan, 0, 0], [1, 2, 3]], dtype=np.float32)      # a NaN projection is passed over
  np.testing.assert_array_equal(O.box_extents_f32(pts, eye[None])['all_lohi'][0], [1, 2, 3, 1, 2, 3])
