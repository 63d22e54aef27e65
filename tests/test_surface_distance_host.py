"""CPU: tests/surface_distance_oracle.py - the float64 restatement of fp_point_mesh_distance and fp_mesh_sample_surface that the GPU tests
compare with - against answers that do not share its arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

from tests import mesh_simplify_oracle as MS
from tests import surface_distance_oracle as O
from tests import tsdf_oracle as TO


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_lattice_cases_all_seven_regions(dtype):
  """hand-written rational d2; in float32 too: every intermediate is a small integer or a dyadic rational (the GPU test asserts equality)"""
  tri = O.LATTICE_TRIANGLE
  for p, (num, den), region in O.LATTICE_CASES:
    d2, q = O.pair_distance2(np.array(p, dtype), *tri.astype(dtype))
    assert d2.dtype == dtype and Fraction(float(d2)) == Fraction(num, den), (p, region, float(d2))
    assert Fraction(float(((np.array(p, np.float64) - q.astype(np.float64)) ** 2).sum())) == Fraction(num, den), (p, region)
  pts = np.array([c[0] for c in O.LATTICE_CASES], dtype)
  d, face, _ = O.point_mesh_distance(pts, tri, [[0, 1, 2]], dtype=dtype)
  assert np.array_equal(d, np.sqrt(np.array([c[1][0] for c in O.LATTICE_CASES], dtype))) and (face == 0).all()


def _segment_distance(p, a, b):
  p, a, b = (np.asarray(x, np.float64) for x in (p, a, b))
  t = np.clip(((p - a) @ (b - a)) / ((b - a) @ (b - a)), 0, 1)
  return np.linalg.norm(p - (a + t * (b - a)))


def test_degenerate_faces():
  rng = np.random.default_rng(3)
  pts = np.concatenate([rng.uniform(-3, 5, (200, 3)), [[1, 0, 0], [0, 0, 0], [2, 0, 0], [3, 0, 0], [-1, 2, 2], [1.5, 1, 0]]])
  v = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0], [1, 1, 1]], np.float64)
  d, face, closest = O.point_mesh_distance(pts, v, [[0, 1, 2]])
  assert np.isfinite(d).all() and (face == 0).all()
  assert np.allclose(d, [_segment_distance(p, v[0], v[1]) for p in pts], rtol=0, atol=1e-14)
  assert np.allclose(np.linalg.norm(pts - closest, axis=1), d, rtol=0, atol=1e-14)
  d, face, closest = O.point_mesh_distance(pts, v, [[3, 3, 3]])
  assert np.array_equal(d, np.sqrt(((pts - v[3]) ** 2).sum(1))) and (closest == v[3]).all()
  # two coincident vertices: the segment between the two distinct ones
  d, _, _ = O.point_mesh_distance(pts, v, [[0, 0, 3]])
  assert np.allclose(d, [_segment_distance(p, v[0], v[3]) for p in pts], rtol=0, atol=1e-14)


def test_ties_nan_and_bad_faces():
  v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [np.nan, 0, 0], [0, 0, 1]], np.float64)
  pts = np.array([[1, 1, 3], [np.nan, 0, 0], [0, np.inf, 0], [1, 1, -1]])
  d, face, closest = O.point_mesh_distance(pts, v, [[0, 1, 3], [0, 1, 7], [0, 1, 2], [0, 1, 2]])
  assert face.tolist() == [2, -1, -1, 2] and d[0] == 3 and d[3] == 1 and np.isnan(d[1:3]).all() and np.isnan(closest[1:3]).all()
  d, face, _ = O.point_mesh_distance(pts, v, [[0, 1, 3], [-1, 1, 2]])
  assert (face == -1).all() and np.isnan(d).all()


def test_cube_ties_by_hand():
  """the hand-written winners of the GPU tie test (tests/test_gpu_surface_distance.py CUBE_TIES), in float32 and float64: every tied face
  gives the same exact d2, and the lowest index wins"""
  ties = [((1, -1, -1), (0, 4), 2), ((-1, -1, -1), (0, 4, 8), 3), ((3, 3, 3), (3, 7, 11), 3), ((3, 1, 3), (3, 11), 2), ((1, 3, 3), (3, 7), 2),
          ((3, 3, 1), (7, 11), 2), ((1, 1, -1), (0, 1), 1), ((1, 1, 1), tuple(range(12)), 1), ((1, 1, 3), (2, 3), 1), ((3, 1, 1), (10, 11), 1)]
  v, f = O.lattice_cube()
  for dtype in (np.float32, np.float64):
    for q, tied, d2 in ties:
      all_d2, _ = O.pair_distance2(np.array(q, dtype), *(v[f].astype(dtype)[:, k] for k in range(3)))
      assert tuple(np.flatnonzero(all_d2 == d2)) == tied and (all_d2 >= d2).all(), (q, all_d2)
    d, face, _ = O.point_mesh_distance([t[0] for t in ties], v, f, dtype=dtype)
    assert face.tolist() == [t[1][0] for t in ties] and np.array_equal(d, np.sqrt(np.array([t[2] for t in ties], dtype)))


@pytest.fixture(scope='module')
def closed_meshes():
  sv, sf, _ = MS.uv_sphere(rings=23, segments=40)
  cv, cf, _, _ = MS.composite_mesh()
  pick = np.random.default_rng(0).choice(len(cf), 2000, replace=False)
  return [(sv, sf), (cv, cf[np.sort(pick)])]


def test_upper_bound_by_nearest_neighbour_and_lower_bound_by_the_plane(closed_meshes):
  """samples lie ON the surface, so the nearest sample can only be farther than the surface; the winning face's plane can only be nearer"""
  from scipy.spatial import cKDTree
  for k, (v, f) in enumerate(closed_meshes):
    v64 = v.astype(np.float64)
    lo, hi = v64[f].min((0, 1)), v64[f].max((0, 1))
    rng = np.random.default_rng(10 + k)
    pts = np.concatenate([rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), (700, 3)), v64[f[:100, 0]],
                          TO.surface_samples(v64, f, n=200, seed=5)])
    d, face, closest = O.point_mesh_distance(pts, v64, f)
    nn, _ = cKDTree(TO.surface_samples(v64, f, n=60000, seed=1)).query(pts)
    assert (d <= nn + 1e-15).all(), float((d - nn).max())
    assert (d[700:800] == 0).all() and d[800:].max() < 1e-15
    tri = v64[f[face]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    plane = np.abs(((pts - tri[:, 0]) * n).sum(1)) / np.linalg.norm(n, axis=1)
    assert (d >= plane - 1e-12).all(), float((plane - d).max())
    assert np.allclose(np.linalg.norm(pts - closest, axis=1), d, rtol=0, atol=1e-15)
    # the sampling is dense enough for the bound to mean something: the median gap is a small part of the mesh's size
    assert np.median(nn - d) < 0.02 * np.linalg.norm(hi - lo)


def test_sphere_bounds():
  R = 0.75
  v, f = O.icosphere(2, radius=R)
  v64 = v.astype(np.float64)
  tri = v64[f]
  n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
  r_in = (np.abs((tri[:, 0] * n).sum(1)) / np.linalg.norm(n, axis=1)).min()
  assert 0.9 * R < r_in < R
  x = np.random.default_rng(4).normal(size=(3000, 3))
  pts = R * x / np.linalg.norm(x, axis=1, keepdims=True)
  d, _, _ = O.point_mesh_distance(pts, v64, f)
  assert (d >= 0).all() and (d <= R - r_in + 1e-7).all() and d.max() > 0.5 * (R - r_in)
  # inside the inscribed ball, along a ray: never nearer than r_in - |p|
  d_in, _, _ = O.point_mesh_distance(0.5 * r_in * x / np.linalg.norm(x, axis=1, keepdims=True), v64, f)
  assert (d_in >= 0.5 * r_in - 1e-7).all() and (d_in <= R - 0.5 * r_in + 1e-7).all()


@pytest.mark.parametrize('n', [1, 7, 1000, 20000])
def test_sampler(n):
  v, f = O.icosphere(1)
  v, f = np.concatenate([v, 3 * v[:3] + 5]), np.concatenate([f, [[42, 43, 44]], [[0, 0, 1]]]).astype(np.int32)      # one large face, one without area
  aq = O.area_q(v, f)
  area = O.face_areas(v, f)
  assert aq[-1] == 0 and abs(int(aq.sum()) - (1 << 40)) <= len(f) and np.abs(aq - area / area.sum() * 2.0 ** 40).max() <= 0.5
  pts, face, bary = O.sample_surface(v, f, n, seed=3)
  counts = np.bincount(face, minlength=len(f))
  assert counts.sum() == n and counts[-1] == 0
  assert (np.abs(counts - n * area / area.sum()) <= 1 + 1e-6).all()
  assert (np.diff(face) >= 0).all()                        # stratified along the face order
  assert bary.dtype == np.float32 and (bary >= 0).all() and (bary <= 1).all() and (bary.astype(np.float64).sum(1) <= 1).all()
  # the points lie on their faces
  d, _ = O.point_face_distance(pts, v, f, face)
  assert d.max() < 1e-12
  _, face_b, bary_b = O.sample_surface(v, f, n, seed=3)
  assert np.array_equal(face, face_b) and np.array_equal(bary, bary_b)
  _, face_c, bary_c = O.sample_surface(v, f, n, seed=4)
  assert np.array_equal(face, face_c) and not np.array_equal(bary, bary_c)


def test_hash_and_uniforms():
  assert [int(x) for x in O.lowbias32(np.array([0, 1, 2, 0xffffffff]))] == [_lowbias32_int(x) for x in (0, 1, 2, 0xffffffff)]
  b = O.sample_bary(200000, 1).astype(np.float64)
  assert abs(b[:, 0].mean() - 1 / 3) < 5e-3 and abs(b[:, 1].mean() - 1 / 3) < 5e-3 and abs((b[:, 0] * b[:, 1]).mean() - 1 / 12) < 5e-3


def _lowbias32_int(x):
  x ^= x >> 16
  x = (x * 0x7feb352d) & 0xffffffff
  x ^= x >> 15
  x = (x * 0x846ca68b) & 0xffffffff
  x ^= x >> 16
  return x
