"""GPU: the exact point-to-mesh distance, the surface sampler and the distance statistics (csrc/surface_distance.hip; Utils.point_mesh_distance,
sample_surface, distance_stats, mesh_distance) against the float64 restatement of the header's rules (tests/surface_distance_oracle.py):
exactly where fp32 is exact (lattice cases, ties, bad values, counts, maxima, the sampler's integers), within a measured multiple of the
fp32 rounding unit elsewhere.

Shapes: T = FP_SURFDIST_TILE queries of a workgroup, C = FP_SURFDIST_CHUNK face records of an LDS chunk; n in {1, T-1, T, T+1, 2T+3} at
F = C+1 and F in {1, C-1, C, C+1, 2C+5} at n = T+1 (prefixes of one seeded soup of independent random triangles in [-1, 1]^3: two or
three face slices of one chunk each, folded by the integer atomicMin); 600 copies of the 2T+3 queries for the form with one slice
of three chunks."""
import math

import numpy as np
import pytest
import torch

from tests import surface_distance_oracle as O
from tests.test_gpu_tsdf import fused, mustard_views  # noqa: F401  (fixtures: the 12 fused mustard views)

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
# |d_dev - d_64| <= TOL_C 2^-24 scale, scale = the bounding-box diagonal of points and mesh.  Measured, not guessed: the largest
# |d_dev - d_64| / (2^-24 scale) over the boundary shapes below on an MI355X is TOL_C_OBSERVED = 0.844 (the float64 excess of the device's
# chosen face over the minimum was 0 for every query; `closest` was off by 2.04 at most); TOL_C is 4 x that, for the compiler's freedom
# to order fp32 sums.
TOL_C_OBSERVED = 0.844
TOL_C = 4 * TOL_C_OBSERVED


def _lib():
  from foundationpose_amd import _lib
  return _lib


def _U():
  from foundationpose_amd import Utils
  return Utils


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _dev(a, dtype=None):
  return torch.as_tensor(np.ascontiguousarray(a), device='cuda').to(dtype) if dtype else torch.as_tensor(np.ascontiguousarray(a), device='cuda')


@pytest.fixture(scope='module')
def soup():
  L = _lib()
  T, C = L.FP_SURFDIST_TILE, L.FP_SURFDIST_CHUNK
  v, f = O.random_soup(2 * C + 5, seed=11)
  pts = np.random.default_rng(12).uniform(-1, 1, (2 * T + 3, 3)).astype(np.float32)
  pts[:40] = v[f[:40, 0]] + np.float32(0.01) * pts[:40]        # some queries close to a face
  pts[40:60] = v[f[40:60, 1]]                                  # and some on a vertex
  scale = float(np.linalg.norm(np.maximum(v.max(0), pts.max(0)).astype(np.float64) - np.minimum(v.min(0), pts.min(0))))
  return dict(T=T, C=C, v=v, f=f, pts=pts, scale=scale, ref={})


def _shapes(T, C):
  return [(n, C + 1) for n in (1, T - 1, T, T + 1, 2 * T + 3)] + [(T + 1, F) for F in (1, C - 1, C, 2 * C + 5)]


def _reference(soup, F):
  """the float64 result of all 2T+3 queries against the first F faces: computed once per F, never changed"""
  if F not in soup['ref']:
    soup['ref'][F] = O.point_mesh_distance(soup['pts'], soup['v'], soup['f'][:F])
  return soup['ref'][F]


# ---- 1. lattice and degenerate cases: exact ---------------------------------------------------------------------------------------------
def test_lattice_cases_are_exact():
  """every intermediate is a small integer or a dyadic rational (tests/test_surface_distance_host.py runs the rule in float32 numpy), so
  d2 is exact and dist is its correctly rounded root: dist is compared bit for bit with sqrt(float32(d2)), which asks no less than
  equality of dist^2 with d2 would if the root were exact (it is not for d2 = 2 and 5)."""
  U = _U()
  pts = np.array([c[0] for c in O.LATTICE_CASES], np.float32)
  want2 = np.array([c[1][0] / c[1][1] for c in O.LATTICE_CASES], np.float32)
  d, face, closest = U.point_mesh_distance(pts, vertices=O.LATTICE_TRIANGLE, faces=[[0, 1, 2]], return_face=True, return_closest=True)
  assert d.dtype == np.float32 and np.array_equal(d, np.sqrt(want2)), d
  assert np.array_equal(d[[0, 1, 5]] ** 2, want2[[0, 1, 5]])      # the perfect squares 9, 25, 4
  assert (face == 0).all()
  assert np.array_equal(closest, np.array([[1, 1, 0], [0, 0, 0], [4, 0, 0], [0, 4, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0]], np.float32))
  # degenerate faces: the collinear face is its segment, the point face its point; a vertex gives exactly 0; never NaN
  v = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0], [1, 1, 1]], np.float32)
  q = np.array([[1, 0, 0], [0, 0, 0], [2, 0, 0], [3, 0, 0], [-1, 2, 2], [1.5, 1, 0], [1, 1, 1], [0.5, -2, 0]], np.float32)
  d, closest = U.point_mesh_distance(q, vertices=v, faces=[[0, 1, 2]], return_closest=True)
  assert np.array_equal(d, np.sqrt(np.array([0, 0, 0, 1, 9, 1, 2, 4], np.float32))), d
  assert np.array_equal(closest, np.array([[1, 0, 0], [0, 0, 0], [2, 0, 0], [2, 0, 0], [0, 0, 0], [1.5, 0, 0], [1, 0, 0], [0.5, 0, 0]], np.float32))
  d, closest = U.point_mesh_distance(q, vertices=v, faces=[[3, 3, 3]], return_closest=True)
  assert np.array_equal(d, np.sqrt(np.array([2, 3, 3, 6, 6, 1.25, 0, 10.25], np.float32))) and (closest == 1).all()
  d = U.point_mesh_distance(q, vertices=v, faces=[[0, 0, 1]])      # two coincident vertices: the segment (0,0,0) - (2,0,0)
  assert np.array_equal(d, np.sqrt(np.array([0, 0, 0, 1, 9, 1, 2, 4], np.float32)))


# ---- 2. boundary shapes against float64 ---------------------------------------------------------------------------------------------------
def test_boundary_shapes_against_float64(soup):
  U = _U()
  tol = TOL_C * EPS * soup['scale']
  v_d, pts_d = _dev(soup['v']), _dev(soup['pts'])
  worst = dict(dist=0.0, face=0.0, closest=0.0)
  failures = []
  for n, F in _shapes(soup['T'], soup['C']):
    d64, _, _ = _reference(soup, F)
    f_d = _dev(soup['f'][:F])
    d, face, closest = (x.cpu().numpy() for x in U.point_mesh_distance(pts_d[:n], vertices=v_d, faces=f_d, return_face=True, return_closest=True))
    assert d.shape == (n,) and face.shape == (n,) and closest.shape == (n, 3) and np.isfinite(d).all()
    assert face.min() >= 0 and face.max() < F
    e_dist = np.abs(d.astype(np.float64) - d64[:n])
    # every query: the float64 distance to the DEVICE's face is the float64 minimum to within tol (ties are the norm, so the index
    # itself is not compared), and `closest` is the float64 closest point on that face to within tol
    d_face, c_face = O.point_face_distance(soup['pts'][:n], soup['v'], soup['f'][:F], face)
    e_face = d_face - d64[:n]
    e_closest = np.linalg.norm(closest.astype(np.float64) - c_face, axis=1)
    ratios = [float(e.max() / (EPS * soup['scale'])) for e in (e_dist, e_face, e_closest)]
    print(f'n {n} F {F}: |d_dev - d_64| {ratios[0]:.3f}, chosen face {ratios[1]:.3f}, closest {ratios[2]:.3f}  (x 2^-24 scale {soup["scale"]:.3f})')
    for k, r in zip(worst, ratios):
      worst[k] = max(worst[k], r)
    if not ((e_dist <= tol).all() and (e_face >= -1e-15).all() and (e_face <= tol).all() and (e_closest <= tol).all()):
      failures.append((n, F, ratios))
  print(f'largest: {worst}; TOL_C {TOL_C}')
  assert not failures, failures
  assert (d64[40:60] == 0).all()


def test_a_query_on_a_vertex_is_exactly_zero(soup):
  d = _U().point_mesh_distance(soup['pts'][40:60], vertices=soup['v'], faces=soup['f'])
  assert (d == 0).all()


# ---- 3. the tie rule ---------------------------------------------------------------------------------------------------------------------
CUBE_TIES = [((1, -1, -1), 0, 2), ((-1, -1, -1), 0, 3), ((3, 3, 3), 3, 3), ((3, 1, 3), 3, 2), ((1, 3, 3), 3, 2), ((3, 3, 1), 7, 2),
             ((1, 1, -1), 0, 1), ((1, 1, 1), 0, 1), ((1, 1, 3), 2, 1), ((3, 1, 1), 10, 1)]      # query, lowest tied face, d2 - by hand


def test_ties_go_to_the_lowest_face_index(soup):
  U = _U()
  tri = np.array([[0.25, -0.5, 0.125], [0.75, 0.5, -0.25], [-0.5, 0.25, 0.5]], np.float32)
  d, face = U.point_mesh_distance(soup['pts'], vertices=np.concatenate([tri, tri]), faces=[[0, 1, 2], [3, 4, 5]], return_face=True)
  assert (face == 0).all()
  d_rev, face_rev = U.point_mesh_distance(soup['pts'], vertices=np.concatenate([tri, tri]), faces=[[3, 4, 5], [0, 1, 2]], return_face=True)
  assert (face_rev == 0).all() and np.array_equal(_bits(d), _bits(d_rev))
  v, f = O.lattice_cube()
  q = np.array([c[0] for c in CUBE_TIES], np.float32)
  d, face = U.point_mesh_distance(q, vertices=v, faces=f, return_face=True)
  assert face.tolist() == [c[1] for c in CUBE_TIES], face
  assert np.array_equal(d, np.sqrt(np.array([c[2] for c in CUBE_TIES], np.float32)))
  # the same cube behind 300 faces that are farther away: the winners move by 300, the order among them stays
  far_v, far_f = O.random_soup(300, seed=2)
  d2, face2 = U.point_mesh_distance(q, vertices=np.concatenate([far_v + np.float32(40), v]), faces=np.concatenate([far_f, f + len(far_v)]),
                                    return_face=True)
  assert np.array_equal(face2, face + 300) and np.array_equal(_bits(d2), _bits(d))


# ---- 4. bit identity -----------------------------------------------------------------------------------------------------------------------
def test_a_result_depends_on_the_point_and_the_mesh_alone(soup):
  U = _U()
  T, C = soup['T'], soup['C']
  v_d, f_d, pts_d = _dev(soup['v']), _dev(soup['f']), _dev(soup['pts'])
  run = lambda p: tuple(x.cpu().numpy() for x in U.point_mesh_distance(p, vertices=v_d, faces=f_d, return_face=True, return_closest=True))
  d, face, closest = run(pts_d)
  again = run(pts_d)
  assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((d, face, closest), again))
  rev = run(pts_d.flip(0).contiguous())
  assert all(np.array_equal(_bits(a), _bits(b[::-1])) for a, b in zip((d, face, closest), rev))
  for i in (0, 1, 63, 64, T - 1, T, 2 * T, 2 * T + 2):
    one = run(pts_d[i:i + 1])
    assert all(np.array_equal(_bits(a[i:i + 1]), _bits(b)) for a, b in zip((d, face, closest), one)), i
  # 600 copies: 1 202 tiles, so the faces stay in ONE slice of three chunks instead of three slices of one
  many = run(pts_d.repeat(600, 1))
  assert all(np.array_equal(_bits(np.tile(a, (600,) + (1,) * (a.ndim - 1))), _bits(b)) for a, b in zip((d, face, closest), many))


# ---- 5. bad values and bad arguments -------------------------------------------------------------------------------------------------------
def test_bad_values_and_arguments(soup):
  U, L = _U(), _lib()
  v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [np.nan, 0, 0], [0, 0, 1], [np.inf, 0, 0]], np.float32)
  q = np.array([[1, 1, 3], [np.nan, 0, 0], [0, np.inf, 0], [1, 1, -1], [0, 0, -np.inf]], np.float32)
  # faces on the device are not validated by the Python layer: the kernels find the index outside [0, V) and never follow the face
  faces = _dev(np.array([[0, 1, 3], [0, 1, 7], [0, -1, 2], [5, 1, 2], [0, 1, 2], [0, 1, 2]], np.int32))
  d, face, closest = (x.cpu().numpy() for x in U.point_mesh_distance(_dev(q), vertices=_dev(v), faces=faces, return_face=True, return_closest=True))
  assert face.tolist() == [4, -1, -1, 4, -1]
  assert d[0] == 3 and d[3] == 1 and np.isnan(d[[1, 2, 4]]).all() and np.isnan(closest[[1, 2, 4]]).all()
  assert np.array_equal(closest[[0, 3]], np.array([[1, 1, 0], [1, 1, 0]], np.float32))
  d, face = (x.cpu().numpy() for x in U.point_mesh_distance(_dev(q), vertices=_dev(v), faces=faces[:4], return_face=True))
  assert (face == -1).all() and np.isnan(d).all()
  with pytest.raises(ValueError, match='faces must be integers in'):
    U.point_mesh_distance(q, vertices=v, faces=[[0, 1, 7]])
  with pytest.raises(ValueError, match='at least one'):
    U.point_mesh_distance(q, vertices=v, faces=np.zeros((0, 3), np.int32))
  # the C ABI: F = 0 is FP_EINVAL, n = 0 succeeds and writes nothing
  ctx = L.Context.get(torch.device('cuda', torch.cuda.current_device()))
  v_d, q_d = _dev(v), _dev(q)
  out = torch.full((5,), 7.0, device='cuda')
  call = lambda n, F: L.lib().fp_point_mesh_distance(ctx.handle, L.ptr(q_d), n, L.ptr(v_d), len(v), L.ptr(faces), F, L.ptr(out), None, None,
                                                     L.stream_ptr())
  assert call(5, 0) == L.FP_EINVAL and b'F 0' in L.lib().fp_last_error()
  assert call(0, 6) == 0 and call(-1, 6) == L.FP_EINVAL
  torch.cuda.synchronize()
  assert (out == 7).all()
  assert U.point_mesh_distance(np.zeros((0, 3), np.float32), vertices=v, faces=[[0, 1, 2]]).shape == (0,)


# ---- 6. statistics -------------------------------------------------------------------------------------------------------------------------
def test_statistics(soup):
  U, L = _U(), _lib()
  d = U.point_mesh_distance(_dev(soup['pts']).repeat(5, 1), vertices=_dev(soup['v']), faces=_dev(soup['f']))      # 10 255 entries: 3 tiles
  h = d.cpu().numpy()
  taus = [0.0, float(np.median(h)), float(h[7]), 0.05, float(h.max()), 10.0]
  s = U.distance_stats(d, taus)
  h64 = h.astype(np.float64)
  assert s['n'] == len(h) and s['not_finite'] == 0 and s['max'] == float(h.max())
  assert s['within'] == [int((h64 <= t).sum()) for t in taus] and s['within'][0] >= 20 and s['within'][-1] == len(h)
  # n 2^-53 relative for a double sum of n terms in any order; n <= 2^22 gives 5e-10
  assert abs(s['sum'] - math.fsum(h64)) <= 1e-9 * math.fsum(h64) and abs(s['sum_sq'] - math.fsum(h64 * h64)) <= 1e-9 * math.fsum(h64 * h64)
  raw = [U._distance_stats_on(d, taus).cpu().numpy() for _ in range(2)]
  assert np.array_equal(_bits(raw[0]), _bits(raw[1])) and len(raw[0]) == L.FP_SURFDIST_STATS_TAU0 + len(taus)
  # NaN and inf are left out of everything and counted
  bad = d.clone()
  bad[[0, 4097, 10254]] = float('nan')
  bad[5000] = float('inf')
  keep = np.ones(len(h), bool)
  keep[[0, 4097, 10254, 5000]] = False
  sb = U.distance_stats(bad, taus)
  assert sb['n'] == len(h) - 4 and sb['not_finite'] == 4 and sb['max'] == float(h[keep].max())
  assert sb['within'] == [int((h64[keep] <= t).sum()) for t in taus]
  assert abs(sb['sum'] - math.fsum(h64[keep])) <= 1e-9 * math.fsum(h64[keep])
  assert U.distance_stats(d[:0]) == dict(n=0, not_finite=0, sum=0.0, sum_sq=0.0, max=0.0, within=[])
  with pytest.raises(ValueError, match='at most 8'):
    U.distance_stats(d, [0.1] * 9)


# ---- 7. the sampler ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [1, 2, 1025])
@pytest.mark.parametrize('n', [1, 1000])
def test_sampler(F, n):
  U = _U()
  v, f = O.random_soup(F, seed=20 + F)
  pts, face, info = U.sample_surface((v, f), n, seed=9, return_face=True, return_info=True)
  assert pts.is_cuda and pts.shape == (n, 3) and face.shape == (n,) and info['bary'].shape == (n, 2) and info['area_q'].shape == (F,)
  p, face_h, bary, aq = pts.cpu().numpy(), face.cpu().numpy(), info['bary'].cpu().numpy(), info['area_q'].cpu().numpy()
  assert np.abs(aq - O.area_q(v, f)).max() <= 1 and abs(int(aq.sum()) - (1 << 40)) <= F
  assert np.array_equal(face_h, O.sample_faces(aq, n))                 # the integer rule on the DEVICE's own table
  assert np.array_equal(_bits(bary), _bits(O.sample_bary(n, 9)))
  extent = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)))
  assert np.abs(p - O.sample_points(v, f, face_h, bary)).max() <= 8 * EPS * extent
  again = U.sample_surface((v, f), n, seed=9, return_face=True, return_info=True)
  assert np.array_equal(_bits(p), _bits(again[0].cpu().numpy())) and np.array_equal(face_h, again[1].cpu().numpy())
  other = U.sample_surface((v, f), n, seed=10, return_info=True)
  assert not np.array_equal(bary, other[1]['bary'].cpu().numpy())


def test_sampler_refuses_a_mesh_without_area_and_skips_bad_faces():
  U, L = _U(), _lib()
  v = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
  with pytest.raises(L.FoundationPoseAmdError, match='total area'):
    U.sample_surface((v, [[0, 1, 2], [3, 3, 3]]), 10)
  pts, face, info = U.sample_surface((_dev(v), _dev(np.array([[0, 1, 9], [0, 1, 2], [0, 1, 3], [-1, 0, 1]], np.int32))), 50, return_face=True, return_info=True)
  assert (face == 2).all() and info['area_q'].tolist() == [0, 0, 1 << 40, 0]
  p = pts.cpu().numpy()
  assert (p[:, 2] == 0).all() and (p[:, :2] >= 0).all() and (p[:, :2].sum(1) <= 2).all()


# ---- 8. mesh_distance ----------------------------------------------------------------------------------------------------------------------
def test_mesh_distance(soup):
  U = _U()
  v, f = O.icosphere(1, radius=0.05)
  same = U.mesh_distance((v, f), (v, f), n_samples=0)
  assert same['hausdorff'] == 0.0 and same['chamfer'] == 0.0 and same['a_to_b'] == dict(n=len(v), mean=0.0, rms=0.0, max=0.0)
  assert same['precision'] == [1.0] * 3 and same['recall'] == [1.0] * 3 and same['fscore'] == [1.0] * 3
  sampled = U.mesh_distance((v, f), (v, f), n_samples=3000)
  tol = TOL_C * EPS * float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)))
  assert sampled['a_to_b']['n'] == len(v) + 3000 and 0 <= sampled['hausdorff'] <= tol and 0 <= sampled['chamfer'] <= 2 * tol
  cv, cf = O.lattice_cube()
  shifted = cv + np.array([0.25, 0, 0], np.float32)
  r = U.mesh_distance((cv, cf), (shifted, cf), n_samples=2000, taus=(0.5, 0.125))
  assert r['hausdorff'] == 0.25 and r['a_to_b']['max'] == 0.25 and r['b_to_a']['max'] == 0.25
  assert r['precision'][0] == 1.0 and r['recall'][0] == 1.0 and r['fscore'][0] == 1.0
  assert 0 < r['precision'][1] < 1 and 0 < r['recall'][1] < 1 and 0 < r['fscore'][1] < 1
  assert abs(r['fscore'][1] - 2 * r['precision'][1] * r['recall'][1] / (r['precision'][1] + r['recall'][1])) < 1e-15
  assert r['chamfer'] == r['a_to_b']['mean'] + r['b_to_a']['mean'] and 0 < r['chamfer'] < 0.5
  assert r['a_to_b']['mean'] <= r['a_to_b']['rms'] <= r['a_to_b']['max']
  # powers of two are exact in fp32 and in the double sums: twice the size, twice the distances, bit for bit
  r2 = U.mesh_distance((2 * cv, cf), (2 * shifted, cf), n_samples=2000, taus=(1.0, 0.25))
  assert r2['chamfer'] == 2 * r['chamfer'] and r2['hausdorff'] == 0.5 and r2['precision'] == r['precision'] and r2['recall'] == r['recall']
  assert U.mesh_distance((cv, cf), (shifted, cf), n_samples=2000, taus=(0.5, 0.125)) == r
  only_samples = U.mesh_distance((cv, cf), (shifted, cf), n_samples=500, use_vertices=False, taus=())
  assert only_samples['a_to_b']['n'] == 500 and only_samples['precision'] == []
  with pytest.raises(ValueError, match='nothing to measure'):
    U.mesh_distance((cv, cf), (shifted, cf), n_samples=0, use_vertices=False)


# ---- 9. exact against the nearest-neighbour bound on a pipeline product -------------------------------------------------------------------
def test_exact_distance_is_below_the_sampled_bound_on_the_fused_mustard(mustard_views, fused):  # noqa: F811
  from scipy.spatial import cKDTree
  from tests import tsdf_oracle as TO
  src = mustard_views[1]['mesh']
  q = np.asarray(fused.vertices[:2000], np.float32)
  d = _U().point_mesh_distance(q, mesh=src)
  sv = np.asarray(src.vertices, np.float64)
  nn, _ = cKDTree(TO.surface_samples(sv, src.faces)).query(q.astype(np.float64))
  scale = float(np.linalg.norm(np.maximum(sv.max(0), q.max(0)) - np.minimum(sv.min(0), q.min(0))))
  tol = TOL_C * EPS * scale
  print(f'exact: mean {d.mean():.6f} max {d.max():.6f}; nearest of 400 000 samples: mean {nn.mean():.6f} max {nn.max():.6f}; '
        f'largest excess of the exact one {float((d - nn).max()):.3e} (tol {tol:.3e})')
  assert np.isfinite(d).all() and (d <= nn + tol).all()
  assert d.mean() < nn.mean()
