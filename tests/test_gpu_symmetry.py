"""GPU: fp_symmetry_residuals (csrc/surface_distance.hip) and Utils.symmetry_residuals / find_symmetries on top of it.

The kernel against fp_point_mesh_distance, bit for bit (its optional outputs d_q and d_dist exist for that), its statistics against the
same numbers computed on the host from d_dist, exact lattice cases, and the float64 restatement tests/symmetry_oracle.py; the search on
analytic meshes whose groups are known, placed by an arbitrary rotation and an off-origin translation, at the tolerances whose margins
tests/test_symmetry_host.py asserts in float64.

Shapes: Tq = FP_SURFDIST_TILE queries of a workgroup, C = FP_SURFDIST_CHUNK face records of an LDS chunk.  n in {1, Tq-1, Tq, Tq+1} with
T = 3 at F = C+1 (tiles that hold three transforms, a transform boundary one before, on and one after a tile boundary), T = 1 and T = 7 at
n = Tq+1, F in {1, C-1, C, 2C+5} at n = Tq+1 (T = 3): prefixes of the seeded triangle soup of tests/test_gpu_surface_distance.py under
seeded random rigid transforms."""
import math

import numpy as np
import pytest
import torch

from tests import surface_distance_oracle as SD
from tests import symmetry_oracle as O
from tests.test_gpu_tsdf import MVOXEL, fused, mustard_views  # noqa: F401  (fixtures: the 12 fused mustard views)

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
# |d_dev - d_64| <= TOL_C 2^-24 scale, scale = the bounding-box diagonal of the transformed points and the mesh.  d_64 is the float64
# restatement with q = R p + t formed in float64 from the fp32 inputs, so the bound covers the fp32 rounding of q (three fma per
# coordinate) as well as the distance's own.  Measured, not guessed: the largest |d_dev - d_64| / (2^-24 scale) over the shapes below on an
# MI355X is TOL_C_OBSERVED = 0.641 (n = Tq+1, T = 1, F = C+1); TOL_C is 4 x that, as in tests/test_gpu_surface_distance.py.
TOL_C_OBSERVED = 0.641
TOL_C = 4 * TOL_C_OBSERVED
STEP = 1.0                       # angle_step_deg of the searches below


def _lib():
  from foundationpose_amd import _lib
  return _lib


def _U():
  from foundationpose_amd import Utils
  return Utils


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _dev(a):
  return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _random_rigid(n, seed):
  rng = np.random.default_rng(seed)
  out = []
  for _ in range(n):
    axis = rng.normal(size=3)
    t = O.rotation(axis, float(rng.uniform(0, 360)))
    t[:3, 3] = rng.uniform(-0.5, 0.5, 3)
    out.append(t)
  return np.stack(out)


@pytest.fixture(scope='module')
def soup():
  L = _lib()
  Tq, C = L.FP_SURFDIST_TILE, L.FP_SURFDIST_CHUNK
  v, f = SD.random_soup(2 * C + 5, seed=11)
  pts = np.random.default_rng(12).uniform(-1, 1, (Tq + 1, 3)).astype(np.float32)
  tfs = _random_rigid(7, seed=13)
  tfs[1] = np.eye(4)                                           # the identity among them: q = p exactly
  pts[:40] = v[f[:40, 0]]                                      # some samples on a vertex: distance exactly 0 under the identity
  return dict(Tq=Tq, C=C, v=v, f=f, pts=pts, tfs=tfs, ref={})


def _shapes(Tq, C):
  """(n, T, F)"""
  return [(n, 3, C + 1) for n in (1, Tq - 1, Tq, Tq + 1)] + [(Tq + 1, 1, C + 1), (Tq + 1, 7, C + 1)] + [(Tq + 1, 3, F) for F in (1, C - 1, C, 2 * C + 5)]


def _run(soup, n, T, F, taus=(), first=0):
  U = _U()
  stats, q, dist = U._symmetry_residuals_on(_dev(soup['pts'][:n]), U._tfs_f32_on(soup['tfs'][first:first + T], 'cuda'), _dev(soup['v']),
                                            _dev(soup['f'][:F]), taus, want_q=True, want_dist=True)
  return stats.cpu().numpy(), q, dist


# ---- 1. the distance of a query is fp_point_mesh_distance's, bit for bit; the statistics are those of d_dist ----------------------------------
def test_distances_are_those_of_point_mesh_distance_and_statistics_those_of_the_distances(soup):
  U, L = _U(), _lib()
  taus = [0.0, 0.05, 0.2, 10.0]
  for n, T, F in _shapes(soup['Tq'], soup['C']):
    stats, q, dist = _run(soup, n, T, F, taus)
    assert stats.shape == (T, L.FP_SURFDIST_STATS_TAU0 + len(taus)) and q.shape == (T * n, 3) and dist.shape == (T * n,)
    want = U.point_mesh_distance(q, vertices=_dev(soup['v']), faces=_dev(soup['f'][:F]))
    d = dist.cpu().numpy()
    assert np.array_equal(_bits(d), _bits(want.cpu().numpy())), (n, T, F)
    # the same bits when a transform is submitted alone: not a function of T, of the tile or of the neighbours
    for k in range(T):
      s1, q1, d1 = _run(soup, n, 1, F, taus, first=k)
      assert np.array_equal(_bits(q1.cpu().numpy()), _bits(q.cpu().numpy()[k * n:(k + 1) * n])), (n, T, F, k)
      assert np.array_equal(_bits(d1.cpu().numpy()), _bits(d[k * n:(k + 1) * n])), (n, T, F, k)
      assert np.array_equal(_bits(s1[0, [L.FP_SURFDIST_STATS_COUNT, L.FP_SURFDIST_STATS_MAX]]),
                            _bits(stats[k, [L.FP_SURFDIST_STATS_COUNT, L.FP_SURFDIST_STATS_MAX]]))
    # the identity leaves the points as they are
    if T >= 2:
      assert np.array_equal(_bits(q.cpu().numpy()[n:2 * n]), _bits(soup['pts'][:n]))
      assert (d[n:min(2 * n, n + 40)] == 0).all() or F < 40
    # per transform: count, maximum, not-finite count and the counts within tau exactly; the sums to 1e-12 of math.fsum
    for k in range(T):
      cnt, s, s2, mx, bad, le = O.stats_from_distances(d[k * n:(k + 1) * n], taus)
      row = stats[k]
      assert row[L.FP_SURFDIST_STATS_COUNT] == cnt == n and row[L.FP_SURFDIST_STATS_NOT_FINITE] == bad == 0, (n, T, F, k)
      assert row[L.FP_SURFDIST_STATS_MAX] == mx and row[L.FP_SURFDIST_STATS_TAU0:].tolist() == le, (n, T, F, k)
      assert abs(row[L.FP_SURFDIST_STATS_SUM] - s) <= 1e-12 * s and abs(row[L.FP_SURFDIST_STATS_SUM_SQ] - s2) <= 1e-12 * s2, (n, T, F, k)
    again = _run(soup, n, T, F, taus)[0]
    assert np.array_equal(_bits(again), _bits(stats)), (n, T, F)


def test_bad_values_are_counted_per_transform(soup):
  L = _lib()
  U = _U()
  n, F = soup['Tq'] - 1, soup['C'] + 1
  pts = soup['pts'][:n].copy()
  pts[[3, 700]] = np.nan
  tfs = soup['tfs'][:3].copy()
  tfs[2, 0, 3] = np.inf                                        # a transform that is not finite: every query of it is bad
  stats, q, dist = U._symmetry_residuals_on(_dev(pts), U._tfs_f32_on(tfs, 'cuda'), _dev(soup['v']), _dev(soup['f'][:F]), [10.0], True, True)
  stats, d = stats.cpu().numpy(), dist.cpu().numpy().reshape(3, n)
  assert stats[:, L.FP_SURFDIST_STATS_NOT_FINITE].tolist() == [2, 2, n] and stats[:, L.FP_SURFDIST_STATS_COUNT].tolist() == [n - 2, n - 2, 0]
  assert np.isnan(d[:2, [3, 700]]).all() and np.isnan(d[2]).all() and np.isfinite(np.delete(d[:2], [3, 700], axis=1)).all()
  assert stats[2, L.FP_SURFDIST_STATS_MAX] == 0 and stats[2, L.FP_SURFDIST_STATS_SUM] == 0 and stats[2, L.FP_SURFDIST_STATS_TAU0] == 0
  assert stats[0, L.FP_SURFDIST_STATS_MAX] == float(np.nanmax(d[0])) and stats[0, L.FP_SURFDIST_STATS_TAU0] == n - 2


# ---- 2. exact lattice cases ------------------------------------------------------------------------------------------------------------------
def _cube_rotations(pivot):
  gens = [O.rotation((1, 0, 0), 90.0, pivot), O.rotation((0, 0, 1), 90.0, pivot)]
  group = [np.round(g) + 0.0 for g in O.closure(gens)]
  assert len(group) == 24
  return np.stack(group)


def test_lattice_cube_under_its_24_rotations_is_exactly_zero():
  """0 / +-1 matrices and integer translations about the centre (1, 1, 1) of the 0..2 cube, sample points on the half-integer lattice of
  its surface: q is exact, it lies on the surface again, and every distance is exactly 0."""
  U, L = _U(), _lib()
  v, f = SD.lattice_cube(0.0, 2.0)
  g = np.arange(5) * 0.5
  pts = np.array([[x, y, z] for x in g for y in g for z in g if min(x, y, z) == 0 or max(x, y, z) == 2], np.float32)
  tfs = _cube_rotations((1, 1, 1))
  stats, q, dist = U._symmetry_residuals_on(_dev(pts), U._tfs_f32_on(tfs, 'cuda'), _dev(v), _dev(f), [0.0], True, True)
  assert (dist == 0).all() and len(pts) == 98
  s = stats.cpu().numpy()
  assert (s[:, [L.FP_SURFDIST_STATS_SUM, L.FP_SURFDIST_STATS_SUM_SQ, L.FP_SURFDIST_STATS_MAX, L.FP_SURFDIST_STATS_NOT_FINITE]] == 0).all()
  assert (s[:, L.FP_SURFDIST_STATS_COUNT] == 98).all() and (s[:, L.FP_SURFDIST_STATS_TAU0] == 98).all()
  want = np.einsum('tij,nj->tni', tfs[:, :3, :3], pts.astype(np.float64)) + tfs[:, None, :3, 3]
  assert np.array_equal(q.cpu().numpy().reshape(24, 98, 3), want.astype(np.float32))
  r = U.symmetry_residuals(vertices=v, faces=f, tfs=tfs, n_samples=512)
  assert r['max'].max() <= 4 * EPS * math.sqrt(12.0) and (r['n'] == 512).all()      # arbitrary samples: fp32 rounding of q alone


def test_lattice_box_under_a_quarter_turn_has_the_analytic_maximum():
  """the box [0,1] x [0,2] x [0,4] turned by 90 degrees about z, (x, y, z) -> (-y, x, z): exact integers"""
  U, L = _U(), _lib()
  v, f = SD.lattice_cube(0.0, 1.0)
  v = v * np.array([1, 2, 4], np.float32)
  pts = np.array([[1, 2, 0], [1, 0, 4], [0, 2, 2], [1, 2, 4], [0.5, 1, 0], [0, 0, 0], [1, 1, 3]], np.float32)
  want = np.array([2, 0, 2, 2, 1, 0, 1], np.float32)           # (-2,1,0) (0,1,4) (-2,0,2) (-2,1,4) (-1,.5,0) (0,0,0) (-1,1,3)
  tfs = np.stack([np.eye(4), O.rotation((0, 0, 1), 90.0).round() + 0.0])
  stats, q, dist = U._symmetry_residuals_on(_dev(pts), U._tfs_f32_on(tfs, 'cuda'), _dev(v), _dev(f), [0.0, 1.0], True, True)
  d, s = dist.cpu().numpy().reshape(2, -1), stats.cpu().numpy()
  assert (d[0] == 0).all() and np.array_equal(d[1], want)
  assert s[1, L.FP_SURFDIST_STATS_MAX] == 2 and s[1, L.FP_SURFDIST_STATS_SUM] == 8 and s[1, L.FP_SURFDIST_STATS_SUM_SQ] == 14
  assert s[1, L.FP_SURFDIST_STATS_TAU0:].tolist() == [2, 4] and s[0, L.FP_SURFDIST_STATS_MAX] == 0


# ---- 3. against float64 ----------------------------------------------------------------------------------------------------------------------
def test_boundary_shapes_against_float64(soup):
  """every shape of section 1 at F = C+1 (the T = 7 reference holds them all), and the first transform of the other F"""
  Tq, C = soup['Tq'], soup['C']
  worst, failures = 0.0, []
  ref = {}
  for n, T, F in _shapes(Tq, C):
    _, q, dist = _run(soup, n, T, F)
    d = dist.cpu().numpy().astype(np.float64).reshape(T, n)
    rows = T if F == C + 1 else 1
    if F not in ref:                                            # computed once per F, never changed
      ref[F] = O.residual_distances(soup['pts'], soup['tfs'][:7 if F == C + 1 else 1], soup['v'], soup['f'][:F])
    d64 = ref[F][:rows, :n]
    qh = q.cpu().numpy().astype(np.float64)
    scale = float(np.linalg.norm(np.maximum(qh.max(0), soup['v'].max(0)) - np.minimum(qh.min(0), soup['v'].min(0))))
    ratio = float(np.abs(d[:rows] - d64).max() / (EPS * scale))
    print(f'n {n} T {T} F {F}: |d_dev - d_64| {ratio:.3f} x 2^-24 scale {scale:.3f}')
    worst = max(worst, ratio)
    if ratio > TOL_C:
      failures.append((n, T, F, ratio))
  print(f'largest ratio {worst:.3f}; TOL_C_OBSERVED {TOL_C_OBSERVED}, TOL_C {TOL_C}')
  assert not failures, failures


# ---- 4. find_symmetries on analytic meshes -------------------------------------------------------------------------------------------------------
# one final refinement step of a 2-fold axis is STEP / 64; the rotation it stands for is then off by twice that.  The fp32 residual
# bound (a few 2^-24 of a size of order 1 over a lever of order 1) adds below 1e-4 degrees.
AXIS_TOL_DEG = STEP / 64 + 1e-4


def _mesh(name):
  from foundationpose_amd.synthetic import SimpleMesh
  v, f, group, cont_axis, tol = O.shapes()[name]
  return SimpleMesh(O.placed(v).astype(np.float32), f), group, cont_axis, tol


@pytest.fixture(scope='module')
def found():
  cache = {}

  def get(name):
    if name not in cache:
      mesh, group, cont_axis, tol = _mesh(name)
      cache[name] = (_U().find_symmetries(mesh, tol=tol, angle_step_deg=STEP), mesh, group, cont_axis, tol)
    return cache[name]
  return get


@pytest.mark.parametrize('name,order', [('box123', 4), ('prism113', 8), ('prism5', 10), ('prism6', 12), ('prism7', 14), ('tetrahedron', 1)])
def test_discrete_groups(found, name, order):
  info, mesh, group, _, tol = found(name)
  sym = info['symmetry_tfs']
  want = O.conjugated(group)
  assert len(want) == order and sym.shape == (order, 4, 4) and sym.dtype == np.float64 and np.array_equal(sym[0], np.eye(4)), len(sym)
  worst = O.match_one_to_one(list(sym), want)
  assert worst is not None and worst <= 2 * AXIS_TOL_DEG, worst
  assert (info['max'] <= tol).all() and info['closed'] and info['symmetries_continuous'] == [] and info['continuous_axes'] == []
  assert len(info['symmetries_discrete']) == order - 1 and info['tol'] == tol and info['n_candidates'] >= 1752
  c = info['centroid']
  assert np.abs(np.einsum('sij,j->si', sym[:, :3, :3], c) + sym[:, :3, 3] - c).max() <= 1e-12      # the pivot is fixed
  assert np.abs(c - O.surface_moments(np.asarray(mesh.vertices, np.float64), mesh.faces)[1]).max() <= 1e-12
  for m, s in zip(info['symmetries_discrete'], sym[1:]):
    m = np.array(m).reshape(4, 4)
    assert np.array_equal(m[:3, :3], s[:3, :3]) and np.allclose(m[:3, 3], 1000.0 * s[:3, 3], rtol=0, atol=1e-9)
  # 2-fold axes: within one final refinement step of the analytic ones
  for s in sym[1:]:
    if abs(O.angle_between(s, np.eye(4)) - 180.0) < 0.1:
      axis = np.linalg.eigh(0.5 * (s[:3, :3] + s[:3, :3].T))[1][:, -1]
      errs = []
      for g in want:
        if abs(O.angle_between(g, np.eye(4)) - 180.0) < 1e-3:
          a = np.linalg.eigh(0.5 * (g[:3, :3] + g[:3, :3].T))[1][:, -1]
          errs.append(math.degrees(math.asin(min(1.0, float(np.linalg.norm(np.cross(axis, a)))))))
      assert min(errs) <= AXIS_TOL_DEG, min(errs)


@pytest.mark.parametrize('name,n_discrete', [('lathe_asym', 0), ('lathe_sym', 1)])
def test_continuous_axis(found, name, n_discrete):
  info, mesh, group, cont_axis, tol = found(name)
  axis_want = O.PLACEMENT[:3, :3] @ np.asarray(cont_axis, np.float64)
  assert len(info['symmetries_continuous']) == 1 and len(info['continuous_axes']) == 1 and len(info['symmetries_discrete']) == n_discrete
  axis = np.array(info['symmetries_continuous'][0]['axis'])
  assert abs(np.linalg.norm(axis) - 1) <= 1e-12 and math.degrees(math.asin(min(1.0, float(np.linalg.norm(np.cross(axis, axis_want)))))) <= 1e-3
  assert np.allclose(info['symmetries_continuous'][0]['offset'], 1000.0 * info['centroid'], rtol=0, atol=1e-9)
  sym = info['symmetry_tfs']
  assert len(sym) == 72 * (1 + n_discrete) and np.array_equal(sym[0], np.eye(4)) and (info['max'] <= tol).all()
  # every element keeps the axis (up to its sign: the flips turn it over) and the pivot; the turns are 5 degrees apart
  along = np.einsum('sij,j,i->s', sym[:, :3, :3], axis, axis)
  assert (np.abs(np.abs(along) - 1) <= 1e-6).all() and int((along < 0).sum()) == 72 * n_discrete
  angles = sorted(round(O.angle_between(s, np.eye(4)), 6) for s in sym[:72])
  assert angles == sorted(round(min(a, 360.0 - a), 6) for a in np.arange(0.0, 360.0, 5.0))
  if n_discrete:
    flip = np.array(info['symmetries_discrete'][0]).reshape(4, 4)
    b = np.linalg.eigh(0.5 * (flip[:3, :3] + flip[:3, :3].T))[1][:, -1]
    assert abs(O.angle_between(flip, np.eye(4)) - 180.0) < 1e-3 and math.degrees(math.asin(min(1.0, abs(float(b @ axis_want))))) <= AXIS_TOL_DEG


# ---- 5. use --------------------------------------------------------------------------------------------------------------------------------------
def test_found_symmetries_in_use(found):
  U = _U()
  info, mesh, group, _, tol = found('prism6')
  sym = info['symmetry_tfs']
  gt = O.rotation((0.2, 0.9, -0.4), 71.0)
  gt[:3, 3] = [0.05, -0.1, 0.8]
  poses = np.stack([gt @ s for s in sym])
  e = U.pose_errors(poses, gt, mesh.vertices, symmetry_tfs=sym, metrics=('add', 'add_sym'))
  add, add_sym = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (e['add'], e['add_sym']))
  assert (add_sym <= tol).all() and add[0] <= 1e-6 and (add[1:] > 0.3).all(), (add_sym.max(), add.min())      # the prism's radius is 1
  # the same bits on a second run
  again = U.find_symmetries(mesh, tol=tol, angle_step_deg=STEP)
  assert np.array_equal(_bits(again['symmetry_tfs']), _bits(sym)) and np.array_equal(_bits(again['max']), _bits(info['max']))
  assert np.array_equal(_bits(again['mean']), _bits(info['mean']))


def test_auto_symmetries_thin_the_rotation_grid():
  from foundationpose_amd.estimater import FoundationPose
  mesh = _mesh('prism6')[0]
  mesh.vertices = np.asarray(mesh.vertices) * 0.05              # a hand-sized object, metres
  kept = {}
  for how in (None, 'auto'):
    est = FoundationPose.__new__(FoundationPose)                # the object set-up alone: no networks
    est.reset_object(mesh.vertices, mesh.vertex_normals, symmetry_tfs=how, mesh=mesh, diameter='exact')
    est.make_rotation_grid(min_n_views=40, inplane_step=60)
    kept[how] = len(est.rot_grid)
    if how == 'auto':
      assert len(est.symmetry_tfs) == 12 and est.symmetry_info['closed']
      c = est.symmetry_info['centroid']
      assert np.abs(c).max() <= 1e-6                            # found on the centred mesh
  assert 0 < kept['auto'] < kept[None], kept


def test_reconstruct_object_returns_the_symmetries_and_models_info_reads_them_back(mustard_views, fused, tmp_path):  # noqa: F811
  """the plumbing on a reconstructed mesh, at the default tol: reconstruct_object(symmetries=), write_models_info, BopModels"""
  from foundationpose_amd import bop
  from foundationpose_amd.reconstruct import reconstruct_object
  U = _U()
  kw = dict(n_samples=1024, n_coarse=256)
  mesh, info = reconstruct_object(mustard_views[0], voxel_size=MVOXEL, symmetries=kw)
  assert np.array_equal(mesh.vertices, fused.vertices) and np.array_equal(mesh.faces, fused.faces)      # the mesh as without the option
  diameter = U.mesh_diameter(model_pts=mesh.vertices)
  assert info['tol'] == U.SYMMETRY_TOL_FRACTION * diameter and np.array_equal(info['symmetry_tfs'][0], np.eye(4))
  assert (info['max'] <= info['tol']).all() and info['symmetries_continuous'] == [] and len(info['max']) == len(info['symmetry_tfs'])
  again = U.find_symmetries(mesh, **kw)
  assert np.array_equal(_bits(again['symmetry_tfs']), _bits(info['symmetry_tfs'])) and np.array_equal(_bits(again['max']), _bits(info['max']))
  given = bop.write_models_info(tmp_path / 'given', {5: mesh}, symmetries={5: info})
  auto = bop.write_models_info(tmp_path / 'auto', {5: mesh}, symmetries='auto', **kw)
  assert given == auto and bop.write_models_info(tmp_path / 'none', {5: mesh}, symmetries=None)[5].keys() == {
    'diameter', 'min_x', 'min_y', 'min_z', 'size_x', 'size_y', 'size_z'}
  models = bop.BopModels(tmp_path / 'auto')
  assert abs(models.diameter(5) - diameter) <= 1e-12 * diameter
  got = models.symmetry_tfs(5)
  assert got.shape == info['symmetry_tfs'].shape and np.abs(got - info['symmetry_tfs']).max() <= 1e-9


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------------------
def test_arguments(soup, found):
  U, L = _U(), _lib()
  ctx = L.Context.get(torch.device('cuda', torch.cuda.current_device()))
  v_d, f_d, p_d = _dev(soup['v']), _dev(soup['f']), _dev(soup['pts'])
  t_d = U._tfs_f32_on(soup['tfs'], 'cuda')
  n_terms = L.FP_SURFDIST_STATS_TAU0
  stats = torch.full((7, n_terms), 7.0, dtype=torch.float64, device='cuda')

  def call(n=5, T=7, V=len(soup['v']), F=len(soup['f']), pts=p_d, tfs=t_d, pos=v_d, faces=f_d, out=stats, n_taus=0):
    return L.lib().fp_symmetry_residuals(ctx.handle, L.ptr(pts), n, L.ptr(tfs), T, L.ptr(pos), V, L.ptr(faces), F, None, n_taus, L.ptr(out),
                                         None, None, L.stream_ptr())
  assert call(T=0) == L.FP_EINVAL and b'T 0' in L.lib().fp_last_error()
  assert call(T=-1) == L.FP_EINVAL and call(n=-1) == L.FP_EINVAL
  assert call(n=L.FP_SURFDIST_MAX_POINTS // 7 + 1) == L.FP_EINVAL
  assert call(V=0) == L.FP_EINVAL and call(F=0) == L.FP_EINVAL and call(F=L.FP_SURFDIST_MAX_FACES + 1) == L.FP_EINVAL
  assert call(pts=None) == L.FP_EINVAL and call(tfs=None) == L.FP_EINVAL and call(pos=None) == L.FP_EINVAL and call(faces=None) == L.FP_EINVAL
  assert call(out=None) == L.FP_EINVAL and call(n_taus=1) == L.FP_EINVAL and call(n_taus=L.FP_SURFDIST_MAX_TAUS + 1) == L.FP_EINVAL
  torch.cuda.synchronize()
  assert (stats == 7).all()
  assert call(n=0, pts=None) == 0                               # n = 0: zeros
  torch.cuda.synchronize()
  assert (stats == 0).all()
  with pytest.raises(ValueError, match='at most 8'):
    U.symmetry_residuals(vertices=soup['v'], faces=soup['f'], tfs=soup['tfs'], taus=[0.1] * 9)
  with pytest.raises(ValueError, match='needs tfs'):
    U.symmetry_residuals(vertices=soup['v'], faces=soup['f'])
  info, mesh, _, _, tol = found('prism6')
  with pytest.raises(ValueError, match='max_group'):
    U.find_symmetries(mesh, tol=tol, max_group=8)
  with pytest.raises(ValueError, match="'auto'"):
    from foundationpose_amd.estimater import FoundationPose
    FoundationPose.__new__(FoundationPose).reset_object(mesh.vertices, mesh.vertex_normals, symmetry_tfs='all', mesh=mesh, diameter=1.0)
