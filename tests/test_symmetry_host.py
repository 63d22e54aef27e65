"""CPU: the host side of the symmetry search (foundationpose_amd/symmetry.py, bop.write_models_info) against tests/symmetry_oracle.py, which
shares no code with it, and the margins by which the analytic shapes of tests/test_gpu_symmetry.py separate their symmetries from every
other candidate, measured with the float64 restatement of the kernel's rule."""
import json
import math

import numpy as np
import pytest

from tests import surface_distance_oracle as SD
from tests import symmetry_oracle as O

N_SAMPLES = 4096


def _sym():
  from foundationpose_amd import symmetry
  return symmetry


def test_closed_form_moments_against_dense_integration():
  S = _sym()
  for name, (v, f, _, _, _) in O.shapes().items():
    v = O.placed(v)
    area, c, cov = S.surface_moments(v, f)
    area_o, c_o, cov_o = O.surface_moments(v, f)                # edge-midpoint quadrature: exact for quadratics
    assert abs(area - area_o) <= 1e-12 * area and np.abs(c - c_o).max() <= 1e-12 and np.abs(cov - cov_o).max() <= 1e-12, name
    if len(f) > 100:
      continue
    area_n, c_n, cov_n = O.numeric_moments(v, f, n=48)          # point masses at the centroids of 48^2 pieces: error O(1 / 48^2) in cov
    assert abs(area - area_n) <= 1e-9 and np.abs(c - c_n).max() <= 1e-9, name
    assert np.abs(cov - cov_n).max() <= 2.0 * np.abs(cov).max() / 48 ** 2, name
  # eigenvectors are rows, right-handed, and diagonalise the tensor
  w, axes = S.principal_axes(cov)
  assert np.allclose(axes @ cov @ axes.T, np.diag(w), atol=1e-12) and np.isclose(np.linalg.det(axes), 1.0) and (np.diff(w) >= 0).all()


def test_candidate_counts():
  S = _sym()
  c = S.candidates(12, 1.0)
  per_axis = O.candidate_counts(12, 1.0)
  assert per_axis == (45, 359, 180)
  for j in range(3):
    assert tuple(sum(1 for x in c if x[0] == kind and x[1] == j) for kind in ('cyclic', 'grid', 'twofold')) == per_axis
  assert len(c) == 3 * sum(per_axis) == 1752
  assert len(S.candidates(6, 2.0)) == 3 * (len(O.candidate_angles(6)) + 179 + 90)
  # the cyclic angles are the oracle's, each once
  axes, pivot = np.eye(3), np.array([0.2, -0.1, 0.4])
  got = sorted(S.rotation_angle_deg(S.candidate_transform(x, axes, pivot)[:3, :3]) for x in c if x[0] == 'cyclic' and x[1] == 2)
  want = sorted(min(a, 360 - a) for a in O.candidate_angles(12))
  assert np.allclose(got, want, atol=1e-9)
  # every candidate fixes the pivot; library and oracle rotations agree
  for x in c[::37]:
    t = S.candidate_transform(x, axes, pivot)
    assert np.allclose(t[:3, :3] @ pivot + t[:3, 3], pivot, atol=1e-14)
  assert np.allclose(S.rotation_about((0.3, -0.5, 0.8), math.radians(37.0), pivot), O.rotation((0.3, -0.5, 0.8), 37.0, pivot), atol=1e-14)


def test_closure_of_generators_to_d6():
  S = _sym()
  gens = [np.eye(4), O.rotation((0, 0, 1), 60.0), O.rotation((1, 0, 0), 180.0)]
  group, closed = S.close_group(gens, same_deg=0.5)
  want = O.closure(gens[1:])
  assert closed and len(group) == len(want) == 12 and np.array_equal(group[0], np.eye(4))
  assert O.match_one_to_one(group, O.dihedral(6)) < 1e-6 and O.match_one_to_one(want, O.dihedral(6)) < 1e-6
  with pytest.raises(ValueError, match='max_group'):
    S.close_group(gens, same_deg=0.5, max_group=8)
  # modulo a continuous axis the flips of a symmetric lathe are one element
  flips = [np.eye(4)] + [O.rotation((math.cos(a), math.sin(a), 0), 180.0) for a in (0.0, 0.4, 1.1)] + [O.rotation((0, 0, 1), 77.0)]
  group, _ = S.close_group(flips, same_deg=0.5, cont_axis=np.array([0.0, 0.0, 1.0]))
  assert len(group) == 2
  # an element the verifier refuses is left out and reported
  group, closed = S.close_group(gens, same_deg=0.5, verify=lambda new: [False] * len(new))
  assert not closed and len(group) == 3


@pytest.mark.parametrize('name', list(O.shapes()))
def test_oracle_margins(name):
  """What the GPU test relies on, in float64, for every shape at its tol: each true element has max residual < tol / 10 on all 4096
  samples, and every OTHER candidate has max residual > 10 tol.  The other candidates are the cyclic rotations that are no element and the
  grid 2-fold axes further than one grid step from a true 2-fold axis (the grid points next to a true axis are not candidates for
  acceptance: they bracket the refinement, which ends within step / 64 of the axis).  The rotations by multiples of the step decide
  together - 'all pass' - so for them the margin is that of the worst one.  A maximum over a subset of the samples bounds the maximum
  from below, so the other candidates are measured on the samples furthest from the centroid alone (64 of them; 6 on the lathes, whose
  576 faces make the float64 restatement slow).  The turns of a lathe are bounded by the sagitta of its 96-gon and measured at three
  angles on every 8th sample."""
  v, f, group, cont_axis, tol = O.shapes()[name]
  v = O.placed(v).astype(np.float32)
  pts = SD.sample_surface(v, f, N_SAMPLES, seed=0)[0].astype(np.float32)
  true = O.conjugated(group)
  cont = None if cont_axis is None else O.PLACEMENT[:3, :3] @ np.asarray(cont_axis, np.float64)
  _, c, cov = O.surface_moments(v.astype(np.float64), f)
  axes = np.linalg.eigh(cov)[1].T
  if cont is not None:      # a continuous axis: the elements are those of the discrete group times a few turns, the half segment among them
    true = [O.rotation(cont, a, c) @ g for g in true for a in (1.875, 91.0)] + [O.rotation(cont, 180.0, c)]
    rmax = float(np.linalg.norm(np.cross(v.astype(np.float64) - c, cont), axis=1).max())
    assert rmax * (1 - math.cos(math.pi / 96)) < tol / 10      # the sagitta of a 96-gon bounds every turn
  worst_true = float(O.residuals(pts if cont is None else pts[::8], np.stack(true), v, f)[0].max())
  far = pts[np.argsort(-np.linalg.norm(pts.astype(np.float64) - c, axis=1), kind='stable')[:64 if cont is None else 6]]
  has_flip = len(group) > 1
  twofolds = [g for g in true if abs(O.angle_between(g, np.eye(4)) - 180.0) < 1e-3]
  others, grid = [], []
  for j in range(3):
    others += [O.rotation(axes[j], a, c) for a in O.candidate_angles(12)]
    u, w = axes[(j + 1) % 3], axes[(j + 2) % 3]
    others += [O.rotation(math.cos(math.radians(p)) * u + math.sin(math.radians(p)) * w, 180.0, c) for p in range(180)]
    grid.append([O.rotation(axes[j], float(a), c) for a in (29, 90, 133)])

  def near_true(t):
    """a true element, or a 2-fold rotation whose axis is within one grid step (1 degree) of a true 2-fold axis"""
    r = t[:3, :3]
    is_twofold = abs(O.angle_between(t, np.eye(4)) - 180.0) < 1e-3
    if cont is None:
      return any(O.angle_between(t, g) < 1e-3 for g in true) or (is_twofold and any(O.angle_between(t, g) <= 2.0 + 1e-9 for g in twofolds))
    s = float((r @ cont) @ cont)
    if abs(s - 1) < 1e-10 or (has_flip and abs(s + 1) < 1e-10):
      return True
    if not is_twofold:
      return False
    axis = np.linalg.eigh(0.5 * (r + r.T))[1][:, -1]            # R = 2 a a^T - I
    along = min(1.0, abs(float(axis @ cont)))
    return math.degrees(math.acos(along)) <= 1.0 + 1e-9 or (has_flip and math.degrees(math.asin(along)) <= 1.0 + 1e-9)

  others = [t for t in others if not near_true(t)]
  best_other = float(O.residuals(far, np.stack(others), v, f)[0].min()) if others else math.inf
  print(f'{name}: tol {tol}: true elements <= {worst_true:.3e}, {len(others)} other candidates >= {best_other:.3e}')
  assert worst_true < tol / 10
  assert best_other > 10 * tol
  for j in range(3):
    if cont is not None and abs(abs(float(axes[j] @ cont)) - 1) < 1e-9:
      continue
    assert float(O.residuals(far, np.stack(grid[j]), v, f)[0].max()) > 10 * tol


def test_models_info_round_trip(tmp_path):
  """write_models_info -> BopModels: diameter, bounds and the discrete symmetry transforms, through the mm conversion"""
  from foundationpose_amd import Utils as U
  from foundationpose_amd import bop
  from foundationpose_amd.synthetic import SimpleMesh
  v, f, group, _, _ = O.shapes()['prism6']
  v = O.placed(v) * 0.05                                        # metres
  place = O.PLACEMENT.copy()
  place[:3, 3] *= 0.05
  sym = np.stack(O.conjugated(group, place))
  S = _sym()
  disc = []
  for g in sym[1:]:
    m = g.copy()
    m[:3, 3] *= 1000.0
    disc.append([float(x) for x in m.reshape(-1)])
  info = dict(symmetry_tfs=sym, symmetries_discrete=disc, symmetries_continuous=[])
  mesh = SimpleMesh(v, f)
  diameter = float(np.linalg.norm(v[:, None] - v[None], axis=-1).max())
  bop.write_models_info(tmp_path, {3: mesh, 7: mesh}, symmetries={3: info, 7: None}, diameters={3: diameter, 7: diameter})
  raw = json.load(open(tmp_path / 'models_info.json'))
  assert sorted(raw) == ['3', '7'] and 'symmetries_discrete' not in raw['7'] and len(raw['3']['symmetries_discrete']) == 11
  models = bop.BopModels(tmp_path)
  assert models.obj_ids == [3, 7]
  assert abs(models.diameter(3) - diameter) <= 1e-12
  e = models.info(3)
  lo, hi = v.min(0) * 1e3, v.max(0) * 1e3
  assert np.allclose([e['min_x'], e['min_y'], e['min_z']], lo, atol=1e-9) and np.allclose([e['size_x'], e['size_y'], e['size_z']], hi - lo, atol=1e-9)
  got = models.symmetry_tfs(3)
  assert got.shape == sym.shape and np.abs(got - sym).max() <= 1e-9
  assert np.array_equal(models.symmetry_tfs(7), np.eye(4)[None])
  assert S.models_info_entry(v, diameter, None).keys() == {'diameter', 'min_x', 'min_y', 'min_z', 'size_x', 'size_y', 'size_z'}
  # a continuous axis along z through Utils.symmetry_tfs_from_info: identity, then the turns about z every 5 degrees with the offset as
  # translation, as the reference's helper reads it
  cont = dict(symmetries_continuous=[dict(axis=[0.0, 0.0, 1.0], offset=[0.0, 0.0, 0.0])], symmetries_discrete=[])
  entry = S.models_info_entry(v, diameter, cont)
  tfs = U.symmetry_tfs_from_info(entry)
  assert tfs.shape == (73, 4, 4)
  for k in range(72):
    assert np.allclose(tfs[1 + k], O.rotation((0, 0, 1), 5.0 * k), atol=1e-12)
