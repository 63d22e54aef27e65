"""Host restatement, in float64 numpy, of what Utils.find_symmetries rests on: the residual rule of fp_symmetry_residuals
(include/foundationpose_amd.h) on top of surface_distance_oracle.point_mesh_distance, the surface moments, the candidate rotations and the
closure of a set of rotations.  It shares no code with foundationpose_amd/symmetry.py: the moments come from the edge-midpoint quadrature
(exact for quadratics on a triangle) instead of the vertex formula, the rotations from a a^T + cos (I - a a^T) + sin [a]x instead of
Rodrigues' K^2 form, the closure from a fixed-point iteration over rounded keys.  It also builds the analytic meshes of the tests and
their groups."""
import math

import numpy as np

from tests import surface_distance_oracle as SD


# ---- the residual rule ------------------------------------------------------------------------------------------------------------------
def transformed(points, tfs):
  """q (T, n, 3) float64 = R p + t with the fp32 values of tfs (T,4,4 or T,3,4) and points, in float64 (the device forms it in fp32)"""
  t = np.asarray(tfs, dtype=np.float64)[:, :3, :].astype(np.float32).astype(np.float64)
  p = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
  return np.einsum('tij,nj->tni', t[:, :, :3], p) + t[:, None, :, 3]


def residual_distances(points, tfs, vertices, faces):
  """(T, n) float64: the distance of every transformed point to the mesh"""
  q = transformed(points, tfs)
  d = SD.point_mesh_distance(q.reshape(-1, 3), np.asarray(vertices, np.float32).astype(np.float64), faces)[0]
  return d.reshape(q.shape[:2])


def residuals(points, tfs, vertices, faces):
  """(max (T,), mean (T,)) over the points"""
  d = residual_distances(points, tfs, vertices, faces)
  return d.max(axis=1), d.mean(axis=1)


def stats_from_distances(d, taus=()):
  """the entries of fp_distance_stats from one row of distances, the sums by math.fsum: (count, sum, sum_sq, max, not_finite, [<= tau])"""
  d = np.asarray(d)
  fin = np.isfinite(d)
  x = d[fin].astype(np.float64)
  return (int(fin.sum()), math.fsum(x), math.fsum(x * x), float(x.max()) if len(x) else 0.0, int((~fin).sum()),
          [int((x <= float(t)).sum()) for t in taus])


# ---- moments, by the edge-midpoint rule ----------------------------------------------------------------------------------------------------
def surface_moments(vertices, faces):
  v = np.asarray(vertices, np.float64).reshape(-1, 3)
  tri = v[np.asarray(faces, np.int64).reshape(-1, 3)]
  area = 0.5 * np.sqrt((np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) ** 2).sum(1))
  mids = 0.5 * (tri + np.roll(tri, -1, axis=1))             # (F,3,3): the three edge midpoints
  total = area.sum()
  first = (area[:, None, None] / 3.0 * mids).sum((0, 1)) / total
  second = (area[:, None, None, None] / 3.0 * mids[:, :, :, None] * mids[:, :, None, :]).sum((0, 1)) / total
  return float(total), first, second - first[:, None] * first[None, :]


def numeric_moments(vertices, faces, n=64):
  """dense integration: every triangle cut into n^2 congruent ones, a point mass at each centroid"""
  v = np.asarray(vertices, np.float64).reshape(-1, 3)
  tri = v[np.asarray(faces, np.int64).reshape(-1, 3)]
  area = 0.5 * np.sqrt((np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) ** 2).sum(1))
  bary = []
  for i in range(n):
    for j in range(n - i):
      bary.append(((i + 1 / 3) / n, (j + 1 / 3) / n))
      if j < n - i - 1:
        bary.append(((i + 2 / 3) / n, (j + 2 / 3) / n))
  b = np.array(bary)
  assert len(b) == n * n
  pts = tri[:, None, 0] + b[None, :, :1] * (tri[:, None, 1] - tri[:, None, 0]) + b[None, :, 1:] * (tri[:, None, 2] - tri[:, None, 0])
  w = np.repeat(area / (n * n), n * n)
  pts = pts.reshape(-1, 3)
  c = (w[:, None] * pts).sum(0) / w.sum()
  d = pts - c
  return float(w.sum()), c, (w[:, None, None] * d[:, :, None] * d[:, None, :]).sum(0) / w.sum()


# ---- rotations, candidates, closure ---------------------------------------------------------------------------------------------------------
def rotation(axis, angle_deg, pivot=(0, 0, 0)):
  a = np.asarray(axis, np.float64)
  a = a / math.sqrt(float(a @ a))
  c, s = math.cos(math.radians(angle_deg)), math.sin(math.radians(angle_deg))
  cross = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
  r = np.outer(a, a) + c * (np.eye(3) - np.outer(a, a)) + s * cross
  out = np.eye(4)
  out[:3, :3] = r
  p = np.asarray(pivot, np.float64)
  out[:3, 3] = p - r @ p
  return out


def candidate_angles(max_order=12):
  """the distinct angles 360 m / k, k = 2 .. max_order, 0 < m < k, in degrees, ascending"""
  from fractions import Fraction
  return sorted(float(360 * f) for f in {Fraction(m, k) for k in range(2, max_order + 1) for m in range(1, k)})


def candidate_counts(max_order=12, angle_step_deg=1.0):
  """(cyclic, grid, twofold) per eigenvector"""
  return len(candidate_angles(max_order)), int(round(360 / angle_step_deg)) - 1, int(round(180 / angle_step_deg))


def angle_between(g, h):
  """the rotation angle of g^-1 h, degrees"""
  c = (np.trace(g[:3, :3].T @ h[:3, :3]) - 1) / 2
  return math.degrees(math.acos(min(1.0, max(-1.0, float(c)))))


def closure(generators, decimals=6):
  """the group generated by 4x4 matrices, as a list (identity first); elements are told apart by their entries rounded to `decimals`"""
  key = lambda m: tuple(np.round(m, decimals).reshape(-1) + 0.0)
  found = {key(np.eye(4)): np.eye(4)}
  while True:
    items = list(found.values()) + [np.asarray(g, np.float64) for g in generators]
    new = {key(a @ b): a @ b for a in items for b in items}
    if set(new) <= set(found):
      return list(found.values())
    for k, m in new.items():
      found.setdefault(k, m)
    if len(found) > 1000:
      raise ValueError('closure does not end')


def match_one_to_one(found, expected):
  """pairs every found element with its nearest expected one; returns the largest angle, or None when that is no bijection"""
  if len(found) != len(expected):
    return None
  taken, worst = set(), 0.0
  for g in found:
    d = [angle_between(g, e) + 1e3 * float(np.linalg.norm(g[:3, 3] - e[:3, 3]) > 1e30) for e in expected]
    j = int(np.argmin(d))
    if j in taken:
      return None
    taken.add(j)
    worst = max(worst, d[j])
  return worst


# ---- analytic meshes ----------------------------------------------------------------------------------------------------------------------------
def prism(n, radius=1.0, height=1.0):
  """regular n-gon prism about z, centred on the origin: caps as fans about their centres.  Its rotation group is D_n (2 n elements)
  unless the height makes it a cube."""
  ang = 2 * np.pi * np.arange(n) / n
  ring = np.stack([radius * np.cos(ang), radius * np.sin(ang)], 1)
  v = [[x, y, -height / 2] for x, y in ring] + [[x, y, height / 2] for x, y in ring] + [[0, 0, -height / 2], [0, 0, height / 2]]
  f = []
  for i in range(n):
    j = (i + 1) % n
    f += [[i, j, n + j], [i, n + j, n + i], [2 * n, j, i], [2 * n + 1, n + i, n + j]]
  return np.array(v, np.float64), np.array(f, np.int32)


def box(sx, sy, sz):
  """a box as a 4-gon prism scaled per axis: D2 for three different sides, D4 for two equal ones"""
  v, f = prism(4, radius=math.sqrt(0.5), height=1.0)
  r = rotation((0, 0, 1), 45.0)[:3, :3]
  v = v @ r.T
  return v * np.array([sx, sy, sz]), f


def lathe(profile, segments=96):
  """the surface of revolution about z of the polyline profile [(r, z), ..] (r > 0), `segments` around, closed by two fan caps"""
  prof = np.asarray(profile, np.float64)
  ang = 2 * np.pi * np.arange(segments) / segments
  v = [[r * math.cos(a), r * math.sin(a), z] for r, z in prof for a in ang]
  nr = len(prof)
  v += [[0, 0, prof[0, 1]], [0, 0, prof[-1, 1]]]
  bottom, top = nr * segments, nr * segments + 1
  f = []
  for k in range(nr - 1):
    for i in range(segments):
      j = (i + 1) % segments
      a, b, c, d = k * segments + i, k * segments + j, (k + 1) * segments + j, (k + 1) * segments + i
      f += [[a, b, c], [a, c, d]]
  for i in range(segments):
    j = (i + 1) % segments
    f += [[bottom, j, i], [top, (nr - 1) * segments + i, (nr - 1) * segments + j]]
  return np.array(v, np.float64), np.array(f, np.int32)


def tetrahedron():
  """scalene: no rotation but the identity maps it to itself"""
  v = np.array([[0, 0, 0], [1.0, 0, 0], [0.3, 1.4, 0], [0.45, 0.35, 2.1]], np.float64)
  return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)


def dihedral(n, axis=(0, 0, 1), first=(1, 0, 0)):
  """D_n about `axis`: n rotations and n 2-fold axes in the plane across it, the first along `first`, then every 180 / n degrees"""
  a, u = np.asarray(axis, np.float64), np.asarray(first, np.float64)
  w = np.cross(a, u)
  rots = [rotation(a, 360.0 * m / n) for m in range(n)]
  flips = [rotation(math.cos(math.pi * m / n) * u + math.sin(math.pi * m / n) * w, 180.0) for m in range(n)]
  return rots + flips


PLACEMENT = rotation((0.3, -0.5, 0.8), 37.0) @ np.block([[np.eye(3), np.array([[0.11], [-0.07], [0.23]])], [np.zeros((1, 3)), np.ones((1, 1))]])


def placed(vertices, placement=None):
  p = PLACEMENT if placement is None else placement
  return np.asarray(vertices, np.float64) @ p[:3, :3].T + p[:3, 3]


def conjugated(group, placement=None):
  p = PLACEMENT if placement is None else placement
  return [p @ g @ np.linalg.inv(p) for g in group]


# The shapes of tests/test_gpu_symmetry.py and tests/test_symmetry_host.py: name -> (vertices, faces, the discrete group in the shape's own
# frame, continuous axis or None, tol).  The sizes are of order 1; tol is set per shape from the margins test_symmetry_host.py asserts.
def shapes():
  lathe_asym = [(0.25, -1.5), (0.5, -0.5), (0.3, 1.5)]
  lathe_sym = [(0.3, -1.5), (0.5, 0.0), (0.3, 1.5)]
  return {
    'box123': (*box(1, 2, 3), dihedral(2), None, 1e-3),
    'prism113': (*box(1, 1, 3), dihedral(4, first=(1, 0, 0)), None, 1e-3),
    'prism5': (*prism(5, 1.0, 1.3), dihedral(5), None, 1e-3),
    'prism6': (*prism(6, 1.0, 1.3), dihedral(6), None, 1e-3),
    'prism7': (*prism(7, 1.0, 1.3), dihedral(7), None, 1e-3),
    'lathe_asym': (*lathe(lathe_asym), [np.eye(4)], (0, 0, 1), 3e-3),
    'lathe_sym': (*lathe(lathe_sym), [np.eye(4), rotation((1, 0, 0), 180.0)], (0, 0, 1), 3e-3),
    'tetrahedron': (*tetrahedron(), [np.eye(4)], None, 1e-3),
  }
