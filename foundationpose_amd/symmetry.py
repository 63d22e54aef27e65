"""The host side of Utils.find_symmetries, in float64 numpy: the surface moments of a mesh, the candidate rotations, the search over them,
the closure of what was accepted, and the models_info.json form of the result.  Nothing here touches the device: every residual comes
from the `residuals(tfs, n)` callable the search is given (Utils passes fp_symmetry_residuals), so tests/symmetry_oracle.py can run the
same search on a float64 restatement of the kernel.

Proper rotations only: a reflection is not a pose.  A rotational symmetry of a surface fixes its area-weighted centroid and commutes with
its covariance tensor, so an axis of order >= 3 is an eigenvector of that tensor and a 2-fold axis is an eigenvector or lies in the plane
of two equal eigenvalues: the candidates are rotations about the three eigenvectors and 2-fold rotations about axes in the three planes
they span - whatever the eigenvalues are, so no eigenvalue-gap threshold is needed."""
import math

import numpy as np


def surface_moments(vertices, faces):
  """(area, centroid (3,), covariance (3,3)) of the SURFACE of a triangle mesh, area-weighted, in closed form per triangle:
  int x dA = A (v0 + v1 + v2) / 3 and int x x^T dA = A / 12 (sum v v^T + (sum v)(sum v)^T) about the origin, the second shifted to the
  centroid.  No samples."""
  v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
  f = np.asarray(faces).reshape(-1, 3)
  tri = v[f]                                                  # (F,3,3)
  area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
  total = float(area.sum())
  if not (total > 0 and math.isfinite(total)):
    raise ValueError(f'the surface has area {total}: it must be positive and finite')
  s = tri.sum(axis=1)                                         # (F,3)
  centroid = (area[:, None] * s).sum(axis=0) / (3.0 * total)
  second = (area[:, None, None] / 12.0 * (np.einsum('fki,fkj->fij', tri, tri) + s[:, :, None] * s[:, None, :])).sum(axis=0) / total
  return total, centroid, second - np.outer(centroid, centroid)


def principal_axes(cov):
  """(eigenvalues (3,) ascending, axes (3,3) with the eigenvectors as ROWS) of a covariance tensor; each axis has its component of
  largest magnitude positive and the third is the cross product of the first two, so the frame is right-handed and the same on every
  run."""
  w, q = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
  axes = q.T.copy()
  for a in axes[:2]:
    if a[np.argmax(np.abs(a))] < 0:
      a *= -1.0
  axes[2] = np.cross(axes[0], axes[1])
  return w, axes


def rotation_about(axis, angle, pivot):
  """4x4 float64: the rotation by `angle` (radians) about the line through `pivot` along `axis` (Rodrigues)."""
  a = np.asarray(axis, dtype=np.float64)
  a = a / np.linalg.norm(a)
  k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
  r = np.eye(3) + math.sin(angle) * k + (1.0 - math.cos(angle)) * (k @ k)
  t = np.eye(4)
  t[:3, :3] = r
  t[:3, 3] = np.asarray(pivot, dtype=np.float64) - r @ np.asarray(pivot, dtype=np.float64)
  return t


def twofold_axis(axes, j, phi_deg):
  """b(phi) = cos phi u + sin phi v in the plane perpendicular to axes[j]; u, v the other two eigenvectors in cyclic order"""
  u, v = axes[(j + 1) % 3], axes[(j + 2) % 3]
  p = math.radians(phi_deg)
  return math.cos(p) * u + math.sin(p) * v


def candidates(max_order=12, angle_step_deg=1.0):
  """The candidate list, the same for every mesh: per eigenvector j = 0, 1, 2
    ('cyclic', j, m, k)   the rotation by 2 pi m / k about it, k = 2 .. max_order, 0 < m < k, m / k in lowest terms (each angle once)
    ('grid', j, i)        the rotation by i angle_step_deg, 0 < i angle_step_deg < 360: all of them pass on a continuous axis
    ('twofold', j, i)     the rotation by pi about b(i angle_step_deg), 0 <= i angle_step_deg < 180
  in that order."""
  n_grid = int(math.ceil(360.0 / angle_step_deg - 1e-9))
  n_two = int(math.ceil(180.0 / angle_step_deg - 1e-9))
  out = []
  for j in range(3):
    out += [('cyclic', j, m, k) for k in range(2, max_order + 1) for m in range(1, k) if math.gcd(m, k) == 1]
    out += [('grid', j, i) for i in range(1, n_grid)]
    out += [('twofold', j, i) for i in range(n_two)]
  return out


def candidate_transform(c, axes, pivot, angle_step_deg=1.0):
  if c[0] == 'cyclic':
    return rotation_about(axes[c[1]], 2.0 * math.pi * c[2] / c[3], pivot)
  if c[0] == 'grid':
    return rotation_about(axes[c[1]], math.radians(c[2] * angle_step_deg), pivot)
  return rotation_about(twofold_axis(axes, c[1], c[2] * angle_step_deg), math.pi, pivot)


def rotation_angle_deg(r):
  """the angle of a 3x3 rotation, degrees"""
  return math.degrees(math.acos(min(1.0, max(-1.0, (float(np.trace(r)) - 1.0) / 2.0))))


def _separation_deg(g, h, cont_axis):
  """How far apart two elements are: the angle of g^-1 h; with a continuous axis a, elements that differ by a rotation about a are the
  same, and the angle between g a and h a is taken instead."""
  if cont_axis is None:
    return rotation_angle_deg(g[:3, :3].T @ h[:3, :3])
  c = float(np.dot(g[:3, :3] @ cont_axis, h[:3, :3] @ cont_axis))
  return math.degrees(math.acos(min(1.0, max(-1.0, c))))


def close_group(elements, same_deg, max_group=128, cont_axis=None, verify=None):
  """The closure of `elements` (4x4, the identity first) under composition.  Two elements closer than same_deg (_separation_deg) are one:
  the first found stays.  verify(list of 4x4) -> list of bool is asked about every batch of new elements and those it refuses are left
  out.  More than max_group elements: ValueError.  Returns (list of 4x4, closed: nothing was refused)."""
  group = []
  for e in elements:
    if all(_separation_deg(g, e, cont_axis) >= same_deg for g in group):
      group.append(np.asarray(e, dtype=np.float64))
  closed, refused, start = True, [], 0
  while True:
    if len(group) > max_group:
      raise ValueError(f'find_symmetries: more than max_group = {max_group} elements: the object is (nearly) a sphere or tol is too wide')
    new = []
    for i, g in enumerate(group):
      for j, h in enumerate(group):
        if i < start and j < start:
          continue
        p = g @ h
        if all(_separation_deg(x, p, cont_axis) >= same_deg for x in group + new + refused):
          new.append(p)
          if len(group) + len(new) > max_group:
            raise ValueError(f'find_symmetries: more than max_group = {max_group} elements: the object is (nearly) a sphere or tol is too wide')
    if not new:
      return group, closed
    ok = [True] * len(new) if verify is None else verify(new)
    start = len(group)
    for p, good in zip(new, ok):
      if good:
        group.append(p)
      else:
        refused.append(p)
        closed = False
    if not any(ok):
      return group, closed


def _local_minima(values):
  """indices i of a circular sequence with values[i] <= both neighbours and < at least one of them (a flat sequence has none)"""
  v = np.asarray(values, dtype=np.float64)
  prev, nxt = np.roll(v, 1), np.roll(v, -1)
  return [int(i) for i in np.flatnonzero((v <= prev) & (v <= nxt) & ((v < prev) | (v < nxt)))]


def find_symmetries(vertices, faces, residuals, tol, max_order=12, angle_step_deg=1.0, n_samples=4096, n_coarse=512, rot_angle_discrete=5,
                    max_group=128):
  """The search of Utils.find_symmetries (which documents the arguments and the result).  residuals(tfs (S,4,4) float64, n) ->
  (max (S,), mean (S,)) of the distances of n surface samples under each transform to the surface."""
  v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
  _, centroid, cov = surface_moments(v, faces)
  eigenvalues, axes = principal_axes(cov)
  radius = float(np.linalg.norm(v - centroid, axis=1).max())
  step = float(angle_step_deg)
  cands = candidates(max_order, step)
  n_candidates = len(cands)

  # ---- stage 1: every candidate on n_coarse samples, one call
  tfs = np.stack([candidate_transform(c, axes, centroid, step) for c in cands])
  cmax, cmean = residuals(tfs, n_coarse)
  index = {c: i for i, c in enumerate(cands)}

  # 2-fold families: refine the local minima of the mean by halving the bracket, step / 2 .. step / 64.  An axis within one step of a true
  # one composes with it to a rotation by at most 2 steps, which moves no point further than 2 step radius: other minima are skipped.
  n_two = sum(1 for c in cands if c[0] == 'twofold' and c[1] == 0)
  reach = tol + 2.0 * math.radians(step) * radius
  flat = {}
  seeds = []                                                 # [j, phi, mean]
  for j in range(3):
    ids = [index[('twofold', j, i)] for i in range(n_two)]
    flat[j] = bool(np.all(cmax[ids] <= tol))
    if flat[j]:                                              # every axis of the plane passes (a continuous axis with flips): one seed
      i = int(np.argmin(cmean[ids]))
      seeds.append([j, i * step, float(cmean[ids[i]])])
      continue
    seeds += [[j, i * step, float(cmean[ids[i]])] for i in _local_minima(cmean[ids]) if cmax[ids[i]] <= reach]
  h = step
  for _ in range(6):
    h *= 0.5
    if not seeds:
      break
    probe = np.stack([rotation_about(twofold_axis(axes, j, phi + s * h), math.pi, centroid) for j, phi, _ in seeds for s in (-1.0, 1.0)])
    n_candidates += len(probe)
    _, pmean = residuals(probe, n_coarse)
    for k, seed in enumerate(seeds):                         # the best of centre, -h, +h; a tie stays at the centre, then at the lower angle
      phi, best = seed[1], seed[2]
      if float(pmean[2 * k]) < best:
        phi, best = seed[1] - h, float(pmean[2 * k])
      if float(pmean[2 * k + 1]) < best:
        phi, best = seed[1] + h, float(pmean[2 * k + 1])
      seed[1], seed[2] = phi, best

  # ---- stage 2: the survivors on n_samples samples, one call
  # a rotation by 2 pi m / k generates all of C_k: order k about axis j stands only when EVERY multiple of 2 pi / k passes, which keeps
  # a near miss such as 2 pi 2 / 11 beside a true 2 pi / 6 out however wide tol is
  def reduced(j, m, k):
    g = math.gcd(m, k)
    return ('cyclic', j, m // g, k // g)
  orders = [(j, k) for j in range(3) for k in range(2, max_order + 1) if all(cmax[index[reduced(j, m, k)]] <= tol for m in range(1, k))]
  survivors = [('cyclic', c) for c in sorted({reduced(j, m, k) for j, k in orders for m in range(1, k)}, key=lambda c: index[c])]
  grid_ok = {j: bool(np.all(cmax[[index[c] for c in cands if c[0] == 'grid' and c[1] == j]] <= tol)) for j in range(3)}
  survivors += [('grid', c) for c in cands if c[0] == 'grid' and grid_ok[c[1]]]
  survivors += [('twofold', (j, phi)) for j, phi, _ in seeds]
  accepted, grid_pass = [], {j: grid_ok[j] for j in range(3)}
  if survivors:
    stfs = np.stack([candidate_transform(c, axes, centroid, step) if kind != 'twofold' else
                     rotation_about(twofold_axis(axes, c[0], c[1]), math.pi, centroid) for kind, c in survivors])
    smax, smean = residuals(stfs, n_samples)
    verified = {c: bool(mx <= tol) for (kind, c), mx in zip(survivors, smax) if kind == 'cyclic'}
    orders = [(j, k) for j, k in orders if all(verified[reduced(j, m, k)] for m in range(1, k))]
    standing = {reduced(j, m, k) for j, k in orders for m in range(1, k)}
    for (kind, c), t, mx in zip(survivors, stfs, smax):
      if kind == 'grid':
        grid_pass[c[1]] = grid_pass[c[1]] and bool(mx <= tol)
      elif mx <= tol and (kind != 'cyclic' or c in standing):
        accepted.append((float(mx), kind, c, t))
  continuous = [j for j in range(3) if grid_pass[j]]
  cont = continuous[0] if continuous else None               # more than one continuous axis: a sphere; the first is reported
  cont_axis = None if cont is None else axes[cont]

  # ---- closure of the discrete elements (modulo the rotations about a continuous axis), every new element verified
  def verify(new):
    mx, _ = residuals(np.stack(new), n_samples)
    return [bool(m <= tol) for m in mx]

  # two elements closer than half a step are one; so are two that tol cannot tell apart: a turn by x moves no point further than x radius
  same = max(0.5 * min(step, float(rot_angle_discrete)), math.degrees(2.0 * tol / radius))
  accepted.sort(key=lambda a: a[0])                          # stable; of two accepted forms of one element the better one stays
  discrete, closed = close_group([np.eye(4)] + [a[3] for a in accepted], same, max_group, cont_axis, verify)

  # ---- the transforms FoundationPose takes: identity first; a continuous axis sampled every rot_angle_discrete degrees, times the rest
  if cont is None:
    sym = list(discrete)
  else:
    turns = [rotation_about(cont_axis, math.radians(d), centroid) for d in np.arange(0.0, 360.0, float(rot_angle_discrete))]
    sym = [r @ d for d in discrete for r in turns]
  sym = np.stack(sym)
  fmax, fmean = residuals(sym, n_samples)
  disc_mm = []
  for d in discrete[1:]:
    m = d.copy()
    m[:3, 3] *= 1000.0
    disc_mm.append([float(x) for x in m.reshape(-1)])
  info = dict(symmetry_tfs=sym, symmetries_discrete=disc_mm,
              symmetries_continuous=[] if cont is None else [dict(axis=[float(x) for x in cont_axis], offset=[float(x) * 1000.0 for x in centroid])],
              centroid=centroid, eigenvalues=eigenvalues, axes=axes, max=np.asarray(fmax, dtype=np.float64),
              mean=np.asarray(fmean, dtype=np.float64), n_candidates=int(n_candidates), tol=float(tol), closed=bool(closed),
              continuous_axes=[int(j) for j in continuous])
  return info


def models_info_entry(vertices, diameter, info=None):
  """One models_info.json entry, in millimetres, from vertices in metres, the exact diameter in metres and find_symmetries' info (or
  None: no symmetry keys)."""
  v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3) * 1000.0
  lo, hi = v.min(axis=0), v.max(axis=0)
  e = dict(diameter=float(diameter) * 1000.0, min_x=float(lo[0]), min_y=float(lo[1]), min_z=float(lo[2]), size_x=float(hi[0] - lo[0]),
           size_y=float(hi[1] - lo[1]), size_z=float(hi[2] - lo[2]))
  if info is not None:
    if len(info['symmetries_discrete']):
      e['symmetries_discrete'] = [list(m) for m in info['symmetries_discrete']]
    if len(info['symmetries_continuous']):
      e['symmetries_continuous'] = [dict(axis=list(c['axis']), offset=list(c['offset'])) for c in info['symmetries_continuous']]
  return e
