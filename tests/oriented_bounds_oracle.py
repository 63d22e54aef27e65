"""Yardsticks of the oriented-box tests.  Nothing here imports foundationpose_amd.bounds.

box_extents_f32: fp_box_extents' rule (include/foundationpose_amd.h) restated in numpy op for op - np.float32 products and sums in the
stated order, fmin / fmax from +inf / -inf, the fp32 volume, the same total order for the winner.

calipers_min_volume: an independent float64 yardstick of the candidate class "one face flush with a hull face": for every distinct hull
normal, the minimum-area enclosing rectangle of the projected points' 2-D hull - one side lies along a hull edge (Freeman & Shapira
1975), the widths taken by rotating calipers over the edges - times the height along the normal."""
import numpy as np

F32 = np.float32


def box_extents_f32(points, frames, chunk=4096):
  """-> dict(index, lo (3,), hi (3,), volume, all_lohi (C,6), all_volume (C)), all float32; index -1 and NaNs when no volume is >= 0."""
  p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
  r = np.ascontiguousarray(frames, dtype=F32).reshape(-1, 3, 3)
  x, y, z = p[:, 0], p[:, 1], p[:, 2]
  C = len(r)
  lohi = np.empty((C, 6), dtype=F32)
  step = max(1, chunk * 1024 // max(len(p), 1))
  for c0 in range(0, C, step):
    rc = r[c0:c0 + step]
    with np.errstate(invalid='ignore', over='ignore'):
      q = ((rc[:, :, 0, None] * x) + (rc[:, :, 1, None] * y)) + (rc[:, :, 2, None] * z)    # (c,3,n), every operation rounds to fp32
    assert q.dtype == F32
    lohi[c0:c0 + step, :3] = np.fmin.reduce(q, axis=2, initial=F32(np.inf))
    lohi[c0:c0 + step, 3:] = np.fmax.reduce(q, axis=2, initial=F32(-np.inf))
  with np.errstate(invalid='ignore', over='ignore'):
    e = lohi[:, 3:] - lohi[:, :3]
    vol = (e[:, 0] * e[:, 1]) * e[:, 2]
  assert vol.dtype == F32
  with np.errstate(invalid='ignore'):
    ok = vol >= 0
  if ok.any():
    index = int(np.flatnonzero(ok & (vol == vol[ok].min()))[0])          # the smaller volume, then the lower index
    win_lohi, win_vol = lohi[index], vol[index]
  else:
    index, win_lohi, win_vol = -1, np.full(6, np.nan, dtype=F32), F32(np.nan)
  return dict(index=index, lo=win_lohi[:3].copy(), hi=win_lohi[3:].copy(), volume=win_vol, all_lohi=lohi, all_volume=vol)


def winner_f32(points, frames):
  return box_extents_f32(points, frames)['index']


def _min_area_rectangle(xy):
  """Minimum-area enclosing rectangle of 2-D points by rotating calipers on their convex hull: (area, unit direction of one side)."""
  from scipy.spatial import ConvexHull
  H = xy[ConvexHull(xy).vertices]                                        # counter-clockwise
  n = len(H)
  E = np.roll(H, -1, axis=0) - H
  E = E / np.linalg.norm(E, axis=1, keepdims=True)
  # calipers: for edge k the support points in the directions +u, +v, -u advance monotonically round the hull
  dot = lambda k, i: E[k] @ H[i % n]
  perp = lambda k, i: -E[k, 1] * H[i % n, 0] + E[k, 0] * H[i % n, 1]
  right = top = left = 1
  best = (np.inf, None)
  for k in range(n):
    while dot(k, right + 1) > dot(k, right):
      right += 1
    top = max(top, right)
    while perp(k, top + 1) > perp(k, top):
      top += 1
    left = max(left, top)
    while dot(k, left + 1) < dot(k, left):
      left += 1
    area = (dot(k, right) - dot(k, left)) * (perp(k, top) - perp(k, k))
    if area < best[0]:
      best = (area, E[k])
  return best


def _min_area_rectangle_brute(xy):
  """The same by trying every hull edge against every hull vertex (O(h^2), vectorised): what the calipers must agree with."""
  from scipy.spatial import ConvexHull
  H = xy[ConvexHull(xy).vertices]
  E = np.roll(H, -1, axis=0) - H
  E = E / np.linalg.norm(E, axis=1, keepdims=True)
  a = H @ E.T
  b = H @ np.stack([-E[:, 1], E[:, 0]], axis=1).T
  area = np.ptp(a, axis=0) * np.ptp(b, axis=0)
  return float(area.min()), E[int(area.argmin())]


def calipers_min_volume(points, decimals=9, brute=False):
  """(volume, rows (3,3) of the best frame, number of distinct normals) in float64 over every distinct normal of the hull of `points`."""
  from scipy.spatial import ConvexHull
  p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
  hull = ConvexHull(p)
  P = p[hull.vertices]
  nrm = hull.equations[:, :3]
  nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
  nrm = nrm[np.unique(np.round(nrm, decimals), axis=0, return_index=True)[1]]
  rect = _min_area_rectangle_brute if brute else _min_area_rectangle
  best = (np.inf, None)
  for m in nrm:
    a = np.eye(3)[np.argmin(np.abs(m))]
    a = a - (a @ m) * m
    a /= np.linalg.norm(a)
    b = np.cross(m, a)
    area, d = rect(np.stack([P @ a, P @ b], axis=1))
    vol = area * np.ptp(P @ m)
    if vol < best[0]:
      u = d[0] * a + d[1] * b
      best = (float(vol), np.stack([u, np.cross(m, u), m]))
  return best[0], best[1], len(nrm)


def box_volume_f64(points, rows):
  q = np.asarray(points, dtype=np.float64).reshape(-1, 3) @ np.asarray(rows, dtype=np.float64).T
  return float(np.prod(q.max(axis=0) - q.min(axis=0)))


def rotvec_matrix(rv):
  """Rodrigues: the rotation matrix of a rotation vector."""
  rv = np.asarray(rv, dtype=np.float64)
  t = np.linalg.norm(rv)
  k = rv / t
  K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
  return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


ROTVEC = (0.3, -0.7, 0.5)
SHIFT = np.array([0.4, -0.25, 0.9])
BOX = np.array([0.05, 0.12, 0.2])


def rotated_box(n_inside=500, seed=0):
  """The 0.05 x 0.12 x 0.2 m box: its 8 corners and n_inside interior points, turned by ROTVEC and shifted."""
  corners = np.array([[(-1, 1)[(k >> 2) & 1], (-1, 1)[(k >> 1) & 1], (-1, 1)[k & 1]] for k in range(8)], dtype=np.float64) * BOX / 2
  inside = (np.random.RandomState(seed).rand(n_inside, 3) - 0.5) * BOX * 0.98
  return np.concatenate([corners, inside]) @ rotvec_matrix(ROTVEC).T + SHIFT


def gaussian_cloud(n=2000, seed=1):
  return np.random.RandomState(seed).randn(n, 3) * np.array([0.11, 0.06, 0.03])
