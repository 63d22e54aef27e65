"""Masks from depth (fp_plane_score, fp_plane_moments, fp_depth_segment_count / _write) restated in numpy and scipy, operation for
operation as include/foundationpose_amd.h states the rules: fp32 arithmetic in the written order (every numpy operation on float32
arrays rounds once; nothing is contracted), the components by scipy.sparse.csgraph.connected_components on the explicit pixel graph,
numbered by their lowest pixel index, the statistics as the same 2^-20 m integers, the moments in the device's summation order (that of
tests/gn_sums_oracle.py with 10 terms).  Also the analytic table-top scene of the tests.  Imports nothing of the product."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

F = np.float32
TERMS = 10
STATS = 16


def points(depth, K):
  """(x, y, z) float32 maps: p = ((((float)col - cx) / fx) d, (((float)row - cy) / fy) d, d)."""
  d = np.asarray(depth, dtype=F)
  H, W = d.shape
  fx, fy, cx, cy = F(K[0][0]), F(K[1][1]), F(K[0][2]), F(K[1][2])
  col, row = np.arange(W, dtype=F)[None, :], np.arange(H, dtype=F)[:, None]
  x, y = ((col - cx) / fx) * d, ((row - cy) / fy) * d
  assert x.dtype == F and y.dtype == F
  return x, y, d


def ok_map(depth, mask=None, zfar=100):
  d = np.asarray(depth, dtype=F)
  ok = (d >= F(0.001)) & (d < F(zfar))
  return ok if mask is None else ok & (np.asarray(mask) != 0)


def height(plane, x, y, z):
  """((n.x p.x + n.y p.y) + n.z p.z) + dd in fp32; plane is cast to fp32 as the device does."""
  g = np.asarray(plane, dtype=np.float64).astype(F)
  return ((g[0] * x + g[1] * y) + g[2] * z) + g[3]


def plane_score(depth, K, triplets, tol, mask=None, zfar=100):
  """(planes (n_hyp,4) float32, counts (n_hyp,) int32, best)."""
  x, y, z = points(depth, K)
  ok = ok_map(depth, mask, zfar)
  xf, yf, zf, okf = x.ravel(), y.ravel(), z.ravel(), ok.ravel()
  hw = xf.size
  trip = np.asarray(triplets, dtype=np.int64).reshape(-1, 3)
  planes, counts = np.zeros((len(trip), 4), F), np.zeros((len(trip),), np.int32)
  for h, (i, j, k) in enumerate(trip):
    if not (0 <= i < hw and 0 <= j < hw and 0 <= k < hw) or i == j or i == k or j == k or not (okf[i] and okf[j] and okf[k]):
      continue
    pi, pj, pk = (np.array([xf[t], yf[t], zf[t]], dtype=F) for t in (i, j, k))
    u, w = pj - pi, pk - pi
    m = np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]], dtype=F)
    l2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
    if not l2 > 0:
      continue
    n = m / np.sqrt(l2)
    dd = -((n[0] * pi[0] + n[1] * pi[1]) + n[2] * pi[2])
    if dd < 0:
      n, dd = -n, -dd
    assert n.dtype == F and np.asarray(dd).dtype == F
    planes[h] = (n[0], n[1], n[2], dd)
    counts[h] = int((okf & (np.abs(((n[0] * xf + n[1] * yf) + n[2] * zf) + dd) < F(tol))).sum())
  best = -1 if len(counts) == 0 or counts.max() == 0 else int(np.argmax(counts))      # argmax: the first of equals
  return planes, counts, best


def plane_moments(depth, K, plane, tol, mask=None, zfar=100, threads=256, pix=4):
  """The 10 float64 sums n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz in the device's order."""
  x, y, z = points(depth, K)
  inl = (ok_map(depth, mask, zfar) & (np.abs(height(plane, x, y, z)) < F(tol))).ravel()
  X, Y, Z = (np.where(inl, a.ravel().astype(np.float64), 0.0) for a in (x, y, z))
  rows = np.stack([np.where(inl, 1.0, 0.0), X, Y, Z, X * X, X * Y, X * Z, Y * Y, Y * Z, Z * Z], -1)
  tile = threads * pix
  n_tiles = -(-len(rows) // tile)
  t = np.zeros((n_tiles * tile, TERMS))
  t[:len(rows)] = rows
  t = t.reshape(n_tiles, pix, threads, TERMS)
  v = np.zeros((n_tiles, threads, TERMS))
  for q in range(pix):                      # a lane adds q = 0 .. pix - 1 in order from +0.0
    v = v + t[:, q]
  v = v.reshape(n_tiles, threads // 64, 64, TERMS)
  lane = np.arange(64)
  for o in (32, 16, 8, 4, 2, 1):            # the butterfly over each wave
    v = v + v[:, :, lane ^ o]
  red = v[:, :, 0]
  slot = red[:, 0]
  for w in range(1, threads // 64):         # the waves in order
    slot = slot + red[:, w]
  s = np.zeros(TERMS)
  for k in range(n_tiles):                  # the tiles in order from 0.0
    s = s + slot[k]
  return s


def plane_from_moments(s):
  """The least-squares plane of the sums in float64, the camera on the positive side: (plane (4,), eigenvalues ascending)."""
  s = np.asarray(s, dtype=np.float64)
  mean = s[1:4] / s[0]
  second = np.array([[s[4], s[5], s[6]], [s[5], s[7], s[8]], [s[6], s[8], s[9]]]) / s[0]
  w, v = np.linalg.eigh(second - np.outer(mean, mean))
  n = v[:, 0]
  dd = -float(n @ mean)
  if dd < 0:
    n, dd = -n, -dd
  return np.array([n[0], n[1], n[2], dd]), w


def fit_plane(depth, K, mask=None, tol=0.005, n_hyp=512, seed=0, refits=2, zfar=100):
  H, W = np.asarray(depth).shape
  trip = np.random.RandomState(seed).randint(0, H * W, (n_hyp, 3))
  planes, counts, best = plane_score(depth, K, trip, tol, mask, zfar)
  assert best >= 0
  plane = planes[best].astype(np.float64)
  for _ in range(refits):
    s = plane_moments(depth, K, plane, tol, mask, zfar)
    if s[0] >= 3:
      plane = plane_from_moments(s)[0]
  return plane


def q(x):
  """(long long)rintf(min(max(x 1048576.f, -2^34), 2^34))"""
  return np.rint(np.clip(np.asarray(x, dtype=F) * F(1048576.0), F(-2.0 ** 34), F(2.0 ** 34))).astype(np.int64)


def foreground(depth, K, plane, h_min, h_max, mask=None, zfar=100):
  x, y, z = points(depth, K)
  h = height(plane, x, y, z)
  return ok_map(depth, mask, zfar) & (h >= F(h_min)) & (h <= F(h_max))


def pixel_graph(depth, fg, max_jump):
  """The (H W, H W) sparse graph: an edge between two 4-neighbours that are both foreground with fabsf(d_a - d_b) <= max_jump."""
  d = np.asarray(depth, dtype=F)
  H, W = d.shape
  idx = np.arange(H * W).reshape(H, W)
  mj = F(max_jump)
  with np.errstate(invalid='ignore'):
    eh = fg[:, 1:] & fg[:, :-1] & (np.abs(d[:, 1:] - d[:, :-1]) <= mj)
    ev = fg[1:, :] & fg[:-1, :] & (np.abs(d[1:, :] - d[:-1, :]) <= mj)
  a = np.concatenate([idx[:, 1:][eh], idx[1:, :][ev]])
  b = np.concatenate([idx[:, :-1][eh], idx[:-1, :][ev]])
  return sp.coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(H * W, H * W)).tocsr()


def segment(depth, K, plane, h_min=0.01, h_max=0.5, max_jump=0.01, min_pixels=200, mask=None, zfar=100):
  """(labels (H,W) int32, rows (kept, 16) int64, components): the rule of fp_depth_segment_count / _write for one view."""
  d = np.asarray(depth, dtype=F)
  H, W = d.shape
  fg = foreground(d, K, plane, h_min, h_max, mask, zfar)
  _, comp = connected_components(pixel_graph(d, fg, max_jump), directed=False)
  fgf = fg.ravel()
  labels = np.zeros(H * W, np.int32)
  rows = []
  x, y, z = points(d, K)
  qx, qy, qz, qh = q(x).ravel(), q(y).ravel(), q(z).ravel(), q(height(plane, x, y, z)).ravel()
  members = {}
  for p in np.nonzero(fgf)[0]:            # ascending: a component's first member is its lowest pixel
    members.setdefault(comp[p], []).append(p)
  comps = sorted(members.values(), key=lambda m: m[0])
  number = 0
  for m in comps:
    if len(m) < min_pixels:
      continue
    number += 1
    m = np.asarray(m)
    labels[m] = number
    r, c = m // W, m % W
    rows.append([len(m), r.min(), r.max(), c.min(), c.max(), qx[m].sum(), qy[m].sum(), qz[m].sum(), qx[m].min(), qy[m].min(), qz[m].min(),
                 qx[m].max(), qy[m].max(), qz[m].max(), qh[m].max(), m[0]])
  return labels.reshape(H, W), np.asarray(rows, dtype=np.int64).reshape(-1, STATS), len(comps)


def analytic_table(angle_deg, H=72, W=96, radii=(0.05, 0.04, 0.06)):
  """The tests' scene, ray-cast in float64: a table with normal (0, -cos a, -sin a) through p0 = (0, 0.05, 0.8) and three spheres (of
  radius 5, 4 and 6 cm) resting on it.  Returns dict(depth (H,W) float32, K, plane (4,) float64 with the camera on the positive side,
  gt (H,W) int32: 0 the table, 1 .. 3 the spheres, cam_in_ob (4,4): the camera in the frame of the table - origin p0, axes (1,0,0),
  (0, -sin a, cos a) and the normal - in which the spheres do not depend on the angle: scenes of different angles are views of ONE
  rigid scene)."""
  K = np.array([[90.0, 0, 47.5], [0, 90.0, 35.5], [0, 0, 1]])
  a = np.deg2rad(angle_deg)
  n = np.array([0.0, -np.cos(a), -np.sin(a)])
  p0 = np.array([0.0, 0.05, 0.8])
  dd = -float(n @ p0)
  e1, e2 = np.array([1.0, 0, 0]), np.array([0.0, -np.sin(a), np.cos(a)])
  feet = [(-0.13, 0.0), (0.0, 0.03), (0.14, -0.02)]
  col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
  ray = np.stack([(col - K[0, 2]) / K[0, 0], (row - K[1, 2]) / K[1, 1], np.ones_like(col)], -1)      # z = 1: the ray parameter is the depth
  with np.errstate(divide='ignore', invalid='ignore'):
    t = -dd / (ray @ n)
  best = np.where(np.isfinite(t) & (t > 0), t, np.inf)
  gt = np.zeros((H, W), np.int32)
  for s, ((u, w), rad) in enumerate(zip(feet, radii)):
    c = p0 + u * e1 + w * e2 + rad * n
    A, B, C = (ray * ray).sum(-1), ray @ c, c @ c - rad * rad
    disc = B * B - A * C
    with np.errstate(invalid='ignore'):
      ts = (B - np.sqrt(disc)) / A
    hit = (disc > 0) & (ts > 0) & (ts < best)
    best = np.where(hit, ts, best)
    gt[hit] = s + 1
  depth = np.where(np.isfinite(best), best, 0.0).astype(F)
  ob_in_cam = np.eye(4)
  ob_in_cam[:3, 0], ob_in_cam[:3, 1], ob_in_cam[:3, 2], ob_in_cam[:3, 3] = e1, e2, n, p0
  return dict(depth=depth, K=K, plane=np.array([n[0], n[1], n[2], dd]), gt=gt, cam_in_ob=np.linalg.inv(ob_in_cam))
