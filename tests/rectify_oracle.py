"""fp_remap (csrc/rectify.hip) and the plan building of foundationpose_amd/rectify.py restated in numpy, rule for rule as
include/foundationpose_amd.h states it: plans in float64 rounded to fp32 once, the per-pixel map in fp32 numpy with the header's order of
operations and parentheses (every numpy float32 operation is rounded once, as every device operation is without contraction), the
integer blend of colour mode and the nearest-neighbour rule of depth mode.  The GPU has to match it bit for bit.  A checker: never
imported by the product."""
import numpy as np

F = np.float32
NAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]


def dist8(dist):
  d = np.zeros(0) if dist is None else np.asarray(dist, np.float64).reshape(-1)
  assert d.size in (0, 4, 5, 8), d.size
  out = np.zeros(8)
  out[:d.size] = d
  return out


def distort64(xy, K, dist):
  """float64: normalised rays (..., 2) -> raw pixels (..., 2)."""
  k1, k2, p1, p2, k3, k4, k5, k6 = dist8(dist)
  x, y = np.asarray(xy, np.float64)[..., 0], np.asarray(xy, np.float64)[..., 1]
  r2 = x * x + y * y
  radial = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
  xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
  yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
  return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], -1)


def r2_max(dist, step=1.0 / 1024.0, steps=8 * 1024, halvings=60):
  """The fixed scan of monotonic_r2_max, with the slope of r radial(r^2) taken from the product rule written out."""
  k1, k2, _, _, k3, k4, k5, k6 = dist8(dist)

  def slope(r):
    s = r * r
    num, den = 1 + k1 * s + k2 * s ** 2 + k3 * s ** 3, 1 + k4 * s + k5 * s ** 2 + k6 * s ** 3
    if den <= 0:
      return -np.inf
    dnum, dden = (k1 + 2 * k2 * s + 3 * k3 * s ** 2) * 2 * r, (k4 + 2 * k5 * s + 3 * k6 * s ** 2) * 2 * r      # d / dr
    return num / den + r * (dnum * den - num * dden) / den ** 2

  if not any((k1, k2, k3, k4, k5, k6)):
    return np.inf
  for i in range(1, steps + 1):
    if slope(i * step) <= 0:
      lo, hi = (i - 1) * step, i * step
      for _ in range(halvings):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if slope(mid) <= 0 else (mid, hi)
      return hi * hi
  return np.inf


def plan(K_new, rot, K_raw, dist, src_size, dst_size):
  """A plan as a dict of fp32 values: k_new, k_raw (fx, fy, cx, cy), rot (9, new -> raw), dist (8), r2_max, src (H, W), dst (H, W)."""
  k4 = lambda K: np.array([K[0][0], K[1][1], K[0][2], K[1][2]], np.float64).astype(F)
  d = dist8(dist)
  return dict(k_new=k4(K_new), rot=np.asarray(rot, np.float64).reshape(9).astype(F), k_raw=k4(K_raw), dist=d.astype(F), r2_max=F(r2_max(d)),
              src=tuple(src_size), dst=tuple(dst_size), K_new=np.asarray(K_new, np.float64), rot64=np.asarray(rot, np.float64),
              K_raw=np.asarray(K_raw, np.float64), dist64=d)


def undistort_plan(K, dist, size, K_new=None, size_new=None):
  return plan(K if K_new is None else K_new, np.eye(3), K, dist, size, size if size_new is None else size_new)


def rectify_stereo(K1, dist1, K2, dist2, R, T, size, K_new=None, size_new=None):
  """dict(K_new, size_new, baseline, R1, R2, left, right) by the closed-form rule; x2 = R x1 + T."""
  K1, K2, R, T = (np.asarray(a, np.float64) for a in (K1, K2, R, T))
  unit = lambda v: v / np.sqrt((v * v).sum())
  c2 = -(R.T @ T)
  assert c2[0] > 0
  e1 = unit(c2)
  e2 = unit(np.cross(unit(np.array([0, 0, 1.0]) + R.T[:, 2]), e1))
  e3 = np.cross(e1, e2)
  R1 = np.stack([e1, e2, e3])
  R2 = R1 @ R.T
  if K_new is None:
    f = (K1[1, 1] + K2[1, 1]) / 2
    K_new = np.array([[f, 0, (K1[0, 2] + K2[0, 2]) / 2], [0, f, (K1[1, 2] + K2[1, 2]) / 2], [0, 0, 1.0]])
  size_new = tuple(size if size_new is None else size_new)
  return dict(K_new=np.asarray(K_new, np.float64), size_new=size_new, baseline=float(np.sqrt((c2 * c2).sum())), R1=R1, R2=R2,
              left=plan(K_new, R1.T, K1, dist1, size, size_new), right=plan(K_new, R2.T, K2, dist2, size, size_new))


def pixel_map(p):
  """Step 1 in fp32: (u, v (H_dst, W_dst) float32, the quiet NaN where the ray is refused; Z float32; ray bool)."""
  Hd, Wd = p['dst']
  row, col = np.meshgrid(np.arange(Hd, dtype=F), np.arange(Wd, dtype=F), indexing='ij')
  fxn, fyn, cxn, cyn = p['k_new']
  r = p['rot']
  k1, k2, p1, p2, k3, k4, k5, k6 = p['dist']
  one, two = F(1), F(2)
  with np.errstate(all='ignore'):
    x, y = (col - cxn) / fxn, (row - cyn) / fyn
    X, Y, Z = ((r[3 * a] * x + r[3 * a + 1] * y) + r[3 * a + 2] * one for a in range(3))
    ray = Z > 0
    xr, yr = X / Z, Y / Z
    r2 = xr * xr + yr * yr
    ray &= r2 < p['r2_max']
    radial = (one + r2 * (k1 + r2 * (k2 + r2 * k3))) / (one + r2 * (k4 + r2 * (k5 + r2 * k6)))
    xy2 = two * (xr * yr)
    xd = (xr * radial + p1 * xy2) + p2 * (r2 + two * (xr * xr))
    yd = (yr * radial + p1 * (r2 + two * (yr * yr))) + p2 * xy2
    u, v = p['k_raw'][0] * xd + p['k_raw'][2], p['k_raw'][1] * yd + p['k_raw'][3]
  for a in (x, Z, r2, radial, xd, u):
    assert a.dtype == np.float32
  return np.where(ray, u, NAN).astype(F), np.where(ray, v, NAN).astype(F), Z.astype(F), ray


def pixel_map64(p):
  """The same map in float64 from the float64 plan values: distort64 of the rotated ray of every destination pixel."""
  Hd, Wd = p['dst']
  row, col = np.meshgrid(np.arange(Hd, dtype=np.float64), np.arange(Wd, dtype=np.float64), indexing='ij')
  K = p['K_new']
  d = np.stack([(col - K[0, 2]) / K[0, 0], (row - K[1, 2]) / K[1, 1], np.ones_like(col)], -1) @ p['rot64'].T
  return distort64(d[..., :2] / d[..., 2:], p['K_raw'], p['dist64']), d[..., 2]


def remap_colour(img, p):
  """uint8 (H,W) or (H,W,3) -> dict(out, valid uint8, map float32 (H_dst, W_dst, 2))."""
  img = np.asarray(img)
  assert img.dtype == np.uint8 and img.shape[:2] == p['src'], (img.dtype, img.shape, p['src'])
  Hs, Ws = p['src']
  u, v, _, ray = pixel_map(p)
  with np.errstate(invalid='ignore'):
    fu, fv = np.floor(u * F(256) + F(0.5)), np.floor(v * F(256) + F(0.5))
    valid = ray & (fu >= 0) & (fu <= F((Ws - 1) * 256)) & (fv >= 0) & (fv <= F((Hs - 1) * 256))
  qu, qv = np.where(valid, fu, 0).astype(np.int64), np.where(valid, fv, 0).astype(np.int64)
  u0, a, v0, b = qu >> 8, qu & 255, qv >> 8, qv & 255
  u1, v1 = np.minimum(u0 + 1, Ws - 1), np.minimum(v0 + 1, Hs - 1)
  src = img.astype(np.int64).reshape(Hs, Ws, -1)
  w = lambda k: k[..., None]
  acc = w((256 - a) * (256 - b)) * src[v0, u0] + w(a * (256 - b)) * src[v0, u1] + w((256 - a) * b) * src[v1, u0] + w(a * b) * src[v1, u1]
  out = np.where(w(valid), (acc + 32768) >> 16, 0).astype(np.uint8)
  return dict(out=out.reshape(p['dst'] + img.shape[2:]), valid=valid.astype(np.uint8), map=np.stack([u, v], -1))


def remap_depth(depth, p, zfar=np.inf):
  """float32 (H,W) -> dict(out float32, valid uint8, map, Z)."""
  depth = np.asarray(depth)
  assert depth.dtype == np.float32 and depth.shape == p['src']
  Hs, Ws = p['src']
  u, v, Z, ray = pixel_map(p)
  with np.errstate(invalid='ignore'):
    cf, rf = np.floor(u + F(0.5)), np.floor(v + F(0.5))
    valid = ray & (cf >= 0) & (cf <= F(Ws - 1)) & (rf >= 0) & (rf <= F(Hs - 1))
    d = depth[np.where(valid, rf, 0).astype(np.int64), np.where(valid, cf, 0).astype(np.int64)]
    ok = valid & (d >= F(0.001)) & (d < F(zfar))
    out = np.where(ok, d / Z, F(0)).astype(F)
  return dict(out=out, valid=valid.astype(np.uint8), map=np.stack([u, v], -1), Z=Z)


def undistort64(uv, K, dist, iterations=40):
  """float64: raw pixels -> normalised rays, by fixed-point steps on the distorted normalised coordinates."""
  k1, k2, p1, p2, k3, k4, k5, k6 = dist8(dist)
  uv = np.asarray(uv, np.float64)
  xd, yd = (uv[..., 0] - K[0, 2]) / K[0, 0], (uv[..., 1] - K[1, 2]) / K[1, 1]
  x, y = xd, yd
  for _ in range(iterations):
    r2 = x * x + y * y
    radial = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
    x, y = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / radial, (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / radial
  return np.stack([x, y], -1)


def rodrigues(rvec):
  rvec = np.asarray(rvec, np.float64)
  th = np.sqrt((rvec * rvec).sum())
  if th == 0:
    return np.eye(3)
  k = rvec / th
  Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
  return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def dots(seed, cell):
  """A procedural random-dot texture as a function: texture(s, t) -> float64 grey in 0 .. 255 for plane coordinates in metres, bilinear
  between hashed random values on a lattice of `cell` metres (it has no edge)."""
  def value(i, j):
    h = (i.astype(np.int64) * 73856093) ^ (j.astype(np.int64) * 19349663) ^ (seed * 83492791)
    h = (h ^ (h >> 13)) * 1274126177 & 0xffffffff
    return ((h ^ (h >> 16)) & 255).astype(np.float64)

  def texture(s, t):
    s, t = np.asarray(s, np.float64) / cell, np.asarray(t, np.float64) / cell
    i, j = np.floor(s), np.floor(t)
    a, b = s - i, t - j
    return (1 - a) * (1 - b) * value(i, j) + a * (1 - b) * value(i + 1, j) + (1 - a) * b * value(i, j + 1) + a * b * value(i + 1, j + 1)
  return texture


def raw_plane_scene(H=48, W=176, seed=0):
  """The analytic scene of the end-to-end tests: the plane z = 0.8 + 0.1 x (left camera frame, metres) carrying a random-dot texture,
  seen by two RAW cameras - both distorted, the right one 0.1 m to the right, 4 mm off in y, 1 mm in z and rotated by the rotation
  vector (0.025, -0.01, 0.02) (1.9 degrees).  Every raw pixel is synthesised exactly in float64: undistort64 -> ray -> plane -> texture;
  no warp is involved.  Returns dict(left, right uint8 (H,W); K1, dist1, K2, dist2, R, T (x2 = R x1 + T); plane (n, off) with n.X = off)."""
  K1 = np.array([[160.0, 0, 88.5], [0, 161.0, 23.0], [0, 0, 1]])
  K2 = np.array([[158.5, 0, 86.0], [0, 159.0, 25.5], [0, 0, 1]])
  dist1, dist2 = np.array([-0.18, 0.04, 1.0e-3, -5.0e-4, 0.0]), np.array([-0.15, 0.02, -8.0e-4, 6.0e-4, 0.01])
  Q, c2 = rodrigues([0.025, -0.01, 0.02]), np.array([0.1, 0.004, 0.001])      # orientation and centre of the right camera in the left frame
  R, T = Q.T, -Q.T @ c2
  n, off = np.array([-0.1, 0.0, 1.0]), 0.8
  tex = dots(seed, 0.008)
  row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
  images = []
  for K, dist, Rc, c in ((K1, dist1, np.eye(3), np.zeros(3)), (K2, dist2, Q, c2)):      # Rc: camera -> left frame
    xy = undistort64(np.stack([col, row], -1), K, dist)
    d = np.concatenate([xy, np.ones_like(xy[..., :1])], -1) @ Rc.T
    t = (off - n @ c) / (d @ n)
    P = c + t[..., None] * d
    images.append(np.clip(np.floor(tex(P[..., 0], P[..., 1]) + 0.5), 0, 255).astype(np.uint8))
  return dict(left=images[0], right=images[1], K1=K1, dist1=dist1, K2=K2, dist2=dist2, R=R, T=T, plane=(n, off))


def plane_depth(K, rot, size, plane):
  """z along the optical axis of the plane at every pixel of a pinhole camera K whose frame maps into the left frame by `rot` (centre 0)."""
  H, W = size
  row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
  d = np.stack([(col - K[0, 2]) / K[0, 0], (row - K[1, 2]) / K[1, 1], np.ones_like(col)], -1) @ np.asarray(rot).T
  return plane[1] / (d @ plane[0])


def end_to_end(scene, max_disparity=64):
  """The CPU result of stereo_depth(left, right, rectify=rect) and of stereo_depth(left, right, K1, baseline) on the raw pair, with the
  two figures of each: dict(rect, depth, raw_depth, valid_share, median_error, raw_valid_share, raw_median_error).  share: valid pixels
  among those with x >= max_disparity; error: the median over the valid ones of |disparity - f b / z| in pixels."""
  from tests import stereo_oracle as SO
  s = scene
  rect = rectify_stereo(s['K1'], s['dist1'], s['K2'], s['dist2'], s['R'], s['T'], s['left'].shape)
  l, r = remap_colour(s['left'], rect['left'])['out'], remap_colour(s['right'], rect['right'])['out']
  f, b = float(rect['K_new'][0, 0]), rect['baseline']
  depth = SO.sgm(l, r, max_disparity=max_disparity, fx=f, baseline=b)['depth']
  raw_depth = SO.sgm(s['left'], s['right'], max_disparity=max_disparity, fx=float(s['K1'][0, 0]), baseline=b)['depth']
  out = dict(rect=rect, depth=depth, raw_depth=raw_depth)
  out['valid_share'], out['median_error'] = figures(depth, f, b, plane_depth(rect['K_new'], rect['R1'].T, depth.shape, s['plane']), max_disparity)
  out['raw_valid_share'], out['raw_median_error'] = figures(raw_depth, float(s['K1'][0, 0]), b,
                                                            plane_depth(s['K1'], np.eye(3), raw_depth.shape, s['plane']), max_disparity)
  return out


def figures(depth, f, b, z_true, max_disparity):
  fb = float(np.float32(f * b))
  keep = np.zeros(depth.shape, bool)
  keep[:, max_disparity:] = True
  valid = keep & (depth > 0)
  err = np.abs(fb / depth[valid].astype(np.float64) - f * b / z_true[valid])
  return float(valid.sum() / keep.sum()), float(np.median(err)) if err.size else float('inf')


SIZES = (((37, 53), (37, 53)), ((64, 200), (64, 200)), ((37, 53), (45, 61)), ((64, 200), (50, 170)))      # (size, size_new)


def case_arguments(src, dst):
  """The plans of the tests for a source and a destination size, as arguments for plan() or the product's RemapPlan: name -> (K_new, rot,
  K_raw, dist, src, dst).  mild: every coefficient of the five-term model; barrel: k1 = -0.4 with a new camera of half the focal length, so
  that the map leaves the source on all four sides and the corners cross r2_max; rational: k4..k6 != 0; rect_left / rect_right: the two
  plans of a rectification with a 3 degree relative rotation."""
  (Hs, Ws), (Hd, Wd) = src, dst
  f = 0.9 * Ws
  K = np.array([[f, 0, Ws / 2 - 0.3], [0, 1.02 * f, Hs / 2 + 0.4], [0, 0, 1]])
  Kn = np.array([[f, 0, Wd / 2 - 0.3], [0, 1.02 * f, Hd / 2 + 0.4], [0, 0, 1]])
  Kwide = np.array([[0.5 * f, 0, Wd / 2 + 0.2], [0, 0.5 * f, Hd / 2 - 0.1], [0, 0, 1]])
  out = dict(mild=(Kn, np.eye(3), K, [-0.05, 0.01, 5e-4, -3e-4, 0.002], src, dst),
             barrel=(Kwide, np.eye(3), K, [-0.4, 0, 0, 0], src, dst),
             rational=(Kn, np.eye(3), K, [0.1, -0.02, 2e-4, 1e-4, 0.003, 0.05, -0.01, 0.002], src, dst))
  K2 = np.array([[0.98 * f, 0, Ws / 2 + 1.1], [0, 0.99 * f, Hs / 2 - 0.7], [0, 0, 1]])
  Q = rodrigues(np.array([0.6, -0.5, 0.62]) / np.sqrt(0.6 ** 2 + 0.5 ** 2 + 0.62 ** 2) * np.deg2rad(3.0))
  c2 = np.array([0.1, 0.003, -0.002])
  out['rectification'] = (K, [-0.05, 0.01, 5e-4, -3e-4, 0.002], K2, [-0.04, 0.008, -2e-4, 3e-4], Q.T, -Q.T @ c2, src, None, dst)
  return out


def case_plans(src, dst):
  """name -> oracle plan, the rectification as rect_left and rect_right."""
  out = {}
  for name, a in case_arguments(src, dst).items():
    if name == 'rectification':
      r = rectify_stereo(*a)
      out['rect_left'], out['rect_right'] = r['left'], r['right']
    else:
      out[name] = plan(*a)
  return out
