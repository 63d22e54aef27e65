"""fp_depth_reproject (csrc/reproject.hip) restated in numpy, rule for rule as include/foundationpose_amd.h states it: cameras and
transforms rounded to fp32 once, every step in fp32 numpy with the header's order of operations and parentheses (every numpy float32
operation is rounded once, as every device operation is without contraction), the z-buffer as np.minimum.at on uint64 keys over the
8 x 8 footprint offsets.  The GPU has to match it bit for bit.  Also the analytic scenes the tests share.  A checker: never imported by
the product."""
import numpy as np

F = np.float32
MAX_VIEWS, MAX_SPLAT = 8, 8
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def cam4(K):
  """fx, fy, cx, cy of a 3x3 matrix rounded to fp32 (pinhole_of)."""
  K = np.asarray(K, np.float64).reshape(3, 3)
  return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float64).astype(F)


def rigid(T):
  """(r (9), t (3)) of a 4x4 matrix rounded to fp32 (rigid_of)."""
  T = np.asarray(T, np.float64).reshape(4, 4)
  return T[:3, :3].reshape(9).astype(F), T[:3, 3].astype(F)


def rodrigues(w):
  w = np.asarray(w, np.float64)
  a = np.sqrt((w * w).sum())
  if a == 0:
    return np.eye(3)
  k = w / a
  Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
  return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


def transform(R=None, t=(0, 0, 0)):
  T = np.eye(4)
  T[:3, :3] = np.eye(3) if R is None else R
  T[:3, 3] = t
  return T


def depth_ok(d, zfar):
  return (d >= F(0.001)) & (d < F(zfar))


def _point(cam, col, row, d):
  """pinhole_point: ((col - cx) / fx d, (row - cy) / fy d, d)."""
  fx, fy, cx, cy = cam
  return (col - cx) / fx * d, (row - cy) / fy * d, d


def _apply(rt, p):
  """rigid_apply on the three rows: ((r0 x + r1 y) + r2 z) + t."""
  r, t = rt
  x, y, z = p
  return tuple(((r[3 * a] * x + r[3 * a + 1] * y) + r[3 * a + 2] * z) + t[a] for a in range(3))


def _project(cam, q):
  """project_ratio: fx (x / z) + cx, fy (y / z) + cy."""
  fx, fy, cx, cy = cam
  return fx * (q[0] / q[2]) + cx, fy * (q[1] / q[2]) + cy


def _range(e0, e1, c):
  one, half = F(1), F(0.5)
  a, b = np.ceil(np.minimum(e0, e1)), np.ceil(np.maximum(e0, e1)) - one
  pc = np.floor(c + half)
  return np.minimum(a, pc), np.maximum(b, pc), pc


def reproject(depths, Ks, T_dst_src, K_dst, size_dst, zfar=np.inf):
  """depths (V, Hs, Ws) or (n, V, Hs, Ws) float32 -> dict(depth (.., Hd, Wd) float32, source (.., Hd, Wd) int32, capped, behind): the
  last two count, over all frames, the source pixels whose footprint the cap shrank and those skipped because a corner fell behind the
  target camera."""
  depths = np.asarray(depths)
  assert depths.dtype == np.float32
  batch = depths.ndim == 4
  dd = depths if batch else depths[None]
  n, V, Hs, Ws = dd.shape
  Hd, Wd = size_dst
  Ks, Ts = np.asarray(Ks, np.float64).reshape(V, 3, 3), np.asarray(T_dst_src, np.float64).reshape(V, 4, 4)
  assert 1 <= V <= MAX_VIEWS
  dst = cam4(K_dst)
  row, col = np.meshgrid(np.arange(Hs, dtype=F), np.arange(Ws, dtype=F), indexing='ij')
  pix = np.arange(Hs * Ws, dtype=np.uint64).reshape(Hs, Ws)
  one, half = F(1), F(0.5)
  keys = np.full((n, Hd * Wd), EMPTY, np.uint64)
  capped = behind = 0
  with np.errstate(all='ignore'):
    for f in range(n):
      for s in range(V):
        cam, rt = cam4(Ks[s]), rigid(Ts[s])
        d = dd[f, s]
        ok = depth_ok(d, zfar)                                                   # 1
        q = _apply(rt, _point(cam, col, row, d))                                 # 2
        ok &= depth_ok(q[2], zfar)
        q0 = _apply(rt, _point(cam, col - half, row - half, d))                  # 3
        q1 = _apply(rt, _point(cam, col + half, row + half, d))
        front = (q0[2] > 0) & (q1[2] > 0)
        behind += int((ok & ~front).sum())
        ok &= front
        (uc, vc), (u0, v0), (u1, v1) = _project(dst, q), _project(dst, q0), _project(dst, q1)
        for a in (uc, vc, u0, v0, u1, v1):
          assert a.dtype == np.float32
          ok &= np.isfinite(a)
        x_lo, x_hi, xc = _range(u0, u1, uc)                                      # 4
        y_lo, y_hi, yc = _range(v0, v1, vc)
        ok &= np.isfinite(x_lo) & np.isfinite(x_hi) & np.isfinite(y_lo) & np.isfinite(y_hi)
        cap = ((x_hi - x_lo) + one > F(MAX_SPLAT)) | ((y_hi - y_lo) + one > F(MAX_SPLAT))      # 5
        capped += int((ok & cap).sum())
        x_lo, x_hi, y_lo, y_hi = np.where(cap, xc, x_lo), np.where(cap, xc, x_hi), np.where(cap, yc, y_lo), np.where(cap, yc, y_hi)
        x_lo, x_hi = np.maximum(x_lo, F(0)), np.minimum(x_hi, F(Wd - 1))         # 6
        y_lo, y_hi = np.maximum(y_lo, F(0)), np.minimum(y_hi, F(Hd - 1))
        ok &= (x_lo <= x_hi) & (y_lo <= y_hi)
        x0, x1, y0, y1 = (np.where(ok, a, F(0)).astype(np.int64) for a in (x_lo, x_hi, y_lo, y_hi))
        assert q[2].dtype == np.float32
        key = (np.ascontiguousarray(q[2]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(s * Hs * Ws) + pix)      # 7
        for dy in range(MAX_SPLAT):
          for dx in range(MAX_SPLAT):
            y, x = y0 + dy, x0 + dx
            m = ok & (y <= y1) & (x <= x1)
            if m.any():
              np.minimum.at(keys[f], (y * Wd + x)[m], key[m])
  hit = keys != EMPTY
  depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), F(0)).astype(F).reshape(n, Hd, Wd)
  source = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32).reshape(n, Hd, Wd)
  return dict(depth=depth if batch else depth[0], source=source if batch else source[0], capped=capped, behind=behind)


# ---- the float64 brute force: per target pixel the minimum over the source pixels whose footprint covers its centre ----

def brute_force64(depth, K_src, T, K_dst, size_dst, margin=1e-3):
  """One view (Hs, Ws) in float64 from the fp32-rounded cameras, without the cap, the clip arithmetic or a key: for every target pixel the
  nearest z (float64, not rounded) among the source pixels with min(u0, u1) <= x < max(u0, u1) (likewise y) or whose centre rounds to it, and the lowest index
  among equal z.  Returns (depth, source, excluded): `excluded` counts (target pixel, source pixel) pairs with a footprint edge within
  `margin` px of the pixel centre, or a centre within `margin` of a rounding boundary, where fp32 and float64 may decide differently."""
  Hs, Ws = depth.shape
  Hd, Wd = size_dst
  fx, fy, cx, cy = cam4(K_src).astype(np.float64)
  gx, gy, ox, oy = cam4(K_dst).astype(np.float64)
  r, t = rigid(T)
  R, t = r.astype(np.float64).reshape(3, 3), t.astype(np.float64)
  best = np.full((Hd, Wd), np.inf)
  src = np.full((Hd, Wd), -1, np.int64)
  xs, ys = np.arange(Wd, dtype=np.float64), np.arange(Hd, dtype=np.float64)
  excluded = 0

  def proj(c, r_, d):
    p = R @ np.array([(c - cx) / fx * d, (r_ - cy) / fy * d, d]) + t
    return gx * p[0] / p[2] + ox, gy * p[1] / p[2] + oy, p[2]

  for rr in range(Hs):
    for cc in range(Ws):
      d = float(depth[rr, cc])
      if not d >= 0.001:
        continue
      uc, vc, z = proj(cc, rr, d)
      u0, v0, _ = proj(cc - 0.5, rr - 0.5, d)
      u1, v1, _ = proj(cc + 0.5, rr + 0.5, d)
      ua, ub, va, vb = min(u0, u1), max(u0, u1), min(v0, v1), max(v0, v1)
      for e in (ua, ub, uc + 0.5):
        excluded += int((np.abs(xs - e) < margin).sum())
      for e in (va, vb, vc + 0.5):
        excluded += int((np.abs(ys - e) < margin).sum())
      mx = ((xs >= ua) & (xs < ub)) | (xs == np.floor(uc + 0.5))
      my = ((ys >= va) & (ys < vb)) | (ys == np.floor(vc + 0.5))
      # the rule's range is the hull of the footprint's pixels and the centre's pixel
      if mx.any() and my.any():
        xi, yi = np.nonzero(mx)[0], np.nonzero(my)[0]
        sl = (slice(yi[0], yi[-1] + 1), slice(xi[0], xi[-1] + 1))
        zf = float(z)
        better = zf < best[sl]      # source pixels come in index order: an equal depth keeps the earlier one
        best[sl] = np.where(better, zf, best[sl])
        src[sl] = np.where(better, rr * Ws + cc, src[sl])
  return np.where(np.isfinite(best), best, 0.0), src, excluded


# ---- inputs the tests share ----

def random_depth(shape, seed, lo=0.5, hi=1.5, zero_share=0.1, bad=6, zfar=None):
  """A smooth-free depth map: uniform in [lo, hi), about `zero_share` of the pixels 0, `bad` pixels NaN and, with a zfar, as many beyond it."""
  rng = np.random.default_rng(seed)
  d = rng.uniform(lo, hi, shape).astype(F)
  flat = d.reshape(-1)
  flat[rng.random(flat.size) < zero_share] = 0
  idx = rng.choice(flat.size, 2 * bad, replace=False)
  flat[idx[:bad]] = np.nan
  if zfar is not None:
    flat[idx[bad:]] = F(zfar) + F(0.25)
  return d


def scaled_K(K, sy, sx):
  K = np.array(K, np.float64)
  K[0] *= sx
  K[1] *= sy
  return K


K_SMALL = np.array([[47.7, 0, 26.2], [0, 48.6, 18.9], [0, 0, 1]])      # 37 x 53
K_WIDE = np.array([[150.3, 0, 101.2], [0, 149.1, 30.7], [0, 0, 1]])     # 64 x 200
K_MID = np.array([[60.4, 0, 31.3], [0, 61.2, 23.8], [0, 0, 1]])         # 48 x 64


def bit_cases():
  """name -> (depths, Ks, Ts, K_dst, size_dst, zfar): the cases of the bit-equality test."""
  cases = {}
  T = transform(rodrigues([0.004, -0.011, 0.006]), [0.021, -0.003, 0.004])
  cases['37x53->41x67'] = (random_depth((1, 37, 53), 1, zfar=1.6), [K_SMALL], [T], scaled_K(K_SMALL, 41 / 37, 67 / 53), (41, 67), 1.6)
  cases['64x200->30x94'] = (random_depth((1, 64, 200), 2), [K_WIDE], [T], scaled_K(K_WIDE, 30 / 64, 94 / 200), (30, 94), np.inf)
  tilt = np.deg2rad(2.0)
  Ts = [transform(rodrigues(tilt * np.array([0.2, 0.9, -0.38])), [0.05, 0.002, -0.004]),
        transform(rodrigues(tilt * np.array([-0.6, -0.7, 0.39])), [-0.04, 0.01, 0.006]),
        transform(rodrigues(tilt * np.array([0.7, 0.1, 0.7])), [0.0, -0.05, 0.01])]
  Ks = [K_MID, scaled_K(K_MID, 1.03, 0.98), scaled_K(K_MID, 0.95, 1.01)]
  for V in (1, 2, 3):
    cases[f'48x64->72x96 V={V}'] = (random_depth((V, 48, 64), 10 + V, zfar=1.6), Ks[:V], Ts[:V], scaled_K(K_MID, 1.5, 1.5), (72, 96), 1.6)
  cases['batch n=2'] = (random_depth((2, 2, 37, 53), 20), [K_SMALL, K_SMALL], Ts[:2], scaled_K(K_SMALL, 41 / 37, 67 / 53), (41, 67), np.inf)
  return cases


def grazing_case():
  """A plane seen at a grazing angle by the target camera, which stands close to it: the steep rows stretch over more than MAX_SPLAT
  target pixels (the cap), and near the target camera's own plane z = 0 some footprint corners fall behind it while the centre does not."""
  Hs, Ws = 40, 56
  K = np.array([[50.0, 0, 27.5], [0, 50.0, 19.5], [0, 0, 1]])
  depth = np.full((1, Hs, Ws), 1.0, F)
  # the target camera looks along the source's +x from inside the view cone, a few millimetres in front of the plane z = 1
  R = rodrigues(np.deg2rad(86.0) * np.array([0.0, 1.0, 0.0]))      # target z axis = source x axis turned a little towards +z
  centre = np.array([-0.295, 0.01, 0.98])
  T = transform(R.T, -R.T @ centre)
  return depth, [K], [T], np.array([[40.0, 0, 31.5], [0, 40.0, 23.5], [0, 0, 1]]), (48, 64), np.inf


# ---- the analytic scene of the end-to-end test: a sphere in front of a plane, a depth camera and a colour camera beside it ----

SPHERE_CENTRE, SPHERE_RADIUS, PLANE_Z = np.array([0.0, 0.0, 0.7]), 0.12, 1.2      # in the depth camera's frame, metres
K_DEPTH, SIZE_DEPTH = np.array([[62.0, 0, 31.5], [0, 62.0, 23.5], [0, 0, 1]]), (48, 64)
T_COLOUR_DEPTH = transform(rodrigues(np.deg2rad(1.9) * np.array([0.1, 0.97, -0.2])), [-0.05, 0.003, 0.002])      # the colour camera 5 cm to the side
COLOUR = {(72, 96): scaled_K(K_DEPTH, 1.5, 1.5) + np.array([[0, 0, 1.2], [0, 0, -0.8], [0, 0, 0]]),
          (30, 40): scaled_K(K_DEPTH, 0.625, 0.625) + np.array([[0, 0, 0.4], [0, 0, -0.3], [0, 0, 0]])}


def analytic_depth(K, size, T_cam_depth):
  """(depth (H, W) float64 along the camera's axis, on_sphere bool) of the scene seen by a pinhole camera whose frame is x_cam = T x_depth."""
  H, W = size
  T = np.asarray(T_cam_depth, np.float64)
  R, t = T[:3, :3], T[:3, 3]
  row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
  ray = np.stack([(col - K[0, 2]) / K[0, 0], (row - K[1, 2]) / K[1, 1], np.ones_like(col)], -1)      # z = 1: the parameter is the depth
  c = R @ SPHERE_CENTRE + t
  nrm = R @ np.array([0.0, 0.0, 1.0])
  with np.errstate(all='ignore'):
    plane = (PLANE_Z + nrm @ t) / (ray @ nrm)
    a, b, cc = (ray * ray).sum(-1), -2 * (ray @ c), c @ c - SPHERE_RADIUS ** 2
    disc = b * b - 4 * a * cc
    sphere = np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
  on_sphere = np.isfinite(sphere) & (sphere > 0)
  return np.where(on_sphere, sphere, np.where(plane > 0, plane, 0.0)), on_sphere


def end_to_end(size_colour, aligned=None):
  """The figures of the end-to-end test at one colour size.  `aligned`: the aligned depth (the device's); None: the restatement's."""
  Kc = COLOUR[size_colour]
  raw = analytic_depth(K_DEPTH, SIZE_DEPTH, np.eye(4))[0].astype(F)
  if aligned is None:
    aligned = reproject(raw[None], [K_DEPTH], [T_COLOUR_DEPTH], Kc, size_colour)['depth']
  truth, on_sphere = analytic_depth(Kc, size_colour, T_COLOUR_DEPTH)
  filled = aligned > 0
  err = np.abs(aligned.astype(np.float64) - truth)
  # what a caller without the alignment reads under the colour mask: the depth map resized to the colour size, nearest neighbour
  Hc, Wc = size_colour
  rr, cc = (np.arange(Hc) * SIZE_DEPTH[0]) // Hc, (np.arange(Wc) * SIZE_DEPTH[1]) // Wc
  naive_err = np.abs(raw[rr][:, cc].astype(np.float64) - truth)
  gap = PLANE_Z - (SPHERE_CENTRE[2] + SPHERE_RADIUS)
  cols = np.nonzero(on_sphere.any(0))[0]
  mid = 0.5 * (cols[0] + cols[-1])
  col = np.arange(Wc)[None, :]
  sides = [on_sphere & (col < mid), on_sphere & (col > mid)]
  return dict(median=float(np.median(err[filled])), beyond=float((err[filled] > 0.02).mean()), filled=float(filled.mean()),
              naive_wrong=[float((naive_err[m] > gap).mean()) for m in sides],
              aligned_wrong=[float((err > gap)[m & filled].mean()) for m in sides], raw=raw, aligned=aligned)


# ---- checks that need no restatement ----

PLANE_SCALES = (0.5, 1.0, 1.27, 1.5, 2.0)
PLANE_T = (0.025, -0.004, 0.003)


def plane_case(scale, size=(37, 53)):
  """A plane d = 0.8 perpendicular to the axis, a pure translation, the target intrinsics scaled: arguments of reproject."""
  Hd, Wd = int(np.ceil(size[0] * scale)), int(np.ceil(size[1] * scale))
  return np.full((1,) + size, 0.8, F), [K_SMALL], [transform(None, PLANE_T)], scaled_K(K_SMALL, scale, scale), (Hd, Wd), np.inf


def plane_check(depth_out, scale, size=(37, 53)):
  """(wrong, holes, must_fill): filled target pixels that are not float32(0.8) + float32(0.003) bit for bit (with an identity rotation
  rigid_apply is one rounded addition), and empty target pixels whose ray meets the plane at a point the source sees at least one pixel
  inside its border (float64)."""
  want = F(0.8) + F(0.003)
  filled = depth_out != 0
  wrong = int((depth_out[filled].view(np.uint32) != want.view(np.uint32)).sum())
  Kt = scaled_K(K_SMALL, scale, scale)
  Hd, Wd = depth_out.shape
  row, col = np.meshgrid(np.arange(Hd, dtype=np.float64), np.arange(Wd, dtype=np.float64), indexing='ij')
  z = 0.8 + PLANE_T[2]
  X, Y = (col - Kt[0, 2]) / Kt[0, 0] * z - PLANE_T[0], (row - Kt[1, 2]) / Kt[1, 1] * z - PLANE_T[1]      # in the source frame, at depth 0.8
  u, v = K_SMALL[0, 0] * X / 0.8 + K_SMALL[0, 2], K_SMALL[1, 1] * Y / 0.8 + K_SMALL[1, 2]
  inside = (u >= 1) & (u <= size[1] - 2) & (v >= 1) & (v <= size[0] - 2)
  return wrong, int((inside & ~filled).sum()), int(inside.sum())


def occlusion_case():
  """A near rectangle (0.6 m) in front of a far plane (1.1 m), seen from a camera 5 cm to the side (tz = 0, no rotation: z_out is the
  source depth itself)."""
  d = np.full((1, 40, 56), 1.1, F)
  d[0, 12:28, 20:36] = 0.6
  K = np.array([[50.0, 0, 27.7], [0, 50.0, 19.6], [0, 0, 1]])
  return d, [K], [transform(None, [-0.05, 0.0, 0.0])], K, (40, 56), np.inf


def occlusion_check(depth_out):
  """(contested, lost): target pixels on which the centres of a near AND a far source pixel land (float64 projection, rounded), and
  those of them that do not show the near depth."""
  d, (K,), (T,), _, (Hd, Wd), _ = occlusion_case()
  row, col = np.meshgrid(np.arange(40, dtype=np.float64), np.arange(56, dtype=np.float64), indexing='ij')
  z = d[0].astype(np.float64)
  u = np.floor(K[0, 0] * (((col - K[0, 2]) / K[0, 0] * z + T[0, 3]) / z) + K[0, 2] + 0.5).astype(int)
  v = np.floor(K[1, 1] * (((row - K[1, 2]) / K[1, 1] * z) / z) + K[1, 2] + 0.5).astype(int)
  ok = (u >= 0) & (u < Wd) & (v >= 0) & (v < Hd)
  near, far = np.zeros((Hd, Wd), bool), np.zeros((Hd, Wd), bool)
  near[v[ok & (d[0] < 1)], u[ok & (d[0] < 1)]] = True
  far[v[ok & (d[0] > 1)], u[ok & (d[0] > 1)]] = True
  contested = near & far
  return int(contested.sum()), int((depth_out[contested] != F(0.6)).sum())
