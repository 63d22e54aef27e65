"""fp_template_match (csrc/detect.hip) and the suppression of foundationpose_amd/detect.py restated in numpy, rule for rule as
include/foundationpose_amd.h states them: every value is a numpy float32 and every operation is rounded once in the written order, so the
kernel has to give the same bits.  `match` also reports why samples and candidates failed, and `clutter_scene` is the recipe of the seeded
scenes that the host and the GPU tests detect the object in."""
import numpy as np

F = np.float32
MIN_DEPTH = F(0.001)

REASONS = ('anchor_no_depth', 'anchor_zfar', 'anchor_nan', 'zc_below', 'zc_above', 'z_small', 'left', 'right', 'top', 'bottom', 'in_tolerance',
           'in_no_reading', 'out_tolerance', 'out_no_reading')


def lattice(H, W, stride, r0, c0):
  return np.arange(r0, H, stride), np.arange(c0, W, stride)


def match(depth, K, table, ranges, n_in, n_out, anchors, stride=4, r0=0, c0=0, z_min=0.05, z_max=20.0, zfar=np.inf, tol_in=0.01, tol_out=0.03):
  """keys, counts (n_obj, Hs, Ws) uint32 of ONE frame and the dict of how often each of REASONS occurred.  'out_no_reading' counts
  out-samples that PASS for want of a reading; every other sample reason counts failures."""
  D = np.asarray(depth, dtype=F)
  H, W = D.shape
  fx, fy, cx, cy = F(K[0][0]), F(K[1][1]), F(K[0][2]), F(K[1][2])
  z_min, z_max, zfar, tol_in, tol_out = F(z_min), F(z_max), F(zfar), F(tol_in), F(tol_out)
  table = np.asarray(table, dtype=F)
  rows, cols = lattice(H, W, stride, r0, c0)
  n_obj = len(ranges) - 1
  keys = np.zeros((n_obj, len(rows), len(cols)), np.uint32)
  counts = np.zeros_like(keys)
  why = dict.fromkeys(REASONS, 0)
  rr, cc = np.meshgrid(rows, cols, indexing='ij')
  d = D[rr, cc]
  with np.errstate(invalid='ignore'):
    live = (d >= MIN_DEPTH) & (d < zfar)
    why['anchor_nan'] += int(np.isnan(d).sum())
    why['anchor_no_depth'] += int((~np.isnan(d) & ~(d >= MIN_DEPTH)).sum())
    why['anchor_zfar'] += int(((d >= MIN_DEPTH) & ~(d < zfar)).sum())
  li, lj = np.nonzero(live)
  d = d[li, lj]
  bx = ((cc[li, lj].astype(F) - cx) / fx) * d
  by = ((rr[li, lj].astype(F) - cy) / fy) * d
  for o in range(n_obj):
    best = np.zeros(len(d), np.uint32)
    best_counts = np.zeros(len(d), np.uint32)
    for t in range(ranges[o], ranges[o + 1]):
      for a in range(anchors):
        A = table[t, a]
        zc = d - A[2]
        ok = (zc >= z_min) & (zc <= z_max)
        why['zc_below'] += int((~(zc >= z_min)).sum())
        why['zc_above'] += int((~(zc <= z_max)).sum())
        if not ok.any():
          continue
        Cx, Cy = (bx - A[0])[ok, None], (by - A[1])[ok, None]
        S = table[t][None, :, :]
        X, Y, Z = Cx + S[:, :, 0], Cy + S[:, :, 1], zc[ok, None] + S[:, :, 2]
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
          z_ok = Z >= MIN_DEPTH
          u, v = (fx * X) / Z + cx, (fy * Y) / Z + cy
          cf, rf = np.floor(u + F(0.5)), np.floor(v + F(0.5))
          inside = z_ok & (cf >= 0) & (cf <= F(W - 1)) & (rf >= 0) & (rf <= F(H - 1))
          why['z_small'] += int((~z_ok).sum())
          why['left'] += int((z_ok & ~(cf >= 0)).sum())
          why['right'] += int((z_ok & ~(cf <= F(W - 1))).sum())
          why['top'] += int((z_ok & ~(rf >= 0)).sum())
          why['bottom'] += int((z_ok & ~(rf <= F(H - 1))).sum())
          obs = D[np.where(inside, rf, 0).astype(np.int64), np.where(inside, cf, 0).astype(np.int64)]
          read = obs >= MIN_DEPTH
          gap = np.abs(obs - Z)
          is_in = np.arange(n_in + n_out)[None, :] < n_in
          in_pass = inside & is_in & read & (gap <= tol_in)
          out_pass = inside & ~is_in & (~read | (gap > tol_out))
          why['in_no_reading'] += int((inside & is_in & ~read).sum())
          why['in_tolerance'] += int((inside & is_in & read & ~(gap <= tol_in)).sum())
          why['out_no_reading'] += int((inside & ~is_in & ~read).sum())
          why['out_tolerance'] += int((inside & ~is_in & read & ~(gap > tol_out)).sum())
        ni, no = in_pass.sum(axis=1).astype(np.uint32), out_pass.sum(axis=1).astype(np.uint32)
        key = ((ni * no) << np.uint32(16)) | np.uint32(0xFFFF - (4 * (t - ranges[o]) + a))
        sel = np.nonzero(ok)[0]
        wins = key > best[sel]
        best[sel[wins]] = key[wins]
        best_counts[sel[wins]] = ((ni << np.uint32(16)) | no)[wins]
    keys[o, li, lj] = best
    counts[o, li, lj] = best_counts
  return keys, counts, why


def nms(keys, depth, K, table, ranges, rotations, radii, top_k=4, stride=4, r0=0, c0=0, min_score=0.0, full=1):
  """Greedy suppression per object in float64: candidates by key descending, the lower flat index first among equal keys; the centre is
  the anchor pixel at its depth minus the anchor sample.  Returns per object a list of (flat index, template, anchor, centre (3,))."""
  K = np.asarray(K, dtype=np.float64)
  out = []
  for o in range(len(ranges) - 1):
    flat = keys[o].reshape(-1).astype(np.int64)
    Ws = keys.shape[2]
    order = sorted(range(len(flat)), key=lambda n: (-flat[n], n))
    kept = []
    for n in order:
      if len(kept) >= top_k or flat[n] == 0:
        break
      score, low = flat[n] >> 16, 0xFFFF - (flat[n] & 0xFFFF)
      if score < min_score * full:
        break
      t, a = ranges[o] + (low >> 2), low & 3
      r, c = r0 + (n // Ws) * stride, c0 + (n % Ws) * stride
      d = float(depth[r, c])
      A = table[t, a].astype(np.float64)
      C = np.array([(c - K[0, 2]) / K[0, 0] * d - A[0], (r - K[1, 2]) / K[1, 1] * d - A[1], d - A[2]])
      if any(np.linalg.norm(C - k[3]) <= radii[o] for k in kept):
        continue
      kept.append((n, int(t), int(a), C))
    out.append(kept)
  return out


# ---- the seeded clutter scenes -------------------------------------------------------------------------------------------------------
SCENE_H, SCENE_W, SCENE_F = 120, 160, 150.0
SCENE_K = np.array([[SCENE_F, 0, (SCENE_W - 1) / 2.0], [0, SCENE_F, (SCENE_H - 1) / 2.0], [0, 0, 1.0]])
SCENE_SEEDS = (1, 8, 28)      # scenes with all of the object visible in which the top-1 beats the mask path (DESIGN.md section 5 lists all forty tried)


def uv_sphere(radius, n_lat=10, n_lon=16):
  """(vertices, faces) of a latitude-longitude sphere about the origin, outward faces."""
  v = [[0, 0, radius]]
  for i in range(1, n_lat):
    th = np.pi * i / n_lat
    for j in range(n_lon):
      ph = 2 * np.pi * j / n_lon
      v.append([radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)])
  v.append([0, 0, -radius])
  f = []
  ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
  for j in range(n_lon):
    f.append([0, ring(1, j), ring(1, j + 1)])
    f.append([len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)])
  for i in range(1, n_lat - 1):
    for j in range(n_lon):
      f.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
      f.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
  return np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int64)


def random_rotation(rs):
  q = rs.randn(4)
  q /= np.linalg.norm(q)
  w, x, y, z = q
  return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def clutter_layout(seed):
  """The seeded layout of a scene: the object's pose (of the CENTRED model) at 0.55 - 0.8 m, four distractor spheres of 4 - 10 cm diameter
  at 0.5 - 0.9 m and a tilted background plane n . x = n . p0 at about 1.1 m."""
  rs = np.random.RandomState(7000 + seed)
  pose = np.eye(4)
  pose[:3, :3] = random_rotation(rs)
  z = rs.uniform(0.55, 0.8)
  pose[:3, 3] = [rs.uniform(-0.12, 0.12) * z / 0.55, rs.uniform(-0.07, 0.07) * z / 0.55, z]
  spheres = []
  for _ in range(4):
    zs = rs.uniform(0.5, 0.9)
    spheres.append((rs.uniform(0.02, 0.05), np.array([rs.uniform(-0.45, 0.45) * zs, rs.uniform(-0.32, 0.32) * zs, zs])))
  normal = np.array([rs.uniform(-0.25, 0.25), rs.uniform(-0.25, 0.25), -1.0])
  normal /= np.linalg.norm(normal)
  return dict(pose=pose, spheres=spheres, plane=(normal, np.array([0.0, 0.0, rs.uniform(1.05, 1.2)])))


def plane_depth(plane, K, H, W):
  """The depth image of the plane n . x = n . p0, float64; 0 where the ray does not meet it in front of the camera."""
  n, p0 = plane
  vs, us = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
  ray = np.stack([(us - K[0, 2]) / K[0, 0], (vs - K[1, 2]) / K[1, 1], np.ones((H, W))], axis=-1)
  z = (n @ p0) / (ray @ n)
  return np.where(z > 0, z, 0.0)


def clutter_scene(seed, render_instances, H=SCENE_H, W=SCENE_W, K=SCENE_K):
  """One scene.  render_instances(K, H, W, [(vertices, faces) | 'object', ...], poses (n,4,4)) -> depths (n, H, W) of each instance alone
  (0 where it does not render): the CPU rasteriser on the host, the library's on the GPU.  Returns depth (H, W) float32 - the nearest of
  the object, the spheres and the plane, rounded to mm after 1 mm of noise, 2 % dropped -, the object's visible mask, its visible
  fraction and its pose."""
  lay = clutter_layout(seed)
  shapes, poses = ['object'], [lay['pose']]
  for radius, centre in lay['spheres']:
    shapes.append(uv_sphere(radius))
    p = np.eye(4)
    p[:3, 3] = centre
    poses.append(p)
  each = np.asarray(render_instances(K, H, W, shapes, np.asarray(poses)), dtype=np.float64)
  layers = np.concatenate([each, plane_depth(lay['plane'], K, H, W)[None]])
  far = np.where(layers >= 0.001, layers, np.inf)
  depth = far.min(axis=0)
  visible = (each[0] >= 0.001) & (far.argmin(axis=0) == 0)
  rs = np.random.RandomState(9000 + seed)
  noisy = np.round((depth + rs.randn(H, W) * 0.001) * 1000.0) / 1000.0
  noisy[~np.isfinite(noisy)] = 0
  noisy[rs.uniform(size=(H, W)) < 0.02] = 0
  return dict(depth=noisy.astype(F), mask=visible, visible_fraction=float(visible.sum()) / max(1, int((each[0] >= 0.001).sum())), pose=lay['pose'], K=K)


# ---- the small case of the condition test and of the bit-for-bit GPU test ----------------------------------------------------------------
SMALL = dict(n_in=12, n_out=9, anchors=2, z_min=0.35, z_max=0.9, zfar=2.0, tol_in=0.01, tol_out=0.03)
SMALL_K = np.array([[110.0, 0, 47.3], [0, 108.0, 35.6], [0, 0, 1.0]])


def small_table(n_templates, seed=0, n_in=12, n_out=9):
  """A seeded synthetic table: in-samples within a 12 x 8 x 4 cm box about the centre, the first two (the anchors) near the centre ray,
  out-samples on a ring of 8 - 9 cm; w = 0."""
  rs = np.random.RandomState(100 + seed)
  t = np.zeros((n_templates, n_in + n_out, 4), F)
  t[:, :n_in, 0] = rs.uniform(-0.06, 0.06, (n_templates, n_in))
  t[:, :n_in, 1] = rs.uniform(-0.04, 0.04, (n_templates, n_in))
  t[:, :n_in, 2] = rs.uniform(-0.04, 0.0, (n_templates, n_in))
  t[:, :2, :2] *= F(0.1)
  ang = rs.uniform(0, 2 * np.pi, (n_templates, n_out))
  rad = rs.uniform(0.08, 0.09, (n_templates, n_out))
  t[:, n_in:, 0], t[:, n_in:, 1] = rad * np.cos(ang), rad * np.sin(ang)
  t[:, n_in:, 2] = rs.uniform(-0.01, 0.01, (n_templates, n_out))
  return t


def small_case():
  """Three 72 x 96 frames, two objects with ranges 0 / 23 / 40: frame 0 a tilted plane with boxes of the templates' size cut by each of the
  four borders and one inside; frame 1 the same with patches of zeros, NaN, values at and beyond zfar and depths that put zc outside
  z_range on either side; frame 2 seeded noise.  Template 5 duplicates template 2 (the lower index must win) and template 7 has one sample
  0.8 m in front of the centre (Z < 0.001)."""
  H, W = 72, 96
  table = small_table(40)
  table[5] = table[2]
  table[7, 11, 2] = F(-0.8)
  vs, us = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
  plane = (0.7 + 0.0009 * us - 0.0012 * vs).astype(F)
  f0 = plane.copy()
  for r, c in ((36, 2), (36, 93), (1, 48), (70, 48), (30, 40)):      # boxes 12 x 8 cm at 0.55 m: about 24 x 16 pixels
    f0[max(r - 8, 0):r + 8, max(c - 12, 0):c + 12] = F(0.55)
  f1 = f0.copy()
  f1[10:20, 10:30] = 0
  f1[40:50, 60:70] = np.nan
  f1[55:60, 20:30] = F(2.0)
  f1[60:64, 20:30] = F(3.5)
  f1[20:26, 70:90] = F(0.32)      # zc below z_min
  f1[4:10, 60:80] = F(0.95)       # zc above z_max for most anchors
  rs = np.random.RandomState(5)
  f2 = rs.uniform(0.3, 1.0, (H, W)).astype(F)
  f2[rs.uniform(size=(H, W)) < 0.1] = 0
  return dict(frames=np.stack([f0, f1, f2]), K=SMALL_K, table=table, ranges=np.array([0, 23, 40], np.int32), **SMALL)
