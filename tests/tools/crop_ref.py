"""A plain reference of the observed crop (csrc/crop.hip: fp_crop_observed, fp_warp_nearest), written from the definitions, not from the kernel:
numpy + fractions, no torch, no GPU.

  coordinates   kornia 0.7.2's warp_perspective for the axis-aligned tf = [[sx,0,tx],[0,sy,ty],[0,0,1]]: normalise both images with (size - 1),
                invert, un-normalise as F.grid_sample(align_corners=False) does - evaluated step by step in `fractions.Fraction` from the float32
                entries of tf (source_coords), so a coordinate is the real number the definition names.
  nearest       the project's tie rule (oracle/warp.py:round_half_even_snapped): closer than 1e-4 px to a half-integer counts as an exact tie,
                ties go to the even integer; everything else is floor(x + 1/2).  Zeros outside the source.
  bilinear      F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=False) on the float32-rounded coordinate, float32 op by op
                (numpy rounds every elementwise operation), then / 255.  bilinear_f64 is the same sum in float64 at the UNROUNDED coordinate,
                with the per-pixel bound a float32 evaluation may differ by (see bilinear_bound).
  scorer mode   depth -> crop (nearest) -> back to the frame (nearest, tf^-1) -> depth2xyzmap_batch (zfar = inf, float32) -> crop (nearest).
  batch transform   oracle/predict.py:_xyz_transform restated with np.float32: threshold 0.001 (0.1 for the scorer), minus the pose translation,
                times 1 / (d / 2), zero where invalid or |v| >= 2; without normalize_xyz only the translation is subtracted.

The lattice cases below make all of this EXACT: frames with (H - 1), (W - 1) powers of two and dyadic tf entries give source coordinates that float32
and float64 hold exactly, so every tie is an exact tie and nothing is left to a tolerance; the colours are multiples of 16, so that every bilinear
product and partial sum is a float32 (tests/test_crop_ref_host.py proves it in Fractions) and the only rounding is the division by 255.
Nothing here is random at import: every generator seeds its own numpy Generator."""
import functools
import math
from fractions import Fraction

import numpy as np

f32 = np.float32
HALF = Fraction(1, 2)
TIE_EPS = Fraction(1, 10000)
DIAMETER = 0.25                      # 1 / (d / 2) = 8: exact


# ------------------------------------------------------------------------------------------------------------------------------------------
# coordinates and lookups
# ------------------------------------------------------------------------------------------------------------------------------------------
def source_coords(s, t, n_out, n_src):
  """The source coordinate (grid_sample pixel units, align_corners=False) of output pixels 0 .. n_out - 1 along one axis, as Fractions.
  s, t: the float32 scale and offset of tf on this axis (dst = s * src + t); n_src: the source image's size on this axis."""
  s, t = Fraction(float(f32(s))), Fraction(float(f32(t)))
  out = []
  for i in range(n_out):
    g = Fraction(2 * i, n_out - 1) - 1            # the output grid: linspace(-1, 1, n_out)
    p = (g + 1) * (n_out - 1) / 2                 # normalised destination -> destination pixel (normal_transform_pixel, inverted)
    q = (p - t) / s                               # tf^-1
    n = 2 * q / (n_src - 1) - 1                   # source pixel -> normalised source (normal_transform_pixel)
    out.append(((n + 1) * n_src - 1) / 2)         # grid_sample's un-normalisation with align_corners=False
  return out


def inverse_coords(s, t, n_dst, n_src):
  """source_coords of the warp by tf^-1 = [[1/s, -t/s]]: destination = the frame axis (n_dst pixels), source = the crop axis (n_src)."""
  s, t = Fraction(float(f32(s))), Fraction(float(f32(t)))
  out = []
  for i in range(n_dst):
    q = s * i + t                                 # (tf^-1)^-1 = tf
    n = 2 * q / (n_src - 1) - 1
    out.append(((n + 1) * n_src - 1) / 2)
  return out


def nearest_index(x, tie='even', eps=TIE_EPS):
  """The tie rule on an exact coordinate.  tie='up' is a deliberately WRONG rule (ties round half up) for the discrimination test."""
  f = math.floor(x)
  if abs(x - f - HALF) < eps:
    if tie == 'even':
      return f if f % 2 == 0 else f + 1
    return f + 1
  return math.floor(x + HALF)


def to_f32(xs):
  return np.array([float(x) for x in xs], dtype=np.float64).astype(np.float32)


def gather(img, iy, ix):
  """img (H,W,C)[iy[:,None], ix[None,:]] with zeros outside -> (len(iy), len(ix), C)"""
  H, W = img.shape[:2]
  iy, ix = np.asarray(iy, dtype=np.int64), np.asarray(ix, dtype=np.int64)
  ok = ((iy >= 0) & (iy < H))[:, None] & ((ix >= 0) & (ix < W))[None, :]
  out = img[np.clip(iy, 0, H - 1)[:, None], np.clip(ix, 0, W - 1)[None, :]]
  return np.where(ok[..., None], out, img.dtype.type(0))


def _taps(img, x, y):
  """floor corners and the four zero-padded taps (nw, ne, sw, se) of coordinates x (Wo,), y (Ho,) of either float type"""
  x0, y0 = np.floor(x), np.floor(y)
  ix, iy = x0.astype(np.int64), y0.astype(np.int64)
  return x0, y0, (gather(img, iy, ix), gather(img, iy, ix + 1), gather(img, iy + 1, ix), gather(img, iy + 1, ix + 1))


def bilinear_f32(img, x32, y32):
  """grid_sample's bilinear sum in float32, every operation rounded: img (H,W,C) float32, float32 coordinates -> (Ho,Wo,C) / 255."""
  assert img.dtype == np.float32 and x32.dtype == np.float32 and y32.dtype == np.float32
  x0, y0, (nw, ne, sw, se) = _taps(img, x32, y32)
  wx1, wy1 = (x32 - x0)[None, :, None], (y32 - y0)[:, None, None]
  wx0, wy0 = ((x0 + f32(1)) - x32)[None, :, None], ((y0 + f32(1)) - y32)[:, None, None]
  acc = nw * (wx0 * wy0)
  acc = acc + ne * (wx1 * wy0)
  acc = acc + sw * (wx0 * wy1)
  acc = acc + se * (wx1 * wy1)
  assert acc.dtype == np.float32
  return acc / f32(255)


# float32 roundings of a value <= 1 between the float64 sum and a float32 evaluation of it (csrc/crop.hip, the rgb block): one in each of the two
# factors of a weight and one in their product (3, relative, on weights that sum to 1), one per tap product (1), three additions of partial sums
# <= 255 (the first adds to 0: exact), the division by 255 (1).  Second-order terms and float64's own rounding stay below 2^-40.
N_ROUNDINGS = 8
ARITH_TERM = N_ROUNDINGS * 2.0 ** -24 + 2.0 ** -40


def bilinear_f64(img, xs, ys, dx=None, dy=None):
  """The same sum in float64 at the exact coordinates (lists of Fractions) and the bound a float32 evaluation of it may differ by:
     coordinate term   |dx| * (largest horizontal difference among the four taps) + |dy| * (largest vertical difference), over 255: the sum is
                       continuous and piecewise linear in x and y with those slopes, and a coordinate rounded to float32 cannot leave its cell
                       (the integers are float32 numbers; a coordinate ON an integer takes the taps of both cells).  dx, dy default to half a float32 ulp of the coordinate.
     arithmetic term   ARITH_TERM."""
  x, y = np.array([float(v) for v in xs]), np.array([float(v) for v in ys])
  img = img.astype(np.float64)
  x0, y0, (nw, ne, sw, se) = _taps(img, x, y)
  wx1, wy1 = (x - x0)[None, :, None], (y - y0)[:, None, None]
  val = (nw * (1 - wx1) * (1 - wy1) + ne * wx1 * (1 - wy1) + sw * (1 - wx1) * wy1 + se * wx1 * wy1) / 255.0
  if dx is None:
    dx, dy = 0.5 * np.spacing(np.abs(x).astype(np.float32)).astype(np.float64), 0.5 * np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)
  hdiff, vdiff = 0.0, 0.0
  for ex in (0, 1):                  # a coordinate exactly on an integer lies on the border of two cells: both count
    for ey in (0, 1):
      _, _, (nw, ne, sw, se) = _taps(img, np.ceil(x) - 1 if ex else x, np.ceil(y) - 1 if ey else y)
      hdiff = np.maximum(hdiff, np.maximum(np.abs(ne - nw), np.abs(se - sw)))
      vdiff = np.maximum(vdiff, np.maximum(np.abs(sw - nw), np.abs(se - ne)))
  bound = (np.abs(dx)[None, :, None] * hdiff + np.abs(dy)[:, None, None] * vdiff) / 255.0 + ARITH_TERM
  return val, bound


def taps_outside(xs, ys, H, W):
  """(Ho,Wo) count of bilinear taps outside an H x W image.  The taps are {x0, x0+1} x {y0, y0+1}, so the count is 4 - (#x inside)(#y inside):
  0, 2 (an edge), 3 (a corner) or 4 - exactly one tap outside cannot happen on a rectangle."""
  nx = np.array([(0 <= math.floor(v) < W) + (0 <= math.floor(v) + 1 < W) for v in xs])
  ny = np.array([(0 <= math.floor(v) < H) + (0 <= math.floor(v) + 1 < H) for v in ys])
  return 4 - ny[:, None] * nx[None, :]


# ------------------------------------------------------------------------------------------------------------------------------------------
# the operations
# ------------------------------------------------------------------------------------------------------------------------------------------
def depth2xyz_f32(depth, K):
  """depth2xyzmap_batch (zfar = inf) of one image in float32, op by op: (H,W) -> (H,W,3)"""
  K = np.asarray(K, dtype=np.float64).astype(np.float32)
  H, W = depth.shape
  us, vs = np.arange(W, dtype=np.float32)[None, :], np.arange(H, dtype=np.float32)[:, None]
  xs = (us - K[0, 2]) * depth / K[0, 0]
  ys = (vs - K[1, 2]) * depth / K[1, 1]
  xyz = np.stack([xs, ys, depth], -1).astype(np.float32)
  xyz[depth < f32(0.001)] = 0
  return xyz


def xyz_transform(xyz, t, diameter, normalize_xyz, thres, ge2=True, info=None):
  """_xyz_transform of one item: xyz (Ho,Wo,3) float32, t the pose translation (3,).  ge2=False is a deliberately WRONG variant (> instead of >=)."""
  invalid = xyz[..., 2:3] < f32(thres)
  v = xyz - np.asarray(t, dtype=np.float32).reshape(1, 1, 3)
  if normalize_xyz:
    radius = f32(diameter) / f32(2)
    v = v * (f32(1) / radius)
    if info is not None:
      info['pre'] = v.copy()
      info['invalid'] = invalid.copy()
    big = (np.abs(v) >= f32(2)) if ge2 else (np.abs(v) > f32(2))
    v = np.where(invalid | big, f32(0), v)
  return v.astype(np.float32)


def crop_observed(rgb, geom, K, tf, poses, Ho, Wo, mode, diameter=DIAMETER, normalize_xyz=True, tie='even', ge2=True, eps=TIE_EPS, infos=None):
  """fp_crop_observed: rgb (H,W,3) float32 [0,255]; geom the xyz map (H,W,3) (mode 0, refiner) or the depth (H,W) (mode 1, scorer);
  tf (N,3,3) float32, poses (N,4,4) float32 -> planar (N,6,Ho,Wo) float32.  `infos`: a list that receives one dict of intermediates per item."""
  rgb, geom = np.asarray(rgb, dtype=np.float32), np.asarray(geom, dtype=np.float32)
  H, W = rgb.shape[:2]
  tf, poses = np.asarray(tf, dtype=np.float32), np.asarray(poses, dtype=np.float32)
  out = np.zeros((len(tf), 6, Ho, Wo), dtype=np.float32)
  near = lambda xs: [nearest_index(x, tie, eps) for x in xs]
  for b in range(len(tf)):
    sx, sy, tx, ty = tf[b, 0, 0], tf[b, 1, 1], tf[b, 0, 2], tf[b, 1, 2]
    xs, ys = source_coords(sx, tx, Wo, W), source_coords(sy, ty, Ho, H)
    info = dict(xs=xs, ys=ys)
    out[b, :3] = bilinear_f32(rgb, to_f32(xs), to_f32(ys)).transpose(2, 0, 1)
    qx, qy = near(xs), near(ys)
    info.update(qx=qx, qy=qy)
    if mode == 0:
      xyz = gather(geom, qy, qx)
      thres = 0.001
    else:
      crop = gather(geom[..., None], qy, qx)                                                 # depthBs (Ho,Wo,1)
      bx, by = inverse_coords(sx, tx, W, Wo), inverse_coords(sy, ty, H, Ho)
      info.update(bx=bx, by=by)
      frame = gather(crop, near(by), near(bx))[..., 0]                                       # back at full resolution (H,W)
      xyz = gather(depth2xyz_f32(frame, K), qy, qx)
      info.update(depth_crop=crop[..., 0], depth_frame=frame)
      thres = 0.1
    info['xyz'] = xyz
    v = xyz_transform(xyz, poses[b, :3, 3], diameter, normalize_xyz, thres, ge2, info)
    out[b, 3:] = v.transpose(2, 0, 1)
    if infos is not None:
      infos.append(info)
  return out


def to_nhwc8_half(planar):
  """the network-ready form: (N,6,Ho,Wo) float32 -> (N,Ho,Wo,8) float16, channels 6 and 7 zero"""
  n, _, h, w = planar.shape
  out = np.zeros((n, h, w, 8), dtype=np.float16)
  out[..., :6] = planar.transpose(0, 2, 3, 1).astype(np.float16)
  return out


def warp_nearest(src, tf, Ho, Wo, tie='even'):
  """fp_warp_nearest: src (1 or N, Hs, Ws, C) channel-last float32 (one image broadcasts), tf (N,3,3) -> planar (N,C,Ho,Wo)."""
  src, tf = np.asarray(src, dtype=np.float32), np.asarray(tf, dtype=np.float32)
  Hs, Ws, C = src.shape[1:]
  out = np.zeros((len(tf), C, Ho, Wo), dtype=np.float32)
  for b in range(len(tf)):
    qx = [nearest_index(x, tie) for x in source_coords(tf[b, 0, 0], tf[b, 0, 2], Wo, Ws)]
    qy = [nearest_index(y, tie) for y in source_coords(tf[b, 1, 1], tf[b, 1, 2], Ho, Hs)]
    out[b] = gather(src[b if len(src) > 1 else 0], qy, qx).transpose(2, 0, 1)
  return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------------
def make_tf(items):
  tf = np.zeros((len(items), 3, 3), dtype=np.float32)
  for b, (sx, sy, tx, ty) in enumerate(items):
    tf[b] = [[sx, 0, tx], [0, sy, ty], [0, 0, 1]]
  return tf


def make_poses(ts):
  poses = np.tile(np.eye(4, dtype=np.float32), (len(ts), 1, 1))
  poses[:, :3, 3] = np.asarray(ts, dtype=np.float32)
  return poses


# (sx, sy, tx, ty): dyadic scales, offsets multiples of 1/8.  On the 33 x 65 frame (source pixel q = (i - tx) / sx, x = q 65/64 - 1/2):
FAMILY_33x65 = [
    (0.5, 0.5, 0.0, 0.0),            # the whole frame at 17 x 33: ties at -0.5 and at W - 0.5 = 64.5, H - 0.5 = 32.5
    (1.0, 0.5, -8.125, 4.0),         # sx != sy; crosses the top edge
    (2.0, 1.0, 10.25, -20.5),        # crosses the left and the bottom edge
    (0.25, 0.25, -10.0, 2.5),        # crosses the right, the top and the bottom edge
    (4.0, 2.0, -100.5, -20.25),      # zoomed in, inside the frame: the bilinear weights with the most bits
    (1.0, 1.0, 100.0, 3.0),          # wholly outside (left of the frame)
]
FAMILY_65x129 = [
    (0.25, 0.25, 0.0, 0.0),          # the whole frame: ties at -0.5, 128.5 and 64.5
    (0.5, 1.0, -30.125, 8.0),
    (2.0, 0.5, 12.5, -50.25),
    (1.0, 1.0, 3.0, -70.0),          # wholly outside (below the frame)
]
# pose translations (dyadic); the first makes the threshold values of the pools below land on |v| = 2 exactly
TRANSLATIONS = [(0.0, -0.125, 0.5), (0.125, 0.0, 0.75), (0.0, 0.0, 0.0), (-0.25, 0.125, 0.5), (0.0, -0.125, 0.5), (0.125, -0.25, 1.0)]
K_LATTICE = np.array([[64.0, 0, 32.0], [0, 64.0, 16.0], [0, 0, 1.0]])

BELOW = lambda v: np.nextafter(f32(v), f32(0))
# mode 0, translation (0, -0.125, 0.5), 1 / radius = 8: x = 0.25 -> 2.0 exactly (zeroed), its nextafter below -> nextafter(2, 0) (kept); y = 0.125 and
# z = 0.75 likewise; z = 0.001f is valid, its nextafter below is not
X_POOL = [f32(0.25), BELOW(0.25), f32(-0.25), -BELOW(0.25), f32(0.125), f32(-0.0625), f32(0.0), f32(0.1875)]
Y_POOL = [f32(0.125), f32(0.125) - f32(2.0 ** -26), f32(-0.375), f32(0.0), f32(0.0625), f32(-0.125)]
Z_POOL = [f32(0.001), BELOW(0.001), f32(0.0), f32(0.75), f32(0.75) - f32(2.0 ** -24), f32(0.5), f32(0.625), f32(0.375)]
# mode 1: x = (qx - 32) z / 64, so column 48 with z = 1 gives 8 x = 2.0 and z = nextafter(1, 0) gives nextafter(2, 0) (translation x = 0)
D_POOL = [f32(0.0), BELOW(0.001), f32(0.001), BELOW(0.1), f32(0.1), BELOW(1.0), f32(1.0), f32(0.5), f32(0.75), f32(1.5)]


def lattice_frame(H, W, seed):
  """rgb in multiples of 16, the xyz map and the depth image drawn from the pools above"""
  rng = np.random.default_rng(seed)
  rgb = (rng.integers(0, 16, (H, W, 3)) * 16).astype(np.float32)
  pick = lambda pool: np.array(pool, dtype=np.float32)[rng.integers(0, len(pool), (H, W))]
  xyz = np.stack([pick(X_POOL), pick(Y_POOL), pick(Z_POOL)], -1)
  depth = pick(D_POOL)
  c = 3 * (W - 1) // 4                      # column 48 of 65 (96 of 129): (c - cx) / fx = 1/4 resp. 1
  depth[0::2, c], depth[1::2, c] = f32(1.0), BELOW(1.0)
  return rgb, xyz, depth


def unique_frame(H, W):
  """every pixel differs from its neighbours in every geometry channel (for the band probes: a lookup one pixel off is seen)"""
  r, c = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
  rng = np.random.default_rng(7)
  rgb = (rng.integers(0, 16, (H, W, 3)) * 16).astype(np.float32)
  depth = (0.5 + (r * W + c) / 8192.0).astype(np.float32)
  xyz = np.stack([(c - 30) / 256.0, (r - 10) / 256.0, depth], -1).astype(np.float32)
  return rgb, xyz, depth


# name: (H, W, Ho, Wo, modes, family)
LATTICE = {
    'r17x33': (33, 65, 17, 33, (0, 1), FAMILY_33x65),
    'r12x40': (33, 65, 12, 40, (0,), FAMILY_33x65),          # 480 px: two workgroups, the last one ragged
    'r20x24': (33, 65, 20, 24, (0,), FAMILY_33x65),
    's9x17': (33, 65, 9, 17, (1,), FAMILY_33x65),
    'big_frame': (65, 129, 17, 33, (0, 1), FAMILY_65x129),   # 561 px: three workgroups, ragged
    'production': (33, 65, 160, 160, (0, 1), FAMILY_33x65[:3]),
    'tiny_frame': (2, 2, 9, 17, (0,), [(4.0, 4.0, 6.0, 2.0), (2.0, 4.0, 3.0, 6.0)]),      # x = 2 q - 1/2: a tie every half source pixel, -1.5 among them
}
PROBE_DELTAS = (0.5e-4, 2e-4)        # inside the 1e-4 snapping band / outside it
PROBE_I, PROBE_J = 5, 3


def _probe_offset(i0, k, d, n_src):
  """the float32 offset t (scale 1) that puts output pixel i0 at source coordinate k + 0.5 + d"""
  return f32(i0 - (k + 1 + d) * (n_src - 1) / n_src)


@functools.lru_cache(maxsize=None)
def case(name):
  """dict(H, W, Ho, Wo, modes, rgb, xyz, depth, K, tf, poses, diameter, lattice)"""
  if name in LATTICE:
    H, W, Ho, Wo, modes, fam = LATTICE[name]
    rgb, xyz, depth = lattice_frame(H, W, seed=sorted(LATTICE).index(name))
    K = K_LATTICE * np.array([[(W - 1) / 64.0], [(H - 1) / 32.0], [1.0]]) if H > 2 else K_LATTICE
    return dict(name=name, H=H, W=W, Ho=Ho, Wo=Wo, modes=modes, rgb=rgb, xyz=xyz, depth=depth, K=K, tf=make_tf(fam),
                poses=make_poses(TRANSLATIONS[:len(fam)]), diameter=DIAMETER, lattice=True)
  if name == 'band_probes':
    # not dyadic: item n puts column PROBE_I at kx + 0.5 + d and row PROBE_J at ky + 0.5 + d, d = +-0.5e-4 (snaps) or +-2e-4 (does not), for an
    # even and an odd k, and once at -1.5; all |coordinates| < 100
    H, W, Ho, Wo = 33, 65, 9, 17
    rgb, xyz, depth = unique_frame(H, W)
    items, probes = [], []
    for kx, ky in ((10, 6), (21, 13), (-2, -2)):
      for mag in PROBE_DELTAS:
        for sgn in (1, -1):
          d = sgn * mag
          items.append((1.0, 1.0, _probe_offset(PROBE_I, kx, d, W), _probe_offset(PROBE_J, ky, d, H)))
          probes.append((kx, ky, d))
    return dict(name=name, H=H, W=W, Ho=Ho, Wo=Wo, modes=(0, 1), rgb=rgb, xyz=xyz, depth=depth, K=K_LATTICE, tf=make_tf(items),
                poses=make_poses([(0.0, 0.0, 0.0)] * len(items)), diameter=DIAMETER, lattice=False, probes=probes)
  if name == 'non_lattice':
    # what compute_crop_window_tf_batch produces (sx = out_w / (right - left), tx = sx * (-left) in float32, integer window borders); the first
    # window overhangs the frame's top-left corner, the second its bottom-right corner
    H, W, Ho, Wo = 33, 65, 20, 24
    rng = np.random.default_rng(11)
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.float32)
    depth = rng.uniform(0.3, 1.5, (H, W)).astype(np.float32)
    depth[rng.uniform(size=(H, W)) < 0.15] = 0
    K = np.array([[61.7, 0, 31.4], [0, 60.3, 16.2], [0, 0, 1.0]])
    xyz = depth2xyz_f32(depth, K)
    items = []
    for left, right, top, bottom in ((-5, 32, -7, 20), (40, 77, 15, 45), (11, 30, 4, 27)):
      sx, sy = f32(Wo) / f32(right - left), f32(Ho) / f32(bottom - top)
      items.append((sx, sy, sx * f32(-left), sy * f32(-top)))
    ts = [(-0.11, -0.07, 0.83), (0.21, 0.13, 0.91), (0.01, -0.02, 0.77)]
    return dict(name=name, H=H, W=W, Ho=Ho, Wo=Wo, modes=(0, 1), rgb=rgb, xyz=xyz, depth=depth, K=K, tf=make_tf(items), poses=make_poses(ts),
                diameter=0.31, lattice=False)
  raise KeyError(name)


LATTICE_CASES = tuple(LATTICE)
ALL_CASES = LATTICE_CASES + ('band_probes', 'non_lattice')
RUNS = tuple((n, m) for n in ALL_CASES for m in (LATTICE[n][4] if n in LATTICE else (0, 1)))      # every (case, mode) a test runs


@functools.lru_cache(maxsize=None)
def expected(name, mode, normalize_xyz):
  """(reference output (N,6,Ho,Wo), per-item intermediates): computed once, shared by the tests; treat as read-only"""
  c = case(name)
  infos = []
  out = crop_observed(c['rgb'], c['xyz'] if mode == 0 else c['depth'], c['K'], c['tf'], c['poses'], c['Ho'], c['Wo'], mode, c['diameter'],
                      normalize_xyz, infos=infos)
  out.setflags(write=False)
  return out, infos


def rgb_f64_and_bound(name):
  """float64 rgb (N,3,Ho,Wo) at the exact coordinates and the derived per-pixel bound for a float32 evaluation (the non-lattice comparison)"""
  c = case(name)
  vals, bounds = [], []
  for b in range(len(c['tf'])):
    xs = source_coords(c['tf'][b, 0, 0], c['tf'][b, 0, 2], c['Wo'], c['W'])
    ys = source_coords(c['tf'][b, 1, 1], c['tf'][b, 1, 2], c['Ho'], c['H'])
    v, bd = bilinear_f64(c['rgb'], xs, ys)
    vals.append(v.transpose(2, 0, 1)), bounds.append(bd.transpose(2, 0, 1))
  return np.stack(vals), np.stack(bounds)
