"""Exact reference of the rasteriser (csrc/raster.hip) on LATTICE meshes.  numpy, Python ints and `fractions` only: nothing here imports
foundationpose_amd or oracle.  tests/test_raster_ref_host.py checks what is here (and the CPU mirror oracle/raster_c.c against it),
tests/test_gpu_raster_exact.py the HIP kernels.

THE CONSTRUCTION.  Frame W = H = 64, K = [[64,0,32],[0,64,32],[0,0,1]], identity rotation, translation (tx, ty, 1).  The documented camera model
(nvdiffrast_render: clip = P @ glcam_in_cvcam @ pose, optional bbox2d window transform on rows 0 / 1, screen = (ndc + 1) / 2 * size, snapped to
1/16 px by round-half-even, rows bottom-up, pixel centres at half-integers) then gives, for a vertex (px, py, pz):
    w = pz + 1,   X = 16 hw (t00 2 (px + tx) / w + t30 + 1),   Y = 16 hh (-t11 2 (py + ty) / w + t31 + 1)          (hw = Wo/2, hh = Ho/2)
A case CHOOSES the lattice coordinates (X, Y) in 1/16 px (pixel centre (i, j) is (16 i + 8, 16 j + 8)), and w from {1/2, 1, 2, 4, 8}, and places
the vertex at px = w (X / (16 hw) - 1 - t30) / (2 t00), py likewise: every float32 intermediate of the transform is a dyadic rational of at most
24 bits, so nothing rounds (transform_check).  A caller's projection_mat may replace row 2 = (0, 0, A, B) only: z/w = B / w - A, one exact value
per depth layer.  Hypotheses differ by translations tx = dx / (32 hw t00): the whole lattice moves by dx / w, an integer.

COVERAGE (coverage_exact).  With the raw integers e_k = dx_k (Py - Y_{k+1}) - dy_k (Px - X_{k+1}) of the edge opposite vertex k and the doubled
signed area a, the barycentric weight of vertex k at a point is e_k / a whatever the winding.  The documented rule is "top-left": a centre ON an
edge belongs to the triangle whose interior lies to the right of / below it in the image (rows top-down), i.e. to the right of / ABOVE it in the
bottom-up rows used here - a point moved a little to the left and, by less, downwards (bottom-up: y decreasing) stays in the same triangle.
So the reference asks for the centre displaced by the symbolic infinitesimal (-eps, -eps^2) to be STRICTLY inside:
    e_k(P + d) / a = (e_k + eps dy_k - eps^2 dx_k) / a > 0   <=>   sign(a) (e_k, dy_k, -dx_k) > (0, 0, 0) lexicographically.
No "tl" flag and no sign normalisation appear; the host test shows that this equals the literal statement of the rule and an evaluation with
the concrete rational eps = 2^-40.  Zero-area faces cover nothing.  The winner of a pixel is the minimum of (exact z/w, face id) over the faces
that claim it with -1 <= z/w <= 1.

WHERE THE KERNEL'S FLOAT DEPTH IS EXACT.  z/w at a pixel is fmaf(b2, z2, fmaf(b1, z1, b0 z0)), b_k = float(e_k) / float(a).  That equals the
exact value (a) at z = 0, (b) where every b_k is 0, 1/2 or 1 - all covered centres of a right triangle with legs of 1 or 2 px on centres -
and (c) for a few-bit constant z on a triangle whose doubled area is a power of two.  Cases whose decision hangs on one ulp (depth_signs_ulp*,
zclip_hi / _lo, ties at z = 0) use only such faces; everywhere else two competing depths are at least DEPTH_GAP apart (checked on the host).

TOLERANCES of the float outputs, against interp_float64 (float64 from the lattice integers):
  u, v, z/w.  Roundings of u = (b0 / w0) / ((q0 + q1) + q2): e/a (2^-24 relative), / w (2^-24; exact for w a power of two), two adds of positive
    terms (2 x 2^-24 on the sum), / qs (2^-24): at most 2 + 2 + 2 + 1 = 7 half-ulps, 7 x 2^-24 = 4.2e-7 on a value <= 1.  A float32 emulation of
    that operation order (emulate_f32) over every case and hypothesis gives a largest error of EMU_UVZ = 1.25e-7 (zclip_slant); TOL_UVZ = 4 x that = 5.0e-7.
  depth, xyz, colour.  w2 = (1 - u) - v carries the errors of u and v; the attribute is fmaf(u, a0, fmaf(v, a1, w2 a2)).  Normalised by the
    largest |vertex value| of the case the emulation gives at most EMU_ATTR = 1.54e-7 (far64_1600008); TOL_ATTR = 4 x that = 6.2e-7 (times the value range).
  (python -m tests.tools.raster_ref prints both maxima per case; the host test asserts that they stay inside the recorded constants.)

TEXTURE FETCH AND LIGHTING (SHADE_CASES; shade_float64, written from src/Utils.py:185-216 and nvdiffrast's documented dr.texture, not from oracle/).
  Texel (r, c) of tex[0] (Ht, Wt, 3), row 0 first in memory, has its centre at uv = ((c + 0.5) / Wt, (r + 0.5) / Ht); the fetch at the perspective-
  correct uv[uv_idx[face]] blends floor(x), floor(x) + 1 and floor(y), floor(y) + 1 of x = u Wt - 0.5, y = v Ht - 0.5, indices modulo the size,
  weights the fractional parts; no v flip.  Lighting is per vertex and interpolated; then the clip to [0, 1]; the normal map is the normalised
  interpolation of R n.
  colour.  The fetch is continuous in uv (a floor that falls on the other side of an integer changes weights 0 / 1 by the same few ulps), with slope
    (texel-to-texel step) x (texture size); uv carries the errors of u, v and its own fmaf chain relative to max(1, |uv|).  tex_scale(case) is that
    product (not below 1), shade_tol adds the lighting's factors.  The float32 emulation (emulate_shade_f32) over every SHADE case, hypothesis and light
    setting gives at most EMU_TEX = 1.73e-7 x scale (tex_perspective: 1.38e-6 at scale 8); TOL_TEX = 4 x that = 6.9e-7 (times the scale: 5.5e-6 for
    the 16-texel checker, 1.6e-5 for the 8 x 16 texture of distinct texels, 1.2e-6 for lit vertex colours).
  bit equality (claims['exact']).  On a w = 1 right triangle with power-of-two legs b_k = e_k / a, qs = 1, u, v and w2 are exact; with dyadic uv and
    dyadic texels so are texc, x, the weights (0 or 1/2) and every blend: the emulation equals float64 bit for bit (host test), and so must the kernel.
  normal map.  Within TOL_ATTR of a unit vector; the emulation's largest error is 1.27e-7 (lit_*: interpolated normals never shorter than 0.68).
"""
import functools
from fractions import Fraction as Fr

import numpy as np

W = H = 64
K = np.array([[64.0, 0, 32.0], [0, 64.0, 32.0], [0, 0, 1.0]])
EMU_UVZ, EMU_ATTR = 1.25e-7, 1.54e-7
EMU_TEX = 1.73e-7
TOL_UVZ, TOL_ATTR, TOL_TEX = 4 * EMU_UVZ, 4 * EMU_ATTR, 4 * EMU_TEX
DEPTH_GAP = 2.0 ** -10          # competing depths that are not exact in float32 are at least this far apart
ZCLIP_CAP = 0.02                # share of a slanted triangle's pixels that may lie within TOL_UVZ of z/w = +-1
RB_SMALL, RB_MEDIUM = 4, 32     # candidate pixels of the size classes (restated in face_classes)


def _f32_exact(x):
  x = Fr(x)
  return Fr(float(np.float32(float(x)))) == x


class _Mesh:
  def __init__(self):
    self.v, self.f = [], []

  def vert(self, X, Y, w=1):
    self.v.append((Fr(X), Fr(Y), Fr(w)))
    return len(self.v) - 1

  def tri(self, p0, p1, p2, w=1, flip=False, rot=0):
    """a triangle of its own three vertices; p = (X, Y) or (X, Y, w)"""
    ids = [self.vert(*(tuple(p) + (w,))[:3]) for p in (p0, p1, p2)]
    ids = ids[rot:] + ids[:rot]
    if flip:
      ids = [ids[0], ids[2], ids[1]]
    self.f.append(tuple(ids))
    return len(self.f) - 1


def _window(bbox):
  """src/Utils.py:172-180: the bbox2d window transform of clip rows 0 / 1 as exact rationals (t00, t11, t30, t31)"""
  if bbox is None:
    return Fr(1), Fr(1), Fr(0), Fr(0)
  l, t, r, b = Fr(bbox[0]), H - Fr(bbox[1]), Fr(bbox[2]), H - Fr(bbox[3])
  return W / (r - l), H / (t - b), (W - r - l) / (r - l), (H - t - b) / (t - b)


def _finish(name, m, claims, AB=None, bbox=None, out=(64, 64), shifts=None, real=None, order=None, tex=None, corner_uv=None, normals_cam=None, rot=None):
  """lattice mesh -> the case dict.  AB = (A, B): projection_mat row 2 = (0, 0, A, B), z/w = B / w - A; None: the default projection (w = 1 only).
  tex (Ht, Wt, 3) with corner_uv (F, 3, 2): a textured case (uv / uv_idx built by _uv_table, no vertex_color).  normals_cam (V, 3): per-vertex normals
  as the camera is to see them; rot: the poses' rotation R, a signed permutation (exact in float32) - the model holds R^T (position | normal)."""
  Ho, Wo = out
  hw, hh = Fr(Wo, 2), Fr(Ho, 2)
  t00, t11, t30, t31 = _window(bbox)
  V = len(m.v)
  Xq = np.array([float(v[0]) for v in m.v])
  Yq = np.array([float(v[1]) for v in m.v])
  w = np.array([float(v[2]) for v in m.v])
  pos = np.zeros((V, 3), np.float32)
  for i, (X, Y, wv) in enumerate(m.v):
    px = wv * (X / (16 * hw) - 1 - t30) / (2 * t00)
    py = -wv * (Y / (16 * hh) - 1 - t31) / (2 * t11)
    assert _f32_exact(px) and _f32_exact(py) and _f32_exact(wv - 1), (name, i, X, Y, wv)
    pos[i] = [float(px), float(py), float(wv - 1)]
  Rm = np.eye(3, dtype=np.float32) if rot is None else np.asarray(rot, np.float32)
  assert np.array_equal(Rm @ Rm.T, np.eye(3)) and np.linalg.det(Rm) == 1 and set(np.abs(Rm).ravel()) == {0, 1}, name
  pos = pos @ Rm                                        # rows R^T p: the pose's R p gives the lattice position back, exactly
  ncam = np.tile(np.array([0, 0, -1], np.float32), (V, 1)) if normals_cam is None else np.asarray(normals_cam, np.float32)
  assert ncam.shape == (V, 3)
  faces = np.array(m.f, np.int32).reshape(-1, 3)
  if order is not None:
    assert corner_uv is None
    faces = faces[np.asarray(order)]
  proj = None
  if AB is not None:
    A, B = Fr(AB[0]), Fr(AB[1])
    proj = np.array([[2 * K[0, 0] / W, 0, (-2 * K[0, 2] + W) / W, 0], [0, 2 * K[1, 1] / H, (2 * K[1, 2] - H) / H, 0],
                     [0, 0, float(A), float(B)], [0, 0, -1, 0]], np.float64)
    zw = np.array([float(B / v[2] - A) for v in m.v])
    for v in m.v:
      assert _f32_exact(B / v[2] - A) and _f32_exact(B - A * v[2]), (name, v)
  else:
    assert np.all(w == 1), name
    zn, zf = Fr(1, 1000), Fr(100)                      # default near / far; row 2 of the clip matrix at pz = 0, rounded once (float64 -> float32)
    zw = np.full(V, float(np.float32(float((zf + zn) / (zf - zn) - 2 * zf * zn / (zf - zn)))))
  shifts = shifts or [(0, 0), (16, -32), (-48, 16), (32, 48), (-16, -16)]
  poses = np.tile(np.eye(4, dtype=np.float32), (len(shifts), 1, 1))
  for h, (dx, dy) in enumerate(shifts):
    tx, ty = Fr(dx) / (32 * hw * t00), -Fr(dy) / (32 * hh * t11)
    assert _f32_exact(tx) and _f32_exact(ty)
    assert all((Fr(dx) / wv).denominator == 1 and (Fr(dy) / wv).denominator == 1 for wv in set(v[2] for v in m.v)), (name, dx, dy)
    poses[h, :3, 3] = [float(tx), float(ty), 1.0]
    poses[h, :3, :3] = Rm
  rs = np.random.RandomState(len(name) * 7919 + V)
  vcol = (rs.randint(0, 257, (V, 3)) / 256.0).astype(np.float32)
  real = np.arange(len(faces)) if real is None else np.asarray(real)
  mt = dict(pos=pos, faces=faces, vnormals=ncam @ Rm)
  if tex is None:
    mt['vertex_color'] = vcol
  else:
    tex = np.asarray(tex, np.float32)
    assert tex.ndim == 3 and tex.shape[2] == 3 and max(tex.shape[:2]) <= 16
    mt['uv'], mt['uv_idx'] = _uv_table(np.asarray(corner_uv, np.float64), faces, V, rs)
    mt['tex'] = tex[None].copy()
  return dict(name=name, Ho=Ho, Wo=Wo, H=H, W=W, K=K.copy(), projection_mat=proj, bbox2d=None if bbox is None else np.tile(np.asarray(bbox, np.float32), (len(shifts), 1)),
              Xq=Xq, Yq=Yq, X=np.rint(Xq).astype(np.int64), Y=np.rint(Yq).astype(np.int64), w=w, zw=zw, faces=faces, real=real, shifts=shifts, poses=poses,
              mesh_tensors=mt,
              claims=claims, mesh_diameter=2.0)


def _uv_table(corner_uv, faces, V, rs):
  """(F, 3, 2) uv of every face corner -> uv (rows, 2) float32, uv_idx (F, 3) int32.  Rows 0 .. V - 1 are decoys (what a fetch through `faces` would
  read), the distinct corner values follow in shuffled order with more decoys between them: uv_idx differs from faces in every entry and there are
  more uv rows than vertices, as in a baked atlas."""
  assert corner_uv.shape == faces.shape + (2,) and np.array_equal(corner_uv.astype(np.float32).astype(np.float64), corner_uv)
  keys = sorted(set(map(tuple, corner_uv.reshape(-1, 2))))
  slot = rs.permutation(len(keys) + 3)
  rows = np.zeros((V + len(keys) + 3, 2), np.float32)
  rows[:] = (rs.randint(0, 33, rows.shape) - 8) / 16.0           # decoys everywhere ...
  where = {}
  for k, key in enumerate(keys):
    rows[V + slot[k]] = key                                      # ... but in the rows in use
    where[key] = V + slot[k]
  idx = np.array([[where[tuple(c)] for c in f] for f in corner_uv], np.int32)
  assert not (idx == faces).any() and len(rows) > V
  return rows, idx


def _c(i):
  """lattice coordinate of pixel centre i (half-pixel units h: _c(h / 2))"""
  return 16 * i + 8


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def _small_grid(m, i0, j0, n, w=1, leg=1, seed=0):
  """n x n cells of `leg` px, corners on pixel centres, each split by a diagonal whose direction alternates: right triangles with the right angle in
  all four corners, both windings, all three vertex rotations"""
  k = 0
  for j in range(n):
    for i in range(n):
      a, b = (_c(i0 + leg * i), _c(j0 + leg * j)), (_c(i0 + leg * (i + 1)), _c(j0 + leg * j))
      c, d = (_c(i0 + leg * (i + 1)), _c(j0 + leg * (j + 1))), (_c(i0 + leg * i), _c(j0 + leg * (j + 1)))
      pair = ((a, b, c), (a, c, d)) if (i + j) % 2 == 0 else ((a, b, d), (b, c, d))
      for t in pair:
        m.tri(*t, w=w, flip=(k // 3 + seed) % 2 == 1, rot=(k + seed) % 3)
        k += 1


def _case_centres_small():
  m = _Mesh()
  _small_grid(m, 20, 26, 12)
  return _finish('centres_small', m, dict(classes={'small'}, only_classes=True, on_edge=200))


def _medium_shapes():
  """(triangle in half-pixel units, odd = pixel centre): bounding boxes at least 5 wide, at most 32 candidates; slopes 0, inf, +-1, +-1/2, +-2"""
  base = [((1, 1), (15, 1), (15, 7)), ((1, 1), (15, 7), (1, 7)),                # 7 x 3 px rectangle on centres, split: slopes 0, inf, 3/7
          ((1, 7), (13, 7), (7, 13)), ((1, 7), (7, 1), (13, 7)),                # diamond halves: slopes +-1 and 0
          ((1, 1), (11, 1), (17, 4)), ((1, 1), (17, 4), (7, 4)),                # slope 1/2 parallelogram, two vertices on half-pixel points
          ((1, 1), (9, 1), (5, 9)),                                             # slopes +-2
          ((2, 2), (12, 2), (12, 8)), ((0, 3), (10, 3), (4, 6))]                # vertices on half-pixel points (pixel corners / edges)
  return base


def _case_centres_medium():
  m = _Mesh()
  k = 0
  for s, tri in enumerate(_medium_shapes()):
    for mirror in (False, True):
      ox, oy = (k % 3) * 20 + 2, (k // 3) * 10 + 1           # tile origin, px
      pts = [((16 - x if mirror else x), y) for x, y in tri]
      pts = [(8 * (px + 2 * ox), 8 * (py + 2 * oy)) for px, py in pts]
      m.tri(*pts, flip=k % 2 == 1, rot=k % 3)
      k += 1
  return _finish('centres_medium', m, dict(classes={'medium'}, only_classes=True, on_edge=60), AB=(0.5, 1))


def _combs(m, w=1, far=None):
  """two interlocking combs of 90-px teeth (slope +-1/16, every edge through pixel centres) that tile the window"""
  L = lambda j: (-200, 8 - 180 + 180 * j)
  R = lambda j: (1240, 8 - 90 + 180 * j)
  for j in range(0, 9):
    m.tri(L(j), L(j + 1), R(j), w=w, flip=j % 2 == 1, rot=j % 3)
    m.tri(R(j - 1), R(j), L(j), w=w, flip=j % 2 == 0, rot=(j + 1) % 3)


def _fan(m, w=2):
  A = (-520, -120)
  for k in range(12):
    m.tri(A, (1016, -120 + 96 * k), (1016, -120 + 96 * (k + 1)), w=w, flip=k % 2 == 1, rot=k % 3)


def _case_large32():
  m = _Mesh()
  _combs(m)
  _fan(m)
  order = np.random.RandomState(5).permutation(len(m.f))
  return _finish('large32', m, dict(classes={'large'}, only_classes=True, on_edge=60, tiles=True), AB=(0.5, 1), order=order,
                 shifts=[(0, 0), (32, -32), (-64, 32), (96, 64), (-32, -96)])


def _case_far64(far):
  """Teeth with ONE vertex pushed out along a horizontal / vertical edge (through pixel centres) to |X| or |Y| = far, in both directions, and a
  background triangle with all three vertices out there: far = 16383 packs into int16 (list B, 32-bit), 16384 does not (RB_SLOW, 64-bit)."""
  m = _Mesh()
  for j in range(16):          # w = 1 (z/w 0.5): horizontal teeth 4 px high, far vertex to the right / left alternately
    y0, y1 = _c(4 * j), _c(4 * j + 4)
    if j % 2 == 0:                                       # horizontal lower edge, interior above it
      m.tri((-8, y0), (far, y0), (-8, y1), w=1, flip=j % 4 == 2, rot=j % 3)
    else:                                                # horizontal upper edge, interior below it
      m.tri((1032, y1), (-far, y1), (1032, y0), w=1, flip=j % 4 == 3, rot=j % 3)
  for i in range(8):           # w = 2 (z/w 0): vertical teeth 4 px wide in the right half, far vertex up / down
    x0, x1 = _c(32 + 4 * i), _c(36 + 4 * i)
    if i % 2 == 0:                                       # vertical edge with the interior to its right
      m.tri((x0, -8), (x0, far), (x1, -8), w=2, flip=i % 4 >= 2, rot=i % 3)
    else:                                                # ... to its left
      m.tri((x1, 1032), (x1, -far), (x0, 1032), w=2, flip=i % 4 >= 2, rot=i % 3)
  m.tri((-far, -far), (far, -far), (8, far), w=4)        # z/w -0.25: nearest wherever it covers... and it covers the whole window
  m.tri((-far, far), (far, far), (8, -far + 16), w=8, flip=True)  # z/w -0.375
  order = np.random.RandomState(6).permutation(len(m.f))
  cls = {'large'} if far < 16384 else {'slow'}
  # (no translations: they would carry the far vertices across the packing boundary this case is about)
  return _finish('far64_%d' % far, m, dict(classes=cls, only_classes=far >= 16384, on_edge=40), AB=(0.5, 1), order=order, shifts=[(0, 0)] * 5)


_POLY = [(8, 4), (30, 1), (51, 6), (60, 20), (57, 41), (44, 57), (22, 60), (7, 49), (1, 30), (2, 14)]       # convex, half-pixel units / 2: px
_POLY_W = [1, 2, 4, 1, 2, 1, 4, 2, 1, 2]


def _tessellations():
  n = len(_POLY)
  fan = [(0, i, i + 1) for i in range(1, n - 1)]
  strip, lo, hi, k = [], 0, n - 1, 0
  a, b = 0, n - 1
  lo, hi = 1, n - 2
  while lo <= hi:
    if k % 2 == 0:
      strip.append((a, lo, b)); a = lo; lo += 1
    else:
      strip.append((a, hi, b)); b = hi; hi -= 1
    k += 1
  rs = np.random.RandomState(11)
  ring, ear = list(range(n)), []
  while len(ring) > 3:
    i = rs.randint(len(ring))
    ear.append((ring[i - 1], ring[i], ring[(i + 1) % len(ring)]))
    ring.pop(i)
  ear.append(tuple(ring))
  return dict(fan=fan, strip=strip, ear=ear)


def _case_tiling(kind, permuted):
  m = _Mesh()
  vid = [m.vert(_c(x) if i % 2 == 0 else 16 * x, _c(y) if i % 3 != 1 else 16 * y, _POLY_W[i]) for i, (x, y) in enumerate(_POLY)]
  tris = _tessellations()[kind]
  assert len(tris) == len(_POLY) - 2
  for k, t in enumerate(tris):
    t = [vid[i] for i in t]
    if permuted:
      t = t[k % 3:] + t[:k % 3]
      if k % 2 == 0:
        t = [t[0], t[2], t[1]]
    m.f.append(tuple(t))
  order = list(range(len(tris)))[::-1] if permuted else None
  return _finish('tiling_%s%s' % (kind, '_perm' if permuted else ''), m, dict(classes=set(), on_edge=4, polygon=True), AB=(0, 0.25), order=order,
                 shifts=[(0, 0), (16, 16), (-32, 16), (48, -16), (-16, 32)])


def _case_ties_zero(reverse):
  """everything at w = 2, z/w = 0 exactly: interpolated depth is exactly 0 on every face, so every overlap is an exact tie"""
  m = _Mesh()
  big = ((_c(2), _c(2)), (_c(50), _c(6)), (_c(10), _c(58)))
  m.tri(*big, w=2)                                                       # large
  _small_grid(m, 8, 8, 4, w=2)                                           # small ones inside it
  m.tri(*big, w=2, flip=True, rot=1)                                     # the same triangle again, other winding
  m.tri((_c(20), _c(1)), (_c(62), _c(30)), (_c(30), _c(40)), w=2)        # partial overlaps, large
  m.tri((_c(12), _c(12)), (_c(19), _c(12)), (_c(19), _c(15)), w=2)       # medium inside
  m.tri((_c(12), _c(12)), (_c(19), _c(12)), (_c(19), _c(15)), w=2, rot=2)
  _small_grid(m, 30, 20, 3, w=2, leg=2, seed=1)
  m.tri((_c(25), _c(15)), (_c(45), _c(20)), (_c(28), _c(36)), w=2, flip=True)
  order = list(range(len(m.f)))[::-1] if reverse else None
  return _finish('ties_zero' + ('_rev' if reverse else ''), m, dict(classes={'small', 'medium', 'large'}, ties=300), AB=(0.5, 1), order=order,
                 shifts=[(0, 0), (32, -32), (-64, 32), (96, 64), (-32, -96)])


def _layers(m, ws, seed, n=4):
  """overlapping layers of 2-px right triangles on centres (barycentrics 0, 1/2, 1: exact float depth), one per w, each shifted by 2 px"""
  for k, w in enumerate(ws):
    _small_grid(m, 10 + 4 * k, 12 + 2 * k, n, w=w, leg=2, seed=seed + k)          # 3 x 3 candidates: medium
    _small_grid(m, 44 + k, 6 + k, 4, w=w, leg=1, seed=seed + k)                   # 2 x 2 candidates: small


def _case_depth_signs(kind):
  m = _Mesh()
  if kind == 'mixed':                        # z/w = 1/w - 0.5: 1.5 (clipped), 0.5, 0, -0.25, -0.375
    AB, ws = (0.5, 1), [Fr(1, 2), 1, 2, 4, 8]
    m.tri((_c(1), _c(1)), (_c(33), _c(1)), (_c(1), _c(33)), w=4)        # power-of-two area (exact depth), large: -0.25
    m.tri((_c(30), _c(30)), (_c(62), _c(30)), (_c(62), _c(62)), w=1, flip=True)        # 0.5
  elif kind == 'ulp_pos':                    # 0.5 + 2^-22, + 2^-23, + 2^-24 (adjacent floats)
    AB, ws = (-0.5, 2.0 ** -22), [1, 2, 4]
  elif kind == 'ulp_neg':                    # -0.5 + 2^-23, + 2^-24, + 2^-25 (adjacent floats)
    AB, ws = (0.5, 2.0 ** -23), [1, 2, 4]
  else:                                      # around zero: 2^-24, 0, -2^-25, -2^-25 - 2^-26
    AB, ws = (2.0 ** -24, 2.0 ** -23), [1, 2, 4, 8]
  _layers(m, ws, seed=len(kind))
  order = np.random.RandomState(len(kind)).permutation(len(m.f))
  return _finish('depth_signs_' + kind, m, dict(classes={'small', 'medium'}, layers=len(ws) - (kind == 'mixed'), exact_depth=kind != 'mixed'), AB=AB, order=order,
                 shifts=[(0, 0), (128, -128), (-128, 256), (256, 128), (-256, -128)])


def _case_zclip(kind):
  m = _Mesh()
  if kind in ('hi', 'lo'):                   # w = 1: one ulp outside; w = 2: exactly +-1; w = 4: one ulp (of the binade below) inside
    s = 1 if kind == 'hi' else -1
    AB = (s * (2.0 ** -23 - 1), s * 2.0 ** -22)
    _layers(m, [1, 2, 4], seed=3)
    m.tri((_c(30), _c(1)), (_c(62), _c(1)), (_c(62), _c(33)), w=2)        # power-of-two area at exactly +-1: kept, large
    order = np.random.RandomState(9).permutation(len(m.f))
    return _finish('zclip_' + kind, m, dict(classes={'small', 'medium', 'large'}, exact_depth=True, dropped=True), AB=AB, order=order,
                   shifts=[(0, 0), (128, -128), (-128, 256), (256, 128), (-256, -128)])
  # slanted: z/w = 1.5 / w: 1.5, 0.75, 0.375 at the vertices - crosses +1 inside each triangle; general w makes u, v perspective-correct
  AB = (0, 1.5)
  m.tri((_c(2), _c(3), 1), (_c(58), _c(9), 2), (_c(20), _c(60), 4))
  m.tri((_c(40), _c(40), 4), (_c(47), _c(41), 1), (_c(42), _c(44), 2), flip=True)
  m.tri((_c(50), _c(50), 2), (_c(52), _c(50), 1), (_c(50), _c(52), 4))
  m.tri((_c(44), _c(60), 2), (_c(62), _c(60), 2), (_c(62), _c(48), 1), rot=1)
  return _finish('zclip_slant', m, dict(classes={'large'}, band=True, general_w=True), AB=AB,
                 shifts=[(0, 0), (64, -64), (-64, 64), (64, 64), (-64, 0)])


def _junk(m, k):
  """one face that covers nothing, kind k (cycled): repeated index, collinear, snaps to zero area, sub-pixel without a centre, outside each of the
  four sides"""
  k = k % 8
  if k == 0:
    a, b = m.vert(_c(5), _c(5)), m.vert(_c(9), _c(7))
    m.f.append((a, b, a))
  elif k == 1:
    m.tri((_c(3), _c(3)), (_c(13), _c(8)), (_c(23), _c(13)))
  elif k == 2:
    m.tri((_c(6), _c(6)), (_c(16), _c(6) + Fr(1, 4)), (_c(26), _c(6) - Fr(1, 4)))        # non-degenerate in float, zero area after the snap
  elif k == 3:
    m.tri((16 * 7 + 1, 16 * 9 + 1), (16 * 7 + 7, 16 * 9 + 2), (16 * 7 + 3, 16 * 9 + 7))  # inside one pixel, short of its centre
  elif k == 4:
    m.tri((-400, _c(5)), (-120, _c(20)), (-200, _c(40)))
  elif k == 5:
    m.tri((1130, _c(5)), (1400, _c(20)), (1200, _c(40)))
  elif k == 6:
    m.tri((_c(5), -400), (_c(20), -109), (_c(40), -200))
  else:
    m.tri((_c(5), 1125), (_c(20), 1400), (_c(40), 1200))


def _case_degenerate():
  m = _Mesh()
  real = []
  k = 0

  def add(*a, **kw):
    nonlocal k
    _junk(m, k); k += 1
    real.append(m.tri(*a, w=2, **kw))
  g = _Mesh()
  _small_grid(g, 24, 24, 5)
  for f in g.f:
    add(*[g.v[i][:2] for i in f])
  add((-100, _c(10)), (_c(12), _c(4)), (_c(12), _c(20)))                  # partly outside, left
  add((_c(50), _c(50)), (1200, _c(55)), (_c(55), 1200), flip=True)        # partly outside, right and top
  add((_c(30), -200), (_c(45), _c(6)), (_c(20), _c(9)))                   # partly outside, bottom
  add((0, _c(30)), (_c(6), _c(33)), (0, _c(40)))                          # vertices exactly on the window border
  add((1024, 1024), (_c(60), _c(50)), (_c(50), _c(60)))
  # vertices off the lattice: 1/4 unit either side of a pixel centre / corner, also at negative coordinates (the snap is round-half-even)
  add((_c(40) - Fr(1, 4), _c(10) + Fr(1, 4)), (_c(47) + Fr(1, 4), _c(10) - Fr(1, 4)), (_c(40) + Fr(1, 4), _c(17) - Fr(1, 4)))
  add((_c(40) + Fr(3, 4) - 1, _c(20) - Fr(3, 4) + 1), (_c(46) - Fr(1, 4), _c(20) + Fr(1, 4)), (_c(46) + Fr(1, 4), _c(24) + Fr(3, 4) - 1), flip=True)
  add((-8 - Fr(3, 4), _c(44) - Fr(1, 4)), (_c(9) + Fr(1, 4), _c(44) + Fr(1, 4)), (-8 + Fr(1, 4), _c(50) - Fr(3, 4) + 1))
  for _ in range(8):
    _junk(m, k); k += 1
  return _finish('degenerate', m, dict(classes={'small'}, junk=True, on_edge=30), AB=(0.5, 1), real=real)


def _case_window(kind):
  m = _Mesh()
  if kind == 'zoom':                         # a 32 x 32 frame window onto 64 x 64: t00 = t11 = 2
    bbox, out = (16, 16, 48, 48), (64, 64)
  elif kind == 'half_out':                   # a window half outside the frame
    bbox, out = (-16, 8, 16, 40), (64, 64)
  else:                                      # 48 x 160 output of the whole frame: the lattice is multiples of 5 (x) and 3 (y)
    bbox, out = None, (48, 160)
  if kind == 'wide':
    X = lambda i: 5 * 8 * i                  # 2.5-px steps; centres where 40 i = 16 p + 8
    Y = lambda j: 3 * 8 * j                  # 1.5-px steps
    for j in range(0, 30, 6):
      for i in range(0, 60, 4):                # 5 x 4.5 px cells: at most 6 x 5 candidates
        a, b, c, d = (X(i + 1), Y(j + 1)), (X(i + 3), Y(j + 1)), (X(i + 3), Y(j + 4)), (X(i + 1), Y(j + 4))
        m.tri(a, b, c, w=1, flip=(i + j) % 2 == 1)
        m.tri(a, c, d, w=1, rot=(i // 4) % 3)
    m.tri((X(1), Y(1)), (X(61), Y(3)), (X(3), Y(31)), w=2)
    return _finish('window_wide', m, dict(classes={'medium', 'large'}, on_edge=10), AB=(0.5, 1), out=out,
                   shifts=[(0, 0), (30, -30), (-60, 30), (90, 60), (-30, -90)])
  _small_grid(m, 6, 6, 5, w=2)
  for k, tri in enumerate(_medium_shapes()):
    ox, oy = (k % 3) * 20 + 2, 20 + (k // 3) * 12
    m.tri(*[(8 * (x + 2 * ox), 8 * (y + 2 * oy)) for x, y in tri], w=1, flip=k % 2 == 1)
  m.tri((_c(2), _c(2)), (_c(60), _c(8)), (_c(8), _c(60)), w=4)
  return _finish('window_' + kind, m, dict(classes={'small', 'medium', 'large'}, on_edge=30), AB=(0.5, 1), bbox=bbox, out=out,
                 shifts=[(0, 0), (128, -128), (-128, 256), (256, 128), (-256, -128)])


# ---- textured and lit cases (SHADE_CASES): not part of BASE_CASES / ALL_CASES, whose fill-rule and path claims they do not make ------------------
def _quad(m, x0, y0, x1, y1, w=(1, 1, 1, 1)):
  """axis-parallel quad of four SHARED vertices a (x0, y0), b (x1, y0), c (x1, y1), d (x0, y1) (lattice units, rows bottom-up), faces (a, b, c), (a, c, d)"""
  a, b, c, d = m.vert(x0, y0, w[0]), m.vert(x1, y0, w[1]), m.vert(x1, y1, w[2]), m.vert(x0, y1, w[3])
  m.f += [(a, b, c), (a, c, d)]
  return a, b, c, d


def _quad_uv(u0, v0, u1, v1):
  """corner uv of _quad's two faces: (u0, v1) at a (bottom left) ... (u0, v0) at d (top left): v grows DOWN the image, like the texture's rows"""
  a, b, c, d = (u0, v1), (u1, v1), (u1, v0), (u0, v0)
  return [(a, b, c), (a, c, d)]


def _distinct_texture(Ht, Wt, seed):
  """every texel and channel distinct, dyadic (k / 512), inside [1/4, 1): exact half / quarter blends, and no value so small that one fp16 ulp of
  the network tensor falls below the float32 error of the fetch"""
  n = Ht * Wt * 3
  assert n <= 384
  k = 128 + np.random.RandomState(seed).permutation(384)[:n]
  return (k / 512.0).reshape(Ht, Wt, 3).astype(np.float32)


def _case_tex_grid(name, Ht, Wt, px_w, px_h, periods, half):
  """A w = 1 quad of px_w x px_h pixels showing `periods` repeats of an Ht x Wt texture each way, px_w = periods Wt and px_h = periods Ht: a
  pixel step is a texel step.  half = 0: corners on pixel CORNERS, every pixel centre is a texel centre (the texel itself); half = 1: corners on
  pixel CENTRES, every pixel centre is a texel corner (the mean of four texels, the column left of u = 0 being the last one).  Power-of-two legs
  make the barycentrics, u, v and the fetch position exact in float32 (claims['exact'])."""
  assert px_w == periods * Wt and px_h == periods * Ht
  m = _Mesh()
  i0, j0 = (64 - px_w) // 2, (64 - px_h) // 2
  x0, y0 = 16 * i0 + 8 * half, 16 * j0 + 8 * half
  _quad(m, x0, y0, x0 + 16 * px_w, y0 + 16 * px_h)
  pow2 = (px_w & (px_w - 1)) == 0 and (px_h & (px_h - 1)) == 0
  return _finish(name, m, dict(exact=pow2, grid=(i0, j0, px_w, px_h, half)), tex=_distinct_texture(Ht, Wt, Ht * 100 + Wt),
                 corner_uv=_quad_uv(0, 0, periods, periods))


def _case_tex_wrap(name, Ht, Wt, offset=(0, 0)):
  """uv from -1.25 to 2.25 both ways over 56 px between pixel centres 4 and 60: 1/16 of a period per pixel, so the centres 24 and 40 lie exactly on
  u = 0 and u = 1 (x = -0.5: the last column blended with the first) and likewise on v.  `offset`: whole periods added to every uv (the host
  test's periodicity check)."""
  m = _Mesh()
  _quad(m, _c(4), _c(4), _c(60), _c(60))
  du, dv = offset
  return _finish(name, m, dict(wrap=True), tex=_distinct_texture(Ht, Wt, Ht * 100 + Wt), corner_uv=_quad_uv(-1.25 + du, -1.25 + dv, 2.25 + du, 2.25 + dv))


def _case_tex_charts():
  """Two triangles over the diagonal a - c of one quad, each addressing a chart of its own in a 16 x 16 texture of distinct texels: the shared
  vertices a and c have different uv rows in the two faces (no per-vertex uv exists), the charts differ in place, size and orientation."""
  m = _Mesh()
  _quad(m, _c(8), _c(6), _c(56), _c(54), w=(1, 2, 1, 2))
  rs = np.random.RandomState(77)
  tex = (rs.permutation(768).reshape(16, 16, 3) / 1024.0 + 0.25).astype(np.float32)
  uv = [((1 / 16, 1 / 16), (7 / 16, 2 / 16), (6 / 16, 7 / 16)), ((15 / 16, 9 / 16), (9 / 16, 15 / 16), (9 / 16, 10 / 16))]
  return _finish('tex_charts', m, dict(charts=True), AB=(0.5, 1), tex=tex, corner_uv=uv)


ATLAS_T, ATLAS_C = 16, 8           # the atlas of include/foundationpose_amd.h for 8 faces: g = 2, cells of c = 8 texels, m = c - 3 = 5


def atlas_face_colors():
  return np.array([[(f + 1) / 16.0, (16 - f) / 32.0, ((5 * f) % 8 + 1) / 8.0] for f in range(8)], np.float32)


def _case_tex_atlas():
  """Eight faces with the uv and texel ownership of the texture bake's atlas rule (restated from the header): cell k = faces 2k (A: corners at texel
  centres (0,0), (m,0), (0,m) of the cell, owns i + j <= c - 2) and 2k + 1 (B: (c-1,c-1), (c-1-m,c-1), (c-1,c-1-m), owns i + j >= c); every owned
  texel holds its face's colour, everything else 0.  General w, so that the interpolated uv carries its float32 rounding."""
  T, c = ATLAS_T, ATLAS_C
  mm, g = c - 3, T // c
  col = atlas_face_colors()
  tex = np.zeros((T, T, 3), np.float32)
  m = _Mesh()
  uv = []
  ws = [1, 2, 4, 2, 1, 4, 2, 1, 2]
  grid = [[m.vert(_c(6 + 25 * i), _c(5 + 26 * j), ws[3 * j + i]) for i in range(3)] for j in range(3)]
  for k in range(4):
    ci, cj = (k % g) * c, (k // g) * c
    for j in range(c):
      for i in range(c):
        if i + j <= c - 2:
          tex[cj + j, ci + i] = col[2 * k]
        elif i + j >= c:
          tex[cj + j, ci + i] = col[2 * k + 1]
    ctr = lambda i, j: ((ci + i + 0.5) / T, (cj + j + 0.5) / T)
    uv += [(ctr(0, 0), ctr(mm, 0), ctr(0, mm)), (ctr(c - 1, c - 1), ctr(c - 1 - mm, c - 1), ctr(c - 1, c - 1 - mm))]
    gi, gj = k % 2, k // 2
    a, b, cc, d = grid[gj][gi], grid[gj][gi + 1], grid[gj + 1][gi + 1], grid[gj + 1][gi]
    m.f += [(a, b, cc), (cc, d, a)] if k % 2 == 0 else [(b, cc, d), (d, a, b)]
  return _finish('tex_atlas', m, dict(atlas=True), AB=(0.5, 1), tex=tex, corner_uv=uv)


def _case_tex_perspective():
  """A slanted quad, w = 1 on its left and 4 on its right edge (zclip_slant's w layout: 1, 2, 4 at general positions, here on shared vertices), with
  a 16 x 16 checker whose neighbours differ by 1/2: u interpolated affinely would be off by up to 16 (1/2 - 1/5) = 4.8 texels.  One more face has a
  vertex 1300 px to the right (list B, the 64-bit record form)."""
  m = _Mesh()
  a, b, c, d = m.vert(_c(4), _c(8), 1), m.vert(_c(52), _c(4), 4), m.vert(_c(56), _c(40), 4), m.vert(_c(6), _c(36), 1)
  m.f += [(a, b, c), (a, c, d)]
  m.tri((_c(8), _c(58), 1), (_c(28), _c(46), 2), (_c(1300), _c(62), 4))
  rr, cc = np.mgrid[0:16, 0:16]
  tex = ((0.25 + 0.5 * ((rr + cc) % 2))[..., None] * np.array([1.0, 0.5, 0.75])).astype(np.float32)
  uv = _quad_uv(0, 0, 1, 1) + [((0, 0), (0.5, 0.25), (1, 1))]
  return _finish('tex_perspective', m, dict(general_w=True), AB=(0.5, 1), tex=tex, corner_uv=uv, shifts=[(0, 0), (64, -64), (-64, 64), (64, 64), (-64, 0)])


LIT_ROT = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float32)          # 120 degrees about (1, 1, 1): exact, moves every axis, R != R^T


def _case_lit(textured):
  """A 2 x 2 grid of quads on nine shared vertices (w 1 and 2 alternating), posed with LIT_ROT.  Camera-space normals (4, y, z) / 4 with |y|, |z| <= 3:
  not unit length, different at every vertex, z of either sign (the default light's Lambert term -n_z / |n| is clipped at 0 for about half of them),
  any two at most 94 degrees apart, so an interpolated normal is never shorter than 0.68 of its vertices' (the normal map stays well conditioned)."""
  m = _Mesh()
  ws = [1, 2, 1, 2, 1, 2, 1, 2, 1]
  grid = [[m.vert(_c(5 + 26 * i), _c(7 + 25 * j), ws[3 * j + i]) for i in range(3)] for j in range(3)]
  uv = []
  for j in range(2):
    for i in range(2):
      a, b, c, d = grid[j][i], grid[j][i + 1], grid[j + 1][i + 1], grid[j + 1][i]
      m.f += [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
      q = _quad_uv(i - 0.5, j - 0.75, i + 0.5, j + 0.25)
      uv += q if (i + j) % 2 == 0 else [(q[0][0], q[0][1], q[1][2]), (q[0][1], q[0][2], q[1][2])]
  yz = [(0, -3), (2, 3), (-3, -1), (3, 2), (-1, -2), (-2, 3), (1, 1), (3, -3), (-3, 2)]
  ncam = np.array([(4, y, z) for y, z in yz], np.float32) / 4
  kw = dict(tex=_distinct_texture(8, 8, 88), corner_uv=uv) if textured else {}
  return _finish('lit_tex' if textured else 'lit_vcol', m, dict(lit=True), AB=(0.5, 1), normals_cam=ncam, rot=LIT_ROT, **kw)


LIGHTS = {            # name -> nvdiffrast_render's light arguments (use_light = True)
    'default': dict(),
    'dir': dict(light_dir=(0.5, -1.0, 1.0)),
    'pos': dict(light_dir=None, light_pos=(0.5, -0.25, 0.25)),
    'default_color': dict(light_color=(1.0, 0.75, 0.5)),
    'dir_color': dict(light_dir=(0.5, -1.0, 1.0), light_color=(1.0, 0.75, 0.5)),
    'pos_color': dict(light_dir=None, light_pos=(0.5, -0.25, 0.25), light_color=(1.0, 0.75, 0.5)),
    'bright': dict(w_ambient=0.9, w_diffuse=0.9),          # 0.9 base (1 + d) > 1 wherever base (1 + d) > 1.12: the final clip acts
}

_SHADE_BUILDERS = {
    'tex_identity': lambda: _case_tex_grid('tex_identity', 8, 16, 32, 16, 2, 0),
    'tex_identity_5x7': lambda: _case_tex_grid('tex_identity_5x7', 5, 7, 21, 15, 3, 0),
    'tex_corners': lambda: _case_tex_grid('tex_corners', 8, 16, 32, 16, 2, 1),
    'tex_wrap': lambda: _case_tex_wrap('tex_wrap', 4, 8),
    'tex_wrap_shifted': lambda: _case_tex_wrap('tex_wrap_shifted', 4, 8, offset=(-1, -1)),          # host only: equals tex_wrap
    'tex_thin_1x1': lambda: _case_tex_wrap('tex_thin_1x1', 1, 1), 'tex_thin_1x6': lambda: _case_tex_wrap('tex_thin_1x6', 1, 6),
    'tex_thin_6x1': lambda: _case_tex_wrap('tex_thin_6x1', 6, 1),
    'tex_charts': _case_tex_charts, 'tex_atlas': _case_tex_atlas, 'tex_perspective': _case_tex_perspective,
    'lit_vcol': lambda: _case_lit(False), 'lit_tex': lambda: _case_lit(True),
}
TEX_CASES = ['tex_identity', 'tex_identity_5x7', 'tex_corners', 'tex_wrap', 'tex_thin_1x1', 'tex_thin_1x6', 'tex_thin_6x1', 'tex_charts', 'tex_atlas',
             'tex_perspective']
LIT_CASES = ['lit_vcol', 'lit_tex']
SHADE_CASES = TEX_CASES + LIT_CASES


def shade_variants(name):
  """the light settings a case is rendered with: None (use_light = False) for the texture cases, every entry of LIGHTS for the lit ones"""
  return sorted(LIGHTS) if name in LIT_CASES else [None]


def plan_restated(N, V, F, Ho, Wo, num_cu=256):
  """The launch plan of the rasteriser (strips, face ranges, one-launch form), restated: dict(S, strip_rows, lds_verts, G, Fg, solo)."""
  budget = 148 * 1024
  lds_verts = V * 8 <= 64 * 1024
  a_lds = ((V * 8 + 15) & ~15) if lds_verts else 0
  rows_max = (budget - a_lds - 16) // (Wo * 10)
  rows_max = max(1, min(rows_max, Ho))
  S = (Ho + rows_max - 1) // rows_max
  while S < 4 and Ho // (S * 2) >= 8:
    S *= 2
  while N * S * 5 <= num_cu * 4 and S < 16 and Ho // (S * 2) >= 8:
    S *= 2
  rows = (Ho + S - 1) // S
  S = (Ho + rows - 1) // rows
  G = 1
  while N * G * 4 <= num_cu and G < 8 and F // (G * 2) >= 1024:
    G *= 2
  solo_lds = ((rows * Wo * 8 + ((rows * Wo * 2 + 15) & ~15) + ((V + 1) & ~1) * 8 + 15) & ~15) + 2 * ((F + 7) & ~7) * 2
  return dict(S=S, strip_rows=rows, lds_verts=lds_verts, G=G, Fg=(F + G - 1) // G, solo=N <= 2 and lds_verts and F <= 65535 and solo_lds <= budget)


def solo_face_limit(V, Ho=64, Wo=64):
  """largest F that still takes the one-launch form for one hypothesis"""
  F = 65535
  while not plan_restated(1, V, F, Ho, Wo)['solo']:
    F -= 1
  return F


def _case_padded(base, F, V=None):
  """`base` with off-window and degenerate faces and unused vertices added up to F faces (and V vertices); the real faces sit at ids Fg - 1 and Fg of
  every face range the classification may be cut into (G = 2, 4, 8), at the last id, and spread over the rest.  claims['remap'][i] = id of base face i."""
  b = lattice_case(base)
  nb = len(b['faces'])
  m = _Mesh()
  m.v = [(Fr(x), Fr(y), Fr(w)) for x, y, w in zip(b['Xq'], b['Yq'], b['w'])]
  v0 = len(m.v)
  while len(m.v) < max(V or 0, v0 + 24):                # unused / off-window vertices
    i = len(m.v) - v0
    m.vert(-4000 - 16 * (i % 50), _c(i % 64))
  slots = []
  for G in (8, 4, 2):
    Fg = (F + G - 1) // G
    for g in range(1, G):
      slots += [g * Fg - 1, g * Fg]
  slots = sorted(set(slots + [F - 1, 0]))
  rest = [int(x) for x in np.linspace(1, F - 2, 3 * nb).astype(int) if x not in slots]
  assert len(slots) <= nb, (len(slots), nb)
  ids = sorted(slots + rest[:nb - len(slots)])
  assert len(ids) == nb and len(set(ids)) == nb, (len(ids), nb)
  # base face order preserved: the k-th real id holds base face k, so ties resolve the same way
  faces = np.zeros((F, 3), np.int32)
  pad = np.ones(F, bool)
  pad[ids] = False
  pi = np.flatnonzero(pad)
  a = v0 + (pi % 20)
  kind = pi % 3
  faces[pi, 0] = a
  faces[pi, 1] = np.where(kind == 0, a, a + 1)          # repeated index | off-window triangle | off-window collinear
  faces[pi, 2] = np.where(kind == 1, a + 3, a + 2)
  faces[ids] = b['faces']
  m.f = [tuple(int(x) for x in f) for f in faces]
  AB = None if b['projection_mat'] is None else (b['projection_mat'][2, 2], b['projection_mat'][2, 3])
  name = 'padded_%s_F%d%s' % (base, F, '_V%d' % V if V else '')
  c = _finish(name, m, dict(classes=b['claims']['classes'], base=base, remap=np.asarray(ids), F=F), AB=AB, real=ids, shifts=b['shifts'])
  c['mesh_tensors']['vertex_color'][:v0] = b['mesh_tensors']['vertex_color']          # the base's vertices keep their colours
  return c


def padded_cases():
  """name -> (base, F, V).  F >= 2048 / 4096 / 8192: G = 2 / 4 / 8 at five hypotheses; V > 8192: the A records stay in global memory (lds_verts == 0);
  'solo_max' / 'solo_over': the largest F that still takes the one-launch form at 64 x 64 with the base's vertices, and one above."""
  out = {}
  for base in ('centres_small', 'large32'):
    for F in (2048, 4096, 8192):
      out['padded_%s_F%d' % (base, F)] = (base, F, None)
  out['padded_large32_F2051_V8200'] = ('large32', 2051, 8200)
  out['padded_centres_small_F4099_V8200'] = ('centres_small', 4099, 8200)
  return out


_BUILDERS = {
    'centres_small': _case_centres_small, 'centres_medium': _case_centres_medium, 'large32': _case_large32,
    'far64_16383': lambda: _case_far64(16383), 'far64_16384': lambda: _case_far64(16384), 'far64_1600008': lambda: _case_far64(1600008),
    'ties_zero': lambda: _case_ties_zero(False), 'ties_zero_rev': lambda: _case_ties_zero(True),
    'depth_signs_mixed': lambda: _case_depth_signs('mixed'), 'depth_signs_ulp_pos': lambda: _case_depth_signs('ulp_pos'),
    'depth_signs_ulp_neg': lambda: _case_depth_signs('ulp_neg'), 'depth_signs_tiny': lambda: _case_depth_signs('tiny'),
    'zclip_hi': lambda: _case_zclip('hi'), 'zclip_lo': lambda: _case_zclip('lo'), 'zclip_slant': lambda: _case_zclip('slant'),
    'degenerate': _case_degenerate,
    'window_zoom': lambda: _case_window('zoom'), 'window_half_out': lambda: _case_window('half_out'), 'window_wide': lambda: _case_window('wide'),
}
for _k in ('fan', 'strip', 'ear'):
  for _p in (False, True):
    _BUILDERS['tiling_%s%s' % (_k, '_perm' if _p else '')] = (lambda k=_k, p=_p: _case_tiling(k, p))
BASE_CASES = sorted(_BUILDERS)
PADDED_CASES = sorted(padded_cases()) + ['padded_solo_max', 'padded_solo_over']
ALL_CASES = BASE_CASES + PADDED_CASES


@functools.lru_cache(maxsize=None)
def lattice_case(name):
  if name in _BUILDERS:
    return _BUILDERS[name]()
  if name in _SHADE_BUILDERS:
    return _SHADE_BUILDERS[name]()
  if name in ('padded_solo_max', 'padded_solo_over'):
    V = len(lattice_case('centres_small')['X']) + 24
    F = solo_face_limit(V) + (1 if name.endswith('over') else 0)
    c = dict(_case_padded('centres_small', F))
    c['name'] = name
    return c
  base, F, V = padded_cases()[name]
  return _case_padded(base, F, V)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------------
def hyp_lattice(case, h):
  """intended snapped integers of hypothesis h: the lattice moved by shift / w"""
  dx, dy = case['shifts'][h]
  X = np.rint(case['Xq'] + dx / case['w']).astype(np.int64)
  Y = np.rint(case['Yq'] + dy / case['w']).astype(np.int64)
  return X, Y


def transform_check(case):
  """The vertex transform of the documented camera model, restated in float64 (every step checked to be a dyadic rational of at most 24 bits, so the
  float32 transform cannot round) up to the unsnapped position; then the snap.  Returns per hypothesis (X, Y) and asserts they are the intended ones."""
  def ex(a, what):
    a = np.asarray(a, np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a), (case['name'], what)
    return a
  Ho, Wo = case['Ho'], case['Wo']
  pos = case['mesh_tensors']['pos'].astype(np.float64)
  if case['projection_mat'] is not None:
    P = case['projection_mat']
  else:
    zn, zf = 0.001, 100.0
    P = np.array([[2 * K[0, 0] / W, -2 * K[0, 1] / W, (-2 * K[0, 2] + W) / W, 0], [0, 2 * K[1, 1] / H, (2 * K[1, 2] - H) / H, 0],
                  [0, 0, -(zf + zn) / (zf - zn), -2 * zf * zn / (zf - zn)], [0, 0, -1, 0]])
  out = []
  for h in range(len(case['poses'])):
    pose = case['poses'][h].astype(np.float64)
    M = P @ (np.diag([1.0, -1.0, -1.0, 1.0]) @ pose)
    if case['bbox2d'] is not None:
      l, t, r, b = [float(x) for x in case['bbox2d'][h]]
      t, b = H - t, H - b
      r3 = M[3].copy()
      M[0] = W / (r - l) * M[0] + (W - r - l) / (r - l) * r3
      M[1] = H / (t - b) * M[1] + (H - t - b) / (t - b) * r3
    M = M.astype(np.float32).astype(np.float64)           # rounded once
    c = []
    for r in range(4):                                    # the fmaf chain, innermost first; every partial sum exact (row 2 of the default projection: pz = 0)
      s = ex(M[r, 2] * pos[:, 2] + M[r, 3], 'c%d inner' % r) if (r != 2 or case['projection_mat'] is not None) else M[r, 2] * pos[:, 2] + M[r, 3]
      s = ex(M[r, 1] * pos[:, 1] + s, 'c%d mid' % r)
      c.append(ex(M[r, 0] * pos[:, 0] + s, 'c%d' % r))
    assert np.all(c[3] > 0) and np.array_equal(c[3], case['w'])
    xn, yn, zw = ex(c[0] / c[3], 'xn'), ex(c[1] / c[3], 'yn'), ex(c[2] / c[3], 'zw')
    assert np.array_equal(zw, case['zw']), case['name']
    sx, sy = ex(xn * (Wo / 2) + Wo / 2, 'sx'), ex(yn * (Ho / 2) + Ho / 2, 'sy')
    assert np.abs(sx).max() <= 1e6 and np.abs(sy).max() <= 1e6
    X16, Y16 = ex(sx * 16, 'X'), ex(sy * 16, 'Y')
    dx, dy = case['shifts'][h]
    assert np.array_equal(X16, case['Xq'] + dx / case['w']) and np.array_equal(Y16, case['Yq'] + dy / case['w']), case['name']
    assert not np.any(np.abs(X16 - np.floor(X16) - 0.5) < 1e-9) and not np.any(np.abs(Y16 - np.floor(Y16) - 0.5) < 1e-9)      # no snap on a tie
    X, Y = np.rint(X16).astype(np.int64), np.rint(Y16).astype(np.int64)
    Xi, Yi = hyp_lattice(case, h)
    assert np.array_equal(X, Xi) and np.array_equal(Y, Yi)
    out.append((X, Y))
  return out


def _edges(case, h, XY=None):
  """raw (not sign-normalised) integers of the real faces: e (3, F, Ho, Wo) at every pixel centre, dx, dy (3, F), a (F,)"""
  X, Y = hyp_lattice(case, h) if XY is None else XY
  f = case['faces'][case['real']].astype(np.int64)
  Xs, Ys = X[f], Y[f]                                     # (F, 3)
  Px = (16 * np.arange(case['Wo'], dtype=np.int64) + 8)[None, None, :]
  Py = (16 * np.arange(case['Ho'], dtype=np.int64) + 8)[None, :, None]
  e, dxs, dys = [], [], []
  for k in range(3):
    p, q = (k + 1) % 3, (k + 2) % 3
    dx, dy = Xs[:, q] - Xs[:, p], Ys[:, q] - Ys[:, p]
    e.append(dx[:, None, None] * (Py - Ys[:, p][:, None, None]) - dy[:, None, None] * (Px - Xs[:, p][:, None, None]))
    dxs.append(dx), dys.append(dy)
  a = (Xs[:, 1] - Xs[:, 0]) * (Ys[:, 2] - Ys[:, 0]) - (Xs[:, 2] - Xs[:, 0]) * (Ys[:, 1] - Ys[:, 0])
  return np.stack(e), np.stack(dxs), np.stack(dys), a


def claims_exact(case, h, XY=None):
  """(F, Ho, Wo) bool: the centre displaced by (-eps, -eps^2) is strictly inside the face (module docstring); rows bottom-up"""
  e, dx, dy, a = _edges(case, h, XY)
  s = np.sign(a)[None, :, None, None]
  c0, c1, c2 = s * e, (s[..., 0, 0] * dy)[:, :, None, None], (-s[..., 0, 0] * dx)[:, :, None, None]
  pos = (c0 > 0) | ((c0 == 0) & ((c1 > 0) | ((c1 == 0) & (c2 > 0))))
  return pos.all(0) & (a != 0)[:, None, None]


def coverage_exact(case, h, XY=None):
  """dict, images top-down like the kernel's: face (Ho, Wo) winning face id or -1; zw its exact z/w; band: pixels where a face with interpolated
  (not constant) depth comes within TOL_UVZ of +-1 (zclip's stated exclusion; empty elsewhere); claims (F, Ho, Wo) bottom-up; lam (3, Ho, Wo) the
  winner's barycentrics e_k / a."""
  e, dx, dy, a = _edges(case, h, XY)
  cl = claims_exact(case, h, XY)
  f = case['faces'][case['real']]
  z = case['zw'][f]                                       # (F, 3)
  const = (z[:, 0] == z[:, 1]) & (z[:, 0] == z[:, 2])
  an = np.where(a == 0, 1, a).astype(np.float64)[:, None, None]
  lam = e.astype(np.float64) / an[None]
  zw = np.where(const[:, None, None], z[:, 0][:, None, None], (lam * z.T[:, :, None, None]).sum(0))
  band = (cl & ~const[:, None, None] & (np.abs(np.abs(zw) - 1) <= TOL_UVZ)).any(0)
  ok = cl & (zw >= -1) & (zw <= 1)
  key = np.where(ok, zw, np.inf)
  win = key.argmin(0)                                     # first minimum: the real faces are in ascending id order, so ties go to the lower id
  any_ok = ok.any(0)
  face = np.where(any_ok, case['real'][win], -1)
  zwin = np.where(any_ok, np.take_along_axis(key, win[None], 0)[0], 0.0)
  lamw = np.stack([np.take_along_axis(lam[k], win[None], 0)[0] for k in range(3)])
  return dict(face=face[::-1].copy(), zw=zwin[::-1].copy(), band=band[::-1].copy(), claims=cl, ok=ok, key=key, lam=lamw[:, ::-1].copy(), win=win[::-1].copy())


def _cam64(case, h):
  """camera-space vertex positions R p + t of hypothesis h in float64 (pts_cam, src/Utils.py:168)"""
  P = case['poses'][h].astype(np.float64)
  return case['mesh_tensors']['pos'].astype(np.float64) @ P[:3, :3].T + P[:3, 3]


def fetch_float64(tex, tu, tv):
  """dr.texture(filter_mode='linear'), wrap: texel (r, c) has its centre at uv = ((c + 0.5) / Wt, (r + 0.5) / Ht); x = u Wt - 0.5, y = v Ht - 0.5,
  bilinear over floor and floor + 1, every index modulo the size, weights the fractional parts.  tex (Ht, Wt, 3), row 0 first in memory; no v flip."""
  tex = np.asarray(tex, np.float64)
  Ht, Wt = tex.shape[:2]
  x, y = np.asarray(tu, np.float64) * Wt - 0.5, np.asarray(tv, np.float64) * Ht - 0.5
  x0, y0 = np.floor(x), np.floor(y)
  fx, fy = (x - x0)[..., None], (y - y0)[..., None]
  c0, r0 = np.mod(x0, Wt).astype(np.int64), np.mod(y0, Ht).astype(np.int64)
  c1, r1 = (c0 + 1) % Wt, (r0 + 1) % Ht
  return (1 - fy) * ((1 - fx) * tex[r0, c0] + fx * tex[r0, c1]) + fy * ((1 - fx) * tex[r1, c0] + fx * tex[r1, c1])


def _base64(case, uvw, vid, tri):
  """unlit colour before the clip: the texture at the perspective-correct uv[uv_idx[face]] (src/Utils.py:186-187) or the vertex-colour blend (:189)"""
  mt = case['mesh_tensors']
  if 'tex' not in mt:
    return (uvw[..., None] * mt['vertex_color'].astype(np.float64)[vid]).sum(-2)
  texc = (uvw[..., None] * mt['uv'].astype(np.float64)[mt['uv_idx'][tri]]).sum(-2)
  return fetch_float64(mt['tex'][0], texc[..., 0], texc[..., 1])


def _fma32(a, b, c):
  return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _base32(case, u, v, w2, vid, tri):
  """float32, in the documented order: texc = fmaf(u, uv0, fmaf(v, uv1, w2 uv2)); x = texc Wt - 0.5 (product rounded, then the difference); floor,
  fx = x - floor; indices modulo the size; ta = t00 + fx (t10 - t00), tb = t01 + fx (t11 - t01), colour = ta + fy (tb - ta), every operation rounded."""
  f32 = np.float32
  mt = case['mesh_tensors']
  if 'tex' not in mt:
    vc = mt['vertex_color'][vid]
    return np.stack([_fma32(u, vc[..., 0, c], _fma32(v, vc[..., 1, c], w2 * vc[..., 2, c])) for c in range(3)], -1)
  tex = mt['tex'][0]
  Ht, Wt = tex.shape[:2]
  t = mt['uv'][mt['uv_idx'][tri]]                          # (Ho, Wo, 3, 2)
  tu = _fma32(u, t[..., 0, 0], _fma32(v, t[..., 1, 0], w2 * t[..., 2, 0]))
  tv = _fma32(u, t[..., 0, 1], _fma32(v, t[..., 1, 1], w2 * t[..., 2, 1]))
  x, y = tu * f32(Wt) - f32(0.5), tv * f32(Ht) - f32(0.5)
  x0, y0 = np.floor(x), np.floor(y)
  fx, fy = (x - x0)[..., None], (y - y0)[..., None]
  c0, r0 = x0.astype(np.int64) % Wt, y0.astype(np.int64) % Ht
  c1, r1 = (c0 + 1) % Wt, (r0 + 1) % Ht
  ta = tex[r0, c0] + fx * (tex[r0, c1] - tex[r0, c0])
  tb = tex[r1, c0] + fx * (tex[r1, c1] - tex[r1, c0])
  out = ta + fy * (tb - ta)
  assert out.dtype == f32
  return out


def _light_args(use_light=False, light_dir=(0, 0, 1), light_pos=(0, 0, 0), light_color=None, w_ambient=0.8, w_diffuse=0.5):
  return use_light, light_dir, light_pos, light_color, w_ambient, w_diffuse


def shade_float64(case, h, cov=None, **light):
  """Colour and normal map of hypothesis h in float64, top-down, by src/Utils.py:185-216 (`light`: nvdiffrast_render's use_light, light_dir, light_pos,
  light_color, w_ambient, w_diffuse): base colour as _base64; per VERTEX d = clip(normalize(R n) . normalize(l), 0, 1), l = -light_dir, or light_pos -
  p_cam when light_dir is None, interpolated like any attribute; colour = base w_ambient + d (light_color or base) w_diffuse; clip to [0, 1]; zero
  outside coverage.  normal = normalize(interpolated R n), zero outside coverage.  Returns dict(color, normal, covered, preclip, dvert)."""
  use_light, light_dir, light_pos, light_color, wa, wd = _light_args(**light)
  cov = cov or coverage_exact(case, h)
  g = interp_float64(case, h, cov)
  uvw, vid, covered = g['uvw'], g['vid'], g['covered']
  Rm = case['poses'][h][:3, :3].astype(np.float64)
  nc = case['mesh_tensors']['vnormals'].astype(np.float64) @ Rm.T
  col = _base64(case, uvw, vid, g['tri'])
  dvert = None
  if use_light:
    if light_dir is not None:
      l = np.broadcast_to(-np.asarray(light_dir, np.float64), nc.shape)
    else:
      l = np.asarray(light_pos, np.float64)[None] - _cam64(case, h)
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    dvert = (unit(nc) * unit(l)).sum(-1)
    d = (uvw * np.clip(dvert, 0, 1)[vid]).sum(-1)[..., None]
    col = col * wa + d * (col if light_color is None else np.asarray(light_color, np.float64)) * wd
  nrm = (uvw[..., None] * nc[vid]).sum(-2)
  nrm = nrm / np.where(covered, np.linalg.norm(nrm, axis=-1), 1.0)[..., None]
  m = covered[..., None]
  return dict(color=np.where(m, np.clip(col, 0, 1), 0.0), normal=np.where(m, nrm, 0.0), covered=covered, preclip=np.where(m, col, 0.0), dvert=dvert)


def emulate_shade_f32(case, h, cov=None, **light):
  """shade_float64 in float32 in the documented operation order, on emulate_f32's u, v, w2: per vertex nc = R n as an fmaf chain (innermost the last
  column), nn = sqrt(fmaf(nc0, nc0, fmaf(nc1, nc1, nc2 nc2))); the default light: d = clip(-(nc2 / nn)); otherwise L = -light_dir | light_pos - p_cam,
  ln likewise, d = clip(fmaf(nc0 / nn, L0 / ln, fmaf(nc1 / nn, L1 / ln, (nc2 / nn) (L2 / ln)))); per pixel d = fmaf(u, d0, fmaf(v, d1, w2 d2)),
  colour = base w_ambient + (d (light_color | base)) w_diffuse, each operation rounded; normal = fmaf-interpolated nc divided by its fmaf-chain norm."""
  use_light, light_dir, light_pos, light_color, wa, wd = _light_args(**light)
  f32 = np.float32
  cov = cov or coverage_exact(case, h)
  g = emulate_f32(case, h, cov)
  (u, v, w2), vid, covered = g['uvw'], g['vid'], g['covered']
  P = case['poses'][h].astype(f32)
  n = case['mesh_tensors']['vnormals'].astype(f32)
  nc = np.stack([_fma32(P[r, 0], n[:, 0], _fma32(P[r, 1], n[:, 1], P[r, 2] * n[:, 2])) for r in range(3)], -1)
  norm = lambda a: np.maximum(np.sqrt(_fma32(a[..., 0], a[..., 0], _fma32(a[..., 1], a[..., 1], a[..., 2] * a[..., 2]))), f32(1e-12))
  nn = norm(nc)
  col = _base32(case, u, v, w2, vid, g['tri'])
  if use_light:
    if light_dir is not None and np.array_equal(np.asarray(light_dir, float).reshape(-1), [0, 0, 1]):
      dv = np.clip(-(nc[:, 2] / nn), f32(0), f32(1))
    else:
      if light_dir is not None:
        L = np.broadcast_to(-np.asarray(light_dir, f32), nc.shape)
      else:
        L = np.asarray(light_pos, f32)[None] - _cam64(case, h).astype(f32)
      ln = norm(L)
      dv = np.clip(_fma32(nc[:, 0] / nn, L[:, 0] / ln, _fma32(nc[:, 1] / nn, L[:, 1] / ln, (nc[:, 2] / nn) * (L[:, 2] / ln))), f32(0), f32(1))
    dv = dv[vid]
    d = _fma32(u, dv[..., 0], _fma32(v, dv[..., 1], w2 * dv[..., 2]))[..., None]
    lc = col if light_color is None else np.asarray(light_color, f32)
    col = col * f32(wa) + (d * lc) * f32(wd)
  ncv = nc[vid]
  nrm = np.stack([_fma32(u, ncv[..., 0, c], _fma32(v, ncv[..., 1, c], w2 * ncv[..., 2, c])) for c in range(3)], -1)
  nrm = nrm / norm(nrm)[..., None]
  assert col.dtype == f32 and nrm.dtype == f32
  m = covered[..., None]
  return dict(color=np.where(m, np.clip(col, f32(0), f32(1)), f32(0)), normal=np.where(m, nrm, f32(0)), covered=covered)


def tex_scale(case):
  """What multiplies TOL_TEX for a case's unlit colour.  A bilinear fetch is continuous and piecewise linear in uv with slope (texel-to-texel step)
  x (texels per unit uv), and the float32 uv carries a few 2^-24 relative to max(1, |uv|): the error is bounded by a multiple of the largest
  (step between wrap-adjacent texels along an axis) x (size along it), times max(1, largest |uv| in use); not below 1, the blend's own roundings on a
  value <= 1.  1 for vertex colours."""
  mt = case['mesh_tensors']
  if 'tex' not in mt:
    return 1.0
  tex = mt['tex'][0].astype(np.float64)
  Ht, Wt = tex.shape[:2]
  sx = np.abs(tex - np.roll(tex, 1, axis=1)).max() * Wt
  sy = np.abs(tex - np.roll(tex, 1, axis=0)).max() * Ht
  return float(max(1.0, max(sx, sy) * max(1.0, np.abs(mt['uv'][mt['uv_idx']]).max())))


def shade_tol(case, **light):
  """tolerance of the colour image: TOL_TEX x tex_scale unlit; lit, colour = base wa + d (light_color | base) wd carries base's error (wa + wd) times
  and that of d <= 1 (a few 2^-24 from the two normalisations and the dot product) wd max(1, |light_color|) times"""
  use_light, light_dir, light_pos, light_color, wa, wd = _light_args(**light)
  s = tex_scale(case)
  if use_light:
    s = s * (wa + wd) + wd * (1.0 if light_color is None else max(1.0, float(np.abs(light_color).max())))
  return TOL_TEX * s


def interp_float64(case, h, cov=None):
  """perspective-correct u, v, z/w, camera-space xyz, depth and vertex-colour blend (use_light = False) of every covered pixel in float64, top-down;
  rast (Ho, Wo, 4) = (u, v, z/w, face id + 1) as dr.rasterize returns it"""
  cov = cov or coverage_exact(case, h)
  covered = cov['face'] >= 0
  f = case['faces'][np.where(covered, cov['face'], case['real'][0])]            # (Ho, Wo, 3)
  lam = np.moveaxis(cov['lam'], 0, -1)
  q = lam / case['w'][f]
  qs = q.sum(-1, keepdims=True)
  uvw = q / np.where(qs == 0, 1.0, qs)
  pc = _cam64(case, h)
  xyz = (uvw[..., None] * pc[f]).sum(-2)
  col = np.clip(_base64(case, uvw, f, np.where(covered, cov['face'], case['real'][0])), 0, 1)
  m = covered[..., None]
  rast = np.where(m, np.concatenate([uvw[..., :2], cov['zw'][..., None], (cov['face'] + 1.0)[..., None]], -1), 0.0)
  return dict(rast=rast, xyz=np.where(m, xyz, 0.0), depth=np.where(covered, xyz[..., 2], 0.0), color=np.where(m, col, 0.0), covered=covered,
              attr_scale=dict(xyz=float(np.abs(pc).max()), depth=float(np.abs(pc[:, 2]).max()), color=1.0), uvw=uvw, vid=f,
              tri=np.where(covered, cov['face'], case['real'][0]))


def emulate_f32(case, h, cov=None):
  """The documented float32 operation order on the reference's winner: b_k = float(e_k) / float(a); q_k = b_k / w_k; qs = (q0 + q1) + q2; u = q0 / qs,
  v = q1 / qs, w2 = (1 - u) - v; z/w = fmaf(b2, z2, fmaf(b1, z1, b0 z0)); attribute = fmaf(u, a0, fmaf(v, a1, w2 a2)).  Returns the same dict as
  interp_float64 (float32 values)."""
  cov = cov or coverage_exact(case, h)
  f32 = np.float32
  fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
  covered = cov['face'] >= 0
  f = case['faces'][np.where(covered, cov['face'], case['real'][0])]
  X, Y = hyp_lattice(case, h)
  Xs, Ys = X[f], Y[f]
  Px = (16 * np.arange(case['Wo'], dtype=np.int64) + 8)[None, :]
  Py = (16 * (case['Ho'] - 1 - np.arange(case['Ho'], dtype=np.int64)) + 8)[:, None]
  a = (Xs[..., 1] - Xs[..., 0]) * (Ys[..., 2] - Ys[..., 0]) - (Xs[..., 2] - Xs[..., 0]) * (Ys[..., 1] - Ys[..., 0])
  a = np.where(a == 0, 1, a)
  s = np.sign(a)
  b = []
  for k in range(3):
    p, q = (k + 1) % 3, (k + 2) % 3
    e = s * ((Xs[..., q] - Xs[..., p]) * (Py - Ys[..., p]) - (Ys[..., q] - Ys[..., p]) * (Px - Xs[..., p]))
    b.append(e.astype(f32) / (s * a).astype(f32))
  w = case['w'][f].astype(f32)
  z = case['zw'][f].astype(f32)
  q0, q1, q2 = b[0] / w[..., 0], b[1] / w[..., 1], b[2] / w[..., 2]
  qs = (q0 + q1) + q2
  qs = np.where(covered, qs, f32(1))
  u, v = q0 / qs, q1 / qs
  w2 = (f32(1) - u) - v
  zw = fma(b[2], z[..., 2], fma(b[1], z[..., 1], b[0] * z[..., 0]))
  pc = _cam64(case, h).astype(f32)[f]                     # (exact: transform_check)
  att = lambda t: np.stack([fma(u, t[..., 0, c], fma(v, t[..., 1, c], w2 * t[..., 2, c])) for c in range(t.shape[-1])], -1)
  tri = np.where(covered, cov['face'], case['real'][0])
  xyz, col = att(pc), np.clip(_base32(case, u, v, w2, f, tri), 0, 1)
  m = covered[..., None]
  rast = np.where(m, np.stack([u, v, zw, (cov['face'] + 1).astype(f32)], -1), f32(0))
  return dict(rast=rast, xyz=np.where(m, xyz, f32(0)), depth=np.where(covered, xyz[..., 2], f32(0)), color=np.where(m, col, f32(0)), covered=covered,
              uvw=(u, v, w2), vid=f, tri=tri)


def float_errors(got, ref, skip=None):
  """largest |err| / tol of a result dict (rast, xyz, depth, color arrays) against interp_float64's: (uvz, attr)"""
  keep = np.ones(ref['covered'].shape, bool) if skip is None else ~skip
  uvz = np.abs(np.asarray(got['rast'], np.float64)[..., :3] - ref['rast'][..., :3])[keep].max() / TOL_UVZ
  attr = max(np.abs(np.asarray(got[k], np.float64) - ref[k])[keep].max() / (TOL_ATTR * ref['attr_scale'][k]) for k in ('xyz', 'depth', 'color'))
  return float(uvz), float(attr)


def face_classes(case, h, N):
  """The classification rules restated on the lattice integers, for the strip height the plan picks at N hypotheses: per real face one of 'none' (zero
  area or no candidate pixel), 'small' (<= 4 candidates in every strip it touches), 'medium' (<= 32), 'large' (> 32 in some strip: list B, 32-bit),
  'slow' (a vertex with |X| or |Y| >= 16384: list B, 64-bit record form); mixed small / medium faces count as 'medium'."""
  X, Y = hyp_lattice(case, h)
  rows = plan_restated(N, len(X), len(case['faces']), case['Ho'], case['Wo'])['strip_rows']
  out = []
  for t in case['real']:
    i = case['faces'][t]
    xs, ys = [int(v) for v in X[i]], [int(v) for v in Y[i]]
    assert np.all(case['w'][i] > 0)
    if max(abs(v) for v in xs + ys) >= 16384:
      out.append('slow')
      continue
    if (xs[1] - xs[0]) * (ys[2] - ys[0]) - (xs[2] - xs[0]) * (ys[1] - ys[0]) == 0:
      out.append('none')
      continue
    ia, ib = max((min(xs) - 8 + 15) >> 4, 0), min((max(xs) - 8) >> 4, case['Wo'] - 1)
    ja, jb = max((min(ys) - 8 + 15) >> 4, 0), min((max(ys) - 8) >> 4, case['Ho'] - 1)
    if ia > ib or ja > jb:
      out.append('none')
      continue
    worst = max((ib - ia + 1) * (min(jb, (s + 1) * rows - 1) - max(ja, s * rows) + 1) for s in range(ja // rows, jb // rows + 1))
    out.append('small' if worst <= RB_SMALL else 'medium' if worst <= RB_MEDIUM else 'large')
  return out


if __name__ == '__main__':
  for name in BASE_CASES:
    c = lattice_case(name)
    mu = ma = 0.0
    for h in range(len(c['shifts'])):
      cov = coverage_exact(c, h)
      u, a = float_errors(emulate_f32(c, h, cov), interp_float64(c, h, cov), cov['band'])
      mu, ma = max(mu, u * TOL_UVZ), max(ma, a * TOL_ATTR)
    print('%-24s faces %4d  covered %5d  emulated max error: u,v,z/w %.3e  attributes / range %.3e' % (name, len(c['real']), int((cov['face'] >= 0).sum()), mu, ma))


def with_default_projection(case):
  """The case as fp_render_net sees it (no projection_mat argument: near 1 mm, far 100 m): z/w per vertex from the float32 clip row 2, one fmaf and
  one division, as documented.  Depth order: the smaller w is the nearer; layers differ by 2.5e-4 or more, exact ties do not survive (use cases
  whose overlapping faces of equal w have barycentrics 0, 1/2, 1 only)."""
  zn, zf = 0.001, 100.0
  q, qn = -(zf + zn) / (zf - zn), -2 * zf * zn / (zf - zn)
  m10, m11 = np.float32(-q), np.float32(-q + qn)
  pz = case['mesh_tensors']['pos'][:, 2]
  c2 = (np.float64(m10) * pz.astype(np.float64) + np.float64(m11)).astype(np.float32)
  c = dict(case, projection_mat=None, zw=(c2 / case['w'].astype(np.float32)).astype(np.float64))
  return c
