"""Host restatement of the rules of fp_point_mesh_distance and fp_mesh_sample_surface (include/foundationpose_amd.h), in numpy:
float64 by default, vectorised over (points x faces).  It shares no code with the library; tests/test_surface_distance_host.py checks it
against answers that do not share its arithmetic (hand-written rationals, nearest-neighbour bounds, a sphere)."""
import numpy as np

_BLOCK_PAIRS = 1 << 22      # pairs evaluated at once


def _dot(a, b):
  return (a * b).sum(-1)


def _segment(w, e):
  """closest point of the segment t e, t in [0, 1], to w (both relative to the segment's origin): (d2, q).  Zero length: the end point."""
  ee = _dot(e, e)
  with np.errstate(divide='ignore', invalid='ignore'):
    t = np.where(ee > 0, _dot(w, e) / np.where(ee > 0, ee, 1), 0)
  t = np.clip(t, 0, 1)
  q = t[..., None] * e
  return _dot(w - q, w - q), q


def pair_distance2(p, a, b, c):
  """Squared distance and closest point for broadcastable (.., 3) arrays of points and triangle corners, in the arrays' dtype.
  What belongs to the face alone (edges, their dot products and inverses, the unit normal) is formed in float64 and rounded to the
  dtype once, as the library does.  Seven regions (three vertices, three edges, the interior) by the six dot products of coordinates
  translated to a; the first region that applies in the order a, b, ab, c, ac, bc, interior; the interior is the foot of the
  perpendicular; a face whose cross product is exactly zero is the minimum over its segments ab, ac, bc (a later one only when strictly
  smaller)."""
  p, a, b, c = np.broadcast_arrays(p, a, b, c)
  dtype = p.dtype
  a64, b64, c64 = (x.astype(np.float64) for x in (a, b, c))
  ab64, ac64 = b64 - a64, c64 - a64
  bc64 = ac64 - ab64
  n64 = np.cross(ab64, ac64)
  det64 = _dot(n64, n64)
  with np.errstate(divide='ignore', invalid='ignore'):
    inv = lambda x: np.where(x > 0, 1 / np.where(x > 0, x, 1), 0).astype(dtype)
    unit = np.where(det64[..., None] > 0, n64 / np.sqrt(np.where(det64 > 0, det64, 1))[..., None], 0).astype(dtype)
  ab, ac = ab64.astype(dtype), ac64.astype(dtype)
  e00, e01, e11, det = (x.astype(dtype) for x in (_dot(ab64, ab64), _dot(ab64, ac64), _dot(ac64, ac64), det64))
  inv_e00, inv_e11, inv_ebc = inv(_dot(ab64, ab64)), inv(_dot(ac64, ac64)), inv(_dot(bc64, bc64))
  ap = p - a
  bp, cp = ap - ab, ap - ac
  d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
  vc, vb = e00 * d2 - e01 * d1, e11 * d1 - e01 * d2
  with np.errstate(invalid='ignore', over='ignore'):
    inside = np.ones(d1.shape, bool)
    s, t = np.zeros_like(d1), np.zeros_like(d1)
    on_bc = (vb + vc >= det) & (d4 - d3 >= 0) & (d5 - d6 >= 0)               # edge bc: b + w bc
    inside = inside & ~on_bc
    bc = ac - ab
    w = np.clip(_dot(bc, bp) * inv_ebc, 0, 1)
    m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)                                    # edge ac
    s, t, inside, on_bc = np.where(m, 0, s), np.where(m, d2 * inv_e11, t), inside & ~m, on_bc & ~m
    m = (d6 >= 0) & (d5 <= d6)                                               # vertex c
    s, t, inside, on_bc = np.where(m, 0, s), np.where(m, 1, t), inside & ~m, on_bc & ~m
    m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)                                    # edge ab
    s, t, inside, on_bc = np.where(m, d1 * inv_e00, s), np.where(m, 0, t), inside & ~m, on_bc & ~m
    m = (d3 >= 0) & (d4 <= d3)                                               # vertex b
    s, t, inside, on_bc = np.where(m, 1, s), np.where(m, 0, t), inside & ~m, on_bc & ~m
    m = (d1 <= 0) & (d2 <= 0)                                                # vertex a
    s, t, inside, on_bc = np.where(m, 0, s), np.where(m, 0, t), inside & ~m, on_bc & ~m
    foot = ap - _dot(unit, ap)[..., None] * unit                             # the interior
    q = np.where(on_bc[..., None], ab + w[..., None] * bc, s[..., None] * ab + t[..., None] * ac)
    q = np.where(inside[..., None], foot, q).astype(dtype)
    diff = np.where(inside[..., None], _dot(unit, ap)[..., None] * unit, ap - q)
    dist2 = _dot(diff, diff)
    deg = ~(det64 > 0) | ~(det > 0)
    if deg.any():
      g2, gq = _segment(ap, ab)
      h2, hq = _segment(ap, ac)
      m = h2 < g2
      g2, gq = np.where(m, h2, g2), np.where(m[..., None], hq, gq)
      h2, hq = _segment(ap - ab, ac - ab)
      m = h2 < g2
      g2, gq = np.where(m, h2, g2), np.where(m[..., None], ab + hq, gq)
      dist2, q = np.where(deg, g2, dist2), np.where(deg[..., None], gq, q)
  return dist2.astype(dtype), (a + q).astype(dtype)


def _usable_faces(vertices, faces):
  """faces the rule follows: every index in [0, V) and every vertex finite"""
  V = len(vertices)
  in_range = ((faces >= 0) & (faces < V)).all(1)
  safe = np.where(in_range[:, None], faces, 0)
  return in_range & np.isfinite(vertices[safe]).all((1, 2)), safe


def point_mesh_distance(points, vertices, faces, dtype=np.float64):
  """(dist, face, closest): the minimum over ALL faces, equal squared distances to the lowest face index, dist = sqrt(d2).  A query
  with a non-finite coordinate, or with no usable face, gets NaN, -1, NaN."""
  points, vertices = np.asarray(points, dtype).reshape(-1, 3), np.asarray(vertices, dtype).reshape(-1, 3)
  faces = np.asarray(faces, np.int64).reshape(-1, 3)
  usable, safe = _usable_faces(vertices, faces)
  tri = np.where(usable[:, None, None], vertices[safe], 0)
  n, F = len(points), len(faces)
  best = np.full(n, np.inf, dtype)
  face = np.full(n, -1, np.int64)
  closest = np.full((n, 3), np.nan, dtype)
  ok = np.isfinite(points).all(1)
  pts = np.where(ok[:, None], points, 0)
  step = max(1, _BLOCK_PAIRS // max(F, 1))
  for i0 in range(0, n, step):
    p = pts[i0:i0 + step, None, :]
    d2, q = pair_distance2(p, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
    d2 = np.where(usable[None, :] & np.isfinite(d2), d2, np.inf)
    f = d2.argmin(1)                                       # the first of equal minima: the lowest face index
    r = np.arange(len(f))
    found = np.isfinite(d2[r, f]) & ok[i0:i0 + step]
    best[i0:i0 + step] = np.where(found, d2[r, f], np.nan)
    face[i0:i0 + step] = np.where(found, f, -1)
    closest[i0:i0 + step] = np.where(found[:, None], q[r, f], np.nan)
  return np.sqrt(best), face, closest


def point_face_distance(points, vertices, faces, face_index, dtype=np.float64):
  """(dist, closest) of point i to the one face face_index[i]"""
  points, vertices = np.asarray(points, dtype).reshape(-1, 3), np.asarray(vertices, dtype).reshape(-1, 3)
  tri = vertices[np.asarray(faces, np.int64).reshape(-1, 3)[np.asarray(face_index, np.int64)]]
  d2, q = pair_distance2(points, tri[:, 0], tri[:, 1], tri[:, 2])
  return np.sqrt(d2), q


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------
def face_areas(vertices, faces):
  """0.5 |ab x ac| in float64 from the float32 positions; 0 for a face that is not followed or whose area is not finite"""
  vertices = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
  faces = np.asarray(faces, np.int64).reshape(-1, 3)
  in_range = ((faces >= 0) & (faces < len(vertices))).all(1)
  tri = vertices[np.where(in_range[:, None], faces, 0)]
  with np.errstate(invalid='ignore', over='ignore'):
    area = 0.5 * np.sqrt((np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) ** 2).sum(1))
  return np.where(in_range & np.isfinite(area), area, 0.0)


def area_q(vertices, faces):
  """int64 areas in units of 2^-40 of the total"""
  area = face_areas(vertices, faces)
  return np.rint(area / area.sum() * 2.0 ** 40).astype(np.int64)


def sample_faces(aq, n):
  """sample i lands on the first face whose inclusive prefix sum exceeds t_i = ((2 i + 1) A_q) // (2 n): exact integers"""
  incl = np.cumsum(np.asarray(aq, np.int64))
  total = int(incl[-1])
  t = np.array([((2 * i + 1) * total) // (2 * n) for i in range(n)], dtype=np.int64)
  return np.searchsorted(incl, t, side='right')


def lowbias32(x):
  x = np.asarray(x, np.uint64) & 0xffffffff
  x ^= x >> 16
  x = (x * 0x7feb352d) & 0xffffffff
  x ^= x >> 15
  x = (x * 0x846ca68b) & 0xffffffff
  x ^= x >> 16
  return x


def sample_bary(n, seed):
  """(u, v) float32 (n, 2): two 24-bit uniforms of the hash of (seed, i), (k + 0.5) / 2^24, reflected on the integers when u + v > 1"""
  i = np.arange(n, dtype=np.uint64)
  base = lowbias32(seed)
  ku = (lowbias32((base + 2 * i) & 0xffffffff) >> 8).astype(np.int64)
  kv = (lowbias32((base + 2 * i + 1) & 0xffffffff) >> 8).astype(np.int64)
  m = ku + kv >= 1 << 24
  ku, kv = np.where(m, (1 << 24) - 1 - ku, ku), np.where(m, (1 << 24) - 1 - kv, kv)
  return np.stack([((ku + 0.5) * 2.0 ** -24).astype(np.float32), ((kv + 0.5) * 2.0 ** -24).astype(np.float32)], 1)


def sample_points(vertices, faces, face, bary):
  """a + u ab + v ac in float64"""
  tri = np.asarray(vertices, np.float64).reshape(-1, 3)[np.asarray(faces, np.int64).reshape(-1, 3)[face]]
  u, v = np.asarray(bary, np.float64)[:, :1], np.asarray(bary, np.float64)[:, 1:]
  return tri[:, 0] + u * (tri[:, 1] - tri[:, 0]) + v * (tri[:, 2] - tri[:, 0])


def sample_surface(vertices, faces, n, seed=0):
  """(points float64, face, bary float32) by the rule, with the host's own area_q"""
  face = sample_faces(area_q(vertices, faces), n)
  bary = sample_bary(n, seed)
  return sample_points(vertices, faces, face, bary), face, bary


# ---- shapes the tests share -------------------------------------------------------------------------------------------------------------
LATTICE_TRIANGLE = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float64)
# query, exact d2 as a fraction (numerator, denominator), the region
LATTICE_CASES = [
  ((1, 1, 3), (9, 1), 'interior'),
  ((-3, -4, 0), (25, 1), 'vertex a'),
  ((5, -1, 0), (2, 1), 'vertex b'),
  ((-1, 5, 0), (2, 1), 'vertex c'),
  ((2, -2, 1), (5, 1), 'edge ab'),
  ((-2, 2, 0), (4, 1), 'edge ac'),
  ((3, 3, 0), (2, 1), 'edge bc'),
]


def random_soup(n_faces, seed):
  """n_faces independent random triangles with coordinates in [-1, 1]: (vertices float32 (3 n, 3), faces int32)"""
  rng = np.random.default_rng(seed)
  v = rng.uniform(-1, 1, (3 * n_faces, 3)).astype(np.float32)
  return v, np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


def lattice_cube(lo=0.0, hi=2.0):
  """closed cube, 8 vertices, 12 faces; the two triangles of a side share the side's diagonal"""
  v = np.array([[x, y, z] for z in (lo, hi) for y in (lo, hi) for x in (lo, hi)], np.float32)
  f = np.array([[0, 2, 1], [1, 2, 3],      # z = lo
                [4, 5, 6], [5, 7, 6],      # z = hi
                [0, 1, 4], [1, 5, 4],      # y = lo
                [2, 6, 3], [3, 6, 7],      # y = hi
                [0, 4, 2], [2, 4, 6],      # x = lo
                [1, 3, 5], [3, 7, 5]], np.int32)      # x = hi
  return v, f


def icosphere(subdivisions=1, radius=1.0):
  """icosahedron, each face split in four `subdivisions` times, the vertices on the sphere: 20 * 4^s faces (80 at s = 1)"""
  g = (1 + 5 ** 0.5) / 2
  v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1),
       (-g, 0, 1)]
  f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
       (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
  v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
  for _ in range(subdivisions):
    mid, out = {}, []
    def midpoint(i, j):
      key = (min(i, j), max(i, j))
      if key not in mid:
        m = v[i] + v[j]
        v.append(m / np.linalg.norm(m))
        mid[key] = len(v) - 1
      return mid[key]
    for a, b, c in f:
      ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
      out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    f = out
  return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)
