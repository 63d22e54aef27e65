"""numpy restatement of the TSDF rule of include/foundationpose_amd.h (fp_tsdf_integrate, fp_tsdf_extract_*): integration in np.float32,
operation for operation in the stated order, and marching tetrahedra with the stated vertex and face order.  It imports nothing from
foundationpose_amd - the product cannot check itself - and derives its own 16-case table from the geometric rule.

Also here, because both the host and the GPU tests need them: an analytic ray-cast sphere (float64) and the mesh conditions (closed,
outward, volume)."""
import itertools

import numpy as np

F = np.float32
SLOT_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))      # +x +y +z +xy +xz +yz +xyz
PLANES = ('tsdf', 'weight', 'r', 'g', 'b', 'color_weight')


def invert_view(cam_in_ob):
  """camera-to-object (4,4) float64 -> (R (3,3), t (3,)) object-to-camera in float32, by the header's formula."""
  m = np.asarray(cam_in_ob, dtype=np.float64)
  R = m[:3, :3].T.copy()
  t = np.array([-((m[0, i] * m[0, 3] + m[1, i] * m[1, 3]) + m[2, i] * m[2, 3]) for i in range(3)], dtype=np.float64)
  return R.astype(F), t.astype(F)


class Volume:
  def __init__(self, origin, voxel_size, dims, trunc=None):
    self.dims = tuple(int(d) for d in dims)
    self.origin = np.asarray(origin, dtype=np.float64).astype(F)
    self.vs = F(voxel_size)
    self.trunc = F(4 * voxel_size if trunc is None else trunc)
    nx, ny, nz = self.dims
    self.planes = {p: np.zeros((nz, ny, nx), dtype=F) for p in PLANES}

  def coords(self):
    """s of every point: three (nz,ny,nx) float32 arrays"""
    nx, ny, nz = self.dims
    sx = self.origin[0] + self.vs * np.arange(nx, dtype=F)
    sy = self.origin[1] + self.vs * np.arange(ny, dtype=F)
    sz = self.origin[2] + self.vs * np.arange(nz, dtype=F)
    shape = (nz, ny, nx)
    return (np.broadcast_to(sx[None, None, :], shape), np.broadcast_to(sy[None, :, None], shape), np.broadcast_to(sz[:, None, None], shape))

  def integrate(self, depths, K, cam_in_obs, rgbs=None, masks=None, zfar=np.inf):
    depths = np.asarray(depths, dtype=F)
    n, H, W = depths.shape
    K = np.asarray(K, dtype=np.float64)
    fx, fy, cx, cy = F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2])
    zfar = F(zfar)
    sx, sy, sz = self.coords()
    P = self.planes
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
      for v in range(n):
        R, t = invert_view(cam_in_obs[v])
        q = [((R[a, 0] * sx + R[a, 1] * sy) + R[a, 2] * sz) + t[a] for a in range(3)]
        ok = q[2] >= F(0.001)
        col = np.floor((fx * (q[0] / q[2]) + cx) + F(0.5))
        row = np.floor((fy * (q[1] / q[2]) + cy) + F(0.5))
        ok &= (col >= 0) & (col < F(W)) & (row >= 0) & (row < F(H))
        ci = np.where(ok, col, 0).astype(np.int64)
        ri = np.where(ok, row, 0).astype(np.int64)
        d = depths[v][ri, ci]
        ok &= (d >= F(0.001)) & (d < zfar)
        if masks is not None:
          ok &= np.asarray(masks[v])[ri, ci] != 0
        sdf = d - q[2]
        ok &= ~(sdf < -self.trunc)
        tau = np.minimum(F(1), sdf / self.trunc)
        T, Wt = P['tsdf'], P['weight']
        P['tsdf'] = np.where(ok, (T * Wt + tau) / (Wt + F(1)), T)
        P['weight'] = np.where(ok, Wt + F(1), Wt)
        if rgbs is not None:
          okc = ok & (sdf <= self.trunc)
          cw = P['color_weight']
          w1 = cw + F(1)
          for ch, name in enumerate('rgb'):
            c = np.asarray(rgbs[v])[ri, ci, ch].astype(F)
            P[name] = np.where(okc, (P[name] * cw + c) / w1, P[name])
          P['color_weight'] = np.where(okc, w1, cw)
    assert all(a.dtype == F for a in P.values())

  def extract(self, min_weight=1):
    return extract(self.planes, self.origin, self.vs, min_weight)


# ---- marching tetrahedra --------------------------------------------------------------------------------------------------------
def tet_corners():
  """6 x 4 x 3: the corners of the Kuhn tetrahedra, permutations of the axes in lexicographic order"""
  out = []
  for perm in itertools.permutations(range(3)):
    c = np.zeros(3, dtype=np.int64)
    path = [c.copy()]
    for a in perm:
      c[a] += 1
      path.append(c.copy())
    out.append(path)
  return np.array(out)


def case_table():
  """{(tet, case): [triangle, ...]}; a triangle = three edges, an edge = (lower corner, upper corner) as corner numbers 0 .. 3 of the
  tetrahedron.  case bit q: corner q is negative."""
  tab = {}
  for p, P in enumerate(tet_corners().astype(np.float64)):
    for m in range(1, 15):
      neg = [q for q in range(4) if (m >> q) & 1]
      pos = [q for q in range(4) if not (m >> q) & 1]
      if len(neg) == 2:
        quad = [(neg[0], pos[0]), (neg[0], pos[1]), (neg[1], pos[1]), (neg[1], pos[0])]
        tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
      else:
        lone, others = (neg[0], pos) if len(neg) == 1 else (pos[0], neg)
        tris = [[(lone, o) for o in others]]
      direction = P[pos].mean(0) - P[neg].mean(0)
      out = []
      for tri in tris:
        mid = [0.5 * (P[a] + P[b]) for a, b in tri]
        if np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), direction) < 0:
          tri = [tri[0], tri[2], tri[1]]
        out.append([(min(e), max(e)) for e in tri])
      tab[(p, m)] = out
  return tab


def _shift(a, off, fill):
  """a[k+dz, j+dy, i+dx] where inside, `fill` elsewhere (off = (dx, dy, dz))"""
  dx, dy, dz = off
  out = np.full_like(a, fill)
  nz, ny, nx = a.shape
  out[:nz - dz, :ny - dy, :nx - dx] = a[dz:, dy:, dx:]
  return out


def _gradient(T, obs):
  g = []
  for axis in (2, 1, 0):                # x, y, z
    Tp, Tm = np.roll(T, -1, axis), np.roll(T, 1, axis)
    hp, hm = np.roll(obs, -1, axis), np.roll(obs, 1, axis)
    edge = [slice(None)] * 3
    edge[axis] = -1
    hp[tuple(edge)] = False
    edge[axis] = 0
    hm[tuple(edge)] = False
    g.append(np.where(hp & hm, (Tp - Tm) * F(0.5), np.where(hp, Tp - T, np.where(hm, T - Tm, F(0)))).astype(F))
  return g


def extract(planes, origin, vs, min_weight=1):
  """-> dict(vertices (V,3) f32, normals (V,3) f32, colors (V,3) u8, faces (F,3) i32)"""
  T, Wt = planes['tsdf'], planes['weight']
  nz, ny, nx = T.shape
  n = nx * ny * nz
  obs = Wt >= F(min_weight)
  neg = T < 0
  inside = np.ones(T.shape, dtype=bool)
  flags = np.zeros((n, 7), dtype=bool)
  for s, off in enumerate(SLOT_OFFSETS):
    flags[:, s] = (obs & _shift(obs, off, False) & _shift(inside, off, False) & (neg != _shift(neg, off, False))).reshape(-1)
  vbase = np.concatenate([[0], np.cumsum(flags.sum(1))])[:-1]
  pidx, slot = np.nonzero(flags)                       # row-major: by point index, then slot
  rank = np.cumsum(flags, axis=1) - flags              # lower slots of the same point that carry a vertex
  k, j, i = np.unravel_index(pidx, (nz, ny, nx))
  offs = np.array(SLOT_OFFSETS)[slot]
  ib, jb, kb = i + offs[:, 0], j + offs[:, 1], k + offs[:, 2]
  Ta, Tb = T[k, j, i], T[kb, jb, ib]
  with np.errstate(divide='ignore', invalid='ignore'):
    u = Ta / (Ta - Tb)
    o = np.asarray(origin, dtype=F)
    lerp = lambda a, b: a + (b - a) * u
    verts = np.stack([lerp(o[0] + vs * i.astype(F), o[0] + vs * ib.astype(F)), lerp(o[1] + vs * j.astype(F), o[1] + vs * jb.astype(F)),
                      lerp(o[2] + vs * k.astype(F), o[2] + vs * kb.astype(F))], 1).astype(F)
    cols = np.stack([np.clip(np.floor(lerp(planes[c][k, j, i], planes[c][kb, jb, ib]) + F(0.5)), 0, 255) for c in 'rgb'], 1).astype(np.uint8)
    g = _gradient(T, obs)
    nv = [lerp(ga[k, j, i], ga[kb, jb, ib]) for ga in g]
    length = np.sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2])
    normals = np.stack([np.where(length > 0, c / length, c) for c in nv], 1).astype(F)
  assert u.dtype == F and length.dtype == F

  # faces: per cube (the point index of its (0,0,0) corner), tetrahedron, triangle
  corners = tet_corners()
  tab = case_table()
  slot_of = {off: s for s, off in enumerate(SLOT_OFFSETS)}
  cube_ok = np.zeros(T.shape, dtype=bool)
  cube_ok[:nz - 1, :ny - 1, :nx - 1] = True
  sh = {off: (_shift(obs, off, False), _shift(neg, off, False)) for off in itertools.product((0, 1), repeat=3)}
  any_change = np.zeros(T.shape, dtype=bool)
  for off in SLOT_OFFSETS:
    any_change |= sh[off][1] != neg
  cand = np.nonzero((cube_ok & any_change).reshape(-1))[0]
  rank_flat, keys, tris = rank, [], []
  for p in range(6):
    cs = [tuple(int(x) for x in c) for c in corners[p]]
    ob4 = np.stack([sh[c][0].reshape(-1)[cand] for c in cs], 1)
    ng4 = np.stack([sh[c][1].reshape(-1)[cand] for c in cs], 1)
    case = (ng4 * (1 << np.arange(4))).sum(1)
    case[~ob4.all(1)] = 0
    for m in range(1, 15):
      sel = cand[case == m]
      if not len(sel):
        continue
      for tn, tri in enumerate(tab[(p, m)]):
        ids = []
        for lo, hi in tri:
          owner = sel + cs[lo][0] + nx * (cs[lo][1] + ny * cs[lo][2])
          s = slot_of[tuple(b - a for a, b in zip(cs[lo], cs[hi]))]
          assert flags[owner, s].all()
          ids.append(vbase[owner] + rank_flat[owner, s])
        tris.append(np.stack(ids, 1))
        keys.append(np.stack([sel, np.full(len(sel), p), np.full(len(sel), tn)], 1))
  if tris:
    tris, keys = np.concatenate(tris), np.concatenate(keys)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    faces = tris[order].astype(np.int32)
  else:
    faces = np.zeros((0, 3), dtype=np.int32)
  return dict(vertices=verts, normals=normals, colors=cols, faces=faces)


# ---- analytic scenes and mesh conditions ------------------------------------------------------------------------------------------
def skew_camera(H, W, fx):
  """A camera that tells fx from fy and cx from cy: fy = 1.25 fx, the principal point off the middle of the image by (0.37, -0.61) pixels."""
  return np.array([[fx, 0, W / 2 - 0.5 + 0.37], [0, 1.25 * fx, H / 2 - 0.5 - 0.61], [0, 0, 1.0]])


def look_at(eye, target=(0, 0, 0), up=(0, 0, 1)):
  """camera-to-object pose (4,4) float64: z looks from eye to target, x right, y down"""
  eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
  z = target - eye
  z /= np.linalg.norm(z)
  up = np.asarray(up, dtype=np.float64)
  if abs(np.dot(up, z)) > 0.99:
    up = np.array([0.0, 1.0, 0.0])
  x = np.cross(z, up)
  x /= np.linalg.norm(x)
  y = np.cross(z, x)
  m = np.eye(4)
  m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
  return m


def fibonacci_eyes(n, radius):
  i = np.arange(n) + 0.5
  z = 1 - 2 * i / n
  phi = i * np.pi * (3 - np.sqrt(5))
  r = np.sqrt(1 - z * z)
  return radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def sphere_depth(cam_in_ob, K, H, W, radius, center=(0, 0, 0)):
  """z-depth (H,W) float32 of a sphere in the object frame seen from cam_in_ob: the ray through every pixel centre against the sphere,
  solved in float64; 0 where the ray misses."""
  K = np.asarray(K, dtype=np.float64)
  us, vs_ = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
  d = np.stack([(us - K[0, 2]) / K[0, 0], (vs_ - K[1, 2]) / K[1, 1], np.ones_like(us)], -1)      # camera frame, z = 1
  c = np.linalg.inv(cam_in_ob) @ np.append(np.asarray(center, dtype=np.float64), 1.0)
  c = c[:3]
  a = (d * d).sum(-1)
  b = d @ c
  disc = b * b - a * (c @ c - radius * radius)
  hit = disc > 0
  z = (b - np.sqrt(np.where(hit, disc, 0))) / a
  return np.where(hit & (z > 0), z, 0).astype(F)


def plane_depth(H, W, z):
  return np.full((H, W), z, dtype=F)


def edge_use(faces):
  """how many faces use every undirected edge: (edges (E,2), counts (E,))"""
  f = np.asarray(faces, dtype=np.int64)
  e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
  e.sort(1)
  return np.unique(e, axis=0, return_counts=True)


def signed_volume(vertices, faces):
  v = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
  return float(np.einsum('ij,ij->i', v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def components(faces, n_vertices):
  """label of the connected component of every face (union-find over shared vertices), labels 0 .. by decreasing face count"""
  f = np.asarray(faces, dtype=np.int64)
  parent = np.arange(n_vertices)

  def find(x):
    while parent[x] != x:
      parent[x] = parent[parent[x]]
      x = parent[x]
    return x
  for a, b, c in f:
    ra, rb, rc = find(a), find(b), find(c)
    parent[rb] = ra
    parent[find(rc)] = ra
  roots = np.array([find(x) for x in f[:, 0]])
  uniq, inv, cnt = np.unique(roots, return_inverse=True, return_counts=True)
  order = np.argsort(-cnt, kind='stable')
  relabel = np.empty(len(uniq), dtype=np.int64)
  relabel[order] = np.arange(len(uniq))
  return relabel[inv]


# ---- the sphere both test files use -------------------------------------------------------------------------------------------------
SPHERE_RADIUS, SPHERE_VIEWS, SPHERE_HW, SPHERE_F, SPHERE_DIST = 0.05, 12, (120, 160), 400.0, 0.4
# the largest |radius of a vertex - SPHERE_RADIUS| of this restatement on sphere_case((35, 33, 37), 0.004), in voxels (measured: 0.640;
# DESIGN.md section 5), and what the tests allow: 1.5 x that, under one voxel
SPHERE_MEASURED_VOXELS = 0.640
RADIAL_BOUND_VOXELS = 1.5 * SPHERE_MEASURED_VOXELS


def sphere_case(dims, voxel_size):
  """A sphere of SPHERE_RADIUS at the origin seen by SPHERE_VIEWS cameras on a Fibonacci sphere: (origin, K, cam_in_obs, depths).  The
  volume is centred on the sphere but for a fraction of a voxel, so that no sample point is special."""
  H, W = SPHERE_HW
  K = np.array([[SPHERE_F, 0, W / 2 - 0.5], [0, SPHERE_F, H / 2 - 0.5], [0, 0, 1.0]])
  dims = np.asarray(dims)
  origin = -(dims - 1) * voxel_size / 2 + np.array([0.0007, -0.0011, 0.0013])
  poses = np.stack([look_at(e) for e in fibonacci_eyes(SPHERE_VIEWS, SPHERE_DIST)])
  depths = np.stack([sphere_depth(p, K, H, W, SPHERE_RADIUS) for p in poses])
  return origin, K, poses, depths


def check_closed_outward_sphere(vertices, faces, voxel_size, normals=None):
  """The conditions on a fused sphere; returns the largest radial error in voxels."""
  vertices, faces = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
  assert len(faces) > 0 and faces.min() >= 0 and faces.max() < len(vertices), 'face index out of range'
  assert len(np.unique(faces)) == len(vertices), 'a vertex is not referenced'
  _, counts = edge_use(faces)
  assert (counts == 2).all(), f'edges used by {np.unique(counts)} faces: the surface is not closed'
  vol, exact = signed_volume(vertices, faces), 4.0 / 3.0 * np.pi * SPHERE_RADIUS ** 3
  assert vol > 0, 'the faces are wound inward'
  # a shell of the radial bound around the sphere changes the volume by 3 * bound / radius at most (first order)
  assert abs(vol / exact - 1) < 3.2 * RADIAL_BOUND_VOXELS * voxel_size / SPHERE_RADIUS, vol / exact
  rad = np.linalg.norm(vertices, axis=1)
  if normals is not None:
    assert ((np.asarray(normals, dtype=np.float64) * vertices).sum(1) > 0).all(), 'a vertex normal points inward'
  return float(np.abs(rad - SPHERE_RADIUS).max() / voxel_size)


def mustard_eyes():
  """12 camera centres around the synthetic bottle, 0.42 m from its centre: a ring of eight on the equator, which sees the sides only,
  and two steep views (1.35 rad of elevation) of the cap and two of the bottom.  No camera sees the flat cap or bottom at a grazing
  angle: there the depth changes by several millimetres from one pixel to the next, the nearest pixel of a point just outside the
  surface then lies on the surface in front of it, and the fused surface moves outward - rings at 0.3 rad of elevation, 4 degrees
  above the plane of the cap, left 1.1 - 1.4 % of the vertices beyond the radial bound.  With these poses the restatement leaves
  0.8 % beyond it (0.4 % on the GPU, behind the depth filter) and the largest component holds every face (tests/test_tsdf_host.py)."""
  def ring(n, el, ph):
    a = np.arange(n) * 2 * np.pi / n + ph
    return 0.42 * np.stack([np.cos(el) * np.cos(a), np.cos(el) * np.sin(a), np.full(n, np.sin(el))], 1)
  return np.concatenate([ring(8, 0.0, 0.3), ring(2, 1.35, 0.2), ring(2, -1.35, 1.8)])


MUSTARD_HW, MUSTARD_VOXEL = (120, 160), 0.004
MUSTARD_K = np.array([[200.0, 0, 79.5], [0, 200.0, 59.5], [0, 0, 1.0]])


def surface_samples(vertices, faces, n=400000, seed=0):
  """n points drawn uniformly over the triangles (seeded)"""
  tri = np.asarray(vertices, dtype=np.float64)[np.asarray(faces)]
  rs = np.random.RandomState(seed)
  area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
  pick = rs.choice(len(tri), n, p=area / area.sum())
  u = rs.rand(n, 2)
  u[u.sum(1) > 1] = 1 - u[u.sum(1) > 1]
  return tri[pick, 0] + (tri[pick, 1] - tri[pick, 0]) * u[:, :1] + (tri[pick, 2] - tri[pick, 0]) * u[:, 1:]


def fraction_beyond_bound(vertices, source_vertices, source_faces, voxel_size):
  """(fraction of `vertices` farther than RADIAL_BOUND_VOXELS voxels from the sampled source surface, largest distance in voxels)"""
  from scipy.spatial import cKDTree
  dist, _ = cKDTree(surface_samples(source_vertices, source_faces)).query(np.asarray(vertices, dtype=np.float64))
  return float((dist > RADIAL_BOUND_VOXELS * voxel_size).mean()), float(dist.max() / voxel_size)
