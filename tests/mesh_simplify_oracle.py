"""numpy restatement of the vertex-clustering rule of include/foundationpose_amd.h (fp_mesh_simplify_count / _write) and of the
max_vertices search of Utils.simplify_mesh, plus the composite test mesh.  No device code: np.unique on the keys, np.add.at on int64,
the packed-triple dedup, the bisection."""
import numpy as np

MAX_DIM = 1 << 21
FIX = float(1 << 30)


def cells(pos, cell):
  """(origin float32 (3,), cell index (V,3) int64, dims (3,) int64); ValueError when a dim exceeds 2^21."""
  pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
  cell = np.float32(cell)
  o = pos.min(0)
  c = np.floor((pos - o) / cell).astype(np.int64)      # subtraction and division in float32
  dims = c.max(0) + 1
  if (dims > MAX_DIM).any():
    raise ValueError(f'cell {cell} gives dims {dims.tolist()}')
  return o, c, dims


def simplify(pos, faces, cell, normals=None, colors=None):
  """Returns a dict: pos, normals, colors, faces, vertex_map and the counts of every branch (clusters, degenerate, duplicate,
  unreferenced)."""
  pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
  faces = np.zeros((0, 3), dtype=np.int32) if faces is None else np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
  V, F = len(pos), len(faces)
  o, c, dims = cells(pos, cell)
  key = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
  _, first, inv = np.unique(key, return_index=True, return_inverse=True)
  inv = inv.reshape(-1)
  order = np.argsort(first, kind='stable')             # clusters by their lowest member, ascending
  rank = np.empty(len(order), dtype=np.int64)
  rank[order] = np.arange(len(order))
  cid = rank[inv]
  low = first[order]
  C = len(low)
  n = np.bincount(cid, minlength=C).astype(np.int64)
  single = n == 1

  o64 = o.astype(np.float64)
  q = np.rint((pos.astype(np.float64) - o64) * FIX).astype(np.int64)
  S = np.zeros((C, 3), dtype=np.int64)
  np.add.at(S, cid, q)
  cpos = (o64 + S.astype(np.float64) / n[:, None].astype(np.float64) / FIX).astype(np.float32)
  cpos[single] = pos[low[single]]
  cnrm = ccol = None
  if normals is not None:
    normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    N = np.zeros((C, 3), dtype=np.int64)
    np.add.at(N, cid, np.rint(normals.astype(np.float64) * FIX).astype(np.int64))
    s = N.astype(np.float64)
    length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    with np.errstate(invalid='ignore', divide='ignore'):
      cnrm = np.where(length[:, None] > 0, s / length[:, None], 0.0).astype(np.float32)
    cnrm[single] = normals[low[single]]
  if colors is not None:
    colors = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)
    Cs = np.zeros((C, 3), dtype=np.int64)
    np.add.at(Cs, cid, colors.astype(np.int64))
    ccol = ((2 * Cs + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
    ccol[single] = colors[low[single]]

  stats = dict(clusters=C, degenerate=0, duplicate=0, unreferenced=0)
  if F > 0:
    ids = cid[faces.astype(np.int64)]
    nondeg = (ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 0] != ids[:, 2])
    srt = np.sort(ids, axis=1)
    packed = (srt[:, 0] << 42) | (srt[:, 1] << 21) | srt[:, 2]
    cand = np.nonzero(nondeg)[0]
    _, firstf = np.unique(packed[cand], return_index=True)      # the first occurrence: the lowest face index
    keep = np.sort(cand[firstf])
    ref = np.zeros(C, dtype=bool)
    ref[ids[keep].reshape(-1)] = True
    new = np.cumsum(ref) - 1
    out_faces = new[ids[keep]].astype(np.int32)
    vmap = np.where(ref[cid], new[cid], -1).astype(np.int32)
    stats.update(degenerate=int(F - len(cand)), duplicate=int(len(cand) - len(keep)), unreferenced=int(C - ref.sum()))
  else:
    ref = np.ones(C, dtype=bool)
    out_faces = np.zeros((0, 3), dtype=np.int32)
    vmap = cid.astype(np.int32)
  return dict(pos=cpos[ref], normals=None if cnrm is None else cnrm[ref], colors=None if ccol is None else ccol[ref], faces=out_faces,
              vertex_map=vmap, cell=np.float32(cell), **stats)


def count_vertices(pos, faces, cell):
  return len(simplify(pos, faces, cell)['pos'])


SEARCH_STEPS = 20


def search_cell(pos, faces, max_vertices, count=count_vertices):
  """The bisection of Utils.simplify_mesh(max_vertices=...): returns (float32 cell, lo, hi) - the mesh is the one at float32(hi)."""
  pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
  lo, hi = 0.0, float((pos.max(0).astype(np.float64) - pos.min(0).astype(np.float64)).max())
  for _ in range(SEARCH_STEPS):
    mid = (lo + hi) / 2
    if count(pos, faces, np.float32(mid)) <= max_vertices:
      hi = mid
    else:
      lo = mid
  return np.float32(hi), lo, hi


# ---- the composite mesh ------------------------------------------------------------------------------------------------------------
def uv_sphere(rings=95, segments=200, radius=0.05):
  """rings x segments vertices between two poles; the analytic normals.  (rings * segments + 2 vertices, 2 * rings * segments faces)"""
  th = np.pi * (np.arange(rings, dtype=np.float64) + 1) / (rings + 1)
  ph = 2 * np.pi * np.arange(segments, dtype=np.float64) / segments
  T, P = np.meshgrid(th, ph, indexing='ij')
  n = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
  n = np.concatenate([n, [[0.0, 0.0, 1.0]], [[0.0, 0.0, -1.0]]])
  idx = lambda r, s: r * segments + (s % segments)
  r, s = np.meshgrid(np.arange(rings - 1), np.arange(segments), indexing='ij')
  a, b, c, d = idx(r, s), idx(r, s + 1), idx(r + 1, s), idx(r + 1, s + 1)
  body = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
  s1 = np.arange(segments)
  top, bot = rings * segments, rings * segments + 1
  cap_t = np.stack([np.full(segments, top), idx(0, s1), idx(0, s1 + 1)], -1)
  cap_b = np.stack([np.full(segments, bot), idx(rings - 1, s1 + 1), idx(rings - 1, s1)], -1)
  return (n * radius).astype(np.float32), np.concatenate([body, cap_t, cap_b]).astype(np.int32), n.astype(np.float32)


def lattice_sheet(n=41, pitch=0.0011, origin=(0.0, 0.0, 0.0), reverse=False):
  i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
  v = np.stack([origin[0] + pitch * i, origin[1] + pitch * j, np.full(i.shape, origin[2], dtype=np.float64)], -1).reshape(-1, 3)
  a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
  f = np.concatenate([np.stack([a, a + n, a + 1], -1), np.stack([a + 1, a + n, a + n + 1], -1)])
  if reverse:
    f = f[:, ::-1]
  nz = -1.0 if reverse else 1.0
  return v.astype(np.float32), f.astype(np.int32), np.tile(np.array([0.0, 0.0, nz], dtype=np.float32), (len(v), 1))


def composite_mesh(seed=0):
  """A UV sphere of 95 x 200 (radius 0.05), two 41 x 41 lattice sheets of pitch 1.1 mm, 0.9 mm apart, the second with reversed faces, and
  one isolated vertex (the last one): 22 365 vertices, 44 400 faces.  Returns pos, faces, normals (float32), colours (uint8, seeded)."""
  sv, sf, sn = uv_sphere()
  av, af, an = lattice_sheet(origin=(0.06, -0.02, 0.0))
  bv, bf, bn = lattice_sheet(origin=(0.06, -0.02, 0.0009), reverse=True)
  pos = np.concatenate([sv, av, bv, np.array([[0.09, 0.04, 0.03]], dtype=np.float32)])
  faces = np.concatenate([sf, af + len(sv), bf + len(sv) + len(av)]).astype(np.int32)
  normals = np.concatenate([sn, an, bn, np.array([[1.0, 0.0, 0.0]], dtype=np.float32)])
  colors = np.random.RandomState(seed).randint(0, 256, size=(len(pos), 3)).astype(np.uint8)
  assert pos.shape == (22365, 3) and faces.shape == (44400, 3)
  return pos, faces, normals, colors


def check_consequences(pos, faces, out, cell):
  """The consequences listed under the rule; raises AssertionError."""
  pos = np.asarray(pos, dtype=np.float32)
  vm, op, of = out['vertex_map'], out['pos'], out['faces']
  kept = vm >= 0
  extent = float((pos.max(0).astype(np.float64) - pos.min(0).astype(np.float64)).max())
  d = np.linalg.norm(pos[kept].astype(np.float64) - op[vm[kept]].astype(np.float64), axis=1)
  assert d.size == 0 or d.max() <= np.sqrt(3.0) * float(cell) + 1e-6 * extent, (d.max(), cell)
  if len(of):
    assert of.min() >= 0 and of.max() < len(op)
    assert ((of[:, 0] != of[:, 1]) & (of[:, 1] != of[:, 2]) & (of[:, 0] != of[:, 2])).all()
    s = np.sort(of.astype(np.int64), axis=1)
    assert len(np.unique((s[:, 0] << 42) | (s[:, 1] << 21) | s[:, 2])) == len(of)
  if faces is not None and len(faces):
    assert len(np.unique(of)) == len(op)
  return float(d.max() / float(cell)) if d.size else 0.0
