"""numpy / scipy restatement of the connected-components rule of include/foundationpose_amd.h (fp_mesh_components_count / _write): scipy's
connected_components over the edges a-b and b-c of every face, relabelled by the lowest member, the per-component counts, the selection
and the order-preserving compaction.  No device code.  union_find_labels is a second, pure-Python statement of rule 1 and 2 that the
host tests hold the scipy one against."""
import numpy as np


def labels(faces, V):
  """(label (V,) int32: the lowest vertex index of every vertex' component; number (V,) int64: its component number)."""
  from scipy.sparse import coo_matrix
  from scipy.sparse.csgraph import connected_components
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  if V == 0:
    return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64)
  if len(f) and (f.min() < 0 or f.max() >= V):
    raise ValueError(f'a face names a vertex outside 0 .. {V - 1}')
  rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
  g = coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(V, V))
  C, raw = connected_components(g, directed=False)
  low = np.full(C, V, dtype=np.int64)
  np.minimum.at(low, raw, np.arange(V))                  # the lowest member of every scipy component
  order = np.argsort(low, kind='stable')                 # numbered by that lowest member, ascending - whatever scipy's own order is
  number = np.empty(C, dtype=np.int64)
  number[order] = np.arange(C)
  return low[raw].astype(np.int32), number[raw]


def union_find_labels(faces, V):
  """Rule 1 and 2 in plain Python: union by lowest root, then the root of every vertex."""
  parent = list(range(V))

  def find(x):
    while parent[x] != x:
      parent[x] = parent[parent[x]]
      x = parent[x]
    return x

  for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
    for u, w in ((a, b), (b, c)):
      ru, rw = find(u), find(w)
      if ru != rw:
        parent[max(ru, rw)] = min(ru, rw)
  return np.array([find(v) for v in range(V)], dtype=np.int32).reshape(V)


def select(n_faces, keep='largest', min_faces=1, min_fraction=0.0):
  """Boolean (C,) mask of the kept components from their face counts (rule 5)."""
  if keep not in ('largest', 'all'):
    raise ValueError(f"keep must be 'largest' or 'all', got {keep!r}")
  n = np.asarray(n_faces, dtype=np.int64)
  if len(n) == 0:
    return np.zeros(0, dtype=bool)
  M = int(n.max())
  bound = np.float64(np.float32(min_fraction)) * np.float64(M)       # the device takes min_fraction as float32
  cand = (n >= 1) & (n >= int(min_faces)) & (n.astype(np.float64) >= bound)
  if keep == 'all':
    return cand
  best = int(np.argmax(n))                               # the first of equals: the lowest component number
  out = np.zeros(len(n), dtype=bool)
  out[best] = cand[best]
  return out


def components(pos, faces, normals=None, colors=None, keep='largest', min_faces=1, min_fraction=0.0):
  """Returns a dict: pos, normals, colors, faces, vertex_map, labels, stats (C,2) int32 {n_vertices, n_faces}, kept (C,) bool and counts
  (components, kept components, kept vertices, kept faces)."""
  pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
  faces = np.zeros((0, 3), dtype=np.int32) if faces is None else np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
  V, F = len(pos), len(faces)
  label, number = labels(faces, V)
  C = int(number.max()) + 1 if V else 0
  stats = np.zeros((C, 2), dtype=np.int32)
  stats[:, 0] = np.bincount(number, minlength=C)
  if F:
    stats[:, 1] = np.bincount(number[faces[:, 0].astype(np.int64)], minlength=C)      # a face belongs to its first vertex
  kept = select(stats[:, 1], keep, min_faces, min_fraction)
  vkeep = kept[number] if V else np.zeros(0, dtype=bool)
  fkeep = vkeep[faces[:, 0].astype(np.int64)] if F else np.zeros(0, dtype=bool)
  new = np.cumsum(vkeep) - 1
  vmap = np.where(vkeep, new, -1).astype(np.int32)
  out_faces = vmap[faces[fkeep].astype(np.int64)].astype(np.int32).reshape(-1, 3)
  if normals is not None:
    normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)[vkeep]
  if colors is not None:
    colors = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)[vkeep]
  return dict(pos=pos[vkeep], normals=normals, colors=colors, faces=out_faces, vertex_map=vmap, labels=label, stats=stats, kept=kept,
              counts=(C, int(kept.sum()), int(vkeep.sum()), int(fkeep.sum())))


# ---- small graphs and the stress meshes of the device tests --------------------------------------------------------------------------
def small_cases():
  """name -> (V, faces): a bow-tie (two triangles that share one vertex), isolated vertices, degenerate faces, repeated faces, F = 0."""
  f = lambda *rows: np.array(rows, dtype=np.int32).reshape(-1, 3)
  return {
    'bow_tie': (5, f([4, 3, 2], [2, 1, 0])),
    'isolated': (9, f([1, 2, 3], [7, 5, 6])),                         # 0, 4 and 8 are named by no face
    'degenerate': (8, f([5, 5, 5], [0, 1, 1], [2, 2, 3], [6, 4, 6], [3, 0, 0])),
    'repeated': (7, f([0, 1, 2], [2, 1, 0], [0, 1, 2], [4, 5, 6], [4, 5, 6])),
    'no_faces': (4, np.zeros((0, 3), dtype=np.int32)),
  }


def tie_case():
  """Two components of 3 faces each; the one that holds vertex 0 comes LATER in the face list.  (V, faces)"""
  late = [[0, 2, 4], [2, 4, 6], [4, 6, 8]]
  early = [[1, 3, 5], [3, 5, 7], [5, 7, 9]]
  return 10, np.array(early + late, dtype=np.int32)


def strip(n_faces, order):
  """A triangle strip of n_faces faces over n_faces + 2 vertices whose vertex k is called order[k].  (V, faces)"""
  k = np.arange(n_faces)
  f = np.stack([k, k + 1, k + 2], -1)
  return n_faces + 2, np.asarray(order, dtype=np.int64)[f].astype(np.int32)


def fan(n_faces):
  """n_faces faces (hub, rim k, rim k + 1) around the hub V - 1, the highest index; the rim is 0 .. n_faces.  (V, faces)"""
  V = n_faces + 2
  k = np.arange(n_faces)
  return V, np.stack([np.full(n_faces, V - 1), k, k + 1], -1).astype(np.int32)


def soup(n_tri=3000, n_isolated=500, seed=3):
  """n_tri disjoint triangles and n_isolated vertices that no face names, under one shuffled vertex numbering.  (V, faces)"""
  V = 3 * n_tri + n_isolated
  perm = np.random.RandomState(seed).permutation(V)
  return V, perm[:3 * n_tri].reshape(-1, 3).astype(np.int32)


def positions(V, seed=11):
  """Attributes that make a wrong gather visible: every vertex its own position, normal and colour."""
  r = np.random.RandomState(seed)
  return r.uniform(-1, 1, (V, 3)).astype(np.float32), r.uniform(-1, 1, (V, 3)).astype(np.float32), r.randint(0, 256, (V, 3)).astype(np.uint8)
