"""The minimum-volume oriented box of a model (what main.py:38-39 asks of trimesh.bounds.oriented_bounds) and the boxes of a point set
in given frames (fp_box_extents, csrc/bounds.hip).  A build extension: the reference leaves this to trimesh.

Candidate class: every box that has ONE FACE FLUSH WITH A FACE OF THE CONVEX HULL.  For a fixed face normal m the smallest enclosing
rectangle of the projection along m has a side along an edge of the projection's 2-D hull; those edges are projections of hull edges
whose two faces look opposite ways along m - the silhouette edges.  The candidates are therefore the pairs (distinct hull normal m,
hull edge e with (m.n_a)(m.n_b) <= SILHOUETTE_TOL), without the edges between coplanar hull triangles and the pairs whose
u = e - (e.m)m vanishes; the frame of a pair has the rows u / |u|, m x u, m.  This is the class trimesh searches; it is not O'Rourke's
exact minimum, whose box may touch the hull along edges only.

The hull is qhull's, on the host in float64 (scipy, imported lazily); the frames are built in float64 in numpy; the device evaluates every
frame against the hull's vertices in fp32 (one fp_box_extents call, more only above its limits) and the winning frame's float64 original
is evaluated again on the host over ALL points: the returned box contains every point in float64, whatever fp32 did.  fp32 can only make
the search pick a nearly tied candidate.  A symmetric model has many exactly tied boxes: the lowest candidate index wins, and that index
follows qhull's face order, not a canonical rule.  Axis order and signs are this project's convention (see oriented_bounds); parity with
trimesh's cannot be pinned without trimesh."""
import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

SILHOUETTE_TOL = 1e-9       # (m.n_a)(m.n_b) <= this: the edge is on the silhouette along m (unit normals)
VANISH_TOL = 1e-9           # |e - (e.m)m| <= this for a unit edge e: the edge runs along m and gives no frame
RANK_TOL = 1e-10            # a singular value of the centred points below this fraction of the largest: no extent in that direction
NORMAL_DECIMALS = 10        # hull normals that agree to this many decimals are one face


# ---------------------------------------------------------------------------------------------------------------- the device primitive
def _device_of(x):
  return x.device if torch.is_tensor(x) and x.is_cuda else torch.device('cuda', torch.cuda.current_device())


def better(vol_a, idx_a, vol_b, idx_b):
  """fp_box_extents' total order on (volume, index) for folding the winners of several calls: an eligible candidate (vol >= 0; a NaN
  never is) beats an ineligible one, then the smaller volume, then the lower index."""
  ea, eb = bool(vol_a >= 0), bool(vol_b >= 0)
  if ea != eb:
    return ea
  return ea and (vol_a < vol_b or (vol_a == vol_b and idx_a < idx_b))


def box_extents(points, frames, return_all=False):
  """The boxes of `points` (n,3) in `frames` (C,3,3) - rows are axes, normalised by the caller - and the smallest of them, on the
  device (fp_box_extents; the fp32 rule is stated in include/foundationpose_amd.h).  numpy arrays or tensors, rounded to float32; a
  float32 device tensor is read where it lies.

  Returns a dict: 'index' (int; -1 when no candidate has a volume >= 0), 'lo', 'hi' (3,) float32 and 'volume' (float32) of the winner -
  the smallest fp32 volume, ties to the lowest index - and with return_all=True 'all_lohi' (C,6) and 'all_volume' (C): numpy arrays when
  `points` is one, else device tensors.  More candidates than one call takes (FP_BOX_EXTENTS_MAX_FRAMES, or n C above
  FP_BOX_EXTENTS_MAX_EVALS) are cut into several calls and their winners folded on the host by the same total order.  It is also the
  box of any cloud in given frames.  The winner is read back, so this call synchronises."""
  as_numpy = not torch.is_tensor(points)
  dev = _device_of(points) if not as_numpy else _device_of(frames)
  pts = torch.as_tensor(points).to(device=dev, dtype=torch.float).reshape(-1, 3).contiguous()
  fr = torch.as_tensor(frames).to(device=dev, dtype=torch.float).reshape(-1, 3, 3).contiguous()
  n, C = len(pts), len(fr)
  if n < 1 or C < 1:
    raise ValueError(f'box_extents: {n} points and {C} frames (at least one of each)')
  if n > _lib.FP_BOX_EXTENTS_MAX_POINTS:
    raise ValueError(f'box_extents: {n} points (at most {_lib.FP_BOX_EXTENTS_MAX_POINTS})')
  per_call = max(1, min(_lib.FP_BOX_EXTENTS_MAX_FRAMES, _lib.FP_BOX_EXTENTS_MAX_EVALS // n))
  ctx = _lib.Context.get(dev)
  all_lohi = torch.empty((C, 6), dtype=torch.float, device=dev) if return_all else None
  all_vol = torch.empty(C, dtype=torch.float, device=dev) if return_all else None
  best = None
  for c0 in range(0, C, per_call):
    c1 = min(C, c0 + per_call)
    idx = torch.empty(1, dtype=torch.int32, device=dev)
    rec = torch.empty(7, dtype=torch.float, device=dev)                # lo[3], hi[3], volume
    check(lib().fp_box_extents(ctx.handle, ptr(pts), n, ptr(fr[c0:c1]), c1 - c0, ptr(idx), ptr(rec[:6]), ptr(rec[6:]),
                               ptr(all_lohi[c0:c1]) if return_all else None, ptr(all_vol[c0:c1]) if return_all else None, stream_ptr(dev)))
    i, r = int(idx.item()), rec.cpu().numpy()
    if i >= 0 and (best is None or better(r[6], c0 + i, best[1][6], best[0])):
      best = (c0 + i, r)
  if best is None:
    best = (-1, np.full(7, np.nan, dtype=np.float32))
  out = dict(index=best[0], lo=best[1][:3].copy(), hi=best[1][3:6].copy(), volume=np.float32(best[1][6]))
  if return_all:
    out['all_lohi'] = all_lohi.cpu().numpy() if as_numpy else all_lohi
    out['all_volume'] = all_vol.cpu().numpy() if as_numpy else all_vol
  return out


def _device_winner(points32, frames32):
  return box_extents(points32, frames32)['index']


# ----------------------------------------------------------------------------------------------------------------- candidates (host)
def _points_of(mesh_or_points):
  x = getattr(mesh_or_points, 'vertices', mesh_or_points)
  if torch.is_tensor(x):
    x = x.detach().cpu().numpy()
  pts = np.asarray(x, dtype=np.float64).reshape(-1, 3)
  if len(pts) < 1:
    raise ValueError('oriented_bounds: no points')
  if not np.isfinite(pts).all():
    raise ValueError('oriented_bounds: the points are not finite')
  return pts


def _unit(v):
  return v / np.linalg.norm(v, axis=-1, keepdims=True)


def hull_candidates(points, silhouette=True, chunk=256):
  """The candidate frames of a full-rank point set.  Returns a dict:
    'center'    (3,)     the midpoint of the hull vertices' extent, subtracted from them in float64 before anything is rounded
    'vertices'  (H,)     indices of the hull's vertices into `points`;  'points' (H,3) float64 = points[vertices] - center
    'normals'   (M,3)    the distinct unit outward normals of the hull's faces
    'edges'     (E,2)    the hull's edges between faces of different normals, as indices into `points`
    'pairs'     (C,2)    int64 (normal, edge) of every candidate;  'frames' (C,3,3) float64, rows u, m x u, m
  silhouette=False keeps every (normal, edge) pair whose u does not vanish (the tests enumerate that class on small hulls)."""
  from scipy.spatial import ConvexHull
  pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
  hull = ConvexHull(pts)
  hv = np.sort(hull.vertices)
  P = pts[hv]
  center = (P.min(axis=0) + P.max(axis=0)) / 2
  tri_n = _unit(hull.equations[:, :3])
  tri_id = np.asarray(np.unique(np.round(tri_n, NORMAL_DECIMALS), axis=0, return_inverse=True)[1]).reshape(-1)
  normals = np.zeros((tri_id.max() + 1, 3))
  np.add.at(normals, tri_id, tri_n)
  normals = _unit(normals)
  # every edge of a closed triangulated hull lies in exactly two triangles
  s = hull.simplices
  e = np.sort(np.concatenate([s[:, [0, 1]], s[:, [1, 2]], s[:, [2, 0]]]), axis=1)
  f = np.tile(np.arange(len(s)), 3)
  order = np.lexsort((e[:, 1], e[:, 0]))
  e, f = e[order], f[order]
  if len(e) % 2 or not (e[0::2] == e[1::2]).all():
    raise ValueError('oriented_bounds: the hull is not a closed triangulated surface')
  edges, fa, fb = e[0::2], tri_id[f[0::2]], tri_id[f[1::2]]
  keep = fa != fb                                                # not between coplanar hull triangles
  edges, fa, fb = edges[keep], fa[keep], fb[keep]
  edir = _unit(pts[edges[:, 1]] - pts[edges[:, 0]])
  na, nb = normals[fa], normals[fb]
  pairs, frames = [], []
  for m0 in range(0, len(normals), chunk):
    m = normals[m0:m0 + chunk]
    if silhouette:
      mi, ei = np.nonzero(np.einsum('ik,jk->ij', m, na) * np.einsum('ik,jk->ij', m, nb) <= SILHOUETTE_TOL)
    else:
      mi, ei = np.divmod(np.arange(len(m) * len(edges)), len(edges))
    mm, ee = m[mi], edir[ei]
    u = ee - (ee * mm).sum(axis=1, keepdims=True) * mm
    un = np.linalg.norm(u, axis=1)
    ok = un > VANISH_TOL
    mm, u, mi, ei = mm[ok], u[ok] / un[ok, None], mi[ok], ei[ok]
    pairs.append(np.stack([mi + m0, ei], axis=1))
    frames.append(np.stack([u, np.cross(mm, u), mm], axis=1))
  return dict(center=center, vertices=hv, points=P - center, normals=normals, edges=edges, pairs=np.concatenate(pairs).astype(np.int64),
              frames=np.concatenate(frames))


def _extents_in(R, pts):
  q = pts @ R.T
  return q.min(axis=0), q.max(axis=0)


def _convention(R, pts, ordered, zero):
  """Rows by ascending extent (stable: ties keep u, m x u, m), rows 0 and 1 signed so that their largest-magnitude component (the
  first of equals) is positive, row 2 = row 0 x row 1.  zero: the rows (before ordering) whose extent is 0 by construction."""
  lo, hi = _extents_in(R, pts)
  ext = np.where(zero, 0.0, hi - lo)
  if ordered:
    order = np.argsort(ext, kind='stable')
    R, zero = R[order], np.asarray(zero)[order]
  R = R.copy()
  for k in (0, 1):
    if R[k, np.argmax(np.abs(R[k]))] < 0:
      R[k] = -R[k]
  R[2] = np.cross(R[0], R[1])
  lo, hi = _extents_in(R, pts)
  extents = np.where(zero, 0.0, hi - lo)
  to_origin = np.eye(4)
  to_origin[:3, :3] = R
  to_origin[:3, 3] = -(lo + hi) / 2
  return to_origin, extents


def _degenerate(pts, rank, Vt):
  """(R rows u, v, w; zero flags; n_candidates) of a point set of rank 0, 1 or 2 (Vt: right singular vectors of the centred points)."""
  if rank == 0:
    return np.eye(3), np.array([True, True, True]), 1
  if rank == 1:
    d = Vt[0]
    a = np.eye(3)[np.argmin(np.abs(d))]
    v = _unit(a - (a @ d) * d)
    return np.stack([d, v, np.cross(d, v)]), np.array([False, True, True]), 1
  from scipy.spatial import ConvexHull
  a, b, m = Vt[0], Vt[1], np.cross(Vt[0], Vt[1])
  xy = np.stack([pts @ a, pts @ b], axis=1)
  hv = ConvexHull(xy).vertices                                   # counter-clockwise
  H = xy[hv]
  e = _unit(np.roll(H, -1, axis=0) - H)
  best = None
  for k in range(len(e)):
    u2, v2 = e[k], np.array([-e[k, 1], e[k, 0]])
    area = np.ptp(H @ u2) * np.ptp(H @ v2)
    if best is None or area < best[0]:
      best = (area, k)
  u = e[best[1], 0] * a + e[best[1], 1] * b
  return np.stack([u, np.cross(m, u), m]), np.array([False, False, True]), len(e)


def oriented_bounds(mesh_or_points, ordered=True, return_info=False, evaluate=None):
  """(to_origin (4,4) float64, extents (3,) float64) of the smallest box of the module's candidate class around a mesh's vertices or an
  (N,3) point set, with the meaning of trimesh.bounds.oriented_bounds (main.py:38-39): to_origin moves the model so that its box is
  centred at the origin and axis-aligned, bbox = [-extents / 2, extents / 2].

  Convention (the project's own): ordered=True sorts the extents ascending, ties keeping the order u, m x u, m; rows 0 and 1 of the
  rotation are signed so that each row's largest-magnitude component (the first of equals) is positive; row 2 = row 0 x row 1, so
  det = +1 always.  The box contains every point in float64.

  Degenerate input is handled on the host alone: planar points (a singular value of the centred points below RANK_TOL of the largest)
  take the plane's normal and the 2-D hull's edges and get one extent exactly 0; collinear points a box along the line with two, a
  single point (or N copies of one) three extents 0.  No point: ValueError.

  return_info=True adds a dict: 'volume', 'n_candidates', 'hull_vertices', 'normal' and 'edge' of the winner (the unit normal; the two
  indices into the points; None for degenerate input), 'aabb_volume', 'pca_volume', 'rank'.
  evaluate: a callable (points (H,3) float32, frames (C,3,3) float32) -> winning index in place of the device call (the CPU tests pass
  the numpy restatement of fp_box_extents).  Hull and frame building take a few tenths of a second on an 8 000-vertex model: cache the result."""
  pts = _points_of(mesh_or_points)
  mid = (pts.min(axis=0) + pts.max(axis=0)) / 2
  X = pts - mid
  sv, Vt = np.linalg.svd(X - X.mean(axis=0), full_matrices=False)[1:]
  rank = int((sv > RANK_TOL * sv[0]).sum()) if sv[0] > 0 else 0
  info = dict(rank=rank, normal=None, edge=None)
  if rank == 3:
    cand = hull_candidates(X)
    winner = int((evaluate or _device_winner)(cand['points'].astype(np.float32), cand['frames'].astype(np.float32)))
    if not 0 <= winner < len(cand['frames']):
      raise ValueError('oriented_bounds: no candidate has a finite volume')
    R, zero = cand['frames'][winner], np.zeros(3, dtype=bool)
    mi, ei = cand['pairs'][winner]
    info.update(n_candidates=len(cand['frames']), hull_vertices=len(cand['vertices']), normal=cand['normals'][mi].copy(),
                edge=tuple(int(i) for i in cand['edges'][ei]))
  else:
    R, zero, n_cand = _degenerate(X, rank, Vt)
    info.update(n_candidates=n_cand, hull_vertices=None)
  to_origin, extents = _convention(R, X, ordered, zero)
  to_origin[:3, 3] -= to_origin[:3, :3] @ mid
  if return_info:
    info['volume'] = float(np.prod(extents))
    info['aabb_volume'] = float(np.prod(pts.max(axis=0) - pts.min(axis=0)))
    info['pca_volume'] = float(np.prod(np.ptp(X @ Vt.T, axis=0))) if len(Vt) == 3 else 0.0
    return to_origin, extents, info
  return to_origin, extents
