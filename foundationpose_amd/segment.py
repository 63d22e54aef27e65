"""Masks from depth: the objects standing on one supporting plane (csrc/segment.hip; the rules are stated in
include/foundationpose_amd.h and restated in numpy by tests/segment_oracle.py).

    plane, info = fit_plane(depth, K)                    # fp_plane_score over seeded three-pixel hypotheses, then least-squares refits
    labels, stats = segment_on_plane(depth, K, plane)    # int32 label image + per-segment statistics (fp_depth_segment_*)
    ids, cost = assign_segments(stats, diameters)        # which segment is which object, by size only

This is geometry, not a learned segmenter: objects that touch without a depth step between them are ONE segment, everything must stand
on (or above) one dominant plane, and nothing is recognised - segments are told apart by their size or by the caller.  The reference
has a mask-painting GUI in this place (src/masking.py).
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, k_ptr, lib, ptr, stream_ptr

MAX_VIEWS = _lib.FP_TSDF_MAX_VIEWS
Q_SCALE = 1048576.0      # the statistics are 2^-20 m fixed point


def _maps_on(depth, mask, device):
  """(device, depths (n,H,W) float32 device tensor, masks (n,H,W) uint8 or None, whether the depth came as a batch / as a device tensor)."""
  on_device = torch.is_tensor(depth) and depth.is_cuda
  dev = depth.device if on_device else torch.device(device)
  depths = torch.as_tensor(depth, device=dev).to(torch.float).contiguous()
  batch = depths.dim() == 3
  if not batch:
    depths = depths[None]
  if depths.dim() != 3:
    raise ValueError(f'depth must be (H,W) or (n,H,W), got {tuple(depths.shape)}')
  n, H, W = depths.shape
  if mask is not None:
    mask = torch.as_tensor(mask, device=dev)
    if not batch:
      mask = mask[None]
    if tuple(mask.shape) != (n, H, W):
      raise ValueError(f'mask must have the shape of the depth {(n, H, W)}, got {tuple(mask.shape)}')
    mask = (mask != 0).to(torch.uint8).contiguous()
  return dev, depths, mask, batch, on_device


def _planes_of(plane, n):
  p = np.asarray(plane.detach().cpu() if torch.is_tensor(plane) else plane, dtype=np.float64)
  if p.shape == (4,):
    p = np.tile(p, (n, 1))
  if p.shape != (n, 4):
    raise ValueError(f'plane must be (4,) or ({n},4), got {p.shape}')
  return np.ascontiguousarray(p)


def plane_score(depths, K, triplets, tol, masks=None, zfar=100, device='cuda'):
  """fp_plane_score on (n,H,W) maps: triplets (n_hyp,3) or (n,n_hyp,3) int32 pixel indices -> (planes (n,n_hyp,4) float32, counts
  (n,n_hyp) int32, best (n,) int32), numpy.  Synchronises."""
  dev, depths, masks, _, _ = _maps_on(depths, masks, device)
  n, H, W = depths.shape
  trip = np.asarray(triplets, dtype=np.int32)
  if trip.ndim == 2:
    trip = np.tile(trip[None], (n, 1, 1))
  if trip.ndim != 3 or trip.shape[0] != n or trip.shape[2] != 3:
    raise ValueError(f'triplets must be (n_hyp,3) or ({n},n_hyp,3), got {trip.shape}')
  trip = np.ascontiguousarray(trip)
  n_hyp = trip.shape[1]
  Kd, Kp = k_ptr(K)
  planes = np.zeros((n, n_hyp, 4), np.float32)
  counts = np.zeros((n, n_hyp), np.int32)
  best = np.full((n,), -1, np.int32)
  for a in range(0, n, MAX_VIEWS):      # views are independent: more than MAX_VIEWS are cut into calls
    b = min(a + MAX_VIEWS, n)
    pl, ct, bs = (np.ascontiguousarray(x[a:b]) for x in (planes, counts, best))
    check(lib().fp_plane_score(_lib.Context.get(dev).handle, ptr(depths[a:b]), None if masks is None else ptr(masks[a:b]), b - a, H, W, Kp, float(zfar),
                               ptr(np.ascontiguousarray(trip[a:b])) if n_hyp else None, n_hyp, float(tol), ptr(pl) if n_hyp else None,
                               ptr(ct) if n_hyp else None, ptr(bs), stream_ptr(dev)))
    planes[a:b], counts[a:b], best[a:b] = pl, ct, bs
  return planes, counts, best


def plane_moments(depths, K, planes, tol, masks=None, zfar=100, device='cuda'):
  """fp_plane_moments on (n,H,W) maps: planes (4,) or (n,4) -> (n,10) float64 numpy: n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz over the
  usable pixels within tol of the view's plane.  Synchronises."""
  dev, depths, masks, _, _ = _maps_on(depths, masks, device)
  n, H, W = depths.shape
  planes = _planes_of(planes, n)
  Kd, Kp = k_ptr(K)
  sums = np.zeros((n, _lib.FP_PLANE_MOMENT_TERMS), np.float64)
  for a in range(0, n, MAX_VIEWS):
    b = min(a + MAX_VIEWS, n)
    sm = np.ascontiguousarray(sums[a:b])
    check(lib().fp_plane_moments(_lib.Context.get(dev).handle, ptr(depths[a:b]), None if masks is None else ptr(masks[a:b]), b - a, H, W, Kp, float(zfar),
                                 ptr(np.ascontiguousarray(planes[a:b])), float(tol), ptr(sm), stream_ptr(dev)))
    sums[a:b] = sm
  return sums


def plane_from_moments(sums):
  """The least-squares plane of the 10 sums of fp_plane_moments, in float64: the eigenvector of the smallest eigenvalue of the covariance
  through the centroid, oriented so that the camera (the origin) is on the positive side.  Returns (plane (4,), eigenvalues (3,) ascending);
  needs at least 3 points."""
  s = np.asarray(sums, dtype=np.float64)
  n = s[0]
  if not n >= 3:
    raise ValueError(f'a plane needs at least 3 points, got {n:g}')
  mean = s[1:4] / n
  second = np.array([[s[4], s[5], s[6]], [s[5], s[7], s[8]], [s[6], s[8], s[9]]]) / n
  w, v = np.linalg.eigh(second - np.outer(mean, mean))
  nrm = v[:, 0]
  dd = -float(nrm @ mean)
  if dd < 0:
    nrm, dd = -nrm, -dd
  return np.array([nrm[0], nrm[1], nrm[2], dd]), w


def fit_plane(depth, K, mask=None, tol=0.005, n_hyp=512, seed=0, refits=2, zfar=100, device='cuda'):
  """The dominant plane of a depth map, (plane (4,) float64, info): plane = (n.x, n.y, n.z, dd) in the camera frame with the camera on the
  positive side, (n . p) + dd the height of a point above it.  The hypotheses are the planes through the three pixels of each row of
  np.random.RandomState(seed).randint(0, H*W, (n_hyp, 3)) - an unusable triplet simply scores 0, so the device input is explicit and
  reproducible; one fp_plane_score picks the hypothesis with the most usable pixels within `tol` metres, then `refits` rounds of
  fp_plane_moments and the least-squares solve on the host (plane_from_moments) over the pixels within `tol` of the current plane.
  depth (H,W) or a batch (n,H,W) (then plane is (n,4) and every entry of info has a leading n; each view gets the same triplets, so a
  view's plane does not depend on its batch), mask non-zero = usable; numpy arrays or device tensors.  info: counts (n_hyp,), best,
  hypothesis_plane (4,), inliers (refits,), eigenvalues (3,) of the last refit (ascending; zeros with refits=0).  ValueError when no
  hypothesis of a view has an inlier.  Synchronises."""
  dev, depths, masks, batch, _ = _maps_on(depth, mask, device)
  n, H, W = depths.shape
  n_hyp = int(n_hyp)
  if not 1 <= n_hyp <= _lib.FP_PLANE_MAX_HYP:
    raise ValueError(f'n_hyp must be in 1 .. {_lib.FP_PLANE_MAX_HYP}, got {n_hyp}')
  trip = np.random.RandomState(seed).randint(0, H * W, (n_hyp, 3)).astype(np.int32)
  hyp, counts, best = plane_score(depths, K, trip, tol, masks=masks, zfar=zfar)
  if (best < 0).any():
    raise ValueError(f'fit_plane: no hypothesis has an inlier in view(s) {np.nonzero(best < 0)[0].tolist()} ({n_hyp} triplets, seed {seed})')
  hyp_plane = hyp[np.arange(n), best].astype(np.float64)
  planes = hyp_plane.copy()
  inliers = np.zeros((n, int(refits)), np.int64)
  eig = np.zeros((n, 3))
  for r in range(int(refits)):
    sums = plane_moments(depths, K, planes, tol, masks=masks, zfar=zfar)
    inliers[:, r] = sums[:, 0].astype(np.int64)
    for v in range(n):
      if sums[v, 0] >= 3:      # fewer: the plane of the round before stands
        planes[v], eig[v] = plane_from_moments(sums[v])
  info = dict(counts=counts, best=best.astype(np.int64), hypothesis_plane=hyp_plane, inliers=inliers, eigenvalues=eig)
  if not batch:
    return planes[0], {k: v[0] for k, v in info.items()}
  return planes, info


def stats_from_rows(rows):
  """The statistics dict of segment_on_plane from the (k, FP_SEGMENT_STATS) int64 rows of fp_depth_segment_write of ONE view."""
  rows = np.asarray(rows, dtype=np.int64).reshape(-1, _lib.FP_SEGMENT_STATS)
  k = len(rows)
  npx = rows[:, 0]
  bounds = np.stack([rows[:, 8:11], rows[:, 11:14]], 1) / Q_SCALE
  return dict(label=np.arange(1, k + 1, dtype=np.int32), n_pixels=npx.copy(), bbox=rows[:, [1, 3, 2, 4]].copy(),
              centroid=rows[:, 5:8] / np.maximum(npx, 1)[:, None] / Q_SCALE, bounds=bounds,
              extent=np.linalg.norm(bounds[:, 1] - bounds[:, 0], axis=1), height=rows[:, 14] / Q_SCALE, lowest_pixel=rows[:, 15].copy(), rows=rows)


def segment_on_plane(depth, K, plane=None, mask=None, h_min=0.01, h_max=0.5, max_jump=0.01, min_pixels=200, zfar=100, device='cuda', **fit_kw):
  """What stands on a plane, cut into connected components: (labels, stats).  A pixel is foreground when its depth is usable (>= 0.001,
  < zfar, mask non-zero) and its height above `plane` is in [h_min, h_max] metres; two 4-neighbours are joined when both are foreground and
  their depths differ by at most `max_jump` metres (the gate of depth_normals); a component of at least `min_pixels` pixels is kept; the
  kept ones are numbered 1, 2, .. by their lowest pixel index, 0 is everything else.  plane=None: fit_plane(depth, K, mask, zfar=zfar,
  **fit_kw) first.  depth (H,W) or a batch (n,H,W) with one plane (4,) for all or (n,4); numpy arrays or device tensors.
  labels: int32, the shape of the depth - a device tensor when the depth was one (MultiObjectTracker.register takes it as it is), else
  numpy.  stats: a dict of numpy arrays with one entry per kept segment (a list of such dicts for a batch): label, n_pixels, bbox (rmin,
  cmin, rmax, cmax), centroid (3,) and bounds (2,3) in the camera frame, extent (the diagonal of bounds), height (the largest height above
  the plane), lowest_pixel, rows (the integers of fp_depth_segment_write they come from), plane and components (all of them, kept or
  not).  Exact: every number is an integer sum, minimum or maximum in 2^-20 m fixed point, the same in any batch.  Objects that touch
  without a depth step are one segment; there is one plane; nothing is recognised.  Synchronises."""
  dev, depths, masks, batch, on_device = _maps_on(depth, mask, device)
  n, H, W = depths.shape
  planes = _planes_of(fit_plane(depths, K, mask=masks, zfar=zfar, **fit_kw)[0] if plane is None else plane, n)
  Kd, Kp = k_ptr(K)
  ctx = _lib.Context.get(dev)
  labels = torch.empty((n, H, W), dtype=torch.int32, device=dev)
  out = []
  for a in range(0, n, MAX_VIEWS):
    b = min(a + MAX_VIEWS, n)
    counts = np.zeros((b - a, 2), np.int32)
    pl = np.ascontiguousarray(planes[a:b])
    check(lib().fp_depth_segment_count(ctx.handle, ptr(depths[a:b]), None if masks is None else ptr(masks[a:b]), b - a, H, W, Kp, float(zfar), ptr(pl),
                                       float(h_min), float(h_max), float(max_jump), int(min_pixels), ptr(counts), stream_ptr(dev)))
    kept = int(counts[:, 1].sum())
    rows = torch.empty((kept, _lib.FP_SEGMENT_STATS), dtype=torch.int64, device=dev)
    check(lib().fp_depth_segment_write(ctx.handle, ptr(depths[a:b]), b - a, H, W, ptr(labels[a:b]), ptr(rows) if kept else None, kept, stream_ptr(dev)))
    rows = rows.cpu().numpy()
    ends = np.concatenate([[0], np.cumsum(counts[:, 1])])
    for v in range(b - a):
      st = stats_from_rows(rows[ends[v]:ends[v + 1]])
      st.update(plane=planes[a + v].copy(), components=int(counts[v, 0]))
      out.append(st)
  if not on_device:
    labels = labels.cpu().numpy()
  return (labels, out) if batch else (labels[0], out[0])


def assign_segments(stats, diameters, K=None, prefer='size'):
  """Which segment is which object: (labels, cost) - labels[o] the label of the segment given to object o, for
  MultiObjectTracker.register(rgb, depth, K, label_image, labels=labels); cost (n_objects, n_segments) float64 = |extent_s - diameter_o|,
  so that a caller can see an ambiguous assignment.  Greedy by increasing cost; equal costs go to the lower object index, then to the
  lower label; each segment serves one object.  An object left without a segment gets a negative label, which matches no pixel (register
  handles an empty mask): -1 for the first such object, -2 for the next, .. - register wants the labels pairwise different.
  This rule is the project's own, not the reference's, and it is by SIZE only: objects of similar diameter cannot be told apart by it
  (look at `cost`, or assign them yourself, e.g. by position from stats['centroid']).  `K` is not needed by prefer='size', the one rule
  there is; it is in the signature for rules that look at the image.  Runs on the host."""
  if prefer != 'size':
    raise ValueError(f"prefer must be 'size', got {prefer!r}")
  diam = np.asarray(diameters, dtype=np.float64).reshape(-1)
  extent = np.asarray(stats['extent'], dtype=np.float64).reshape(-1)
  seg = np.asarray(stats['label']).reshape(-1)
  cost = np.abs(extent[None, :] - diam[:, None])
  order = sorted((cost[o, s], o, int(seg[s]), s) for o in range(len(diam)) for s in range(len(seg)))
  labels, used = [None] * len(diam), set()
  for _, o, lab, s in order:
    if labels[o] is None and s not in used:
      labels[o] = lab
      used.add(s)
  free = 0
  for o in range(len(diam)):
    if labels[o] is None:
      free += 1
      labels[o] = -free
  return labels, cost
