"""The drawing rule of fp_draw_poses (include/foundationpose_amd.h) restated in numpy float64, vectorised over the frame.  Written from the
rule's text, not from the kernel: no tiles, no culling, no clipping to the frame - every segment is blended over every pixel of the
window its capsule can reach (outside it the coverage is 0 by the rule itself)."""
import numpy as np

BOX, AXES, FILL, CONTOUR = 1, 2, 4, 8
ZNEAR = 0.01
MAX_COORD = 2.0 ** 20


def make_object(bbox, offset=None, axis_scale=0.1, box_color=(0, 255, 0), axis_color=((255, 0, 0), (0, 255, 0), (0, 0, 255)), fill_color=None):
  """One object as the C structure holds it: float32 box / offset / scale, uint8 colours"""
  return dict(bbox=np.asarray(bbox, dtype=np.float32).reshape(2, 3), offset=np.asarray(np.eye(4) if offset is None else offset, dtype=np.float32).reshape(4, 4),
              axis_scale=np.float32(axis_scale), box_color=np.asarray(box_color, dtype=np.uint8), axis_color=np.asarray(axis_color, dtype=np.uint8).reshape(3, 3),
              fill_color=np.asarray(box_color if fill_color is None else fill_color, dtype=np.uint8))


def object_segments(ob):
  """[(p0, p1, colour, is_axis)] of one object in the rule's order: x-edges over (y, z), y-edges over (x, z), z-edges over (x, y), each
  min before max; then the axes x, y, z"""
  b = ob['bbox'].astype(np.float64)
  lo, hi = np.minimum(b[0], b[1]), np.maximum(b[0], b[1])
  segs = []
  for axis in range(3):
    others = [c for c in range(3) if c != axis]
    for first in (lo, hi):
      for second in (lo, hi):
        p0, p1 = np.zeros(3), np.zeros(3)
        p0[axis], p1[axis] = lo[axis], hi[axis]
        p0[others[0]] = p1[others[0]] = first[others[0]]
        p0[others[1]] = p1[others[1]] = second[others[1]]
        segs.append((p0, p1, ob['box_color'], False))
  for axis in range(3):
    p1 = np.zeros(3)
    p1[axis] = float(ob['axis_scale'])
    segs.append((np.zeros(3), p1, ob['axis_color'][axis], True))
  return segs


def project_segment(p0, p1, M, K):
  """The rule's endpoints: None (dropped) or (unrounded (2,2) [[u0, v0], [u1, v1]], rounded (2,2))"""
  c0, c1 = M[:3, :3] @ p0 + M[:3, 3], M[:3, :3] @ p1 + M[:3, 3]
  if not (c0[2] >= ZNEAR) and not (c1[2] >= ZNEAR):
    return None
  if c0[2] < ZNEAR or c1[2] < ZNEAR:
    inside, outside = (c1, c0) if c0[2] < ZNEAR else (c0, c1)
    t = (ZNEAR - inside[2]) / (outside[2] - inside[2])
    cut = inside + t * (outside - inside)
    cut[2] = ZNEAR
    c0, c1 = (cut, c1) if c0[2] < ZNEAR else (c0, cut)
  uv = np.array([[K[0] @ c / c[2], K[1] @ c / c[2]] for c in (c0, c1)])
  r = np.round(uv)
  if not np.all(np.abs(r) <= MAX_COORD):
    return None
  return uv, r


def segments(K, poses, objs, flags, box_thickness, axis_thickness):
  """Every kept segment of the call in drawing order: dict(uv unrounded, xy rounded, half = thickness / 2 + 0.5, color)"""
  K = np.asarray(K, dtype=np.float64).reshape(3, 3)
  out = []
  for pose, ob in zip(np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4), objs):
    M = pose.astype(np.float64) @ ob['offset'].astype(np.float64)
    for p0, p1, color, is_axis in object_segments(ob):
      if not (flags & (AXES if is_axis else BOX)):
        continue
      pr = project_segment(p0, p1, M, K)
      if pr is None:
        continue
      th = float(np.float32(axis_thickness if is_axis else box_thickness))
      out.append(dict(uv=pr[0], xy=pr[1], half=th / 2 + 0.5, color=color.astype(np.float64)))
  return out


def endpoint_margin(segs):
  """The smallest distance of an unrounded endpoint coordinate to a half-integer (where rounding flips)"""
  if not segs:
    return np.inf
  uv = np.concatenate([s['uv'].reshape(-1) for s in segs])
  return float(np.min(np.abs(uv - np.floor(uv) - 0.5)))


def _blend_segment(c, touched, seg, opacity):
  H, W = c.shape[:2]
  (x0, y0), (x1, y1) = seg['xy']
  reach = seg['half'] + 1
  ulo, uhi = int(max(0, np.floor(min(x0, x1) - reach))), int(min(W - 1, np.ceil(max(x0, x1) + reach)))
  vlo, vhi = int(max(0, np.floor(min(y0, y1) - reach))), int(min(H - 1, np.ceil(max(y0, y1) + reach)))
  if ulo > uhi or vlo > vhi:
    return
  xs, ys = np.meshgrid(np.arange(ulo, uhi + 1, dtype=np.float64), np.arange(vlo, vhi + 1, dtype=np.float64))
  dx, dy = x1 - x0, y1 - y0
  l2 = dx * dx + dy * dy
  if l2 == 0:
    d = np.hypot(xs - x0, ys - y0)
  else:
    t = np.clip(((xs - x0) * dx + (ys - y0) * dy) / l2, 0.0, 1.0)
    d = np.hypot(xs - (x0 + t * dx), ys - (y0 + t * dy))
  a = np.clip(seg['half'] - d, 0.0, 1.0) * opacity
  win = c[vlo:vhi + 1, ulo:uhi + 1]
  win += a[..., None] * (seg['color'][None, None, :] - win)
  touched[vlo:vhi + 1, ulo:uhi + 1] |= a > 0


def draw(img, K, poses, objs, flags=BOX | AXES, box_thickness=2, axis_thickness=3, opacity=1.0, fill_alpha=0.0, owner=None):
  """(out uint8 (H,W,3), touched bool (H,W), segs): the rule applied to `img`.  The scalar arguments count as the float32 values the C
  structure holds."""
  img = np.asarray(img)
  H, W = img.shape[:2]
  c = img.astype(np.float64)
  touched = np.zeros((H, W), dtype=bool)
  opacity, fill_alpha = float(np.float32(opacity)), float(np.float32(fill_alpha))
  n = len(objs)
  segs = []
  if n and flags:
    if flags & (FILL | CONTOUR):
      own = np.asarray(owner).astype(np.int64)
      own = np.where((own >= 0) & (own < n), own, -1)
      valid = own >= 0
      if flags & FILL:
        fill = np.stack([ob['fill_color'] for ob in objs]).astype(np.float64)[np.maximum(own, 0)]
        c = np.where(valid[..., None], c + fill_alpha * (fill - c), c)
        touched |= valid
      if flags & CONTOUR:
        edge = np.zeros((H, W), dtype=bool)
        edge[1:] |= own[1:] != own[:-1]
        edge[:-1] |= own[:-1] != own[1:]
        edge[:, 1:] |= own[:, 1:] != own[:, :-1]
        edge[:, :-1] |= own[:, :-1] != own[:, 1:]
        edge &= valid
        line = np.stack([ob['box_color'] for ob in objs]).astype(np.float64)[np.maximum(own, 0)]
        c = np.where(edge[..., None], line, c)
        touched |= edge
    segs = segments(K, poses, objs, flags, box_thickness, axis_thickness)
    for s in segs:
      _blend_segment(c, touched, s, opacity)
  return np.clip(np.rint(c), 0, 255).astype(np.uint8), touched, segs
