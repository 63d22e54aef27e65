"""Finding an object in a depth frame without a mask: depth templates rendered from the model and matched against the whole frame on the
device (fp_template_match, csrc/detect.hip; the rule is stated in include/foundationpose_amd.h and restated in numpy by
tests/detect_oracle.py).

    ts = build_templates(mesh)                                  # once per object: 42 views x 12 in-plane rolls, 64 + 48 samples each
    dets = detect(depth, K, ts, top_k=4)                        # [{'ob_in_cam', 'centre', 'in_fraction', 'out_fraction', 'pixel', 'template', ..}]
    keys, counts = match_templates(depth, K, ts, return_counts=True)      # the primitive: the best candidate of every anchor pixel

The reference has nothing in this place (a person paints the mask, src/masking.py); the rule is the library's own.  With the depth known
at the anchor pixel there is no scale search: a candidate is (template rotation, anchor sample, anchor pixel) and its centre follows in
closed form.  What comes out is what register needs - a few centres with a rough rotation; the trained refiner and scorer make the final
choice (FoundationPose.register_detected).
**Limits: geometry only, nothing learned; a candidate whose anchor pixel is occluded or has no reading is lost (anchors > 1 gives it
further chances at that many times the work); the templates are rendered with the object on the optical axis, so towards the frame's edge
the object is seen up to the half field of view off the template's direction; a thin or flat object lying on a surface has little depth
step to show; clutter of the model's size scores like the model, and a compact template of a wrong rotation often outscores the right one
at the right place - the best centre is typically 5 cm off along the ray - which is why several centres go on to
the networks.**
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, k_ptr, lib, ptr, stream_ptr

_MIN_DEPTH = 0.001


class TemplateSet:
  """The templates of one or several objects.  table (T, n_in + n_out, 4) float32: per template its in-samples (the first `anchors` of them
  are the anchors), then its out-samples, each the offset (x, y, z, 0) in metres from the object's centre in camera axes; rotations
  (T, 3, 3) float64, R_t of every template; ranges (n_obj + 1) int32: object o owns templates ranges[o] .. ranges[o + 1] - 1; diameters
  (n_obj,); dropped: per object the (index into the rotation grid, reason) of every template that was not kept."""

  def __init__(self, table, rotations, n_in, n_out, anchors, ranges, diameters, dropped):
    self.table = np.ascontiguousarray(table, dtype=np.float32)
    self.rotations = np.ascontiguousarray(rotations, dtype=np.float64)
    self.n_in, self.n_out, self.anchors = int(n_in), int(n_out), int(anchors)
    self.ranges = np.ascontiguousarray(ranges, dtype=np.int32)
    self.diameters = np.asarray(diameters, dtype=np.float64).reshape(-1)
    self.dropped = list(dropped)
    check_table_limits(self.n_in, self.n_out, self.anchors, np.diff(self.ranges))
    if self.table.shape != (self.ranges[-1], self.n_in + self.n_out, 4) or self.rotations.shape != (self.ranges[-1], 3, 3):
      raise ValueError(f'table {self.table.shape} and rotations {self.rotations.shape} do not hold {self.ranges[-1]} templates of '
                       f'{self.n_in} + {self.n_out} samples')
    self._device = {}

  n_obj = property(lambda self: len(self.ranges) - 1)
  n_templates = property(lambda self: int(self.ranges[-1]))

  def device_table(self, device):
    """The table on `device`, uploaded once."""
    dev = torch.device(device)
    dev = torch.device('cuda', torch.cuda.current_device()) if dev.type == 'cuda' and dev.index is None else dev
    if dev not in self._device:
      self._device[dev] = torch.as_tensor(self.table).to(dev).contiguous()
    return self._device[dev]

  @staticmethod
  def concat(sets):
    """Several objects' sets as one, for one match call over all of them: the sample counts and `anchors` must agree."""
    sets = list(sets)
    if not sets:
      raise ValueError('TemplateSet.concat of nothing')
    first = sets[0]
    for s in sets[1:]:
      if (s.n_in, s.n_out, s.anchors) != (first.n_in, first.n_out, first.anchors):
        raise ValueError(f'sets of {(s.n_in, s.n_out, s.anchors)} and {(first.n_in, first.n_out, first.anchors)} (n_in, n_out, anchors) cannot be concatenated')
    counts = np.concatenate([np.diff(s.ranges) for s in sets])
    return TemplateSet(np.concatenate([s.table for s in sets]), np.concatenate([s.rotations for s in sets]), first.n_in, first.n_out, first.anchors,
                       np.concatenate([[0], np.cumsum(counts)]), np.concatenate([s.diameters for s in sets]), sum((s.dropped for s in sets), []))


def check_table_limits(n_in, n_out, anchors, counts):
  """What fp_template_match refuses about a table, said on the host: the key holds the score in 16 bits and 4 t + a in 16 bits."""
  if n_in < 1 or n_out < 1 or n_in * n_out > 65535:
    raise ValueError(f'n_in {n_in}, n_out {n_out}: each >= 1 and n_in n_out <= 65535 (the score takes 16 bits of the key)')
  if n_in + n_out > _lib.FP_TEMPLATE_MAX_SAMPLES:
    raise ValueError(f'{n_in + n_out} samples a template (at most {_lib.FP_TEMPLATE_MAX_SAMPLES})')
  if not 1 <= anchors <= min(_lib.FP_TEMPLATE_MAX_ANCHORS, n_in):
    raise ValueError(f'anchors {anchors} (1 .. {_lib.FP_TEMPLATE_MAX_ANCHORS}, at most n_in)')
  counts = np.asarray(counts).reshape(-1)
  if len(counts) < 1 or len(counts) > _lib.FP_TEMPLATE_MAX_OBJECTS:
    raise ValueError(f'{len(counts)} objects (1 .. {_lib.FP_TEMPLATE_MAX_OBJECTS})')
  if (counts < 0).any() or (4 * counts > 65536).any():
    raise ValueError(f'{int(counts.max())} templates of one object (at most 16384: 4 T <= 65536)')


def template_rotations(n_views=42, inplane_step=30):
  """(T, 3, 3) float64: the icosphere viewpoints times the in-plane rolls, inverted to ob_in_cam, in the order make_rotation_grid builds
  its grid - without its symmetry clustering, so a template index is (view, roll)."""
  from . import Utils as U
  views = U.sample_views_icosphere(n_views=n_views)
  rolls = [U.euler_matrix(0, 0, a) for a in np.deg2rad(np.arange(0, 360, inplane_step))]
  return np.asarray([np.linalg.inv(cam_in_ob @ roll)[:3, :3] for cam_in_ob in views for roll in rolls])


def _grow(m):
  """3 x 3 dilation of a boolean image (the border counts as False)."""
  p = np.pad(m, 1)
  h, w = m.shape
  out = np.zeros_like(m)
  for dr in range(3):
    for dc in range(3):
      out |= p[dr:dr + h, dc:dc + w]
  return out


def _template_samples(depth, f, cx, cy, z0, n_in, n_out, anchors, margin_px):
  """The samples of one rendered depth map, (n_in + n_out, 3) float64, or the reason why there are none."""
  sil = depth >= _MIN_DEPTH
  if not sil.any():
    return None, 'the render is empty'
  core = ~_grow(~sil)                                    # eroded by one pixel: all eight neighbours rendered
  rows, cols = np.nonzero(core)                          # scan order
  if len(rows) < n_in:
    return None, f'the eroded silhouette has {len(rows)} pixels, fewer than n_in = {n_in}'
  pick = np.floor((np.arange(n_in) + 0.5) * len(rows) / n_in).astype(np.int64)
  pr, pc = rows[pick], cols[pick]
  z = depth[pr, pc].astype(np.float64)
  s_in = np.stack([(pc - cx) / f * z, (pr - cy) / f * z, z - z0], axis=1)
  # the anchors: the sample nearest the centre ray, then farthest-point sampling among the samples (the lowest index at a tie)
  chosen = [int(np.argmin(s_in[:, 0] ** 2 + s_in[:, 1] ** 2))]
  while len(chosen) < anchors:
    gap = np.min(np.linalg.norm(s_in[:, None] - s_in[chosen][None], axis=2), axis=1)
    gap[chosen] = -1.0
    chosen.append(int(np.argmax(gap)))
  s_in = s_in[chosen + [i for i in range(n_in) if i not in chosen]]
  # the ring margin_px (chessboard distance) outside the silhouette
  grown = sil
  for _ in range(margin_px - 1):
    grown = _grow(grown)
  outer = _grow(grown)
  if outer[0].any() or outer[-1].any() or outer[:, 0].any() or outer[:, -1].any():
    return None, 'the silhouette with its margin does not fit the render'
  rr, rc = np.nonzero(outer & ~grown)
  if len(rr) < n_out:
    return None, f'the ring has {len(rr)} pixels, fewer than n_out = {n_out}'
  sr, sc = np.nonzero(sil)
  by_angle = np.argsort(np.arctan2(rr - sr.mean(), rc - sc.mean()), kind='stable')
  pick = by_angle[np.floor((np.arange(n_out) + 0.5) * len(rr) / n_out).astype(np.int64)]
  qr, qc = rr[pick], rc[pick]
  nearest = np.argmin((sr[None] - qr[:, None]) ** 2 + (sc[None] - qc[:, None]) ** 2, axis=1)      # the first in scan order at a tie
  z = depth[sr[nearest], sc[nearest]].astype(np.float64)
  s_out = np.stack([(qc - cx) / f * z, (qr - cy) / f * z, z - z0], axis=1)
  return np.concatenate([s_in, s_out]), None


def templates_from_depths(depths, f, z0, rotations, diameter, n_in=64, n_out=48, anchors=1, margin_px=6):
  """The TemplateSet of one object from the depth maps (T, s, s) of its centred model rendered at [R_t | (0, 0, z0)] by a pinhole camera of
  focal length f with the principal point at the centre pixel ((s - 1) / 2).  Deterministic numpy on those maps.
  In-samples: n_in pixels of the silhouette eroded by one pixel, spread evenly over it in scan order, back-projected and expressed
  relative to the centre, S = (X, Y, Z - z0); the anchors - the sample nearest the centre ray, further ones by farthest-point sampling
  among the samples - come first.  Out-samples: n_out pixels of the ring margin_px outside the silhouette, spread evenly over the ring's
  pixels sorted by angle about the silhouette's centroid; each takes the depth of its nearest silhouette pixel and is back-projected the
  same way.  A template whose render is empty, too small or does not fit the render is dropped and reported in `dropped`."""
  depths = np.asarray(depths, dtype=np.float32)
  rotations = np.asarray(rotations, dtype=np.float64)
  if depths.ndim != 3 or depths.shape[1] != depths.shape[2] or rotations.shape != (len(depths), 3, 3):
    raise ValueError(f'depths must be (T, s, s) with rotations (T, 3, 3), got {depths.shape} and {rotations.shape}')
  if margin_px < 1:
    raise ValueError(f'margin_px {margin_px} (>= 1)')
  check_table_limits(n_in, n_out, anchors, [0])
  c = (depths.shape[1] - 1) / 2.0
  rows, kept, dropped = [], [], []
  for t, d in enumerate(depths):
    s, why = _template_samples(d, float(f), c, c, float(z0), n_in, n_out, anchors, int(margin_px))
    if s is None:
      dropped.append((t, why))
    else:
      rows.append(s), kept.append(t)
  table = np.zeros((len(rows), n_in + n_out, 4), np.float32)
  if rows:
    table[:, :, :3] = np.asarray(rows)
  return TemplateSet(table, rotations[kept].reshape(-1, 3, 3), n_in, n_out, anchors, [0, len(rows)], [diameter], dropped)


def render_camera(extent, render_size=96, z0=0.7):
  """(f, K) of the template render: the model's circumscribed sphere of diameter `extent` spans half the render at distance z0, so the
  silhouette and its margin fit at every rotation."""
  f = 0.5 * render_size * z0 / extent
  c = (render_size - 1) / 2.0
  return f, np.array([[f, 0, c], [0, f, c], [0, 0, 1.0]])


def build_templates(mesh=None, mesh_tensors=None, n_views=42, inplane_step=30, n_in=64, n_out=48, anchors=1, margin_px=6, render_size=96,
                    z0=0.7, diameter=None, glctx=None, chunk=256):
  """The TemplateSet of one object: its model - a mesh or a mesh_tensors dict, centred on the point that is to count as its centre
  (FoundationPose.mesh is) - rendered by the library's rasteriser at template_rotations(n_views, inplane_step) and (0, 0, z0), `chunk`
  poses a call, then templates_from_depths.  n_views=42 (504 templates) is the default because 162 (1944 templates) found the object no
  more often in the scenes of DESIGN.md section 5 and costs more than a registration; diameter: the object's (the default radius of detect's suppression is half of it); None
  takes the diameter of the circumscribed sphere about the origin."""
  from . import Utils as U
  if mesh_tensors is None:
    mesh_tensors = U.make_mesh_tensors(mesh)
  extent = 2.0 * float(torch.linalg.norm(mesh_tensors['pos'].double(), dim=1).max())
  if not extent > 0 or not z0 > extent:
    raise ValueError(f'z0 {z0} must exceed the extent of the model about its origin, {extent}')
  f, K = render_camera(extent, render_size, z0)
  rot = template_rotations(n_views, inplane_step)
  poses = np.tile(np.eye(4), (len(rot), 1, 1))
  poses[:, :3, :3] = rot
  poses[:, 2, 3] = z0
  if glctx is None:
    glctx = U.RasterizeContext(mesh_tensors['pos'].device)
  depths = []
  for i in range(0, len(poses), chunk):
    _, d, _ = U.nvdiffrast_render(K=K, H=render_size, W=render_size, ob_in_cams=poses[i:i + chunk], glctx=glctx, mesh_tensors=mesh_tensors)
    depths.append(d.cpu().numpy())
  return templates_from_depths(np.concatenate(depths), f, z0, rot, extent if diameter is None else float(diameter), n_in=n_in, n_out=n_out,
                               anchors=anchors, margin_px=margin_px)


def lattice_shape(H, W, stride, offset=(0, 0)):
  """(Hs, Ws) of the anchor lattice: pixels (r0 + i stride, c0 + j stride) inside the frame."""
  return (H - offset[0] + stride - 1) // stride, (W - offset[1] + stride - 1) // stride


def match_templates(depth, K, templates, stride=4, offset=(0, 0), tol_in=0.015, tol_out=0.06, z_range=(0.05, 20.0), zfar=np.inf,
                    anchors=None, return_counts=False, device='cuda'):
  """fp_template_match: the best candidate of every anchor pixel.  depth: float32 metres (H, W), or (n, H, W) for a batch of frames;
  templates: a TemplateSet.  Returns keys (n_obj, Hs, Ws), with a batch (n, n_obj, Hs, Ws), uint32: (score << 16) | (0xFFFF - (4 t_local + a)),
  0 where there is no candidate (decode_keys takes them apart); return_counts adds n_in_pass << 16 | n_out_pass of the winner:
  (keys, counts).  numpy in gives numpy out; a device tensor in gives device tensors out without a host copy or a synchronisation.
  anchors: how many of the set's anchors to try (None: all of them).  The same bits on every run and in any batch."""
  on_device = torch.is_tensor(depth) and depth.is_cuda
  dev = depth.device if on_device else torch.device(device)
  t = torch.as_tensor(depth)
  if t.dtype != torch.float32:
    raise ValueError(f'depth must be float32, got {t.dtype}')
  if t.dim() not in (2, 3):
    raise ValueError(f'depth must be (H, W) or (n, H, W), got {tuple(t.shape)}')
  batch = t.dim() == 3
  t = t if batch else t[None]
  n, H, W = t.shape
  stride, r0, c0 = int(stride), int(offset[0]), int(offset[1])
  if stride < 1 or not (0 <= r0 < H and 0 <= c0 < W):
    raise ValueError(f'stride {stride} (>= 1) and offset {(r0, c0)} (inside the {H} x {W} frame)')
  if not (tol_in > 0 and tol_out > 0):
    raise ValueError(f'tol_in {tol_in} and tol_out {tol_out} must be > 0')
  if not z_range[0] <= z_range[1]:
    raise ValueError(f'z_range {z_range}: the least depth of a centre exceeds the greatest')
  if not float(zfar) > 0:
    raise ValueError(f'zfar must be > 0, got {zfar}')
  anchors = templates.anchors if anchors is None else int(anchors)
  if not 1 <= anchors <= templates.anchors:
    raise ValueError(f'anchors {anchors} (1 .. {templates.anchors}, what the set was built with)')
  Kd, Kp = k_ptr(K)
  if not (np.isfinite(Kd).all() and Kd[0, 0] > 0 and Kd[1, 1] > 0):
    raise ValueError('K must be finite with positive focal lengths')
  Hs, Ws = lattice_shape(H, W, stride, (r0, c0))
  t = t.to(dev).contiguous()
  empty = n == 0 or templates.n_templates == 0      # nothing to launch: no frame, or no template and so no candidate
  keys = (torch.zeros if empty else torch.empty)((n, templates.n_obj, Hs, Ws), dtype=torch.uint32, device=dev)
  counts = (torch.zeros if empty else torch.empty)(keys.shape, dtype=torch.uint32, device=dev) if return_counts else None
  table = templates.device_table(dev)
  if not empty:
    check(lib().fp_template_match(_lib.Context.get(dev).handle, ptr(t), n, H, W, Kp, ptr(table), ptr(templates.ranges), templates.n_obj, templates.n_in,
                                  templates.n_out, anchors, stride, r0, c0, float(z_range[0]), float(z_range[1]), float(zfar), float(tol_in),
                                  float(tol_out), ptr(keys), ptr(counts), stream_ptr(dev)))

  def finish(x):
    x = x if batch else x[0]
    return x if on_device else x.cpu().numpy()
  return (finish(keys), finish(counts)) if return_counts else finish(keys)


def staged_templates(n_in, n_out):
  """How many templates of n_in + n_out samples the kernel stages at once (fp_template_match_info)."""
  out = _lib.c_int()
  check(lib().fp_template_match_info(int(n_in) + int(n_out), _lib.byref(out)))
  return out.value


def decode_keys(keys):
  """(score, t_local, anchor) of uint32 keys as numpy int64 arrays; where a key is 0 there is no candidate."""
  k = np.asarray(keys).astype(np.int64)
  low = 0xFFFF - (k & 0xFFFF)
  return k >> 16, low >> 2, low & 3


def candidate_centres(templates, obj, t_local, anchor, rows, cols, d, K):
  """The centres (n, 3) float64 of candidates: the anchor pixel (rows, cols) back-projected at its depth d minus the anchor sample."""
  K = np.asarray(K, dtype=np.float64)
  A = templates.table[templates.ranges[obj] + t_local, anchor, :3].astype(np.float64)
  d = np.asarray(d, dtype=np.float64)
  return np.stack([(cols - K[0, 2]) / K[0, 0] * d - A[:, 0], (rows - K[1, 2]) / K[1, 1] * d - A[:, 1], d - A[:, 2]], axis=1)


def detections_from_keys(keys, counts, depth, K, templates, top_k=4, stride=4, offset=(0, 0), nms_radius=None, min_score=0.0):
  """Greedy non-maximum suppression per object on the host, in float64, from the downloaded maps of ONE frame: keys, counts
  (n_obj, Hs, Ws), depth (H, W).  Candidates go by key descending, the lower flat index first among equal keys; one whose centre lies
  within nms_radius (a number, or one per object; None: half the object's diameter) of an accepted one is dropped, as is one whose score
  is below min_score n_in n_out.  Returns per object a list of up to top_k records: ob_in_cam (4, 4) float64 = [R_t | centre], centre,
  score, in_fraction, out_fraction, pixel (row, col), template (index into the set), anchor, object."""
  keys, depth = np.asarray(keys), np.asarray(depth)
  Hs, Ws = keys.shape[1:]
  full = templates.n_in * templates.n_out
  radii = templates.diameters / 2 if nms_radius is None else np.broadcast_to(np.asarray(nms_radius, dtype=np.float64), (templates.n_obj,))
  out = []
  for o in range(templates.n_obj):
    flat = keys[o].reshape(-1).astype(np.int64)
    order = np.argsort(-flat, kind='stable')
    score, t_local, anchor = decode_keys(flat[order])
    keep = (flat[order] > 0) & (score >= min_score * full)
    order, score, t_local, anchor = order[keep], score[keep], t_local[keep], anchor[keep]
    rows, cols = offset[0] + (order // Ws) * stride, offset[1] + (order % Ws) * stride
    centres = candidate_centres(templates, o, t_local, anchor, rows, cols, depth[rows, cols], K)
    found, taken = [], np.zeros((0, 3))
    for n in range(len(order)):
      if len(found) >= top_k:
        break
      if len(taken) and (np.linalg.norm(taken - centres[n], axis=1) <= radii[o]).any():
        continue
      taken = np.concatenate([taken, centres[n:n + 1]])
      t = int(templates.ranges[o] + t_local[n])
      pose = np.eye(4)
      pose[:3, :3], pose[:3, 3] = templates.rotations[t], centres[n]
      rec = dict(ob_in_cam=pose, centre=centres[n].copy(), score=int(score[n]), pixel=(int(rows[n]), int(cols[n])), template=t,
                 anchor=int(anchor[n]), object=o)
      if counts is not None:
        cnt = int(np.asarray(counts)[o].reshape(-1)[order[n]])
        rec['in_fraction'], rec['out_fraction'] = (cnt >> 16) / templates.n_in, (cnt & 0xFFFF) / templates.n_out
      found.append(rec)
    out.append(found)
  return out


def detect(depth, K, templates, top_k=4, stride=4, tol_in=0.015, tol_out=0.06, z_range=(0.05, 20.0), nms_radius=None, min_score=0.0,
           zfar=np.inf, offset=(0, 0), anchors=None, device='cuda'):
  """Up to top_k detections of each object of `templates` in ONE depth frame (H, W) float32 metres, numpy or a device tensor:
  match_templates on the device, then detections_from_keys on the host.  Returns the list of records of a single-object set, a list of
  such lists (one per object) of a concatenated one.  The defaults of the tolerances and of the builder's sample counts and margin were
  fixed with the numpy oracle over seeded clutter scenes."""
  if torch.as_tensor(depth).dim() != 2:
    raise ValueError('detect takes one frame (H, W); match_templates takes a batch')
  keys, counts = match_templates(depth, K, templates, stride=stride, offset=offset, tol_in=tol_in, tol_out=tol_out, z_range=z_range, zfar=zfar,
                                 anchors=anchors, return_counts=True, device=device)
  if torch.is_tensor(keys):
    keys, counts = keys.cpu().numpy(), counts.cpu().numpy()
  host = depth.detach().cpu().numpy() if torch.is_tensor(depth) else np.asarray(depth)
  found = detections_from_keys(keys, counts, host, K, templates, top_k=top_k, stride=stride, offset=offset, nms_radius=nms_radius, min_score=min_score)
  return found[0] if templates.n_obj == 1 else found
