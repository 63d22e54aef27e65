"""One frame on the device and one C call per frame: what FoundationPose._run_frame, MultiObjectTracker.track and
MultiObjectTracker.register share.  `frame_sections` / `is_packed` say how a frame lies in ONE byte buffer, `FrameBuffer` owns that buffer
(the upload rule is stated there, once) and `GraphedCall` is the hipGraph capture protocol of a frame's call.
"""
import numpy as np
import torch


def frame_sections(H, W, rgb_u8, labels=False, n_masks=0):
  """Byte (offset, size) of every section of a frame buffer, in buffer order: depth f32 | labels i32 (optional) | rgb (u8 or f32) |
  masks u8 (optional, n_masks x H x W); a section that is absent is not listed, the sections leave no gaps (the buffer's size is the end
  of the last one) and every float32 / int32 section lies before every byte section, so on a 4-byte boundary.  The tracking layout (no
  labels, no masks) is
  [depth | rgb] with rgb at exactly H * W * 4: what a caller packs to upload a frame with one device copy (is_packed)."""
  HW = H * W
  sizes = [('depth', HW * 4), ('labels', HW * 4 if labels else 0), ('rgb', HW * 3 * (1 if rgb_u8 else 4)), ('masks', n_masks * HW)]
  out, at = {}, 0
  for name, size in sizes:
    if size:
      out[name] = (at, size)
      at += size
  return out


def is_packed(depth, rgb):
  """True if `depth` (float32) and `rgb` already lie as the tracking layout [depth | rgb]: both contiguous, in one storage, rgb beginning
  exactly H * W * 4 bytes behind depth."""
  return (depth.is_contiguous() and rgb.is_contiguous() and depth.untyped_storage().data_ptr() == rgb.untyped_storage().data_ptr() and
          rgb.data_ptr() == depth.data_ptr() + depth.numel() * 4)


_NP = {torch.float: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}


class FrameBuffer:
  """The static device buffers of a frame: ONE byte buffer laid out by frame_sections with typed views `depth / labels / rgb / masks`
  (None where absent), its pinned host twin, and the depth prelude's outputs `depth_f / xyz / rgb_f` (rgb_f None for a float frame).

  Upload rule (`put`), the same for every caller.  If NO input is a device tensor (numpy arrays, CPU tensors), the frame is written into
  the pinned twin and goes up in ONE non-blocking host-to-device copy.  Otherwise every input is copied into its own section - a device
  tensor by a device copy, a host array of a mixed frame by a host-to-device copy of its own - except that depth and rgb go up in ONE
  device copy when they already lie packed (is_packed) and the buffer holds no label image between them.  Either way depth is stored as
  float32, rgb as uint8 or float32, a label image as int32 and mask o as the bytes `masks[o] != 0`."""

  def __init__(self, H, W, rgb_u8, device, labels=False, n_masks=0):
    sec = frame_sections(H, W, rgb_u8, labels, n_masks)
    self.H, self.W, self.rgb_u8 = int(H), int(W), bool(rgb_u8)
    self.frame = torch.empty((sum(n for _, n in sec.values()),), dtype=torch.uint8, device=device)
    self.host = torch.empty_like(self.frame, device='cpu').pin_memory()
    shapes = dict(depth=(torch.float, (H, W)), labels=(torch.int32, (H, W)), rgb=(torch.uint8 if rgb_u8 else torch.float, (H, W, 3)),
                  masks=(torch.uint8, (n_masks, H, W)))
    hb, self._host = self.host.numpy(), {}
    for name, (dtype, shape) in shapes.items():
      at, size = sec.get(name, (0, 0))
      setattr(self, name, self.frame[at:at + size].view(dtype).reshape(shape) if size else None)
      self._host[name] = hb[at:at + size].view(_NP[dtype]).reshape(-1) if size else None
    if n_masks:
      self._host['masks'] = self._host['masks'].view(bool).reshape(n_masks, -1)
    self._packed = self.frame[:sec['rgb'][0] + sec['rgb'][1]] if not labels else None      # [depth | rgb], where they are neighbours
    self.depth_f = torch.empty((H, W), dtype=torch.float, device=device)
    self.xyz = torch.empty((H, W, 3), dtype=torch.float, device=device)
    self.rgb_f = torch.empty((H, W, 3), dtype=torch.float, device=device) if rgb_u8 else None

  def put(self, rgb, depth, labels=None, masks=None):
    """Store one frame (see the class docstring for the route it takes); the copies are enqueued on the current stream."""
    inputs = [rgb, depth] + ([] if labels is None else [labels]) + (list(masks) if masks is not None else [])
    if not any(torch.is_tensor(x) and x.is_cuda for x in inputs):
      h = self._host
      h['depth'][:] = np.asarray(depth).reshape(-1)
      h['rgb'][:] = np.asarray(rgb).reshape(-1)
      if labels is not None:
        h['labels'][:] = np.asarray(labels).reshape(-1)
      for o, m in enumerate(masks or ()):
        np.not_equal(np.asarray(m).reshape(-1), 0, out=h['masks'][o])
      self.frame.copy_(self.host, non_blocking=True)
      return
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    d = t(depth).to(torch.float)
    r = t(rgb) if self.rgb_u8 else t(rgb).to(torch.float)
    if self._packed is not None and is_packed(d, r):
      self._packed.copy_(torch.as_strided(d.view(torch.uint8).reshape(-1), (self._packed.numel(),), (1,)))
    else:
      self.depth.copy_(d)
      self.rgb.copy_(r)
    if labels is not None:
      self.labels.copy_(t(labels))
    if masks is not None:
      for o, m in enumerate(masks):
        self.masks[o].copy_(t(m) != 0)

  def fill(self, args):
    """The frame fields of FpTrackArgs, FpTrackObjectsArgs or FpRegisterObjectsArgs."""
    args.d_rgb, args.rgb_is_u8, args.d_depth, args.H, args.W = self.rgb.data_ptr(), 1 if self.rgb_u8 else 0, self.depth.data_ptr(), self.H, self.W
    args.d_depth_f, args.d_xyz = self.depth_f.data_ptr(), self.xyz.data_ptr()
    args.d_rgb_f = self.rgb_f.data_ptr() if self.rgb_u8 else None
    if hasattr(args, 'd_labels'):
      args.d_labels = self.labels.data_ptr() if self.labels is not None else None


class GraphedCall:
  """A frame's C call, run eagerly or replayed as ONE hipGraph.  `call()` makes the C call on the current stream and checks its return
  code; `keep` is the device tensor (the pose, or the poses) the call refines in place, which warm-up and capture must leave as they found
  it; `reserve` is the hypothesis count the library's arena is reserved for before every eager call.  The graph is captured at the first
  graphed frame, after two eager passes on a side stream, and again whenever the arena has moved since (ctx.arena_generation(): the
  captured addresses are stale); `drop()` forgets it."""

  def __init__(self, ctx, call, keep, reserve):
    self.ctx, self.call, self.keep, self.reserve = ctx, call, keep, int(reserve)
    self.graph = None                                      # (torch.cuda.CUDAGraph, arena generation at capture)

  def drop(self):
    self.graph = None

  def __call__(self, st, graphed):
    """Run the frame on stream `st` (the current one): the replay of its graph if `graphed`, else the eager call."""
    ctx, call = self.ctx, self.call
    if not graphed:
      ctx.reserve(self.reserve)
      call()
      return
    g = self.graph
    if g is not None and g[1] != ctx.arena_generation():
      g = None                                             # the library's arena moved: the captured addresses are stale
    if g is None:
      ctx.reserve(self.reserve)
      keep = self.keep.clone()
      side = torch.cuda.Stream()
      side.wait_stream(st)
      with torch.cuda.stream(side):                        # eager passes first: lazy initialisation, allocator warm-up
        for _ in range(2):
          call()
          self.keep.copy_(keep)
      st.wait_stream(side)
      graph = torch.cuda.CUDAGraph()
      with torch.cuda.graph(graph):
        call()
      self.keep.copy_(keep)                                # (capturing does not execute)
      g = self.graph = (graph, ctx.arena_generation())
    g[0].replay()
