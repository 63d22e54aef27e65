"""Multi-hypothesis tracking (BASELINE.json configs[4]: "track_one() with 64-hypothesis refine per frame").

The reference's track_one refines exactly one pose (src/estimater.py:263) and never scores; the 64-hypothesis mode is this
build's extension on top of the same two predictors: the previous pose plus n-1 fixed, seeded perturbations of it are
refined together, scored by ScoreNet, and the best one becomes the new pose (FoundationPose.track_multi).  The
perturbation set is a constant of (n, seed, sigmas), so the CPU oracle and the HIP path start from identical hypotheses.
"""
import ctypes
import functools

import numpy as np
import torch


@functools.lru_cache(maxsize=8)
def perturbation_set(n, trans_sigma=0.01, rot_sigma_deg=5.0, seed=0):
  """(n,4,4) float32: identity first, then n-1 small rigid motions [dR | dt] with dt ~ N(0, trans_sigma) per axis and
  dR = exp(hat(w)), w ~ N(0, rot_sigma) per axis."""
  rs = np.random.RandomState(seed)
  out = np.tile(np.eye(4), (n, 1, 1))
  dt = rs.randn(n, 3) * trans_sigma
  w = rs.randn(n, 3) * np.deg2rad(rot_sigma_deg)
  for i in range(1, n):
    th = np.linalg.norm(w[i])
    Kx = np.array([[0, -w[i, 2], w[i, 1]], [w[i, 2], 0, -w[i, 0]], [-w[i, 1], w[i, 0], 0]])
    out[i, :3, :3] = np.eye(3) + (np.sin(th) / max(th, 1e-12)) * Kx + ((1 - np.cos(th)) / max(th * th, 1e-12)) * (Kx @ Kx)
    out[i, :3, 3] = dt[i]
  return out.astype(np.float32)


@functools.lru_cache(maxsize=8)
def _device_set(n, trans_sigma, rot_sigma_deg, seed, device):
  """The perturbation set on `device`, uploaded once (no host copy per frame: a frame can be captured in a hipGraph)."""
  return torch.as_tensor(perturbation_set(n, trans_sigma, rot_sigma_deg, seed), device=device)


def tracking_hypotheses(pose, n, trans_sigma=0.01, rot_sigma_deg=5.0, seed=0):
  """pose (4,4) tensor -> (n,4,4) hypotheses on its device: R_i = dR_i R, t_i = t + dt_i (the egocentric update form of
  the refiner, src/Utils.py:848-855); hypothesis 0 is `pose` itself."""
  P = _device_set(int(n), float(trans_sigma), float(rot_sigma_deg), int(seed), str(pose.device))
  pose = pose.reshape(4, 4).to(torch.float)
  hyp = torch.eye(4, dtype=torch.float, device=pose.device).repeat(n, 1, 1)
  hyp[:, :3, :3] = P[:, :3, :3] @ pose[:3, :3]
  hyp[:, :3, 3] = pose[:3, 3] + P[:, :3, 3]
  return hyp


def registration_hypotheses(rot_grids, stats, K):
  """generate_random_pose_hypo of several objects in one launch (fp_register_hypotheses): `rot_grids` a list of (n_o,4,4) device tensors,
  `stats` the objects' mask_depth_stats (Utils.mask_depth_stats_objects).  Returns the (sum n_o, 4, 4) hypotheses, object after object."""
  from ._lib import Context, check, lib, ptr, stream_ptr
  grids = [g.to(torch.float).contiguous() for g in rot_grids]
  n = len(grids)
  dev = grids[0].device
  st = (ctypes.c_int32 * (6 * n))(*[int(s[k]) for s in stats for k in ('cmin', 'cmax', 'rmin', 'rmax', 'n_mask', 'n_usable')])
  med = (ctypes.c_float * n)(*[float(s['median']) for s in stats])
  Kinv = np.ascontiguousarray(np.linalg.inv(K), dtype=np.float64)
  out = torch.empty((sum(len(g) for g in grids), 4, 4), dtype=torch.float, device=dev)
  check(lib().fp_register_hypotheses(Context.get(dev).handle, (ctypes.c_void_p * n)(*[g.data_ptr() for g in grids]), (ctypes.c_int * n)(*[len(g) for g in grids]),
                                     n, st, med, Kinv.ctypes.data, ptr(out), stream_ptr(dev)))
  return out


class MultiObjectTracker:
  """track_one for several objects of ONE camera stream in one call per frame (fp_track_objects, a build extension): the frame is uploaded
  once, its depth prelude runs once, and every refinement iteration is one render, one observed-crop and one network pass over all the
  objects' images instead of one of each per object.

      tracker = MultiObjectTracker([est_a, est_b, est_c])      # registered FoundationPose instances sharing one PoseRefinePredictor
      poses = tracker.track(rgb, depth, K, iteration=2)        # np (n_obj, 4, 4) float32: row o = what est_o.track_one would return
      tracker.enable_graph(True)                               # one hipGraph per (objects, frame size, camera, iteration)
      poses = tracker.register(rgb, depth, K, masks)           # the first poses of all objects in one call (fp_register_objects)

  Each object's pose is what its estimator's track_one gives, except for the last bits of the network pass: its kernels depend on the
  number of images, so a frame of K objects matches K separate track_one calls only within tolerance (one object:
  bit for bit).  Contract, as in FoundationPose._run_frame: after a frame every estimator's `pose_last` is a (1,4,4) VIEW of this
  tracker's static buffers, overwritten by its next frame of the same kind; a later `est.track_one` continues from it, and an estimator
  whose `pose_last` was set elsewhere since (register, track_one, assignment) has it reloaded at the start of the next frame.  The returned
  array is a copy.  No debug canvases: unlike track_one at `debug >= 2`, this call produces no refiner visualisation."""

  def __init__(self, estimators):
    from ._lib import FP_TRACK_MAX_OBJECTS
    ests = list(estimators)
    if not 1 <= len(ests) <= FP_TRACK_MAX_OBJECTS:
      raise ValueError(f'MultiObjectTracker: {len(ests)} estimators given; it tracks 1 .. {FP_TRACK_MAX_OBJECTS} objects')
    r0 = ests[0].refiner
    for i, e in enumerate(ests):
      if any(e is f for f in ests[:i]):
        raise ValueError(f'MultiObjectTracker: estimator {i} is listed twice; each estimator holds the pose of one object')
      if getattr(e, 'dist_group', None) is not None:
        raise ValueError(f'MultiObjectTracker: estimator {i} has a dist_group; sharded estimators track with track_one')
      if e.refiner.ctx is not r0.ctx or e.refiner.model.handle.value != r0.model.handle.value:
        raise ValueError(f'MultiObjectTracker: estimator {i} does not share estimator 0\'s refiner (refiner.model.handle and refiner.ctx): '
                         'one network pass needs one RefineNet')
    self.estimators = ests
    self._ws = {}
    self._graph_on = False

  def enable_graph(self, on=True):
    """Replay a frame as ONE hipGraph, captured at the first frame of a given (objects, frame size, camera, iteration) after two eager
    warm-up frames, and re-captured when the library's workspace is re-allocated."""
    self._graph_on = bool(on)
    for ws in self._ws.values():
      ws['graph'] = None

  def _workspace(self, iteration, shape, is_u8, K):
    from . import _lib
    ests = self.estimators
    key = (int(iteration), tuple(shape), bool(is_u8), np.asarray(K, dtype=np.float64).tobytes(),
           tuple((id(e.mesh_tensors['pos']), float(e.diameter), np.asarray(e.model_center, dtype=np.float64).tobytes()) for e in ests))
    ws = self._ws.get(key)
    if ws is not None:
      return ws
    n, (H, W) = len(ests), shape
    ctx = ests[0].refiner.ctx
    dev = ests[0].mesh_tensors['pos'].device
    n_rgb = H * W * 3 * (1 if is_u8 else 4)
    frame = torch.empty((H * W * 4 + n_rgb,), dtype=torch.uint8, device=dev)
    ws = dict(frame=frame, depth=frame[:H * W * 4].view(torch.float).reshape(H, W),
              rgb=(frame[H * W * 4:].reshape(H, W, 3) if is_u8 else frame[H * W * 4:].view(torch.float).reshape(H, W, 3)),
              host=torch.empty((H * W * 4 + n_rgb,), dtype=torch.uint8).pin_memory(),
              depth_f=torch.empty((H, W), dtype=torch.float, device=dev), xyz=torch.empty((H, W, 3), dtype=torch.float, device=dev),
              rgb_f=torch.empty((H, W, 3), dtype=torch.float, device=dev) if is_u8 else None,
              poses=torch.eye(4, dtype=torch.float, device=dev).repeat(n, 1, 1).contiguous(),
              pose_of_mesh=torch.zeros((n, 4, 4), dtype=torch.float).pin_memory(),
              Kd=np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(3, 3)), cfg=ests[0].refiner._c_cfg(), holds=[None] * n, graph=None)
    ws['meshes'] = [_lib.device_mesh(ctx, e.mesh_tensors) for e in ests]
    objs = (_lib.FpTrackObject * n)()
    for o, e in enumerate(ests):
      objs[o].mesh, objs[o].mesh_diameter = ws['meshes'][o].handle, float(e.diameter)
      objs[o].model_center[:] = [float(x) for x in np.asarray(e.model_center, dtype=np.float32)]
      objs[o].d_pose, objs[o].d_pose_of_mesh = ws['poses'][o].data_ptr(), ws['pose_of_mesh'][o].data_ptr()
    a = _lib.FpTrackObjectsArgs()
    a.struct_size = ctypes.sizeof(a)
    a.refine_net = ests[0].refiner.model.handle
    a.d_rgb, a.rgb_is_u8, a.d_depth, a.H, a.W = ws['rgb'].data_ptr(), 1 if is_u8 else 0, ws['depth'].data_ptr(), H, W
    a.K, a.refine_cfg = ws['Kd'].ctypes.data, ctypes.addressof(ws['cfg'])
    a.iteration, a.n_obj, a.objs = int(iteration), n, ctypes.addressof(objs)
    a.d_depth_f, a.d_xyz = ws['depth_f'].data_ptr(), ws['xyz'].data_ptr()
    a.d_rgb_f = ws['rgb_f'].data_ptr() if is_u8 else None
    ws['objs'], ws['args'] = objs, a
    self._ws[key] = ws
    return ws

  def track(self, rgb, depth, K, iteration=2):
    """One frame: np (n_obj, 4, 4) float32, row o = est_o's pose @ get_tf_to_centered_mesh() (what est_o.track_one returns)."""
    from ._lib import check, lib, stream_ptr
    for i, e in enumerate(self.estimators):
      if e.pose_last is None:
        raise ValueError(f'MultiObjectTracker: estimator {i} has no pose to track from (pose_last is None): register it first')
    ctx = self.estimators[0].refiner.ctx
    is_np = isinstance(rgb, np.ndarray)
    is_u8 = (rgb.dtype == np.uint8) if is_np else (rgb.dtype == torch.uint8)
    H, W = depth.shape[:2]
    self._last_frame = (int(H), int(W), K)
    ws = self._workspace(iteration, (H, W), is_u8, K)
    # the frame as in FoundationPose._run_frame: ONE host-to-device copy through pinned memory, or one device copy of a packed [depth | rgb]
    if is_np or not torch.is_tensor(depth) or not depth.is_cuda:
      hb = ws['host'].numpy()
      hb[:H * W * 4].view(np.float32)[:] = np.asarray(depth.cpu() if torch.is_tensor(depth) else depth, dtype=np.float32).reshape(-1)
      r = np.asarray(rgb.cpu() if torch.is_tensor(rgb) else rgb)
      if is_u8:
        hb[H * W * 4:] = r.reshape(-1)
      else:
        hb[H * W * 4:].view(np.float32)[:] = r.astype(np.float32, copy=False).reshape(-1)
      ws['frame'].copy_(ws['host'], non_blocking=True)
    else:
      d = depth.to(torch.float)
      r = rgb if is_u8 else rgb.to(torch.float)
      packed = (d.is_contiguous() and r.is_contiguous() and d.untyped_storage().data_ptr() == r.untyped_storage().data_ptr() and
                r.data_ptr() == d.data_ptr() + H * W * 4)
      if packed:
        ws['frame'].copy_(torch.as_strided(d.view(torch.uint8).reshape(-1), (ws['frame'].numel(),), (1,)))
      else:
        ws['depth'].copy_(d)
        ws['rgb'].copy_(r)
    # each pose lives in the workspace and is refined in place; reloaded only when pose_last was set by someone else
    for o, e in enumerate(self.estimators):
      if ws['holds'][o] is not e.pose_last:
        ws['poses'][o].copy_(torch.as_tensor(e.pose_last, device=ws['poses'].device, dtype=torch.float).reshape(4, 4))
    st = torch.cuda.current_stream(ws['poses'].device)
    run = lambda: check(lib().fp_track_objects(ctx.handle, ctypes.byref(ws['args']), stream_ptr(ws['poses'].device)))
    if self._graph_on:
      g = ws['graph']
      if g is not None and g[1] != ctx.arena_generation():
        g = None                                            # the library's arena moved: the captured addresses are stale
      if g is None:
        ctx.reserve(64)
        keep = ws['poses'].clone()
        side = torch.cuda.Stream()
        side.wait_stream(st)
        with torch.cuda.stream(side):                        # eager passes first: lazy initialisation, allocator warm-up
          for _ in range(2):
            run()
            ws['poses'].copy_(keep)
        st.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
          run()
        ws['poses'].copy_(keep)                              # (capturing does not execute)
        g = ws['graph'] = (graph, ctx.arena_generation())
      g[0].replay()
    else:
      ctx.reserve(64)
      run()
    st.synchronize()                                         # the results were written to pinned host memory by the frame's last launch
    out = ws['pose_of_mesh'].numpy().copy()
    for o, e in enumerate(self.estimators):
      e.pose_last = ws['poses'][o].reshape(1, 4, 4)
      ws['holds'][o] = e.pose_last
    self._returned = [(e.pose_last, out[o].copy()) for o, e in enumerate(self.estimators)]
    return out

  def _check_register(self, depth, masks, labels):
    """The argument checks of register(): (H, W, label image or None, list of masks or None); ValueError names the cause."""
    ests = self.estimators
    s0 = ests[0].scorer
    for i, e in enumerate(ests):
      if e.scorer.ctx is not s0.ctx or e.scorer.model.handle.value != s0.model.handle.value:
        raise ValueError(f'MultiObjectTracker.register: estimator {i} does not share estimator 0\'s scorer (scorer.model.handle and scorer.ctx): '
                         'one network pass needs one ScoreNet')
    if s0.ctx is not ests[0].refiner.ctx:
      raise ValueError('MultiObjectTracker.register: the scorer and the refiner live in different contexts (scorer.ctx, refiner.ctx)')
    H, W = (int(x) for x in depth.shape[:2])
    is_image = (isinstance(masks, np.ndarray) or torch.is_tensor(masks)) and masks.ndim == 2
    if is_image:
      if labels is None:
        raise ValueError('MultiObjectTracker.register: one (H, W) label image needs labels=[id_0, ...], the id of every object')
      labels = [int(x) for x in labels]
      if len(labels) != len(ests):
        raise ValueError(f'MultiObjectTracker.register: {len(labels)} labels for {len(ests)} objects')
      if len(set(labels)) != len(labels):
        raise ValueError(f'MultiObjectTracker.register: a label is repeated in {labels}; each object has its own id')
      if tuple(masks.shape) != (H, W):
        raise ValueError(f'MultiObjectTracker.register: the label image is {tuple(masks.shape)}, the depth image {(H, W)}: the shapes differ')
      return H, W, masks, None, labels
    if labels is not None:
      raise ValueError('MultiObjectTracker.register: labels= goes with one (H, W) label image, not with a list of masks')
    masks = list(masks)
    if len(masks) != len(ests):
      raise ValueError(f'MultiObjectTracker.register: {len(masks)} masks for {len(ests)} objects')
    for o, m in enumerate(masks):
      if tuple(m.shape) != (H, W):
        raise ValueError(f'MultiObjectTracker.register: mask {o} is {tuple(m.shape)}, the depth image {(H, W)}: the shapes differ')
    return H, W, None, masks, None

  def register(self, rgb, depth, K, masks, iteration=5, labels=None, max_pass_hyp=0):
    """FoundationPose.register for every object of ONE frame in one call (fp_register_objects): np (n_obj, 4, 4) float32, row o = what
    `self.estimators[o].register(K, rgb, depth, masks[o], iteration=iteration)` returns.  `masks`: a sequence of n_obj (H,W) masks (anything
    non-zero = object; they may overlap, each object sees its own) or ONE (H,W) integer label image with `labels=[id_0, ...]` (pixel ==
    id_o: object o) - numpy arrays or device tensors.  The frame goes up once, the depth prelude and the mask reductions of all objects
    run once, the networks run over the hypotheses of all objects in passes of at most `max_pass_hyp` hypotheses (0: 1008), cut at object
    boundaries; one host wait (the mask reductions: the validity test needs them) and one at the end.

    Afterwards every registered estimator holds what its own register() leaves: pose_last, poses / scores (best first), best_id, H, W, K,
    ob_mask; `track` can follow at once.  An object with fewer than 4 usable mask pixels is not registered: its row is eye(4) with the
    guessed translation (register() returns that as float64; here it is rounded to the array's float32) and its estimator stays as it was.
    set_seed(0) is called once, as register() does.  No debug canvases: unlike register() at `debug >= 2`, this call writes nothing."""
    from . import _lib, Utils as U
    from ._lib import check, lib, stream_ptr
    ests = self.estimators
    H, W, label_img, mask_list, labels = self._check_register(depth, masks, labels)
    self._last_frame = (H, W, K)
    U.set_seed(0)
    for e in ests:
      if e.glctx is None:
        e.glctx = U.RasterizeContext()
    n = len(ests)
    ctx = ests[0].refiner.ctx
    dev = ests[0].mesh_tensors['pos'].device
    is_u8 = (rgb.dtype == np.uint8) if isinstance(rgb, np.ndarray) else (rgb.dtype == torch.uint8)
    HW = H * W
    n_lab, n_rgb, n_msk = (HW * 4 if label_img is not None else 0), HW * 3 * (1 if is_u8 else 4), (0 if label_img is not None else n * HW)
    key = (H, W, is_u8, label_img is not None)
    ws = self._reg_ws.get(key) if hasattr(self, '_reg_ws') else None
    if ws is None:
      if not hasattr(self, '_reg_ws'):
        self._reg_ws = {}
      # the frame, the label image or the masks behind one another in ONE buffer: host arrays go up in one copy
      frame = torch.empty((HW * 4 + n_lab + n_rgb + n_msk,), dtype=torch.uint8, device=dev)
      o_rgb, o_msk = HW * 4 + n_lab, HW * 4 + n_lab + n_rgb
      ws = self._reg_ws[key] = dict(
        frame=frame, host=torch.empty_like(frame, device='cpu').pin_memory(), depth=frame[:HW * 4].view(torch.float).reshape(H, W),
        labels=frame[HW * 4:o_rgb].view(torch.int32).reshape(H, W) if n_lab else None,
        rgb=frame[o_rgb:o_msk].reshape(H, W, 3) if is_u8 else frame[o_rgb:o_msk].view(torch.float).reshape(H, W, 3),
        masks=frame[o_msk:].reshape(n, H, W) if n_msk else None,
        depth_f=torch.empty((H, W), dtype=torch.float, device=dev), xyz=torch.empty((H, W, 3), dtype=torch.float, device=dev),
        rgb_f=torch.empty((H, W, 3), dtype=torch.float, device=dev) if is_u8 else None,
        pose_of_mesh=torch.zeros((n, 4, 4), dtype=torch.float).pin_memory())
    host_in = all(isinstance(x, np.ndarray) for x in [rgb, depth] + ([label_img] if mask_list is None else mask_list))
    if host_in:
      hb = ws['host'].numpy()
      view = lambda t: hb[t.data_ptr() - ws['frame'].data_ptr():][:t.numel() * t.element_size()].view(
        {torch.float: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}[t.dtype]).reshape(tuple(t.shape))
      view(ws['depth'])[:] = depth
      view(ws['rgb'])[:] = rgb
      if label_img is not None:
        view(ws['labels'])[:] = label_img
      else:
        mv = view(ws['masks'])
        for o, m in enumerate(mask_list):
          np.not_equal(m, 0, out=mv[o].view(bool))
      ws['frame'].copy_(ws['host'], non_blocking=True)
    else:
      up = lambda x: torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x).to(dev)
      ws['depth'].copy_(up(depth))
      ws['rgb'].copy_(up(rgb))
      if label_img is not None:
        ws['labels'].copy_(up(label_img))
      else:
        for o, m in enumerate(mask_list):
          ws['masks'][o].copy_(up(m) != 0)
    Kd = np.ascontiguousarray(np.asarray(K.detach().cpu().numpy() if torch.is_tensor(K) else K, dtype=np.float64).reshape(3, 3))
    Kinv = np.ascontiguousarray(np.linalg.inv(K.detach().cpu().numpy() if torch.is_tensor(K) else K), dtype=np.float64)
    cfg = ests[0].refiner._c_cfg()
    meshes = [_lib.device_mesh(ctx, e.mesh_tensors) for e in ests]
    grids = [e.rot_grid.to(device=dev, dtype=torch.float).contiguous() for e in ests]
    out_p = [torch.empty((len(g), 4, 4), dtype=torch.float, device=dev) for g in grids]
    out_s = [torch.empty((len(g),), dtype=torch.float, device=dev) for g in grids]
    out_o = [torch.empty((len(g),), dtype=torch.int64, device=dev) for g in grids]
    objs = (_lib.FpRegisterObject * n)()
    for o, e in enumerate(ests):
      objs[o].mesh, objs[o].mesh_diameter = meshes[o].handle, float(e.diameter)
      objs[o].model_center[:] = [float(x) for x in np.asarray(e.model_center, dtype=np.float32)]
      objs[o].d_mask = ws['masks'][o].data_ptr() if label_img is None else None
      objs[o].label = labels[o] if labels is not None else 0
      objs[o].d_rot_grid, objs[o].n_hyp = grids[o].data_ptr(), len(grids[o])
      objs[o].d_poses, objs[o].d_scores, objs[o].d_order = out_p[o].data_ptr(), out_s[o].data_ptr(), out_o[o].data_ptr()
      objs[o].d_pose_of_mesh = ws['pose_of_mesh'][o].data_ptr()
    a = _lib.FpRegisterObjectsArgs()
    a.struct_size = ctypes.sizeof(a)
    a.refine_net, a.score_net = ests[0].refiner.model.handle, ests[0].scorer.model.handle
    a.d_rgb, a.rgb_is_u8, a.d_depth, a.H, a.W = ws['rgb'].data_ptr(), 1 if is_u8 else 0, ws['depth'].data_ptr(), H, W
    a.K, a.K_inv, a.refine_cfg = Kd.ctypes.data, Kinv.ctypes.data, ctypes.addressof(cfg)
    scfg = ests[0].scorer.cfg
    a.score_crop_ratio, a.score_normalize_xyz = float(scfg['crop_ratio']), 1 if scfg['normalize_xyz'] else 0
    a.iteration, a.n_obj, a.objs = int(iteration), n, ctypes.addressof(objs)
    a.d_labels = ws['labels'].data_ptr() if label_img is not None else None
    a.max_pass_hyp = int(max_pass_hyp)
    a.d_depth_f, a.d_xyz = ws['depth_f'].data_ptr(), ws['xyz'].data_ptr()
    a.d_rgb_f = ws['rgb_f'].data_ptr() if is_u8 else None
    check(lib().fp_register_objects(ctx.handle, ctypes.byref(a), stream_ptr(dev)))
    torch.cuda.current_stream(dev).synchronize()             # the results were written to pinned host memory by the call's last launch
    out = np.empty((n, 4, 4), dtype=np.float32)
    for o, e in enumerate(ests):
      if not objs[o].registered:
        st = objs[o].stats
        stats = dict(cmin=st[0], cmax=st[1], rmin=st[2], rmax=st[3], n_mask=st[4], n_usable=st[5], median=np.float32(objs[o].median))
        out[o] = np.eye(4)
        out[o, :3, 3] = e.guess_translation(depth=None, mask=None, K=K, stats=stats)
        continue
      e.H, e.W, e.K, e.ob_id = H, W, K, None
      e.ob_mask = mask_list[o] if mask_list is not None else (label_img == labels[o])
      e.poses, e.scores, e.best_id = out_p[o], out_s[o], out_o[o][0]
      e.pose_last = e.poses[0]
      out[o] = ws['pose_of_mesh'][o].numpy()
    self._returned = [(e.pose_last if objs[o].registered else False, out[o].copy()) for o, e in enumerate(ests)]      # (False: never a pose_last)
    return out

  def instance_masks(self, depth=None, K=None, occluders=None, delta=0.015):
    """Which pixels every object covers at its current pose, after `register` / `track`: dict(owner (H,W) int32 device tensor, the
    object in front at the pixel, -1 = none; mask_visib (n_obj,H,W) uint8 0 / 255; visib_fract (n_obj,) float64 numpy, the visible
    fraction of each object's silhouette).  One Utils.scene_instances call (fp_scene_instances) over the estimators' centred meshes at
    their `pose_last`; the frame size and K (unless given) are those of the last frame.  depth=None: only the objects hide one another;
    with the frame's depth image (H,W) it hides them as well (occluders as in scene_instances)."""
    from . import Utils as U
    for i, e in enumerate(self.estimators):
      if e.pose_last is None:
        raise ValueError(f'MultiObjectTracker.instance_masks: estimator {i} has no pose yet (pose_last is None): register it first')
    if getattr(self, '_last_frame', None) is None:
      raise ValueError('MultiObjectTracker.instance_masks: no frame seen yet: call register or track first')
    H, W, K_last = self._last_frame
    dev = self.estimators[0].mesh_tensors['pos'].device
    poses = torch.stack([torch.as_tensor(e.pose_last, device=dev, dtype=torch.float).reshape(4, 4) for e in self.estimators])
    out = U.scene_instances(K_last if K is None else K, H, W, [e.mesh_tensors for e in self.estimators], poses, depth=depth, occluders=occluders,
                            delta=delta, want=('mask_visib', 'owner', 'info'), glctx=self.estimators[0].refiner.ctx)
    return dict(owner=out['owner'], mask_visib=out['mask_visib'], visib_fract=np.array([r['visib_fract'] for r in out['info']], dtype=np.float64))

  def draw(self, rgb, fill_alpha=0.0, contour=False, depth=None, **kw):
    """The frame `rgb` (H,W,3) uint8, numpy or device tensor, with every object's box and xyz axes at its current pose of the ORIGINAL
    mesh - the poses the last `register` / `track` returned - in one Utils.draw_poses call; the result is of the kind of `rgb`.  The box
    of object o is Utils.model_box of its mesh, in object o's palette colour.  fill_alpha > 0 tints each object's visible pixels,
    contour=True outlines them: the owner map then comes from instance_masks(depth=depth).  Other keywords go to Utils.draw_poses."""
    from . import Utils as U
    ests = self.estimators
    for i, e in enumerate(ests):
      if e.pose_last is None:
        raise ValueError(f'MultiObjectTracker.draw: estimator {i} has no pose yet (pose_last is None): register it first')
    if getattr(self, '_last_frame', None) is None:
      raise ValueError('MultiObjectTracker.draw: no frame seen yet: call register or track first')
    returned = getattr(self, '_returned', None) or [(None, None)] * len(ests)
    poses, boxes, offs = [], [], []
    for e, (held, pose) in zip(ests, returned):
      if held is not e.pose_last:                           # set elsewhere since: the pose of the original mesh as track_one forms it
        last = torch.as_tensor(e.pose_last, dtype=torch.float).reshape(4, 4)
        pose = (last.to(e.get_tf_to_centered_mesh().device) @ e.get_tf_to_centered_mesh()).cpu().numpy()
      to_origin, bbox = U.model_box(e.mesh_ori)
      poses.append(pose), boxes.append(bbox), offs.append(np.linalg.inv(to_origin))
    owner = None
    if fill_alpha > 0 or contour:
      owner = self.instance_masks(depth=depth)['owner']
    K = kw.pop('K', self._last_frame[2])
    return U.draw_poses(rgb, K, np.stack(poses), bboxes=np.stack(boxes), offsets=np.stack(offs), owner=owner, fill_alpha=fill_alpha, contour=contour,
                        glctx=ests[0].refiner.ctx, **kw)
