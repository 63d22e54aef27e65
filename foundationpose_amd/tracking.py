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
    self._ws, self._reg_ws = {}, {}          # workspaces of track() and of register(), by what they were built for
    self._graph_on = False
    self._last_frame = None                  # (H, W, K) of the last frame seen
    self._returned = None                    # per estimator (the pose_last handed out, the pose of the original mesh returned with it)

  def enable_graph(self, on=True):
    """Replay a frame as ONE hipGraph, captured at the first frame of a given (objects, frame size, camera, iteration) after two eager
    warm-up frames, and re-captured when the library's workspace is re-allocated (frame.GraphedCall)."""
    self._graph_on = bool(on)
    for ws in self._ws.values():
      ws['run'].drop()

  def _need_poses(self, who, frame=False):
    """Every estimator has a pose (and, with `frame`, a frame was seen), or ValueError in the name of the method `who`."""
    for i, e in enumerate(self.estimators):
      if e.pose_last is None:
        raise ValueError(f'MultiObjectTracker.{who}: estimator {i} has no pose yet (pose_last is None): register it first')
    if frame and self._last_frame is None:
      raise ValueError(f'MultiObjectTracker.{who}: no frame seen yet: call register or track first')

  def _workspace(self, iteration, shape, is_u8, K):
    from . import _lib
    from .frame import FrameBuffer, GraphedCall
    ests = self.estimators
    key = (int(iteration), tuple(shape), bool(is_u8), np.asarray(K, dtype=np.float64).tobytes(),
           tuple((id(e.mesh_tensors['pos']), float(e.diameter), np.asarray(e.model_center, dtype=np.float64).tobytes()) for e in ests))
    ws = self._ws.get(key)
    if ws is not None:
      return ws
    n = len(ests)
    ctx = ests[0].refiner.ctx
    dev = ests[0].mesh_tensors['pos'].device
    Kd, K_ptr = _lib.k_ptr(K)
    ws = dict(fb=FrameBuffer(*shape, is_u8, dev), poses=torch.eye(4, dtype=torch.float, device=dev).repeat(n, 1, 1).contiguous(),
              pose_of_mesh=torch.zeros((n, 4, 4), dtype=torch.float).pin_memory(), Kd=Kd, cfg=ests[0].refiner._c_cfg(), holds=[None] * n)
    ws['meshes'] = [_lib.device_mesh(ctx, e.mesh_tensors) for e in ests]
    objs = (_lib.FpTrackObject * n)()
    for o, e in enumerate(ests):
      objs[o].mesh, objs[o].mesh_diameter, objs[o].model_center = ws['meshes'][o].handle, float(e.diameter), _lib.center3(e.model_center)
      objs[o].d_pose, objs[o].d_pose_of_mesh = ws['poses'][o].data_ptr(), ws['pose_of_mesh'][o].data_ptr()
    a = _lib.FpTrackObjectsArgs()
    a.struct_size = ctypes.sizeof(a)
    a.refine_net = ests[0].refiner.model.handle
    ws['fb'].fill(a)
    a.K, a.refine_cfg = K_ptr, ctypes.addressof(ws['cfg'])
    a.iteration, a.n_obj, a.objs = int(iteration), n, ctypes.addressof(objs)
    ws['objs'], ws['args'] = objs, a
    track_objects, check, stream_ptr = _lib.lib().fp_track_objects, _lib.check, _lib.stream_ptr
    ws['run'] = GraphedCall(ctx, lambda: check(track_objects(ctx.handle, ctypes.byref(a), stream_ptr(dev))), ws['poses'], 64)
    self._ws[key] = ws
    return ws

  def track(self, rgb, depth, K, iteration=2):
    """One frame: np (n_obj, 4, 4) float32, row o = est_o's pose @ get_tf_to_centered_mesh() (what est_o.track_one returns)."""
    self._need_poses('track')
    is_u8 = rgb.dtype == (np.uint8 if isinstance(rgb, np.ndarray) else torch.uint8)
    H, W = depth.shape[:2]
    self._last_frame = (int(H), int(W), K)
    ws = self._workspace(iteration, (H, W), is_u8, K)
    ws['fb'].put(rgb, depth)                                 # (ONE copy: the rule of frame.FrameBuffer)
    # each pose lives in the workspace and is refined in place; reloaded only when pose_last was set by someone else
    for o, e in enumerate(self.estimators):
      if ws['holds'][o] is not e.pose_last:
        ws['poses'][o].copy_(torch.as_tensor(e.pose_last, device=ws['poses'].device, dtype=torch.float).reshape(4, 4))
    st = torch.cuda.current_stream(ws['poses'].device)
    ws['run'](st, self._graph_on)
    st.synchronize()                                         # the results were written to pinned host memory by the frame's last launch
    out = ws['pose_of_mesh'].numpy().copy()
    for o, e in enumerate(self.estimators):
      e.pose_last = ws['poses'][o].reshape(1, 4, 4)
      ws['holds'][o] = e.pose_last
    self._returned = [(e.pose_last, out[o].copy()) for o, e in enumerate(self.estimators)]
    return out

  def polish(self, depth, K, masks=None, iterations=None, dist_max=None, cos_min=None, crop=160, crop_ratio=1.2, max_jump=0.01, min_pixels=None,
             damping=None):
    """Move every object's pose onto the measured depth by geometry alone (fp_pose_polish, a build extension; off unless called): np
    (n_obj, 4, 4) float32, row o = est_o's polished pose @ get_tf_to_centered_mesh().  One fp_pose_polish per object, all on one stream,
    and ONE synchronisation at the end.  masks: None, or a sequence of n_obj (H,W) masks (non-zero = may be the object) that enter each
    object's observed normals and nothing else.  The other arguments are Utils.polish_poses' (None: its defaults).  Every estimator's
    `pose_last` becomes a fresh (1,4,4) tensor; `self.polish_info[o]` holds object o's fit (valid, rendered, observed, rms, stopped,
    xi_last): reported, not judged."""
    from . import _lib, pose_icp as PI
    self._need_poses('polish')
    ests = self.estimators
    if masks is not None and len(masks) != len(ests):
      raise ValueError(f'MultiObjectTracker.polish: {len(masks)} masks for {len(ests)} objects')
    pick = lambda v, d: d if v is None else v
    iterations, dist_max, cos_min = pick(iterations, PI.DEFAULT_ITERATIONS), pick(dist_max, PI.DEFAULT_DIST_MAX), pick(cos_min, PI.DEFAULT_COS_MIN)
    min_pixels, damping = pick(min_pixels, PI.DEFAULT_MIN_PIXELS), pick(damping, PI.DEFAULT_DAMPING)
    ctx = ests[0].refiner.ctx
    dev = ests[0].mesh_tensors['pos'].device
    depth = torch.as_tensor(depth, device=dev).to(torch.float).contiguous()
    H, W = depth.shape
    self._last_frame = (int(H), int(W), K)
    Kd, Kp = _lib.k_ptr(K)
    n = len(ests)
    if masks is None:
      normals = [PI.depth_normals(depth, K, None, max_jump=max_jump, device=dev)[0]] * n
    else:
      m = torch.stack([torch.as_tensor(x, device=dev) != 0 for x in masks])
      normals = list(PI.depth_normals(depth[None].expand(n, H, W).contiguous(), K, m, max_jump=max_jump, device=dev))
    poses = torch.stack([torch.as_tensor(e.pose_last, device=dev, dtype=torch.float).reshape(4, 4) for e in ests]).contiguous()
    state = PI.new_pose_state(n, dev)
    sums = torch.zeros((n, _lib.FP_POSE_ALIGN_TERMS), dtype=torch.float64, device=dev)
    counts = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    meshes = [_lib.device_mesh(ctx, e.mesh_tensors) for e in ests]
    for o, e in enumerate(ests):
      PI.enqueue_polish(ctx, meshes[o].handle, poses[o:o + 1], Kp, H, W, depth, normals[o], crop, crop_ratio, float(e.diameter), iterations, dist_max,
                        cos_min, damping, min_pixels, state[o:o + 1], sums[o:o + 1], counts[o:o + 1])
    of_mesh = torch.stack([poses[o] @ e.get_tf_to_centered_mesh().to(dev) for o, e in enumerate(ests)])
    out = of_mesh.cpu().numpy()                              # the one synchronisation
    info = PI.polish_info(state, counts)
    self.polish_info = [{k: v[o] for k, v in info.items()} for o in range(n)]
    for o, e in enumerate(ests):
      e.pose_last = poses[o].clone().reshape(1, 4, 4)
    self._returned = [(e.pose_last, out[o].copy()) for o, e in enumerate(ests)]
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
    from .frame import FrameBuffer
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
    is_u8 = rgb.dtype == (np.uint8 if isinstance(rgb, np.ndarray) else torch.uint8)
    key = (H, W, is_u8, label_img is not None)
    ws = self._reg_ws.get(key)
    if ws is None:
      # the frame, the label image or the masks behind one another in ONE buffer: host arrays go up in one copy
      ws = self._reg_ws[key] = dict(fb=FrameBuffer(H, W, is_u8, dev, labels=label_img is not None, n_masks=0 if mask_list is None else n),
                                    pose_of_mesh=torch.zeros((n, 4, 4), dtype=torch.float).pin_memory())
    fb = ws['fb']
    fb.put(rgb, depth, labels=label_img, masks=mask_list)
    Kd, K_ptr = _lib.k_ptr(K)
    Kinv = np.ascontiguousarray(np.linalg.inv(K.detach().cpu().numpy() if torch.is_tensor(K) else K), dtype=np.float64)
    cfg = ests[0].refiner._c_cfg()
    meshes = [_lib.device_mesh(ctx, e.mesh_tensors) for e in ests]
    grids = [e.rot_grid.to(device=dev, dtype=torch.float).contiguous() for e in ests]
    out_p = [torch.empty((len(g), 4, 4), dtype=torch.float, device=dev) for g in grids]
    out_s = [torch.empty((len(g),), dtype=torch.float, device=dev) for g in grids]
    out_o = [torch.empty((len(g),), dtype=torch.int64, device=dev) for g in grids]
    objs = (_lib.FpRegisterObject * n)()
    for o, e in enumerate(ests):
      objs[o].mesh, objs[o].mesh_diameter, objs[o].model_center = meshes[o].handle, float(e.diameter), _lib.center3(e.model_center)
      objs[o].d_mask = fb.masks[o].data_ptr() if label_img is None else None
      objs[o].label = labels[o] if labels is not None else 0
      objs[o].d_rot_grid, objs[o].n_hyp = grids[o].data_ptr(), len(grids[o])
      objs[o].d_poses, objs[o].d_scores, objs[o].d_order = out_p[o].data_ptr(), out_s[o].data_ptr(), out_o[o].data_ptr()
      objs[o].d_pose_of_mesh = ws['pose_of_mesh'][o].data_ptr()
    a = _lib.FpRegisterObjectsArgs()
    a.struct_size = ctypes.sizeof(a)
    a.refine_net, a.score_net = ests[0].refiner.model.handle, ests[0].scorer.model.handle
    fb.fill(a)
    a.K, a.K_inv, a.refine_cfg = K_ptr, Kinv.ctypes.data, ctypes.addressof(cfg)
    scfg = ests[0].scorer.cfg
    a.score_crop_ratio, a.score_normalize_xyz = float(scfg['crop_ratio']), 1 if scfg['normalize_xyz'] else 0
    a.iteration, a.n_obj, a.objs = int(iteration), n, ctypes.addressof(objs)
    a.max_pass_hyp = int(max_pass_hyp)
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

  def segment(self, depth, K, **kw):
    """Masks for `register` from the depth image alone, for objects standing on one plane: (label_image, labels) with label_image an
    (H,W) int32 DEVICE tensor (Utils.segment_on_plane; keywords go to it) and labels[o] the segment given to object o by
    Utils.assign_segments on the estimators' diameters - by size only, so objects of similar diameter cannot be told apart; an object
    without a segment gets a negative label, which matches no pixel.  `register(rgb, depth, K, label_image, labels=labels)` takes both
    without a host copy of the image.  Also leaves `self.segments` = dict(stats, cost) of the call."""
    from . import Utils as U
    dev = self.estimators[0].mesh_tensors['pos'].device
    depth = torch.as_tensor(depth, device=dev)
    if depth.dim() != 2:
      raise ValueError(f'MultiObjectTracker.segment: depth must be one (H,W) image, got {tuple(depth.shape)}')
    label_image, stats = U.segment_on_plane(depth, K, **kw)
    labels, cost = U.assign_segments(stats, [float(e.diameter) for e in self.estimators], K=K)
    self.segments = dict(stats=stats, cost=cost)
    return label_image, labels

  def detect(self, depth, K, delta=0.015, **kw):
    """Masks for `register` from the depth image and the models alone, with nothing said about the scene (Utils.detect; geometry only -
    see its limits): (detections, masks).  ONE match call runs over the concatenated template sets of all objects
    (FoundationPose.templates, built once per object); detections[o] is object o's best record - ob_in_cam of the CENTRED mesh, centre,
    pass fractions, anchor pixel, template - or None when the frame holds no candidate for it, and masks[o] the (H,W) uint8 DEVICE tensor
    (0 / 255) of the pixels the object shows at that pose in front of the frame's depth (Utils.scene_instances, mask_visib with the depth
    image and the other detections as occluders), all zero without a detection.  `tracker.register(rgb, depth, K, masks)` follows
    unchanged.  Two instances of one model get the same detection: give them apart by hand.  Keywords of Utils.build_templates go to the
    sets, the others to Utils.detect.  Also leaves `self.detections` = detections."""
    from . import Utils as U
    from .detect import TemplateSet
    ests = self.estimators
    build = {k: kw.pop(k) for k in ('n_views', 'inplane_step', 'n_in', 'n_out', 'anchors', 'margin_px', 'render_size', 'z0') if k in kw}
    dev = ests[0].mesh_tensors['pos'].device
    raw = torch.as_tensor(np.ascontiguousarray(depth) if isinstance(depth, np.ndarray) else depth, dtype=torch.float, device=dev)
    if raw.dim() != 2:
      raise ValueError(f'MultiObjectTracker.detect: depth must be one (H,W) image, got {tuple(raw.shape)}')
    H, W = (int(x) for x in raw.shape)
    sets = TemplateSet.concat([e.templates(**build) for e in ests])
    found = U.detect(ests[0]._prelude(raw), K, sets, top_k=1, **kw)
    found = [found] if len(ests) == 1 else found
    self.detections = [f[0] if f else None for f in found]
    masks = [torch.zeros((H, W), dtype=torch.uint8, device=dev) for _ in ests]
    have = [o for o, d in enumerate(self.detections) if d is not None]
    if have:
      out = U.scene_instances(K, H, W, [ests[o].mesh_tensors for o in have], np.stack([self.detections[o]['ob_in_cam'] for o in have]), depth=raw,
                              occluders='both', delta=delta, want=('mask_visib',), glctx=ests[0].refiner.ctx)
      for k, o in enumerate(have):
        masks[o] = out['mask_visib'][k]
    return self.detections, masks

  def instance_masks(self, depth=None, K=None, occluders=None, delta=0.015):
    """Which pixels every object covers at its current pose, after `register` / `track`: dict(owner (H,W) int32 device tensor, the
    object in front at the pixel, -1 = none; mask_visib (n_obj,H,W) uint8 0 / 255; visib_fract (n_obj,) float64 numpy, the visible
    fraction of each object's silhouette).  One Utils.scene_instances call (fp_scene_instances) over the estimators' centred meshes at
    their `pose_last`; the frame size and K (unless given) are those of the last frame.  depth=None: only the objects hide one another;
    with the frame's depth image (H,W) it hides them as well (occluders as in scene_instances)."""
    from . import Utils as U
    self._need_poses('instance_masks', frame=True)
    H, W, K_last = self._last_frame
    dev = self.estimators[0].mesh_tensors['pos'].device
    poses = torch.stack([torch.as_tensor(e.pose_last, device=dev, dtype=torch.float).reshape(4, 4) for e in self.estimators])
    out = U.scene_instances(K_last if K is None else K, H, W, [e.mesh_tensors for e in self.estimators], poses, depth=depth, occluders=occluders,
                            delta=delta, want=('mask_visib', 'owner', 'info'), glctx=self.estimators[0].refiner.ctx)
    return dict(owner=out['owner'], mask_visib=out['mask_visib'], visib_fract=np.array([r['visib_fract'] for r in out['info']], dtype=np.float64))

  def draw(self, rgb, fill_alpha=0.0, contour=False, depth=None, oriented=False, **kw):
    """The frame `rgb` (H,W,3) uint8, numpy or device tensor, with every object's box and xyz axes at its current pose of the ORIGINAL
    mesh - the poses the last `register` / `track` returned - in one Utils.draw_poses call; the result is of the kind of `rgb`.  The box
    of object o is Utils.model_box of its mesh (oriented=True: its minimum-volume box, FoundationPose.model_box(oriented=True), found once
    per object), in object o's palette colour.  fill_alpha > 0 tints each object's visible pixels,
    contour=True outlines them: the owner map then comes from instance_masks(depth=depth).  Other keywords go to Utils.draw_poses."""
    from . import Utils as U
    ests = self.estimators
    self._need_poses('draw', frame=True)
    returned = self._returned or [(None, None)] * len(ests)
    poses, boxes, offs = [], [], []
    for e, (held, pose) in zip(ests, returned):
      if held is not e.pose_last:                           # set elsewhere since: the pose of the original mesh as track_one forms it
        last = torch.as_tensor(e.pose_last, dtype=torch.float).reshape(4, 4)
        pose = (last.to(e.get_tf_to_centered_mesh().device) @ e.get_tf_to_centered_mesh()).cpu().numpy()
      to_origin, bbox = e.model_box(oriented=True) if oriented else U.model_box(e.mesh_ori)
      poses.append(pose), boxes.append(bbox), offs.append(np.linalg.inv(to_origin))
    owner = None
    if fill_alpha > 0 or contour:
      owner = self.instance_masks(depth=depth)['owner']
    K = kw.pop('K', self._last_frame[2])
    return U.draw_poses(rgb, K, np.stack(poses), bboxes=np.stack(boxes), offsets=np.stack(offs), owner=owner, fill_alpha=fill_alpha, contour=contour,
                        glctx=ests[0].refiner.ctx, **kw)
