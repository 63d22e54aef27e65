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


class MultiObjectTracker:
  """track_one for several objects of ONE camera stream in one call per frame (fp_track_objects, a build extension): the frame is uploaded
  once, its depth prelude runs once, and every refinement iteration is one render, one observed-crop and one network pass over all the
  objects' images instead of one of each per object.

      tracker = MultiObjectTracker([est_a, est_b, est_c])      # registered FoundationPose instances sharing one PoseRefinePredictor
      poses = tracker.track(rgb, depth, K, iteration=2)        # np (n_obj, 4, 4) float32: row o = what est_o.track_one would return
      tracker.enable_graph(True)                               # one hipGraph per (objects, frame size, camera, iteration)

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
    return out
