"""Polishing object poses against the depth of the frame they are seen in (a build extension; the reference has no such stage): point-to-
plane ICP between the rendered model and the observed depth with projective association, linearised for all poses in one launch
(fp_pose_depth_align), stepped on the device (fp_pose_gn_step) and looped without the host (fp_pose_polish) - csrc/pose_icp.hip; the
rules are stated in include/foundationpose_amd.h.  Everything here is additive: no other call of the package changes what it returns.

Geometry only.  Symmetric objects and flat faces slide along their free directions (info['xi_last'] and the sums show it); projective
association needs a start within dist_max of the surface; several crop pixels can land on one observed pixel when the crop magnifies;
there is no occlusion reasoning beyond the two gates; the fit numbers (valid, rendered, observed, rms) are reported, not judged."""
import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .reconstruct import depth_normals

# This project's own choice, fixed by the experiment with the restatement on the CPU that DESIGN.md section 5 records (the last stage of
# reconstruct.DEFAULT_STAGES, 5 mm / 0.7, loses poses that start 4 mm off; 20 mm / 0.5 loses one that starts 10 mm off)
DEFAULT_DIST_MAX, DEFAULT_COS_MIN, DEFAULT_ITERATIONS, DEFAULT_DAMPING, DEFAULT_MIN_PIXELS = 0.010, 0.5, 8, 1e-9, 100
MAX_POSES = _lib.FP_POSE_ALIGN_MAX_POSES


def _dev_of(*xs, device='cuda'):
  for x in xs:
    if torch.is_tensor(x) and x.is_cuda:
      return x.device
  d = torch.device(device)
  return torch.device('cuda', d.index if d.index is not None else torch.cuda.current_device())


def new_pose_state(n, device):
  """n fresh fp_pose_state records as an (n,136) uint8 device tensor: all-zero bytes"""
  return torch.zeros((int(n), _lib.POSE_STATE_DTYPE.itemsize), dtype=torch.uint8, device=device)


def read_pose_state(state):
  """the records of a state tensor as a numpy record array (fields of _lib.POSE_STATE_DTYPE); synchronises"""
  return state.cpu().numpy().view(_lib.POSE_STATE_DTYPE).reshape(-1)


def align_poses_step(xyz, normal, depth, normals, poses, K, dist_max, cos_min, rows=False, on_device=False):
  """One linearisation of point-to-plane ICP of N posed models against one frame (fp_pose_depth_align).  xyz, normal (N,h,w,3): the
  camera-space maps of the model at the poses, as nvdiffrast_render writes them (extra['xyz_map'], normal_map), background 0; depth
  (H,W) and normals (H,W,4, of reconstruct.depth_normals) the observed frame; poses (N,4,4).  Returns (sums (N,29) float64 - per pose
  the upper triangle of J^T J, J^T r, sum r^2, the number of valid pixels -, counts (N,2) int32 - rendered and observed pixels -) and,
  with rows=True, the (N,h,w,8) float32 device tensor of the per-pixel rows.  sums and counts are numpy arrays and the call synchronises;
  with on_device=True they are device tensors and nothing synchronises.  More than MAX_POSES poses are cut into calls (a pose's numbers
  do not depend on the batch it is in)."""
  dev = _dev_of(xyz, normal, depth, normals, poses)
  xyz = torch.as_tensor(xyz, device=dev).to(torch.float).contiguous()
  normal = torch.as_tensor(normal, device=dev).to(torch.float).contiguous()
  if xyz.dim() != 4 or xyz.shape[-1] != 3 or xyz.shape != normal.shape:
    raise ValueError(f'xyz and normal must both be (N,h,w,3), got {tuple(xyz.shape)} and {tuple(normal.shape)}')
  N, h, w = xyz.shape[:3]
  depth = torch.as_tensor(depth, device=dev).to(torch.float).contiguous()
  H, W = depth.shape
  normals = torch.as_tensor(normals, device=dev).contiguous()
  if tuple(normals.shape) != (H, W, 4) or normals.dtype != torch.float:
    raise ValueError(f'normals must be float32 of shape {(H, W, 4)}, got {normals.dtype} {tuple(normals.shape)}')
  poses = torch.as_tensor(poses, device=dev).to(torch.float).reshape(-1, 4, 4).contiguous()
  if len(poses) != N:
    raise ValueError(f'{N} maps, {len(poses)} poses')
  Kd, Kp = _lib.k_ptr(K)
  ctx = _lib.Context.get(dev)
  sums = torch.zeros((N, _lib.FP_POSE_ALIGN_TERMS), dtype=torch.float64, device=dev)
  counts = torch.zeros((N, 2), dtype=torch.int32, device=dev)
  out = torch.empty((N, h, w, 8), dtype=torch.float, device=dev) if rows else None
  host = None if on_device else np.zeros((N, _lib.FP_POSE_ALIGN_TERMS), dtype=np.float64)
  for a in range(0, N, MAX_POSES):
    b = min(a + MAX_POSES, N)
    part = None if host is None else np.zeros((b - a, _lib.FP_POSE_ALIGN_TERMS), dtype=np.float64)
    check(lib().fp_pose_depth_align(ctx.handle, ptr(xyz[a:b]), ptr(normal[a:b]), b - a, h, w, ptr(depth), ptr(normals), H, W, Kp, ptr(poses[a:b]),
                                    float(dist_max), float(cos_min), None if out is None else ptr(out[a:b]), ptr(sums[a:b]), ptr(counts[a:b]),
                                    ptr(part), stream_ptr(dev)))
    if host is not None:
      host[a:b] = part
  res = (sums, counts) if on_device else (host, counts.cpu().numpy())
  return res + (out,) if rows else res


def pose_gn_step(sums, poses, state=None, damping=DEFAULT_DAMPING, min_pixels=DEFAULT_MIN_PIXELS, closing=False):
  """The Gauss-Newton step of every pose on the device (fp_pose_gn_step): sums (N,29) float64 of align_poses_step, poses (N,4,4) float32
  DEVICE tensor, contiguous, changed in place; state an (N,136) uint8 device tensor of new_pose_state (None: fresh records).  A pose with
  fewer than min_pixels valid pixels, or whose mean square residual rose, goes back to the pose before its last step and stops; otherwise,
  unless closing, it moves by the solution of (A + damping trace(A) I) xi = -b.  Returns the state tensor (read_pose_state shows it).
  Nothing synchronises."""
  if not (torch.is_tensor(poses) and poses.is_cuda and poses.dtype == torch.float and poses.is_contiguous()):
    raise ValueError('poses must be a contiguous float32 device tensor: it is changed in place')
  dev = poses.device
  N = poses.numel() // 16
  sums = torch.as_tensor(sums, device=dev).to(torch.float64).contiguous()
  if tuple(sums.shape) != (N, _lib.FP_POSE_ALIGN_TERMS):
    raise ValueError(f'sums must be {(N, _lib.FP_POSE_ALIGN_TERMS)}, got {tuple(sums.shape)}')
  if state is None:
    state = new_pose_state(N, dev)
  if tuple(state.shape) != (N, _lib.POSE_STATE_DTYPE.itemsize) or state.dtype != torch.uint8 or state.device != dev or not state.is_contiguous():
    raise ValueError(f'state must be a contiguous uint8 tensor of shape {(N, _lib.POSE_STATE_DTYPE.itemsize)} on {dev}')
  ctx = _lib.Context.get(dev)
  for a in range(0, N, MAX_POSES):
    b = min(a + MAX_POSES, N)
    check(lib().fp_pose_gn_step(ctx.handle, ptr(sums[a:b]), ptr(poses.reshape(-1, 16)[a:b]), ptr(state[a:b]), b - a, float(damping), int(min_pixels),
                                1 if closing else 0, stream_ptr(dev)))
  return state


def enqueue_polish(ctx, mesh_handle, poses, Kp, H, W, depth, normals, crop, crop_ratio, mesh_diameter, iterations, dist_max, cos_min, damping,
                   min_pixels, state, sums, counts):
  """fp_pose_polish on device tensors that are all in place (poses (N,4,4) float32 in and out); nothing synchronises"""
  dev = poses.device
  for a in range(0, len(poses), MAX_POSES):
    b = min(a + MAX_POSES, len(poses))
    check(lib().fp_pose_polish(ctx.handle, mesh_handle, ptr(poses[a:b]), b - a, Kp, int(H), int(W), ptr(depth), ptr(normals), int(crop),
                               float(crop_ratio), float(mesh_diameter), int(iterations), float(dist_max), float(cos_min), float(damping),
                               int(min_pixels), ptr(state[a:b]), ptr(sums[a:b]), ptr(counts[a:b]), stream_ptr(dev)))


def polish_info(state, counts):
  """info of polish_poses from the state and counts tensors; synchronises"""
  st = read_pose_state(state)
  c = counts.cpu().numpy()
  return dict(valid=st['fit_count'].astype(np.int64), rendered=c[:, 0].astype(np.int64), observed=c[:, 1].astype(np.int64),
              rms=np.sqrt(st['fit_ms']), stopped=[_lib.FP_POSE_STOP_REASONS.get(int(s)) for s in st['stopped']], xi_last=st['xi'].copy(),
              steps=st['steps'].astype(np.int64))


def polish_poses(poses, depth, K, mesh=None, mesh_tensors=None, mask=None, iterations=DEFAULT_ITERATIONS, dist_max=DEFAULT_DIST_MAX,
                 cos_min=DEFAULT_COS_MIN, crop=160, crop_ratio=1.2, max_jump=0.01, min_pixels=DEFAULT_MIN_PIXELS, damping=DEFAULT_DAMPING,
                 mesh_diameter=None, glctx=None):
  """Move object poses onto the measured depth by geometry alone (fp_pose_polish): `iterations` Gauss-Newton steps of point-to-plane ICP
  between the model rendered at each pose - through crop windows of `crop` x `crop` pixels around it, as the refiner's; crop=0 renders
  the full frame - and the observed depth, plus one closing evaluation, all on the device.

  poses (N,4,4) or (4,4): object-in-camera poses of `mesh` / `mesh_tensors` (make_mesh_tensors layout); depth (H,W) metres; numpy arrays
  or device tensors.  mask (H,W), non-zero = may be the object, enters the observed normals (fp_depth_normals, computed once per call,
  with max_jump) and nothing else.  mesh_diameter sizes the crop windows (None: Utils.mesh_diameter of the vertices).
  Returns (poses, info): poses as given (numpy in, numpy out; a fresh tensor otherwise); info per pose: valid (valid pixels) and rms
  (metres) of the returned pose's fit, rendered and observed (pixels the model covers, and of those the ones that found an observed
  normal, at the last evaluation), stopped (None, or 'too few valid pixels' / 'residual rose' / 'singular': such a pose is the one before
  its last step), xi_last (the last step taken, (translation, rotation vector) about the pose's origin), steps.  These are reported,
  not judged.  One synchronisation, at the end."""
  from . import Utils as U
  as_numpy = not torch.is_tensor(poses)
  dev = _dev_of(poses, depth)
  if mesh_tensors is None:
    if mesh is None:
      raise ValueError('polish_poses needs mesh or mesh_tensors')
    mesh_tensors = U.make_mesh_tensors(mesh, device=dev)
  ctx = U._ctx_of(glctx, dev)
  p = torch.as_tensor(poses, device=dev).to(torch.float).reshape(-1, 4, 4).contiguous().clone()
  N = len(p)
  depth = torch.as_tensor(depth, device=dev).to(torch.float).contiguous()
  H, W = depth.shape
  normals = depth_normals(depth, K, None if mask is None else torch.as_tensor(mask, device=dev)[None], max_jump=max_jump, device=dev)[0]
  if mesh_diameter is None:
    mesh_diameter = U.mesh_diameter(mesh_tensors=mesh_tensors) if crop else 1.0
  Kd, Kp = _lib.k_ptr(K)
  dm = _lib.device_mesh(ctx, mesh_tensors)
  state = new_pose_state(N, dev)
  sums = torch.zeros((N, _lib.FP_POSE_ALIGN_TERMS), dtype=torch.float64, device=dev)
  counts = torch.zeros((N, 2), dtype=torch.int32, device=dev)
  enqueue_polish(ctx, dm.handle, p, Kp, H, W, depth, normals, crop, crop_ratio, mesh_diameter, iterations, dist_max, cos_min, damping, min_pixels,
                 state, sums, counts)
  info = polish_info(state, counts)
  info['sums'] = sums.cpu().numpy()
  p = p.reshape(tuple(np.shape(poses)) if as_numpy else tuple(poses.shape))
  if as_numpy:
    kind = np.asarray(poses).dtype
    p = p.cpu().numpy().astype(kind if kind.kind == 'f' else np.float32)
  return p, info
