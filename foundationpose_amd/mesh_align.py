"""Rigid alignment of a mesh or a point cloud to a model (a build extension; the reference has no such step): ICP against the EXACT nearest
triangle of the target, linearised for N poses in one call (fp_points_mesh_align), stepped on the device (fp_pose_gn_step) and looped
without the host (fp_points_mesh_polish) - csrc/surface_distance.hip; the rules are stated in include/foundationpose_amd.h and restated
in tests/mesh_align_oracle.py.  Everything here is additive: no other call of the package changes what it returns.

Limits.  Rigid only, no scale.  Align the PARTIAL surface to the COMPLETE one, not the reverse: every source point looks for a partner on
the target.  A symmetric target makes several starts equally good: they are listed in info['ambiguous'], not judged.  init='axes' rests on
the principal axes of both surfaces: nearly equal covariance eigenvalues make them arbitrary, and the 24 rotations of the cube cover
permutations and signs of the axes but not an arbitrary in-plane angle.  The search is brute force, N n F pair tests per iteration."""
import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .pose_icp import new_pose_state, read_pose_state

# This project's own choice, as fractions of the target's exact diameter: (mode, dist_max / diameter, iterations).
# Point to point first - it has no flat directions, so a start 90 degrees off still turns -, then point to plane at a closing gate.
DEFAULT_STAGE_FRACTIONS = (('point', 0.5, 10), ('plane', 0.1, 20), ('plane', 0.02, 10))
DEFAULT_DAMPING, DEFAULT_MIN_POINTS, DEFAULT_AMBIGUITY, AMBIGUITY_ANGLE_DEG = 1e-9, 100, 1.5, 5.0
MAX_POSES = _lib.FP_POSE_ALIGN_MAX_POSES
_SIGNED_AXES = ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0), (2, 1.0), (2, -1.0))      # +x, -x, +y, -y, +z, -z


def cube_rotations():
  """The 24 proper rotations of the cube, (24,3,3) float64, in a fixed order: the image a of the x axis runs over +x, -x, +y, -y, +z,
  -z; for each, the image b of the y axis over the four signed axes perpendicular to a in that same order; z goes to a x b.  The columns
  of a matrix are (a, b, a x b); index 0 is the identity."""
  out = []
  for ia, sa in _SIGNED_AXES:
    for ib, sb in _SIGNED_AXES:
      if ib != ia:
        a, b = np.zeros(3), np.zeros(3)
        a[ia], b[ib] = sa, sb
        out.append(np.stack([a, b, np.cross(a, b)], 1))
  return np.stack(out)


def axes_starts(centroid_s, axes_s, centroid_t, axes_t):
  """The 24 starts of init='axes', (24,4,4) float64 `target from source`: R = U_t g U_s^T about the two centroids, t = c_t - R c_s, with
  U the principal axes as columns (symmetry.principal_axes returns them as rows, right-handed) and g over cube_rotations()."""
  out = np.tile(np.eye(4), (24, 1, 1))
  for k, g in enumerate(cube_rotations()):
    R = np.asarray(axes_t).T @ g @ np.asarray(axes_s)
    out[k, :3, :3], out[k, :3, 3] = R, np.asarray(centroid_t) - R @ np.asarray(centroid_s)
  return out


def _stage_array(stages):
  st = np.zeros(len(stages), dtype=_lib.MESH_ALIGN_STAGE_DTYPE)
  if not 1 <= len(stages) <= _lib.FP_MESH_ALIGN_MAX_STAGES:
    raise ValueError(f'{len(stages)} stages (1 .. {_lib.FP_MESH_ALIGN_MAX_STAGES})')
  for k, (mode, dist_max, iterations) in enumerate(stages):
    if mode not in _lib.FP_MESH_ALIGN_MODES:
      raise ValueError(f"stage {k}: mode {mode!r} ('plane' or 'point')")
    st[k] = (_lib.FP_MESH_ALIGN_MODES[mode], dist_max, iterations)
  return st


def align_step_on(pts, poses, pos, fc, mode, dist_max, keys=None, debug=False, h_sums=False):
  """fp_points_mesh_align on device tensors: pts (n,3), poses (N,4,4) float32 contiguous, pos (V,3), fc (F,3) int32.  Returns (sums
  (N,29) float64 - a device tensor, or with h_sums a numpy array and the call synchronises -, the dict of per-query outputs or None)."""
  dev, n, N = pos.device, len(pts), len(poses)
  if mode not in _lib.FP_MESH_ALIGN_MODES:
    raise ValueError(f"mode {mode!r} ('plane' or 'point')")
  R = 3 if mode == 'point' else 1
  if N > MAX_POSES or N * n > _lib.FP_SURFDIST_MAX_POINTS:
    raise ValueError(f'{N} poses of {n} points (at most {MAX_POSES} poses and {_lib.FP_SURFDIST_MAX_POINTS} queries a call)')
  if keys is None:
    keys = torch.empty(max(N * n, 1), dtype=torch.int64, device=dev)
  sums = torch.zeros((N, _lib.FP_POSE_ALIGN_TERMS), dtype=torch.float64, device=dev)
  host = np.zeros((N, _lib.FP_POSE_ALIGN_TERMS), dtype=np.float64) if h_sums else None
  d = None
  if debug:
    d = dict(q=torch.empty((N, n, 3), device=dev), dist=torch.empty((N, n), device=dev), face=torch.empty((N, n), dtype=torch.int32, device=dev),
             closest=torch.empty((N, n, 3), device=dev), normal=torch.empty((N, n, 3), device=dev), rows=torch.empty((N, n, R, 8), device=dev))
  o = (lambda k: ptr(d[k]) if d is not None and N * n else None)
  check(lib().fp_points_mesh_align(_lib.Context.get(dev).handle, ptr(pts) if n else None, n, ptr(poses), N, ptr(pos), len(pos), ptr(fc), len(fc),
                                   _lib.FP_MESH_ALIGN_MODES[mode], float(dist_max), ptr(keys), o('q'), o('dist'), o('face'), o('closest'), o('normal'),
                                   o('rows'), ptr(sums), ptr(host), stream_ptr(dev)))
  return (host if h_sums else sums), d


def align_points_step(points, poses, mesh=None, vertices=None, faces=None, mode='plane', dist_max=float('inf'), return_debug=False):
  """One Gauss-Newton linearisation of ICP between a point set under N poses and a mesh (fp_points_mesh_align): points (n,3) in the
  source's frame, poses (N,4,4) or (4,4) `target from source`, the target as `mesh` or vertices and faces.  Every point is matched to the
  exact nearest triangle (point_mesh_distance's rule); a pair farther apart than dist_max is left out.  mode 'plane': r = n . (y - c) with
  n the FACE normal; 'point': r = y - c, three rows.  Returns sums (N,29) float64 numpy - per pose the upper triangle of J^T J, J^T r,
  sum r^2 and the number of valid points, what pose_gn_step takes - and with return_debug also a dict of device tensors: q (N,n,3) the
  moved points, dist, face, closest, normal (zeros for a degenerate face) and rows (N,n,R,8).  Synchronises."""
  from . import Utils as U
  v = U._mesh_parts(mesh)[0] if mesh is not None else vertices
  dev = U._device_of(v)
  pos, fc = U._surface_on(mesh, vertices, faces, dev, 'align_points_step')
  pts = torch.as_tensor(points).to(device=dev, dtype=torch.float).reshape(-1, 3).contiguous()
  p = torch.as_tensor(poses).to(device=dev, dtype=torch.float).reshape(-1, 4, 4).contiguous()
  sums, d = align_step_on(pts, p, pos, fc, mode, dist_max, debug=return_debug, h_sums=True)
  return (sums, d) if return_debug else sums


def enqueue_polish(pts, poses, pos, fc, stages, damping, min_points, state, sums, keys):
  """fp_points_mesh_polish on device tensors that are all in place (poses (N,4,4) float32 in and out; stages the record array of
  _stage_array); nothing synchronises"""
  dev, n, N = pos.device, len(pts), len(poses)
  check(lib().fp_points_mesh_polish(_lib.Context.get(dev).handle, ptr(pts) if n else None, n, ptr(poses), N, ptr(pos), len(pos), ptr(fc), len(fc),
                                    stages.ctypes.data, len(stages), float(damping), int(min_points), ptr(state), ptr(sums), ptr(keys),
                                    stream_ptr(dev)))


def polish_on(pts, poses, pos, fc, stages, damping=DEFAULT_DAMPING, min_points=DEFAULT_MIN_POINTS):
  """The loop on device tensors, any number of poses (cut into calls of what fp_points_mesh_polish takes: a pose's numbers do not depend
  on its batch).  stages: [(mode, dist_max, iterations)].  Returns (poses (N,4,4) float32, a fresh tensor; state (N,136) uint8; sums)."""
  dev, n = pos.device, len(pts)
  p = poses.to(torch.float).reshape(-1, 4, 4).contiguous().clone()
  N = len(p)
  st = _stage_array(stages)
  state = new_pose_state(N, dev)
  sums = torch.zeros((N, _lib.FP_POSE_ALIGN_TERMS), dtype=torch.float64, device=dev)
  per_call = max(1, min(MAX_POSES, _lib.FP_SURFDIST_MAX_POINTS // max(n, 1)))
  keys = torch.empty(max(min(per_call, N) * n, 1), dtype=torch.int64, device=dev)
  for a in range(0, N, per_call):
    b = min(a + per_call, N)
    enqueue_polish(pts, p[a:b], pos, fc, st, damping, min_points, state[a:b], sums[a:b], keys)
  return p, state, sums


def _rotation_angle_deg(Ra, Rb):
  return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0))))


def align_to_mesh(source, target, init='axes', n_samples=4096, seed=0, stages=None, damping=DEFAULT_DAMPING, min_points=DEFAULT_MIN_POINTS,
                  ambiguity=DEFAULT_AMBIGUITY, return_info=True):
  """The rigid transform that lays `source` onto the mesh `target`: T (4,4) float64, `target from source`, and info.

  source: a mesh (an object with .vertices / .faces or a (vertices, faces) tuple), of which n_samples surface samples are taken
  (sample_surface, a function of the mesh, n_samples and seed), or an (n,3) point array, used as it is - a back-projected masked depth map
  will do.  target: a mesh.  init: (N,4,4) or (4,4) starts, or 'axes': the 24 starts U_t g U_s^T about the two centroids, with U the
  principal axes of the two surfaces (symmetry.surface_moments / principal_axes; of a point array: its mean and covariance) and g the 24
  proper rotations of the cube in cube_rotations()' order.  All starts run as ONE batch through fp_points_mesh_polish.
  stages: [(mode, dist_max, iterations)], mode 'point' or 'plane'; None is DEFAULT_STAGE_FRACTIONS times the target's exact
  mesh_diameter - this project's own choice.  Every stage starts the poses' records afresh; after the last, one closing evaluation.

  The winner is the start with the lowest mean squared distance over ALL source points, ungated (fp_symmetry_residuals on the final
  poses); ties go to the lowest index.  info: per start 'rms' and 'max' (that measure, metres), 'stopped' (None, 'too few valid pixels'
  - points, here -, 'residual rose', 'singular'), 'steps', 'valid' (of the last stage); 'poses' (N,4,4) float64, all final poses;
  'chosen'; 'ambiguous': the starts whose rms is within `ambiguity` times the winner's and whose rotation differs from the winner's by
  more than 5 degrees - reported, not judged: a symmetric target makes several starts equally good.  Synchronises (cold path)."""
  from . import Utils as U, symmetry as S
  tv = U._mesh_parts(target)[0]
  dev = U._device_of(tv)
  pos, fc = U._surface_on(target, None, None, dev, 'align_to_mesh')
  is_points = not isinstance(source, (tuple, list)) and not hasattr(source, 'faces')
  if is_points:
    pts = torch.as_tensor(source).to(device=dev, dtype=torch.float).reshape(-1, 3).contiguous()
  else:
    spos, sfc = U._surface_on(source, None, None, dev, 'align_to_mesh')
    pts = U._sample_surface_on(spos, sfc, int(n_samples), seed)[0]
  if len(pts) < 1:
    raise ValueError('align_to_mesh: no source points')
  if isinstance(init, str):
    if init != 'axes':
      raise ValueError(f"init {init!r}: 'axes', a (4,4) or an (N,4,4) array")
    if is_points:
      p64 = pts.cpu().numpy().astype(np.float64)
      c_s = p64.mean(0)
      cov_s = (p64 - c_s).T @ (p64 - c_s) / len(p64)
    else:
      _, c_s, cov_s = S.surface_moments(spos.cpu().numpy(), sfc.cpu().numpy())
    _, c_t, cov_t = S.surface_moments(pos.cpu().numpy(), fc.cpu().numpy())
    starts = axes_starts(c_s, S.principal_axes(cov_s)[1], c_t, S.principal_axes(cov_t)[1])
  else:
    starts = np.asarray(init.cpu() if torch.is_tensor(init) else init, dtype=np.float64).reshape(-1, 4, 4)
  if stages is None:
    d = U.mesh_diameter(model_pts=pos)
    stages = [(m, f * d, it) for m, f, it in DEFAULT_STAGE_FRACTIONS]
  p0 = torch.as_tensor(starts.astype(np.float32), device=dev)
  poses, state, _ = polish_on(pts, p0, pos, fc, stages, damping, min_points)
  per_call = max(1, _lib.FP_SURFDIST_MAX_POINTS // len(pts))
  stats = torch.cat([U._symmetry_residuals_on(pts, poses[a:a + per_call, :3, :].contiguous(), pos, fc)[0] for a in range(0, len(poses), per_call)])
  sd = U._stats_dict(stats.cpu().numpy())
  st = read_pose_state(state)
  final = poses.cpu().numpy().astype(np.float64)
  bad = (sd['not_finite'] > 0) | (sd['n'] == 0)
  rms = np.where(bad, np.inf, sd['rms'])
  chosen = int(np.argmin(rms))                                     # the first of equal minima: the lowest index
  ambiguous = [k for k in range(len(final)) if k != chosen and rms[k] <= ambiguity * rms[chosen]
               and _rotation_angle_deg(final[chosen, :3, :3], final[k, :3, :3]) > AMBIGUITY_ANGLE_DEG]
  info = dict(rms=rms, max=np.where(bad, np.inf, sd['max']), stopped=[_lib.FP_POSE_STOP_REASONS.get(int(s)) for s in st['stopped']],
              steps=st['steps'].astype(np.int64), valid=st['fit_count'].astype(np.int64), poses=final, starts=starts, chosen=chosen,
              ambiguous=ambiguous, stages=list(stages), n_points=len(pts))
  return (final[chosen], info) if return_info else final[chosen]


def transform_mesh(mesh, T):
  """A copy of `mesh` (an object with .vertices / .faces, e.g. synthetic.SimpleMesh or a trimesh.Trimesh, or a (vertices, faces[, normals[,
  colors]]) tuple) under the rigid transform T (4,4): positions R v + t, normals R n; faces, texture coordinates and colours are kept."""
  import copy
  T = np.asarray(T.cpu() if torch.is_tensor(T) else T, dtype=np.float64).reshape(4, 4)
  R, t = T[:3, :3], T[:3, 3]
  move = lambda v: (np.asarray(v, dtype=np.float64) @ R.T + t).astype(np.asarray(v).dtype if np.asarray(v).dtype.kind == 'f' else np.float64)
  turn = lambda n: (np.asarray(n, dtype=np.float64) @ R.T).astype(np.asarray(n).dtype if np.asarray(n).dtype.kind == 'f' else np.float64)
  if isinstance(mesh, (tuple, list)):
    parts = list(mesh)
    parts[0] = move(parts[0])
    if len(parts) > 2 and parts[2] is not None:
      parts[2] = turn(parts[2])
    return tuple(parts)
  out = copy.deepcopy(mesh)
  normals = getattr(mesh, '_vn', None) if hasattr(mesh, '_vn') else None
  out.vertices = move(mesh.vertices)
  if hasattr(mesh, '_vn'):
    if normals is not None:
      out._vn = turn(normals)
  elif getattr(mesh, 'vertex_normals', None) is not None:
    try:
      out.vertex_normals = turn(mesh.vertex_normals)
    except AttributeError:
      pass
  return out
