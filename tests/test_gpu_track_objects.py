"""GPU: track_one for several objects of one frame in one call (tracking.MultiObjectTracker, fp_track_objects).

One object equals FoundationPose.track_one bit for bit; K objects equal PoseRefinePredictor.predict_multi over the same objects bit for
bit (same network pass size) and separate track_one calls within the pose tolerance; one render and one observed-crop launch per
iteration; graph replay equals eager; poses hand over to and from the estimators; bad input is refused."""
import copy
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-3
H, W = 480, 640


def _estimator(mesh, refiner, scorer):
  from foundationpose_amd.estimater import FoundationPose
  np.random.seed(0)
  return FoundationPose(model_pts=mesh.vertices, model_normals=mesh.vertex_normals, mesh=mesh, refiner=refiner, scorer=scorer)


def _pose(t, rot_seed):
  from foundationpose_amd import synthetic as S
  p = np.eye(4, dtype=np.float32)
  p[:3, :3] = S.random_rotation(np.random.RandomState(rot_seed))
  p[:3, 3] = t
  return p


def _nudge(p, seed, dt=0.004, deg=2.0):
  """p moved by a few mm and degrees: a start pose the refiner has work to do from."""
  rs = np.random.RandomState(seed)
  w = rs.randn(3)
  w *= np.deg2rad(deg) / np.linalg.norm(w)
  th = np.linalg.norm(w)
  Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
  R = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx
  q = p.astype(np.float64).copy()
  q[:3, :3] = R @ q[:3, :3]
  q[:3, 3] += rs.randn(3) * dt
  return q.astype(np.float32)


def _frame(ests, poses, seed=0):
  """RGB-D frame z-composited from the HIP renders of every estimator's centred mesh at its pose, over a background plane at 1.2 m:
  (rgb uint8 (H,W,3), depth float32 (H,W)) on the device."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.Utils import nvdiffrast_render
  g = torch.Generator(device='cuda').manual_seed(seed)
  vs, us = torch.meshgrid(torch.arange(H, device='cuda'), torch.arange(W, device='cuda'), indexing='ij')
  rgb = torch.stack([0.5 + 0.3 * torch.sin(us * 0.07) * torch.cos(vs * 0.05), 0.45 + 0.3 * torch.sin(us * 0.031 + vs * 0.043),
                     0.4 + 0.25 * torch.cos(vs * 0.09 - us * 0.02)], -1)
  depth = torch.full((H, W), 1.2, device='cuda')
  for e, p in zip(ests, poses):
    c, d, _ = nvdiffrast_render(K=S.YCB_K, H=H, W=W, ob_in_cams=torch.as_tensor(p, device='cuda').reshape(1, 4, 4), mesh_tensors=e.mesh_tensors,
                                use_light=True)
    near = (d[0] > 0) & (d[0] < depth)
    depth = torch.where(near, d[0], depth)
    rgb = torch.where(near[..., None], c[0], rgb)
  rgb = (rgb * 255 + torch.randn(rgb.shape, device='cuda', generator=g) * 1.5).clamp(0, 255).to(torch.uint8)
  depth = depth + torch.randn(depth.shape, device='cuda', generator=g) * 0.001
  return rgb.contiguous(), depth.contiguous()


@pytest.fixture(scope='module')
def world():
  """One refiner (the low-gain chain refiner of the tracking fixtures) and estimators of three distinct meshes, a fourth instance of
  mesh 0 (the same mesh tensors: one fp_mesh) and one mesh beyond the one-launch render (8 642 vertices: its A records exceed 64 KiB)."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.config import REFINE_DEFAULT, SCORE_DEFAULT
  from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
  from foundationpose_amd.predict_score import ScorePredictor
  refiner = PoseRefinePredictor(state_dict=S.make_refine_state_dict(cases.REFINE_SEED, head_gain=cases.GAIN_CHAIN), cfg=REFINE_DEFAULT)
  scorer = ScorePredictor(state_dict=S.make_score_state_dict(cases.SCORE_SEED), cfg=SCORE_DEFAULT)
  meshes = [S.make_mustard_mesh(seed=0), S.make_mustard_mesh(seed=1, n_theta=80, n_z=70), S.make_mustard_mesh(seed=2, n_theta=64, n_z=60)]
  ests = [_estimator(m, refiner, scorer) for m in meshes]
  twin = _estimator(meshes[0], refiner, scorer)
  twin.mesh_tensors, twin.diameter = ests[0].mesh_tensors, ests[0].diameter       # a second instance of part 0
  big = _estimator(S.make_mustard_mesh(seed=3, n_theta=96, n_z=90), refiner, scorer)
  assert big.mesh_tensors['pos'].shape[0] * 8 > 64 * 1024
  gt = [_pose((-0.07, -0.04, 0.75), 1), _pose((0.07, -0.03, 0.80), 2), _pose((0.0, 0.07, 0.70), 3), _pose((0.09, 0.08, 0.85), 4)]
  refiner.ctx.reserve(64)
  return dict(refiner=refiner, scorer=scorer, ests=ests + [twin], big=big, gt=gt)


def _set_poses(ests, poses):
  for e, p in zip(ests, poses):
    e.pose_last = torch.as_tensor(p, device='cuda').reshape(4, 4).clone()


def _tf(e):
  tf = np.eye(4, dtype=np.float32)
  tf[:3, 3] = -np.asarray(e.model_center, dtype=np.float32)
  return tf


def test_one_object_equals_track_one_bit_for_bit(world):
  """MultiObjectTracker([est]) against a twin estimator's track_one, 5 chained frames of cases.tracking_frames, eager and graph: every
  frame's pose and pose-of-mesh identical."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  sc, frames = cases.tracking_frames(5)
  mesh = S.make_mustard_mesh(seed=0)
  a, b = _estimator(mesh, world['refiner'], world['scorer']), _estimator(mesh, world['refiner'], world['scorer'])
  tracker = MultiObjectTracker([a])
  start = _nudge(frames[0]['gt_pose'], 11)
  for graph in (False, True):
    tracker.enable_graph(graph)
    b.enable_track_graph(graph)
    _set_poses([a, b], [start, start])
    for fr in frames:
      got = tracker.track(fr['rgb'], fr['depth'], fr['K'], iteration=2)
      want = b.track_one(fr['rgb'], fr['depth'], fr['K'], iteration=2)
      assert got.shape == (1, 4, 4) and got.dtype == np.float32
      assert np.array_equal(got[0], want)
      assert torch.equal(a.pose_last, b.pose_last) and a.pose_last.shape == (1, 4, 4)
  tracker.enable_graph(False)
  b.enable_track_graph(False)
  assert not np.array_equal(start, a.pose_last.reshape(4, 4).cpu().numpy())        # (the frames did move the pose)


def _predict_multi_reference(refiner, ests, starts, rgb, depth, K, iteration):
  """PoseRefinePredictor.predict_multi over the same objects, fed the prelude of fp_track_frame: depth_prefilter with the float32 K
  (zfar 100 / inf, as the frame), float colours."""
  import foundationpose_amd.Utils as U
  d, xyz, rgb_f = U.depth_prefilter(depth, np.asarray(K, dtype=np.float32), rgb_u8=rgb)
  objs = [dict(rgb=rgb_f, xyz_map=xyz, K=K, mesh_tensors=e.mesh_tensors, mesh_diameter=e.diameter, ob_in_cams=torch.as_tensor(p).reshape(1, 4, 4))
          for e, p in zip(ests, starts)]
  return refiner.predict_multi(objs, iteration=iteration).cpu().numpy()


def _check_against_predict_multi(world, ests, iteration=2):
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  rgb, depth = _frame(ests, world['gt'][:len(ests)])
  starts = [_nudge(p, 20 + o) for o, p in enumerate(world['gt'][:len(ests)])]
  _set_poses(ests, starts)
  ctx = world['refiner'].ctx
  ctx.prof_reset()
  ctx.prof_enable(2)
  got = MultiObjectTracker(ests).track(rgb, depth, S.YCB_K, iteration=iteration)
  torch.cuda.synchronize()
  ctx.prof_enable(False)
  counts = {c: ctx.prof_read(c)['launches'] for c in ('render', 'crop')}
  ctx.prof_reset()
  want = _predict_multi_reference(world['refiner'], ests, starts, rgb, depth, S.YCB_K, iteration)
  for o, e in enumerate(ests):
    pose = e.pose_last.reshape(4, 4).cpu().numpy()
    assert np.array_equal(pose, want[o]), f'object {o}: max diff {np.abs(pose - want[o]).max():.2e}'
    assert np.abs(got[o] - pose @ _tf(e)).max() <= 1e-6
    assert np.abs(pose - starts[o]).max() > 1e-5                 # (refined)
  return counts


def test_objects_equal_predict_multi_bit_for_bit(world):
  """Three distinct meshes and a second instance of mesh 0 at another pose, one frame at iteration=2: each refined pose equals
  predict_multi's for that object; pose-of-mesh = pose @ get_tf_to_centered_mesh()."""
  _check_against_predict_multi(world, world['ests'])


def test_one_launch_per_stage(world):
  """Eager, profiled: a 4-object frame has the render and crop launch counts of a 1-object frame (`iteration` each).  An object whose mesh
  the one-launch render cannot take is rendered by the plain form - one more render launch per iteration - with predict_multi's poses."""
  it = 2
  one = _check_against_predict_multi(world, world['ests'][:1], it)
  four = _check_against_predict_multi(world, world['ests'], it)
  print(f'launches per frame: 1 object {one}, 4 objects {four}')
  assert one == four == {'render': it, 'crop': it}
  mixed = world['ests'][:2] + [world['big']] + world['ests'][3:]
  counts = _check_against_predict_multi(world, mixed, it)
  print(f'with a mesh beyond the one-launch render: {counts}')
  assert counts == {'render': 2 * it, 'crop': it}


def test_close_to_separate_track_one(world):
  """10 frames, 4 objects moving along their own trajectories; every frame starts both sides from the same poses (the trajectory's
  previous ones).  Each object's pose within the 1e-3 tolerance of its own track_one."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  ests = world['ests']
  trajs = [S.trajectory(10, seed=o, t0=tuple(world['gt'][o][:3, 3])) for o in range(4)]
  tracker = MultiObjectTracker(ests)
  worst = 0.0
  for f in range(1, 10):
    rgb, depth = _frame(ests, [t[f] for t in trajs], seed=f)
    starts = [t[f - 1] for t in trajs]
    _set_poses(ests, starts)
    got = tracker.track(rgb, depth, S.YCB_K, iteration=2)
    for o, e in enumerate(ests):
      e.pose_last = torch.as_tensor(starts[o], device='cuda').reshape(4, 4).clone()
      want = e.track_one(rgb, depth, S.YCB_K, iteration=2)
      worst = max(worst, float(np.abs(got[o] - want).max()))
  print(f'max |pose(MultiObjectTracker) - pose(track_one)| over 9 frames x 4 objects: {worst:.2e}')
  assert worst < POSE_TOL


def test_graph_replay_equals_eager_and_recaptures(world):
  """Several 4-object frames as one hipGraph each equal the eager frames bit for bit, including frames after ctx.reserve has moved the
  library's arena (the graph is captured again)."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  ests, ctx = world['ests'], world['refiner'].ctx
  frames = [_frame(ests, [_nudge(p, 40 + 4 * f + o, 0.002, 1.0) for o, p in enumerate(world['gt'])], seed=f) for f in range(4)]
  starts = [_nudge(p, 30 + o) for o, p in enumerate(world['gt'])]
  tracker = MultiObjectTracker(ests)
  runs = []
  for graph in (False, True):
    tracker.enable_graph(graph)
    _set_poses(ests, starts)
    out = []
    for f, (rgb, depth) in enumerate(frames):
      if graph and f == 2:
        g0, n = ctx.arena_generation(), 128
        while ctx.arena_generation() == g0 and n <= 4096:
          ctx.reserve(n)
          n *= 2
        assert ctx.arena_generation() != g0
      out.append(tracker.track(rgb, depth, S.YCB_K, iteration=2))
    runs.append(out)
  tracker.enable_graph(False)
  for a, b in zip(*runs):
    assert np.array_equal(a, b)
  assert not np.array_equal(runs[0][0], runs[0][1])


def test_hand_off_between_tracker_and_estimators(world):
  """Between tracker frames one estimator is re-registered and another steps with track_one: the next tracker frame starts from their
  poses (it equals a frame started from copies of them).  A track_one after a tracker frame continues from the tracker's pose."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  ests = world['ests'][:3]
  rgb, depth = _frame(ests, world['gt'][:3])
  tracker = MultiObjectTracker(ests)
  _set_poses(ests, [_nudge(p, 50 + o) for o, p in enumerate(world['gt'][:3])])
  tracker.track(rgb, depth, S.YCB_K, iteration=2)
  # a track_one right after continues from the tracker's pose
  p1 = ests[1].pose_last.clone()
  twin = copy.copy(ests[1])
  twin._track_ws = {}
  twin.pose_last = p1.clone()
  stepped = ests[1].track_one(rgb, depth, S.YCB_K, iteration=2)
  assert np.array_equal(stepped, twin.track_one(rgb, depth, S.YCB_K, iteration=2))
  # object 0 re-registered (its mask from the composite: the pixels nearer than the background of its own render)
  from foundationpose_amd.Utils import nvdiffrast_render
  _, d0, _ = nvdiffrast_render(K=S.YCB_K, H=H, W=W, ob_in_cams=torch.as_tensor(world['gt'][0], device='cuda').reshape(1, 4, 4),
                               mesh_tensors=ests[0].mesh_tensors)
  mask = ((d0[0] > 0) & ((d0[0] - depth).abs() < 0.01)).cpu().numpy()
  ests[0].register(K=S.YCB_K, rgb=rgb.cpu().numpy(), depth=depth.cpu().numpy(), ob_mask=mask, iteration=1)
  handed = [e.pose_last.reshape(4, 4).clone() for e in ests]
  got = tracker.track(rgb, depth, S.YCB_K, iteration=2)
  for e, p in zip(ests, handed):
    e.pose_last = p.clone()
  again = tracker.track(rgb, depth, S.YCB_K, iteration=2)
  assert np.array_equal(got, again)


def test_refusals(world):
  from foundationpose_amd import _lib
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  ests = world['ests']
  with pytest.raises(ValueError, match='1 .. 8'):
    MultiObjectTracker([])
  with pytest.raises(ValueError, match='1 .. 8'):
    MultiObjectTracker([ests[0]] * 9)
  other = copy.copy(ests[1])
  other.refiner = types.SimpleNamespace(ctx=ests[0].refiner.ctx, model=types.SimpleNamespace(handle=ctypes.c_void_p(1)))
  with pytest.raises(ValueError, match='refiner'):
    MultiObjectTracker([ests[0], other])
  other.refiner = types.SimpleNamespace(ctx=types.SimpleNamespace(), model=ests[0].refiner.model)       # same network, another context
  with pytest.raises(ValueError, match='refiner'):
    MultiObjectTracker([ests[0], other])
  with pytest.raises(ValueError, match='listed twice'):
    MultiObjectTracker([ests[0], ests[1], ests[0]])
  sharded = copy.copy(ests[1])
  sharded.dist_group = object()
  with pytest.raises(ValueError, match='dist_group'):
    MultiObjectTracker([ests[0], sharded])
  fresh = copy.copy(ests[1])
  fresh.pose_last = None
  rgb, depth = _frame(ests[:1], world['gt'][:1])
  _set_poses(ests[:1], world['gt'][:1])
  with pytest.raises(ValueError, match='pose_last is None'):
    MultiObjectTracker([ests[0], fresh]).track(rgb, depth, S.YCB_K, iteration=2)
  # the C-ABI, on an otherwise valid frame
  tracker = MultiObjectTracker(ests[:2])
  _set_poses(ests[:2], world['gt'][:2])
  tracker.track(rgb, depth, S.YCB_K, iteration=1)
  ws = next(iter(tracker._ws.values()))
  ctx = world['refiner'].ctx

  def call(**changes):
    a = _lib.FpTrackObjectsArgs.from_buffer_copy(ws['args'])
    objs = (_lib.FpTrackObject * 9)(*[ws['objs'][o % 2] for o in range(9)])
    a.objs = ctypes.addressof(objs)
    for k, v in changes.items():
      if k == 'null_mesh':
        objs[1].mesh = None
      else:
        setattr(a, k, v)
    _lib.check(_lib.lib().fp_track_objects(ctx.handle, ctypes.byref(a), _lib.stream_ptr()))
  call()
  torch.cuda.synchronize()
  for changes, msg in ((dict(struct_size=ctypes.sizeof(_lib.FpTrackObjectsArgs) - 8), 'struct_size'), (dict(n_obj=0), 'n_obj = 0'),
                       (dict(n_obj=9), 'n_obj = 9'), (dict(null_mesh=True), 'object 1 has a null field')):
    with pytest.raises(_lib.FoundationPoseAmdError, match=msg):
      call(**changes)
