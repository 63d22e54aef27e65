"""GPU: how a frame reaches the device and how a frame's call is captured, through the three callers that share foundationpose_amd/frame.py
(FoundationPose.track_one / track_multi, MultiObjectTracker.track, MultiObjectTracker.register).

Every upload route - numpy arrays, CPU tensors, separate device tensors, device tensors carved from one packed [depth | rgb] buffer, a
non-contiguous device view - must leave the same bytes in the frame buffer and give the same poses bit for bit; a frame replayed as a
hipGraph must equal the eager frame, also after the library's arena has moved and after the graph was switched off and on.  The frame
is 121 x 161: an odd pixel count, so the colours of a uint8 frame end, and the masks of a registration start, at odd byte offsets."""
import numpy as np
import pytest
import torch

from tests import cases
from tests.test_gpu_track_objects import _estimator, _nudge, _pose

pytestmark = pytest.mark.gpu
H, W = 121, 161
ROUTES = ['numpy', 'cpu tensors', 'two device tensors', 'packed device buffer', 'non-contiguous device rgb']


def _fb(ws):
  """The frame buffer of a workspace: its views `depth / rgb / labels / masks`."""
  return ws['fb']


def _camera():
  """The YCB intrinsics scaled from 480 x 640 to this frame."""
  from foundationpose_amd import synthetic as S
  return np.diag([W / 640.0, H / 480.0, 1.0]) @ np.asarray(S.YCB_K, dtype=np.float64)


def _frame(ests, poses, K, seed=0):
  """RGB-D frame z-composited from the HIP renders of every estimator's centred mesh at its pose, over a background plane at 1.2 m: device
  tensors (rgb uint8 (H,W,3), depth float32 (H,W), owner int32 (H,W): the object visible at a pixel, -1 = background)."""
  from foundationpose_amd.Utils import nvdiffrast_render
  g = torch.Generator(device='cuda').manual_seed(seed)
  vs, us = torch.meshgrid(torch.arange(H, device='cuda'), torch.arange(W, device='cuda'), indexing='ij')
  rgb = torch.stack([0.5 + 0.3 * torch.sin(us * 0.28) * torch.cos(vs * 0.2), 0.45 + 0.3 * torch.sin(us * 0.12 + vs * 0.17),
                     0.4 + 0.25 * torch.cos(vs * 0.36 - us * 0.08)], -1)
  depth = torch.full((H, W), 1.2, device='cuda')
  owner = torch.full((H, W), -1, device='cuda', dtype=torch.int32)
  for o, (e, p) in enumerate(zip(ests, poses)):
    c, d, _ = nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=torch.as_tensor(p, device='cuda').reshape(1, 4, 4), mesh_tensors=e.mesh_tensors, use_light=True)
    near = (d[0] > 0) & (d[0] < depth)
    depth = torch.where(near, d[0], depth)
    rgb = torch.where(near[..., None], c[0], rgb)
    owner = torch.where(near, torch.full_like(owner, o), owner)
  rgb = (rgb * 255 + torch.randn(rgb.shape, device='cuda', generator=g) * 1.5).clamp(0, 255).to(torch.uint8)
  depth = depth + torch.randn(depth.shape, device='cuda', generator=g) * 0.001
  return rgb.contiguous(), depth.contiguous(), owner


@pytest.fixture(scope='module')
def world():
  """The refiner, scorer and mustard meshes of the tracking fixtures; two objects; three frames along small motions; the start poses."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.config import REFINE_DEFAULT, SCORE_DEFAULT
  from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
  from foundationpose_amd.predict_score import ScorePredictor
  refiner = PoseRefinePredictor(state_dict=S.make_refine_state_dict(cases.REFINE_SEED, head_gain=cases.GAIN_CHAIN), cfg=REFINE_DEFAULT)
  scorer = ScorePredictor(state_dict=S.make_score_state_dict(cases.SCORE_SEED), cfg=SCORE_DEFAULT)
  ests = [_estimator(S.make_mustard_mesh(seed=0), refiner, scorer), _estimator(S.make_mustard_mesh(seed=1, n_theta=80, n_z=70), refiner, scorer)]
  K = _camera()
  gt = [_pose((-0.05, -0.02, 0.75), 1), _pose((0.06, 0.02, 0.80), 2)]
  frames = [_frame(ests, [_nudge(p, 40 + 2 * f + o, 0.002, 1.0) for o, p in enumerate(gt)], K, seed=f) for f in range(3)]
  assert all((fr[2] == o).sum() > 200 for fr in frames for o in range(2))       # both objects are in every frame
  starts = [torch.as_tensor(_nudge(p, 30 + o), device='cuda') for o, p in enumerate(gt)]
  return dict(refiner=refiner, scorer=scorer, ests=ests, K=K, frames=frames, starts=starts)


def _routes(rgb, depth):
  """The frame (device tensors) as every kind of input the callers take: (name, rgb, depth), in the order of ROUTES."""
  from foundationpose_amd.frame import is_packed
  n_d, n_c = depth.numel() * 4, rgb.numel() * rgb.element_size()
  buf = torch.empty((n_d + n_c,), dtype=torch.uint8, device='cuda')             # [depth | rgb], as bench.py packs its resident frames
  buf[:n_d] = depth.reshape(-1).view(torch.uint8)
  buf[n_d:] = rgb.reshape(-1).view(torch.uint8)
  p_depth, p_rgb = buf[:n_d].view(torch.float).reshape(H, W), buf[n_d:].view(rgb.dtype).reshape(H, W, 3)
  wide = torch.zeros((H, W, 6), dtype=rgb.dtype, device='cuda')
  wide[..., :3] = rgb
  out = [(rgb.cpu().numpy(), depth.cpu().numpy()), (rgb.cpu(), depth.cpu()), (rgb.clone(), depth.clone()), (p_rgb, p_depth), (wide[..., :3], depth.clone())]
  assert [is_packed(d, r) for r, d in out[2:]] == [False, True, False] and not out[4][0].is_contiguous()
  return [(name, r, d) for name, (r, d) in zip(ROUTES, out)]


def _bits(t):
  return t.contiguous().view(torch.uint8).reshape(-1)


@pytest.mark.parametrize('rgb_dtype', [torch.uint8, torch.float], ids=['u8', 'f32'])
def test_track_one_upload_routes(world, rgb_dtype):
  """After every route the workspace's depth and rgb views hold the input bit for bit, and the returned pose is that of the numpy route."""
  est, K = world['ests'][0].instance(), world['K']
  rgb, depth = world['frames'][0][0].to(rgb_dtype), world['frames'][0][1]
  want = None
  for name, r, d in _routes(rgb, depth):
    est.pose_last = world['starts'][0].clone()
    got = est.track_one(r, d, K, iteration=1)
    fb = _fb(est._track_workspace(1, None, 1, (H, W), rgb_dtype == torch.uint8, K))
    assert fb.depth.dtype == torch.float and fb.rgb.dtype == rgb_dtype and fb.rgb.shape == (H, W, 3)
    assert torch.equal(_bits(fb.depth), _bits(depth)) and torch.equal(_bits(fb.rgb), _bits(rgb)), name
    want = got if want is None else want
    assert got.shape == (4, 4) and got.dtype == np.float32 and np.array_equal(got, want), name
  assert len(est._track_ws) == 1                                  # one workspace served every route
  assert not np.array_equal(want[:3, :3], world['starts'][0][:3, :3].cpu().numpy())          # (the frame did move the pose)


@pytest.mark.parametrize('rgb_dtype', [torch.uint8, torch.float], ids=['u8', 'f32'])
def test_tracker_upload_routes(world, rgb_dtype):
  """MultiObjectTracker.track with two objects: the five routes return identical arrays."""
  from foundationpose_amd.tracking import MultiObjectTracker
  ests = [e.instance() for e in world['ests']]
  tracker = MultiObjectTracker(ests)
  rgb, depth = world['frames'][0][0].to(rgb_dtype), world['frames'][0][1]
  want = None
  for name, r, d in _routes(rgb, depth):
    for e, p in zip(ests, world['starts']):
      e.pose_last = p.clone()
    got = tracker.track(r, d, world['K'], iteration=1)
    want = got if want is None else want
    assert got.shape == (2, 4, 4) and got.dtype == np.float32 and np.array_equal(got, want), name
  assert not np.array_equal(want[0], want[1])


def test_register_input_kinds(world):
  """MultiObjectTracker.register with two objects, as a list of masks (non-zero values 255 and 7: anything non-zero is the object) and
  as one label image, each from numpy and from device inputs: the stored masks are the bytes `m != 0`, the stored label image is int32,
  and the returned array and every estimator's poses / scores / best_id / pose_last are identical over all four."""
  from foundationpose_amd.tracking import MultiObjectTracker
  rgb, depth, owner = world['frames'][0]
  masks = [(owner == 0).to(torch.uint8) * 255, (owner == 1).to(torch.int32) * 7]
  image = torch.where(owner == 0, 5, torch.where(owner == 1, 9, 0)).to(torch.int64)
  host = lambda x: x.cpu().numpy()
  runs = {}
  for kind, on_host in (('masks', True), ('masks', False), ('labels', True), ('labels', False)):
    put = host if on_host else (lambda x: x.clone())
    ests = [e.instance() for e in world['ests']]
    tracker = MultiObjectTracker(ests)
    if kind == 'masks':
      got = tracker.register(put(rgb), put(depth), world['K'], [put(m) for m in masks], iteration=1)
    else:
      got = tracker.register(put(rgb), put(depth), world['K'], put(image), iteration=1, labels=[5, 9])
    fb = _fb(next(iter(tracker._reg_ws.values())))
    assert torch.equal(_bits(fb.depth), _bits(depth)) and torch.equal(fb.rgb, rgb)
    if kind == 'masks':
      assert fb.labels is None and fb.masks.dtype == torch.uint8 and torch.equal(fb.masks, torch.stack([owner == 0, owner == 1]).to(torch.uint8))
    else:
      assert fb.masks is None and fb.labels.dtype == torch.int32 and torch.equal(fb.labels, image.to(torch.int32))
    assert got.shape == (2, 4, 4) and got.dtype == np.float32 and all(e.pose_last is not None for e in ests)
    runs[kind, on_host] = (got, [(e.poses.clone(), e.scores.clone(), e.best_id.clone(), e.pose_last.clone()) for e in ests])
  first = runs['masks', True]
  assert len(first[1][0][0]) == len(world['ests'][0].rot_grid) and not np.array_equal(first[0][0], first[0][1])
  for key, (got, state) in runs.items():
    assert np.array_equal(got, first[0]), key
    for o in range(2):
      assert all(torch.equal(a, b) for a, b in zip(state[o], first[1][o])), (key, o)


@pytest.mark.parametrize('mode', ['track_one', 'track_multi'])
def test_graph_frames_equal_eager_and_recapture(world, mode, monkeypatch):
  """Three chained frames as one hipGraph each equal the eager frames bit for bit, the third after ctx.reserve has moved the library's
  arena; the graph is captured at the first graphed frame, again after the arena moved, and again after the graph was switched off and on."""
  captures, real = [], torch.cuda.CUDAGraph
  monkeypatch.setattr(torch.cuda, 'CUDAGraph', lambda *a, **kw: captures.append(1) or real(*a, **kw))
  est, K, ctx = world['ests'][0].instance(), world['K'], world['refiner'].ctx
  if mode == 'track_one':
    step = lambda fr: (est.track_one(fr[0], fr[1], K, iteration=1), est.pose_last.clone())
  else:
    step = lambda fr: (est.track_multi(fr[0], fr[1], K, iteration=1, n_hypotheses=4), est.pose_last.clone(), est.poses.clone(), est.scores.clone(),
                       est.best_id.clone())
  runs = []
  for graph in (False, True):
    est.enable_track_graph(graph)
    est.pose_last = world['starts'][0].clone()
    out = []
    for f, fr in enumerate(world['frames']):
      if graph and f == 2:
        # (in steps of 64 hypotheses, not by doubling: the arena only grows, and later modules of the suite move it the same way)
        g0, n = ctx.arena_generation(), 128
        while ctx.arena_generation() == g0 and n <= 4096:
          ctx.reserve(n)
          n += 64
        assert ctx.arena_generation() != g0
      out.append(step(fr))
    runs.append(out)
    assert len(captures) == (2 if graph else 0)
  for a, b in zip(*runs):
    assert np.array_equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
  assert not np.array_equal(runs[0][0][0], runs[0][1][0])
  est.enable_track_graph(False)
  est.enable_track_graph(True)
  est.pose_last = world['starts'][0].clone()
  again = step(world['frames'][0])
  est.enable_track_graph(False)
  assert len(captures) == 3 and np.array_equal(again[0], runs[0][0][0])
