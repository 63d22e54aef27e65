"""GPU: posed boxes, axes and silhouettes drawn on the frame (Utils.draw_poses, fp_draw_poses) against the numpy float64 restatement of
the drawing rule (tests/draw_oracle.py).

The bound: every byte within 1 grey level of the oracle - the kernel blends in fp32, the oracle in float64, and the two can differ where
the unrounded value lies at a rounding tie, by no more - and every pixel the oracle leaves untouched exactly the input.  The seeds are
such that no unrounded endpoint of the oracle lies within 1e-6 of a half-integer (asserted on the oracle's values), so that no endpoint
can legitimately round the other way."""
import ctypes

import numpy as np
import pytest
import torch

from tests import draw_oracle as O
from tests.test_gpu_register_objects import world      # noqa: F401  (the multi-object scene, as a fixture of this module too)

pytestmark = pytest.mark.gpu
FULL_HD_K = np.array([[1600.0, 0, 955.5], [0, 1600.0, 603.2], [0, 0, 1]])
FRAMES = {'640x480': (480, 640), '641x479': (479, 641), '1920x1200': (1200, 1920)}


def _K(h, w):
  from foundationpose_amd import synthetic as S
  return FULL_HD_K if w > 1000 else np.asarray(S.YCB_K, dtype=np.float64)


@pytest.fixture(scope='module')
def base_frame():
  """The synthetic scene's frame (640 x 480 uint8): the other sizes are cut from its mirrored tiling"""
  from tests import util
  rgb = np.ascontiguousarray(util.scene(0)['rgb'])
  assert rgb.dtype == np.uint8 and rgb.shape == (480, 640, 3)
  return rgb


def _frame(base, h, w):
  row = np.concatenate([base, base[:, ::-1]], axis=1)
  big = np.concatenate([row, row[::-1]], axis=0)
  big = np.tile(big, (2, 2, 1))
  return np.ascontiguousarray(big[:h, :w])


def _scene(seed, n, h, w, z_range=(0.4, 1.5)):
  """n random poses whose origins project into the frame, boxes of 5 .. 25 cm and, for every other object, an offset"""
  from foundationpose_amd import synthetic as S
  rs = np.random.RandomState(seed)
  K = _K(h, w)
  poses = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
  boxes = np.zeros((n, 2, 3), dtype=np.float32)
  offs = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
  for o in range(n):
    z = rs.uniform(*z_range)
    u, v = rs.uniform(0, w), rs.uniform(0, h)
    poses[o, :3, :3] = S.random_rotation(np.random.RandomState(seed * 1000 + o))
    poses[o, :3, 3] = [(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z]
    half = rs.uniform(0.025, 0.125, 3)
    boxes[o] = [-half, half]
    if o % 2:
      offs[o, :3, :3] = S.random_rotation(np.random.RandomState(seed * 1000 + 500 + o))
      offs[o, :3, 3] = rs.uniform(-0.03, 0.03, 3)
  return K, poses, boxes, offs


def _oracle_objects(n, boxes, offs, axis_scale=0.1, rgb=True):
  from foundationpose_amd import Utils as U
  pal = U.DRAW_PALETTE[np.arange(n) % 8]
  axis = np.eye(3, dtype=np.uint8) * 255
  if not rgb:
    pal, axis = pal[:, ::-1], axis[:, ::-1]
  return [O.make_object(boxes[o], offs[o], axis_scale=axis_scale, box_color=pal[o], axis_color=axis) for o in range(n)]


def _compare(got, img, want, touched, label):
  got = np.asarray(got)
  diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
  n_off = int((diff > 0).sum())
  print(f'{label}: max |kernel - oracle| = {int(diff.max())} grey levels, {n_off} of {diff.size} bytes differ, {int(touched.sum())} pixels touched')
  assert diff.max() <= 1, f'{label}: {int((diff > 1).sum())} bytes differ from the oracle by more than 1 grey level (max {int(diff.max())})'
  assert np.array_equal(got[~touched], img[~touched]), f'{label}: a pixel the oracle leaves untouched is not the input'


@pytest.mark.parametrize('n', [1, 8, 64])
@pytest.mark.parametrize('frame', list(FRAMES))
def test_parity_with_the_oracle(base_frame, frame, n):
  from foundationpose_amd import Utils as U
  h, w = FRAMES[frame]
  img = _frame(base_frame, h, w)
  seed = {'640x480': 1, '641x479': 2, '1920x1200': 3}[frame] * 10 + {1: 0, 8: 1, 64: 2}[n]
  K, poses, boxes, offs = _scene(seed, n, h, w)
  transparency = 0.25 if n == 8 else 0.0
  want, touched, segs = O.draw(img, K, poses, _oracle_objects(n, boxes, offs), opacity=1.0 - transparency)
  assert O.endpoint_margin(segs) > 1e-6, 'pick another seed: an endpoint lies at a rounding tie'
  assert touched.any()
  got = U.draw_poses(torch.as_tensor(img, device='cuda'), K, torch.as_tensor(poses, device='cuda'), bboxes=boxes, offsets=offs, transparency=transparency)
  assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.uint8
  _compare(got.cpu().numpy(), img, want, touched, f'{frame} n={n}')


def test_numpy_in_numpy_out_thickness_and_bgr(base_frame):
  from foundationpose_amd import Utils as U
  h, w = FRAMES['640x480']
  K, poses, boxes, offs = _scene(7, 3, h, w)
  want, touched, segs = O.draw(base_frame, K, poses, _oracle_objects(3, boxes, offs, axis_scale=0.07, rgb=False), box_thickness=5, axis_thickness=1.5)
  assert O.endpoint_margin(segs) > 1e-6
  got = U.draw_poses(base_frame, K, poses, bboxes=boxes, offsets=offs, box_thickness=5, axis_thickness=1.5, axis_scale=0.07, is_input_rgb=False)
  assert isinstance(got, np.ndarray) and got is not base_frame
  _compare(got, base_frame, want, touched, 'numpy, thickness 5 / 1.5, BGR')


def test_in_place_equals_out_of_place_and_two_calls_are_identical(base_frame):
  from foundationpose_amd import Utils as U
  for frame in ('640x480', '641x479'):
    h, w = FRAMES[frame]
    img = torch.as_tensor(_frame(base_frame, h, w), device='cuda')
    K, poses, boxes, offs = _scene(11, 8, h, w)
    a = U.draw_poses(img, K, poses, bboxes=boxes, offsets=offs)
    b = U.draw_poses(img, K, poses, bboxes=boxes, offsets=offs)
    assert a.data_ptr() != img.data_ptr() and torch.equal(a, b)
    work = img.clone()
    c = U.draw_poses(work, K, poses, bboxes=boxes, offsets=offs, out=work)
    assert c is work and torch.equal(work, a) and not torch.equal(work, img)


def test_objects_that_do_not_overlap_are_drawn_as_each_alone(base_frame):
  from foundationpose_amd import Utils as U
  h, w = FRAMES['640x480']
  K = _K(h, w)
  img = torch.as_tensor(base_frame, device='cuda')
  poses = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
  poses[0, :3, 3], poses[1, :3, 3] = [-0.2, 0.0, 0.8], [0.2, 0.02, 0.8]
  boxes = np.array([[[-0.05, -0.06, -0.04], [0.05, 0.06, 0.04]], [[-0.04, -0.05, -0.06], [0.04, 0.05, 0.06]]], dtype=np.float32)
  cols = np.array([[255, 0, 0], [0, 0, 255]])
  both = U.draw_poses(img, K, poses, bboxes=boxes, colors=cols)
  first = U.draw_poses(img, K, poses[:1], bboxes=boxes[:1], colors=cols[:1])
  second = U.draw_poses(img, K, poses[1:], bboxes=boxes[1:], colors=cols[1:])
  t1, t2 = (first != img).any(-1), (second != img).any(-1)
  assert t1.any() and t2.any() and not (t1 & t2).any()
  expect = torch.where(t1[..., None], first, torch.where(t2[..., None], second, img))
  assert torch.equal(both, expect)


def test_edge_cases(base_frame):
  from foundationpose_amd import Utils as U
  h, w = FRAMES['640x480']
  K = _K(h, w)
  img = torch.as_tensor(base_frame, device='cuda')
  box = np.array([[-0.1, -0.08, -0.3], [0.1, 0.08, 0.3]], dtype=np.float32)
  # partly behind the camera: the box reaches from z = -0.1 to z = 0.5
  pose = np.eye(4, dtype=np.float32)
  pose[:3, 3] = [0.03, 0.02, 0.2]
  ob = _oracle_objects(1, box[None], np.eye(4, dtype=np.float32)[None], axis_scale=0.4)
  want, touched, segs = O.draw(base_frame, K, pose[None], ob)
  assert O.endpoint_margin(segs) > 1e-6
  assert 0 < len(segs) < 15 and max(np.abs(s['xy']).max() for s in segs) > 3000      # some edges dropped, some cut on the near plane
  _compare(U.draw_poses(img, K, pose[None], bboxes=box, axis_scale=0.4).cpu().numpy(), base_frame, want, touched, 'partly behind the camera')
  # wholly behind the camera, and wholly beside the frame: nothing changes
  for t in ([0.0, 0.0, -1.0], [3.0, 0.0, 1.0]):
    pose[:3, 3] = t
    assert torch.equal(U.draw_poses(img, K, pose[None], bboxes=box), img)
  # a box of no extent: twelve points at the origin's pixel
  pose[:3, 3] = [0.05, -0.03, 0.7]
  zero = np.zeros((2, 3), dtype=np.float32)
  want, touched, segs = O.draw(base_frame, K, pose[None], _oracle_objects(1, zero[None], np.eye(4, dtype=np.float32)[None]), flags=O.BOX)
  assert len(segs) == 12 and 0 < touched.sum() <= 9
  _compare(U.draw_poses(img, K, pose[None], bboxes=zero, axes=False).cpu().numpy(), base_frame, want, touched, 'zero-extent box')
  # no object: a copy; in place: untouched
  out = U.draw_poses(img, K, np.zeros((0, 4, 4), dtype=np.float32))
  assert out.data_ptr() != img.data_ptr() and torch.equal(out, img)
  # nothing to draw (no box given, axes off): a copy as well
  assert torch.equal(U.draw_poses(img, K, pose[None], axes=False), img)


@pytest.fixture(scope='module')
def three_instances():
  """Three overlapping instances of the mustard mesh on the 640 x 480 frame and their owner map (Utils.scene_instances)"""
  from foundationpose_amd import Utils as U, synthetic as S
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  mesh = S.make_mustard_mesh(seed=0, n_theta=48, n_z=42)
  mesh.vertices = mesh.vertices - (mesh.vertices.min(0) + mesh.vertices.max(0)) / 2
  mt = make_mesh_tensors(mesh)
  poses = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
  for o, t in enumerate(([-0.03, 0.0, 0.6], [0.03, 0.01, 0.65], [0.0, -0.04, 0.7])):
    poses[o, :3, :3] = S.random_rotation(np.random.RandomState(20 + o))
    poses[o, :3, 3] = t
  K = np.asarray(S.YCB_K, dtype=np.float64)
  owner = U.scene_instances(K, 480, 640, mt, poses, want=('owner',))['owner']
  to_origin, bbox = U.model_box(mesh)
  return dict(K=K, poses=poses, owner=owner, bbox=bbox.astype(np.float32), mesh=mesh)


def test_fill_and_contour(base_frame, three_instances):
  from foundationpose_amd import Utils as U
  t = three_instances
  K, poses, owner = t['K'], t['poses'], t['owner']
  own = owner.cpu().numpy()
  assert all((own == o).any() for o in range(3)) and (own == -1).any()
  img = torch.as_tensor(base_frame, device='cuda')
  boxes, offs = np.tile(t['bbox'], (3, 1, 1)), np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
  objs = _oracle_objects(3, boxes, offs)
  for fill_alpha, contour, flags in ((0.35, True, O.BOX | O.AXES | O.FILL | O.CONTOUR), (0.5, False, O.BOX | O.AXES | O.FILL), (0.0, True, O.AXES | O.CONTOUR)):
    want, touched, segs = O.draw(base_frame, K, poses, objs, flags=flags, fill_alpha=fill_alpha, owner=own)
    assert O.endpoint_margin(segs) > 1e-6
    got = U.draw_poses(img, K, poses, bboxes=boxes if flags & O.BOX else None, owner=owner, fill_alpha=fill_alpha, contour=contour)
    _compare(got.cpu().numpy(), base_frame, want, touched, f'fill_alpha {fill_alpha} contour {contour}')
  # the byte path reads the owner map pixel by pixel: the same scene on a 637-wide cut of the frame
  cut, own_cut = np.ascontiguousarray(base_frame[:, :637]), np.ascontiguousarray(own[:, :637])
  want, touched, _ = O.draw(cut, K, poses, objs, flags=15, fill_alpha=0.35, owner=own_cut)
  got = U.draw_poses(cut, K, poses, bboxes=boxes, owner=own_cut, fill_alpha=0.35, contour=True)
  _compare(got, cut, want, touched, 'fill + contour, 637 wide')
  # owner values that name no object count as none
  none = torch.full_like(owner, -1)
  plain = U.draw_poses(img, K, poses, bboxes=boxes)
  assert torch.equal(U.draw_poses(img, K, poses, bboxes=boxes, owner=none, fill_alpha=0.35, contour=True), plain)
  assert torch.equal(U.draw_poses(img, K, poses, bboxes=boxes, owner=torch.full_like(owner, 3), fill_alpha=0.35, contour=True), plain)
  assert torch.equal(U.draw_poses(img, K, poses, box=False, axes=False, owner=none, fill_alpha=0.35, contour=True), img)
  with pytest.raises(ValueError, match='owner'):
    U.draw_poses(img, K, poses, fill_alpha=0.3)


def _raw_args(img_in, img_out, K, poses, objs, n, flags=3, owner=None, box_thickness=2.0, axis_thickness=3.0, opacity=1.0, fill_alpha=0.0):
  from foundationpose_amd import _lib
  a = _lib.FpDrawArgs()
  a.struct_size = ctypes.sizeof(a)
  a.d_img_in = img_in.data_ptr() if img_in is not None else None
  a.d_img_out = img_out.data_ptr() if img_out is not None else None
  a.H, a.W = (int(img_in.shape[0]), int(img_in.shape[1])) if img_in is not None else (480, 640)
  a.K = K.ctypes.data if K is not None else None
  a.d_poses = poses.data_ptr() if poses is not None else None
  a.n_obj = n
  a.objs = ctypes.addressof(objs) if objs is not None else None
  a.flags, a.box_thickness, a.axis_thickness, a.opacity, a.fill_alpha = flags, box_thickness, axis_thickness, opacity, fill_alpha
  a.d_owner = owner.data_ptr() if owner is not None else None
  return a


def _raw_objects(n, boxes, offs):
  from foundationpose_amd import Utils as U, _lib
  objs = (_lib.FpDrawObject * n)()
  for o in range(n):
    objs[o].bbox_min[:], objs[o].bbox_max[:] = boxes[o, 0].tolist(), boxes[o, 1].tolist()
    objs[o].offset[:] = offs[o].reshape(-1).tolist()
    objs[o].axis_scale = 0.1
    objs[o].box_color[:] = objs[o].fill_color[:] = U.DRAW_PALETTE[o % 8].tolist()
    objs[o].axis_color[:] = [255, 0, 0, 0, 255, 0, 0, 0, 255]
  return objs


def test_every_refusal(base_frame):
  from foundationpose_amd import _lib
  from foundationpose_amd._lib import lib, stream_ptr
  ctx = _lib.Context.get('cuda:0')
  h, w = FRAMES['640x480']
  K, poses, boxes, offs = _scene(5, 2, h, w)
  Kd = np.ascontiguousarray(K)
  img = torch.as_tensor(base_frame, device='cuda')
  buf = torch.zeros((2 * h * w * 3,), dtype=torch.uint8, device='cuda')
  out = buf[:h * w * 3].reshape(h, w, 3)
  P = torch.as_tensor(poses, device='cuda')
  owner = torch.full((h, w), -1, dtype=torch.int32, device='cuda')
  objs = _raw_objects(2, boxes, offs)
  call = lambda a, c=ctx.handle: lib().fp_draw_poses(c, ctypes.byref(a) if a is not None else None, stream_ptr())
  good = lambda **kw: _raw_args(kw.pop('img_in', img), kw.pop('img_out', out), kw.pop('K', Kd), kw.pop('poses', P), kw.pop('objs', objs), kw.pop('n', 2), **kw)
  assert call(good()) == 0
  assert call(good(), None) == _lib.FP_EINVAL and call(None) == _lib.FP_EINVAL
  bad = [good(img_in=None), good(img_out=None), good(K=None), good(objs=None), good(poses=None)]
  a = good(); a.struct_size = ctypes.sizeof(a) - 8; bad.append(a)
  a = good(); a.struct_size = 0; bad.append(a)
  for hh, ww in ((0, 640), (480, 0), (-1, 640), (1 << 16, 1 << 15)):
    a = good(); a.H, a.W = hh, ww; bad.append(a)
  bad += [good(n=-1), good(n=_lib.FP_DRAW_MAX_OBJECTS + 1), good(flags=16), good(flags=-1), good(flags=_lib.FP_DRAW_FILL), good(flags=_lib.FP_DRAW_CONTOUR | 1)]
  nan = float('nan')
  bad += [good(box_thickness=v) for v in (0.0, -1.0, 64.5, nan)] + [good(axis_thickness=v) for v in (0.0, -1.0, 64.5, nan)]
  bad += [good(opacity=v) for v in (-0.01, 1.01, nan)] + [good(fill_alpha=v) for v in (-0.01, 1.01, nan)]
  bad += [good(img_in=buf[3:3 + h * w * 3].reshape(h, w, 3), img_out=out), good(img_in=out, img_out=buf[h * w * 3 - 1:2 * h * w * 3 - 1].reshape(h, w, 3))]
  before = out.clone()
  for i, a in enumerate(bad):
    assert call(a) == _lib.FP_EINVAL, f'refusal {i} was accepted'
    assert lib().fp_last_error()
  torch.cuda.synchronize()
  assert torch.equal(out, before)                                # nothing was queued
  # adjoining images are not overlapping ones; n_obj = 0 and flags = 0 copy (null objs / d_poses allowed with n_obj = 0)
  second = buf[h * w * 3:].reshape(h, w, 3)
  assert call(good(img_in=out, img_out=second)) == 0
  second.zero_()
  assert call(good(img_out=second, n=0, objs=None, poses=None)) == 0 and torch.equal(second, img)
  second.zero_()
  assert call(good(img_out=second, flags=0, owner=None)) == 0 and torch.equal(second, img)
  assert call(good(img_out=second, flags=15, owner=owner, fill_alpha=0.3)) == 0


def test_graph_capture_reads_the_poses_at_replay(base_frame):
  from foundationpose_amd import _lib
  from foundationpose_amd._lib import check, lib, stream_ptr
  ctx = _lib.Context.get('cuda:0')
  ctx.reserve(1)
  h, w = FRAMES['640x480']
  K, poses_a, boxes, offs = _scene(21, 8, h, w)
  _, poses_b, _, _ = _scene(22, 8, h, w)
  Kd = np.ascontiguousarray(K)
  img = torch.as_tensor(base_frame, device='cuda')
  objs = _raw_objects(8, boxes, offs)
  P = torch.as_tensor(poses_a, device='cuda')
  out = torch.zeros_like(img)
  args = _raw_args(img, out, Kd, P, objs, 8)

  def eager(p):
    res = torch.zeros_like(img)
    check(lib().fp_draw_poses(ctx.handle, ctypes.byref(_raw_args(img, res, Kd, torch.as_tensor(p, device='cuda'), objs, 8)), stream_ptr()))
    torch.cuda.synchronize()
    return res
  want_a, want_b = eager(poses_a), eager(poses_b)
  assert not torch.equal(want_a, want_b) and not torch.equal(want_a, img)
  generation = ctx.arena_generation()
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    check(lib().fp_draw_poses(ctx.handle, ctypes.byref(args), stream_ptr()))
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    check(lib().fp_draw_poses(ctx.handle, ctypes.byref(args), stream_ptr()))
  assert ctx.arena_generation() == generation
  out.zero_()
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(out, want_a)
  P.copy_(torch.as_tensor(poses_b, device='cuda'))
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(out, want_b)


def test_reference_signatures(base_frame):
  from foundationpose_amd import Utils as U
  h, w = FRAMES['640x480']
  K = _K(h, w)
  pose = np.eye(4)
  pose[:3, 3] = [0.02, -0.01, 0.6]
  bbox = np.array([[-0.06, -0.04, -0.09], [0.06, 0.04, 0.09]])
  img = base_frame.copy()
  ret = U.draw_posed_3d_box(K, img=img, ob_in_cam=pose, bbox=bbox)
  assert ret is img and not np.array_equal(img, base_frame)     # drawn IN PLACE, as cv2.line does (main.py:68-69 relies on it)
  want, touched, _ = O.draw(base_frame, K, pose[None], [O.make_object(bbox)], flags=O.BOX)
  _compare(img, base_frame, want, touched, 'draw_posed_3d_box')
  assert (img[touched][:, 1] >= base_frame[touched][:, 1]).all()      # the default line colour is green
  before = img.copy()
  vis = U.draw_xyz_axis(img, ob_in_cam=pose, scale=0.1, K=K, thickness=3, transparency=0, is_input_rgb=True)
  assert vis is not img and np.array_equal(img, before) and not np.array_equal(vis, img)     # a new array: the input stays
  want, touched, segs = O.draw(before, K, pose[None], [O.make_object(np.zeros((2, 3)))], flags=O.AXES)
  _compare(vis, before, want, touched, 'draw_xyz_axis rgb')
  # the x axis is red in either channel order
  x_end = segs[0]['xy'][1].astype(int)
  assert list(vis[x_end[1], x_end[0]]) == [255, 0, 0]
  bgr = U.draw_xyz_axis(before, ob_in_cam=pose, scale=0.1, K=K)
  assert list(bgr[x_end[1], x_end[0]]) == [0, 0, 255]
  # on the device the box is drawn in place too
  dev = torch.as_tensor(base_frame, device='cuda')
  assert U.draw_posed_3d_box(K, dev, pose, bbox) is dev and np.array_equal(dev.cpu().numpy(), img)
  np.testing.assert_array_equal(U.project_3d_to_2d(np.array([0, 0, 0, 1.0]), K, pose), segs[0]['xy'][0])


def test_pipeline_visualize_sets_data_vis():
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.config import REFINE_DEFAULT, SCORE_DEFAULT
  from foundationpose_amd.pipeline import FoundationPoseEstimator, Pipeline, PipelineData, Processor
  from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
  from foundationpose_amd.predict_score import ScorePredictor
  from tests import cases, util
  sc = util.scene(0)

  class Frame(Processor):
    def process(self, data):
      data.rgb, data.depth, data.K, data.mask = sc['rgb'], sc['depth'], sc['K'], sc['mask']
      return data
  refiner = PoseRefinePredictor(state_dict=S.make_refine_state_dict(0, head_gain=cases.GAIN_CHAIN), cfg=REFINE_DEFAULT)
  scorer = ScorePredictor(state_dict=S.make_score_state_dict(1), cfg=SCORE_DEFAULT)
  stage = FoundationPoseEstimator(mesh=S.make_mustard_mesh(seed=0), K=sc['K'], est_refine_iter=1, scorer=scorer, refiner=refiner)
  np.random.seed(0)
  data = Pipeline('demo', stop_on_error=True, visualize=True).add_processor(Frame()).add_processor(stage).run(PipelineData())
  assert not data.errors
  assert isinstance(data.vis, np.ndarray) and data.vis.shape == np.asarray(data.rgb).shape and data.vis.dtype == np.uint8
  assert not np.array_equal(data.vis, data.rgb)
  assert Pipeline('plain').add_processor(Frame()).run(PipelineData()).__dict__.get('vis') is None


def test_tracker_draw_after_register_and_track(world):      # noqa: F811
  """MultiObjectTracker.draw on the multi-object scene of tests/test_gpu_register_objects.py"""
  from foundationpose_amd import Utils as U, synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  from tests import test_gpu_register_objects as R
  ests = [R._instance(e) for e in world['ests'][:3]]
  rgb, depth, masks = world['rgb'], world['depth'], world['masks'][:3]
  tracker = MultiObjectTracker(ests)
  with pytest.raises(ValueError, match='register it first'):
    tracker.draw(rgb)
  tracker.register(rgb, depth, S.YCB_K, masks, iteration=1)
  poses = tracker.track(rgb, depth, S.YCB_K, iteration=1)
  boxes, offs = zip(*[(U.model_box(e.mesh_ori)[1], np.linalg.inv(U.model_box(e.mesh_ori)[0])) for e in ests])
  want = U.draw_poses(rgb, S.YCB_K, poses, bboxes=np.stack(boxes), offsets=np.stack(offs))
  got = tracker.draw(rgb)
  assert isinstance(got, np.ndarray) and np.array_equal(got, want) and not np.array_equal(got, rgb)
  on_dev = tracker.draw(torch.as_tensor(rgb, device='cuda'))
  assert torch.is_tensor(on_dev) and np.array_equal(on_dev.cpu().numpy(), want)
  # the tint lands on the objects' visible pixels only
  owner = tracker.instance_masks()['owner'].cpu().numpy()
  assert (owner >= 0).any()
  tinted = tracker.draw(rgb, fill_alpha=0.5, box=False, axes=False)
  changed = (tinted != rgb).any(-1)
  assert changed.any() and not changed[owner < 0].any()
  full = tracker.draw(rgb, fill_alpha=0.5, contour=True, depth=depth)
  assert (full != got).any() and np.array_equal(full[owner < 0], got[owner < 0])
