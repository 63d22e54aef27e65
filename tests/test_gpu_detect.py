"""GPU: fp_template_match (csrc/detect.hip) against its numpy restatement tests/detect_oracle.py, bit for bit; what needs no restatement
(batch and run independence, an empty frame, a captured graph); the detector on seeded clutter scenes rendered by the library against
the TRUTH; and the public layers over it (FoundationPose.detect / register_at / register_detected, MultiObjectTracker.detect).
tests/test_detect_host.py pins the restatement itself.  Every case is a few thousand anchor pixels."""
import numpy as np
import pytest
import torch

from tests import detect_oracle as O

pytestmark = pytest.mark.gpu
F = np.float32


def small_set(table, ranges):
  from foundationpose_amd import detect as Dt
  n = len(table)
  return Dt.TemplateSet(table, np.tile(np.eye(3), (n, 1, 1)), 12, 9, 2, ranges, [0.1] * (len(ranges) - 1), [])


def match_kw(c):
  return dict(tol_in=c['tol_in'], tol_out=c['tol_out'], z_range=(c['z_min'], c['z_max']), zfar=c['zfar'])


@pytest.fixture(scope='module')
def small():
  c = O.small_case()
  c['set'] = small_set(c['table'], c['ranges'])
  return c


@pytest.mark.parametrize('stride,offset', [(2, (0, 0)), (3, (1, 2))])
def test_maps_and_counts_equal_the_restatement(small, stride, offset):
  from foundationpose_amd import detect as Dt
  c = small
  keys, counts = Dt.match_templates(c['frames'], c['K'], c['set'], stride=stride, offset=offset, return_counts=True, **match_kw(c))
  assert keys.dtype == np.uint32 and keys.shape == (3, 2) + Dt.lattice_shape(72, 96, stride, offset)
  for f in range(3):
    want_k, want_n, _ = O.match(c['frames'][f], c['K'], c['table'], c['ranges'], 12, 9, 2, stride, offset[0], offset[1], c['z_min'], c['z_max'], c['zfar'],
                                c['tol_in'], c['tol_out'])
    assert (keys[f] == want_k).all(), f'frame {f}: {int((keys[f] != want_k).sum())} keys differ'
    assert (counts[f] == want_n).all(), f'frame {f}: {int((counts[f] != want_n).sum())} counts differ'
    assert (want_k > 0).mean() > 0.5
  _, t_local, _ = Dt.decode_keys(keys[0, 0])
  assert (t_local[keys[0, 0] > 0] != 5).all() and (t_local[keys[0, 0] > 0] == 2).any()      # the duplicate: the lower index wins
  # keys alone, and one anchor of the two
  assert (Dt.match_templates(c['frames'], c['K'], c['set'], stride=stride, offset=offset, **match_kw(c)) == keys).all()
  one = Dt.match_templates(c['frames'][0], c['K'], c['set'], stride=stride, offset=offset, anchors=1, **match_kw(c))
  want_k, _, _ = O.match(c['frames'][0], c['K'], c['table'], c['ranges'], 12, 9, 1, stride, offset[0], offset[1], c['z_min'], c['z_max'], c['zfar'], c['tol_in'],
                         c['tol_out'])
  assert (one == want_k).all()


def test_template_count_of_two_staged_chunks_plus_one(small):
  from foundationpose_amd import detect as Dt
  chunk = Dt.staged_templates(12, 9)
  n = 2 * chunk + 1
  table = O.small_table(n, seed=1)
  frame = np.ascontiguousarray(small['frames'][0][20:44, 24:56])
  K = np.array([[110.0, 0, 15.3], [0, 108.0, 11.6], [0, 0, 1.0]])
  for count in (n, chunk, chunk + 1):
    ts = small_set(table[:count], [0, count])
    keys, counts = Dt.match_templates(frame, K, ts, stride=1, return_counts=True, **match_kw(small))
    want_k, want_n, _ = O.match(frame, K, table[:count], [0, count], 12, 9, 2, 1, 0, 0, small['z_min'], small['z_max'], small['zfar'], small['tol_in'],
                                small['tol_out'])
    assert (keys == want_k).all() and (counts == want_n).all()
    _, t_local, _ = Dt.decode_keys(keys)
    if count == n:
      assert t_local[keys > 0].max() >= 2 * chunk - 8      # winners come from the last chunk too


def test_same_bits_alone_in_any_batch_and_on_a_second_run(small):
  from foundationpose_amd import detect as Dt
  c = small
  kw = dict(stride=2, return_counts=True, **match_kw(c))
  alone = [Dt.match_templates(c['frames'][f], c['K'], c['set'], **kw) for f in range(3)]
  for order in ((0, 1, 2), (2, 0, 1), (1, 1, 0, 2, 2)):
    keys, counts = Dt.match_templates(np.ascontiguousarray(c['frames'][list(order)]), c['K'], c['set'], **kw)
    for i, f in enumerate(order):
      assert (keys[i] == alone[f][0]).all() and (counts[i] == alone[f][1]).all()
  again = Dt.match_templates(c['frames'][1], c['K'], c['set'], **kw)
  assert (again[0] == alone[1][0]).all() and (again[1] == alone[1][1]).all()


def test_an_empty_frame_gives_an_empty_map_and_empty_calls_launch_nothing(small):
  from foundationpose_amd import detect as Dt
  c = small
  for frame in (np.zeros((72, 96), F), np.full((72, 96), np.nan, F), np.full((72, 96), c['zfar'], F)):
    keys, counts = Dt.match_templates(frame, c['K'], c['set'], stride=2, return_counts=True, **match_kw(c))
    assert not keys.any() and not counts.any()
  none = small_set(c['table'][:0], [0, 0])
  assert not Dt.match_templates(c['frames'][0], c['K'], none, stride=2, **match_kw(c)).any()
  assert Dt.match_templates(c['frames'][:0], c['K'], c['set'], stride=2, **match_kw(c)).shape == (0, 2, 36, 48)


def test_capture_and_replay_give_the_same_bits(small):
  from foundationpose_amd import detect as Dt
  c = small
  dev = torch.device('cuda', 0)
  depth = torch.as_tensor(c['frames'][0], device=dev)
  kw = dict(stride=2, return_counts=True, **match_kw(c))
  want = Dt.match_templates(depth, c['K'], c['set'], **kw)
  torch.cuda.synchronize()
  stream = torch.cuda.Stream(dev)
  with torch.cuda.stream(stream):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
      got = Dt.match_templates(depth, c['K'], c['set'], **kw)
    for k in got:
      k.view(torch.int32).zero_()
    graph.replay()
    depth.copy_(torch.as_tensor(c['frames'][1], device=dev))
    stream.synchronize()
    assert all((g.cpu().numpy() == w.cpu().numpy()).all() for g, w in zip(got, want))
    graph.replay()      # the same launch on the frame now in the buffer
    stream.synchronize()
  other = Dt.match_templates(c['frames'][1], c['K'], c['set'], **kw)
  assert all((g.cpu().numpy() == w).all() for g, w in zip(got, other))


# ---- the detector against the truth, and the public layers ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rig():
  """One estimator on the mustard model with seeded random networks (as smoke() builds it) and its 504 templates."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.config import REFINE_DEFAULT, SCORE_DEFAULT
  from foundationpose_amd.estimater import FoundationPose
  from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
  from foundationpose_amd.predict_score import ScorePredictor
  torch.cuda.set_device(0)
  mesh = S.make_mustard_mesh(seed=0, n_theta=48, n_z=42)
  refiner = PoseRefinePredictor(state_dict=S.make_refine_state_dict(0), cfg=REFINE_DEFAULT)
  scorer = ScorePredictor(state_dict=S.make_score_state_dict(1), cfg=SCORE_DEFAULT)
  np.random.seed(0)
  est = FoundationPose(model_pts=mesh.vertices, model_normals=mesh.vertex_normals, mesh=mesh, refiner=refiner, scorer=scorer)
  est.rot_grid = est.rot_grid[:8].contiguous()
  return dict(est=est, mesh=mesh, refiner=refiner, scorer=scorer, build=dict(n_views=42))


def library_instances(est):
  """render_instances of O.clutter_scene on the device: the object alone through the rasteriser, the spheres through the compositor
  (Utils.scene_instances: each sphere's layer is the composite where it is in front)."""
  from foundationpose_amd import Utils as U
  from foundationpose_amd import synthetic as S

  def render(K, H, W, shapes, poses):
    obj = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=poses[:1], mesh_tensors=est.mesh_tensors)[1][0].cpu().numpy()
    meshes = [est.mesh_tensors] + [U.make_mesh_tensors(S.SimpleMesh(s[0], s[1])) for s in shapes[1:]]
    out = U.scene_instances(K, H, W, meshes, poses, want=('owner', 'depth'))
    owner, depth = out['owner'].cpu().numpy(), out['depth'].cpu().numpy()
    return np.stack([obj] + [np.where(owner == i, depth, 0) for i in range(1, len(shapes))])
  return render


@pytest.mark.parametrize('seed', O.SCENE_SEEDS)
def test_clutter_scene_top1_is_the_object_and_beats_the_mask_path(rig, seed):
  """tests/test_detect_host.py's scene test with the library in every place: its rasteriser and compositor make the scene, its prelude
  filters the depth, its kernel matches, and the TRUTH judges: the best detection projects into the object's visible mask and its centre
  is no farther from the true one than guess_translation's from the perfect visible mask of the same filtered depth."""
  est = rig['est']
  sc = O.clutter_scene(seed, library_instances(est))
  assert sc['visible_fraction'] >= 0.9
  top = est.detect(sc['depth'], sc['K'], top_k=1, stride=2, **rig['build'])[0]
  truth = sc['pose'][:3, 3]
  uv = sc['K'] @ top['centre'] / top['centre'][2]
  err = np.linalg.norm(top['centre'] - truth)
  filtered = est._prelude(sc['depth'])
  err_mask = np.linalg.norm(est.guess_translation(filtered, sc['mask'], sc['K']) - truth)
  print(f'seed {seed}: detect {err * 1000:.1f} mm, guess_translation {err_mask * 1000:.1f} mm, in {top["in_fraction"]:.2f} out {top["out_fraction"]:.2f}')
  assert sc['mask'][int(round(uv[1])), int(round(uv[0]))]
  assert err <= err_mask
  assert np.abs(top['pose'] @ np.linalg.inv(est.get_tf_to_centered_mesh().double().cpu().numpy()) - top['ob_in_cam']).max() < 1e-12


@pytest.fixture(scope='module')
def frame(rig):
  """One RGB-D clutter frame with colours: the scene of the first seed, the object's colours from the rasteriser over a grey ramp."""
  from foundationpose_amd import Utils as U
  est = rig['est']
  sc = O.clutter_scene(O.SCENE_SEEDS[0], library_instances(est))
  H, W = sc['depth'].shape
  color = U.nvdiffrast_render(K=sc['K'], H=H, W=W, ob_in_cams=sc['pose'][None], mesh_tensors=est.mesh_tensors, use_light=True)[0][0].cpu().numpy()
  ramp = np.broadcast_to((np.arange(W)[None, :, None] * 255.0 / W), (H, W, 3))
  sc['rgb'] = np.where(sc['mask'][..., None], color * 255.0, ramp).astype(np.uint8)
  return sc


def test_register_at_the_guessed_centre_returns_registers_bits(rig, frame):
  est = rig['est']
  pose = est.register(K=frame['K'], rgb=frame['rgb'], depth=frame['depth'], ob_mask=frame['mask'], iteration=1)
  poses, scores = est.poses.clone(), est.scores.clone()
  c = est.guess_translation(est._prelude(frame['depth']), frame['mask'], frame['K'])
  pose_at = est.register_at(frame['K'], frame['rgb'], frame['depth'], [c], iteration=1)
  assert pose.dtype == pose_at.dtype == np.float32 and (pose.view(np.uint32) == pose_at.view(np.uint32)).all()
  assert torch.equal(poses, est.poses) and torch.equal(scores, est.scores)
  assert (est.register_at(frame['K'], frame['rgb'], frame['depth'], c, iteration=1).view(np.uint32) == pose.view(np.uint32)).all()      # (3,) as well
  with pytest.raises(ValueError, match='finite'):
    est.register_at(frame['K'], frame['rgb'], frame['depth'], [[0.0, np.nan, 0.7]])


def test_register_detected_ends_near_a_detected_centre(rig, frame):
  est = rig['est']
  pose = est.register_detected(frame['K'], frame['rgb'], frame['depth'], top_k=3, iteration=1, stride=2, **rig['build'])
  assert pose.shape == (4, 4) and np.isfinite(pose).all()
  found = est.detect(frame['depth'], frame['K'], top_k=3, stride=2, **rig['build'])
  assert [d['template'] for d in found] == [d['template'] for d in est.detections] and 1 <= len(found) <= 3
  assert len(est.poses) == 8 * len(found) and len(est.scores) == len(est.poses)
  centred = est.pose_last.reshape(4, 4).double().cpu().numpy()
  gaps = [np.linalg.norm(centred[:3, 3] - d['centre']) for d in found]
  assert min(gaps) <= est.diameter / 2, gaps      # with seeded random networks nothing more can be claimed
  assert est.templates(**rig['build']) is est.templates(**rig['build'])      # cached


def test_tracker_detect_feeds_register_and_equals_single_object_calls(rig, frame):
  from foundationpose_amd import Utils as U
  from foundationpose_amd import detect as Dt
  from foundationpose_amd.estimater import FoundationPose
  from foundationpose_amd.tracking import MultiObjectTracker
  small = rig['mesh'].copy()
  small.vertices = small.vertices * 0.7
  np.random.seed(0)
  other = FoundationPose(model_pts=small.vertices, model_normals=small.vertex_normals, mesh=small, refiner=rig['refiner'], scorer=rig['scorer'])
  other.rot_grid = other.rot_grid[:8].contiguous()
  ests = [rig['est'].instance(), other]
  tracker = MultiObjectTracker(ests)
  dets, masks = tracker.detect(frame['depth'], frame['K'], stride=2, **rig['build'])
  assert len(dets) == len(masks) == 2 and all(m.shape == frame['depth'].shape and m.dtype == torch.uint8 for m in masks)
  assert dets[0] is not None and dets[0]['object'] == 0 and masks[0].any()
  poses = tracker.register(frame['rgb'], frame['depth'], frame['K'], masks, iteration=1)
  assert poses.shape == (2, 4, 4) and np.isfinite(poses).all()
  # one call over the concatenated sets gives each object the map of its own call
  sets = [e.templates(**rig['build']) for e in ests]
  depth = rig['est']._prelude(frame['depth'])
  both = Dt.match_templates(depth, frame['K'], Dt.TemplateSet.concat(sets), stride=2, return_counts=True)
  for o, ts in enumerate(sets):
    alone = Dt.match_templates(depth, frame['K'], ts, stride=2, return_counts=True)
    assert all((both[k][o].cpu().numpy() == alone[k][0].cpu().numpy()).all() for k in (0, 1))
    top = U.detect(depth, frame['K'], ts, top_k=1, stride=2)
    assert (top[0]['template'] + int(Dt.TemplateSet.concat(sets).ranges[o]) == dets[o]['template']) if top else dets[o] is None


def test_pipeline_stage_and_bop_mask_source_make_masks(rig, frame):
  from foundationpose_amd import bop, pipeline
  stage = pipeline.Detect(mesh=rig['mesh'], K=frame['K'], stride=2)
  data = stage.process(pipeline.PipelineData(rgb=frame['rgb'], depth=frame['depth']))
  assert data.mask is not None and data.mask.dtype == bool and data.mask.shape == frame['depth'].shape
  assert data.detections and (data.mask & frame['mask']).any()
  assert np.linalg.norm(data.detections[0]['centre'] - frame['pose'][:3, 3]) < 0.1
  again = stage.process(pipeline.PipelineData(rgb=frame['rgb'], depth=frame['depth']))      # a later frame: left alone unless lost
  assert again.mask is None
  assert stage.process(pipeline.PipelineData(rgb=frame['rgb'], depth=frame['depth'], lost=True)).mask is not None
  given = np.zeros_like(frame['mask'])
  fresh = pipeline.Detect(mesh=rig['mesh'], K=frame['K'], stride=2)
  assert fresh.process(pipeline.PipelineData(rgb=frame['rgb'], depth=frame['depth'], mask=given)).mask is given and fresh.templates is None

  class Scene:
    depth = staticmethod(lambda im_id: frame['depth'])
    K = staticmethod(lambda im_id: frame['K'])
  inst = bop.image_instances(Scene(), 0, [dict(obj_id=5, inst_count=2)], 'detect', estimators={5: rig['est']})
  assert 1 <= len(inst) <= 2 and all(o == 5 and m.dtype == bool and m.shape == frame['depth'].shape and m.any() for o, m in inst)
  with pytest.raises(ValueError, match='estimators'):
    bop.image_instances(Scene(), 0, [dict(obj_id=5, inst_count=1)], 'detect')
