"""GPU: a BOP-format dataset end to end (foundationpose_amd.bop): run_bop against the direct MultiObjectTracker.register call on what
BopScene reads, FoundationPose.instance(), and evaluate_results through the whole chain - CSV, ground truth, device errors, matching -
on estimates whose errors are known by construction.

The tree is written at run time: four models (millimetre PLY + models_info.json), one scene with two 480 x 640 images composed from the
HIP renders of the models (depth quantised by the 16-bit PNG at depth_scale 0.1): image 0 holds objects 1, 2, 3 and a second instance of
object 1; image 1 holds objects 1 .. 4 once each."""
import os

import numpy as np
import pytest
import torch

from tests import bop_tree, cases

pytestmark = pytest.mark.gpu
H, W = 480, 640
SCORE_GAIN = 3.0e4
SPOTS = [((-0.07, -0.04, 0.75), 1), ((0.07, -0.03, 0.80), 2), ((0.0, 0.07, 0.70), 3), ((0.09, 0.08, 0.85), 4)]
IMAGE_OBJECTS = {0: [1, 2, 3, 1], 1: [1, 2, 3, 4]}
SHIFTS = (0.0, 0.12, 0.31, 0.60)             # x the diameter, along the camera x axis: each well away from every MSSD threshold


def _pose(t, rot_seed):
  from foundationpose_amd import synthetic as S
  p = np.eye(4, dtype=np.float32)
  p[:3, :3] = S.random_rotation(np.random.RandomState(rot_seed))
  p[:3, 3] = t
  return p


def _frame(ests, poses, seed):
  """RGB-D frame z-composited from the HIP renders of every estimator's centred mesh at its pose over a background plane at 1.2 m
  (as tests/test_gpu_register_objects.py composes its frame): rgb uint8, depth float32, owner int32 (-1 = background)."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.Utils import nvdiffrast_render
  g = torch.Generator(device='cuda').manual_seed(seed)
  vs, us = torch.meshgrid(torch.arange(H, device='cuda'), torch.arange(W, device='cuda'), indexing='ij')
  rgb = torch.stack([0.5 + 0.3 * torch.sin(us * 0.07) * torch.cos(vs * 0.05), 0.45 + 0.3 * torch.sin(us * 0.031 + vs * 0.043),
                     0.4 + 0.25 * torch.cos(vs * 0.09 - us * 0.02)], -1)
  depth = torch.full((H, W), 1.2, device='cuda')
  owner = torch.full((H, W), -1, device='cuda', dtype=torch.int32)
  for o, (e, p) in enumerate(zip(ests, poses)):
    c, d, _ = nvdiffrast_render(K=S.YCB_K, H=H, W=W, ob_in_cams=torch.as_tensor(p, device='cuda').reshape(1, 4, 4), mesh_tensors=e.mesh_tensors,
                                use_light=True)
    near = (d[0] > 0) & (d[0] < depth)
    depth = torch.where(near, d[0], depth)
    rgb = torch.where(near[..., None], c[0], rgb)
    owner = torch.where(near, torch.full_like(owner, o), owner)
  rgb = (rgb * 255 + torch.randn(rgb.shape, device='cuda', generator=g) * 1.5).clamp(0, 255).to(torch.uint8)
  depth = depth + torch.randn(depth.shape, device='cuda', generator=g) * 0.001
  return rgb.cpu().numpy(), depth.cpu().numpy(), owner.cpu().numpy()


@pytest.fixture(scope='module')
def world(tmp_path_factory):
  from foundationpose_amd import bop
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.config import REFINE_DEFAULT, SCORE_DEFAULT
  from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
  from foundationpose_amd.predict_score import ScorePredictor
  refiner = PoseRefinePredictor(state_dict=S.make_refine_state_dict(cases.REFINE_SEED, head_gain=cases.GAIN_CHAIN), cfg=REFINE_DEFAULT)
  # the output layer of the seeded scorer is scaled as in tests/test_gpu_register_objects.py, for the reason given there: the scores of a
  # registration must be unique, or the order of its hypotheses has no single answer
  ssd = S.make_score_state_dict(cases.SCORE_SEED)
  ssd['linear.weight'] = ssd['linear.weight'] * SCORE_GAIN
  ssd['linear.bias'] = ssd['linear.bias'] * SCORE_GAIN - SCORE_GAIN * 0.0795
  scorer = ScorePredictor(state_dict=ssd, cfg=SCORE_DEFAULT)
  root = tmp_path_factory.mktemp('bop_gpu')
  meshes = {1: S.make_mustard_mesh(seed=0), 2: S.make_mustard_mesh(seed=1, n_theta=80, n_z=70), 3: S.make_mustard_mesh(seed=2, n_theta=64, n_z=60),
            4: S.make_mustard_mesh(seed=3, n_theta=72, n_z=64)}
  models = bop.BopModels(bop_tree.write_models(root, {o: (m, {}) for o, m in meshes.items()}))
  ests = bop.build_estimators(models, [1, 2, 3, 4], refiner, scorer, diameter='info')
  images = []
  for im_id, objs in IMAGE_OBJECTS.items():
    poses = [_pose(t, s + 10 * im_id) for t, s in SPOTS]
    rgb, depth, owner = _frame([ests[o] for o in objs], poses, seed=im_id)
    gt = [dict(obj_id=o, pose=p.astype(np.float64) @ ests[o].get_tf_to_centered_mesh().double().cpu().numpy(), mask=owner == k, visib_fract=1.0)
          for k, (o, p) in enumerate(zip(objs, poses))]
    images.append(dict(im_id=im_id, K=S.YCB_K, depth_scale=0.1, rgb=rgb, depth_png=np.round(depth * 1e4).astype(np.uint16), gt=gt))
  bop_tree.write_scene(root, images)
  targets = bop.targets_from_gt(root, 'test')
  assert targets == [dict(scene_id=1, im_id=0, obj_id=1, inst_count=2), dict(scene_id=1, im_id=0, obj_id=2, inst_count=1),
                     dict(scene_id=1, im_id=0, obj_id=3, inst_count=1)] + [dict(scene_id=1, im_id=1, obj_id=o, inst_count=1) for o in (1, 2, 3, 4)]
  bop_tree.write_targets(root, targets)
  return dict(root=str(root), refiner=refiner, scorer=scorer, models=models, ests=ests, targets=targets,
              scene=bop.BopScene(os.path.join(str(root), 'test', '000001')))


def test_models_info_diameter_is_the_exact_one(world):
  """models_info.json (written by the test from a float64 all-pairs maximum) against the device's exact diameter of the loaded model."""
  from foundationpose_amd import Utils as U
  for o in (1, 2, 3, 4):
    d = U.mesh_diameter(mesh=world['models'].mesh(o))
    assert abs(d - world['models'].diameter(o)) <= 4 * 2.0 ** -23 * d + 1e-9
    assert world['ests'][o].diameter == world['models'].diameter(o)


@pytest.mark.parametrize('max_objects', [None, 2])
def test_run_bop_equals_the_direct_call_bit_for_bit(world, max_objects):
  from foundationpose_amd import bop
  from foundationpose_amd.tracking import MultiObjectTracker
  targets = [t for t in world['targets'] if t['im_id'] == 0]
  rows = bop.run_bop(world['root'], 'test', world['models'], world['refiner'], world['scorer'], targets=targets, iteration=2,
                     max_objects=max_objects)
  assert [(r['scene_id'], r['im_id'], r['obj_id']) for r in rows] == [(1, 0, 1), (1, 0, 1), (1, 0, 2), (1, 0, 3)]
  assert len(set(r['time'] for r in rows)) == 1 and rows[0]['time'] > 0                # one time per image
  # the direct call: estimators built anew with the same diameters, the arrays BopScene read, the same masks in the same order
  scene = world['scene']
  inst = bop.image_instances(scene, 0, targets)
  twins = bop.build_estimators(world['models'], [1, 2, 3], world['refiner'], world['scorer'], diameter='info')
  rgb, depth, K = scene.color(0), scene.depth(0), scene.K(0)
  assert rgb.dtype == np.uint8 and depth.dtype == np.float32 and 0.5 < depth[depth > 0].min() and depth.max() < 1.3
  step = 4 if max_objects is None else max_objects
  k = 0
  for g0 in range(0, len(inst), step):
    group = inst[g0:g0 + step]
    ests = [twins[o].instance() for o, _ in group]
    want = MultiObjectTracker(ests).register(rgb, depth, K, [m for _, m in group], iteration=2)
    for e, w in zip(ests, want):
      assert len(torch.unique(e.scores)) == len(e.scores), 'two hypotheses share a score; the order would be ambiguous'
      assert rows[k]['pose'].dtype == np.float32 and np.array_equal(rows[k]['pose'], w), f'row {k}: max diff {np.abs(rows[k]["pose"] - w).max():.3e}'
      assert rows[k]['score'] == float(e.scores[0])
      k += 1
  assert k == len(rows) == 4
  # the two instances of object 1 are two different poses
  assert np.abs(rows[0]['pose'] - rows[1]['pose']).max() > 0.01


def test_instance_shares_the_object_and_owns_its_pose(world):
  from foundationpose_amd import bop
  base = world['ests'][1]
  marker = torch.full((4, 4), 7.0, device='cuda')
  base.pose_last = marker
  twin = base.instance()
  assert twin is not base and twin.pose_last is None and twin.poses is None and twin.scores is None and twin.best_id is None
  assert twin.mesh_tensors['pos'].data_ptr() == base.mesh_tensors['pos'].data_ptr() and twin.mesh_tensors is base.mesh_tensors
  assert twin.rot_grid.data_ptr() == base.rot_grid.data_ptr() and twin.refiner is base.refiner and twin.scorer is base.scorer
  assert twin.diameter == base.diameter and twin._track_ws == {} and twin._track_ws is not base._track_ws
  scene = world['scene']
  mask = bop.image_instances(scene, 0, [t for t in world['targets'] if t['im_id'] == 0])[0][1]
  pose = twin.register(scene.K(0), scene.color(0), scene.depth(0), mask, iteration=1)
  assert pose.shape == (4, 4) and twin.pose_last is not None and base.pose_last is marker
  base.pose_last = None


def test_evaluation_of_known_errors_through_the_whole_chain(world, tmp_path):
  """Image 1: four distinct objects without symmetry, one instance each.  The results file holds the ground truth with instance k moved
  along the camera x axis by SHIFTS[k] x its diameter.  A pure translation moves every vertex by the same vector, so MSSD is that length:
  against BOP19_MSSD_THETAS = 0.05 .. 0.5 the instances are correct at 10, 8, 4 and 0 of the ten thresholds - AR_MSSD = 22 / 40."""
  from foundationpose_amd import bop
  from foundationpose_amd import Utils as U
  models, scene = world['models'], world['scene']
  targets = [t for t in world['targets'] if t['im_id'] == 1]
  gts = scene.gt(1)
  rows = []
  for k, g in enumerate(gts):
    pose = g['pose'].copy()
    pose[0, 3] += SHIFTS[k] * models.diameter(g['obj_id'])
    rows.append(dict(scene_id=1, im_id=1, obj_id=g['obj_id'], score=0.9 - 0.1 * k, pose=pose, time=0.5))
  path = str(tmp_path / 'known.csv')
  bop.write_results(path, rows)
  got = bop.evaluate_results(world['root'], 'test', models, path, targets=targets)
  assert got['n_targets'] == 4 and got['n_estimates'] == 4
  assert np.array_equal(got['recalls']['mssd'] * 4, [1, 1, 2, 2, 2, 2, 3, 3, 3, 3])
  assert got['AR_MSSD'] == 22 / 40
  # one instance per object in this image: the recalls are Utils.bop_average_recall of the paired errors
  back = bop.read_results(path)
  depth, K = scene.depth(1), scene.K(1)
  e_mssd, e_mspd, e_vsd, diam = [], [], [], []
  for r, g in zip(back, gts):
    o = g['obj_id']
    e = U.bop_pose_errors(r['pose'][None], g['pose'], models.mesh(o).vertices, K=K, symmetry_tfs=models.symmetry_tfs(o))
    e_mssd.append(float(e['mssd'][0])), e_mspd.append(float(e['mspd'][0])), diam.append(models.diameter(o))
    e_vsd.append(U.vsd_errors(r['pose'][None], g['pose'], depth, K, mesh=models.mesh(o), diameter=models.diameter(o))[0].cpu().numpy())
  for k in range(4):
    print(f'instance {k}: mssd / d = {e_mssd[k] / diam[k]:.6f} (shift {SHIFTS[k]}), mspd = {e_mspd[k]:.3f} px, vsd = {np.round(e_vsd[k], 3)}')
    assert abs(e_mssd[k] / diam[k] - SHIFTS[k]) < 1e-4
  want = U.bop_average_recall(e_vsd=np.stack(e_vsd), e_mssd=np.array(e_mssd), e_mspd=np.array(e_mspd), diameter=np.array(diam), image_width=W)
  for key in ('AR_VSD', 'AR_MSSD', 'AR_MSPD', 'AR'):
    assert got[key] == want[key], key
  assert got['per_object'][1]['AR_MSSD'] == 1.0 and got['per_object'][4]['AR_MSSD'] == 0.0
  # without row 0 every recall is lower by that row's share: the thresholds it met, over all thresholds x the four targets
  less = bop.evaluate_results(world['root'], 'test', models, back[1:], targets=targets)
  share = dict(AR_MSSD=(e_mssd[0] < U.BOP19_MSSD_THETAS * diam[0]).sum() / 40.0,
               AR_MSPD=(e_mspd[0] < U.BOP19_MSPD_THETAS * (W / 640.0)).sum() / 40.0,
               AR_VSD=(e_vsd[0][:, None] < U.BOP19_VSD_THETAS[None]).sum() / 400.0)
  assert less['n_targets'] == 4 and less['n_estimates'] == 3 and share['AR_MSSD'] == 0.25 and share['AR_MSPD'] == 0.25 and share['AR_VSD'] > 0
  for key, s in share.items():
    assert abs(less[key] - (got[key] - s)) < 1e-12, key


def test_run_bop_results_can_be_written_and_evaluated(world, tmp_path):
  """The whole loop as a user runs it.  With seeded random weights the poses are far from the ground truth, so the recall is near zero
  and is NOT asserted: the call runs, keeps one row per target instance and returns the keys."""
  from foundationpose_amd import bop
  rows = bop.run_bop(world['root'], 'test', world['models'], world['refiner'], world['scorer'], iteration=1, estimators=world['ests'])
  assert [(r['im_id'], r['obj_id']) for r in rows] == [(0, 1), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (1, 4)]
  path = str(tmp_path / 'run.csv')
  bop.write_results(path, rows)
  res = bop.evaluate_results(world['root'], 'test', world['models'], path)
  assert res['n_targets'] == 8 and res['n_estimates'] == 8
  assert set(res) >= {'AR', 'AR_VSD', 'AR_MSSD', 'AR_MSPD', 'per_object', 'recalls'} and sorted(res['per_object']) == [1, 2, 3, 4]
  assert all(0.0 <= res[k] <= 1.0 for k in ('AR', 'AR_VSD', 'AR_MSSD', 'AR_MSPD'))
