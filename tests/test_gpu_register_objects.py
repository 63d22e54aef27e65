"""GPU: FoundationPose.register for several objects of one frame in one call (tracking.MultiObjectTracker.register, fp_register_objects).

The yardstick throughout is the per-object FoundationPose.register() run on twin estimators (same mesh tensors, refiner, scorer, rotation
grid) on the same frame: the one call must equal it bit for bit - returned poses, sorted hypotheses, scores, best_id, pose_last - for
masks and for a label image, for rotation grids of different lengths, next to degenerate objects, beyond one network pass, and the tracker
must continue from it.  The pieces (mask reductions, hypothesis sets) are checked through their own exports."""
import copy
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu
H, W = 480, 640
SCORE_GAIN = 3.0e4


def _estimator(mesh, refiner, scorer, symmetry_tfs=None):
  from foundationpose_amd.estimater import FoundationPose
  np.random.seed(0)
  return FoundationPose(model_pts=mesh.vertices, model_normals=mesh.vertex_normals, mesh=mesh, refiner=refiner, scorer=scorer, symmetry_tfs=symmetry_tfs)


def _instance(est):
  """Another instance of est's part: the same mesh tensors and rotation grid, its own pose state."""
  e = copy.copy(est)
  e._track_ws = {}
  e.pose_last = e.poses = e.scores = e.best_id = None
  return e


def _pose(t, rot_seed):
  from foundationpose_amd import synthetic as S
  p = np.eye(4, dtype=np.float32)
  p[:3, :3] = S.random_rotation(np.random.RandomState(rot_seed))
  p[:3, 3] = t
  return p


def _frame(ests, poses, seed=0):
  """RGB-D frame z-composited from the HIP renders of every estimator's centred mesh at its pose, over a background plane at 1.2 m:
  numpy (rgb uint8 (H,W,3), depth float32 (H,W), owner int32 (H,W): index of the object visible at a pixel, -1 = background)."""
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


GT = [((-0.07, -0.04, 0.75), 1), ((0.07, -0.03, 0.80), 2), ((0.0, 0.07, 0.70), 3), ((0.09, 0.08, 0.85), 4), ((-0.10, 0.09, 0.90), 5)]


@pytest.fixture(scope='module')
def world():
  """One refiner and one scorer; estimators of three distinct meshes, a second instance of mesh 0 and one of mesh 1 (five objects), an
  estimator of mesh 1 with a 2-fold symmetry axis (a shorter rotation grid); the five-object frame and the objects' visible pixels."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.config import REFINE_DEFAULT, SCORE_DEFAULT
  from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
  from foundationpose_amd.predict_score import ScorePredictor
  refiner = PoseRefinePredictor(state_dict=S.make_refine_state_dict(cases.REFINE_SEED, head_gain=cases.GAIN_CHAIN), cfg=REFINE_DEFAULT)
  # The seeded scorer's logits of one registration lie within 1e-3 of each other: at scores = logit + 100 that is some hundred float32
  # values for 252 hypotheses, so scores tie and register()'s (unstable) argsort has no unique answer.  The output layer of this file's
  # scorer is scaled, and its bias moved, so that the scores of a registration spread over tens of units around 100.
  ssd = S.make_score_state_dict(cases.SCORE_SEED)
  ssd['linear.weight'] = ssd['linear.weight'] * SCORE_GAIN
  ssd['linear.bias'] = ssd['linear.bias'] * SCORE_GAIN - SCORE_GAIN * 0.0795
  scorer = ScorePredictor(state_dict=ssd, cfg=SCORE_DEFAULT)
  meshes = [S.make_mustard_mesh(seed=0), S.make_mustard_mesh(seed=1, n_theta=80, n_z=70), S.make_mustard_mesh(seed=2, n_theta=64, n_z=60)]
  base = [_estimator(m, refiner, scorer) for m in meshes]
  ests = base + [_instance(base[0]), _instance(base[1])]
  half_turn = np.stack([np.eye(4), np.diag([-1.0, -1.0, 1.0, 1.0])])
  sym = _estimator(meshes[1], refiner, scorer, symmetry_tfs=half_turn)
  gt = [_pose(t, s) for t, s in GT]
  rgb, depth, owner = _frame(ests[:4], gt[:4])
  return dict(refiner=refiner, scorer=scorer, ests=ests, sym=sym, gt=gt, rgb=rgb, depth=depth, owner=owner,
              masks=[owner == o for o in range(4)])


def _assert_equals_register(tracker_ests, rgb, depth, masks, got, iteration, skip=()):
  """Every object of the one call against register() on a twin estimator: returned pose, poses, scores, best_id, pose_last."""
  from foundationpose_amd import synthetic as S
  for o, e in enumerate(tracker_ests):
    if o in skip:
      continue
    twin = _instance(e)
    want = twin.register(S.YCB_K, rgb, depth, masks[o], iteration=iteration)
    assert len(torch.unique(twin.scores)) == len(twin.scores), f'object {o}: two hypotheses share a score; the order would be ambiguous'
    assert want.dtype == np.float32 and np.array_equal(got[o], want), f'object {o}: max diff {np.abs(got[o] - want).max():.3e}'
    assert torch.equal(e.poses, twin.poses), f'object {o}: poses differ by {float((e.poses - twin.poses).abs().max()):.3e}'
    assert torch.equal(e.scores, twin.scores), f'object {o}: scores differ by {float((e.scores - twin.scores).abs().max()):.3e}'
    assert torch.equal(e.best_id, twin.best_id) and e.best_id.shape == twin.best_id.shape
    assert torch.equal(e.pose_last, twin.pose_last) and e.pose_last.shape == twin.pose_last.shape
    assert (e.H, e.W) == (twin.H, twin.W) and e.K is twin.K and e.ob_mask is masks[o]


@pytest.mark.parametrize('iteration', [5, 2])
def test_four_objects_equal_register_bit_for_bit(world, iteration):
  """Three distinct meshes and a second instance of mesh 0 in one 480 x 640 frame, masks = each object's visible pixels."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  ests = [_instance(e) for e in world['ests'][:4]]
  got = MultiObjectTracker(ests).register(world['rgb'], world['depth'], S.YCB_K, world['masks'], iteration=iteration)
  assert got.shape == (4, 4, 4) and got.dtype == np.float32
  _assert_equals_register(ests, world['rgb'], world['depth'], world['masks'], got, iteration)


def test_rotation_grids_of_different_lengths(world):
  """An estimator with a 2-fold symmetry axis (a clustered, shorter rotation grid) between full-grid ones."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  sym = _instance(world['sym'])
  assert 2 < len(sym.rot_grid) < 252 == len(world['ests'][0].rot_grid)
  ests = [_instance(world['ests'][0]), sym, _instance(world['ests'][2])]
  got = MultiObjectTracker(ests).register(world['rgb'], world['depth'], S.YCB_K, world['masks'][:3], iteration=2)
  _assert_equals_register(ests, world['rgb'], world['depth'], world['masks'][:3], got, 2)


def test_label_image_equals_mask_list_and_masks_may_overlap(world):
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  rgb, depth, masks = world['rgb'], world['depth'], world['masks']
  a, b = [_instance(e) for e in world['ests'][:4]], [_instance(e) for e in world['ests'][:4]]
  from_masks = MultiObjectTracker(a).register(rgb, depth, S.YCB_K, masks, iteration=2)
  ids = [7, 3, 11, 5]
  image = np.zeros((H, W), dtype=np.int32)
  for o, m in enumerate(masks):
    image[m] = ids[o]
  from_labels = MultiObjectTracker(b).register(rgb, depth, S.YCB_K, image, iteration=2, labels=ids)
  assert np.array_equal(from_masks, from_labels)
  for x, y in zip(a, b):
    assert torch.equal(x.poses, y.poses) and torch.equal(x.scores, y.scores) and torch.equal(x.best_id, y.best_id)
    assert np.array_equal(y.ob_mask, x.ob_mask)
  # device tensors give the same
  c = [_instance(e) for e in world['ests'][:4]]
  on_dev = MultiObjectTracker(c).register(torch.as_tensor(rgb, device='cuda'), torch.as_tensor(depth, device='cuda'), S.YCB_K,
                                          torch.as_tensor(image, device='cuda'), iteration=2, labels=ids)
  assert np.array_equal(on_dev, from_masks)
  # overlapping masks (object 1's mask also covers object 0's pixels, as uint8 255): each object sees its own mask
  over = [masks[0], (masks[0] | masks[1]).astype(np.uint8) * 255]
  ests = [_instance(e) for e in world['ests'][:2]]
  got = MultiObjectTracker(ests).register(rgb, depth, S.YCB_K, over, iteration=1)
  _assert_equals_register(ests, rgb, depth, over, got, 1)


def test_degenerate_objects(world):
  """An empty mask and a mask of 3 usable pixels: eye(4) with register()'s fallback translation, those estimators untouched, the others
  registered as usual.  All objects degenerate: nothing runs."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  rgb, depth = world['rgb'], world['depth']
  masks = list(world['masks'])
  masks[1] = np.zeros((H, W), dtype=bool)
  three = np.zeros((H, W), dtype=bool)
  rows, cols = np.nonzero(world['masks'][2])
  mid = len(rows) // 2
  three[rows[mid], cols[mid]:cols[mid] + 3] = True
  masks[2] = three
  ests = [_instance(e) for e in world['ests'][:4]]
  marker = torch.full((4, 4), 7.0, device='cuda')
  ests[1].pose_last, ests[2].pose_last = marker, marker
  got = MultiObjectTracker(ests).register(rgb, depth, S.YCB_K, masks, iteration=2)
  for o in (1, 2):
    twin = _instance(world['ests'][o])
    want = twin.register(S.YCB_K, rgb, depth, masks[o], iteration=2)
    assert want.dtype == np.float64 and twin.pose_last is None                      # (register()'s fallback)
    assert np.array_equal(got[o], want.astype(np.float32))
    assert np.array_equal(got[o, :3, :3], np.eye(3)) and ests[o].pose_last is marker and ests[o].poses is None
  assert np.array_equal(got[1, :3, 3], np.zeros(3)) and np.abs(got[2, :3, 3]).max() > 0.05
  _assert_equals_register(ests, rgb, depth, masks, got, 2, skip=(1, 2))
  ctx = world['refiner'].ctx
  ctx.prof_reset()
  ctx.prof_enable(2)
  none = MultiObjectTracker([_instance(e) for e in world['ests'][:2]]).register(rgb, depth, S.YCB_K, [masks[1], masks[2]], iteration=2)
  torch.cuda.synchronize()
  ctx.prof_enable(False)
  launches = {c: ctx.prof_read(c)['launches'] for c in ('mask_stats', 'render', 'crop', 'linear', 'attention')}
  ctx.prof_reset()
  assert launches == dict(mask_stats=1, render=0, crop=0, linear=0, attention=0), launches
  assert np.array_equal(none[0], got[1]) and np.array_equal(none[1], got[2])


def _special_masks(world, depth_h):
  """Masks with an odd and an even count of USABLE pixels (the prelude's erosion zeroes some depths inside a mask), one pixel, none, all."""
  m = world['masks'][0]
  rows, cols = np.nonzero(m & (depth_h >= 0.001))
  odd = m.copy()
  if len(rows) % 2 == 0:
    odd[rows[0], cols[0]] = False
  even = odd.copy()
  even[rows[-1], cols[-1]] = False
  one = np.zeros((H, W), dtype=bool)
  one[rows[len(rows) // 2], cols[len(rows) // 2]] = True
  return dict(odd=odd, even=even, one=one, empty=np.zeros((H, W), dtype=bool), full=np.ones((H, W), dtype=bool))


def test_mask_reductions_of_all_objects_in_one_launch(world):
  """fp_mask_depth_stats_objects against fp_mask_depth_stats per mask, and the median against np.median of the same float32 values."""
  import foundationpose_amd.Utils as U
  depth = U.bilateral_filter_depth(U.erode_depth(torch.as_tensor(world['depth'], device='cuda'), radius=2, device='cuda'), radius=2, device='cuda')
  depth_h = depth.cpu().numpy()
  special = _special_masks(world, depth_h)
  groups = [world['masks'], [special[k] for k in ('odd', 'even', 'one', 'empty', 'full')] + [world['masks'][3].astype(np.uint8) * 200]]
  for masks in groups:
    got = U.mask_depth_stats_objects(depth, masks)
    assert len(got) == len(masks)
    for m, g in zip(masks, got):
      want = U.mask_depth_stats(depth, m)
      assert g == want and type(g['median']) is type(want['median']), (g, want)
      usable = depth_h[(m != 0) & (depth_h >= 0.001)]
      assert g['n_usable'] == len(usable) and g['n_mask'] == int((m != 0).sum())
      if len(usable):
        assert g['median'] == np.median(usable) and np.median(usable).dtype == np.float32
  n_odd, n_even = (int(((special[k] != 0) & (depth_h >= 0.001)).sum()) for k in ('odd', 'even'))
  assert n_odd % 2 == 1 and n_even % 2 == 0 and n_even > 0
  # the same objects as one label image (the special masks overlap, the scene's do not)
  image = np.full((H, W), -5, dtype=np.int32)
  ids = [40, -1, 0, 9]
  for o, m in enumerate(world['masks']):
    image[m] = ids[o]
  by_label = U.mask_depth_stats_objects(depth, image, labels=ids + [12345])
  assert by_label[:4] == U.mask_depth_stats_objects(depth, world['masks'])
  assert by_label[4] == U.mask_depth_stats(depth, np.zeros((H, W), dtype=bool))


def test_hypothesis_sets_equal_generate_random_pose_hypo(world):
  import foundationpose_amd.Utils as U
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import registration_hypotheses
  depth = U.bilateral_filter_depth(U.erode_depth(torch.as_tensor(world['depth'], device='cuda'), radius=2, device='cuda'), radius=2, device='cuda')
  ests = [world['ests'][0], world['sym'], world['ests'][2], world['ests'][3]]
  stats = U.mask_depth_stats_objects(depth, world['masks'])
  got = registration_hypotheses([e.rot_grid for e in ests], stats, S.YCB_K)
  want = torch.cat([e.generate_random_pose_hypo(K=S.YCB_K, rgb=None, depth=depth, mask=m) for e, m in zip(ests, world['masks'])], 0)
  assert got.shape == want.shape and torch.equal(got, want)
  assert len(torch.unique(want[:, :3, 3], dim=0)) == 4                  # (one translation per object)


def test_track_continues_from_register(world):
  """tracker.register then tracker.track on the next frame == four register() calls then tracker.track on a second tracker."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  rgb, depth, masks = world['rgb'], world['depth'], world['masks']
  moved = [p.copy() for p in world['gt'][:4]]
  for o, p in enumerate(moved):
    p[:3, 3] += np.array([0.002, -0.001, 0.003], dtype=np.float32) * (o + 1) / 2
  rgb2, depth2, _ = _frame(world['ests'][:4], moved, seed=1)
  a, b = [_instance(e) for e in world['ests'][:4]], [_instance(e) for e in world['ests'][:4]]
  ta, tb = MultiObjectTracker(a), MultiObjectTracker(b)
  first = ta.register(rgb, depth, S.YCB_K, masks, iteration=2)
  got = ta.track(rgb2, depth2, S.YCB_K, iteration=2)
  for o, e in enumerate(b):
    assert np.array_equal(e.register(S.YCB_K, rgb, depth, masks[o], iteration=2), first[o])
  want = tb.track(rgb2, depth2, S.YCB_K, iteration=2)
  assert np.array_equal(got, want) and not np.array_equal(got, first)


def test_five_objects_are_cut_into_passes_at_object_boundaries(world):
  """5 x 252 = 1260 hypotheses exceed one network pass of 1008: four objects in the first pass, the fifth in a second one."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  src = world['ests'][:5]
  rgb, depth, owner = _frame(src, world['gt'])
  masks = [owner == o for o in range(5)]
  assert all(m.sum() > 500 for m in masks) and sum(len(e.rot_grid) for e in src) == 1260
  ests = [_instance(e) for e in src]
  got = MultiObjectTracker(ests).register(rgb, depth, S.YCB_K, masks, iteration=2)
  _assert_equals_register(ests, rgb, depth, masks, got, 2)
  # a smaller pass size cuts elsewhere and changes nothing
  again = [_instance(e) for e in src]
  assert np.array_equal(MultiObjectTracker(again).register(rgb, depth, S.YCB_K, masks, iteration=2, max_pass_hyp=504), got)
  for x, y in zip(ests, again):
    assert torch.equal(x.poses, y.poses) and torch.equal(x.scores, y.scores)


def test_refusals(world):
  from foundationpose_amd import _lib
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  rgb, depth, masks = world['rgb'], world['depth'], world['masks']
  ests = [_instance(e) for e in world['ests'][:2]]
  tracker = MultiObjectTracker(ests)
  image = np.zeros((H, W), dtype=np.int32)
  for kw, msg in ((dict(masks=masks[:3]), '3 masks for 2 objects'), (dict(masks=[masks[0], masks[1][:, :-1]]), 'shapes differ'),
                  (dict(masks=image), 'needs labels='), (dict(masks=masks[:2], labels=[1, 2]), 'label image, not with a list'),
                  (dict(masks=image, labels=[4, 4]), 'repeated'), (dict(masks=image, labels=[1, 2, 3]), '3 labels for 2 objects'),
                  (dict(masks=image[:-2], labels=[1, 2]), 'shapes differ')):
    with pytest.raises(ValueError, match=msg):
      tracker.register(rgb, depth, S.YCB_K, iteration=1, **kw)
  other = _instance(world['ests'][1])
  other.scorer = types.SimpleNamespace(ctx=ests[0].scorer.ctx, model=types.SimpleNamespace(handle=ctypes.c_void_p(1)), cfg=ests[0].scorer.cfg)
  with pytest.raises(ValueError, match='scorer'):
    MultiObjectTracker([ests[0], other]).register(rgb, depth, S.YCB_K, masks[:2], iteration=1)
  assert all(e.pose_last is None for e in ests)                          # (a refused call registers nothing)
  # the C-ABI
  ctx = world['refiner'].ctx
  a = _lib.FpRegisterObjectsArgs()
  a.struct_size = ctypes.sizeof(a) - 8
  with pytest.raises(_lib.FoundationPoseAmdError, match='struct_size'):
    _lib.check(_lib.lib().fp_register_objects(ctx.handle, ctypes.byref(a), _lib.stream_ptr()))
  a.struct_size = ctypes.sizeof(a)
  with pytest.raises(_lib.FoundationPoseAmdError, match='null field'):
    _lib.check(_lib.lib().fp_register_objects(ctx.handle, ctypes.byref(a), _lib.stream_ptr()))
  st, med = (ctypes.c_int32 * 6)(), (ctypes.c_float * 1)()
  d = torch.ones((H, W), device='cuda')
  with pytest.raises(_lib.FoundationPoseAmdError, match='n_obj = 9'):
    _lib.check(_lib.lib().fp_mask_depth_stats_objects(ctx.handle, _lib.ptr(d), None, _lib.ptr(d), st, 9, H, W, 0.001, st, med, _lib.stream_ptr()))


def test_one_prelude_and_one_mask_reduction_per_call(world):
  """Profiled: one depth prelude and one mask-reduction launch whatever the number of objects, and no more render / crop / network
  launches than predict_multi (`iteration` passes) plus extract_features_multi issue for the same objects."""
  import foundationpose_amd.Utils as U
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  rgb, depth, masks = world['rgb'], world['depth'], world['masks']
  ctx = world['refiner'].ctx
  classes = ('prelude', 'mask_stats', 'render', 'crop', 'conv3x3_halo', 'linear', 'attention')

  def profiled(fn):
    torch.cuda.synchronize()
    ctx.prof_reset()
    ctx.prof_enable(2)
    fn()
    torch.cuda.synchronize()
    ctx.prof_enable(False)
    counts = {c: ctx.prof_read(c)['launches'] for c in classes}
    ctx.prof_reset()
    return counts
  it = 2
  seen = {}
  for n in (1, 4):
    ests = [_instance(e) for e in world['ests'][:n]]
    seen[n] = profiled(lambda: MultiObjectTracker(ests).register(rgb, depth, S.YCB_K, masks[:n], iteration=it))
    assert seen[n]['prelude'] == 1 and seen[n]['mask_stats'] == 1, seen[n]
  d = U.bilateral_filter_depth(U.erode_depth(torch.as_tensor(depth, device='cuda'), radius=2, device='cuda'), radius=2, device='cuda')
  xyz = U.depth2xyzmap(d, S.YCB_K)
  rgb_f = torch.as_tensor(rgb, device='cuda').float()
  objs = [dict(rgb=rgb_f, depth=d, xyz_map=xyz, K=S.YCB_K, mesh_tensors=e.mesh_tensors, mesh_diameter=e.diameter, ob_in_cams=e.rot_grid,
               shared_translation=True) for e in world['ests'][:4]]

  def reference():
    refined = world['refiner'].predict_multi(objs, iteration=it)
    offs = np.cumsum([0] + [len(o['ob_in_cams']) for o in objs])
    world['scorer'].extract_features_multi([dict(o, ob_in_cams=refined[a:b]) for o, a, b in zip(objs, offs[:-1], offs[1:])])
  want = profiled(reference)
  print(f'launches: register of 1 object {seen[1]}, of 4 objects {seen[4]}, predict_multi + extract_features_multi of 4 objects {want}')
  for c in ('render', 'crop', 'conv3x3_halo', 'linear', 'attention'):
    assert seen[4][c] <= want[c], (c, seen[4], want)
