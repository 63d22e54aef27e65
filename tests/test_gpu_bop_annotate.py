"""GPU: a BOP tree that has ground-truth poses but neither masks nor scene_gt_info.json is annotated on the device
(bop.annotate_scene over Utils.scene_instances), read back through BopScene, and used: targets_from_gt counts by the computed
visib_fract, and image_instances(mask_source='gt_render') on the bare tree gives the masks 'gt_visib' gives on the annotated one.

The frame's depth is the z-composite of the rendered ground truth over a background plane at 1.2 m, quantised by the 16-bit PNG:
object 1 unoccluded, a second instance of it in front of object 2, object 2 partly behind that, object 3 behind the plane."""
import os

import numpy as np
import pytest
import torch

from tests import bop_tree

pytestmark = pytest.mark.gpu
H, W = 480, 640


def _pose(t, rot_seed):
  from foundationpose_amd import synthetic as S
  p = np.eye(4)
  p[:3, :3] = S.random_rotation(np.random.RandomState(rot_seed))
  p[:3, 3] = t
  return p


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
  from foundationpose_amd import bop
  from foundationpose_amd import synthetic as S
  from foundationpose_amd import Utils as U
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  root = tmp_path_factory.mktemp('bop_annotate')
  meshes = {1: S.make_mustard_mesh(seed=0), 2: S.make_mustard_mesh(seed=1, n_theta=80, n_z=70), 3: S.make_mustard_mesh(seed=2, n_theta=64, n_z=60)}
  models = bop.BopModels(bop_tree.write_models(root, {o: (m, {}) for o, m in meshes.items()}))
  centre = lambda o: (models.mesh(o).vertices.min(0) + models.mesh(o).vertices.max(0)) / 2

  def at(o, t, seed):                          # the model-frame pose that puts the model's centre at t
    p = _pose((0, 0, 0), seed)
    p[:3, 3] = np.asarray(t) - p[:3, :3] @ centre(o)
    return p
  # gt order: 0 unoccluded; 1 a twin of object 1 in front of 2; 2 object 2 partly behind it; 3 object 3 behind the plane
  gt = [dict(obj_id=1, pose=at(1, (-0.10, -0.05, 0.75), 1)), dict(obj_id=1, pose=at(1, (0.10, 0.02, 0.70), 2)),
        dict(obj_id=2, pose=at(2, (0.17, 0.02, 0.95), 3)), dict(obj_id=3, pose=at(3, (-0.05, 0.12, 1.6), 4))]
  tensors = {o: make_mesh_tensors(models.mesh(o)) for o in meshes}
  depth = torch.full((H, W), 1.2, device='cuda')
  for g in gt:
    _, d, _ = U.nvdiffrast_render(K=S.YCB_K, H=H, W=W, ob_in_cams=torch.as_tensor(g['pose'], dtype=torch.float, device='cuda').reshape(1, 4, 4),
                                  mesh_tensors=tensors[g['obj_id']])
    depth = torch.where((d[0] > 0) & (d[0] < depth), d[0], depth)
  images = [dict(im_id=0, K=S.YCB_K, depth_scale=0.1, rgb=np.zeros((H, W, 3), np.uint8), depth_png=np.round(depth.cpu().numpy() * 1e4).astype(np.uint16),
                 gt=[dict(g, mask=None) for g in gt])]
  bare = bop_tree.write_scene(root / 'bare', images, gt_info=False)
  full = bop_tree.write_scene(root / 'full', images, gt_info=False)
  for r in ('bare', 'full'):
    os.symlink(models.models_dir, os.path.join(str(root), r, 'models'))
  return dict(root=root, models=models, bare=bare, full=full, gt=gt, tensors=tensors)


def test_annotate_scene_writes_what_scene_instances_returns(tree):
  from foundationpose_amd import bop
  from foundationpose_amd import Utils as U
  t = tree
  before = bop.BopScene(t['full'])
  assert before.gt_info(0) is None and before.mask(0, 0) is None and not os.path.isdir(os.path.join(t['full'], 'mask'))
  assert [x['inst_count'] for x in bop.targets_from_gt(t['root'] / 'full', 'test')] == [2, 1, 1]          # every instance counts: nothing says otherwise
  info = bop.annotate_scene(t['full'], t['models'])
  scene = bop.BopScene(t['full'])
  gts = scene.gt(0)
  want = U.scene_instances(scene.K(0), H, W, [t['tensors'][g['obj_id']] for g in gts], np.stack([g['pose'] for g in gts]).astype(np.float32),
                           depth=scene.depth(0), occluders='depth', pad='bop', want=('mask', 'mask_visib', 'info'))
  assert list(info) == [0] and info[0] == want['info']
  assert scene.gt_info(0) == [{k: e[k] for k in U.SCENE_INFO_KEYS} for e in want['info']]
  for g in range(4):
    assert np.array_equal(scene.mask(0, g, 'mask'), want['mask'][g].cpu().numpy() > 0)
    assert np.array_equal(scene.mask(0, g, 'mask_visib'), want['mask_visib'][g].cpu().numpy() > 0)
  vf = [e['visib_fract'] for e in info[0]]
  print('visib_fract', vf)
  assert vf[0] == 1.0 and vf[1] == 1.0          # unoccluded and inside the frame: exactly 1
  assert vf[3] == 0.0 and info[0][3]['bbox_visib'] == [-1] * 4 and info[0][3]['px_count_all'] > 500          # behind the plane (no holes in this depth)
  assert 0.0 < vf[2] < 1.0                                        # partly behind the twin
  assert all(e['px_count_valid'] == e['px_count_all'] for e in info[0])
  # the hidden instance is no target any more
  assert scene.counted(0) == [True, True, vf[2] >= 0.1, False]
  after = bop.targets_from_gt(t['root'] / 'full', 'test')
  assert 3 not in [x['obj_id'] for x in after] and after[0] == dict(scene_id=1, im_id=0, obj_id=1, inst_count=2)
  # a second call leaves the files alone; overwrite=True rewrites them with the same content
  files = [os.path.join(t['full'], 'scene_gt_info.json')] + [os.path.join(t['full'], k, f'000000_{g:06d}.png') for k in ('mask', 'mask_visib') for g in range(4)]
  old = {f: (os.stat(f).st_mtime_ns, open(f, 'rb').read()) for f in files}
  for f in files:
    os.utime(f, ns=(1, 1))
  again = bop.annotate_scene(t['full'], t['models'])          # nothing is missing: the entries come back from the file
  assert again == {0: [{k: e[k] for k in U.SCENE_INFO_KEYS} for e in info[0]]}
  assert all(os.stat(f).st_mtime_ns == 1 for f in files)
  bop.annotate_scene(t['full'], t['models'], overwrite=True)
  assert all(os.stat(f).st_mtime_ns != 1 and open(f, 'rb').read() == old[f][1] for f in files)


def test_gt_render_equals_gt_visib_on_the_annotated_tree(tree):
  from foundationpose_amd import bop
  t = tree
  full, bare = bop.BopScene(t['full']), bop.BopScene(t['bare'])
  assert full.gt_info(0) is not None and bare.gt_info(0) is None and bare.mask(0, 0) is None
  targets = bop.targets_from_gt(t['root'] / 'full', 'test')
  want = bop.image_instances(full, 0, targets, mask_source='gt_visib')
  assert [o for o, _ in want][:2] == [1, 1] and 3 not in [o for o, _ in want] and all(m.any() for _, m in want)
  got = bop.image_instances(bare, 0, targets, mask_source='gt_render', models=t['models'])
  assert [o for o, _ in got] == [o for o, _ in want]
  for (_, a), (_, b) in zip(got, want):
    assert a.dtype == bool and np.array_equal(a, b)
  assert bop.image_instances(bare, 0, targets, mask_source='gt_visib') == []          # 'gt_visib' still drops what has no file
  assert not os.path.isdir(os.path.join(t['bare'], 'mask')) and not os.path.isfile(os.path.join(t['bare'], 'scene_gt_info.json'))
