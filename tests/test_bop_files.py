"""CPU: foundationpose_amd.bop on a small BOP-format tree written at run time - models, scenes, targets, the results CSV - and the BOP-19
matching rule on hand-made error matrices."""
import json
import os

import numpy as np
import pytest

from foundationpose_amd import bop
from foundationpose_amd import synthetic as S
from foundationpose_amd import Utils as U
from tests import bop_tree

H, W = 48, 64
K1 = np.array([[600.0, 0.0, 31.5], [0.0, 601.0, 23.5], [0.0, 0.0, 1.0]])
K2 = np.array([[610.5, 0.0, 30.25], [0.0, 611.25, 22.75], [0.0, 0.0, 1.0]])
HALF_TURN_MM = [-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 12.0, 0, 0, 0, 1]      # about z, with a translation of 12 mm along it


def _pose(seed, t):
  p = np.eye(4)
  p[:3, :3] = S.random_rotation(np.random.RandomState(seed))
  p[:3, 3] = t
  return p


def _rect(r0, r1, c0, c1):
  m = np.zeros((H, W), dtype=bool)
  m[r0:r1, c0:c1] = True
  return m


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
  root = tmp_path_factory.mktemp('bop')
  meshes = {1: S.make_mustard_mesh(seed=0, n_theta=16, n_z=12), 2: S.make_mustard_mesh(seed=1, n_theta=12, n_z=10)}
  bop_tree.write_models(root, {1: (meshes[1], dict(symmetries_discrete=[HALF_TURN_MM])),
                               2: (meshes[2], dict(symmetries_continuous=[dict(axis=[0, 0, 1], offset=[0, 0, 0])]))})
  rs = np.random.RandomState(0)
  depth_png = [rs.randint(300, 60000, (H, W)).astype(np.uint16) for _ in range(2)]
  depth_png[0][0, :4] = [0, 5, 9, 10]             # x 0.1 mm: 0, 0.5 mm, 0.9 mm (all dropped), 1.0 mm (kept)
  depth_png[1][0, :4] = [0, 1, 2, 3000]           # x 1.0 mm: 1 mm and 2 mm are kept, 0 is missing
  images = [
    dict(im_id=3, K=K1, depth_scale=0.1, rgb=rs.randint(0, 256, (H, W, 3)).astype(np.uint8), depth_png=depth_png[0],
         gt=[dict(obj_id=1, pose=_pose(1, (0.01, 0.02, 0.6)), mask=_rect(2, 20, 3, 30), visib_fract=0.9),
             dict(obj_id=2, pose=_pose(2, (-0.05, 0.0, 0.7)), mask=_rect(10, 40, 35, 60), visib_fract=0.5),
             dict(obj_id=1, pose=_pose(3, (0.06, -0.03, 0.8)), mask=_rect(25, 44, 5, 25), visib_fract=0.1)]),
    dict(im_id=7, K=K2, depth_scale=1.0, rgb=rs.randint(0, 256, (H, W, 3)).astype(np.uint8), depth_png=depth_png[1],
         gt=[dict(obj_id=2, pose=_pose(4, (0.0, 0.0, 1.1)), mask=_rect(5, 30, 5, 30), visib_fract=1.0),
             dict(obj_id=1, pose=_pose(5, (0.1, 0.1, 1.4)), mask=None, visib_fract=0.05)])]
  scene_dir = bop_tree.write_scene(root, images)
  targets = [dict(im_id=3, inst_count=2, obj_id=1, scene_id=1), dict(im_id=3, inst_count=1, obj_id=2, scene_id=1),
             dict(im_id=7, inst_count=1, obj_id=2, scene_id=1)]
  bop_tree.write_targets(root, targets)
  return dict(root=str(root), scene_dir=scene_dir, meshes=meshes, images=images, targets=targets)


def test_models(tree):
  models = bop.BopModels(os.path.join(tree['root'], 'models'))
  assert models.obj_ids == [1, 2]
  for o in (1, 2):
    want = (tree['meshes'][o].vertices * 1000.0).astype(np.float32).astype(np.float64) * 1e-3        # the file holds float32 millimetres
    mesh = models.mesh(o)
    assert np.array_equal(mesh.vertices, want) and np.array_equal(mesh.faces, tree['meshes'][o].faces)
    assert models.mesh(o) is mesh
    assert models.diameter(o) == models.info(o)['diameter'] / 1e3
    assert abs(models.diameter(o) - bop_tree.exact_diameter(want)) < 1e-9
  sym = models.symmetry_tfs(1)
  assert sym.shape == (2, 4, 4) and np.array_equal(sym[0], np.eye(4))
  assert np.array_equal(sym[1], np.array(HALF_TURN_MM, dtype=np.float64).reshape(4, 4) * np.array([[1, 1, 1, 1e-3]] * 3 + [[1, 1, 1, 1]]))
  assert np.array_equal(sym, U.symmetry_tfs_from_info(models.info(1)))
  assert models.symmetry_tfs(2).shape == (1 + 72, 4, 4)                     # the identity, then every 5 degrees about z


def test_scene(tree):
  scene = bop.BopScene(tree['scene_dir'])
  assert scene.im_ids == [3, 7]
  for im in tree['images']:
    i = im['im_id']
    assert np.array_equal(scene.K(i), im['K']) and scene.K(i).dtype == np.float64
    assert scene.depth_scale(i) == im['depth_scale']                        # per image: 0.1 and 1.0 in one scene
    color = scene.color(i)
    assert color.dtype == np.uint8 and np.array_equal(color, im['rgb'])
    want = (im['depth_png'].astype(np.float64) * 1e-3) * im['depth_scale']
    want[want < 0.001] = 0
    depth = scene.depth(i)
    assert depth.dtype == np.float32 and np.array_equal(depth, want.astype(np.float32))
    gt = scene.gt(i)
    assert [g['obj_id'] for g in gt] == [e['obj_id'] for e in im['gt']] and [g['gt_id'] for g in gt] == list(range(len(gt)))
    for g, e in zip(gt, im['gt']):
      assert g['pose'].dtype == np.float64 and np.array_equal(g['pose'][:3, :3], e['pose'][:3, :3]) and np.array_equal(g['pose'][3], [0, 0, 0, 1])
      assert np.allclose(g['pose'][:3, 3], e['pose'][:3, 3], rtol=0, atol=1e-15)        # metres -> mm in the file -> metres
      m = scene.mask(i, g['gt_id'])
      assert (m is None) if e['mask'] is None else (m.dtype == bool and np.array_equal(m, e['mask']))
    assert [x['visib_fract'] for x in scene.gt_info(i)] == [e['visib_fract'] for e in im['gt']]
  assert list(scene.depth(3)[0, :4]) == [0.0, 0.0, 0.0, np.float32(10 * 1e-3 * 0.1)]
  assert list(scene.depth(7)[0, :4]) == [0.0, np.float32(0.001), np.float32(0.002), np.float32(3.0)]
  assert scene.counted(3) == [True, True, True] and scene.counted(7) == [True, False]
  assert scene.mask(7, 1) is None and scene.mask(3, 0, kind='mask') is None
  # beyond zfar: dropped
  near = bop.BopScene(tree['scene_dir'], zfar=2.5)
  d, full = near.depth(7), scene.depth(7)
  assert d[0, 3] == 0 and np.array_equal(d, np.where(full > 2.5, 0, full)) and (full > 2.5).any() and (d > 0).any()


def test_gray_scene_is_tiled_and_a_scene_without_gt_info_counts_everything(tmp_path):
  rs = np.random.RandomState(1)
  gray = rs.randint(0, 256, (H, W)).astype(np.uint8)
  im = dict(im_id=0, K=K1, depth_scale=1.0, rgb=gray, depth_png=np.full((H, W), 700, np.uint16),
            gt=[dict(obj_id=5, pose=np.eye(4), mask=_rect(0, 5, 0, 5), visib_fract=0.01), dict(obj_id=5, pose=np.eye(4), mask=_rect(5, 9, 0, 5))])
  d = bop_tree.write_scene(tmp_path, [im], split='val', scene_id=12, color_dir='gray', gt_info=False)
  scene = bop.BopScene(d)
  assert scene.im_ids == [0] and scene.gt_info(0) is None and scene.counted(0) == [True, True]
  color = scene.color(0)
  assert color.shape == (H, W, 3) and color.dtype == np.uint8 and all(np.array_equal(color[..., c], gray) for c in range(3))
  assert bop.targets_from_gt(tmp_path, 'val') == [dict(scene_id=12, im_id=0, obj_id=5, inst_count=2)]


def test_targets(tree):
  targets = bop.load_targets(os.path.join(tree['root'], 'test_targets_bop19.json'))
  assert targets == tree['targets']
  assert bop.targets_from_gt(tree['root'], 'test') == targets                 # (the instance seen to 5 % is no target)
  assert bop.targets_from_gt(tree['root'], 'test', visib_gt_min=0.0)[-1] == dict(scene_id=1, im_id=7, obj_id=2, inst_count=1)
  assert len(bop.targets_from_gt(tree['root'], 'test', visib_gt_min=0.0)) == 4
  assert bop.targets_from_gt(tree['root'], 'test', visib_gt_min=0.2)[0]['inst_count'] == 1


def test_image_instances(tree):
  scene = bop.BopScene(tree['scene_dir'])
  by_im = {3: tree['targets'][:2], 7: tree['targets'][2:]}
  inst = bop.image_instances(scene, 3, by_im[3])
  assert [o for o, _ in inst] == [1, 1, 2]
  assert np.array_equal(inst[0][1], tree['images'][0]['gt'][0]['mask']) and np.array_equal(inst[1][1], tree['images'][0]['gt'][2]['mask'])
  assert [o for o, _ in bop.image_instances(scene, 7, by_im[7])] == [2]
  # a target whose instance has no mask file yields nothing; a detector plugs in through a callable, best detections first
  assert bop.image_instances(scene, 7, [dict(scene_id=1, im_id=7, obj_id=1, inst_count=1)]) == []
  a, b, c = _rect(0, 4, 0, 4), _rect(4, 8, 0, 4), _rect(8, 12, 0, 4)
  det = lambda s, i: [(1, a, 0.2), (1, b, 0.9), (2, c, 0.5), (1, c, 0.5), (1, np.zeros((H, W), bool), 0.95)]
  got = bop.image_instances(scene, 3, by_im[3], det)
  assert [o for o, _ in got] == [1, 2] and np.array_equal(got[0][1], b) and np.array_equal(got[1][1], c)      # (the empty mask is dropped)


def test_results_csv_round_trip(tmp_path):
  rs = np.random.RandomState(5)
  rows = []
  for k in range(6):
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = S.random_rotation(rs).astype(np.float32)
    pose[:3, 3] = (rs.randn(3) * 0.3 + (0, 0, 0.8)).astype(np.float32)
    rows.append(dict(scene_id=1 + k // 3, im_id=k, obj_id=k % 2 + 1, score=float(np.float32(rs.rand() * 100)), pose=pose, time=0.25 + k // 3))
  path = str(tmp_path / 'est.csv')
  bop.write_results(path, rows)
  lines = open(path).read().splitlines()
  assert lines[0] == 'scene_id,im_id,obj_id,score,R,t,time' and len(lines) == 7
  f = lines[1].split(',')
  assert len(f) == 7 and (int(f[0]), int(f[1]), int(f[2])) == (1, 0, 1) and float(f[3]) == rows[0]['score'] and float(f[6]) == 0.25
  assert [float(x) for x in f[4].split()] == [float(x) for x in rows[0]['pose'][:3, :3].reshape(-1)]            # row-major, exact
  t_mm = [float(x) for x in f[5].split()]
  assert np.allclose(t_mm, rows[0]['pose'][:3, 3].astype(np.float64) * 1000.0, rtol=1e-15) and abs(t_mm[2]) > 100      # millimetres
  back = bop.read_results(path)
  assert len(back) == 6
  for a, b in zip(rows, back):
    assert (a['scene_id'], a['im_id'], a['obj_id'], a['score'], a['time']) == (b['scene_id'], b['im_id'], b['obj_id'], b['score'], b['time'])
    assert np.array_equal(b['pose'].astype(np.float32).view(np.uint32), a['pose'].view(np.uint32))              # bit for bit
  bop.write_results(path, [dict(scene_id=1, im_id=2, obj_id=3, score=1, pose=np.eye(4))])
  assert bop.read_results(path)[0]['time'] == -1.0                              # unknown time
  with open(path, 'w') as fh:
    fh.write('scene_id,im_id,obj_id,score,R,t\n')
  with pytest.raises(ValueError, match='first line'):
    bop.read_results(path)


# ---------------------------------------------------------------------------------------------- matching
TH = U.BOP19_MSSD_THETAS                     # 0.05 .. 0.5, x the diameter
D = 0.2


def _mssd_group(err_over_d, scores, inst_count, gt_counts=None, obj_id=1):
  return dict(obj_id=obj_id, inst_count=inst_count, scores=scores, mssd=np.asarray(err_over_d, dtype=np.float64) * D, diameter=D,
              gt_counts=gt_counts)


def _recalls(groups):
  return bop.match_and_recall(groups, errors=('mssd',))


def test_one_instance_per_target_equals_bop_average_recall():
  rs = np.random.RandomState(0)
  n = 40
  e_vsd, e_mssd, e_mspd = rs.rand(n, len(U.BOP19_VSD_TAUS)), rs.rand(n) * 0.12, rs.rand(n) * 60
  diam = rs.uniform(0.1, 0.3, n)
  groups = [dict(obj_id=1 + k % 3, inst_count=1, scores=[rs.rand()], vsd=e_vsd[k].reshape(1, 1, -1), mssd=[[e_mssd[k]]], mspd=[[e_mspd[k]]],
                 diameter=diam[k], image_width=800) for k in range(n)]
  groups += [dict(obj_id=2, inst_count=1, scores=[], gt_counts=[True], diameter=0.2) for _ in range(5)]       # five targets nobody estimated
  got = bop.match_and_recall(groups)
  want = U.bop_average_recall(e_vsd=e_vsd, e_mssd=e_mssd, e_mspd=e_mspd, diameter=diam, image_width=800, n_targets=n + 5)
  assert got['n_targets'] == n + 5
  for k in ('AR_VSD', 'AR_MSSD', 'AR_MSPD', 'AR'):
    assert got[k] == want[k], k
  assert 0.05 < got['AR'] < 0.95
  # per object: the same rule on that object's targets
  ids = np.array([1 + k % 3 for k in range(n)])
  for o in (1, 2, 3):
    sel = ids == o
    w = U.bop_average_recall(e_vsd=e_vsd[sel], e_mssd=e_mssd[sel], e_mspd=e_mspd[sel], diameter=diam[sel], image_width=800,
                             n_targets=int(sel.sum()) + (5 if o == 2 else 0))
    assert got['per_object'][o]['AR'] == w['AR'] and got['per_object'][o]['AR_VSD'] == w['AR_VSD']
  only = bop.match_and_recall(groups, errors=('mspd',))
  assert only['AR'] == only['AR_MSPD'] == want['AR_MSPD'] and 'AR_VSD' not in only


def test_greedy_matching_two_instances():
  """Two ground truths g0, g1 and two estimates; errors as fractions of the diameter.  Estimate A (score 0.9): 0.12 to g0, 0.22 to
  g1; estimate B (score 0.5): 0.17 to g0, 0.9 to g1.  By hand, per threshold theta (an estimate is within when error < theta):
    theta 0.05, 0.10   nobody within                                                    0 matches
    theta 0.15         A within g0 only -> takes g0; B within nothing                   1
    theta 0.20         A within g0 only -> takes g0; B within g0 only, taken            1
    theta 0.25 .. 0.5  A within both, prefers g0 (least error); B within g0 only, taken 1   <- the case of the rule
  Swapped (A: 0.22 to g0, 0.12 to g1): from 0.15 A takes g1; B takes g0 from 0.20:      0 0 1 2 2 2 2 2 2 2."""
  first = _recalls([_mssd_group([[0.12, 0.22], [0.17, 0.9]], [0.9, 0.5], 2)])
  assert first['n_targets'] == 2
  assert np.array_equal(first['recalls']['mssd'] * 2, [0, 0, 1, 1, 1, 1, 1, 1, 1, 1])
  assert first['AR_MSSD'] == np.mean(np.array([0, 0, 1, 1, 1, 1, 1, 1, 1, 1]) / 2)
  swapped = _recalls([_mssd_group([[0.22, 0.12], [0.17, 0.9]], [0.9, 0.5], 2)])
  assert np.array_equal(swapped['recalls']['mssd'] * 2, [0, 0, 1, 2, 2, 2, 2, 2, 2, 2])
  # the order of the rows does not matter, the scores do
  assert np.array_equal(_recalls([_mssd_group([[0.17, 0.9], [0.12, 0.22]], [0.5, 0.9], 2)])['recalls']['mssd'], first['recalls']['mssd'])
  # with the scores exchanged B goes first and takes g0; A then takes g1 from 0.25
  assert np.array_equal(_recalls([_mssd_group([[0.12, 0.22], [0.17, 0.9]], [0.5, 0.9], 2)])['recalls']['mssd'] * 2,
                        [0, 0, 1, 1, 2, 2, 2, 2, 2, 2])


def test_only_the_inst_count_best_scored_estimates_are_kept():
  """Three estimates for inst_count = 2: the lowest-scored is dropped although it alone is accurate."""
  got = _recalls([_mssd_group([[0.9, 0.9], [0.9, 0.9], [0.01, 0.9]], [0.8, 0.7, 0.1], 2)])
  assert got['n_targets'] == 2 and got['AR_MSSD'] == 0.0
  kept = _recalls([_mssd_group([[0.9, 0.9], [0.9, 0.9], [0.01, 0.9]], [0.8, 0.05, 0.1], 2)])
  assert kept['AR_MSSD'] == 0.5                           # now it is the second best: one of two targets at every threshold


def test_barely_visible_ground_truth_is_neither_matched_nor_counted():
  """g1 is seen to less than 10 %: the estimate that fits g1 only matches nothing, and n_targets is 1."""
  got = _recalls([_mssd_group([[0.9, 0.01]], [1.0], 1, gt_counts=[True, False])])
  assert got['n_targets'] == 1 and got['AR_MSSD'] == 0.0
  got = _recalls([_mssd_group([[0.01, 0.9]], [1.0], 1, gt_counts=[True, False])])
  assert got['n_targets'] == 1 and got['AR_MSSD'] == 1.0


def test_a_target_without_an_estimate_lowers_the_recall():
  hit = _mssd_group([[0.01]], [1.0], 1)
  assert _recalls([hit])['AR_MSSD'] == 1.0
  miss = dict(obj_id=2, inst_count=2, scores=[], gt_counts=[True, True, False], diameter=D)
  got = _recalls([hit, miss])
  assert got['n_targets'] == 3 and got['AR_MSSD'] == np.mean(np.full(10, 1 / 3))
  assert got['per_object'][1]['AR_MSSD'] == 1.0 and got['per_object'][2]['AR_MSSD'] == 0.0 and got['per_object'][2]['n_targets'] == 2
  with pytest.raises(ValueError):
    bop.match_and_recall([hit], errors=('add',))
