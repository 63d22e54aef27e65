"""CPU: the host side of the scene-instance annotations: Utils.scene_info_rows on hand-made rows, the scene_gt_info.json writer read back
through BopScene, the arguments of scripts/bop_annotate.py, and image_instances' mask_source check."""
import importlib.util
import json
import os

import numpy as np
import pytest

from tests import bop_tree

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scene_info_rows():
  from foundationpose_amd import Utils as U
  from foundationpose_amd import _lib
  assert _lib.FP_SCENE_INFO_COLS == 12
  rows = np.array([[10, 5, 4, 8, -3, 2, 6, 9, 0, 2, 3, 5],                     # cut by the left border: bbox_obj starts at x = -3
                   [0, 0, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1],               # renders nowhere
                   [7, 7, 0, 7, 5, 5, 5, 11, -1, -1, -1, -1],                  # wholly hidden: a one-pixel-wide column of 7
                   [3, 0, 3, 3, -1, -1, 1, -1, -1, -1, 1, -1],                 # a box whose corner is legitimately -1 (padding): told by the count
                   [3, 1, 1, 3, 0, 0, 2, 0, 1, 0, 1, 0]], dtype=np.int32)
  info = U.scene_info_rows(rows)
  assert [sorted(e) for e in info] == [sorted(U.SCENE_INFO_KEYS + ('px_count_in_frame',))] * 5
  assert info[0] == dict(px_count_all=10, px_count_valid=5, px_count_visib=4, visib_fract=0.4, bbox_obj=[-3, 2, 10, 8], bbox_visib=[0, 2, 4, 4],
                         px_count_in_frame=8)
  assert info[1]['visib_fract'] == 0.0 and info[1]['bbox_obj'] == [-1] * 4 and info[1]['bbox_visib'] == [-1] * 4
  assert info[2]['visib_fract'] == 0.0 and info[2]['bbox_obj'] == [5, 5, 1, 7] and info[2]['bbox_visib'] == [-1] * 4
  assert info[3]['visib_fract'] == 1.0 and info[3]['bbox_obj'] == [-1, -1, 3, 1] and info[3]['bbox_visib'] == [-1, -1, 3, 1]
  assert info[4]['visib_fract'] == np.float64(1) / np.float64(3) and info[4]['bbox_visib'] == [1, 0, 1, 1]
  for e in info:                                                                # plain Python numbers: json takes them
    assert all(type(x) is int for k in ('bbox_obj', 'bbox_visib') for x in e[k]) and type(e['visib_fract']) is float
    assert type(e['px_count_all']) is int
  json.dumps(info)
  assert U.scene_info_rows(np.zeros((0, 12), np.int32)) == []
  for bad in (np.zeros((12,), np.int32), np.zeros((2, 11), np.int32)):
    with pytest.raises(ValueError, match='scene_info_rows takes'):
      U.scene_info_rows(bad)


def test_scene_pad_and_occluders():
  from foundationpose_amd import Utils as U
  assert U._scene_pad(0, 480, 640) == (0, 0) and U._scene_pad(16, 480, 640) == (16, 16)
  assert U._scene_pad((8, 4), 480, 640) == (8, 4) and U._scene_pad('bop', 480, 640) == (640, 480)
  with pytest.raises(ValueError, match='pad must be'):
    U._scene_pad('toolkit', 480, 640)
  assert U._scene_occluders(None, True) == 3 and U._scene_occluders(None, False) == 2
  assert U._scene_occluders('depth', True) == 1 and U._scene_occluders(('depth', 'instances'), True) == 3 and U._scene_occluders('both', True) == 3
  with pytest.raises(ValueError, match='unknown occluder'):
    U._scene_occluders('plane', True)
  assert U.BOP19_VSD_DELTA == 0.015


def _bare_scene(tmp_path):
  """A scene with ground truth but neither masks nor scene_gt_info.json"""
  pose = np.eye(4)
  pose[:3, 3] = [0.0, 0.0, 0.8]
  gt = [dict(obj_id=1, pose=pose, mask=None), dict(obj_id=2, pose=pose, mask=None)]
  images = [dict(im_id=i, K=np.array([[500.0, 0, 16], [0, 500.0, 12], [0, 0, 1]]), depth_scale=1.0, rgb=np.zeros((24, 32, 3), np.uint8),
                 depth_png=np.full((24, 32), 800, np.uint16), gt=gt) for i in (0, 3)]
  return bop_tree.write_scene(tmp_path, images, gt_info=False)


def test_gt_info_round_trip(tmp_path):
  from foundationpose_amd import bop
  from foundationpose_amd import Utils as U
  d = _bare_scene(tmp_path)
  assert bop.BopScene(d).gt_info(0) is None and bop.BopScene(d).counted(0) == [True, True]
  rows = {0: np.array([[100, 90, 100, 100, 2, 3, 11, 12, 2, 3, 11, 12], [200, 10, 15, 120, -8, 0, 11, 19, 0, 4, 2, 9]]),
          3: np.array([[100, 0, 0, 100, 2, 3, 11, 12, -1, -1, -1, -1], [0, 0, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1]])}
  info = {i: U.scene_info_rows(r) for i, r in rows.items()}
  bop.write_gt_info(d, info)
  scene = bop.BopScene(d)
  for i in (0, 3):
    back = scene.gt_info(i)
    assert [set(e) for e in back] == [set(U.SCENE_INFO_KEYS)] * 2                                   # BOP's keys, nothing else
    assert back == [{k: e[k] for k in U.SCENE_INFO_KEYS} for e in info[i]]                           # floats and ints read back as written
  assert scene.gt_info(0)[1]['visib_fract'] == 15 / 200 and scene.gt_info(0)[1]['bbox_obj'] == [-8, 0, 20, 20]
  assert scene.counted(0) == [True, False] and scene.counted(3) == [False, False]
  os.makedirs(os.path.join(str(tmp_path), 'models'), exist_ok=True)
  assert bop.targets_from_gt(tmp_path, 'test') == [dict(scene_id=1, im_id=0, obj_id=1, inst_count=1)]


def _script():
  spec = importlib.util.spec_from_file_location('bop_annotate', os.path.join(REPO, 'scripts', 'bop_annotate.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_bop_annotate_arguments(capsys):
  mod = _script()
  a = mod.parse_args(['/data/mine', 'test'])
  assert (a.dataset, a.split, a.scenes, a.delta, a.overwrite, a.pad) == ('/data/mine', 'test', None, 0.015, False, 'bop')
  a = mod.parse_args(['/data/mine', 'val', '--scenes', '3', '12', '--delta', '0.02', '--overwrite', '--pad', '320', '180'])
  assert (a.split, a.scenes, a.delta, a.overwrite, a.pad) == ('val', [3, 12], 0.02, True, (320, 180))
  assert mod.parse_args(['/data/mine', 'test', '--pad', '64']).pad == (64, 64) and mod.parse_args(['/data/mine', 'test', '--pad', 'bop']).pad == 'bop'
  for bad in (['/data/mine', 'test', '--pad', '-4'], ['/data/mine', 'test', '--pad', '1', '2', '3'], ['/data/mine', 'test', '--pad', 'bop', '2'],
              ['/data/mine'], ['/data/mine', 'test', '--delta', '-1'], ['/data/mine', 'test', '--delta', 'nan'], ['/data/mine', 'test', '--scenes', 'x']):
    with pytest.raises(SystemExit):
      mod.parse_args(bad)
  capsys.readouterr()


def test_mask_source_validation(tmp_path):
  from foundationpose_amd import bop
  scene = bop.BopScene(_bare_scene(tmp_path))
  targets = [dict(scene_id=1, im_id=0, obj_id=1, inst_count=1)]
  for bad in ('gt', 'gt_full', 'render', ''):
    with pytest.raises(ValueError, match='mask_source must be'):
      bop.image_instances(scene, 0, targets, mask_source=bad)
  with pytest.raises(ValueError, match='needs models'):
    bop.image_instances(scene, 0, targets, mask_source='gt_render')
  assert bop.image_instances(scene, 0, targets) == []                                                # 'gt_visib' as before: no file, no instance
  with pytest.raises(ValueError, match='unknown item'):
    bop.annotate_scene(scene.scene_dir, None, write=('masks',))
