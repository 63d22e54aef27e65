"""Writes a small BOP-format dataset tree (models in millimetres, one scene of a split) for the tests of foundationpose_amd.bop."""
import json
import os

import numpy as np


def exact_diameter(pts):
  """float64 diameter over all pairs, in blocks."""
  pts = np.asarray(pts, dtype=np.float64)
  return float(max(np.linalg.norm(pts[None] - pts[s:s + 256, None], axis=-1).max() for s in range(0, len(pts), 256)))


def write_models(root, models):
  """models: {obj_id: (mesh in METRES, extra models_info fields such as symmetries_discrete)}.  Writes models/obj_{id:06d}.ply in
  millimetres and models_info.json with the exact diameter (mm) of the float32 millimetre vertices the PLY holds."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.mesh_io import save_ply
  d = os.path.join(str(root), 'models')
  os.makedirs(d, exist_ok=True)
  info = {}
  for obj_id, (mesh, extra) in models.items():
    mm = S.SimpleMesh(np.asarray(mesh.vertices) * 1000.0, mesh.faces, vertex_normals=mesh.vertex_normals, visual=mesh.visual)
    save_ply(mm, os.path.join(d, f'obj_{obj_id:06d}.ply'))
    v = mm.vertices.astype(np.float32).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    info[str(obj_id)] = dict(diameter=exact_diameter(v), min_x=lo[0], min_y=lo[1], min_z=lo[2], size_x=hi[0] - lo[0], size_y=hi[1] - lo[1],
                             size_z=hi[2] - lo[2], **extra)
  with open(os.path.join(d, 'models_info.json'), 'w') as f:
    json.dump(info, f)
  return d


def write_scene(root, images, split='test', scene_id=1, color_dir='rgb', gt_info=True):
  """images: [dict(im_id, K (3,3), depth_scale, rgb uint8 (H,W,3) (or (H,W) for color_dir='gray'), depth_png uint16 (H,W),
  gt=[dict(obj_id, pose (4,4) metres, mask bool (H,W) or None, visib_fract)])].  Returns the scene directory."""
  from PIL import Image
  d = os.path.join(str(root), split, f'{scene_id:06d}')
  for sub in (color_dir, 'depth', 'mask_visib'):
    os.makedirs(os.path.join(d, sub), exist_ok=True)
  camera, gts, infos = {}, {}, {}
  for im in images:
    i = int(im['im_id'])
    camera[str(i)] = dict(cam_K=[float(x) for x in np.asarray(im['K']).reshape(-1)], depth_scale=float(im['depth_scale']))
    Image.fromarray(np.asarray(im['rgb'], dtype=np.uint8)).save(os.path.join(d, color_dir, f'{i:06d}.png'))
    Image.fromarray(np.asarray(im['depth_png'], dtype=np.uint16)).save(os.path.join(d, 'depth', f'{i:06d}.png'))
    gts[str(i)], infos[str(i)] = [], []
    for g, e in enumerate(im['gt']):
      pose = np.asarray(e['pose'], dtype=np.float64)
      gts[str(i)].append(dict(cam_R_m2c=[float(x) for x in pose[:3, :3].reshape(-1)], cam_t_m2c=[float(x) * 1000.0 for x in pose[:3, 3]],
                              obj_id=int(e['obj_id'])))
      m = e.get('mask')
      box = [-1, -1, -1, -1]
      if m is not None:
        Image.fromarray(np.asarray(m, dtype=np.uint8) * 255).save(os.path.join(d, 'mask_visib', f'{i:06d}_{g:06d}.png'))
        if np.any(m):
          r, c = np.nonzero(m)
          box = [int(c.min()), int(r.min()), int(c.max() - c.min() + 1), int(r.max() - r.min() + 1)]
      infos[str(i)].append(dict(visib_fract=float(e.get('visib_fract', 1.0)), bbox_visib=box, px_count_visib=int(0 if m is None else np.sum(m))))
  dump = lambda name, obj: json.dump(obj, open(os.path.join(d, name), 'w'))
  dump('scene_camera.json', camera)
  dump('scene_gt.json', gts)
  if gt_info:
    dump('scene_gt_info.json', infos)
  return d


def write_targets(root, targets, split='test'):
  with open(os.path.join(str(root), f'{split}_targets_bop19.json'), 'w') as f:
    json.dump(targets, f)
