"""BOP-format datasets end to end: object models, scenes, targets, the results CSV, registration of every target and the BOP-19 recalls.

The file layout is the one the reference's readers take (src/datareader.py:183-394, BopBaseReader): `models/obj_{id:06d}.ply` +
`models_info.json`, and per scene `scene_camera.json`, `scene_gt.json`, `scene_gt_info.json`, `rgb/` or `gray/`, `depth/`,
`mask_visib/{im:06d}_{gt:06d}.png`; targets as `test_targets_bop19.json`.  Files hold millimetres; every length leaves this module in
METRES.  Images are decoded with PIL, imported only where one is read.

    models = BopModels(f'{root}/models')
    rows = run_bop(root, 'test', models, refiner, scorer)            # one MultiObjectTracker.register per image (and group of 8)
    write_results('est_dataset-test.csv', rows)
    print(evaluate_results(root, 'test', models, rows))                # AR_VSD, AR_MSSD, AR_MSPD, AR

A home-made dataset that has scene_gt.json but no masks and no scene_gt_info.json gets them from annotate_scene (the device's
Utils.scene_instances in place of bop_toolkit's calc_gt_masks.py / calc_gt_info.py) before run_bop.
"""
import csv
import glob
import json
import os
import time

import numpy as np

VISIB_GT_MIN = 0.1                 # a ground-truth instance counts when at least this fraction of it is visible (BOP-19)
RESULTS_HEADER = 'scene_id,im_id,obj_id,score,R,t,time'
_IMAGE_EXTS = ('.png', '.jpg', '.jpeg', '.tif', '.tiff')


def _read_json(path):
  with open(path) as f:
    return json.load(f)


def _read_image(path):
  from PIL import Image
  with Image.open(path) as im:
    return np.array(im)


# ---------------------------------------------------------------------------------------------- models
class BopModels:
  """`models_dir`: models_info.json + obj_{id:06d}.ply (src/datareader.py:318-331, 380-389).  Host only; meshes are loaded on demand
  and kept."""

  def __init__(self, models_dir):
    self.models_dir = str(models_dir)
    self._info = {int(k): v for k, v in _read_json(os.path.join(self.models_dir, 'models_info.json')).items()}
    self.obj_ids = sorted(self._info)
    self._meshes = {}
    self._tensors = {}

  def info(self, obj_id):
    return self._info[int(obj_id)]

  def path(self, obj_id):
    return os.path.join(self.models_dir, f'obj_{int(obj_id):06d}.ply')

  def mesh(self, obj_id):
    """The model in metres (load_mesh(scale=1e-3)); one object per id: do not edit it."""
    obj_id = int(obj_id)
    if obj_id not in self._meshes:
      from .mesh_io import load_mesh
      self._meshes[obj_id] = load_mesh(self.path(obj_id), scale=1e-3)
    return self._meshes[obj_id]

  def mesh_tensors(self, obj_id):
    """make_mesh_tensors of mesh(obj_id) (the model as the file holds it, in metres, not centred), built once and kept: one upload
    per model however many images render it."""
    obj_id = int(obj_id)
    if obj_id not in self._tensors:
      from .mesh_tensors import make_mesh_tensors
      self._tensors[obj_id] = make_mesh_tensors(self.mesh(obj_id))
    return self._tensors[obj_id]

  def diameter(self, obj_id):
    """models_info's exact diameter, in metres."""
    return float(self.info(obj_id)['diameter']) / 1e3

  def symmetry_tfs(self, obj_id):
    """(S,4,4) float64, Utils.symmetry_tfs_from_info of the models_info entry (identity first)."""
    from .Utils import symmetry_tfs_from_info
    return symmetry_tfs_from_info(self.info(obj_id))


def write_models_info(models_dir, meshes, symmetries='auto', diameters=None, **find_kw):
  """Write `models_dir`/models_info.json, the file BopModels reads, for {obj_id: mesh} with meshes in METRES (as BopModels.mesh gives
  them): per object `diameter` (the exact one, Utils.mesh_diameter on the device, unless `diameters` {obj_id: metres} has it),
  `min_x/y/z` and `size_x/y/z`, all in millimetres, and the two symmetry keys from `symmetries`: 'auto' runs Utils.find_symmetries on
  every mesh (find_kw are its keyword arguments: tol, max_order, ..), None writes none, a dict {obj_id: info or None} takes
  find_symmetries' results as given.  `symmetries_discrete` holds each element but the identity as 16 numbers, the translation in mm;
  `symmetries_continuous` [{'axis', 'offset'}] the true unit axis and a point on it in mm.  BopModels.symmetry_tfs reads the discrete
  elements back exactly; the reference's helper behind it (Utils.symmetry_tfs_from_info) reads a continuous axis only along x, y or z
  and takes the offset as a translation, so for a continuous axis off the coordinate axes the entry written here is correct but that
  helper cannot express it: pass info['symmetry_tfs'] to FoundationPose and the metrics directly.  Returns {obj_id: entry}."""
  from .symmetry import models_info_entry
  if not (symmetries is None or isinstance(symmetries, dict) or symmetries == 'auto'):
    raise ValueError(f"write_models_info: symmetries must be 'auto', None or a dict, got {symmetries!r}")
  entries = {}
  for obj_id in sorted(int(k) for k in meshes):
    mesh = meshes[obj_id]
    if diameters is not None and obj_id in diameters:
      diameter = float(diameters[obj_id])
    else:
      from .Utils import mesh_diameter
      diameter = mesh_diameter(model_pts=np.asarray(mesh.vertices))
    info = None
    if isinstance(symmetries, dict):
      info = symmetries.get(obj_id)
    elif symmetries == 'auto':
      from .Utils import find_symmetries
      info = find_symmetries(mesh, **find_kw)
    entries[obj_id] = models_info_entry(np.asarray(mesh.vertices), diameter, info)
  os.makedirs(str(models_dir), exist_ok=True)
  with open(os.path.join(str(models_dir), 'models_info.json'), 'w') as f:
    json.dump({str(k): v for k, v in entries.items()}, f, indent=2)
  return entries


# ---------------------------------------------------------------------------------------------- scenes
class BopScene:
  """One scene directory (src/datareader.py:183-344).  Deviation from the reference: `depth_scale` is taken PER IMAGE from
  scene_camera.json, as the format defines it; the reference keeps the value of the last image it read for the whole scene."""

  def __init__(self, scene_dir, zfar=np.inf):
    self.scene_dir = str(scene_dir)
    self.zfar = float(zfar)
    by_int = lambda d: {int(k): v for k, v in d.items()}
    self._camera = by_int(_read_json(os.path.join(self.scene_dir, 'scene_camera.json')))
    gt_path, info_path = os.path.join(self.scene_dir, 'scene_gt.json'), os.path.join(self.scene_dir, 'scene_gt_info.json')
    self._gt = by_int(_read_json(gt_path)) if os.path.isfile(gt_path) else {}
    self._gt_info = by_int(_read_json(info_path)) if os.path.isfile(info_path) else None
    self._color_dir = 'rgb'
    self._color_files = self._image_files('rgb')
    if not self._color_files:
      self._color_dir = 'gray'
      self._color_files = self._image_files('gray')
    self.im_ids = sorted(self._color_files)

  def _image_files(self, sub):
    out = {}
    for p in sorted(glob.glob(os.path.join(self.scene_dir, sub, '*'))):
      stem, ext = os.path.splitext(os.path.basename(p))
      if ext.lower() in _IMAGE_EXTS and stem.isdigit():
        out.setdefault(int(stem), p)
    return out

  def K(self, im_id):
    return np.asarray(self._camera[int(im_id)]['cam_K'], dtype=np.float64).reshape(3, 3)

  def depth_scale(self, im_id):
    return float(self._camera[int(im_id)].get('depth_scale', 1.0))

  def color(self, im_id):
    """(H,W,3) uint8; a grey image is tiled to three channels."""
    im = _read_image(self._color_files[int(im_id)])
    if im.ndim == 2:
      im = np.tile(im[..., None], (1, 1, 3))
    if im.dtype != np.uint8:
      im = (im >> 8).astype(np.uint8) if im.dtype.kind in 'ui' and im.max() > 255 else im.astype(np.uint8)
    return np.ascontiguousarray(im[..., :3])

  def depth(self, im_id):
    """(H,W) float32 metres: (file * 1e-3) * depth_scale evaluated in float64, values below 0.001 or beyond zfar set to 0."""
    files = self._image_files('depth')
    d = (_read_image(files[int(im_id)]).astype(np.float64) * 1e-3) * self.depth_scale(im_id)
    d[(d < 0.001) | (d > self.zfar)] = 0
    return d.astype(np.float32)

  def gt(self, im_id):
    """[dict(obj_id, pose (4,4) float64 object-to-camera in metres, gt_id)], in file order (gt_id = the index the mask files carry)."""
    out = []
    for g, e in enumerate(self._gt.get(int(im_id), [])):
      pose = np.eye(4)
      pose[:3, :3] = np.asarray(e['cam_R_m2c'], dtype=np.float64).reshape(3, 3)
      pose[:3, 3] = np.asarray(e['cam_t_m2c'], dtype=np.float64).reshape(3) / 1e3
      out.append(dict(obj_id=int(e['obj_id']), pose=pose, gt_id=g))
    return out

  def gt_info(self, im_id):
    """scene_gt_info.json's entries of the image (visib_fract, bbox_visib, ..), or None without that file."""
    return None if self._gt_info is None else self._gt_info.get(int(im_id), [])

  def counted(self, im_id, visib_gt_min=VISIB_GT_MIN):
    """Per ground-truth instance: does it count as a target (visib_fract >= visib_gt_min; every instance without scene_gt_info)."""
    info = self.gt_info(im_id)
    n = len(self._gt.get(int(im_id), []))
    return [True] * n if info is None else [float(info[g]['visib_fract']) >= visib_gt_min for g in range(n)]

  def mask(self, im_id, gt_id, kind='mask_visib'):
    """bool (H,W) from {kind}/{im_id:06d}_{gt_id:06d}.png, None when the file is absent."""
    p = os.path.join(self.scene_dir, kind, f'{int(im_id):06d}_{int(gt_id):06d}.png')
    if not os.path.isfile(p):
      return None
    m = _read_image(p)
    return (m if m.ndim == 2 else m[..., 0]) > 0


# ---------------------------------------------------------------------------------------------- masks and gt_info from the ground truth
def _render_gt(scene, im_id, models, delta=0.015, pad='bop', want=('mask', 'mask_visib', 'info')):
  """Utils.scene_instances over the ground-truth instances of one image, as bop_toolkit annotates: the recorded depth is the only
  occluder, the models are rendered as the files hold them (metres, NOT centred: the poses are model-frame poses).  Host arrays: mask /
  mask_visib (n,H,W) bool, info (list of dicts)."""
  from . import Utils as U
  gts = scene.gt(im_id)
  depth = scene.depth(im_id)
  H, W = depth.shape
  out = U.scene_instances(scene.K(im_id), H, W, [models.mesh_tensors(g['obj_id']) for g in gts], np.stack([g['pose'] for g in gts]).astype(np.float32),
                          depth=depth, occluders='depth', delta=delta, pad=pad, want=want)
  return {k: (v.cpu().numpy() > 0 if k in ('mask', 'mask_visib') else v) for k, v in out.items()}


def write_gt_info(scene_dir, info_by_image):
  """scene_gt_info.json from {im_id: [dict per ground-truth instance, in gt order]} (keys as Utils.scene_info_rows gives them; the BOP
  keys are written, px_count_in_frame is not one)."""
  from .Utils import SCENE_INFO_KEYS
  doc = {str(int(i)): [{k: e[k] for k in SCENE_INFO_KEYS if k in e} for e in entries] for i, entries in sorted(info_by_image.items())}
  with open(os.path.join(str(scene_dir), 'scene_gt_info.json'), 'w') as f:
    json.dump(doc, f)


def annotate_scene(scene_dir, models, im_ids=None, delta=0.015, pad='bop', write=('mask', 'mask_visib', 'gt_info'), overwrite=False):
  """Write what a recorded scene with ground-truth poses still lacks to be evaluated: `mask/{im:06d}_{gt:06d}.png` and
  `mask_visib/..png` (8-bit, 0 / 255) of every ground-truth instance and `scene_gt_info.json` (px_count_all, px_count_valid,
  px_count_visib, visib_fract, bbox_obj, bbox_visib per instance, one list per image in gt order) - bop_toolkit's calc_gt_masks.py and
  calc_gt_info.py, on the device: one Utils.scene_instances call per image, the recorded depth image as the occluder (delta: BOP's
  15 mm), pad='bop' so that the part of an object outside the image counts in px_count_all.  Deviation from the toolkit: masks, counts
  and boxes come from ONE render on the padded canvas, so px_count_visib == count(mask_visib) always.
  pad: as Utils.scene_instances takes it; 'bop' fits frames up to 640 x 480, a larger frame needs a smaller pad (an (x, y) pair), and
  what lies beyond the canvas is then not counted in px_count_all.
  im_ids=None: every image of scene_gt.json.  Existing files are kept unless overwrite=True, and an image that lacks nothing is not
  rendered; an existing scene_gt_info.json keeps its entries of images outside im_ids either way.  Returns {im_id: [info dicts]}: as
  computed (px_count_in_frame included), or as scene_gt_info.json holds them for an image that was complete."""
  unknown = [w for w in write if w not in ('mask', 'mask_visib', 'gt_info')]
  if unknown:
    raise ValueError(f"unknown item(s) {unknown} in write: choose from 'mask', 'mask_visib', 'gt_info'")
  from PIL import Image
  if not isinstance(models, BopModels):
    models = BopModels(models)
  scene = BopScene(scene_dir)
  im_ids = sorted(scene._gt) if im_ids is None else [int(i) for i in im_ids]
  info_path = os.path.join(scene.scene_dir, 'scene_gt_info.json')
  mask_path = lambda kind, im_id, g: os.path.join(scene.scene_dir, kind, f"{im_id:06d}_{g['gt_id']:06d}.png")
  out = {}
  for im_id in im_ids:
    gts = scene.gt(im_id)
    if not gts:
      out[im_id] = []
      continue
    have = scene.gt_info(im_id)
    if not overwrite and ('gt_info' not in write or (have is not None and len(have) == len(gts))) and \
       all(os.path.isfile(mask_path(k, im_id, g)) for k in ('mask', 'mask_visib') if k in write for g in gts):
      if have is not None and len(have) == len(gts):
        out[im_id] = have                         # nothing to write for this image: it is not rendered, its entries are the file's
        continue
    r = _render_gt(scene, im_id, models, delta=delta, pad=pad)
    out[im_id] = r['info']
    for kind in ('mask', 'mask_visib'):
      if kind not in write:
        continue
      os.makedirs(os.path.join(scene.scene_dir, kind), exist_ok=True)
      for g in gts:
        p = mask_path(kind, im_id, g)
        if overwrite or not os.path.isfile(p):
          Image.fromarray(r[kind][g['gt_id']].astype(np.uint8) * 255).save(p)
  if 'gt_info' in write and (overwrite or not os.path.isfile(info_path)):
    doc = {} if scene._gt_info is None else dict(scene._gt_info)
    doc.update(out)
    write_gt_info(scene.scene_dir, doc)
  return out


def _scene_dirs(dataset_dir, split):
  out = {}
  for p in sorted(glob.glob(os.path.join(str(dataset_dir), split, '*'))):
    if os.path.isdir(p) and os.path.basename(p).isdigit():
      out[int(os.path.basename(p))] = p
  return out


# ---------------------------------------------------------------------------------------------- targets
def load_targets(path):
  """test_targets_bop19.json: [dict(scene_id, im_id, obj_id, inst_count)] with int values."""
  return [dict(scene_id=int(t['scene_id']), im_id=int(t['im_id']), obj_id=int(t['obj_id']), inst_count=int(t['inst_count']))
          for t in _read_json(path)]


def targets_from_gt(dataset_dir, split, visib_gt_min=VISIB_GT_MIN):
  """Targets of a split without a targets file: one per (scene, image, object) in that order, inst_count = the instances whose
  visib_fract >= visib_gt_min (all instances without scene_gt_info.json); objects left with none are no target."""
  out = []
  for scene_id, d in _scene_dirs(dataset_dir, split).items():
    scene = BopScene(d)
    for im_id in sorted(scene._gt):
      counted = scene.counted(im_id, visib_gt_min)
      count = {}
      for g, c in zip(scene.gt(im_id), counted):
        count[g['obj_id']] = count.get(g['obj_id'], 0) + int(c)
      out += [dict(scene_id=scene_id, im_id=im_id, obj_id=o, inst_count=n) for o, n in sorted(count.items()) if n > 0]
  return out


def _default_targets(dataset_dir, split):
  path = os.path.join(str(dataset_dir), f'{split}_targets_bop19.json')
  return load_targets(path) if os.path.isfile(path) else targets_from_gt(dataset_dir, split)


# ---------------------------------------------------------------------------------------------- results CSV
def write_results(path, rows):
  """The BOP results file: `scene_id,im_id,obj_id,score,R,t,time`; R nine and t three space-separated numbers, row-major, t in
  MILLIMETRES, time in seconds (-1 = unknown).  rows: dicts with scene_id, im_id, obj_id, score, pose ((4,4) object-to-camera, metres)
  and optionally time.  Numbers are written with repr, the shortest text that reads back to the same float64."""
  num = lambda x: repr(float(x))
  with open(path, 'w', newline='') as f:
    f.write(RESULTS_HEADER + '\n')
    for r in rows:
      pose = np.asarray(r['pose'], dtype=np.float64).reshape(4, 4)
      R = ' '.join(num(x) for x in pose[:3, :3].reshape(-1))
      t = ' '.join(num(x * 1000.0) for x in pose[:3, 3])
      f.write(f"{int(r['scene_id'])},{int(r['im_id'])},{int(r['obj_id'])},{num(r['score'])},{R},{t},{num(r.get('time', -1))}\n")


def read_results(path):
  """-> rows as write_results takes them; pose (4,4) float64 in metres (t / 1000).  The rotation reads back bit for bit and the
  translation to within one float64 rounding, so a float32 pose is recovered exactly by .astype(np.float32)."""
  rows = []
  with open(path, newline='') as f:
    reader = csv.reader(f)
    header = next(reader, None)
    if header is None or ','.join(header) != RESULTS_HEADER:
      raise ValueError(f'{path}: the first line must be {RESULTS_HEADER!r}')
    for n, rec in enumerate(reader, 2):
      if not rec:
        continue
      if len(rec) != 7:
        raise ValueError(f'{path}:{n}: expected 7 fields, got {len(rec)}')
      R, t = np.array(rec[4].split(), dtype=np.float64), np.array(rec[5].split(), dtype=np.float64)
      if R.size != 9 or t.size != 3:
        raise ValueError(f'{path}:{n}: R needs 9 numbers and t 3')
      pose = np.eye(4)
      pose[:3, :3], pose[:3, 3] = R.reshape(3, 3), t / 1000.0
      rows.append(dict(scene_id=int(rec[0]), im_id=int(rec[1]), obj_id=int(rec[2]), score=float(rec[3]), pose=pose, time=float(rec[6])))
  return rows


# ---------------------------------------------------------------------------------------------- registration of every target
def build_estimators(models, obj_ids, refiner, scorer, diameter='info'):
  """{obj_id: FoundationPose} on the models in metres, symmetry transforms from models_info.  diameter: 'info' = the models_info value,
  'exact' = Utils.mesh_diameter, None = the reference's sampled value (depends on numpy's seed above 10000 vertices)."""
  from .estimater import FoundationPose
  if diameter not in ('info', 'exact', None):
    raise ValueError(f"diameter must be 'info', 'exact' or None, got {diameter!r}")
  out = {}
  for o in sorted(set(int(x) for x in obj_ids)):
    mesh = models.mesh(o)
    out[o] = FoundationPose(model_pts=mesh.vertices, model_normals=mesh.vertex_normals, symmetry_tfs=models.symmetry_tfs(o), mesh=mesh,
                            refiner=refiner, scorer=scorer, diameter=models.diameter(o) if diameter == 'info' else diameter)
  return out


def detect_instances(scene, im_id, targets, estimators, delta=0.015, **detect_kw):
  """[(obj_id, mask bool (H,W), det_score)] of an image without any ground truth: for every target the inst_count best detections of
  its object's estimator (FoundationPose.detect on the recorded depth: templates of the model, geometry only) and, per detection, the
  pixels the model shows at the detected pose in front of the recorded depth (Utils.scene_instances, mask_visib); det_score is the
  match score as a fraction of n_in n_out.  What mask_source='detect' feeds image_instances."""
  from . import Utils as U
  depth, K = scene.depth(im_id), scene.K(im_id)
  H, W = depth.shape[:2]
  out = []
  for t in targets:
    est = estimators[t['obj_id']]
    found = est.detect(depth, K, top_k=int(t['inst_count']), **detect_kw)
    if not found:
      continue
    ts = est.templates()
    masks = U.scene_instances(K, H, W, est.mesh_tensors, np.stack([d['ob_in_cam'] for d in found]), depth=depth, occluders='depth', delta=delta,
                              want=('mask_visib',))['mask_visib'].cpu().numpy() > 0
    out += [(t['obj_id'], m, d['score'] / float(ts.n_in * ts.n_out)) for d, m in zip(found, masks)]
  return out


def image_instances(scene, im_id, targets, mask_source='gt_visib', models=None, pad='bop', estimators=None):
  """The instances run_bop registers in one image, in order: [(obj_id, mask bool (H,W))].  targets: the image's targets.
  mask_source='gt_visib': for every target the `mask_visib` of the object's counted ground-truth instances (visib_fract >= 0.1), in
  gt_id order, inst_count at most; a callable (scene, im_id) -> [(obj_id, mask, det_score)]: the inst_count best-scored detections of
  the object.  An instance without a mask file, or with an empty mask, is left out.
  mask_source='gt_render' (needs `models`, a BopModels): as 'gt_visib', but an instance without a mask file gets the mask_visib that
  annotate_scene would write (Utils.scene_instances on the image's ground truth, the recorded depth as the occluder), and without
  scene_gt_info.json the instances are counted by the computed visib_fract; `pad` as annotate_scene takes it.
  mask_source='detect' (needs `estimators`, {obj_id: FoundationPose}): no ground truth is read; detect_instances finds the objects in
  the recorded depth."""
  out = []
  if mask_source == 'detect':
    if estimators is None:
      raise ValueError("mask_source='detect' needs estimators={obj_id: FoundationPose}")
    mask_source = lambda sc, im: detect_instances(sc, im, targets, estimators)
  if callable(mask_source):
    dets = list(mask_source(scene, im_id))
    for t in targets:
      mine = sorted([d for d in dets if int(d[0]) == t['obj_id']], key=lambda d: -float(d[2]))[:t['inst_count']]
      out += [(t['obj_id'], np.asarray(d[1]) > 0) for d in mine if d[1] is not None and np.any(d[1])]
    return out
  if mask_source not in ('gt_visib', 'gt_render'):
    raise ValueError(f"mask_source must be 'gt_visib', 'gt_render', 'detect' or a callable, got {mask_source!r}")
  gts, counted = scene.gt(im_id), scene.counted(im_id)
  rendered = None
  if mask_source == 'gt_render':
    if models is None:
      raise ValueError("mask_source='gt_render' needs models=BopModels(...)")
    if not isinstance(models, BopModels):
      models = BopModels(models)
    missing = [g for g in gts if not os.path.isfile(os.path.join(scene.scene_dir, 'mask_visib', f"{int(im_id):06d}_{g['gt_id']:06d}.png"))]
    if gts and (missing or scene.gt_info(im_id) is None):
      rendered = _render_gt(scene, im_id, models, pad=pad, want=('mask_visib', 'info'))
      if scene.gt_info(im_id) is None:
        counted = [r['visib_fract'] >= VISIB_GT_MIN for r in rendered['info']]
  for t in targets:
    mine = [g for g, c in zip(gts, counted) if c and g['obj_id'] == t['obj_id']][:t['inst_count']]
    for g in mine:
      m = scene.mask(im_id, g['gt_id'], 'mask_visib')
      if m is None and rendered is not None:
        m = rendered['mask_visib'][g['gt_id']]
      if m is not None and m.any():
        out.append((t['obj_id'], m))
  return out


def _by_image(targets):
  out = {}
  for t in targets:
    out.setdefault((int(t['scene_id']), int(t['im_id'])), []).append(t)
  return out


def run_bop(dataset_dir, split, models, refiner, scorer, targets=None, iteration=5, mask_source='gt_visib', diameter='info',
            max_objects=None, estimators=None, pad='bop', polish=False):
  """Register every target of a BOP split: rows for write_results (pose float32 (4,4) in metres, score = the registration's best
  score, time = the wall time of the image's registrations, the same on every row of an image as BOP asks).

  models: BopModels (or the models directory).  targets: as load_targets returns them (None: {split}_targets_bop19.json of the dataset
  when present, else targets_from_gt).  One FoundationPose per object id is built once (build_estimators; `estimators` passes ready
  ones); every instance of an image gets `FoundationPose.instance()` of its object's estimator, and the image's instances
  (image_instances) are registered by MultiObjectTracker(...).register(rgb, depth, K, masks, iteration) in groups of at most
  max_objects (None: FP_TRACK_MAX_OBJECTS), the image handed over as the numpy arrays BopScene reads.  An instance with fewer than 4
  usable depth pixels in its mask gets register()'s fallback pose with score 0.  pad: the canvas of mask_source='gt_render'.
  mask_source='detect' reads no ground truth at all: the masks come from detect_instances (templates of the models matched against the
  recorded depth; geometry only, so expect far lower recall than with ground-truth masks).
  polish (False; True; or a dict of MultiObjectTracker.polish's arguments): the registered poses of a group are then moved onto the
  depth by geometry alone (fp_pose_polish), each against the normals of its own mask; the score stays the registration's.  Off, the
  rows are what they were before the option existed."""
  from ._lib import FP_TRACK_MAX_OBJECTS
  from .tracking import MultiObjectTracker
  if not isinstance(models, BopModels):
    models = BopModels(models)
  max_objects = FP_TRACK_MAX_OBJECTS if max_objects is None else int(max_objects)
  if not 1 <= max_objects <= FP_TRACK_MAX_OBJECTS:
    raise ValueError(f'max_objects must be 1 .. {FP_TRACK_MAX_OBJECTS}, got {max_objects}')
  targets = _default_targets(dataset_dir, split) if targets is None else list(targets)
  if estimators is None:
    estimators = build_estimators(models, [t['obj_id'] for t in targets], refiner, scorer, diameter)
  dirs, scenes, rows = _scene_dirs(dataset_dir, split), {}, []
  for (scene_id, im_id), ts in _by_image(targets).items():
    if scene_id not in scenes:
      scenes[scene_id] = BopScene(dirs[scene_id])
    scene = scenes[scene_id]
    inst = image_instances(scene, im_id, ts, mask_source, models=models, pad=pad, estimators=estimators)
    if not inst:
      continue
    rgb, depth, K = scene.color(im_id), scene.depth(im_id), scene.K(im_id)
    found, t0 = [], time.perf_counter()
    for g0 in range(0, len(inst), max_objects):
      group = inst[g0:g0 + max_objects]
      ests = [estimators[o].instance() for o, _ in group]
      poses = MultiObjectTracker(ests).register(rgb, depth, K, [m for _, m in group], iteration=iteration)
      if polish:
        reg = [k for k, e in enumerate(ests) if e.pose_last is not None]
        if reg:
          got = MultiObjectTracker([ests[k] for k in reg]).polish(depth, K, masks=[group[k][1] for k in reg], **(polish if isinstance(polish, dict) else {}))
          for j, k in enumerate(reg):
            poses[k] = got[j]
      found += [(o, poses[k], float(e.scores[0]) if e.scores is not None else 0.0) for k, ((o, _), e) in enumerate(zip(group, ests))]
    elapsed = time.perf_counter() - t0
    rows += [dict(scene_id=scene_id, im_id=im_id, obj_id=o, score=s, pose=p, time=elapsed) for o, p, s in found]
  return rows


# ---------------------------------------------------------------------------------------------- matching and recall
def match_and_recall(groups, errors=('vsd', 'mssd', 'mspd')):
  """BOP-19 matching and recall on the host, from error matrices.

  groups: one dict per (scene, image, object) target:
    obj_id, inst_count, scores (E,) of the object's estimates in the image, and for every name in `errors` the errors of every
    estimate against every ground-truth instance of the object in the image: 'mssd' (E,G) metres, 'mspd' (E,G) pixels, 'vsd' (E,G,T)
    (T = len(BOP19_VSD_TAUS)); gt_counts (G,) bool (default all): the instances with visib_fract >= 0.1; diameter (metres, for
    'mssd'); image_width (for 'mspd', default 640).
  The rule:
    1. of a target's estimates the inst_count best-scored are kept (a stable sort: equal scores keep their order);
    2. only the ground-truth instances that count can be matched, and their number over all groups is n_targets;
    3. for every error type and every threshold of it - BOP19_MSSD_THETAS x diameter, BOP19_MSPD_THETAS x image_width / 640, every
       (tau, theta) of BOP19_VSD_THETAS - the kept estimates, best score first, each take, among the still unmatched counted instances
       with error < threshold, the one of the least error; recall = matches / n_targets;
    4. AR_<type> = the mean recall over the type's thresholds; AR = the mean of the AR_<type> asked for.
  Returns dict(AR_VSD, AR_MSSD, AR_MSPD, AR, n_targets, recalls={type: per-threshold recalls}, per_object={obj_id: the same of that
  object's targets}).  With one instance per target this is Utils.bop_average_recall of the paired errors."""
  from .Utils import BOP19_MSPD_THETAS, BOP19_MSSD_THETAS, BOP19_VSD_THETAS
  errors = tuple(errors)
  unknown = [e for e in errors if e not in ('vsd', 'mssd', 'mspd')]
  if unknown:
    raise ValueError(f"unknown error type(s) {unknown}: choose from 'vsd', 'mssd', 'mspd'")

  def columns(g, name, E, G):
    """errors (E, G, C) and thresholds (C,) of every threshold column of an error type"""
    e = np.asarray(g[name], dtype=np.float64)
    if name == 'vsd':
      e = e.reshape(E, G, -1)
      return np.repeat(e, len(BOP19_VSD_THETAS), axis=2), np.tile(np.asarray(BOP19_VSD_THETAS, dtype=np.float64), e.shape[2])
    e = e.reshape(E, G)[..., None]
    th = BOP19_MSSD_THETAS * float(g['diameter']) if name == 'mssd' else BOP19_MSPD_THETAS * (float(g.get('image_width', 640)) / 640.0)
    return np.repeat(e, len(th), axis=2), np.asarray(th, dtype=np.float64)

  def tally(gs):
    n_targets, matches = 0, {name: None for name in errors}
    for g in gs:
      scores = np.asarray(g['scores'], dtype=np.float64).reshape(-1)
      E = len(scores)
      counts = None if g.get('gt_counts') is None else np.asarray(g['gt_counts'], dtype=bool).reshape(-1)
      G = len(counts) if counts is not None else (np.asarray(g[errors[0]]).shape[1] if E else int(g['inst_count']))
      counts = np.ones(G, dtype=bool) if counts is None else counts
      n_targets += int(counts.sum())
      keep = np.argsort(-scores, kind='stable')[:int(g['inst_count'])]
      if not len(keep) or not G:
        continue
      for name in errors:
        err, th = columns(g, name, E, G)
        free = np.repeat(counts[:, None], len(th), axis=1)            # (G, C): counted and not matched yet, per threshold column
        got = np.zeros(len(th), dtype=np.int64)
        cols = np.arange(len(th))
        for e in keep:
          cand = (err[e] < th[None]) & free
          pick = np.where(cand, err[e], np.inf).argmin(axis=0)
          ok = cand.any(axis=0)
          free[pick[ok], cols[ok]] = False
          got += ok
        matches[name] = got if matches[name] is None else matches[name] + got
    out = dict(n_targets=n_targets, recalls={})
    for name in errors:
      if matches[name] is None:
        n_cols = len(BOP19_VSD_THETAS) ** 2 if name == 'vsd' else len(BOP19_MSSD_THETAS if name == 'mssd' else BOP19_MSPD_THETAS)
        matches[name] = np.zeros(n_cols, dtype=np.int64)
      rec = np.array([float(m) / n_targets for m in matches[name]]) if n_targets else np.zeros(len(matches[name]))
      out['recalls'][name] = rec
      out['AR_' + name.upper()] = float(np.mean(rec))
    out['AR'] = float(np.mean([out['AR_' + name.upper()] for name in errors])) if errors else 0.0
    return out

  groups = list(groups)
  res = tally(groups)
  res['per_object'] = {o: tally([g for g in groups if int(g['obj_id']) == o]) for o in sorted(set(int(g['obj_id']) for g in groups))}
  return res


def evaluate_results(dataset_dir, split, models, rows_or_csv, targets=None, errors=('vsd', 'mssd', 'mspd')):
  """BOP-19 recalls of a results file (or of rows) against a split's ground truth: match_and_recall on errors computed on the device,
  one call per (image, object) and error kind - MSSD / MSPD by Utils.bop_pose_errors (the model's vertices in metres, symmetry transforms
  from models_info, the image's K), VSD by Utils.vsd_errors (the scene's depth, diameter from models_info, BOP19_VSD_DELTA,
  BOP19_VSD_TAUS).  Adds n_estimates (rows that belong to a target) to match_and_recall's dict."""
  from . import Utils as U
  if not isinstance(models, BopModels):
    models = BopModels(models)
  rows = read_results(rows_or_csv) if isinstance(rows_or_csv, (str, os.PathLike)) else list(rows_or_csv)
  targets = _default_targets(dataset_dir, split) if targets is None else list(targets)
  by_target = {}
  for r in rows:
    by_target.setdefault((int(r['scene_id']), int(r['im_id']), int(r['obj_id'])), []).append(r)
  dirs, scenes, tensors, groups, n_est = _scene_dirs(dataset_dir, split), {}, {}, [], 0
  for t in targets:
    scene_id, im_id, obj_id = t['scene_id'], t['im_id'], t['obj_id']
    if scene_id not in scenes:
      scenes[scene_id] = BopScene(dirs[scene_id])
    scene = scenes[scene_id]
    gts, counted = scene.gt(im_id), scene.counted(im_id)
    mine = [(g, c) for g, c in zip(gts, counted) if g['obj_id'] == obj_id]
    ests = by_target.get((scene_id, im_id, obj_id), [])
    n_est += len(ests)
    scores = np.array([float(r['score']) for r in ests], dtype=np.float64)
    keep = np.argsort(-scores, kind='stable')[:t['inst_count']]
    E, G = len(keep), len(mine)
    g = dict(obj_id=obj_id, inst_count=t['inst_count'], scores=scores[keep], gt_counts=[c for _, c in mine], diameter=models.diameter(obj_id))
    if E and G:
      depth = scene.depth(im_id) if 'vsd' in errors or 'mspd' in errors else None
      K = scene.K(im_id)
      P = np.repeat(np.stack([np.asarray(ests[k]['pose'], dtype=np.float64) for k in keep])[:, None], G, axis=1).reshape(E * G, 4, 4)
      T = np.repeat(np.stack([x['pose'] for x, _ in mine])[None], E, axis=0).reshape(E * G, 4, 4)
      mesh = models.mesh(obj_id)
      pair = [m for m in ('mssd', 'mspd') if m in errors]
      if pair:
        e = U.bop_pose_errors(P, T, mesh.vertices, K=K, symmetry_tfs=models.symmetry_tfs(obj_id), metrics=tuple(pair))
        for m in pair:
          g[m] = e[m].cpu().numpy().reshape(E, G)
      if 'mspd' in errors:
        g['image_width'] = depth.shape[1]
      if 'vsd' in errors:
        if obj_id not in tensors:
          tensors[obj_id] = U.make_mesh_tensors(mesh)
        e = U.vsd_errors(P, T, depth, K, mesh_tensors=tensors[obj_id], diameter=models.diameter(obj_id), delta=U.BOP19_VSD_DELTA,
                         taus=U.BOP19_VSD_TAUS)
        g['vsd'] = e.cpu().numpy().reshape(E, G, -1)
    else:
      g['scores'] = scores[:0]
    groups.append(g)
  res = match_and_recall(groups, errors=errors)
  res['n_estimates'] = n_est
  return res
