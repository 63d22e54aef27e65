"""The caller-side protocol the reference's readme documents (readme.md:122-185) but does not ship
(SURVEY.md D1): `Processor.process(data) -> data`, optional `visualize(data)`,
`Pipeline(name).add_processor(p)`, `pipeline.run(PipelineData()) -> data` with `data.pose_6d`,
`FoundationPoseEstimator(mesh_file, intrinsics_file)` and `PoseTransformer` (src/transform.py:4-67).
"""
import logging
import math

import numpy as np

METERS_TO_INCHES = 39.3701     # src/transform.py:47


class PipelineData:
  """Attribute bag passed from processor to processor (`rgb, depth, mask, K, pose, pose_6d, errors`)."""

  def __init__(self, **kw):
    self.rgb = self.depth = self.mask = self.K = None
    self.right = None         # the right image of a stereo pair (StereoRectify, StereoDepth), rgb being the left one
    self.baseline = None      # metres, set by StereoRectify for a StereoDepth(baseline=None) behind it
    self.lost = False         # set by the caller when the track is lost: Detect then looks for the object again
    self.detections = None    # Utils.detect's records of the frame, left by Detect
    self.pose = None          # 4x4 ob_in_cam of the original (un-centred) mesh
    self.center_pose = None   # pose @ inv(to_origin) of the model's oriented box (main.py:67), set by FoundationPoseEstimator(box='oriented')
    self.pose_6d = None       # (x, y, z, roll, pitch, yaw)
    self.errors = []
    self.__dict__.update(kw)


class Processor:
  def process(self, data):
    raise NotImplementedError

  def visualize(self, data):
    return None


class Pipeline:
  def __init__(self, name='Pipeline', stop_on_error=False, visualize=False):
    self.name, self.stop_on_error, self.visualize = name, stop_on_error, visualize
    self.processors = []

  def add_processor(self, processor):
    if not callable(getattr(processor, 'process', None)):
      raise TypeError('a processor needs a process(data) method')
    self.processors.append(processor)
    return self

  def run(self, data=None):
    """Runs the processors in order.  A failing processor is recorded in `data.errors`; with
    `stop_on_error` (readme.md:120) the run ends there, otherwise the next processor still runs."""
    data = PipelineData() if data is None else data
    for proc in self.processors:
      try:
        out = proc.process(data)
        data = data if out is None else out
        if self.visualize and hasattr(proc, 'visualize'):
          proc.visualize(data)
      except Exception as exc:          # noqa: BLE001 - the protocol isolates processors from each other
        logging.error(f'[{self.name}] {type(proc).__name__} failed: {exc}')
        data.errors.append((type(proc).__name__, exc))
        if self.stop_on_error:
          break
    return data


def rotation_to_roll_pitch_yaw(R):
  """ZYX Euler angles (radians) with the reference's gimbal-lock convention (src/transform.py:52-67):
  |R[2,0]| > 0.9999 -> yaw = 0, pitch = +-pi/2, roll from atan2(R[0,1], R[1,1])."""
  s = R[2, 0]
  if abs(s) > 0.9999:
    roll = math.atan2(R[0, 1], R[1, 1])
    return (roll, math.pi / 2, 0) if s < 0 else (-roll, -math.pi / 2, 0)
  pitch = -math.asin(s)
  c = math.cos(pitch)
  return math.atan2(R[2, 1] / c, R[2, 2] / c), pitch, math.atan2(R[1, 0] / c, R[0, 0] / c)


class PoseTransformer(Processor):
  """4x4 pose -> (x, y, z, roll, pitch, yaw); inches / degrees by default (src/transform.py:4-50)."""

  def __init__(self, to_inches=True, to_degrees=True):
    self.to_inches, self.to_degrees = to_inches, to_degrees

  def transform_pose(self, center_pose):
    pose = np.asarray(center_pose)
    xyz = [float(v) * (METERS_TO_INCHES if self.to_inches else 1.0) for v in pose[:3, 3]]
    rpy = [math.degrees(a) if self.to_degrees else a for a in rotation_to_roll_pitch_yaw(pose[:3, :3])]
    return (*xyz, *rpy)

  def process(self, data):
    data.pose_6d = self.transform_pose(data.pose)
    return data


class StereoDepth(Processor):
  """Fills `data.depth` from the rectified pair `data.rgb` (left) / `data.right` when `data.depth is None`, and leaves `data` alone
  otherwise: the stage in front of FoundationPoseEstimator on a stereo camera whose vendor SDK is not there (the reference loads that
  SDK's depth, src/file_processing.py:99-138).  baseline in metres; K: the left camera's 3x3 matrix, `data.K` when that is set; **kw:
  the arguments of Utils.stereo_depth (max_disparity, p1, p2, paths, lr_max, min_disparity, subpixel, zfar).  Device tensors in give a
  device tensor in `data.depth`, without a host copy.  The pair must already be rectified and undistorted: StereoRectify in front
  does that for a raw pair, and with baseline=None the baseline it left in `data.baseline` is used."""

  def __init__(self, baseline=None, K=None, **kw):
    self.baseline = None if baseline is None else float(baseline)
    self.K = None if K is None else np.asarray(K, dtype=np.float64)
    self._kw = kw

  def process(self, data):
    if data.depth is not None:
      return data
    right = getattr(data, 'right', None)
    if data.rgb is None or right is None:
      raise ValueError('StereoDepth: data.depth is None and data.rgb / data.right do not hold a pair')
    K = self.K if data.K is None else data.K
    if K is None:
      raise ValueError('StereoDepth: no camera matrix (K=... or data.K)')
    baseline = self.baseline if self.baseline is not None else getattr(data, 'baseline', None)
    if baseline is None:
      raise ValueError('StereoDepth: no baseline (baseline=... or a StereoRectify in front)')
    from .stereo import stereo_depth
    data.depth = stereo_depth(data.rgb, right, K, baseline, **self._kw)
    return data


class StereoRectify(Processor):
  """Replaces the RAW pair `data.rgb` (left) / `data.right` by the rectified, undistorted one and sets `data.K = rect.K_new` and
  `data.baseline = rect.baseline`: the stage in front of StereoDepth on a raw stereo camera.  rect: rectify.rectify_stereo(...).  Leaves
  `data` alone when `data.right` is missing (a frame that is no pair), the way StereoDepth leaves a frame with a depth alone.  One launch
  for both images; device tensors in give device tensors, without a host copy."""

  def __init__(self, rect):
    self.rect = rect

  def process(self, data):
    if data.rgb is None or getattr(data, 'right', None) is None:
      return data
    from .rectify import rectify_pair
    data.rgb, data.right = rectify_pair(data.rgb, data.right, self.rect)
    data.K = self.rect.K_new.copy()
    data.baseline = self.rect.baseline
    return data


class Undistort(Processor):
  """Replaces `data.rgb` and `data.depth` of a camera with lens distortion by their undistorted versions (whichever of the two is there)
  and sets `data.K = plan.K_new`: the stage in front of FoundationPoseEstimator on such an RGB-D stream.  plan: rectify.undistort_plan(...).
  A mask in `data.mask` is NOT warped: make it on the undistorted frame."""

  def __init__(self, plan, zfar=np.inf):
    self.plan, self.zfar = plan, zfar

  def process(self, data):
    from .rectify import undistort_frame
    data.rgb, data.depth = undistort_frame(data.rgb, data.depth, self.plan, zfar=self.zfar)
    data.K = self.plan.K_new.copy()
    return data


class AlignDepth(Processor):
  """Replaces `data.rgb` and `data.depth` of an RGB-D camera whose depth and colour come from two sensors by the frame aligned to the
  colour camera (whichever of the two is there) and sets `data.K = rig.K`: the stage in front of FoundationPoseEstimator on such a
  stream.  rig: reproject.rgbd_rig(...).  A mask in `data.mask` is NOT warped: make it on the colour image, which is the aligned one."""

  def __init__(self, rig, zfar=np.inf):
    self.rig, self.zfar = rig, zfar

  def process(self, data):
    from .reproject import align_frame
    data.rgb, data.depth = align_frame(data.rgb, data.depth, self.rig, zfar=self.zfar)
    data.K = self.rig.K.copy()
    return data


class Detect(Processor):
  """Fills `data.mask` when there is none, from the depth image and the model alone (Utils.detect: depth templates of the model matched
  against the whole frame; geometry only - see foundationpose_amd/detect.py for the limits): the stage in front of FoundationPoseEstimator
  on a stream that nobody paints a mask for.  It acts on the first frame it sees without a mask and afterwards only on frames with
  `data.lost` set (a mask makes FoundationPoseEstimator register again), and leaves `data.detections` = Utils.detect's records; the mask
  is what the model shows at the best record's pose in front of the frame's depth (Utils.scene_instances).  A frame without a candidate
  keeps `data.mask` None.  Keywords of Utils.build_templates go to the template set (built at the first use), the others to Utils.detect."""

  def __init__(self, mesh_file=None, mesh=None, K=None, intrinsics_file=None, delta=0.015, **kw):
    from .mesh_io import load_intrinsics, load_obj
    self.mesh = load_obj(mesh_file) if mesh is None else mesh
    self.K = np.asarray(K, dtype=np.float64) if K is not None else (load_intrinsics(intrinsics_file) if intrinsics_file else None)
    self._build = {k: kw.pop(k) for k in ('n_views', 'inplane_step', 'n_in', 'n_out', 'anchors', 'margin_px', 'render_size', 'z0') if k in kw}
    self._kw, self.delta = kw, delta
    self.templates = self.mesh_tensors = None
    self._seen = False

  def process(self, data):
    from . import Utils as U
    if data.mask is not None or (self._seen and not getattr(data, 'lost', False)):
      return data
    self._seen = True
    if self.templates is None:
      centred = self.mesh.copy()
      centred.vertices = centred.vertices - (self.mesh.vertices.min(axis=0) + self.mesh.vertices.max(axis=0)) / 2      # as FoundationPose.reset_object
      self.mesh_tensors = U.make_mesh_tensors(centred)
      self.templates = U.build_templates(mesh_tensors=self.mesh_tensors, **self._build)
    K = self.K if data.K is None else np.asarray(data.K, dtype=np.float64)
    depth = np.ascontiguousarray(data.depth, dtype=np.float32)
    filtered = U.bilateral_filter_depth(U.erode_depth(depth, radius=2, device='cuda'), radius=2, device='cuda')      # register's prelude
    data.detections = U.detect(filtered, K, self.templates, **self._kw)
    if data.detections:
      H, W = depth.shape
      visib = U.scene_instances(K, H, W, self.mesh_tensors, data.detections[0]['ob_in_cam'][None], depth=depth, occluders='depth', delta=self.delta,
                                want=('mask_visib',))['mask_visib']
      data.mask = visib[0].cpu().numpy() > 0
    return data


class FoundationPoseEstimator(Processor):
  """Wraps foundationpose_amd.estimater.FoundationPose as a pipeline stage (what main.py:34-79 does by hand):
  first frame -> register(), later frames -> track_one().  box='aabb' draws the axis-aligned box of the model in `visualize`;
  box='oriented' draws the minimum-volume box of Utils.oriented_bounds, as main.py:38-39 does with trimesh, and `process` then also sets
  `data.center_pose = data.pose @ inv(to_origin)`, the matrix main.py:67 publishes."""

  def __init__(self, mesh_file=None, intrinsics_file=None, mesh=None, K=None, est_refine_iter=5, track_refine_iter=2,
               scorer=None, refiner=None, debug=0, box='aabb'):
    if box not in ('aabb', 'oriented'):
      raise ValueError(f"box must be 'aabb' or 'oriented', got {box!r}")
    self.box = box
    from .mesh_io import load_intrinsics, load_obj
    self.mesh = load_obj(mesh_file) if mesh is None else mesh
    self.K = np.asarray(K, dtype=np.float64) if K is not None else (load_intrinsics(intrinsics_file) if intrinsics_file else None)
    self.est_refine_iter, self.track_refine_iter = est_refine_iter, track_refine_iter
    self._kw = dict(scorer=scorer, refiner=refiner, debug=debug)
    self.est = None

  def process(self, data):
    from .estimater import FoundationPose
    K = self.K if data.K is None else np.asarray(data.K, dtype=np.float64)
    if self.est is None:
      self.est = FoundationPose(model_pts=self.mesh.vertices, model_normals=self.mesh.vertex_normals, mesh=self.mesh, **self._kw)
    if self.est.pose_last is None or data.mask is not None:
      data.pose = self.est.register(K=K, rgb=data.rgb, depth=data.depth, ob_mask=np.asarray(data.mask).astype(bool),
                                    iteration=self.est_refine_iter)
    else:
      data.pose = self.est.track_one(rgb=data.rgb, depth=data.depth, K=K, iteration=self.track_refine_iter)
    if self.box == 'oriented':
      data.center_pose = np.asarray(data.pose, dtype=np.float64).reshape(4, 4) @ np.linalg.inv(self.est.model_box(oriented=True)[0])
    return data

  def visualize(self, data):
    """The picture main.py:67-71 saves: the model's box and the xyz axes at `data.pose` on `data.rgb`; sets and returns `data.vis`."""
    from . import Utils as U
    K = self.K if data.K is None else np.asarray(data.K, dtype=np.float64)
    if self.box == 'oriented':
      to_origin, bbox = self.est.model_box(oriented=True) if self.est is not None else U.model_box(self.mesh, oriented=True)
    else:
      to_origin, bbox = U.model_box(self.mesh)
    data.vis = U.draw_poses(data.rgb, K, np.asarray(data.pose, dtype=np.float64).reshape(1, 4, 4), bboxes=bbox, offsets=np.linalg.inv(to_origin),
                            colors=(0, 255, 0))
    return data.vis
