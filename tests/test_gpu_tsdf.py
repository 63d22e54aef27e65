"""GPU: TSDF fusion and marching tetrahedra (csrc/tsdf.hip, foundationpose_amd/reconstruct.py) against the numpy restatement of the header's
rule (tests/tsdf_oracle.py), bit for bit where the rule is exact, and through the public layer from rendered views to a registered pose.

Shapes: 40 x 36 x 44 points (three different dims, none a multiple of a workgroup edge, 248 workgroups), 5 views of 96 x 128 with one
camera inside the volume (part of it behind the camera, part projecting outside the image), a mask on two views, a zfar that cuts valid
pixels, colours; 128 x 96 x 100 points for the scan (1 228 801 words: 1 201 block sums, more than the 1 024 of one workgroup, so the scan
recurses twice)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import tsdf_oracle as O

pytestmark = pytest.mark.gpu
DIMS, VOXEL, ZFAR = (40, 36, 44), 0.004, 0.62
H, W = 96, 128
K = np.array([[160.0, 0, 63.5], [0, 160.0, 47.5], [0, 0, 1.0]])


@pytest.fixture(scope='module')
def views():
  """5 views of the 5 cm sphere in front of a far plane at 0.6 m (every pixel valid; the plane is cut by ZFAR in view 2, where it is
  at 0.63), seeded smooth colours, a half-image mask on views 1 and 3; view 4 sits inside the volume, 7.5 cm from the centre."""
  eyes = np.concatenate([O.fibonacci_eyes(4, 0.4), [[0.075, 0.004, -0.006]]])
  poses = np.stack([O.look_at(e) for e in eyes])
  depths = np.stack([O.sphere_depth(p, K, H, W, O.SPHERE_RADIUS) for p in poses])
  for v in range(5):
    depths[v][depths[v] == 0] = 0.63 if v == 2 else 0.6
  rs = np.random.RandomState(5)
  vs, us = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
  rgbs = np.stack([np.stack([127.5 + 127.5 * np.sin(us * rs.uniform(0.05, 0.3) + vs * rs.uniform(0.05, 0.3) + rs.uniform(0, 6)) for _ in range(3)], -1)
                   for _ in range(5)]).astype(np.uint8)
  masks = np.ones((5, H, W), dtype=np.uint8)
  masks[1, :, :W // 2] = 0
  masks[3, H // 3:, :] = 0
  origin = -(np.array(DIMS) - 1) * VOXEL / 2 + np.array([0.0007, -0.0011, 0.0013])
  return dict(origin=origin, poses=poses, depths=depths, rgbs=rgbs, masks=masks)


@pytest.fixture(scope='module')
def oracle(views):
  vol = O.Volume(views['origin'], VOXEL, DIMS)
  vol.integrate(views['depths'], K, views['poses'], rgbs=views['rgbs'], masks=views['masks'], zfar=ZFAR)
  assert len(np.unique(vol.planes['weight'])) >= 4 and (vol.planes['weight'] == 0).any()      # unobserved points and several view counts occur
  return vol, vol.extract(1)


@pytest.fixture(scope='module')
def device_volume(views):
  from foundationpose_amd.reconstruct import TsdfVolume
  vol = TsdfVolume(views['origin'], VOXEL, DIMS)
  vol.integrate(views['depths'], K, views['poses'], rgbs=views['rgbs'], masks=views['masks'], zfar=ZFAR)
  return vol


def _planes(vol):
  return {p: vol.plane(p).cpu().numpy() for p in O.PLANES}


def _same_bits(a, b):
  return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_planes_are_bit_equal_to_the_restatement(device_volume, oracle):
  got = _planes(device_volume)
  for p in O.PLANES:
    want = oracle[0].planes[p]
    diff = np.abs(got[p].astype(np.float64) - want.astype(np.float64)).max()
    print(f'{p}: max |diff| {diff:.3e}, differing points {(got[p].view(np.uint32) != want.view(np.uint32)).sum()}')
    assert _same_bits(got[p], want), p
  assert torch.equal(device_volume.tsdf, device_volume.plane('tsdf')) and device_volume.weight.shape == DIMS[::-1]


def test_planes_under_a_camera_with_fx_not_fy():
  """Three of the views at 31 x 33 pixels through tsdf_oracle.skew_camera (fy = 1.25 fx, cx and cy off the middle by different amounts),
  colours and masks included: a kernel that takes fx for fy or cx for cy in the projection differs from the restatement."""
  from foundationpose_amd.reconstruct import TsdfVolume
  h, w = 31, 33
  Ks = O.skew_camera(h, w, 40.0)
  poses = np.stack([O.look_at(e) for e in O.fibonacci_eyes(3, 0.4)])
  depths = np.stack([O.sphere_depth(p, Ks, h, w, O.SPHERE_RADIUS) for p in poses])
  depths[depths == 0] = 0.6
  rs = np.random.RandomState(9)
  rgbs = rs.randint(0, 256, (3, h, w, 3)).astype(np.uint8)
  masks = np.ones((3, h, w), dtype=np.uint8)
  masks[1, :, :w // 2] = 0
  origin = -(np.array(DIMS) - 1) * VOXEL / 2 + np.array([0.0007, -0.0011, 0.0013])
  want = O.Volume(origin, VOXEL, DIMS)
  want.integrate(depths, Ks, poses, rgbs=rgbs, masks=masks, zfar=ZFAR)
  print(f"weights {np.unique(want.planes['weight'], return_counts=True)}")
  assert len(np.unique(want.planes['weight'])) >= 3 and (want.planes['color_weight'] > 0).any()
  vol = TsdfVolume(origin, VOXEL, DIMS)
  vol.integrate(depths, Ks, poses, rgbs=rgbs, masks=masks, zfar=ZFAR)
  got = _planes(vol)
  for p in O.PLANES:
    assert _same_bits(got[p], want.planes[p]), p


def test_one_call_is_five_calls_and_reset_repeats(device_volume, views):
  from foundationpose_amd.reconstruct import TsdfVolume
  want = _planes(device_volume)
  vol = TsdfVolume(views['origin'], VOXEL, DIMS)
  for v in range(5):
    vol.integrate(views['depths'][v:v + 1], K, views['poses'][v:v + 1], rgbs=views['rgbs'][v:v + 1], masks=views['masks'][v:v + 1], zfar=ZFAR)
  got = _planes(vol)
  for p in O.PLANES:
    assert _same_bits(got[p], want[p]), f'{p}: five calls of one view differ from one call of five'
  vol.reset()
  assert all((a == 0).all() for a in _planes(vol).values())
  vol.integrate(views['depths'], K, views['poses'], rgbs=views['rgbs'], masks=views['masks'], zfar=ZFAR)
  got = _planes(vol)
  for p in O.PLANES:
    assert _same_bits(got[p], want[p]), f'{p}: differs after reset'


def test_extraction_equals_the_restatement(device_volume, oracle):
  """counts, faces, vertices and colours exactly; normals within 1e-6 (unit-vector components, a handful of correctly rounded fp32
  operations at 6e-8 each).  The measured maximum is printed; on an MI355X it is 0: sqrt and / round alike on both sides."""
  want = oracle[1]
  v, n, c, f = (t.cpu().numpy() for t in device_volume.extract_arrays(1))
  assert (len(v), len(f)) == (len(want['vertices']), len(want['faces'])) and len(f) > 1000
  assert np.array_equal(f, want['faces'])
  assert _same_bits(v, want['vertices'])
  assert np.array_equal(c, want['colors']) and c.std() > 10
  dn = np.abs(n.astype(np.float64) - want['normals'].astype(np.float64)).max()
  print(f'normals: max |diff| {dn:.3e}')
  assert dn <= 1e-6
  # min_weight 2 leaves fewer observed points; min_weight 6 none
  w2 = oracle[0].extract(2)
  v2, _, _, f2 = (None if t is None else t.cpu().numpy() for t in device_volume.extract_arrays(2, normals=False, colors=False))
  assert np.array_equal(f2, w2['faces']) and _same_bits(v2, w2['vertices'])
  v6, _, _, f6 = device_volume.extract_arrays(6)
  assert v6.shape == (0, 3) and f6.shape == (0, 3)
  mesh = device_volume.extract_mesh(1)
  assert mesh.vertices.shape == v.shape and mesh.visual.vertex_colors.shape == (len(v), 4) and np.array_equal(mesh.faces, f)


def test_extract_write_needs_a_fresh_count(device_volume, views):
  from foundationpose_amd import _lib
  from foundationpose_amd._lib import lib, ptr, stream_ptr
  from foundationpose_amd.reconstruct import TsdfVolume
  vol = TsdfVolume(views['origin'], VOXEL, DIMS)
  dev = vol.device
  buf_v, buf_f = torch.empty((1 << 16, 3), device=dev), torch.empty((1 << 17, 3), dtype=torch.int32, device=dev)
  write = lambda nv, nf: lib().fp_tsdf_extract_write(vol.ctx.handle, vol.handle, ptr(buf_v), None, None, ptr(buf_f), nv, nf, stream_ptr(dev))
  assert write(0, 0) == _lib.FP_EINVAL                          # no count yet
  vol.integrate(views['depths'][:2], K, views['poses'][:2])
  counts = (ctypes.c_int64 * 2)()
  assert lib().fp_tsdf_extract_count(vol.ctx.handle, vol.handle, 1.0, counts, stream_ptr(dev)) == 0
  nv, nf = int(counts[0]), int(counts[1])
  assert 0 < nv < len(buf_v) and 0 < nf < len(buf_f)
  assert write(nv + 1, nf) == _lib.FP_EINVAL                    # counts disagree
  assert write(nv, nf) == 0
  vol.integrate(views['depths'][2:3], K, views['poses'][2:3])   # invalidates the count
  assert write(nv, nf) == _lib.FP_EINVAL
  vol.reset()
  assert write(nv, nf) == _lib.FP_EINVAL
  torch.cuda.synchronize()


def test_sphere_conditions_on_the_gpu_mesh():
  """closed, outward, within the radial bound: the host test's sphere, fused and extracted on the GPU"""
  from foundationpose_amd.reconstruct import TsdfVolume
  dims, voxel = (35, 33, 37), 0.004
  origin, Ks, poses, depths = O.sphere_case(dims, voxel)
  vol = TsdfVolume(origin, voxel, dims)
  vol.integrate(depths, Ks, poses)
  v, n, _, f = (t.cpu().numpy() for t in vol.extract_arrays(1))
  err = O.check_closed_outward_sphere(v, f, voxel, n)
  print(f'largest radial error: {err:.4f} voxels (bound {O.RADIAL_BOUND_VOXELS:.3f})')
  assert err <= O.RADIAL_BOUND_VOXELS


def test_scan_recurses_on_a_large_volume():
  """1.2 M points: the block sums of the first level exceed one workgroup's tile"""
  from foundationpose_amd.reconstruct import TsdfVolume
  dims, voxel = (128, 96, 100), 0.0011
  origin, Ks, poses, depths = O.sphere_case(dims, voxel)
  ref = O.Volume(origin, voxel, dims)
  ref.integrate(depths, Ks, poses)
  want = ref.extract(1)
  vol = TsdfVolume(origin, voxel, dims)
  vol.integrate(depths, Ks, poses)
  assert _same_bits(vol.plane('tsdf').cpu().numpy(), ref.planes['tsdf'])
  v, _, _, f = vol.extract_arrays(1, normals=False, colors=False)
  assert (len(v), len(f)) == (len(want['vertices']), len(want['faces'])) and len(f) > 200000
  assert np.array_equal(f.cpu().numpy(), want['faces'])
  assert _same_bits(v.cpu().numpy(), want['vertices'])
  assert (O.edge_use(want['faces'])[1] == 2).all()


# ---- the public layer: rendered views of the mustard bottle -> mesh -> estimator --------------------------------------------------
(MH, MW), MVOXEL, MK = O.MUSTARD_HW, O.MUSTARD_VOXEL, O.MUSTARD_K


@pytest.fixture(scope='module')
def mustard_views():
  from foundationpose_amd import Utils as U
  from tests import util
  sc = util.scene(0)
  cams = np.stack([O.look_at(e) for e in O.mustard_eyes()])
  ob_in_cams = np.linalg.inv(cams).astype(np.float32)
  color, depth, _ = U.nvdiffrast_render(K=MK, H=MH, W=MW, ob_in_cams=ob_in_cams, mesh_tensors=util.to_dev(sc['mt']))
  mm = np.round(depth.cpu().numpy().astype(np.float64) * 1e3).astype(np.uint16)       # what a 16-bit PNG in millimetres holds
  depths = (mm.astype(np.float64) / 1e3).astype(np.float32)
  rgbs = np.clip(np.round(color.cpu().numpy() * 255), 0, 255).astype(np.uint8)
  return dict(depths=depths, rgbs=rgbs, masks=(mm > 0).astype(np.uint8), K=MK, cam_in_obs=cams), sc


@pytest.fixture(scope='module')
def fused(mustard_views):
  from foundationpose_amd.reconstruct import reconstruct_object
  return reconstruct_object(mustard_views[0], voxel_size=MVOXEL)


def test_fused_mustard_lies_on_the_source_surface(mustard_views, fused):
  """Nearest-neighbour distance from the fused vertices to a dense sampling of the source triangles: within the sphere's bound
  (RADIAL_BOUND_VOXELS voxels) but for 1 % of the vertices at most (view-coverage seams); before the small components are dropped the
  largest one holds 99 % of the faces.  (The restatement alone on these poses: tests/test_tsdf_host.py.)"""
  from foundationpose_amd import reconstruct as R
  views, sc = mustard_views
  out, far = O.fraction_beyond_bound(fused.vertices, sc['mesh'].vertices, sc['mesh'].faces, MVOXEL)
  print(f'{len(fused.vertices)} vertices, {len(fused.faces)} faces; beyond {O.RADIAL_BOUND_VOXELS:.2f} voxels: {out:.4f}; max {far:.2f} voxels')
  assert len(fused.faces) > 5000 and fused.faces.max() == len(fused.vertices) - 1
  assert out <= 0.01
  origin, dims = R.volume_from_views(views['depths'], views['masks'], MK, views['cam_in_obs'], MVOXEL)
  vol = R.TsdfVolume(origin, MVOXEL, dims)
  vol.integrate(views['depths'], MK, views['cam_in_obs'], masks=views['masks'])
  _, _, _, f = vol.extract_arrays(1, normals=False, colors=False)
  keep = R.largest_component(f.cpu().numpy(), int(f.max()) + 1)
  print(f'largest component: {keep.mean():.4f} of the faces')
  assert keep.mean() >= 0.99
  with pytest.raises(ValueError, match='would fit'):
    R.volume_from_views(views['depths'], views['masks'], MK, views['cam_in_obs'], 1e-4)


def test_fused_mesh_registers(mustard_views, fused):
  """The fused mesh goes where a CAD model goes: make_mesh_tensors, FoundationPose, one register() on a synthetic frame.  Seeded random
  weights: no accuracy claim, a finite pose."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.config import REFINE_DEFAULT, SCORE_DEFAULT
  from foundationpose_amd.estimater import FoundationPose
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
  from foundationpose_amd.predict_score import ScorePredictor
  sc = mustard_views[1]
  mt = make_mesh_tensors(fused)
  assert mt['pos'].shape[1] == 3 and mt['vertex_color'].shape == mt['pos'].shape
  refiner = PoseRefinePredictor(state_dict=S.make_refine_state_dict(0), cfg=REFINE_DEFAULT)
  scorer = ScorePredictor(state_dict=S.make_score_state_dict(1), cfg=SCORE_DEFAULT)
  np.random.seed(0)
  est = FoundationPose(model_pts=fused.vertices, model_normals=fused.vertex_normals, mesh=fused, refiner=refiner, scorer=scorer)
  est.rot_grid = est.rot_grid[:8].contiguous()
  pose = est.register(K=sc['K'], rgb=sc['rgb'], depth=sc['depth'], ob_mask=sc['mask'], iteration=1)
  pose = np.asarray(pose)
  assert pose.shape == (4, 4) and np.isfinite(pose).all()


def test_reference_view_folder_round_trip(mustard_views, fused, tmp_path):
  """the same views written in the reference's layout and read back: the mesh is bit-identical to the in-memory run"""
  from PIL import Image
  from foundationpose_amd.reconstruct import load_reference_views, reconstruct_object
  views = mustard_views[0]
  for sub in ('rgb', 'depth', 'mask', 'cam_in_ob'):
    os.makedirs(tmp_path / sub)
  np.savetxt(tmp_path / 'K.txt', MK, fmt='%.18e')
  for v in range(len(views['depths'])):
    name = f'{v:04d}'
    Image.fromarray(views['rgbs'][v]).save(tmp_path / 'rgb' / f'{name}.png')
    Image.fromarray(np.round(views['depths'][v].astype(np.float64) * 1e3).astype(np.uint16)).save(tmp_path / 'depth' / f'{name}.png')
    Image.fromarray(views['masks'][v] * 255).save(tmp_path / 'mask' / f'{name}.png')
    np.savetxt(tmp_path / 'cam_in_ob' / f'{name}.txt', views['cam_in_obs'][v], fmt='%.18e')
  back = load_reference_views(str(tmp_path))
  for k in ('depths', 'rgbs', 'masks', 'cam_in_obs'):
    assert np.array_equal(back[k], views[k]), k
  mesh = reconstruct_object(str(tmp_path), voxel_size=MVOXEL)
  assert np.array_equal(mesh.vertices, fused.vertices) and np.array_equal(mesh.faces, fused.faces)
  assert np.array_equal(mesh.vertex_normals, fused.vertex_normals) and np.array_equal(mesh.visual.vertex_colors, fused.visual.vertex_colors)
