"""CPU: the numpy restatement of the TSDF rule (tests/tsdf_oracle.py) against analytic truth - a sphere ray-cast in float64 - and the
argument checks of the fp_tsdf_* exports that need no GPU.  The GPU tests (tests/test_gpu_tsdf.py) hold the kernels to this restatement
bit for bit, so what is shown here about the rule holds for them."""
import ctypes

import numpy as np
import pytest

from tests import tsdf_oracle as O

DIMS, VOXEL = (35, 33, 37), 0.004


@pytest.fixture(scope='module')
def sphere():
  origin, K, poses, depths = O.sphere_case(DIMS, VOXEL)
  vol = O.Volume(origin, VOXEL, DIMS)
  vol.integrate(depths, K, poses)
  return vol, vol.extract(1)


def test_sphere_is_closed_outward_and_within_the_radial_bound(sphere):
  """Every edge in two faces, positive volume near 4/3 pi r^3, indices in range, every vertex referenced; the radial error of the
  restatement is 0.640 voxels here (12 views, 4 mm voxels, 5 cm sphere) and the assertion allows 1.5 x that = 0.96, under one voxel."""
  _, m = sphere
  err = O.check_closed_outward_sphere(m['vertices'], m['faces'], VOXEL, m['normals'])
  print(f'largest radial error: {err:.4f} voxels (bound {O.RADIAL_BOUND_VOXELS:.3f})')
  assert O.RADIAL_BOUND_VOXELS <= 1.0
  assert err <= O.RADIAL_BOUND_VOXELS
  assert O.components(m['faces'], len(m['vertices'])).max() == 0


def test_sphere_order_is_by_point_then_slot(sphere):
  """vertex ids ascend with the owning sample point: along every owned edge the vertex lies between the point and its +neighbour"""
  vol, m = sphere
  cell = np.floor((m['vertices'].astype(np.float64) - vol.origin.astype(np.float64)) / VOXEL + 1e-4).astype(np.int64)
  nx, ny, _ = DIMS
  lin = cell[:, 0] + nx * (cell[:, 1] + ny * cell[:, 2])
  assert (np.diff(lin) >= 0).mean() > 0.99      # (a vertex exactly on the far end of its edge floors into the next cell)


def test_single_view_of_a_plane_is_an_open_sheet():
  H, W = 60, 80
  K = np.array([[100.0, 0, 39.5], [0, 100.0, 29.5], [0, 0, 1]])
  depth = O.plane_depth(H, W, 0.3)[None]
  pose = np.eye(4)[None]                         # the camera at the object origin, looking along +z
  vol = O.Volume((-0.04, -0.03, 0.25), 0.004, (21, 17, 26))
  vol.integrate(depth, K, pose)
  m = vol.extract(1)
  assert len(m['faces']) > 0
  z = m['vertices'][:, 2]
  assert np.abs(z - 0.3).max() < 1e-6           # one sheet, at the plane: nothing behind it, where the view saw nothing
  _, counts = O.edge_use(m['faces'])
  assert set(np.unique(counts)) == {1, 2}       # open: it has a boundary
  assert (m['normals'][:, 2] < -0.99).all()     # towards the camera: from negative to positive TSDF
  v = m['vertices'][m['faces']].astype(np.float64)
  assert (np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])[:, 2] <= 0).all()
  # unobserved behind the sheet's band: weight 0 beyond trunc
  assert (vol.planes['weight'][-1] == 0).all() and (vol.planes['weight'][0] == 1).all()
  empty = vol.extract(2)                         # one view cannot give weight 2
  assert empty['vertices'].shape == (0, 3) and empty['faces'].shape == (0, 3)


def test_one_call_equals_one_call_per_view(sphere):
  vol, _ = sphere
  origin, K, poses, depths = O.sphere_case(DIMS, VOXEL)
  again = O.Volume(origin, VOXEL, DIMS)
  for v in range(len(poses)):
    again.integrate(depths[v:v + 1], K, poses[v:v + 1])
  for p in O.PLANES:
    assert np.array_equal(again.planes[p], vol.planes[p])


def test_case_table_is_consistent_across_tetrahedra():
  """every tetrahedron and sign case: 1 or 2 triangles on distinct sign-changing edges"""
  tab = O.case_table()
  assert len(tab) == 6 * 14
  for (p, m), tris in tab.items():
    neg = {q for q in range(4) if (m >> q) & 1}
    assert len(tris) == (2 if len(neg) == 2 else 1)
    for tri in tris:
      assert len(set(tri)) == 3 and all((a in neg) != (b in neg) for a, b in tri)


def test_restatement_stays_inside_the_mustard_caps():
  """The 12 poses of the GPU test (tests/test_gpu_tsdf.py), the views rendered by the CPU oracle's rasteriser and rounded to millimetres:
  the restatement alone leaves at most 1 % of the vertices beyond the radial bound and its largest component holds 99 % of the faces."""
  import torch
  from oracle.render import nvdiffrast_render as oracle_render
  from tests import util
  sc = util.scene(0)
  H, W = O.MUSTARD_HW
  cams = np.stack([O.look_at(e) for e in O.mustard_eyes()])
  _, depth, _ = oracle_render(K=O.MUSTARD_K, H=H, W=W, ob_in_cams=torch.as_tensor(np.linalg.inv(cams).astype(np.float32)), mesh_tensors=sc['mt'])
  depth = (np.round(depth.numpy().astype(np.float64) * 1e3) / 1e3).astype(np.float32)
  vs = O.MUSTARD_VOXEL
  lo, hi = sc['mesh'].vertices.min(0), sc['mesh'].vertices.max(0)
  vol = O.Volume(lo - 5 * vs, vs, np.ceil((hi - lo + 10 * vs) / vs).astype(int) + 1)
  vol.integrate(depth, O.MUSTARD_K, cams, masks=depth > 0)
  m = vol.extract(1)
  label = O.components(m['faces'], len(m['vertices']))
  used = np.unique(m['faces'][label == 0])
  out, far = O.fraction_beyond_bound(m['vertices'][used], sc['mesh'].vertices, sc['mesh'].faces, vs)
  print(f'beyond {O.RADIAL_BOUND_VOXELS:.2f} voxels: {out:.4f}; max {far:.2f} voxels; largest component {(label == 0).mean():.4f}')
  assert out <= 0.01 and (label == 0).mean() >= 0.99


@pytest.fixture(scope='module')
def built():
  import __graft_entry__ as g
  g.build()
  from foundationpose_amd import _lib
  return _lib


def test_argument_checks_need_no_gpu(built):
  L, EINVAL = built.lib(), built.FP_EINVAL
  origin = (ctypes.c_double * 3)(0, 0, 0)
  dims = (ctypes.c_int * 3)(8, 8, 8)
  h = ctypes.c_void_p()
  K = (ctypes.c_double * 9)(100, 0, 4, 0, 100, 4, 0, 0, 1)
  pose = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
  counts = (ctypes.c_int64 * 2)()
  fake = ctypes.c_void_p(64)                     # never dereferenced: the null checks come first
  assert L.fp_tsdf_create(None, origin, 0.004, dims, 0.016, ctypes.byref(h)) == EINVAL
  assert b'null' in L.fp_last_error()
  assert L.fp_tsdf_create(fake, None, 0.004, dims, 0.016, ctypes.byref(h)) == EINVAL
  assert L.fp_tsdf_create(fake, origin, 0.004, dims, 0.016, None) == EINVAL
  assert L.fp_tsdf_create(fake, origin, 0.004, (ctypes.c_int * 3)(8, 1, 8), 0.016, ctypes.byref(h)) == EINVAL
  assert L.fp_tsdf_create(fake, origin, 0.004, (ctypes.c_int * 3)(513, 512, 512), 0.016, ctypes.byref(h)) == EINVAL
  assert L.fp_tsdf_create(fake, origin, 0.0, dims, 0.016, ctypes.byref(h)) == EINVAL
  assert L.fp_tsdf_create(fake, origin, 0.004, dims, -1.0, ctypes.byref(h)) == EINVAL
  assert not h.value
  assert L.fp_tsdf_reset(None, fake, None) == EINVAL and L.fp_tsdf_reset(fake, None, None) == EINVAL
  assert L.fp_tsdf_integrate(None, fake, fake, None, None, 1, 8, 8, K, pose, 1.0, None) == EINVAL
  assert L.fp_tsdf_integrate(fake, None, fake, None, None, 1, 8, 8, K, pose, 1.0, None) == EINVAL
  assert L.fp_tsdf_extract_count(None, fake, 1.0, counts, None) == EINVAL
  assert L.fp_tsdf_extract_count(fake, None, 1.0, counts, None) == EINVAL
  assert L.fp_tsdf_extract_write(None, fake, fake, None, None, fake, 0, 0, None) == EINVAL
  assert L.fp_tsdf_extract_write(fake, None, fake, None, None, fake, 0, 0, None) == EINVAL
  assert L.fp_tsdf_read_plane(fake, None, 0, fake, None) == EINVAL
  assert L.fp_tsdf_destroy(None) == 0
  assert built.FP_TSDF_MAX_POINTS >= 512 ** 3
