"""GPU: fp_mesh_simplify_count / _write and Utils.simplify_mesh against the numpy restatement (tests/mesh_simplify_oracle.py), bit for bit:
positions, normals, colours, faces and the vertex map.  The sums are integer, the numbering comes from scans: nothing may depend on the
order the device ran in, so equality is exact and two runs are the same bits."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mesh_simplify_oracle as M
from tests import tsdf_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mesh():
  return M.composite_mesh()


def _device(pos, faces, cell, normals=None, colors=None):
  from foundationpose_amd import Utils as U
  p, n, c, f, vm = U.simplify_mesh_arrays(pos, faces, cell, normals=normals, colors=colors, return_map=True)
  host = lambda t: None if t is None else t.cpu().numpy()
  return dict(pos=host(p), normals=host(n), colors=host(c), faces=host(f), vertex_map=host(vm))


def _assert_same(got, want):
  for k in ('pos', 'normals', 'colors', 'faces', 'vertex_map'):
    if want[k] is None:
      assert got[k] is None, k
      continue
    assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape, got[k].dtype, want[k].dtype)
    assert got[k].tobytes() == want[k].tobytes(), (k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize('cell', [0.0005, 0.003, 0.010])
def test_composite_mesh_is_bit_equal_to_the_restatement(mesh, cell):
  pos, faces, normals, colors = mesh
  want = M.simplify(pos, faces, cell, normals, colors)
  _assert_same(_device(pos, faces, cell, normals, colors), want)
  bare = _device(pos, faces, cell)
  want_bare = dict(want, normals=None, colors=None)
  _assert_same(bare, want_bare)


def test_vertices_on_cell_boundaries(mesh):
  """A lattice of pitch cell / 2 whose origin is a lattice point, all in exactly representable numbers: every float32 division is exact and
  every second vertex sits ON a cell boundary."""
  n, cell = 37, np.float32(0.0078125)                      # 2^-7; pitch 2^-8
  i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(3), indexing='ij')
  pos = (np.stack([i, j, k], -1).reshape(-1, 3) * 0.00390625 - 0.0625).astype(np.float32)
  idx = lambda a, b: (a * n + b) * 3
  a, b = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing='ij')
  a, b = a.reshape(-1), b.reshape(-1)
  faces = np.concatenate([np.stack([idx(a, b), idx(a + 1, b), idx(a, b + 1)], -1), np.stack([idx(a, b + 1) + 2, idx(a + 1, b) + 2, idx(a + 1, b + 1) + 2], -1)])
  want = M.simplify(pos, faces, cell)
  assert len(want['pos']) > 100 and want['degenerate'] > 0
  _assert_same(_device(pos, faces, cell), want)


@pytest.fixture(scope='module')
def cloud():
  return np.random.RandomState(7).uniform(-0.1, 0.1, size=((1 << 17) + 3, 3)).astype(np.float32)


def test_contended_sums_are_exact_and_repeat(cloud):
  """2^17 + 3 points into 8 clusters: sixteen thousand adds per accumulator."""
  cell = np.float32(0.11)
  normals = np.random.RandomState(8).uniform(-1, 1, size=cloud.shape).astype(np.float32)
  colors = np.random.RandomState(9).randint(0, 256, size=cloud.shape).astype(np.uint8)
  want = M.simplify(cloud, None, cell, normals, colors)
  assert len(want['pos']) == 8
  a, b = _device(cloud, None, cell, normals, colors), _device(cloud, None, cell, normals, colors)
  _assert_same(a, b)
  _assert_same(a, want)


def test_every_point_its_own_cluster(cloud):
  """A table at its fullest: as many clusters as vertices."""
  cell = np.float32(0.2 / (1 << 20))                       # 2^20 cells along an axis: 2^60 cells for 2^17 points
  assert M.simplify(cloud, None, cell)['clusters'] == len(cloud)
  out = _device(cloud, None, cell)
  assert out['pos'].tobytes() == cloud.tobytes()
  assert (out['vertex_map'] == np.arange(len(cloud))).all() and len(out['faces']) == 0


def test_edge_cases():
  from foundationpose_amd import _lib
  one = np.array([[0.25, -1.0, 3.0]], dtype=np.float32)
  out = _device(one, None, 0.01)
  assert out['pos'].tobytes() == one.tobytes() and out['vertex_map'].tolist() == [0]
  tri = np.array([[0, 0, 0], [0.001, 0, 0], [0, 0.001, 0], [0.001, 0.001, 0.001]], dtype=np.float32)
  f = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)
  out = _device(tri, f, 1.0)                               # one cell for everything: 1 cluster, 0 faces, hence 0 vertices
  assert out['pos'].shape == (0, 3) and out['faces'].shape == (0, 3) and (out['vertex_map'] == -1).all()
  _assert_same(out, dict(M.simplify(tri, f, 1.0), normals=None, colors=None))
  out = _device(tri, None, 1.0)
  assert out['pos'].shape == (1, 3) and (out['vertex_map'] == 0).all()
  with pytest.raises(_lib.FoundationPoseAmdError, match=r'a cell of [0-9.e+-]+ fits'):
    _device(tri, f, 1e-10)
  with pytest.raises(_lib.FoundationPoseAmdError, match='outside 0'):
    _device(tri, np.array([[0, 1, 4]], dtype=np.int32), 0.0005)
  assert len(_device(tri, f, 0.0005)['pos']) == 4          # the context still works


def test_one_context_serves_meshes_of_changing_size():
  """One context, four count / write rounds - 4, 3 002, 4 and 9 002 vertices: the first allocation of the tables and of the sums, growth
  by free and malloc, big blobs under a small layout (every offset moves, stale contents lie behind it) and growth again; the scan has
  1, 3, 1 and 9 blocks.  Every round equals the restatement, and the tiny rounds are the same bits."""
  from tests import util
  rs = np.random.RandomState(61)
  tiny, mid, big = [(v, f, n, rs.randint(0, 256, size=v.shape).astype(np.uint8)) for v, f, n in (M.lattice_sheet(2), M.uv_sphere(30, 100), M.uv_sphere(60, 150))]
  rounds = [tiny, mid, tiny, big]
  assert [len(r[0]) for r in rounds] == [4, 3002, 4, 9002]
  cells = [0.001, 0.004, 0.001, 0.003]                                   # pitch 1.1 mm: the sheet keeps its 4 vertices
  with util.own_context():
    got = []
    for (v, f, n, c), cell in zip(rounds, cells):
      want = M.simplify(v, f, cell, n, c)
      got.append(_device(v, f, cell, n, c))
      _assert_same(got[-1], want)
      assert 0 < len(want['faces']) <= len(f) and (len(v) == 4) == (len(want['pos']) == len(v))
  _assert_same(got[2], got[0])


def test_write_needs_its_own_fresh_count(mesh):
  from foundationpose_amd import _lib
  from foundationpose_amd._lib import lib, ptr, stream_ptr
  dev = torch.device('cuda', torch.cuda.current_device())
  ctx = _lib.Context.get(dev)
  pos, faces = torch.as_tensor(mesh[0], device=dev), torch.as_tensor(mesh[1], device=dev)
  other = pos.clone()
  V, F = len(pos), len(faces)
  counts = (ctypes.c_int64 * 2)()

  def count(p, cell):
    return lib().fp_mesh_simplify_count(ctx.handle, ptr(p), V, ptr(faces), F, cell, counts, stream_ptr(dev))

  def write(p, cell, nv, nf):
    o_pos = torch.empty((max(nv, 1), 3), dtype=torch.float, device=dev)
    o_faces = torch.empty((max(nf, 1), 3), dtype=torch.int32, device=dev)
    rc = lib().fp_mesh_simplify_write(ctx.handle, ptr(p), None, None, V, ptr(faces), F, cell, ptr(o_pos), None, None, ptr(o_faces), None, nv, nf,
                                      stream_ptr(dev))
    return rc, o_pos[:nv], o_faces[:nf]

  assert count(pos, 1e-10) == _lib.FP_EINVAL                # a failed count leaves nothing to write from
  assert write(pos, 1e-10, 0, 0)[0] == _lib.FP_EINVAL
  assert count(pos, 0.003) == 0
  nv, nf = int(counts[0]), int(counts[1])
  assert write(pos, 0.004, nv, nf)[0] == _lib.FP_EINVAL     # another cell
  assert write(pos, 0.003, nv + 1, nf)[0] == _lib.FP_EINVAL
  assert write(pos, 0.003, nv, nf - 1)[0] == _lib.FP_EINVAL
  assert write(other, 0.003, nv, nf)[0] == _lib.FP_EINVAL   # another mesh
  assert b'fp_mesh_simplify_write' in lib().fp_last_error()
  rc, p, f = write(pos, 0.003, nv, nf)
  assert rc == 0
  want = M.simplify(mesh[0], mesh[1], 0.003)
  assert p.cpu().numpy().tobytes() == want['pos'].tobytes() and f.cpu().numpy().tobytes() == want['faces'].tobytes()


def test_max_vertices_search(mesh):
  from foundationpose_amd import Utils as U
  pos, faces, normals, colors = mesh
  cell, lo, hi = M.search_cell(pos, faces, 2048)
  want = M.simplify(pos, faces, cell, normals, colors)
  out, info, vmap = U.simplify_mesh((pos, faces, normals, colors), max_vertices=2048, return_map=True)
  assert np.float32(info['cell']) == cell and info['evaluations'] == 21
  assert info['vertices'] == len(want['pos']) <= 2048 and info['faces'] == len(want['faces'])
  assert (info['vertices_in'], info['faces_in']) == (len(pos), len(faces))
  assert out.vertices.astype(np.float32).tobytes() == want['pos'].tobytes()
  assert out.vertex_normals.astype(np.float32).tobytes() == want['normals'].tobytes()
  assert out.visual.vertex_colors[:, :3].tobytes() == want['colors'].tobytes() and (out.visual.vertex_colors[:, 3] == 255).all()
  assert out.faces.astype(np.int32).tobytes() == want['faces'].tobytes()
  assert vmap.tobytes() == want['vertex_map'].tobytes()
  # already within the budget: the input arrays, unchanged
  same, info = U.simplify_mesh((pos, faces, normals, colors), max_vertices=len(pos))
  assert info['cell'] == 0 and info['evaluations'] == 0 and info['vertices'] == len(pos)
  assert (same.vertices == pos).all() and (same.faces == faces).all() and (same.vertex_normals == normals).all()
  assert (same.visual.vertex_colors[:, :3] == colors).all()
  with pytest.raises(ValueError):
    U.simplify_mesh((pos, faces), max_vertices=7)
  with pytest.raises(ValueError):
    U.simplify_mesh((pos, faces))
  with pytest.raises(ValueError):
    U.simplify_mesh((pos, faces), cell=0.01, max_vertices=100)


# ---- the public layer: rendered views of the mustard bottle -> simplified mesh -> estimator ----------------------------------------
(MH, MW), MVOXEL, MK = O.MUSTARD_HW, O.MUSTARD_VOXEL, O.MUSTARD_K


def test_reconstruct_object_to_a_vertex_budget():
  from foundationpose_amd import Utils as U
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.config import REFINE_DEFAULT, SCORE_DEFAULT
  from foundationpose_amd.estimater import FoundationPose
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
  from foundationpose_amd.predict_score import ScorePredictor
  from foundationpose_amd.reconstruct import reconstruct_object
  from tests import util
  sc = util.scene(0)
  cams = np.stack([O.look_at(e) for e in O.mustard_eyes()])
  ob_in_cams = np.linalg.inv(cams).astype(np.float32)
  color, depth, _ = U.nvdiffrast_render(K=MK, H=MH, W=MW, ob_in_cams=ob_in_cams, mesh_tensors=util.to_dev(sc['mt']))
  mm = np.round(depth.cpu().numpy().astype(np.float64) * 1e3).astype(np.uint16)
  views = dict(depths=(mm.astype(np.float64) / 1e3).astype(np.float32), rgbs=np.clip(np.round(color.cpu().numpy() * 255), 0, 255).astype(np.uint8),
               masks=(mm > 0).astype(np.uint8), K=MK, cam_in_obs=cams)
  full = reconstruct_object(views, voxel_size=MVOXEL)
  N = len(full.vertices) // 2
  small = reconstruct_object(views, voxel_size=MVOXEL, max_vertices=N)
  assert 8 <= len(small.vertices) <= N
  f = small.faces
  assert len(f) > 0 and f.min() >= 0 and f.max() == len(small.vertices) - 1 and len(np.unique(f)) == len(small.vertices)
  assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()
  assert len(np.unique(np.sort(f, axis=1), axis=0)) == len(f)
  again, info = U.simplify_mesh(full, max_vertices=N)
  assert small.vertices.tobytes() == again.vertices.tobytes() and small.faces.tobytes() == again.faces.tobytes()
  assert small.vertex_normals.tobytes() == again.vertex_normals.tobytes()
  assert small.visual.vertex_colors.tobytes() == again.visual.vertex_colors.tobytes()
  fixed = reconstruct_object(views, voxel_size=MVOXEL, simplify_cell=info['cell'])
  assert fixed.vertices.tobytes() == small.vertices.tobytes() and fixed.faces.tobytes() == small.faces.tobytes()

  # what the simplification costs in the image: renders of both meshes at the 12 views (printed for DESIGN.md, not asserted)
  _, d_full, _ = U.nvdiffrast_render(K=MK, H=MH, W=MW, ob_in_cams=ob_in_cams, mesh_tensors=make_mesh_tensors(full))
  _, d_small, _ = U.nvdiffrast_render(K=MK, H=MH, W=MW, ob_in_cams=ob_in_cams, mesh_tensors=make_mesh_tensors(small))
  a, b = d_full.cpu().numpy() > 0, d_small.cpu().numpy() > 0
  both = a & b
  dd = np.abs(d_full.cpu().numpy() - d_small.cpu().numpy())[both]
  print(f'{len(full.vertices)} -> {len(small.vertices)} vertices, {len(full.faces)} -> {len(small.faces)} faces at cell {info["cell"] * 1e3:.3f} mm; '
        f'mask IoU {both.sum() / max((a | b).sum(), 1):.4f}, median |ddepth| {np.median(dd) * 1e3:.3f} mm, 95 % {np.percentile(dd, 95) * 1e3:.3f} mm')

  mt = make_mesh_tensors(small)
  assert mt['pos'].shape == (len(small.vertices), 3) and mt['vertex_color'].shape == mt['pos'].shape
  refiner = PoseRefinePredictor(state_dict=S.make_refine_state_dict(0), cfg=REFINE_DEFAULT)
  scorer = ScorePredictor(state_dict=S.make_score_state_dict(1), cfg=SCORE_DEFAULT)
  np.random.seed(0)
  est = FoundationPose(model_pts=small.vertices, model_normals=small.vertex_normals, mesh=small, refiner=refiner, scorer=scorer)
  est.rot_grid = est.rot_grid[:8].contiguous()
  pose = np.asarray(est.register(K=sc['K'], rgb=sc['rgb'], depth=sc['depth'], ob_mask=sc['mask'], iteration=1))
  assert pose.shape == (4, 4) and np.isfinite(pose).all()
