"""GPU: fp_mesh_components_count / _write, Utils.mesh_components / clean_mesh_arrays / clean_mesh and reconstruct_object(components=...)
against the numpy / scipy restatement (tests/mesh_components_oracle.py), bit for bit: positions, normals, colours, faces, the vertex map,
labels and stats.  The final root of the union-find is the minimum of its component whatever order the device ran in, the numberings
come from scans and the counts are integer: equality is exact and two runs are the same bits."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mesh_components_oracle as C
from tests import mesh_simplify_oracle as M
from tests import tsdf_oracle as O

pytestmark = pytest.mark.gpu

KEYS = ('pos', 'normals', 'colors', 'faces', 'vertex_map', 'labels', 'stats')


def _device(pos, faces, normals=None, colors=None, **rule):
  from foundationpose_amd import Utils as U
  p, n, c, f, vm = U.clean_mesh_arrays(pos, faces, normals=normals, colors=colors, return_map=True, **rule)
  labels, stats = U.mesh_components((pos, faces))
  host = lambda t: None if t is None else t.cpu().numpy()
  return dict(pos=host(p), normals=host(n), colors=host(c), faces=host(f), vertex_map=host(vm), labels=host(labels), stats=host(stats))


def _assert_same(got, want):
  for k in KEYS:
    if want[k] is None:
      assert got[k] is None, k
      continue
    assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape, got[k].dtype, want[k].dtype)
    assert got[k].tobytes() == want[k].tobytes(), (k, int((got[k] != want[k]).sum()))


def _check(V, faces, seed=11, **rule):
  pos, normals, colors = C.positions(V, seed)
  want = C.components(pos, faces, normals, colors, **rule)
  got = _device(pos, faces, normals, colors, **rule)
  _assert_same(got, want)
  return got, want


RULES = [dict(keep='largest'), dict(keep='all', min_fraction=0.05), dict(keep='all', min_faces=1)]


@pytest.fixture(scope='module')
def composite():
  pos, faces, normals, colors = M.composite_mesh()
  perm = np.random.RandomState(5).permutation(len(pos))      # new index of every vertex
  inv = np.argsort(perm)
  return {False: (pos, faces, normals, colors), True: (pos[inv], perm[faces].astype(np.int32), normals[inv], colors[inv])}


@pytest.mark.parametrize('rule', RULES, ids=['largest', 'fraction', 'all'])
@pytest.mark.parametrize('permute', [False, True], ids=['as_is', 'permuted'])
def test_composite_mesh_is_bit_equal_to_the_restatement(composite, permute, rule):
  pos, faces, normals, colors = composite[permute]
  want = C.components(pos, faces, normals, colors, **rule)
  assert want['counts'][0] == 4 and want['counts'][1] == {'largest': 1, 'all': 3}[rule['keep']]      # sphere, two sheets, one lone vertex
  _assert_same(_device(pos, faces, normals, colors, **rule), want)
  _assert_same(_device(pos, faces, **rule), dict(want, normals=None, colors=None))


@pytest.mark.parametrize('order', ['reversed', 'shuffled'])
def test_the_minimum_travels_a_whole_strip(order):
  """4096 faces in a row: the lowest index sits at the far end (reversed) or anywhere (shuffled); every vertex must end with it."""
  n = 4096
  idx = np.arange(n + 2)[::-1] if order == 'reversed' else np.random.RandomState(21).permutation(n + 2)
  V, faces = C.strip(n, idx)
  got, want = _check(V, faces, keep='all')
  assert (got['labels'] == 0).all() and got['stats'].tolist() == [[n + 2, n]] and len(got['faces']) == n


def test_one_contended_root_and_two_runs_are_the_same_bits():
  """2^17 faces around the hub V - 1: every union meets the same tree, and its root must end at vertex 0 on the rim."""
  V, faces = C.fan(1 << 17)
  assert faces[:, 0].min() == V - 1 and faces[0, 1] == 0
  a, want = _check(V, faces, keep='largest')
  assert (a['labels'] == 0).all() and a['stats'].tolist() == [[V, 1 << 17]]
  pos, normals, colors = C.positions(V)
  _assert_same(_device(pos, faces, normals, colors, keep='largest'), a)


def test_many_small_components():
  V, faces = C.soup(3000, 500)
  got, want = _check(V, faces, keep='all', min_faces=1)
  assert got['stats'].shape == (3500, 2) and sorted(np.unique(got['stats'], axis=0).tolist()) == [[1, 0], [3, 1]]
  roots = np.nonzero(got['labels'] == np.arange(V))[0]
  assert len(roots) == 3500 and (got['labels'][faces].min(1) == got['labels'][faces].max(1)).all()
  assert (got['labels'][faces[:, 0]] == faces.min(1)).all()                        # the lowest member names the component
  named = np.zeros(V, dtype=bool)
  named[faces.reshape(-1)] = True
  assert ((got['vertex_map'] >= 0) == named).all() and len(got['pos']) == 9000 and len(got['faces']) == 3000
  # all 3000 tie at one face: 'largest' takes the lowest-numbered component that has a face
  one, _ = _check(V, faces, keep='largest')
  first = int(np.nonzero(got['stats'][:, 1] == 1)[0][0])
  kept = np.nonzero(one['vertex_map'] >= 0)[0]
  assert len(kept) == 3 and one['labels'][kept].tolist() == [roots[first]] * 3 and len(one['faces']) == 1
  assert roots[first] == np.nonzero(named)[0][0]


def test_tie_goes_to_the_lower_component_number():
  V, faces = C.tie_case()
  got, _ = _check(V, faces, keep='largest')
  assert (got['vertex_map'] >= 0).tolist() == [True, False] * 5 and got['faces'].tolist() == [[0, 1, 2], [1, 2, 3], [2, 3, 4]]


@pytest.mark.parametrize('name', ['bow_tie', 'isolated', 'degenerate', 'repeated'])
def test_small_graphs(name):
  V, faces = C.small_cases()[name]
  for rule in RULES + [dict(keep='all', min_faces=2), dict(keep='largest', min_faces=4)]:
    _check(V, faces, **rule)


def test_threshold_at_the_exact_boundary():
  """8 faces, 2 faces and 1 face: 0.25 * 8 is 2.0 exactly, the next float32 above 0.25 drops the component of 2."""
  strip8, strip2 = C.strip(8, np.arange(10))[1], C.strip(2, np.arange(4))[1] + 10
  faces = np.concatenate([strip2, strip8, np.array([[14, 15, 16]], dtype=np.int32)])
  up = float(np.nextafter(np.float32(0.25), np.float32(1)))
  got, _ = _check(17, faces, keep='all', min_fraction=0.25)
  assert len(got['faces']) == 10
  got, _ = _check(17, faces, keep='all', min_fraction=up)
  assert len(got['faces']) == 8


def test_scan_block_boundaries():
  """2^18 + 3 vertices of which a few hundred are named, among them the neighbours of the scan's tile edges and the last vertex."""
  V = (1 << 18) + 3
  rs = np.random.RandomState(31)
  edge = np.array([0, 1023, 1024, 1025, 2047, 2048, (1 << 18) - 1, 1 << 18, V - 1, 255, 256])
  named = np.unique(np.concatenate([edge, rs.choice(V, 300, replace=False)]))
  idx = rs.permutation(named)
  pieces = [C.strip(len(p) - 2, p)[1] for p in np.array_split(idx, 3)]
  faces = np.concatenate(pieces)
  got, want = _check(V, faces, keep='all', min_fraction=0.5)
  assert want['counts'][0] == V - len(named) + 3 and want['counts'][1] == 3 and len(got['pos']) == len(named)
  _check(V, faces, keep='largest')


def test_one_context_serves_meshes_of_changing_size():
  """One context, four count / write rounds - 4, 3 000, 4 and 9 002 vertices: the first allocation of the state, growth by free and
  malloc, a big blob under a small layout (every offset moves, stale contents lie behind it) and growth again; the scan has 1, 3, 1
  and 9 blocks.  Every round equals the restatement, and the tiny rounds are the same bits."""
  from tests import util
  tiny = (4, np.array([[3, 1, 2]], dtype=np.int32))                      # vertex 0 is named by no face
  strip_v, strip_f = C.strip(2998, np.random.RandomState(41).permutation(3000))
  soup_v, soup_f = C.soup(2834, 500, seed=43)
  assert (strip_v, soup_v) == (3000, 9002)
  rounds = [tiny, (strip_v, strip_f), tiny, (soup_v, soup_f)]
  rule = dict(keep='all', min_faces=1)
  with util.own_context():
    got = [_check(V, faces, seed=V, **rule)[0] for V, faces in rounds]
  _assert_same(got[2], got[0])
  assert [len(g['stats']) for g in got] == [2, 1, 2, 2834 + 500]


def test_empty_inputs():
  from foundationpose_amd import Utils as U
  pos = C.positions(5)[0]
  got = _device(pos, None)
  _assert_same(got, C.components(pos, None))
  assert got['labels'].tolist() == [0, 1, 2, 3, 4] and got['stats'].tolist() == [[1, 0]] * 5 and got['pos'].shape == (0, 3)
  got = _device(np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32))
  assert got['pos'].shape == (0, 3) and got['faces'].shape == (0, 3) and got['labels'].shape == (0,) and got['stats'].shape == (0, 2)
  mesh, info = U.clean_mesh((pos, None))
  assert (info['components'], info['kept_components'], info['vertices'], info['faces'], info['component_faces']) == (5, 0, 0, 0, [])


def test_errors():
  from foundationpose_amd import _lib
  from foundationpose_amd._lib import lib, ptr, stream_ptr
  dev = torch.device('cuda', torch.cuda.current_device())
  ctx = _lib.Context.get(dev)
  V, f = C.small_cases()['isolated']
  pos, normals, _ = C.positions(V)
  pos, normals = torch.as_tensor(pos, device=dev), torch.as_tensor(normals, device=dev)
  counts = (ctypes.c_int64 * 4)()

  def count(faces, V, min_faces=1, frac=0.0, largest=0):
    return lib().fp_mesh_components_count(ctx.handle, ptr(faces), len(faces), V, min_faces, frac, largest, counts, stream_ptr(dev))

  def write(faces, nv, nf, p=pos, nrm_in=None, nrm_out=False, V=V):
    o_pos = torch.empty((max(nv, 1), 3), dtype=torch.float, device=dev)
    o_nrm = torch.empty((max(nv, 1), 3), dtype=torch.float, device=dev) if nrm_out else None
    o_faces = torch.empty((max(nf, 1), 3), dtype=torch.int32, device=dev)
    rc = lib().fp_mesh_components_write(ctx.handle, ptr(p), ptr(nrm_in), None, V, ptr(faces), len(faces), ptr(o_pos), ptr(o_nrm), None, ptr(o_faces),
                                        None, None, None, nv, nf, stream_ptr(dev))
    return rc, o_pos[:nv], o_faces[:nf]

  good = torch.as_tensor(f, device=dev)
  fresh = _lib.Context(dev.index)                             # a context that has never counted
  o = torch.empty((6, 3), dtype=torch.float, device=dev)
  assert lib().fp_mesh_components_write(fresh.handle, ptr(pos), None, None, V, ptr(good), len(good), ptr(o), None, None, ptr(o), None, None, None, 6, 2,
                                        stream_ptr(dev)) == _lib.FP_EINVAL
  assert b'no fp_mesh_components_count' in lib().fp_last_error()
  assert lib().fp_ctx_destroy(fresh.handle) == 0
  for bad in (V, -1):
    faces = torch.as_tensor(np.array([[1, 2, 3], [7, bad, 6]], dtype=np.int32), device=dev)
    assert count(faces, V) == _lib.FP_EINVAL and b'outside 0' in lib().fp_last_error()
    assert write(faces, 0, 0)[0] == _lib.FP_EINVAL            # a failed count leaves nothing to write from
  assert count(good, _lib.FP_MESH_COMPONENTS_MAX_VERTICES + 1) == _lib.FP_EINVAL
  assert count(good, V, min_faces=0) == _lib.FP_EINVAL and count(good, V, frac=1.5) == _lib.FP_EINVAL
  assert count(good, V, frac=float('nan')) == _lib.FP_EINVAL and count(good, V, largest=2) == _lib.FP_EINVAL
  assert count(good, V) == 0 and list(counts) == [5, 2, 6, 2]
  assert write(good, 7, 2)[0] == _lib.FP_EINVAL               # a wrong n_vertices
  assert write(good, 6, 1)[0] == _lib.FP_EINVAL
  assert write(good.clone(), 6, 2)[0] == _lib.FP_EINVAL       # another mesh
  assert write(good, 6, 2, V=V + 1)[0] == _lib.FP_EINVAL
  assert write(good, 6, 2, nrm_out=True)[0] == _lib.FP_EINVAL      # a normals output without its input
  assert b'fp_mesh_components_write' in lib().fp_last_error()
  rc, p, faces = write(good, 6, 2, nrm_in=normals, nrm_out=True)
  assert rc == 0
  want = C.components(pos.cpu().numpy(), f, keep='all')
  assert p.cpu().numpy().tobytes() == want['pos'].tobytes() and faces.cpu().numpy().tobytes() == want['faces'].tobytes()


# ---- the public layer --------------------------------------------------------------------------------------------------------------
(MH, MW), MVOXEL, MK = O.MUSTARD_HW, O.MUSTARD_VOXEL, O.MUSTARD_K


@pytest.fixture(scope='module')
def mustard():
  """The 12 rendered views of tests/test_gpu_tsdf.py and the mesh the host path makes of them: extract_mesh -> largest_component -> the
  cumsum re-index, in numpy."""
  from foundationpose_amd import Utils as U
  from foundationpose_amd import reconstruct as R
  from foundationpose_amd.synthetic import SimpleMesh
  from tests import util
  sc = util.scene(0)
  cams = np.stack([O.look_at(e) for e in O.mustard_eyes()])
  ob_in_cams = np.linalg.inv(cams).astype(np.float32)
  color, depth, _ = U.nvdiffrast_render(K=MK, H=MH, W=MW, ob_in_cams=ob_in_cams, mesh_tensors=util.to_dev(sc['mt']))
  mm = np.round(depth.cpu().numpy().astype(np.float64) * 1e3).astype(np.uint16)
  views = dict(depths=(mm.astype(np.float64) / 1e3).astype(np.float32), rgbs=np.clip(np.round(color.cpu().numpy() * 255), 0, 255).astype(np.uint8),
               masks=(mm > 0).astype(np.uint8), K=MK, cam_in_obs=cams)
  return views, _host_path(views, MVOXEL, True)


def _host_path(views, voxel, depth_filter):
  from foundationpose_amd import reconstruct as R
  from foundationpose_amd.synthetic import SimpleMesh
  dev = torch.device('cuda', torch.cuda.current_device())
  depths = R._fusion_depths(R._eroded_depths(views, depth_filter, dev), depth_filter, dev)
  origin, dims = R.volume_from_views(depths, views.get('masks'), views['K'], views['cam_in_obs'], voxel, device=dev)
  vol = R.TsdfVolume(origin, voxel, dims, device=dev)
  vol.integrate(depths, views['K'], views['cam_in_obs'], rgbs=views.get('rgbs'), masks=views.get('masks'))
  mesh = vol.extract_mesh(1)
  keep = R.largest_component(mesh.faces, len(mesh.vertices))
  if len(keep) and not keep.all():
    faces = mesh.faces[keep]
    used = np.zeros(len(mesh.vertices), dtype=bool)
    used[faces.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    mesh = SimpleMesh(mesh.vertices[used], new_id[faces], vertex_normals=mesh.vertex_normals[used], vertex_colors=mesh.visual.vertex_colors[used])
  return mesh, (origin, dims)


def _same_mesh(a, b):
  assert a.vertices.dtype == b.vertices.dtype and a.vertices.tobytes() == b.vertices.tobytes()
  assert a.faces.dtype == b.faces.dtype and a.faces.tobytes() == b.faces.tobytes()
  assert a.vertex_normals.tobytes() == b.vertex_normals.tobytes()
  assert a.visual.vertex_colors.dtype == b.visual.vertex_colors.dtype and a.visual.vertex_colors.tobytes() == b.visual.vertex_colors.tobytes()


def test_reconstruct_object_is_unchanged_by_default(mustard):
  from foundationpose_amd.reconstruct import reconstruct_object
  views, (want, _) = mustard
  assert len(want.faces) > 5000
  _same_mesh(reconstruct_object(views, voxel_size=MVOXEL), want)


def test_reconstruct_object_to_a_budget_is_unchanged(mustard):
  from foundationpose_amd import Utils as U
  from foundationpose_amd.reconstruct import reconstruct_object
  views, (want, _) = mustard
  assert len(want.vertices) > 8192
  _same_mesh(reconstruct_object(views, voxel_size=MVOXEL, max_vertices=8192), U.simplify_mesh(want, max_vertices=8192)[0])


SPHERE_R, SPHERE_VOXEL = 0.03, 0.004


@pytest.fixture(scope='module')
def two_spheres():
  """Spheres of radius 30 mm and 24 mm, 3 radii apart, and a 6 mm bead beside them, seen by 6 cameras of tests/tsdf_oracle.py's sphere
  set-up; no depth filter, so that the restatement of the fusion sees what the device sees."""
  H, W = O.SPHERE_HW
  K = np.array([[O.SPHERE_F, 0, W / 2 - 0.5], [0, O.SPHERE_F, H / 2 - 0.5], [0, 0, 1.0]])
  balls = [((-1.5 * SPHERE_R, 0, 0), SPHERE_R), ((1.5 * SPHERE_R, 0, 0), 0.8 * SPHERE_R), ((0.0, 0.055, 0.02), 0.006)]
  poses = np.stack([O.look_at(e) for e in O.fibonacci_eyes(6, O.SPHERE_DIST)])
  depths = []
  for p in poses:
    ds = np.stack([O.sphere_depth(p, K, H, W, r, c) for c, r in balls])
    near = np.where(ds > 0, ds, np.inf).min(0)
    depths.append(np.where(np.isfinite(near), near, 0).astype(np.float32))
  depths = np.stack(depths)
  rgbs = np.random.RandomState(17).randint(0, 256, size=depths.shape + (3,)).astype(np.uint8)
  return dict(depths=depths, rgbs=rgbs, masks=(depths > 0).astype(np.uint8), K=K, cam_in_obs=poses)


def test_a_second_part_is_kept(two_spheres):
  from foundationpose_amd.reconstruct import reconstruct_object
  views = two_spheres
  host, (origin, dims) = _host_path(views, SPHERE_VOXEL, False)
  # the restatement of the fusion on the CPU, before relying on the scene: exactly two components above 20 % of the largest, and floaters
  ref = O.Volume(origin, SPHERE_VOXEL, dims)
  ref.integrate(views['depths'], views['K'], views['cam_in_obs'], rgbs=views['rgbs'], masks=views['masks'])
  m = ref.extract(1)
  want = C.components(m['vertices'], m['faces'], m['normals'], m['colors'], keep='all', min_fraction=0.2)
  nf = np.sort(want['stats'][:, 1])[::-1]
  print('faces of the components:', nf[:8].tolist(), 'of', len(nf))
  assert (nf >= 0.2 * nf[0]).sum() == 2 and want['counts'][1] == 2 and (nf[2:] > 0).sum() >= 2 and nf[0] <= 2 * nf[1]

  one = reconstruct_object(views, voxel_size=SPHERE_VOXEL, depth_filter=False, components='largest')
  _same_mesh(one, host)
  assert len(one.faces) == nf[0] and (one.vertices[:, 0] < 0).all()                     # the larger sphere alone

  both = reconstruct_object(views, voxel_size=SPHERE_VOXEL, depth_filter=False, components=dict(keep='all', min_fraction=0.2))
  assert both.vertices.astype(np.float32).tobytes() == want['pos'].tobytes() and both.faces.astype(np.int32).tobytes() == want['faces'].tobytes()
  assert both.vertex_normals.astype(np.float32).tobytes() == want['normals'].tobytes()
  assert both.visual.vertex_colors[:, :3].tobytes() == want['colors'].tobytes()
  label, number = C.labels(both.faces, len(both.vertices))
  sizes = np.bincount(number[both.faces[:, 0]])
  assert len(sizes) == 2 and sizes.max() <= 2 * sizes.min() and sorted(sizes.tolist()) == sorted(nf[:2].tolist())
  # each part is one of the two spheres; none of the floaters: the bead's centre is 44 mm from the nearer sphere's surface, and the
  # extraction had vertices on the bead (within its radius and a voxel) that are gone
  centres = np.array([[-1.5 * SPHERE_R, 0, 0], [1.5 * SPHERE_R, 0, 0]])
  for k in range(2):
    part = both.vertices[number == k]
    assert np.abs(part.mean(0) - centres[k]).max() < SPHERE_VOXEL, (k, part.mean(0))
  bead = lambda v: np.linalg.norm(np.asarray(v, dtype=np.float64) - np.array([0.0, 0.055, 0.02]), axis=1)
  assert (bead(m['vertices']) < 0.006 + SPHERE_VOXEL).sum() > 10 and bead(both.vertices).min() > 0.04
  with pytest.raises(TypeError):
    reconstruct_object(views, voxel_size=SPHERE_VOXEL, depth_filter=False, components=dict(fraction=0.2))
  with pytest.raises(ValueError):
    reconstruct_object(views, voxel_size=SPHERE_VOXEL, depth_filter=False, components='all')


def test_textured_mesh_keeps_its_texture():
  from foundationpose_amd import Utils as U
  from foundationpose_amd import synthetic as S
  mesh = S.make_mustard_mesh(seed=0, n_theta=48, n_z=42, textured=True)
  V, F = len(mesh.vertices), len(mesh.faces)
  tri = np.array([[0.2, 0.0, 0.0], [0.21, 0.0, 0.0], [0.2, 0.01, 0.0]])
  # the detached triangle goes IN FRONT: every index of the bottle moves
  dirty = S.SimpleMesh(np.concatenate([tri, mesh.vertices]), np.concatenate([[[0, 1, 2]], mesh.faces + 3]),
                       visual=S.TextureVisual(uv=np.concatenate([np.zeros((3, 2)), mesh.visual.uv]), image=mesh.visual.image))
  out, info, vmap = U.clean_mesh(dirty, return_map=True)
  assert (info['components'], info['kept_components'], info['vertices_in'], info['faces_in']) == (2, 1, V + 3, F + 1)
  assert (info['vertices'], info['faces'], info['component_faces']) == (V, F, [F])
  assert vmap.tolist() == [-1] * 3 + list(range(V))
  assert isinstance(out.visual, S.TextureVisual) and out.visual.image is mesh.visual.image
  assert out.visual.uv.tobytes() == np.asarray(dirty.visual.uv)[vmap >= 0].tobytes() == mesh.visual.uv.tobytes()
  assert out.vertices.tobytes() == mesh.vertices.astype(np.float32).astype(np.float64).tobytes() and out.faces.tobytes() == mesh.faces.tobytes()
  kept_all, info = U.clean_mesh(dirty, keep='all')
  assert info['component_faces'] == [1, F] and len(kept_all.vertices) == V + 3 and kept_all.visual.uv.shape == (V + 3, 2)
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  assert make_mesh_tensors(out)['pos'].shape == (V, 3)
