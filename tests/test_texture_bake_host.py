"""CPU: the texture atlas of fp_texture_bake and its numpy restatement (tests/texture_bake_oracle.py) on cases that can be worked out by
hand, and the Python plumbing that carries a per-face atlas: TextureVisual.uv_idx, make_mesh_tensors, save_obj / load_obj.  (The device
kernel against the restatement, bit for bit: tests/test_gpu_texture_bake.py.)"""
import numpy as np
import pytest

from tests import texture_bake_oracle as O
from tests.tsdf_oracle import look_at

F32 = np.float32


# ---- the layout ---------------------------------------------------------------------------------------------------------------------
def _patch_samples(T, n_faces, f, step=0.25):
  """uv (float32, exact) on a quarter-texel lattice over the uv triangle of face f: corners, edge points and interior"""
  g, c = O.grid(n_faces), O.cell(T, n_faces)
  m = c - 3
  k = f // 2
  col, row = k % g, k // g
  a = np.arange(0, m + step / 2, step)
  x, y = [t.reshape(-1) for t in np.meshgrid(a, a)]
  keep = x + y <= m
  x, y = x[keep], y[keep]
  if f % 2:
    x, y = c - 1 - x, c - 1 - y
  u = ((col * c + x).astype(F32) + F32(0.5)) / F32(T)
  v = ((row * c + y).astype(F32) + F32(0.5)) / F32(T)
  assert np.array_equal(u.astype(np.float64), (col * c + x + 0.5) / T) and np.array_equal(v.astype(np.float64), (row * c + y + 0.5) / T)
  return u, v


@pytest.mark.parametrize('n_faces', [1, 2, 3, 7, 8, 9, 512])
def test_bilinear_fetch_stays_inside_the_face(n_faces):
  """T = 64.  512 faces is the largest count that still gives c = 4 there (256 cells on a 16 x 16 grid).  For every sampled uv of a
  face, every texel the rasteriser's bilinear fetch gives a non-zero weight is owned by that face; no texel has two owners; the
  anti-diagonal, a last odd cell's B half and the outside belong to nobody; 1 - (1 - v) is v bit for bit."""
  T = 64
  g, c = O.grid(n_faces), O.cell(T, n_faces)
  assert g * g >= (n_faces + 1) // 2 > (g - 1) * (g - 1) or n_faces <= 2
  if n_faces == 512:
    assert c == 4 and O.cell(T, 513) < 4
  face, _, _ = O.owners(T, n_faces)
  # owners(): one owner per texel by construction of the array; every face owns the same number of texels: c (c - 1) / 2
  counts = np.bincount(face[face >= 0], minlength=n_faces)
  assert (counts == c * (c - 1) // 2).all()
  assert (face >= 0).sum() == n_faces * c * (c - 1) // 2
  uv = O.atlas_uv(T, n_faces)
  assert uv.shape == (3 * n_faces, 2) and uv.dtype == F32
  one = F32(1)
  assert np.array_equal((one - (one - uv[:, 1])).view(np.uint32), uv[:, 1].view(np.uint32))
  for f in range(n_faces):
    u, v = _patch_samples(T, n_faces, f)
    # the lattice contains the three uv entries of the face
    have = set(zip(u.tolist(), v.tolist()))
    assert all((float(a), float(b)) in have for a, b in uv[3 * f:3 * f + 3])
    assert np.array_equal((one - (one - v)).view(np.uint32), v.view(np.uint32))
    total = np.zeros(len(u), dtype=np.float64)
    for x, y, w in O.bilinear_taps(u, v, T):
      hit = w != 0
      assert (face[y[hit], x[hit]] == f).all(), f'face {f} of {n_faces}: a foreign texel gets weight'
      total += w
    assert np.allclose(total, 1, atol=1e-6)


def test_unowned_texels():
  T, n_faces = 64, 7          # 4 cells on a 2 x 2 grid, c = 32; the last cell has no B
  face, i, j = O.owners(T, n_faces)
  c = O.cell(T, n_faces)
  assert c == 32
  Y, X = np.meshgrid(np.arange(T), np.arange(T), indexing='ij')
  assert (face[(X % c) + (Y % c) == c - 1] == -1).all()
  last = (X >= c) & (Y >= c)
  assert set(np.unique(face[last])) == {-1, 6}
  face9, _, _ = O.owners(T, 9)      # 5 cells on a 3 x 3 grid, c = 21: column 63 and row 63 lie outside the cells
  assert O.cell(T, 9) == 21 and (face9[:, 63] == -1).all() and (face9[63, :] == -1).all()
  assert set(np.unique(face9[42:, :])) == {-1}      # cells 6 .. 8 are empty


# ---- the restatement on an octahedron ---------------------------------------------------------------------------------------------------
R_OCT = 0.05
H, W = 48, 64
K = np.array([[120.0, 0, 31.5], [0, 120.0, 23.5], [0, 0, 1.0]])
VIEW_COLOURS = np.array([[200, 40, 40], [40, 200, 40], [40, 40, 200]], dtype=np.uint8)
COS_MIN = np.cos(np.deg2rad(75.0))


def _octahedron():
  v = R_OCT * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
  faces = []
  for sx in (0, 1):
    for sy in (2, 3):
      for sz in (4, 5):
        tri = [sx, sy, sz]
        n = np.cross(v[tri[1]] - v[tri[0]], v[tri[2]] - v[tri[0]])
        if n @ v[tri].mean(0) < 0:
          tri = [sx, sz, sy]
        faces.append(tri)
  colours = np.array([[250, 10, 10], [10, 250, 10], [10, 10, 250], [250, 250, 10], [10, 250, 250], [250, 10, 250]], dtype=np.uint8)
  return v, np.asarray(faces), colours


def _octahedron_depth(cam_in_ob):
  """z-depth (H,W) float32 of |x| + |y| + |z| <= R_OCT: the ray through every pixel centre against the 8 half-spaces, float64"""
  us, vs = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
  d = np.stack([(us - K[0, 2]) / K[0, 0], (vs - K[1, 2]) / K[1, 1], np.ones_like(us)], -1) @ cam_in_ob[:3, :3].T
  o = cam_in_ob[:3, 3]
  enter, leave = np.full((H, W), -np.inf), np.full((H, W), np.inf)
  for s in np.array(np.meshgrid([-1, 1], [-1, 1], [-1, 1])).reshape(3, -1).T:
    den, num = d @ s, R_OCT - o @ s
    with np.errstate(divide='ignore', invalid='ignore'):
      t = num / den
    enter = np.where(den < 0, np.maximum(enter, t), enter)
    leave = np.where(den > 0, np.minimum(leave, t), leave)
  return np.where((enter < leave) & (enter > 0), enter, 0).astype(F32)


@pytest.fixture(scope='module')
def octa_case():
  v, faces, colours = _octahedron()
  eyes = 0.3 * np.array([[1, 0, 0], [0, 1, 0], [0, 0, -1]], dtype=np.float64)
  poses = np.stack([look_at(e) for e in eyes])
  depths = np.stack([_octahedron_depth(p) for p in poses])
  rgbs = np.stack([np.broadcast_to(c, (H, W, 3)) for c in VIEW_COLOURS]).copy()
  assert all((d > 0).sum() > 300 for d in depths)
  T = 64
  tex, uv, used = O.bake(v, faces, colours, rgbs, depths, None, K, poses, T, top_n=4, depth_tol=0.005, cos_min=COS_MIN)
  return dict(v=v, faces=faces, colours=colours, eyes=eyes, poses=poses, depths=depths, rgbs=rgbs, T=T, tex=tex, uv=uv, used=used)


def _texel_points(case):
  return O.texel_points(case['v'], case['faces'], case['T'])


def test_octahedron_texels_are_the_expected_blend(octa_case):
  """Views from +x, +y and -z at 0.3 m; constant images.  Each sees the four faces on its side at about 55 degrees, so faces are seen
  by 0 .. 3 views.  A convex solid hides nothing of a face turned towards the camera: a texel's views are those with cosang >= cos 75
  deg, and its colour is their cosang-weighted mean - worked out here in float64.  Left out: texels within 0.01 of the threshold in some
  view, and those whose bilinear footprint there touches a pixel off the surface by more than 4.5 mm (the silhouette: the nearest pixel
  may lie off the solid; on the face itself a pixel's step in depth is 3.5 mm, inside the 5 mm tolerance).  The rest is the majority."""
  own, f, b, p = _texel_points(octa_case)
  v, faces = octa_case['v'], octa_case['faces']
  n = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
  n /= np.linalg.norm(n, axis=1, keepdims=True)
  assert np.allclose(np.abs(n), 1 / np.sqrt(3))          # outward
  clear = np.ones(len(f), dtype=bool)
  wsum, csum, count = np.zeros(len(f)), np.zeros((len(f), 3)), np.zeros(len(f), dtype=int)
  for k, (eye, pose) in enumerate(zip(octa_case['eyes'], octa_case['poses'])):
    w = eye - p
    cosang = (n[f] * w).sum(1) / np.linalg.norm(w, axis=1)
    sees = cosang >= COS_MIN
    clear &= np.abs(cosang - COS_MIN) > 0.01
    q = (p - pose[:3, 3]) @ pose[:3, :3]
    x, y = K[0, 0] * q[:, 0] / q[:, 2] + K[0, 2], K[1, 1] * q[:, 1] / q[:, 2] + K[1, 2]
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    d = octa_case['depths'][k]
    solid = np.ones(len(f), dtype=bool)
    for dy in (0, 1):
      for dx in (0, 1):
        solid &= np.abs(d[y0 + dy, x0 + dx] - q[:, 2]) < 0.0045
    clear &= ~sees | solid
    wsum += np.where(sees, cosang, 0)
    csum += np.where(sees, cosang, 0)[:, None] * VIEW_COLOURS[k].astype(np.float64)
    count += sees
  print(f'clear texels: {clear.mean():.3f}')
  assert clear.mean() > 0.5, clear.mean()
  used, tex = octa_case['used'][own], octa_case['tex'][own].astype(int)
  assert np.array_equal(used[clear], count[clear])
  assert set(np.unique(count[clear])) == {0, 1, 2, 3}
  seen = clear & (count > 0)
  want = csum[seen] / wsum[seen][:, None]
  assert np.abs(tex[seen] - want).max() <= 0.5 + 1e-3
  # two views blended: neither pure colour
  two = clear & (count == 2)
  assert two.any() and (tex[two].max(1) < 200).all()


def test_octahedron_unseen_face_keeps_its_vertex_colours(octa_case):
  own, f, b, _ = _texel_points(octa_case)
  faces, colours = octa_case['faces'], octa_case['colours']
  centroid = octa_case['v'][faces].mean(1)
  hidden = int(np.flatnonzero((np.sign(centroid) == [-1, -1, 1]).all(1))[0])       # every eye lies behind its plane
  sel = f == hidden
  assert sel.sum() == 32 * 31 // 2 and (octa_case['used'][own][sel] == 0).all()
  want = (b[sel][:, :, None] * colours[faces[hidden]].astype(np.float64)).sum(1)
  got = octa_case['tex'][own][sel].astype(int)
  assert np.abs(got - want).max() <= 0.5 + 1e-3
  assert len(np.unique(got, axis=0)) > 100                   # an interpolation, not one colour
  # without vertex colours: grey
  tex, _, used = O.bake(octa_case['v'], faces, None, octa_case['rgbs'], octa_case['depths'], None, K, octa_case['poses'], octa_case['T'])
  assert np.array_equal(used, octa_case['used']) and (tex[own][sel] == 128).all()
  assert (tex[~own] == 0).all() and (used[~own] == -1).all()


def test_top_n_keeps_the_most_frontal_views_and_the_lower_index_among_equals(octa_case):
  own, f, _, _ = _texel_points(octa_case)
  c = octa_case
  one, _, used1 = O.bake(c['v'], c['faces'], c['colours'], c['rgbs'], c['depths'], None, K, c['poses'], c['T'], top_n=1)
  assert np.array_equal(np.minimum(c['used'], 1), used1)
  pure = one[own][c['used'][own] >= 1]
  assert all(any((row == col).all() for col in VIEW_COLOURS) for row in np.unique(pure, axis=0))
  # the same view twice, other colours: the first one wins everywhere
  rgbs = np.stack([c['rgbs'][0], c['rgbs'][1]])
  tie, _, used = O.bake(c['v'], c['faces'], None, rgbs, c['depths'][[0, 0]], None, K, c['poses'][[0, 0]], c['T'], top_n=1)
  assert (tie[used == 1] == VIEW_COLOURS[0]).all() and (used == 1).sum() > 500


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def _atlas_mesh():
  from foundationpose_amd import synthetic as S
  v, faces, _ = _octahedron()
  uv = O.atlas_uv(64, len(faces))
  uv[:, 1] = F32(1) - uv[:, 1]
  image = np.random.RandomState(3).randint(0, 256, size=(64, 64, 3)).astype(np.uint8)
  uv_idx = np.arange(3 * len(faces)).reshape(-1, 3)
  return S.SimpleMesh(v, faces, visual=S.TextureVisual(uv, image, uv_idx=uv_idx))


def test_make_mesh_tensors_takes_uv_idx_from_the_visual():
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  mesh = _atlas_mesh()
  mt = make_mesh_tensors(mesh, device='cpu')
  nf = len(mesh.faces)
  assert tuple(mt['pos'].shape) == (6, 3) and tuple(mt['faces'].shape) == (nf, 3)
  assert tuple(mt['uv'].shape) == (3 * nf, 2) and tuple(mt['uv_idx'].shape) == (nf, 3) and tuple(mt['tex'].shape) == (1, 64, 64, 3)
  assert np.array_equal(mt['uv_idx'].numpy(), np.arange(3 * nf).reshape(-1, 3))
  assert np.array_equal(mt['uv'].numpy().view(np.uint32), O.atlas_uv(64, nf).view(np.uint32))      # the flip round-trips bit for bit
  # a visual without uv_idx (or with None): the faces, as before
  plain = S.SimpleMesh(mesh.vertices, mesh.faces, visual=S.TextureVisual(np.zeros((6, 2)), mesh.visual.image))
  assert plain.visual.uv_idx is None
  assert np.array_equal(make_mesh_tensors(plain, device='cpu')['uv_idx'].numpy(), mesh.faces)


def test_obj_round_trip_of_an_atlas(tmp_path):
  from foundationpose_amd.mesh_io import load_mesh, load_obj, save_obj
  mesh = _atlas_mesh()
  path = str(tmp_path / 'baked.obj')
  save_obj(mesh, path)
  assert sorted(p.name for p in tmp_path.iterdir()) == ['baked.mtl', 'baked.obj', 'baked.png']
  back = load_obj(path, split_uv=False)
  assert np.array_equal(back.faces, mesh.faces) and np.array_equal(back.visual.uv_idx, mesh.visual.uv_idx)
  assert np.allclose(back.vertices, mesh.vertices, rtol=0, atol=1e-9)
  assert np.abs(back.visual.uv - mesh.visual.uv.astype(np.float64)).max() <= 1e-9       # %.9g: a float32 survives
  assert np.array_equal(back.visual.uv.astype(F32), mesh.visual.uv)
  assert np.array_equal(back.visual.image, mesh.visual.image)
  assert len(load_mesh(path, split_uv=False).vertices) == 6
  split = load_obj(path)
  assert len(split.vertices) == 3 * len(mesh.faces) and split.visual.uv.shape == (3 * len(mesh.faces), 2)
  assert getattr(split.visual, 'uv_idx', None) is None
  assert np.allclose(split.vertices[split.faces], mesh.vertices[mesh.faces], rtol=0, atol=1e-9)


def test_untextured_obj_is_written_as_before(tmp_path):
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.mesh_io import save_obj
  v = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.25, 0], [0, 0, 1 / 3]])
  f = np.array([[0, 2, 1], [0, 1, 3]])
  col = np.array([[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255], [51, 102, 204, 255]], dtype=np.uint8)
  path = tmp_path / 'plain.obj'
  save_obj(S.SimpleMesh(v, f, vertex_colors=col), str(path))
  assert path.read_text() == ('v 0 0 0 1.000000 0.000000 0.000000\n'
                              'v 0.1 0 0 0.000000 1.000000 0.000000\n'
                              'v 0 0.25 0 0.000000 0.000000 1.000000\n'
                              'v 0 0 0.333333333 0.200000 0.400000 0.800000\n'
                              'f 1 3 2\n'
                              'f 1 2 4\n')
  assert [p.name for p in tmp_path.iterdir()] == ['plain.obj']
