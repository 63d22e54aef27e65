"""GPU: texture baking (csrc/texture.hip, Utils.bake_texture, reconstruct_object(texture=...)) against the numpy restatement of the
header's rule (tests/texture_bake_oracle.py), bit for bit, and through the public layer: a baked mesh renders like the oracle rasteriser
says, shows more of the source's texture than the vertex-coloured mesh it was baked for, and registers.

Shapes: icospheres of 80, 79 (odd: the last cell has no B) and 320 faces; T = 64 gives cells of 9 texels for 80 faces and of 4, the
smallest, for 320; T = 128 gives 18.  T = 64 is one workgroup column of 16 workgroups, T = 128 is 2 x 32.  Five views of 64 x 48."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import texture_bake_oracle as O
from tests import tsdf_oracle as TO

pytestmark = pytest.mark.gpu
H, W = 48, 64
K = np.array([[120.0, 0, 31.5], [0, 120.0, 23.5], [0, 0, 1.0]])
RADIUS, DIST = 0.05, 0.3
COS_MIN = np.cos(np.deg2rad(75.0))


def _icosphere(subdivisions):
  t = (1 + np.sqrt(5)) / 2
  v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
  f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
       (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
  v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
  for _ in range(subdivisions):
    mid, nf = {}, []

    def m(a, b):
      key = (min(a, b), max(a, b))
      if key not in mid:
        p = v[a] + v[b]
        v.append(p / np.linalg.norm(p))
        mid[key] = len(v) - 1
      return mid[key]
    for a, b, c in f:
      ab, bc, ca = m(a, b), m(b, c), m(c, a)
      nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    f = nf
  return RADIUS * np.asarray(v), np.asarray(f, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _mesh(n_faces):
  v, f = _icosphere(2 if n_faces > 80 else 1)
  assert len(f) >= n_faces
  f = f[:n_faces]
  n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
  assert ((n * v[f].mean(1)).sum(1) > 0).all()          # outward
  colours = np.random.RandomState(7).randint(0, 256, size=(len(v), 3)).astype(np.uint8)
  return v.astype(np.float32), f, colours


def _render_views(H, W, K, least):
  """Five views of the vertex-coloured 80-face sphere rendered by the rasteriser; depths rounded to millimetres (what a 16-bit PNG holds);
  masks: the object, with the left half of view 1 and the lower two thirds of view 3 cut away.  More than `least` object pixels a view."""
  from foundationpose_amd import Utils as U
  from foundationpose_amd import synthetic as S
  v, f, colours = _mesh(80)
  rgba = np.concatenate([colours, np.full((len(colours), 1), 255, np.uint8)], 1)
  mt = U.make_mesh_tensors(S.SimpleMesh(v, f, vertex_colors=rgba))
  poses = np.stack([TO.look_at(e) for e in TO.fibonacci_eyes(5, DIST)])
  color, depth, _ = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=np.linalg.inv(poses).astype(np.float32), mesh_tensors=mt)
  mm = np.round(depth.cpu().numpy().astype(np.float64) * 1e3).astype(np.uint16)
  depths = (mm.astype(np.float64) / 1e3).astype(np.float32)
  rgbs = np.clip(np.round(color.cpu().numpy() * 255), 0, 255).astype(np.uint8)
  masks = (mm > 0).astype(np.uint8)
  masks[1, :, :W // 2] = 0
  masks[3, H // 3:, :] = 0
  assert all((d > 0).sum() > least for d in depths)
  return dict(rgbs=rgbs, depths=depths, masks=masks, K=K, cam_in_obs=poses)


@functools.lru_cache(maxsize=None)
def _views():
  return _render_views(H, W, K, 500)


@functools.lru_cache(maxsize=None)
def _oracle(n_faces, T, top_n, with_masks):
  v, f, colours = _mesh(n_faces)
  vw = _views()
  return O.bake(v, f, colours, vw['rgbs'], vw['depths'], vw['masks'] if with_masks else None, K, vw['cam_in_obs'], T, top_n=top_n)


def _device_bake(n_faces, T, top_n=4, with_masks=False, views=None, colours=True, **kw):
  from foundationpose_amd import Utils as U
  v, f, c = _mesh(n_faces)
  vw = _views() if views is None else views
  tex, uv, used = U.bake_texture_arrays(v, f, vw['rgbs'], vw['depths'], K, vw['cam_in_obs'], T, colors=c if colours else None,
                                        masks=vw['masks'] if with_masks else None, top_n=top_n, **kw)
  return tex.cpu().numpy(), uv.cpu().numpy(), used.cpu().numpy()


def _subset(vw, idx):
  return {k: (a[list(idx)] if k != 'K' else a) for k, a in vw.items()}


@pytest.mark.parametrize('with_masks', [False, True])
@pytest.mark.parametrize('top_n', [1, 2, 4])
@pytest.mark.parametrize('n_faces,T', [(80, 64), (80, 128), (79, 64), (79, 128), (320, 64)])
def test_bits_equal_the_restatement(n_faces, T, top_n, with_masks):
  want = _oracle(n_faces, T, top_n, with_masks)
  got = _device_bake(n_faces, T, top_n, with_masks)
  again = _device_bake(n_faces, T, top_n, with_masks)
  c = O.cell(T, n_faces)
  assert c == {(80, 64): 9, (80, 128): 18, (79, 64): 9, (79, 128): 18, (320, 64): 4}[(n_faces, T)]
  own = want[2] >= 0
  print(f'F {n_faces} T {T} c {c} top_n {top_n} masks {with_masks}: used histogram {np.bincount(want[2][own], minlength=5).tolist()}, '
        f'texels that differ {int((got[0] != want[0]).any(-1).sum())}, used that differ {int((got[2] != want[2]).sum())}')
  assert (want[2][own] >= 1).mean() > 0.5 and (want[2][own] == 0).any()         # both the blend and the fallback are exercised
  if top_n == 4:
    assert (want[2] >= 2).any()
  assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
  assert np.array_equal(got[2], want[2])
  assert np.array_equal(got[0], want[0])
  for a, b in zip(got, again):
    assert a.tobytes() == b.tobytes()


def test_bits_under_a_camera_with_fx_not_fy():
  """Views of 31 x 33 pixels through tsdf_oracle.skew_camera (fy = 1.25 fx, cx and cy off the middle by different amounts): a kernel that
  takes fx for fy or cx for cy in the projection samples other pixels than the restatement.  Views feed most texels."""
  from foundationpose_amd import Utils as U
  Ks = TO.skew_camera(31, 33, 60.0)
  vw = _render_views(31, 33, Ks, 100)
  v, f, colours = _mesh(80)
  want = O.bake(v, f, colours, vw['rgbs'], vw['depths'], vw['masks'], Ks, vw['cam_in_obs'], 64, top_n=4)
  own = want[2] >= 0
  print(f'used histogram {np.bincount(want[2][own], minlength=5).tolist()}')
  assert (want[2][own] >= 1).mean() > 0.5
  tex, uv, used = U.bake_texture_arrays(v, f, vw['rgbs'], vw['depths'], Ks, vw['cam_in_obs'], 64, colors=colours, masks=vw['masks'], top_n=4)
  assert np.array_equal(used.cpu().numpy(), want[2]) and np.array_equal(tex.cpu().numpy(), want[0])
  assert np.array_equal(uv.cpu().numpy().view(np.uint32), want[1].view(np.uint32))


def test_masks_matter():
  assert (_oracle(80, 64, 4, True)[2] != _oracle(80, 64, 4, False)[2]).sum() > 50


def test_equal_views_the_lower_index_wins():
  """the same view twice with different images, top_n = 1: every coloured texel has the first image's colour"""
  vw = _subset(_views(), [2, 2])
  vw['rgbs'] = np.stack([vw['rgbs'][0], 255 - vw['rgbs'][0]])
  first = _device_bake(80, 64, top_n=1, views=_subset(vw, [0]))
  both = _device_bake(80, 64, top_n=1, views=vw)
  assert (both[2] == 1).sum() > 300
  assert np.array_equal(both[0], first[0]) and np.array_equal(both[2], first[2])
  swapped = _device_bake(80, 64, top_n=1, views=_subset(vw, [1, 0]))
  assert (swapped[0] != first[0]).any(-1).sum() > 300


def test_a_plate_in_front_hides_the_view():
  """A plate at 0.15 m in front of the sphere (0.25 m) in view 0's depth map, over the middle of the image: the texels whose point view 0
  saw through those pixels lose exactly that view."""
  vw = _views()
  plate = {k: (a.copy() if k != 'K' else a) for k, a in vw.items()}
  plate['depths'][0, 14:34, 22:42] = 0.15
  T = 128
  solo_base, solo_plate = _device_bake(80, T, views=_subset(vw, [0])), _device_bake(80, T, views=_subset(plate, [0]))
  behind = (solo_base[2] == 1) & (solo_plate[2] == 0)
  assert behind.sum() > 200 and not ((solo_base[2] == 0) & (solo_plate[2] == 1)).any()
  passing = sum(_device_bake(80, T, views=_subset(vw, [k]))[2].astype(int) for k in range(5))
  assert passing.max() <= 4                              # top_n = 4 never saturates here: `used` counts every passing view
  base, got = _device_bake(80, T), _device_bake(80, T, views=plate)
  assert np.array_equal(base[2].astype(int) - got[2].astype(int), behind.astype(int))
  v, f, colours = _mesh(80)
  want = O.bake(v, f, colours, plate['rgbs'], plate['depths'], None, K, plate['cam_in_obs'], T)
  assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])


def test_faces_turned_away_keep_the_fallback():
  vw = _subset(_views(), [0])
  T = 128
  tex, _, used = _device_bake(80, T, views=vw)
  fallback, _, used0 = _device_bake(80, T, views=_subset(_views(), []))
  v, f, _ = _mesh(80)
  own, face, _, p = O.texel_points(v, f, T)
  n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).astype(np.float64)
  n /= np.linalg.norm(n, axis=1, keepdims=True)
  w = vw['cam_in_obs'][0][:3, 3] - p
  cosang = (n[face] * w).sum(1) / np.linalg.norm(w, axis=1)
  away = cosang < COS_MIN - 1e-3
  assert away.sum() > 1000 and (used[own][away] == 0).all() and np.array_equal(tex[own][away], fallback[own][away])
  assert (used[own][cosang > 0.5] == 1).mean() > 0.9 and set(np.unique(used)) == {-1, 0, 1}
  assert (used0[own] == 0).all() and (used0[~own] == -1).all() and (fallback[~own] == 0).all()


def test_no_views_bakes_the_vertex_colours():
  got = _device_bake(79, 64, views=_subset(_views(), []))
  v, f, colours = _mesh(79)
  want = O.bake(v, f, colours, None, None, None, K, np.zeros((0, 4, 4)), 64)
  assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
  grey = _device_bake(79, 64, views=_subset(_views(), []), colours=False)
  assert (grey[0][want[2] == 0] == 128).all() and (grey[0][want[2] < 0] == 0).all()


def test_refusals_are_made_on_the_host():
  """FP_EINVAL from the C entry and ValueError from Python, all before any launch: more than 64 views, a tex_size that is no power of
  two, cells under 4 texels, top_n outside 1 .. 4."""
  from foundationpose_amd import Utils as U
  from foundationpose_amd import _lib
  v, f, _ = _mesh(80)
  big_v, big_f = _icosphere(3)                               # 1280 faces: cells of 2 texels at T = 64, 4 at T = 128
  dev = torch.device('cuda', torch.cuda.current_device())
  ctx = _lib.Context.get(dev)

  def c_call(pos, faces, n_views, T, top_n=4):
    pos_d = torch.as_tensor(np.asarray(pos, dtype=np.float32), device=dev).contiguous()
    faces_d = torch.as_tensor(np.asarray(faces, dtype=np.int32), device=dev).contiguous()
    n_alloc = max(n_views, 1)
    rgb = torch.zeros((n_alloc, H, W, 3), dtype=torch.uint8, device=dev)
    depth = torch.zeros((n_alloc, H, W), dtype=torch.float, device=dev)
    poses = np.ascontiguousarray(np.tile(np.eye(4), (n_alloc, 1, 1)))
    tex = torch.zeros((max(T, 1), max(T, 1), 3), dtype=torch.uint8, device=dev)
    uv = torch.zeros((3 * len(faces), 2), dtype=torch.float, device=dev)
    cfg = _lib.FpTextureCfg(struct_size=ctypes.sizeof(_lib.FpTextureCfg), tex_size=T, top_n=top_n, depth_tol=0.005, cos_min=COS_MIN, zfar=float('inf'))
    Kd, Kp = _lib.k_ptr(K)
    rc = _lib.lib().fp_texture_bake(ctx.handle, _lib.ptr(pos_d), len(pos), _lib.ptr(faces_d), len(faces), None, _lib.ptr(rgb), _lib.ptr(depth), None,
                                    n_views, H, W, Kp, _lib.ptr(poses), ctypes.byref(cfg), _lib.ptr(tex), _lib.ptr(uv), None, _lib.stream_ptr(dev))
    return rc, (_lib.lib().fp_last_error() or b'').decode()

  assert c_call(v, f, 5, 64)[0] == 0
  rc, msg = c_call(v, f, 65, 64)
  assert rc == _lib.FP_EINVAL and '64' in msg
  for T in (96, 32, 0):
    assert c_call(v, f, 1, T)[0] == _lib.FP_EINVAL
  rc, msg = c_call(big_v, big_f, 1, 64)
  assert rc == _lib.FP_EINVAL and 'tex_size 128 fits' in msg
  assert c_call(big_v, big_f, 1, 128)[0] == 0
  assert c_call(v, f, 1, 64, top_n=0)[0] == _lib.FP_EINVAL and c_call(v, f, 1, 64, top_n=5)[0] == _lib.FP_EINVAL

  vw = _views()
  many = {k: (np.concatenate([a] * 13) if k != 'K' else a) for k, a in vw.items()}      # 65 views
  with pytest.raises(ValueError, match='at most 64'):
    U.bake_texture_arrays(v, f, many['rgbs'], many['depths'], K, many['cam_in_obs'], 64)
  with pytest.raises(ValueError, match='power of two'):
    U.bake_texture_arrays(v, f, vw['rgbs'], vw['depths'], K, vw['cam_in_obs'], 96)
  with pytest.raises(ValueError, match='tex_size 128 fits'):
    U.bake_texture_arrays(big_v, big_f, vw['rgbs'], vw['depths'], K, vw['cam_in_obs'], 64)
  with pytest.raises(ValueError, match='top_n'):
    U.bake_texture_arrays(v, f, vw['rgbs'], vw['depths'], K, vw['cam_in_obs'], 64, top_n=5)
  torch.cuda.synchronize()


def _baked_sphere():
  from foundationpose_amd import Utils as U
  from foundationpose_amd import synthetic as S
  v, f, colours = _mesh(80)
  rgba = np.concatenate([colours, np.full((len(colours), 1), 255, np.uint8)], 1)
  return U.bake_texture(S.SimpleMesh(v, f, vertex_colors=rgba), _views(), tex_size=128, return_info=True)


def test_bake_texture_returns_a_mesh_with_an_atlas():
  from foundationpose_amd import Utils as U
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  mesh, info = _baked_sphere()
  v, f, _ = _mesh(80)
  want = _oracle(80, 128, 4, True)
  assert info['tex_size'] == 128 and info['cell'] == 18 and 0.5 < info['coverage'] <= 1
  own = want[2] >= 0
  assert info['coverage'] == (want[2] >= 1).sum() / own.sum()
  assert np.array_equal(mesh.vertices, v.astype(np.float64)) and np.array_equal(mesh.faces, f)
  assert np.array_equal(mesh.visual.image, want[0]) and mesh.visual.uv.dtype == np.float32
  assert np.array_equal(mesh.visual.uv_idx, np.arange(240).reshape(80, 3))
  mt = make_mesh_tensors(mesh)
  assert np.array_equal(mt['uv'].cpu().numpy().view(np.uint32), want[1].view(np.uint32))
  assert tuple(mt['pos'].shape) == (42, 3) and tuple(mt['uv'].shape) == (240, 2) and tuple(mt['uv_idx'].shape) == (80, 3)
  auto, auto_info = U.bake_texture(mesh_without_visual(mesh), _views(), return_info=True)
  assert auto_info['tex_size'] == 64 and auto_info['cell'] == 9       # the smallest T with cells of at least 8 texels
  with pytest.raises(ValueError, match='uv_idx'):
    U.clean_mesh(mesh)
  with pytest.raises(ValueError, match='textured'):
    U.simplify_mesh(mesh, cell=0.01)


def mesh_without_visual(mesh):
  from foundationpose_amd import synthetic as S
  return S.SimpleMesh(mesh.vertices, mesh.faces)


def test_baked_mesh_renders_like_the_oracle_rasteriser():
  """The baked mesh through nvdiffrast_render at a new view against the oracle's rasteriser (oracle/render.py) given the same uv, uv_idx
  and texture: the same pixels and winning faces, and colours within the allowance of the textured render test of
  tests/test_gpu_kernels.py (2e-6 absolute on values <= 1, on all but 2e-4 of the values)."""
  from foundationpose_amd import Utils as U
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  from oracle.render import nvdiffrast_render as orender
  from tests import util
  mesh, _ = _baked_sphere()
  mt = make_mesh_tensors(mesh, device='cpu')
  Hh, Wh = 120, 160
  Kh = np.array([[400.0, 0, 79.5], [0, 400.0, 59.5], [0, 0, 1.0]])
  pose = np.linalg.inv(TO.look_at([0.21, -0.17, 0.12]))[None].astype(np.float32)
  eo, eg = {}, {'rast': None}
  co, do, _ = orender(K=Kh, H=Hh, W=Wh, ob_in_cams=pose, mesh_tensors=mt, extra=eo)
  cg, dg, _ = U.nvdiffrast_render(K=Kh, H=Hh, W=Wh, ob_in_cams=torch.from_numpy(pose).cuda(), mesh_tensors=util.to_dev(mt), extra=eg)
  id_o, id_g = eo['rast'][..., 3].numpy().astype(np.int64), eg['rast'].cpu()[..., 3].numpy().astype(np.int64)
  assert (id_o > 0).sum() > 3000 and np.array_equal(id_o, id_g)
  frac, mx, _ = util.mismatch_report(co.numpy(), cg.cpu().numpy(), 2e-6)
  print(f'colour: {frac:.2e} of the values differ by more than 2e-6, max {mx:.2e}')
  assert frac <= 2e-4
  # and it shows the views' colours: not grey, not black inside the silhouette
  inside = id_g[0] > 0
  assert (cg.cpu().numpy()[0][inside].max(-1) > 0).mean() > 0.999


# ---- the public layer: reconstruct_object(texture=...) on the textured bottle ------------------------------------------------------------
MAXV = 1500


@pytest.fixture(scope='module')
def bottle():
  """12 views of 160 x 120 of the textured bottle, and what reconstruct_object makes of them with and without the atlas"""
  from foundationpose_amd import Utils as U
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  from foundationpose_amd.reconstruct import reconstruct_object
  src = S.make_mustard_mesh(seed=0, textured=True)
  src.vertices = src.vertices - (src.vertices.min(0) + src.vertices.max(0)) / 2
  src_mt = make_mesh_tensors(src)
  (MH, MW), MK = TO.MUSTARD_HW, TO.MUSTARD_K
  cams = np.stack([TO.look_at(e) for e in TO.mustard_eyes()])
  color, depth, _ = U.nvdiffrast_render(K=MK, H=MH, W=MW, ob_in_cams=np.linalg.inv(cams).astype(np.float32), mesh_tensors=src_mt)
  mm = np.round(depth.cpu().numpy().astype(np.float64) * 1e3).astype(np.uint16)
  views = dict(depths=(mm.astype(np.float64) / 1e3).astype(np.float32), rgbs=np.clip(np.round(color.cpu().numpy() * 255), 0, 255).astype(np.uint8),
               masks=(mm > 0).astype(np.uint8), K=MK, cam_in_obs=cams)
  plain = reconstruct_object(views, voxel_size=TO.MUSTARD_VOXEL, max_vertices=MAXV)
  baked = reconstruct_object(views, voxel_size=TO.MUSTARD_VOXEL, max_vertices=MAXV, texture=512)
  return dict(src_mt=src_mt, views=views, plain=plain, baked=baked)


def test_the_atlas_shows_more_of_the_source_than_vertex_colours(bottle):
  """The point of it all.  The source, the vertex-coloured reconstruction and the baked one rendered at a held-out eye; on the pixels all
  three cover, the mean absolute colour error of the baked mesh against the source is LOWER than that of the vertex-coloured one.  No
  absolute threshold: the yardstick is the vertex-coloured mesh on the same pixels."""
  from foundationpose_amd import Utils as U
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  plain, baked = bottle['plain'], bottle['baked']
  assert np.array_equal(plain.vertices, baked.vertices) and np.array_equal(plain.faces, baked.faces)
  assert len(plain.vertices) <= MAXV and hasattr(baked.visual, 'uv_idx') and baked.visual.image.shape == (512, 512, 3)
  (MH, MW), MK = TO.MUSTARD_HW, TO.MUSTARD_K
  el, az = 0.5, 0.1
  eye = 0.42 * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
  pose = np.linalg.inv(TO.look_at(eye))[None].astype(np.float32)
  out = []
  for mt in (bottle['src_mt'], make_mesh_tensors(plain), make_mesh_tensors(baked)):
    c, d, _ = U.nvdiffrast_render(K=MK, H=MH, W=MW, ob_in_cams=pose, mesh_tensors=mt)
    out.append((c[0].cpu().numpy().astype(np.float64) * 255, d[0].cpu().numpy() > 0))
  common = out[0][1] & out[1][1] & out[2][1]
  assert common.sum() > 0.9 * out[0][1].sum() > 1000
  err_plain = np.abs(out[1][0] - out[0][0])[common].mean()
  err_baked = np.abs(out[2][0] - out[0][0])[common].mean()
  print(f'held-out view, {int(common.sum())} common pixels: mean |colour error| of 255 - vertex colours {err_plain:.2f}, atlas {err_baked:.2f}')
  assert err_baked < err_plain


def test_baked_reconstruction_registers(bottle):
  """The baked mesh goes where a CAD model goes: make_mesh_tensors, FoundationPose, one register() with 8 rotations and 1 iteration, as in
  tests/test_gpu_tsdf.py::test_fused_mesh_registers.  Seeded random weights: a finite pose, no accuracy claim."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.config import REFINE_DEFAULT, SCORE_DEFAULT
  from foundationpose_amd.estimater import FoundationPose
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
  from foundationpose_amd.predict_score import ScorePredictor
  from tests import util
  sc = util.scene(0)
  baked = bottle['baked']
  mt = make_mesh_tensors(baked)
  assert len(mt['pos']) <= MAXV and 'tex' in mt and tuple(mt['uv'].shape) == (3 * len(baked.faces), 2)
  refiner = PoseRefinePredictor(state_dict=S.make_refine_state_dict(0), cfg=REFINE_DEFAULT)
  scorer = ScorePredictor(state_dict=S.make_score_state_dict(1), cfg=SCORE_DEFAULT)
  np.random.seed(0)
  est = FoundationPose(model_pts=baked.vertices, model_normals=baked.vertex_normals, mesh=baked, refiner=refiner, scorer=scorer)
  est.rot_grid = est.rot_grid[:8].contiguous()
  pose = np.asarray(est.register(K=sc['K'], rgb=sc['rgb'], depth=sc['depth'], ob_mask=sc['mask'], iteration=1))
  assert pose.shape == (4, 4) and np.isfinite(pose).all()


def test_reconstruct_texture_options_and_obj_round_trip(bottle, tmp_path):
  """texture=True picks the smallest atlas with cells of 8 texels, a dict sets bake_texture's arguments, unknown keys and views without
  rgbs are refused; the baked mesh written as OBJ + MTL + PNG and read back with split_uv=False gives the same mesh tensors."""
  from foundationpose_amd import Utils as U
  from foundationpose_amd import mesh_io
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  from foundationpose_amd.reconstruct import reconstruct_object
  views, baked = bottle['views'], bottle['baked']
  nf = len(baked.faces)
  auto = reconstruct_object(views, voxel_size=TO.MUSTARD_VOXEL, max_vertices=MAXV, texture=True)
  T = U.texture_size_for(nf, 8)
  assert auto.visual.image.shape == (T, T, 3) and U.texture_cell(T, nf) >= 8 > U.texture_cell(T // 2, nf)
  assert U.texture_cell(T, nf) == O.cell(T, nf)
  one = reconstruct_object(views, voxel_size=TO.MUSTARD_VOXEL, max_vertices=MAXV, texture=dict(tex_size=256, top_n=1, depth_tol=0.01))
  assert one.visual.image.shape == (256, 256, 3) and np.array_equal(one.faces, baked.faces)
  with pytest.raises(TypeError, match='unknown keys'):
    reconstruct_object(views, voxel_size=TO.MUSTARD_VOXEL, max_vertices=MAXV, texture=dict(size=256))
  with pytest.raises(ValueError, match='rgbs'):
    reconstruct_object({k: v for k, v in views.items() if k != 'rgbs'}, voxel_size=TO.MUSTARD_VOXEL, max_vertices=MAXV, texture=True)
  path = str(tmp_path / 'model.obj')
  mesh_io.save_obj(baked, path)
  back = mesh_io.load_obj(path, split_uv=False)
  a, b = make_mesh_tensors(baked, device='cpu'), make_mesh_tensors(back, device='cpu')
  assert sorted(a) == sorted(b) == ['faces', 'pos', 'tex', 'uv', 'uv_idx', 'vnormals']
  for k in ('faces', 'uv_idx', 'tex', 'uv', 'pos'):
    assert torch.equal(a[k], b[k]), k
  with pytest.raises(ValueError, match='uv_idx'):
    mesh_io.save_ply(baked, str(tmp_path / 'model.ply'))
