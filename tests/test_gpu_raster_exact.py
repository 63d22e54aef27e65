"""The HIP rasteriser (csrc/raster.hip) against the exact lattice reference of tests/tools/raster_ref.py: the winning triangle of every pixel
exactly (no exclusions but zclip_slant's stated band), u, v, z/w within TOL_UVZ, depth, xyz and colour within TOL_ATTR times the value range; the
launch forms (one launch for 1 or 2 hypotheses, fused classification at 5, vertex pre-pass + G face ranges, A records in global memory) bit-identical
to each other; the fused network tensor within one fp16 ulp of float64; and the two float64 tests of tests/test_oracle_independent.py (slanted
quad, ground plane through the camera) run on the kernel itself.  Every lattice case passed on the first run.

MEASURED on an MI355X, largest |err| / tol over the five hypotheses (TOL_UVZ = 5.0e-7, TOL_ATTR = 6.2e-7 x value range):
  case                                u,v,z/w  attributes
  centres_medium                     0.119  0.129
  centres_small                      0.000  0.000
  degenerate                         0.128  0.194
  depth_signs_mixed                  0.000  0.000
  depth_signs_tiny                   0.000  0.000
  depth_signs_ulp_neg                0.000  0.000
  depth_signs_ulp_pos                0.000  0.000
  far64_1600008                      0.119  0.250
  far64_16383                        0.060  0.136
  far64_16384                        0.015  0.061
  large32                            0.119  0.206
  ties_zero                          0.110  0.194
  ties_zero_rev                      0.181  0.194
  tiling_ear                         0.208  0.189
  tiling_ear_perm                    0.207  0.217
  tiling_fan                         0.208  0.212
  tiling_fan_perm                    0.226  0.208
  tiling_strip                       0.211  0.206
  tiling_strip_perm                  0.200  0.212
  window_half_out                    0.119  0.155
  window_wide                        0.180  0.194
  window_zoom                        0.119  0.148
  zclip_hi                           0.000  0.000
  zclip_lo                           0.000  0.000
  zclip_slant                        0.246  0.189
  padded_centres_small_F2048         0.000  0.000
  padded_centres_small_F4096         0.000  0.000
  padded_centres_small_F4099_V8200   0.000  0.000
  padded_centres_small_F8192         0.000  0.000
  padded_large32_F2048               0.119  0.206
  padded_large32_F2051_V8200         0.119  0.206
  padded_large32_F4096               0.119  0.206
  padded_large32_F8192               0.119  0.206
  padded_solo_max                    0.000  0.000
  padded_solo_over                   0.000  0.000
  network tensor, largest |err| / fp16 ulp: centres_small 0.400, depth_signs_mixed 0.500, large32 0.498, window_zoom 0.500

TEXTURE FETCH AND LIGHTING (R.SHADE_CASES against shade_float64; tolerance = TOL_TEX 6.9e-7 x the case's scale, normal map TOL_ATTR 6.2e-7), MEASURED
on an MI355X, largest |err| / tol over 1, 2 and 5 hypotheses; every case passed on the first run:
  case               light          colour (tol)       normal
  tex_identity       -              0.000 (1.63e-05)   0.000      bit for bit
  tex_identity_5x7   -              0.110 (1.00e-05)   0.000
  tex_corners        -              0.000 (1.63e-05)   0.000      bit for bit
  tex_wrap           -              0.168 (9.22e-06)   0.000
  tex_thin_1x1       -              0.000 (6.92e-07)   0.000
  tex_thin_1x6       -              0.201 (5.04e-06)   0.000
  tex_thin_6x1       -              0.207 (4.60e-06)   0.000
  tex_charts         -              0.083 (8.02e-06)   0.000
  tex_atlas          -              0.016 (1.11e-05)   0.000      (and within 1e-5 of a colour step of the face's own colour)
  tex_perspective    -              0.250 (5.54e-06)   0.000
  lit_vcol           bright         0.094 (1.87e-06)   0.205
  lit_vcol           default        0.121 (1.25e-06)   0.205
  lit_vcol           default_color  0.107 (1.25e-06)   0.205
  lit_vcol           dir            0.112 (1.25e-06)   0.205
  lit_vcol           dir_color      0.103 (1.25e-06)   0.205
  lit_vcol           pos            0.133 (1.25e-06)   0.205
  lit_vcol           pos_color      0.108 (1.25e-06)   0.205
  lit_tex            bright         0.099 (1.08e-05)   0.205
  lit_tex            default        0.110 (7.66e-06)   0.205
  lit_tex            default_color  0.087 (7.66e-06)   0.205
  lit_tex            dir            0.086 (7.66e-06)   0.205
  lit_tex            dir_color      0.086 (7.66e-06)   0.205
  lit_tex            pos            0.134 (7.66e-06)   0.205
  lit_tex            pos_color      0.092 (7.66e-06)   0.205
  network tensor rgb, largest |err| / fp16 ulp: tex_identity 0.400, tex_wrap 0.500, tex_perspective 0.500
The one change to csrc/ that these tests brought: the fetch reduces a texel index beyond the int range in float before converting it
(test_texture_fetch_far_from_the_origin; no image of any other test moves).

KERNELS of one `rocprofv3 --kernel-trace --stats` run of tests/tools/raster_lattice_digest.py (1, 2 and 5 hypotheses each; workgroups = hypotheses x 8
strips of 8 rows at 64 x 64; every API render is a render_kernel<0, .> and a render_kernel<2, .> launch over the same lists; fp_render_net is
render_kernel<1, .>):
  centres_small, large32 (V <= 8192, F < 2048)   1, 2: render_kernel<0 | 2, true> 8 / 16 workgroups (one launch)
                                                 5: classify_faces_kernel<true> (5, 1), render_kernel<0 | 2, false> 40 workgroups
  padded_large32_F8192 (G = 8)                   1, 2: one launch as above; 5: xform_vertices_kernel (1, 5) x 256 threads, classify_faces_kernel<false> (5, 8),
                                                 render_kernel<0 | 2, false> 40
  padded_centres_small_F4099_V8200 (G = 4, lds_verts == 0)   1, 2, 5: xform_vertices_kernel (33, N), classify_faces_kernel<false> (N, 4), render_kernel<., false> 8 N
  padded_solo_over (F one above the one-launch limit)        1, 2, 5: xform_vertices_kernel (4, N), classify_faces_kernel<false> (N, 8), render_kernel<., false> 8 N
FP_RENDER_SOLO=0 sends 1 and 2 hypotheses through the classification launches, FP_RENDER_PREPASS2=1 replaces classify_faces_kernel<true> by the
pre-pass + classify_faces_kernel<false> (test_other_launch_forms_give_identical_images).
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.tools import raster_ref as R
from tests.test_raster_ref_host import FAR_UV, compare_shaded, compare_with_reference, far_uv_case, render_case, render_shaded, shade_light

pytestmark = pytest.mark.gpu

@pytest.fixture(scope='module')
def U():
  from foundationpose_amd import Utils
  return Utils


_CACHE = {}


def _gpu(U, name, n):
  if (name, n) not in _CACHE:
    _CACHE[(name, n)] = render_case(U.nvdiffrast_render, R.lattice_case(name), n, dev='cuda')
  return _CACHE[(name, n)]


@pytest.mark.parametrize('name', R.ALL_CASES)
def test_lattice_case_against_the_exact_reference(U, name):
  c = R.lattice_case(name)
  compare_with_reference(c, _gpu(U, name, 5), 5, 'hip')


@pytest.mark.parametrize('name', R.ALL_CASES)
def test_one_two_and_five_hypotheses_give_identical_slices(U, name):
  """1 and 2 hypotheses take the one-launch form (where the mesh fits it), 5 the classification launch(es): same images bit for bit"""
  five = _gpu(U, name, 5)
  for n in (1, 2):
    part = _gpu(U, name, n)
    for k in five:
      assert np.array_equal(part[k], five[k][:n]), (name, n, k)


@pytest.mark.parametrize('name', R.PADDED_CASES)
def test_padded_mesh_equals_the_unpadded_one(U, name):
  c = R.lattice_case(name)
  base, ids = c['claims']['base'], c['claims']['remap']
  for n in (1, 5):
    p, b = _gpu(U, name, n), _gpu(U, base, n)
    for k in ('xyz', 'depth', 'color'):
      assert np.array_equal(p[k], b[k]), (name, n, k)
    assert np.array_equal(p['rast'][..., :3], b['rast'][..., :3]), (name, n)
    bi = b['rast'][..., 3].astype(np.int64)
    assert np.array_equal(p['rast'][..., 3].astype(np.int64), np.where(bi > 0, ids[np.maximum(bi, 1) - 1] + 1, 0)), (name, n)


CHILD_CASES = R.BASE_CASES + ['padded_large32_F8192', 'padded_centres_small_F4099_V8200']


def _digest(g):
  h = hashlib.sha1()
  for k in ('rast', 'xyz', 'depth', 'color'):
    h.update(np.ascontiguousarray(g[k]).tobytes())
  return h.hexdigest()


@pytest.mark.parametrize('knob', ['FP_RENDER_SOLO=0', 'FP_RENDER_PREPASS2=1'])
def test_other_launch_forms_give_identical_images(U, knob):
  """A fresh child process (the knobs are read once per process) without the one-launch form / with the vertex pre-pass and the classification as
  two launches: every output of every case at 1, 2 and 5 hypotheses has the digest of this process' render."""
  script = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools', 'raster_lattice_digest.py')
  k, v = knob.split('=')
  r = subprocess.run([sys.executable, script] + CHILD_CASES, env=dict(os.environ, **{k: v}), capture_output=True, text=True, timeout=240)
  assert r.returncode == 0, r.stderr[-1500:]
  got = json.loads([l for l in r.stdout.splitlines() if l.startswith('DIGESTS ')][-1][8:])
  for name in CHILD_CASES:
    for n in (1, 2, 5):
      assert got[name][str(n)] == _digest(_gpu(U, name, n)), (knob, name, n)


def _fp16_ulp(v):
  e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
  return 2.0 ** (e - 10)


@pytest.mark.parametrize('name', ['centres_small', 'depth_signs_mixed', 'large32', 'window_zoom'])
def test_network_tensor_against_float64(name):
  """fp_render_net (render_kernel<1, .>): covered set identical to the reference's, rgb and (xyz - t) 2 / diameter within one fp16 ulp of the float64
  value, zero where the depth is below invalid_thres (all three) or |value| >= 2 (that channel).  diameter 2 and invalid_thres 1.5 put layers on
  both sides of both maskings (depth_signs_mixed: depth = w in {1/2, 1, 2, 4, 8}; the z channel is w - 1)."""
  from foundationpose_amd import _lib
  from foundationpose_amd._lib import check, k_ptr, lib, ptr, stream_ptr
  c = R.with_default_projection(R.lattice_case(name))
  ctx = _lib.Context.get('cuda:0')
  dm = _lib.device_mesh(ctx, {k: torch.as_tensor(v).cuda() for k, v in c['mesh_tensors'].items()})
  Kd, Kp = k_ptr(c['K'])
  diam, thres = 2.0, 1.5
  outs = {}
  for n in (1, 2, 5):
    poses = torch.as_tensor(c['poses'][:n]).cuda().contiguous()
    bb = None if c['bbox2d'] is None else torch.as_tensor(c['bbox2d'][:n]).cuda().contiguous()
    out = torch.zeros((n, c['Ho'], c['Wo'], 8), dtype=torch.float16, device='cuda')
    check(lib().fp_render_net(ctx.handle, dm.handle, ptr(poses), n, Kp, c['H'], c['W'], ptr(bb), c['Ho'], c['Wo'], diam, 1, thres, ptr(out), stream_ptr()))
    torch.cuda.synchronize()
    outs[n] = out.cpu().numpy()
  assert np.array_equal(outs[1], outs[5][:1]) and np.array_equal(outs[2], outs[5][:2])
  sides = np.zeros(4, int)
  worst = 0.0
  for h in range(5):
    cov = R.coverage_exact(c, h)
    ref = R.interp_float64(c, h, cov)
    got = outs[5][h].astype(np.float64)
    assert not got[..., 6:].any()
    x = (ref['xyz'] - c['poses'][h][:3, 3].astype(np.float64)) * 2 / diam
    invalid = ref['depth'] < thres
    big = np.abs(x) >= 2
    assert not (ref['covered'] & (np.abs(ref['depth'] - thres) < 1e-3)).any() and not (ref['covered'][..., None] & (np.abs(np.abs(x) - 2) < 1e-3)).any()
    # make_crop_data_batch renders with use_light: colour 0.8 + 0.5 d, d the interpolated Lambert term = 1 (every normal faces the camera), clipped
    lit = np.clip(ref['color'] * 0.8 + 1.0 * ref['color'] * 0.5, 0, 1)
    want = np.concatenate([lit, np.where(invalid[..., None] | big, 0.0, x)], -1)
    want = np.where(ref['covered'][..., None], want, 0.0)
    # the covered set: colours are k / 256 > 0 almost everywhere; the exact statement is on the pixels the reference leaves empty and on value equality
    assert not got[..., :6][~ref['covered']].any(), (name, h)
    err = np.abs(got[..., :6] - want) / _fp16_ulp(want)
    worst = max(worst, float(err.max()))
    assert err.max() <= 1.0, (name, h, float(err.max()))
    nz = ref['covered'] & (ref['color'].max(-1) > 0)
    assert np.array_equal(got[..., :3].max(-1) > 0, nz), (name, h)
    sides += [int((ref['covered'] & invalid).sum()), int((ref['covered'] & ~invalid).sum()), int((ref['covered'][..., None] & big & ~invalid[..., None]).sum()),
              int((ref['covered'][..., None] & ~big & ~invalid[..., None] & (x != 0)).sum())]
  print('net %s: largest |err| / fp16 ulp %.3f; pixels invalid / valid %d / %d, channels masked / kept %d / %d' % ((name, worst) + tuple(sides)))
  if name == 'depth_signs_mixed':
    assert sides.min() > 0, sides


@pytest.mark.parametrize('name', R.SHADE_CASES)
def test_texture_fetch_and_lighting_against_float64(U, name):
  """Every SHADE case under every light setting at 1, 2 and 5 hypotheses (the one-launch form and the fused classification): winner exactly, colour
  within shade_tol of shade_float64 - bit for bit where the case is exact -, normal map within TOL_ATTR, background exactly 0; the 1- and 2-hypothesis
  renders equal the 5-hypothesis one's slices bit for bit.  Every covered pixel is compared."""
  c = R.lattice_case(name)
  for var in R.shade_variants(name):
    five = render_shaded(U.nvdiffrast_render, c, 5, dev='cuda', **shade_light(var))
    compare_shaded(c, five, 5, 'hip', var)
    for n in (1, 2):
      part = render_shaded(U.nvdiffrast_render, c, n, dev='cuda', **shade_light(var))
      for k in five:
        assert np.array_equal(part[k], five[k][:n]), (name, var, n, k)


@pytest.mark.parametrize('fu,fv', FAR_UV)
def test_texture_fetch_far_from_the_origin(U, fu, fv):
  """a million periods away, and |uv size| beyond the int range (the index reduced in float): the contract's value exactly, on every pixel"""
  c, want = far_uv_case(fu, fv)
  got = render_shaded(U.nvdiffrast_render, c, 1, dev='cuda')
  covered = got['rast'][0][..., 3] > 0
  assert covered.sum() == 512 and np.array_equal(got['color'][0][covered].astype(np.float64), np.tile(want, (512, 1))), (got['color'][0][covered][0], want)


@pytest.mark.parametrize('name', ['tex_identity', 'tex_wrap', 'tex_perspective'])
def test_network_tensor_rgb_of_textured_cases(name):
  """fp_render_net's rgb channels of a textured mesh: 0.8 base + 0.5 d base with d = 1 (make_crop_data_batch's lighting; every normal of these cases faces
  the camera), within one fp16 ulp of float64, zero exactly where the reference covers nothing.  (The cases' texels are >= 1/8: the value never comes
  near the range where an fp16 ulp is smaller than the float32 error of the fetch.)"""
  from foundationpose_amd import _lib
  from foundationpose_amd._lib import check, k_ptr, lib, ptr, stream_ptr
  c = R.with_default_projection(R.lattice_case(name))
  assert c['mesh_tensors']['tex'].min() >= 0.125
  ctx = _lib.Context.get('cuda:0')
  dm = _lib.device_mesh(ctx, {k: torch.as_tensor(v).cuda() for k, v in c['mesh_tensors'].items()})
  Kd, Kp = k_ptr(c['K'])
  outs = {}
  for n in (1, 2, 5):
    poses = torch.as_tensor(c['poses'][:n]).cuda().contiguous()
    out = torch.zeros((n, c['Ho'], c['Wo'], 8), dtype=torch.float16, device='cuda')
    check(lib().fp_render_net(ctx.handle, dm.handle, ptr(poses), n, Kp, c['H'], c['W'], None, c['Ho'], c['Wo'], 2.0, 1, 1.5, ptr(out), stream_ptr()))
    torch.cuda.synchronize()
    outs[n] = out.cpu().numpy()
  assert np.array_equal(outs[1], outs[5][:1]) and np.array_equal(outs[2], outs[5][:2])
  worst = 0.0
  for h in range(5):
    cov = R.coverage_exact(c, h)
    ref = R.shade_float64(c, h, cov, use_light=True)
    got = outs[5][h].astype(np.float64)[..., :3]
    assert not got[~ref['covered']].any() and np.array_equal(got.max(-1) > 0, ref['covered']), (name, h)
    err = np.abs(got - ref['color']) / _fp16_ulp(ref['color'])
    worst = max(worst, float(err.max()))
    assert err.max() <= 1.0, (name, h, float(err.max()))
  print('net rgb %s: largest |err| / fp16 ulp %.3f' % (name, worst))


def test_slanted_quad_against_float64_point_in_triangle(U):
  """tests/test_oracle_independent.py's fronto-parallel quad at a general (not lattice) position, on the kernel: coverage equals a float64 inside test
  farther than 1/8 px from an edge, depth the plane's z, xyz the back-projected ray (same exclusion rule and shares as the oracle's test)."""
  K = np.array([[500.0, 0, 80.3], [0, 480.0, 59.6], [0, 0, 1]])
  H, W = 120, 160
  z = 0.8
  quad = np.array([[-0.071, -0.052, 0], [0.064, -0.047, 0], [0.058, 0.049, 0], [-0.066, 0.055, 0]], np.float32)
  mt = dict(pos=torch.from_numpy(quad).cuda(), faces=torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32).cuda(),
            vnormals=torch.tensor([[0, 0, -1.0]] * 4).cuda(), vertex_color=torch.tensor([[1.0, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0]]).cuda())
  pose = np.eye(4, dtype=np.float32)
  pose[:3, 3] = [0.003, -0.002, z]
  extra = {}
  color, depth, _ = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=torch.from_numpy(pose[None]).cuda(), mesh_tensors=mt, use_light=False, extra=extra)
  depth, xyz = depth[0].cpu().numpy(), extra['xyz_map'][0].cpu().numpy()
  P = quad.astype(np.float64) + pose[:3, 3].astype(np.float64)
  uv = np.c_[K[0, 0] * P[:, 0] / P[:, 2] + K[0, 2], K[1, 1] * P[:, 1] / P[:, 2] + K[1, 2]]
  jj, ii = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing='ij')
  inside = np.ones((H, W), bool)
  dist = np.full((H, W), np.inf)
  for a in range(4):
    p, q = uv[a], uv[(a + 1) % 4]
    e = (q[0] - p[0]) * (jj - p[1]) - (q[1] - p[1]) * (ii - p[0])
    inside &= e > 0
    dist = np.minimum(dist, np.abs(e) / np.hypot(*(q - p)))
  sure = dist > 0.125
  assert sure.mean() > 0.95 and inside[sure].sum() > 2000
  assert np.array_equal(depth[sure] > 0, inside[sure])
  cov = sure & inside
  np.testing.assert_allclose(depth[cov], z, atol=2e-6)
  np.testing.assert_allclose(xyz[cov][:, 0], (ii[cov] - K[0, 2]) * z / K[0, 0], atol=z / K[0, 0] / 16)
  np.testing.assert_allclose(xyz[cov][:, 1], (jj[cov] - K[1, 2]) * z / K[1, 1], atol=z / K[1, 1] / 16)
  c = color[0].cpu().numpy()[cov]
  assert c.min() >= -1e-6 and c.max() <= 1 + 1e-6 and np.abs(c.sum(1) - 1).max() < 1.0 + 1e-6


def test_ground_plane_through_the_camera_against_the_analytic_plane(U):
  """tests/test_oracle_independent.py's ground plane from 1 m behind the camera to 3 m in front, on the kernel: every triangle has a vertex with
  w <= 0, so the whole image comes from the homogeneous path (same margins and shares as the oracle's test)."""
  K = np.array([[300.0, 0, 79.5], [0, 300.0, 40.25], [0, 0, 1]])
  H, W, h = 120, 160, 0.1
  plane = np.array([[-1, h, -1], [1, h, -1], [1, h, 3], [-1, h, 3]], np.float32)
  mt = dict(pos=torch.from_numpy(plane).cuda(), faces=torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32).cuda(),
            vnormals=torch.tensor([[0, -1.0, 0]] * 4).cuda(), vertex_color=torch.tensor([[1.0, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0]]).cuda())
  extra = {}
  _, depth, _ = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=torch.eye(4)[None].cuda(), mesh_tensors=mt, use_light=False, extra=extra)
  depth, xyz = depth[0].cpu().numpy(), extra['xyz_map'][0].cpu().numpy()
  jj, ii = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing='ij')
  with np.errstate(divide='ignore'):
    z = np.where(jj > K[1, 2], h * K[1, 1] / (jj - K[1, 2]), np.inf)
  x = (ii - K[0, 2]) * z / K[0, 0]
  inside = (z <= 3.0) & (np.abs(x) <= 1.0)
  below = jj > K[1, 2] + 1.5
  zz, xx = np.where(below, z, 1.0), np.where(below, x, 0.0)
  margin = (jj < K[1, 2] - 1.5) | (below & (np.abs(zz - 3.0) > 0.05) & (np.abs(np.abs(xx) - 1.0) > 0.02 * zz))
  assert inside[margin].sum() > 5000 and (~inside)[margin].sum() > 5000
  assert np.array_equal(depth[margin] > 0, inside[margin])
  cov = margin & inside
  np.testing.assert_allclose(depth[cov], z[cov], rtol=2e-4)
  np.testing.assert_allclose(xyz[cov][:, 1], h, atol=2e-5)
  ex = np.abs(xyz[cov][:, 0] - x[cov]) / np.maximum(1.0, np.abs(x[cov]))
  assert ex.max() < 2e-4, ex.max()
  assert np.abs(np.diff(depth, axis=1))[cov[:, 1:] & cov[:, :-1]].max() < 1e-3
