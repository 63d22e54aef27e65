"""GPU: warping through a camera model (fp_remap, csrc/rectify.hip) against tests/rectify_oracle.py.  Image, validity mask and the (u, v)
map are compared BIT FOR BIT: the map is fp32 with every operation rounded once in the header's order, the blend is integer, the depth
rule one correctly rounded division.  The shapes are the smallest at which the kernel can still go wrong: 37 x 53 (narrower than a wave,
1961 pixels: no multiple of the four pixels a thread owns, so the last thread takes the element stores) and 64 x 200 (several blocks),
grey and RGB, size_new != size, pairs (two plans in one launch) and batches (threads whose four pixels span two images)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import rectify_oracle as O

pytestmark = pytest.mark.gpu

SINGLE = ('mild', 'barrel', 'rational')


def noise(shape, seed):
  return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def bits(a):
  a = np.ascontiguousarray(a)
  return a.view(np.uint8 if a.dtype.itemsize == 1 else f'u{a.dtype.itemsize}')


def assert_same_bits(got, want, what):
  assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
  bad = bits(got) != bits(want)
  assert not bad.any(), f'{what}: differs in {int(bad.sum())} of {bad.size} entries, first at {tuple(np.argwhere(bad)[0])}'


def product_plans(src, dst):
  """name -> the product's RemapPlan for the oracle's test plans (tests/test_rectify_host.py shows they hold the same fp32 values)."""
  from foundationpose_amd import Utils as U
  from foundationpose_amd import rectify
  args = O.case_arguments(src, dst)
  rect = U.rectify_stereo(*args['rectification'])
  return dict(rect=rect, **{k: rectify.RemapPlan(*args[k]) for k in SINGLE})


@pytest.mark.parametrize('channels', [1, 3], ids=['grey', 'rgb'])
@pytest.mark.parametrize('sizes', O.SIZES, ids=lambda s: f'{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}')
def test_image_valid_and_map_equal_the_oracle(sizes, channels):
  from foundationpose_amd import Utils as U
  src, dst = sizes
  plans, ref = product_plans(src, dst), O.case_plans(src, dst)
  shape = src + ((3,) if channels == 3 else ())
  img, img2 = noise(shape, 1), noise(shape, 2)
  for name in SINGLE:
    out, valid, uv = U.remap_image(img, plans[name], return_valid=True, return_debug=True)
    want = O.remap_colour(img, ref[name])
    assert_same_bits(out, want['out'], f'{name} image')
    assert_same_bits(valid, want['valid'], f'{name} valid')
    assert_same_bits(uv, want['map'], f'{name} map')
    assert (out[valid == 0] == 0).all()
  # the barrel case does what it is there for: the map leaves the source on all four sides and rays cross r2_max
  m = O.remap_colour(img, ref['barrel'])
  u, v = m['map'][..., 0], m['map'][..., 1]
  assert not m['valid'][0].any() and not m['valid'][-1].any() and not m['valid'][:, 0].any() and not m['valid'][:, -1].any() and m['valid'].any()
  with np.errstate(invalid='ignore'):
    assert np.isnan(u).any() and (u < 0).any() and (u > src[1] - 1).any() and (v < 0).any() and (v > src[0] - 1).any()
  # the rectification: both images in one call
  l, r, (vl, vr), (ml, mr) = U.rectify_pair(img, img2, plans['rect'], return_valid=True, return_debug=True)
  for got, gv, gm, source, side in ((l, vl, ml, img, 'rect_left'), (r, vr, mr, img2, 'rect_right')):
    want = O.remap_colour(source, ref[side])
    assert_same_bits(got, want['out'], f'{side} image')
    assert_same_bits(gv, want['valid'], f'{side} valid')
    assert_same_bits(gm, want['map'], f'{side} map')
    assert 0 < want['valid'].mean() < 1 or dst != src


def test_identity_plan_reproduces_its_input():
  from foundationpose_amd import Utils as U
  for shape, K in (((37, 53, 3), [[47.7, 0, 26.2], [0, 48.6, 18.9], [0, 0, 1]]), ((64, 200), [[1067.51, 0, 99.37], [0, 1067.9, 31.81], [0, 0, 1]])):
    img = noise(shape, 3)
    out, valid = U.remap_image(img, U.undistort_plan(np.array(K), [], shape[:2]), return_valid=True)
    assert (out == img).all() and (valid == 1).all(), shape


def test_integer_principal_point_offset_is_an_integer_shift():
  from foundationpose_amd import Utils as U
  img = noise((37, 53, 3), 4)
  K = np.array([[47.7, 0, 26.2], [0, 48.6, 18.9], [0, 0, 1]])
  Ks = K.copy()
  Ks[0, 2] += 5
  Ks[1, 2] -= 3      # new pixel (col, row) shows raw pixel (col - 5, row + 3)
  out, valid = U.remap_image(img, U.undistort_plan(K, [], (37, 53), K_new=Ks), return_valid=True)
  assert (out[:34, 5:] == img[3:, :48]).all() and (valid[:34, 5:] == 1).all()
  assert not valid[34:].any() and not valid[:, :5].any() and not out[34:].any() and not out[:, :5].any()


def raw_depth(shape, seed):
  rng = np.random.default_rng(seed)
  d = rng.uniform(0.3, 2.0, shape).astype(np.float32)
  d[rng.random(shape) < 0.1] = 0.0
  d[rng.random(shape) < 0.05] = np.nan
  d[rng.random(shape) < 0.02] = np.inf
  d[rng.random(shape) < 0.02] = 0.0005      # below depth_ok's 0.001
  d[rng.random(shape) < 0.02] = -1.0
  return d


@pytest.mark.parametrize('sizes', [O.SIZES[0], O.SIZES[3]], ids=['37x53', '64x200to50x170'])
def test_depth_mode(sizes):
  from foundationpose_amd import Utils as U
  src, dst = sizes
  plans, ref = product_plans(src, dst), O.case_plans(src, dst)
  depth = raw_depth(src, 5)
  good = np.isfinite(depth) & (depth >= 0.001)
  # a pure undistortion copies bits and never makes a value that the source does not hold
  for name in SINGLE:
    out, valid, uv = U.remap_image(depth, plans[name], mode='depth', return_valid=True, return_debug=True)
    want = O.remap_depth(depth, ref[name])
    assert_same_bits(out, want['out'], f'{name} depth')
    assert_same_bits(valid, want['valid'], f'{name} valid')
    assert_same_bits(uv, want['map'], f'{name} map')
    assert np.isin(bits(out[out != 0]), bits(depth[good])).all() and (out[valid == 0] == 0).all() and np.isfinite(out).all()
    assert (out != 0).any()
  # with a rotation: out = z_raw / d_raw.z per the oracle, bit for bit; zeros, NaNs and everything that is no depth give 0
  for plan, o in ((plans['rect'].left, ref['rect_left']), (plans['rect'].right, ref['rect_right'])):
    out, valid = U.remap_image(depth, plan, mode='depth', return_valid=True)
    want = O.remap_depth(depth, o)
    assert_same_bits(out, want['out'], 'rotated depth')
    assert_same_bits(valid, want['valid'], 'rotated valid')
    assert np.isfinite(out).all() and (out >= 0).all() and (out != 0).any() and ((valid == 1) & (out == 0)).any()
    assert (want['Z'] != 1).any()      # the division does something here
  # zfar, and undistort_frame with either input missing
  near = U.remap_image(depth, plans['mild'], mode='depth', zfar=1.0)
  assert_same_bits(near, O.remap_depth(depth, ref['mild'], zfar=1.0)['out'], 'zfar')
  assert (near < 1.0).all() and (near > 0).any()
  rgb = noise(src + (3,), 6)
  both = U.undistort_frame(rgb, depth, plans['mild'])
  assert_same_bits(both[0], O.remap_colour(rgb, ref['mild'])['out'], 'undistort_frame rgb')
  assert_same_bits(both[1], O.remap_depth(depth, ref['mild'])['out'], 'undistort_frame depth')
  assert U.undistort_frame(None, depth, plans['mild'])[0] is None and U.undistort_frame(rgb, None, plans['mild'])[1] is None


def test_pair_batch_numpy_and_device_inputs_agree():
  """A pair in one call equals two single calls; a batch of 3 pairs equals single pairs (a thread's four pixels span two images there:
  45 x 61 is odd); numpy in equals device in."""
  from foundationpose_amd import Utils as U
  src, dst = O.SIZES[2]
  rect = product_plans(src, dst)['rect']
  lefts, rights = noise((3,) + src + (3,), 7), noise((3,) + src + (3,), 8)
  bl, br, (bvl, bvr) = U.rectify_pair(lefts, rights, rect, return_valid=True)
  assert bl.shape == (3,) + dst + (3,) and bvl.shape == (3,) + dst and isinstance(bl, np.ndarray)
  for i in range(3):
    l, r, (vl, vr) = U.rectify_pair(lefts[i], rights[i], rect, return_valid=True)
    assert (l == bl[i]).all() and (r == br[i]).all() and (vl == bvl[i]).all() and (vr == bvr[i]).all(), i
    one_l, one_vl = U.remap_image(lefts[i], rect.left, return_valid=True)
    one_r, one_vr = U.remap_image(rights[i], rect.right, return_valid=True)
    assert (one_l == l).all() and (one_r == r).all() and (one_vl == vl).all() and (one_vr == vr).all(), i
  dl, dr = U.rectify_pair(torch.as_tensor(lefts).cuda(), torch.as_tensor(rights).cuda(), rect)
  assert torch.is_tensor(dl) and dl.is_cuda and dl.dtype == torch.uint8 and (dl.cpu().numpy() == bl).all() and (dr.cpu().numpy() == br).all()
  grey = U.remap_image(torch.as_tensor(lefts[..., 0].copy()).cuda(), rect.left)      # a grey batch (n,H,W)
  assert grey.is_cuda and tuple(grey.shape) == (3,) + dst
  for i in range(3):
    assert (grey[i].cpu().numpy() == U.remap_image(np.ascontiguousarray(lefts[i, ..., 0]), rect.left)).all()


def test_repeatable_and_no_stale_state():
  from foundationpose_amd import Utils as U
  big, small = product_plans(*O.SIZES[1]), product_plans(*O.SIZES[0])
  img = noise((64, 200, 3), 9)
  first = U.remap_image(img, big['barrel'], return_valid=True, return_debug=True)
  again = U.remap_image(img, big['barrel'], return_valid=True, return_debug=True)
  U.remap_image(noise((37, 53), 10), small['rational'])
  third = U.remap_image(img, big['barrel'], return_valid=True, return_debug=True)
  for a, b, c in zip(first, again, third):
    assert (bits(a) == bits(b)).all() and (bits(a) == bits(c)).all()


def test_outputs_that_are_not_aligned_take_the_element_stores():
  """The dword / float4 stores need 16-byte aligned outputs; a caller of the C interface may pass others.  Same bits either way."""
  from foundationpose_amd import _lib
  src, dst = O.SIZES[1]
  plan = product_plans(src, dst)['mild']
  img = noise(src + (3,), 11)
  want = O.remap_colour(img, O.case_plans(src, dst)['mild'])
  d_img = torch.as_tensor(img).cuda()
  n_px = dst[0] * dst[1]
  out, valid, uv = (torch.zeros(n_px * 3 + 16, dtype=torch.uint8).cuda(), torch.zeros(n_px + 16, dtype=torch.uint8).cuda(),
                    torch.zeros(n_px * 2 + 4, dtype=torch.float32).cuda())
  o = _lib.FpRemapOpts(struct_size=ctypes.sizeof(_lib.FpRemapOpts), mode=_lib.FP_REMAP_COLOUR, channels=3, n_plans=1, zfar=float('inf'))
  o.plan[0] = plan.as_struct()
  dbg = _lib.FpRemapDebug(struct_size=ctypes.sizeof(_lib.FpRemapDebug), d_map0=uv.data_ptr() + 4, d_map1=None)
  _lib.check(_lib.lib().fp_remap(_lib.Context.get(d_img.device).handle, _lib.ptr(d_img), None, 1, ctypes.byref(o), ctypes.c_void_p(out.data_ptr() + 1), None,
                                 ctypes.c_void_p(valid.data_ptr() + 3), None, ctypes.byref(dbg), _lib.stream_ptr(d_img.device)))
  torch.cuda.synchronize()
  assert_same_bits(out.cpu().numpy()[1:1 + n_px * 3].reshape(dst + (3,)), want['out'], 'image')
  assert_same_bits(valid.cpu().numpy()[3:3 + n_px].reshape(dst), want['valid'], 'valid')
  assert_same_bits(uv.cpu().numpy()[1:1 + n_px * 2].reshape(dst + (2,)), want['map'], 'map')
  assert out[0] == 0 and not out[1 + n_px * 3:].any() and valid[:3].sum() == 0 and not valid[3 + n_px:].any()      # nothing beside the arrays


@pytest.fixture(scope='module')
def scene():
  """The analytic raw pair of tests/test_rectify_host.py and its CPU result, computed once and never written to."""
  s = O.raw_plane_scene()
  return s, O.end_to_end(s)


def test_captured_graph_equals_eager(scene):
  from foundationpose_amd import Utils as U
  from foundationpose_amd import rectify, stereo
  s, e = scene
  rect = U.rectify_stereo(s['K1'], s['dist1'], s['K2'], s['dist2'], s['R'], s['T'], s['left'].shape)
  left, right = torch.as_tensor(s['left']).cuda()[None], torch.as_tensor(s['right']).cuda()[None]
  f, b = float(rect.K_new[0, 0]), rect.baseline

  def call():
    (l, r), _, _ = rectify.remap([left, right], [rect.left, rect.right])
    return stereo.sgm(l, r, max_disparity=64, fx=f, baseline=b)[:2]

  eager = [t.clone() for t in call()]      # also the warm-up: the working memory of the matching is allocated outside the capture
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = call()
  for t in out:
    t.zero_()
  graph.replay()
  torch.cuda.synchronize()
  for a, c, name in zip(out, eager, ('disparity', 'depth')):
    assert torch.equal(a.view(torch.int32), c.view(torch.int32)), name
  assert_same_bits(eager[1][0].cpu().numpy(), e['depth'], 'depth')


def test_raw_pair_to_metric_depth_end_to_end(scene):
  """stereo_depth(raw_left, raw_right, rectify=rect) on the analytic scene of tests/rectify_oracle.raw_plane_scene (a textured plane seen by
  two distorted cameras, the right one rotated by 1.9 degrees and 4 mm off in y; 48 x 176, 64 disparities) equals the CPU result bit for
  bit, so the figures are those measured on the CPU (tests/test_rectify_host.py): 0.9009 of the pixels with x >= 64 valid, median
  |disparity - f b / z_rect| 0.139 px; the same pair without rectify=: 0.432 valid, 16.0 px.  Asserted: >= 0.85 and <= 0.20 px with;
  <= 0.60 and >= 2 px without."""
  from foundationpose_amd import Utils as U
  from foundationpose_amd.pipeline import Pipeline, PipelineData, StereoDepth, StereoRectify
  s, e = scene
  rect = U.rectify_stereo(s['K1'], s['dist1'], s['K2'], s['dist2'], s['R'], s['T'], s['left'].shape)
  depth = U.stereo_depth(s['left'], s['right'], rectify=rect, max_disparity=64)
  assert_same_bits(depth, e['depth'], 'depth with rectify=')
  raw = U.stereo_depth(s['left'], s['right'], s['K1'], rect.baseline, max_disparity=64)
  assert_same_bits(raw, e['raw_depth'], 'depth without rectify=')
  f, b = float(rect.K_new[0, 0]), rect.baseline
  share, err = O.figures(depth, f, b, O.plane_depth(rect.K_new, rect.R1.T, depth.shape, s['plane']), 64)
  raw_share, raw_err = O.figures(raw, float(s['K1'][0, 0]), b, O.plane_depth(s['K1'], np.eye(3), raw.shape, s['plane']), 64)
  print(f'with rectify=: {share:.4f} valid, median error {err:.4f} px; without: {raw_share:.4f} valid, {raw_err:.3f} px')
  assert share >= 0.85 and err <= 0.20
  assert raw_share <= 0.60 and raw_err >= 2.0
  # the pipeline stages give the same depth, on the device
  data = Pipeline('raw stereo').add_processor(StereoRectify(rect)).add_processor(StereoDepth(max_disparity=64)).run(
    PipelineData(rgb=torch.as_tensor(s['left']).cuda(), right=torch.as_tensor(s['right']).cuda()))
  assert not data.errors and data.depth.is_cuda and (data.K == rect.K_new).all()
  assert_same_bits(data.depth.cpu().numpy(), e['depth'], 'pipeline depth')


def scene_calibration_file(s):
  """The cameras of the analytic scene as a sectioned calibration file in millimetres, as mesh_io.load_stereo_calibration reads it."""
  lines = []
  for name, K, d in (('LEFT_CAM_FHD1200', s['K1'], s['dist1']), ('RIGHT_CAM_FHD1200', s['K2'], s['dist2'])):
    lines += [f'[{name}]', f'fx={float(K[0, 0])!r}', f'fy={float(K[1, 1])!r}', f'cx={float(K[0, 2])!r}', f'cy={float(K[1, 2])!r}']
    lines += [f'{k}={float(v)!r}' for k, v in zip(('k1', 'k2', 'p1', 'p2', 'k3'), d) if v != 0] + ['']
  return '\n'.join(lines + ['[STEREO]', 'Baseline=100', 'TY=4', 'TZ=1', 'RX_FHD1200=0.025', 'CV_FHD1200=-0.01', 'RZ_FHD1200=0.02', ''])


def test_command_line_tool_rectifies_with_a_calibration_file(scene, tmp_path):
  """scripts/stereo_depth.py RAW_LEFT RAW_RIGHT --calibration FILE: image files and a calibration file in, metric depth out, with no
  library outside this one - the same bits as stereo_depth(rectify=) gives in the process of the test."""
  import os
  import subprocess
  import sys
  from PIL import Image
  from foundationpose_amd import Utils as U
  s, e = scene
  (tmp_path / 'camera.conf').write_text(scene_calibration_file(s))
  for name in ('left', 'right'):
    Image.fromarray(s[name]).save(tmp_path / f'{name}.png')
  repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  out = tmp_path / 'depth.npy'
  p = subprocess.run([sys.executable, os.path.join(repo, 'scripts', 'stereo_depth.py'), str(tmp_path / 'left.png'), str(tmp_path / 'right.png'),
                      '--calibration', str(tmp_path / 'camera.conf'), '--max-disparity', '64', '-o', str(out)], capture_output=True, text=True, timeout=120)
  assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
  rect = U.rectify_stereo(s['K1'], s['dist1'], s['K2'], s['dist2'], s['R'], s['T'], s['left'].shape)
  assert_same_bits(np.load(out), e['depth'], 'depth.npy')
  assert np.abs(np.loadtxt(str(out) + '.K.txt') - rect.K_new).max() < 1e-12
