"""CPU: registering depth into another camera - the numpy restatement tests/depth_reproject_oracle.py pinned against an independent float64
brute force and against hand-made cases, the figures of the end-to-end scene that the GPU test asserts as well, the refusals of
fp_depth_reproject that need no GPU, rgbd_rig against undistort_plan, the pipeline stage with a stubbed kernel call, gather_by_source and
the calibration file's round trip."""
import ctypes

import numpy as np
import pytest

from foundationpose_amd import Utils as U
from foundationpose_amd import mesh_io, reproject
from tests import depth_reproject_oracle as O

F = np.float32


def lattice_scene():
  """A far plane at 1 m with a near rectangle (0.5 m) and a second one (0.8 m), seen after a pure translation (0.02, -0.0125, 0) by a
  camera magnified 1.25 x.  With tz = 0 and no rotation u is linear in the source column: u = 1.25 c + (cx_dst - 1.25 cx_src + 50 x 0.02 / d),
  and 50 x 0.02 / d is 1, 2 and 1.25 at the three depths - multiples of 0.25.  cx_dst, cy_dst are chosen so that every footprint edge has
  the fraction 0.0625 + k / 4 and every centre-rounding boundary 0.1875 + k / 4: nothing within 0.06 px of a pixel centre, so fp32 and
  float64 decide every pixel alike."""
  Hs, Ws = 24, 32
  K_src = np.array([[40.0, 0, 15.5], [0, 32.0, 11.5], [0, 0, 1]])
  K_dst = np.array([[50.0, 0, 1.25 * 15.5 + 0.6875 - 1.0], [0, 40.0, 1.25 * 11.5 + 0.6875 + 0.5], [0, 0, 1]])
  d = np.full((Hs, Ws), 1.0, F)
  d[6:16, 8:20] = 0.5
  d[3:8, 22:30] = 0.8
  d[20, 5], d[1, 1] = 0, np.nan
  return d, K_src, O.transform(None, [0.02, -0.0125, 0.0]), K_dst, (34, 44)


def test_restatement_equals_the_float64_brute_force():
  """The brute force shares no code with the restatement: per source pixel the float64 footprint, per target pixel the nearest float64 z
  among the footprints that cover its centre.  Sources are equal on every pixel; with tz = 0 and R = 1 the depth is the source depth
  itself, so the depths are equal too."""
  d, K_src, T, K_dst, size = lattice_scene()
  got = O.reproject(d[None], [K_src], [T], K_dst, size)
  depth, source, excluded = O.brute_force64(d, K_src, T, K_dst, size)
  assert excluded == 0
  assert got['capped'] == 0 and got['behind'] == 0
  assert (got['source'] == source).all() and (got['depth'].astype(np.float64) == depth).all()
  filled = source >= 0
  assert 0.7 < filled.mean() < 0.85      # the magnified image is larger than what the source sees; shadows of the rectangles stay empty
  assert set(np.unique(depth)) == {0.0, 0.5, float(F(0.8)), 1.0}
  # the near rectangle hides the plane: its 12 columns x 10 rows cover 15 x 12.5 target pixels, shifted by 2 px against the plane
  assert (depth == 0.5).sum() in range(12 * 15 - 15, 13 * 16)


def test_rule_by_hand():
  # identity: every depth lands on its own pixel, bit for bit; 0, NaN and beyond zfar arrive nowhere
  d = O.random_depth((1, 37, 53), 3, zfar=1.6)
  got = O.reproject(d, [O.K_SMALL], [np.eye(4)], O.K_SMALL, (37, 53), zfar=1.6)
  ok = O.depth_ok(d[0], 1.6)
  assert 0.8 < ok.mean() < 0.95
  assert (got['depth'].view(np.uint32) == np.where(ok, d[0], F(0)).view(np.uint32)).all()
  assert (got['source'] == np.where(ok, np.arange(37 * 53).reshape(37, 53), -1)).all()
  # a 4 x reduction of a constant plane: every target pixel takes the lowest index of the 16 source pixels whose centres round to it
  K = np.array([[40.0, 0, 7.5], [0, 40.0, 5.5], [0, 0, 1]])
  Kq = np.array([[10.0, 0, 1.5], [0, 10.0, 1.0], [0, 0, 1]])      # u = (c - 7.5) / 4 + 1.5: c = 0 .. 3 -> -0.375 .. 0.375 -> pixel 0 (floor(u + 0.5))
  got = O.reproject(np.full((1, 12, 16), 0.9, F), [K], [np.eye(4)], Kq, (3, 4))
  rows = np.floor((np.arange(12) - 5.5) / 4 + 1.0 + 0.5).astype(int)
  cols = np.floor((np.arange(16) - 7.5) / 4 + 1.5 + 0.5).astype(int)
  want = np.array([[min(r * 16 + c for r in range(12) for c in range(16) if rows[r] == y and cols[c] == x) for x in range(4)] for y in range(3)])
  assert (got['source'] == want).all() and (got['depth'] == F(0.9)).all()
  # two views, the second nearer: it wins; equal depths: the first wins
  two = np.stack([np.full((12, 16), 0.9, F), np.full((12, 16), 0.7, F)])
  got = O.reproject(two, [K, K], [np.eye(4), np.eye(4)], K, (12, 16))
  assert (got['depth'] == F(0.7)).all() and (got['source'] == 192 + np.arange(192).reshape(12, 16)).all()
  got = O.reproject(np.stack([two[0], two[0]]), [K, K], [np.eye(4), np.eye(4)], K, (12, 16))
  assert (got['source'] == np.arange(192).reshape(12, 16)).all()


def test_grazing_scene_takes_the_cap_and_the_guard():
  got = O.reproject(*O.grazing_case())
  assert got['capped'] > 100 and got['behind'] > 10 and (got['depth'] > 0).sum() > 200


def test_end_to_end_figures_of_the_analytic_scene():
  """A sphere of radius 0.12 m at 0.7 m in front of a plane at 1.2 m, a 48 x 64 depth camera, the colour camera 5 cm to the side and
  turned by 1.9 degrees, at 72 x 96 and at 30 x 40, through the restatement - bit-equal to the device path, so these are the device's
  numbers (tests/test_gpu_depth_reproject.py asserts that).  Measured over the filled pixels, 72 x 96 / 30 x 40: median |aligned -
  analytic| 0.176 / 0.253 mm; share beyond 2 cm (the occlusion rim) 0.41 / 0.93 %; filled 0.950 / 0.991.  Asserted at twice the figures:
  median <= 0.352 / 0.505 mm, beyond 2 cm <= 0.82 / 1.85 %; filled >= 0.93.
  The point of the feature: the sphere's mask of the colour image read from the UNALIGNED depth map (resized to the colour size) shows the
  plane instead of the sphere - an error above the 0.38 m between them - on 24.6 / 27.4 % of the mask's half towards the depth camera
  and on 1.5 / 2.7 % of the other half; in the aligned depth 1.0 / 0 % and 0 / 0 %.  A 5 cm offset at 0.7 m and fx = 93 is a shift of
  6.6 px against a radius of 16 px: a crescent of about 2 x 6.6 / (pi x 16) = 26 % of the disc, all of it in one half.  Asserted: >= 13 %
  of that half unaligned (half the estimate), <= 2 % aligned."""
  bounds = {(72, 96): (0.352e-3, 0.0082), (30, 40): (0.505e-3, 0.0185)}
  for size, (median, beyond) in bounds.items():
    e = O.end_to_end(size)
    print(size, {k: np.round(v, 5) for k, v in e.items() if k not in ('raw', 'aligned')})
    assert e['median'] <= median and e['beyond'] <= beyond and e['filled'] >= 0.93
    assert max(e['naive_wrong']) >= 0.13 and max(e['aligned_wrong']) <= 0.02
    assert e['naive_wrong'][0] > 5 * e['naive_wrong'][1]      # one side of the sphere


@pytest.fixture(scope='module')
def built():
  import __graft_entry__ as g
  g.build()
  from foundationpose_amd import _lib
  return _lib


def test_argument_checks_need_no_gpu(built):
  L = built.lib()
  fake = ctypes.c_void_p(64)      # never dereferenced: every check of a value comes first
  K = np.array([[50.0, 0, 8], [0, 50.0, 6], [0, 0, 1]])

  def call(ctx=fake, depth=fake, n=1, V=2, Hs=12, Ws=16, Ks=True, Ts=True, Kd=True, Hd=9, Wd=11, zfar=float('inf'), keys=fake, out=fake, source=None,
           k_entry=None, t_entry=None, kd_entry=None):
    ks, ts, kd = np.stack([K] * 8), np.stack([np.eye(4)] * 8), K.copy()
    for arr, e in ((ks, k_entry), (ts, t_entry), (kd, kd_entry)):
      if e is not None:
        arr.reshape(-1)[e[0]] = e[1]
    p = lambda a, on: built.ptr(a) if on else None
    return L.fp_depth_reproject(ctx, depth, n, V, Hs, Ws, p(ks, Ks), p(ts, Ts), p(kd, Kd), Hd, Wd, zfar, keys, out, source, None)

  nan, inf = float('nan'), float('inf')
  bad = [dict(ctx=None), dict(depth=None), dict(Ks=False), dict(Ts=False), dict(Kd=False), dict(keys=None), dict(out=None),
         dict(n=0), dict(n=-1), dict(n=1 << 16), dict(V=0), dict(V=9), dict(V=-1), dict(Hs=0), dict(Ws=0), dict(Hd=0), dict(Wd=-3),
         dict(Hs=(1 << 14) + 1), dict(Ws=1 << 15), dict(Hd=(1 << 14) + 1), dict(Wd=1 << 20),
         dict(V=8, Hs=1 << 14, Ws=1 << 14),      # 2^31 source pixels
         dict(k_entry=(0, nan)), dict(k_entry=(9 + 2, inf)), dict(k_entry=(9 + 4, 0.0)), dict(k_entry=(0, -5.0)), dict(k_entry=(5, 1e300)),
         dict(t_entry=(3, nan)), dict(t_entry=(16 + 5, -inf)), dict(t_entry=(11, 1e39)), dict(kd_entry=(0, 0.0)), dict(kd_entry=(4, nan)), dict(kd_entry=(2, inf)),
         dict(zfar=0.0), dict(zfar=-1.0), dict(zfar=nan), dict(keys=ctypes.c_void_p(68))]
  for kw in bad:
    assert call(**kw) == built.FP_EINVAL, kw
    assert L.fp_last_error()
  assert call(V=9) == built.FP_EINVAL and b'V 9' in L.fp_last_error()
  assert call(keys=ctypes.c_void_p(68)) == built.FP_EINVAL and b'8-byte aligned' in L.fp_last_error()
  assert call(V=8, Hs=1 << 14, Ws=1 << 14) == built.FP_EINVAL and b'2^31 - 1' in L.fp_last_error()
  assert call(zfar=0.0) == built.FP_EINVAL and b'zfar' in L.fp_last_error()
  assert (built.FP_REPROJECT_MAX_VIEWS, built.FP_REPROJECT_MAX_SPLAT) == (O.MAX_VIEWS, O.MAX_SPLAT)


def test_refusals_on_the_host():
  d = np.zeros((1, 4, 6), F)
  K = np.array([[5.0, 0, 3], [0, 5.0, 2], [0, 0, 1]])
  with pytest.raises(ValueError, match='float32'):
    U.reproject_depth(d.astype(np.float64), [K], [np.eye(4)], K, (4, 6), device='cpu')
  with pytest.raises(ValueError, match=r'\(V, H, W\)'):
    U.reproject_depth(d[0], [K], [np.eye(4)], K, (4, 6), device='cpu')
  with pytest.raises(ValueError, match='views'):
    U.reproject_depth(np.zeros((9, 4, 6), F), [K] * 9, [np.eye(4)] * 9, K, (4, 6), device='cpu')
  with pytest.raises(ValueError, match='Ks must be'):
    U.reproject_depth(np.zeros((2, 4, 6), F), [K], [np.eye(4)] * 2, K, (4, 6), device='cpu')
  with pytest.raises(ValueError, match='T_dst_src must be'):
    U.reproject_depth(np.zeros((2, 4, 6), F), [K] * 2, np.eye(4), K, (4, 6), device='cpu')
  with pytest.raises(ValueError, match='finite'):
    U.reproject_depth(d, [K], [np.full((4, 4), np.nan)], K, (4, 6), device='cpu')
  with pytest.raises(ValueError, match='positive'):
    U.reproject_depth(d, [K], [np.eye(4)], np.diag([0.0, 1.0, 1.0]), (4, 6), device='cpu')
  with pytest.raises(ValueError, match='H, W'):
    U.reproject_depth(d, [K], [np.eye(4)], K, (4, 1 << 15), device='cpu')
  with pytest.raises(ValueError, match='zfar'):
    U.reproject_depth(d, [K], [np.eye(4)], K, (4, 6), zfar=0.0, device='cpu')
  with pytest.raises(ValueError, match='rigid'):
    U.rgbd_rig(K, [], K, [], 1.1 * np.eye(4), (4, 6), (4, 6))
  with pytest.raises(ValueError, match='4x4'):
    U.rgbd_rig(K, [], K, [], np.eye(3), (4, 6), (4, 6))
  rig = U.rgbd_rig(K, [], K, [], np.eye(4), (4, 6), (8, 12))
  with pytest.raises(ValueError, match='depth size'):
    U.align_frame(None, np.zeros((8, 12), F), rig, device='cpu')


def test_rgbd_rig_against_undistort_plan():
  Kd = np.array([[60.0, 0, 31.5], [0, 61.0, 23.5], [0, 0, 1]])
  Kc = np.array([[90.0, 0, 48.2], [0, 91.0, 35.1], [0, 0, 1]])
  T = O.T_COLOUR_DEPTH
  dc, dd = [-0.1, 0.02, 1e-3, -2e-3, 0.005], [0.05, 0, 0, 0]
  rig = U.rgbd_rig(Kd, dd, Kc, dc, T, (48, 64), (72, 96))
  want_c, want_d = U.undistort_plan(Kc, dc, (72, 96)), U.undistort_plan(Kd, dd, (48, 64))
  assert (rig.K == want_c.K_new).all() and rig.K is not Kc and rig.size == (72, 96) and rig.size_depth == (48, 64)
  for got, want in ((rig.colour_plan, want_c), (rig.depth_plan, want_d)):
    for k in ('k_new', 'rot', 'k_raw', 'dist'):
      assert (getattr(got, k).view(np.uint32) == getattr(want, k).view(np.uint32)).all(), k
    assert got.r2_max == want.r2_max and got.src_size == want.src_size and got.dst_size == want.dst_size
  assert (rig.K_depth == want_d.K_new).all() and (rig.T_colour_depth == T).all() and rig.T_colour_depth is not T
  # a sensor without distortion has no plan, and K is K_colour itself
  for none in ([], None, np.zeros(5)):
    rig = U.rgbd_rig(Kd, none, Kc, none, T, (48, 64), (72, 96))
    assert rig.colour_plan is None and rig.depth_plan is None and (rig.K == Kc).all() and (rig.K_depth == Kd).all()
  rig = U.rgbd_rig(Kd, dd, Kc, [], T, (48, 64), (72, 96))
  assert rig.colour_plan is None and rig.depth_plan is not None


def test_align_frame_and_the_pipeline_stage_with_a_stubbed_kernel_call(monkeypatch):
  from foundationpose_amd.pipeline import AlignDepth, Pipeline, PipelineData
  Kd, Kc = O.K_DEPTH, O.COLOUR[(72, 96)]
  rig = U.rgbd_rig(Kd, [0.05, 0, 0, 0], Kc, [-0.1, 0, 0, 0], O.T_COLOUR_DEPTH, (48, 64), (72, 96))
  calls = []

  def fake_remap_image(img, plan, mode='colour', zfar=np.inf, **kw):
    calls.append(('remap_image', plan, mode, zfar))
    return img + 1

  def fake_reproject_depth(depths, Ks, Ts, K_dst, size_dst, zfar=np.inf, return_source=False, **kw):
    calls.append(('reproject_depth', depths.shape, np.asarray(Ks).copy(), np.asarray(Ts).copy(), np.asarray(K_dst).copy(), size_dst, zfar, return_source))
    out = np.full(depths.shape[:-3] + tuple(size_dst), depths.reshape(-1)[0], F)
    return (out, out.astype(np.int32)) if return_source else out

  monkeypatch.setattr(reproject, 'remap_image', fake_remap_image)
  monkeypatch.setattr(reproject, 'reproject_depth', fake_reproject_depth)
  rgb, depth = np.zeros((72, 96, 3), np.uint8), np.full((48, 64), 2.0, F)
  out_rgb, out_depth = U.align_frame(rgb, depth, rig, zfar=3.0)
  assert (out_rgb == 1).all() and out_depth.shape == (72, 96) and (out_depth == 3.0).all()      # depth went through its plan, then the reprojection
  assert [c[0] for c in calls] == ['remap_image', 'remap_image', 'reproject_depth']
  assert calls[0][1:] == (rig.colour_plan, 'colour', np.inf) and calls[1][1:] == (rig.depth_plan, 'depth', 3.0)
  _, shape, Ks, Ts, K_dst, size_dst, zfar, rs = calls[2]
  assert shape == (1, 48, 64) and (Ks == rig.K_depth[None]).all() and (Ts == O.T_COLOUR_DEPTH[None]).all() and (K_dst == rig.K).all()
  assert size_dst == (72, 96) and zfar == 3.0 and rs is False
  # a batch is n frames of one view; the winner map on request; a missing image stays missing
  del calls[:]
  _, out_depth, source = U.align_frame(None, np.full((5, 48, 64), 2.0, F), rig, return_source=True)
  assert calls[-1][1] == (5, 1, 48, 64) and out_depth.shape == (5, 72, 96) and source.dtype == np.int32 and len(calls) == 2
  del calls[:]
  assert U.align_frame(rgb, None, rig)[1] is None and [c[0] for c in calls] == ['remap_image']
  # without distortion nothing is warped: the colour image is returned as it is
  del calls[:]
  plain = U.rgbd_rig(Kd, [], Kc, [], O.T_COLOUR_DEPTH, (48, 64), (72, 96))
  out_rgb, _ = U.align_frame(rgb, depth, plain)
  assert out_rgb is rgb and [c[0] for c in calls] == ['reproject_depth']
  # the stage
  monkeypatch.setattr(reproject, 'align_frame', lambda rgb, depth, r, zfar=np.inf, **kw: calls.append(('align_frame', r, zfar)) or ('A:' + rgb, 'A:' + depth))
  data = Pipeline('two sensors').add_processor(AlignDepth(rig, zfar=2.5)).run(PipelineData(rgb='rgb', depth='d', K='the depth camera'))
  assert not data.errors and (data.rgb, data.depth) == ('A:rgb', 'A:d') and (data.K == rig.K).all() and data.K is not rig.K
  assert calls[-1] == ('align_frame', rig, 2.5)


def test_gather_by_source():
  import torch
  source = np.array([[0, 5, -1], [23, -1, 12]], np.int32)      # two views of 3 x 4: 12 .. 23 is the second
  labels = np.arange(100, 124, dtype=np.int32).reshape(2, 3, 4)
  assert U.gather_by_source(labels, source, fill=-7).tolist() == [[100, 105, -7], [123, -7, 112]]
  assert U.gather_by_source(labels[0], source.clip(max=11)).tolist() == [[100, 105, 0], [111, 0, 111]]      # (H, W): one view
  colour = np.arange(24 * 3, dtype=np.uint8).reshape(2, 3, 4, 3)
  out = U.gather_by_source(colour, source)
  assert out.shape == (2, 3, 3) and out[0, 1].tolist() == [15, 16, 17] and out[0, 2].tolist() == [0, 0, 0] and out.dtype == np.uint8
  batch = U.gather_by_source(np.stack([labels, labels + 50]), np.stack([source, source[::-1]]), fill=-1)
  assert batch[0].tolist() == [[100, 105, -1], [123, -1, 112]] and batch[1].tolist() == [[173, -1, 162], [150, 155, -1]]
  t = U.gather_by_source(torch.from_numpy(labels), torch.from_numpy(source), fill=-7)
  assert torch.is_tensor(t) and t.tolist() == [[100, 105, -7], [123, -7, 112]]
  assert U.gather_by_source(torch.from_numpy(colour), torch.from_numpy(source)).numpy().tolist() == out.tolist()
  with pytest.raises(ValueError, match='source must be'):
    U.gather_by_source(labels, source[0])
  # with the restatement's winner map: the depth itself comes back
  case = O.bit_cases()['48x64->72x96 V=2']
  got = O.reproject(*case)
  assert (U.gather_by_source(np.nan_to_num(case[0]), got['source']) > 0).sum() == (got['source'] >= 0).sum()


def test_calibration_file_round_trip(tmp_path):
  Kd, Kc, T = O.K_DEPTH + 0.1 / 3, O.COLOUR[(72, 96)] * (1 + 1e-9), O.T_COLOUR_DEPTH
  p = str(tmp_path / 'rgbd.json')
  mesh_io.save_rgbd_calibration(p, Kd, [0.05, -0.01, 1e-4, 2e-4, 1 / 3], Kc, None, T, (48, 64), (72, 96))
  c = mesh_io.load_rgbd_calibration(p)
  assert tuple(c) == mesh_io.RGBD_CALIBRATION_KEYS      # the order of rgbd_rig's arguments
  assert (c['K_depth'] == Kd).all() and (c['K_colour'] == Kc).all() and (c['T_colour_depth'] == T).all()      # float64, bit for bit
  assert c['dist_depth'].tolist() == [0.05, -0.01, 1e-4, 2e-4, 1 / 3] and c['dist_colour'].size == 0
  assert c['size_depth'] == (48, 64) and c['size_colour'] == (72, 96)
  rig = U.rgbd_rig(**c)
  assert rig.colour_plan is None and rig.depth_plan is not None and rig.size == (72, 96)
  # a file written by hand: flat lists are taken, an absent dist_* is no distortion
  import json
  raw = dict(K_depth=Kd.reshape(-1).tolist(), K_colour=Kc.tolist(), T_colour_depth=T.tolist(), size_depth=[48, 64], size_colour=[72, 96])
  (tmp_path / 'hand.json').write_text(json.dumps(raw))
  h = mesh_io.load_rgbd_calibration(str(tmp_path / 'hand.json'))
  assert (h['K_depth'] == Kd).all() and h['dist_depth'].size == 0 and h['dist_colour'].size == 0
  for broken, match in ((dict(raw, K_depth=[1, 2, 3]), '3x3'), (dict(raw, T_colour_depth=np.eye(3).tolist()), '4x4'), (dict(raw, size_depth=[48]), r'\[H, W\]'),
                        (dict(raw, size_colour=[72.5, 96]), r'\[H, W\]'), (dict(raw, K_color=Kc.tolist()), 'unknown key'),
                        ({k: v for k, v in raw.items() if k != 'T_colour_depth'}, 'missing')):
    (tmp_path / 'broken.json').write_text(json.dumps(broken))
    with pytest.raises(ValueError, match=match):
      mesh_io.load_rgbd_calibration(str(tmp_path / 'broken.json'))
  (tmp_path / 'list.json').write_text('[1, 2]')
  with pytest.raises(ValueError, match='JSON object'):
    mesh_io.load_rgbd_calibration(str(tmp_path / 'list.json'))
