"""CPU: depth from a rectified stereo pair - the numpy restatement of the rule (tests/stereo_oracle.py) pinned on a random-dot
stereogram and against hand-written and scalar-loop values, the calibration-file readers, and the refusals of fp_stereo_sgm that need
no GPU."""
import ctypes

import numpy as np
import pytest

from tests import stereo_oracle as O


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_stereogram(seed):
  """(H,W,D) = (40,176,64), background disparity 6, a foreground rectangle at 41.  Over the pixels that are neither occluded nor in
  x < D the integer winner is the true disparity on at least 0.99 of them (measured: 0.9989, 0.9993, 0.9984), and at least 0.90 of the
  occluded background pixels are declared invalid (measured: 0.971, 0.984, 0.956): the two conditions the GPU test asserts as well."""
  left, right, truth, occ = O.stereogram(seed)
  assert left.shape == (40, 176) and occ.sum() == 20 * 35
  out = O.sgm(left, right, max_disparity=64)
  keep = ~occ & (np.arange(176)[None, :] >= 64)
  exact = float((out['dstar'][keep] == truth[keep]).mean())
  refused = float((~out['valid'][occ]).mean())
  print(f'seed {seed}: exact {exact:.4f}, occluded refused {refused:.3f}')
  assert exact >= 0.99
  assert refused >= 0.90
  assert (out['disparity'][~out['valid']] == -1).all() and (np.abs(out['disparity'][out['valid']] - out['dstar'][out['valid']]) <= 0.5).all()


def test_census_by_hand():
  bit = lambda dy, dx: 61 - ((dy + 3) * 9 + (dx + 4) - ((dy, dx) > (0, 0)))      # row-major without the centre, the first neighbour in bit 61
  g = np.full((7, 9), 10, np.uint8)
  g[1, 2] = 200      # one bright pixel: every neighbour is smaller there, it is smaller than nothing
  want = np.zeros((7, 9), np.uint64)
  want[1, 2] = (1 << 62) - 1
  assert (O.census(g) == want).all()
  g = np.full((7, 9), 100, np.uint8)
  g[3, 4] = 0        # one dark pixel in the middle: one bit in every other code
  c = O.census(g)
  assert c[3, 4] == 0
  assert c[3, 3] == 1 << 30 and c[0, 0] == 1 << 0 and c[6, 8] == 1 << 61 and c[2, 4] == 1 << 22 and c[3, 5] == 1 << 31
  assert all(c[y, x] == 1 << bit(3 - y, 4 - x) for y in range(7) for x in range(9) if (y, x) != (3, 4))
  g = np.full((7, 9), 100, np.uint8)
  g[0, 0] = 0        # a dark corner: clamped coordinates see it again and again
  c = O.census(g)
  assert c[1, 1] == sum(1 << bit(dy, dx) for dy in (-3, -2, -1) for dx in (-4, -3, -2, -1))
  assert c[0, 4] == sum(1 << bit(dy, -4) for dy in (-3, -2, -1, 0))      # rows above the image are row 0
  assert c[0, 5] == 0 and c[4, 0] == 0 and c[3, 0] == sum(1 << bit(-3, dx) for dx in (-4, -3, -2, -1, 0))


def scalar_path(C, r, P1, P2):
  """The recurrence pixel by pixel and disparity by disparity, as the header writes it."""
  dy, dx = O.DIRS[r]
  H, W, D = C.shape
  L = np.zeros((H, W, D), np.int64)
  ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
  xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
  for y in ys:
    for x in xs:
      qy, qx = y - dy, x - dx
      if not (0 <= qy < H and 0 <= qx < W):
        L[y, x] = C[y, x]
        continue
      m = min(int(v) for v in L[qy, qx])
      for d in range(D):
        best = min(int(L[qy, qx, d]), m + P2)
        if d - 1 >= 0:
          best = min(best, int(L[qy, qx, d - 1]) + P1)
        if d + 1 < D:
          best = min(best, int(L[qy, qx, d + 1]) + P1)
        L[y, x, d] = int(C[y, x, d]) + best - m
  return L


@pytest.mark.parametrize('r', range(8))
def test_each_path_against_scalar_loops(r):
  rng = np.random.default_rng(5)
  left, right = (rng.integers(0, 256, (6, 10)).astype(np.uint8) for _ in range(2))
  C = O.cost(O.census(left), O.census(right), 64)
  assert C.shape == (6, 10, 64) and (C[:, 3, 4:] == 64).all() and (C[:, 3, :4] < 64).any()
  for P1, P2 in ((8, 32), (0, 0), (5, 100)):
    L = O.path(C, r, P1, P2)
    assert (L == scalar_path(C, r, P1, P2)).all(), (r, P1, P2)
    assert L.max() <= 64 + P2


def test_winners_and_subpixel_by_hand():
  S = np.full((1, 3, 64), 500, np.uint16)
  S[0, 2, 1], S[0, 2, 2], S[0, 2, 3] = 100, 60, 80      # left pixel 2: d* = 2, parabola (100 - 80) / (2 (100 - 120 + 80)) = 1/6
  S[0, 1, 0], S[0, 0, 0] = 70, 500
  ds, dr = O.winners(S)
  assert ds[0].tolist() == [0, 0, 2] and dr[0].tolist() == [2, 0, 0]      # d_R(0) = argmin(S(0,0), S(1,1), S(2,2)) = 2
  assert np.float32(2) + np.float32(20) / np.float32(120) == np.float32(2.1666667)


def test_grey():
  rgb = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]]], np.uint8)
  assert O.grey(rgb).tolist() == [[255, 0, 77, 149, 29, (770 + 3000 + 870 + 128) >> 8]]


SECTIONED = """
[LEFT_CAM_2K]
fx=1900.5
fy=1901.25
cx=1100
cy=620

[LEFT_CAM_FHD1200]
fx=1067.51
fy=1067.9
cx=960.5
cy=600.25
k1=-0.0512
p1=1.2e-05

[RIGHT_CAM_FHD1200]
fx=1066.1
fy=1066.3
cx=970.5
cy=590.75

[STEREO]
Baseline=119.905
TY=-0.0127
"""


def test_calibration_files(tmp_path):
  from foundationpose_amd import mesh_io
  p = tmp_path / 'camera.conf'
  p.write_text(SECTIONED)
  assert mesh_io.load_intrinsics(str(p)).tolist() == [[1067.51, 0, 960.5], [0, 1067.9, 600.25], [0, 0, 1]]
  assert mesh_io.load_intrinsics(str(p), camera_section='LEFT_CAM_2K').tolist() == [[1900.5, 0, 1100], [0, 1901.25, 620], [0, 0, 1]]
  assert mesh_io.load_intrinsics(str(p), 'RIGHT_CAM_FHD1200')[0, 2] == 970.5
  assert mesh_io.load_stereo_baseline(str(p)) == pytest.approx(0.119905, rel=1e-15)
  assert mesh_io.load_stereo_baseline(str(p), scale=1.0) == 119.905
  with pytest.raises(ValueError, match='LEFT_CAM_VGA'):
    mesh_io.load_intrinsics(str(p), 'LEFT_CAM_VGA')
  (tmp_path / 'nofx.conf').write_text('[LEFT_CAM_FHD1200]\nfy=1\ncx=2\ncy=3\n[STEREO]\nTY=0\n')
  with pytest.raises(ValueError, match='fx='):
    mesh_io.load_intrinsics(str(tmp_path / 'nofx.conf'))
  with pytest.raises(ValueError, match='Baseline='):
    mesh_io.load_stereo_baseline(str(tmp_path / 'nofx.conf'))
  # the nine-number file is read exactly as before
  q = tmp_path / 'cam_K.txt'
  q.write_text('500.5 0 320\n0, 501.5, 240\n0 0 1\n')
  assert mesh_io.load_intrinsics(str(q)).tolist() == [[500.5, 0, 320], [0, 501.5, 240], [0, 0, 1]]
  with pytest.raises(ValueError, match='sectioned'):
    mesh_io.load_stereo_baseline(str(q))
  (tmp_path / 'eight.txt').write_text('1 2 3 4 5 6 7 8')
  with pytest.raises(ValueError, match='expected 9'):
    mesh_io.load_intrinsics(str(tmp_path / 'eight.txt'))


@pytest.fixture(scope='module')
def built():
  import __graft_entry__ as g
  g.build()
  from foundationpose_amd import _lib
  return _lib


def test_argument_checks_need_no_gpu(built):
  L = built.lib()
  fake = ctypes.c_void_p(64)      # never dereferenced: every check of a value comes first

  def call(ctx=fake, left=fake, right=fake, n=1, H=6, W=8, channels=1, opts=True, disparity=fake, depth=fake, dbg=None, opts_size=None, dbg_size=None,
           **kw):
    o = built.FpStereoOpts(struct_size=ctypes.sizeof(built.FpStereoOpts), max_disparity=64, p1=8, p2=32, paths=0xFF, lr_max=1, min_disparity=1,
                           subpixel=1, fx=500.0, baseline=0.1, zfar=float('inf'))
    for k, v in kw.items():
      setattr(o, k, v)
    if opts_size is not None:
      o.struct_size = opts_size
    d = None
    if dbg_size is not None:
      d = ctypes.byref(built.FpStereoDebug(struct_size=dbg_size))
    return L.fp_stereo_sgm(ctx, left, right, n, H, W, channels, ctypes.byref(o) if opts else None, disparity, depth, d, None)

  bad = [dict(ctx=None), dict(left=None), dict(right=None), dict(opts=False), dict(opts_size=0), dict(opts_size=ctypes.sizeof(built.FpStereoOpts) - 8),
         dict(dbg_size=8), dict(n=0), dict(H=0), dict(W=0), dict(n=70000), dict(channels=2), dict(channels=4), dict(max_disparity=0),
         dict(max_disparity=96), dict(max_disparity=320), dict(max_disparity=-64), dict(H=1 << 14, W=1 << 14), dict(p1=33), dict(p1=-1),
         dict(p2=8128), dict(p1=9000, p2=9000), dict(paths=0), dict(paths=0x100), dict(min_disparity=-1), dict(min_disparity=64), dict(subpixel=2),
         dict(fx=0.0), dict(baseline=-0.1), dict(fx=float('nan')), dict(fx=1e30, baseline=1e30), dict(zfar=0.0), dict(zfar=float('nan'))]
  for kw in bad:
    assert call(**kw) == built.FP_EINVAL, kw
    assert L.fp_last_error()
  assert call(p1=33) == built.FP_EINVAL and b'p1 33' in L.fp_last_error()
  assert call(p2=8128) == built.FP_EINVAL and b'16 bits' in L.fp_last_error()


def test_stereo_depth_processor_without_a_pair():
  from foundationpose_amd.pipeline import PipelineData, StereoDepth
  assert PipelineData().right is None
  proc = StereoDepth(0.12, K=np.eye(3))
  data = PipelineData(rgb='left', right='right', depth='as it was')
  assert proc.process(data) is data and data.depth == 'as it was'      # a depth that is there is left alone
  with pytest.raises(ValueError, match='pair'):
    proc.process(PipelineData(rgb=np.zeros((4, 4), np.uint8)))
  with pytest.raises(ValueError, match='camera matrix'):
    StereoDepth(0.12).process(PipelineData(rgb=np.zeros((4, 4), np.uint8), right=np.zeros((4, 4), np.uint8)))
