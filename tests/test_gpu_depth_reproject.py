"""GPU: fp_depth_reproject (csrc/reproject.hip) against its numpy restatement tests/depth_reproject_oracle.py, bit for bit, and against
checks that need no restatement.  tests/test_depth_reproject_host.py pins the restatement itself.  Every case is a few thousand pixels:
narrower than a wave, no multiple of a block, several blocks, magnified and reduced."""
import numpy as np
import pytest
import torch

from tests import depth_reproject_oracle as O

pytestmark = pytest.mark.gpu
F = np.float32


def assert_same_bits(got, want, what):
  assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
  view = f'u{got.dtype.itemsize}'
  bad = np.ascontiguousarray(got).view(view) != np.ascontiguousarray(want).view(view)
  assert not bad.any(), f'{what}: differs in {int(bad.sum())} of {bad.size} entries, first at {tuple(np.argwhere(bad)[0])}'


@pytest.fixture(scope='module')
def cases():
  """The cases of the bit-equality test and their restatement, computed once and never written to."""
  return {k: (c, O.reproject(*c)) for k, c in O.bit_cases().items()}


@pytest.mark.parametrize('name', list(O.bit_cases()))
def test_depth_and_source_equal_the_restatement(cases, name):
  from foundationpose_amd import Utils as U
  c, want = cases[name]
  depth, source = U.reproject_depth(*c[:5], zfar=c[5], return_source=True)
  assert_same_bits(depth, want['depth'], 'depth')
  assert_same_bits(source, want['source'], 'source')
  assert (want['source'] >= 0).mean() > 0.5 and np.isnan(c[0]).sum() >= 6 and 0.05 < (c[0] == 0).mean() < 0.15
  if name == '64x200->30x94':      # reduced: most target pixels take several atomics
    assert (np.isfinite(c[0]) & (c[0] > 0)).sum() > 4 * (want['source'] >= 0).sum()
  assert_same_bits(U.reproject_depth(*c[:5], zfar=c[5]), want['depth'], 'depth alone')


def test_same_bits_on_a_second_run_and_inside_a_batch(cases):
  from foundationpose_amd import Utils as U
  c, want = cases['batch n=2']
  d = torch.as_tensor(c[0]).cuda()
  first = U.reproject_depth(d, *c[1:5], return_source=True)
  second = U.reproject_depth(d, *c[1:5], return_source=True)
  assert first[0].is_cuda and first[1].dtype == torch.int32
  for a, b in zip(first, second):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
  assert not np.array_equal(want['depth'][0], want['depth'][1])      # the second frame differs
  for i in range(2):
    alone = U.reproject_depth(d[i], *c[1:5], return_source=True)
    assert torch.equal(alone[0].view(torch.int32), first[0][i].view(torch.int32)) and torch.equal(alone[1], first[1][i])
    assert_same_bits(alone[0].cpu().numpy(), want['depth'][i], f'frame {i}')


def test_identity():
  """Same K, T = 1, same size: every depth lands on its own pixel bit for bit, 0 where it is no depth; the winner is the pixel's index."""
  from foundationpose_amd import Utils as U
  d = O.random_depth((1, 37, 53), 3, zfar=1.6)
  depth, source = U.reproject_depth(d, [O.K_SMALL], [np.eye(4)], O.K_SMALL, (37, 53), zfar=1.6, return_source=True)
  ok = O.depth_ok(d[0], 1.6)
  assert_same_bits(depth, np.where(ok, d[0], F(0)), 'depth')
  assert_same_bits(source, np.where(ok, np.arange(37 * 53).reshape(37, 53), -1).astype(np.int32), 'source')


@pytest.mark.parametrize('scale', O.PLANE_SCALES)
def test_translated_plane_is_one_value_without_holes(scale):
  """No restatement: a plane d = 0.8, a pure translation (0.025, -0.004, 0.003).  Every filled target pixel is float32(0.8) +
  float32(0.003) bit for bit, and no target pixel whose ray meets the source image at least one pixel inside its border is empty - the
  test of the footprint rule, at reductions and magnifications."""
  from foundationpose_amd import Utils as U
  c = O.plane_case(scale)
  depth = U.reproject_depth(*c[:5])
  wrong, holes, must_fill = O.plane_check(depth, scale)
  assert must_fill > 400 * scale * scale and wrong == 0 and holes == 0


def test_occlusion_and_ties():
  from foundationpose_amd import Utils as U
  c = O.occlusion_case()
  depth = U.reproject_depth(*c[:5])
  contested, lost = O.occlusion_check(depth)
  assert contested >= 16 and lost == 0      # where a near and a far pixel land together the near one shows
  assert set(np.unique(depth)) == {0.0, float(F(0.6)), float(F(1.1))}
  # a 4 x reduction of a constant plane: equal depths everywhere, the lowest index among the 16 contributors wins
  K = np.array([[40.0, 0, 7.5], [0, 40.0, 5.5], [0, 0, 1]])
  Kq = np.array([[10.0, 0, 1.5], [0, 10.0, 1.0], [0, 0, 1]])
  depth, source = U.reproject_depth(np.full((1, 12, 16), 0.9, F), [K], [np.eye(4)], Kq, (3, 4), return_source=True)
  rows = np.floor((np.arange(12) - 5.5) / 4 + 1.0 + 0.5).astype(int)
  cols = np.floor((np.arange(16) - 7.5) / 4 + 1.5 + 0.5).astype(int)
  want = np.array([[min(r * 16 + c for r in range(12) for c in range(16) if rows[r] == y and cols[c] == x) for x in range(4)] for y in range(3)])
  assert (source == want).all() and (depth == F(0.9)).all()
  # two views of equal depth: the first wins; the second nearer: it wins
  two = np.stack([np.full((12, 16), 0.9, F), np.full((12, 16), 0.9, F)])
  assert (U.reproject_depth(two, [K, K], [np.eye(4)] * 2, K, (12, 16), return_source=True)[1] == np.arange(192).reshape(12, 16)).all()
  two[1] = 0.7
  assert (U.reproject_depth(two, [K, K], [np.eye(4)] * 2, K, (12, 16), return_source=True)[1] == 192 + np.arange(192).reshape(12, 16)).all()


def test_the_cap_and_the_guards():
  """A plane at a grazing angle, the target camera close to it: rows that stretch over more than 8 target pixels take the cap, and some
  footprint corners fall behind the target camera.  Both branches are taken (counted in the restatement) and the bits are equal."""
  from foundationpose_amd import Utils as U
  c = O.grazing_case()
  want = O.reproject(*c)
  assert want['capped'] > 100 and want['behind'] > 10
  depth, source = U.reproject_depth(*c[:5], return_source=True)
  assert_same_bits(depth, want['depth'], 'depth')
  assert_same_bits(source, want['source'], 'source')
  # huge and non-finite projections never reach a cast: depths next to the largest float, a camera that sees them at infinity
  d = np.full((1, 8, 8), 3e38, F)
  d[0, 0, 0] = np.inf
  out = U.reproject_depth(d, [np.array([[1e-3, 0, 4], [0, 1e-3, 4], [0, 0, 1]])], [np.eye(4)], np.array([[1e30, 0, 4], [0, 1e30, 4], [0, 0, 1]]), (8, 8))
  assert_same_bits(out, O.reproject(d, [np.array([[1e-3, 0, 4], [0, 1e-3, 4], [0, 0, 1]])], [np.eye(4)], np.array([[1e30, 0, 4], [0, 1e30, 4], [0, 0, 1]]),
                                    (8, 8))['depth'], 'huge')


@pytest.mark.parametrize('size', list(O.COLOUR), ids=['72x96', '30x40'])
def test_align_frame_end_to_end(size):
  """A sphere of radius 0.12 m at 0.7 m in front of a plane at 1.2 m, a 48 x 64 depth camera, the colour camera 5 cm to the side and
  turned by 1.9 degrees, at 72 x 96 and at 30 x 40.  align_frame's depth equals the restatement bit for bit, so the figures are those
  measured on the CPU (tests/test_depth_reproject_host.py), 72 x 96 / 30 x 40 over the filled pixels: median |aligned - analytic| 0.176 /
  0.253 mm, share beyond 2 cm (the occlusion rim) 0.41 / 0.93 %, filled 0.950 / 0.991.  Asserted at twice the figures: median <= 0.352 /
  0.505 mm, beyond 2 cm <= 0.82 / 1.85 %; filled >= 0.93.  The sphere's mask read from the UNALIGNED depth shows the plane instead of the
  sphere (an error above the 0.38 m between them) on 24.6 / 27.4 % of the mask's half towards the depth camera; aligned, on at most 1 %.
  Asserted: >= 13 % unaligned (half of the geometric estimate, see the host test), <= 2 % aligned."""
  from foundationpose_amd import Utils as U
  from foundationpose_amd.pipeline import AlignDepth, PipelineData
  bounds = {(72, 96): (0.352e-3, 0.0082), (30, 40): (0.505e-3, 0.0185)}[size]
  want = O.end_to_end(size)
  rig = U.rgbd_rig(O.K_DEPTH, [], O.COLOUR[size], None, O.T_COLOUR_DEPTH, O.SIZE_DEPTH, size)
  rgb = np.zeros(size + (3,), np.uint8)
  out_rgb, depth, source = U.align_frame(rgb, want['raw'], rig, return_source=True)
  assert out_rgb is rgb
  assert_same_bits(depth, want['aligned'], 'aligned depth')
  e = O.end_to_end(size, aligned=depth)
  print(size, {k: np.round(v, 5) for k, v in e.items() if k not in ('raw', 'aligned')})
  assert e['median'] <= bounds[0] and e['beyond'] <= bounds[1] and e['filled'] >= 0.93
  assert max(e['naive_wrong']) >= 0.13 and max(e['aligned_wrong']) <= 0.02 and e['naive_wrong'][0] > 5 * e['naive_wrong'][1]
  # the winner map carries the depth image itself onto the colour grid: the same pixels, and depths that differ by the change of axis
  # alone (at most sin(1.9 deg) x 0.77 m off the axis + 3 mm of translation = 0.029 m); the stage gives the same frame on the device
  carried = U.gather_by_source(want['raw'], source)
  assert ((carried > 0) == (depth > 0)).all() and np.abs(carried - depth).max() < 0.03
  data = AlignDepth(rig).process(PipelineData(rgb=torch.as_tensor(rgb).cuda(), depth=torch.as_tensor(want['raw']).cuda()))
  assert data.depth.is_cuda and (data.K == rig.K).all()
  assert_same_bits(data.depth.cpu().numpy(), want['aligned'], 'pipeline depth')


def test_captured_graph_equals_eager():
  """align_frame of a rig with lens distortion on both sensors - two undistortion launches, then the memset and the two launches of the
  reprojection - captured once and replayed twice on new inputs."""
  from foundationpose_amd import Utils as U
  rig = U.rgbd_rig(O.K_DEPTH, [0.05, -0.01, 1e-3, 0, 0], O.COLOUR[(72, 96)], [-0.1, 0.02, 0, 1e-3, 0], O.T_COLOUR_DEPTH, O.SIZE_DEPTH, (72, 96))
  rng = np.random.default_rng(5)
  frames = [(rng.integers(0, 256, (72, 96, 3)).astype(np.uint8), O.random_depth(O.SIZE_DEPTH, 30 + i)) for i in range(3)]
  rgb, depth = torch.as_tensor(frames[0][0]).cuda(), torch.as_tensor(frames[0][1]).cuda()
  eager = []
  for r, d in frames:      # also the warm-up
    rgb.copy_(torch.as_tensor(r)), depth.copy_(torch.as_tensor(d))
    eager.append([t.clone() for t in U.align_frame(rgb, depth, rig, zfar=1.6, return_source=True)])
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = U.align_frame(rgb, depth, rig, zfar=1.6, return_source=True)
  for i in (1, 2):
    rgb.copy_(torch.as_tensor(frames[i][0])), depth.copy_(torch.as_tensor(frames[i][1]))
    for t in out:
      t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[i][0]) and torch.equal(out[1].view(torch.int32), eager[i][1].view(torch.int32)) and torch.equal(out[2], eager[i][2])
    assert (out[1] > 0).float().mean() > 0.5
  assert not torch.equal(eager[1][1], eager[2][1])


def test_command_line_tool_aligns_with_a_calibration_file(tmp_path):
  """scripts/align_depth.py RGB DEPTH --calibration FILE --out DIR: image files and this project's calibration file in, the aligned frame
  and its camera matrix out - the same bits as align_frame gives in the process of the test."""
  import os
  import subprocess
  import sys
  from PIL import Image
  from foundationpose_amd import mesh_io
  size = (72, 96)
  want = O.end_to_end(size)
  rgb = np.random.default_rng(7).integers(0, 256, size + (3,)).astype(np.uint8)
  Image.fromarray(rgb).save(tmp_path / 'rgb.png')
  np.save(tmp_path / 'depth.npy', want['raw'])
  mesh_io.save_rgbd_calibration(str(tmp_path / 'rgbd.json'), O.K_DEPTH, [], O.COLOUR[size], [], O.T_COLOUR_DEPTH, O.SIZE_DEPTH, size)
  repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  out = tmp_path / 'aligned'
  p = subprocess.run([sys.executable, os.path.join(repo, 'scripts', 'align_depth.py'), str(tmp_path / 'rgb.png'), str(tmp_path / 'depth.npy'),
                      '--calibration', str(tmp_path / 'rgbd.json'), '--out', str(out), '--source'], capture_output=True, text=True, timeout=120)
  assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
  assert_same_bits(np.load(out / 'depth.npy'), want['aligned'], 'depth.npy')
  assert (np.asarray(Image.open(out / 'rgb.png')) == rgb).all() and (np.loadtxt(out / 'cam_K.txt') == O.COLOUR[size]).all()
  source = np.load(out / 'source.npy')
  assert source.dtype == np.int32 and ((source >= 0) == (want['aligned'] > 0)).all()
