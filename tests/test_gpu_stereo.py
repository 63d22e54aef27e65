"""GPU: depth from a rectified stereo pair (fp_stereo_sgm, csrc/stereo.hip) against tests/stereo_oracle.py.  Every stage the debug
structure exposes - both census images, C, S, d*, d_R - and disparity and depth are compared BIT FOR BIT: the arithmetic is integer up to
the winner, and the two float32 steps are single correctly rounded operations.  The shapes are the smallest that reach every path of the
kernels: one, two, three and four disparities a lane (D = 64, 128, 192, 256), widths that are no multiple of 64, W < D, H below the
census window, one pixel, each direction alone (a wrong diagonal start or direction shows only there)."""
import numpy as np
import pytest
import torch

from tests import stereo_oracle as O

pytestmark = pytest.mark.gpu

FX, BASELINE = 500.25, 0.12
STAGES = (('census_left', 'census_l'), ('census_right', 'census_r'), ('cost', 'cost'), ('sum', 'sum'), ('dstar', 'dstar'), ('dright', 'dright'))


def noise(shape, seed):
  return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def gpu(left, right, D, **kw):
  """One call with every output: dict of numpy arrays (leading n) - the stages, disparity, depth."""
  from foundationpose_amd import stereo
  disparity, depth, stages = stereo.sgm(left, right, max_disparity=D, fx=FX, baseline=BASELINE, return_debug=True, **kw)
  out = stereo._debug_numpy(stages)
  out['disparity'], out['depth'] = disparity.cpu().numpy(), depth.cpu().numpy()
  return out


def assert_equal_to_oracle(got, ref, v=0, what=''):
  for g, r in STAGES + (('disparity', 'disparity'), ('depth', 'depth')):
    a, b = got[g][v], ref[r]
    assert a.dtype == b.dtype and a.shape == b.shape, (what, g, a.dtype, b.dtype, a.shape, b.shape)
    bad = a.view(np.uint8 if a.dtype.itemsize == 1 else f'u{a.dtype.itemsize}') != b.view(np.uint8 if b.dtype.itemsize == 1 else f'u{b.dtype.itemsize}')
    assert not bad.any(), f'{what}: {g} differs in {int(bad.sum())} of {bad.size} entries, first at {tuple(np.argwhere(bad)[0])}'


def check_pair(left, right, D, what='', **kw):
  got = gpu(left, right, D, **kw)
  ref = O.sgm(left, right, max_disparity=D, fx=FX, baseline=BASELINE, **kw)
  assert_equal_to_oracle(got, ref, 0, what)
  return got, ref


@pytest.fixture(scope='module')
def grams():
  """The stereograms of tests/test_stereo_host.py and their oracle stages, computed once and never written to."""
  out = {}
  for seed in (0, 1, 2):
    left, right, truth, occ = O.stereogram(seed)
    out[seed] = dict(left=left, right=right, truth=truth, occ=occ, ref=O.sgm(left, right, max_disparity=64, fx=FX, baseline=BASELINE))
  return out


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_stereogram_all_paths(grams, seed):
  g = grams[seed]
  got = gpu(g['left'], g['right'], 64)
  assert_equal_to_oracle(got, g['ref'], 0, f'stereogram {seed}')
  H, W = g['truth'].shape
  keep = ~g['occ'] & (np.arange(W)[None, :] >= 64)
  exact = float((got['dstar'][0][keep] == g['truth'][keep]).mean())
  refused = float((got['disparity'][0][g['occ']] < 0).mean())
  print(f'stereogram seed {seed}: d* exact on {exact:.4f} of the unoccluded pixels with x >= D; {refused:.3f} of the occluded ones invalid')
  assert exact >= 0.99
  assert refused >= 0.90


@pytest.mark.parametrize('bit', range(8))
def test_each_direction_alone_on_noise(bit):
  check_pair(noise((13, 70), 10 + bit), noise((13, 70), 30 + bit), 64, f'direction {bit}', paths=1 << bit)


@pytest.mark.parametrize('shape', [(9, 150, 128), (5, 100, 192), (7, 300, 256), (5, 40, 64), (1, 1, 64)])
def test_shapes(shape):
  H, W, D = shape
  tex = noise((H, W + 5), 50 + D)
  got, ref = check_pair(np.ascontiguousarray(tex[:, :W]), np.ascontiguousarray(tex[:, 5:]), D, str(shape))      # left(x) = right(x - 5)
  if shape == (1, 1, 64):
    assert got['disparity'][0, 0, 0] == -1 and got['depth'][0, 0, 0] == 0
  if shape == (9, 150, 128):
    assert (ref['disparity'] > 0).mean() > 0.5      # the case is not trivially all invalid


@pytest.mark.parametrize('kw', [dict(subpixel=False), dict(lr_max=-1), dict(paths=0x0F), dict(p1=3, p2=70, min_disparity=0, lr_max=0)],
                         ids=['no_subpixel', 'no_lr_check', 'four_paths', 'other_penalties'])
def test_option_switches(grams, kw):
  g = grams[0]
  got, ref = check_pair(g['left'], g['right'], 64, str(kw), **kw)
  assert any((ref[k] != g['ref'][k]).any() for k in ('sum', 'disparity'))      # the switch does something on this input


def test_depth_is_fb_over_integer_disparity_and_zfar(grams):
  g = grams[0]
  got = gpu(g['left'], g['right'], 64, subpixel=False)
  valid = got['disparity'][0] >= 0
  assert valid.mean() > 0.5
  want = np.float32(FX * BASELINE) / got['dstar'][0][valid].astype(np.float32)
  assert (got['depth'][0][valid].view(np.uint32) == want.astype(np.float32).view(np.uint32)).all()
  assert (got['depth'][0][~valid] == 0).all()
  zfar = 5.0      # the background (d = 6) is at 10 m, the foreground (d = 41) at 1.46 m
  near, ref = check_pair(g['left'], g['right'], 64, 'zfar', zfar=zfar)
  assert (near['depth'] <= zfar).all() and (near['depth'] > 0).any() and ((near['depth'] == 0) & (near['disparity'] > 0)).any()


def test_rgb_pair_equals_its_grey_conversion():
  left, right = noise((13, 70, 3), 70), noise((13, 70, 3), 71)
  left[0, :5] = [[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]]      # the extremes of the weighted sum
  got, ref = check_pair(left, right, 64, 'rgb')
  grey = gpu(ref['grey_l'], ref['grey_r'], 64)
  for k in got:
    assert (got[k] == grey[k]).all(), k


def test_batch_equals_single_calls(grams):
  left = np.stack([grams[s]['left'] for s in (0, 1, 2)])
  right = np.stack([grams[s]['right'] for s in (0, 1, 2)])
  got = gpu(left, right, 64)
  for v, s in enumerate((0, 1, 2)):
    assert_equal_to_oracle(got, grams[s]['ref'], v, f'batch entry {v}')
    one = gpu(left[v], right[v], 64)
    for k in got:
      assert (got[k][v] == one[k][0]).all(), (k, v)


def test_repeatable_and_no_stale_state(grams):
  """The same call twice gives the same bits, and a smaller call in between (whose arrays lie elsewhere in the same allocation) does not
  change what the larger one gives afterwards."""
  g = grams[1]
  first = gpu(g['left'], g['right'], 64)
  again = gpu(g['left'], g['right'], 64)
  check_pair(noise((13, 70), 90), noise((13, 70), 91), 64, 'small call in between')
  third = gpu(g['left'], g['right'], 64)
  for k in first:
    assert (first[k] == again[k]).all() and (first[k] == third[k]).all(), k
  assert_equal_to_oracle(third, g['ref'], 0, 'after the smaller call')


def test_captured_graph_equals_eager(grams):
  from foundationpose_amd import stereo
  g = grams[2]
  left, right = torch.as_tensor(g['left']).cuda(), torch.as_tensor(g['right']).cuda()
  call = lambda: stereo.sgm(left, right, max_disparity=64, fx=FX, baseline=BASELINE)[:2]
  eager = [t.clone() for t in call()]      # also the warm-up: the working memory is allocated outside the capture
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = call()
  for t in out:
    t.zero_()
  graph.replay()
  torch.cuda.synchronize()
  for a, b, name in zip(out, eager, ('disparity', 'depth')):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
  assert (eager[0].cpu().numpy().view(np.uint32) == g['ref']['disparity'].view(np.uint32)).all()


def test_stereo_depth_processor_feeds_the_depth_prelude(grams):
  from foundationpose_amd import Utils as U
  from foundationpose_amd.pipeline import PipelineData, StereoDepth
  g = grams[0]
  K = np.array([[FX, 0, 88.0], [0, FX, 20.0], [0, 0, 1]])
  left, right = torch.as_tensor(g['left']).cuda(), torch.as_tensor(g['right']).cuda()
  data = StereoDepth(BASELINE, K=K, max_disparity=64).process(PipelineData(rgb=left, right=right))
  assert torch.is_tensor(data.depth) and data.depth.is_cuda and data.depth.dtype == torch.float32 and tuple(data.depth.shape) == (40, 176)
  assert (data.depth.cpu().numpy().view(np.uint32) == g['ref']['depth'].view(np.uint32)).all()
  depth, xyz = U.depth_prefilter(data.depth, K)
  assert depth.is_cuda and tuple(xyz.shape) == (40, 176, 3) and bool(torch.isfinite(depth).all()) and float(depth.max()) > 0
  # numpy in, numpy out; a depth that is already there is left alone
  d_np = U.stereo_depth(g['left'], g['right'], K, BASELINE, max_disparity=64)
  assert isinstance(d_np, np.ndarray) and (d_np.view(np.uint32) == g['ref']['depth'].view(np.uint32)).all()
  kept = StereoDepth(BASELINE, K=K).process(PipelineData(rgb=left, right=right, depth='as it was'))
  assert kept.depth == 'as it was'
