"""The depth prelude (csrc/crop.hip: erode_depth, bilateral_filter_depth, depth2xyzmap_batch and the fused depth_prefilter) at its thresholds and
the radix-select medians (mask_depth_stats in crop.hip, mask_depth_stats_objects in register.hip) on crafted values, against the oracle's float32
CPU code and numpy.  The inputs and the CPU checks that they sit on the boundaries they name are in tests/test_depth_edges_host.py.

erode_depth, depth2xyzmap_batch, the medians and the six integer statistics: exact.  bilateral_filter_depth: atol 2e-6, the allowance of
tests/test_gpu_kernels.py::test_depth_filters for expf against np.exp on weights that sum to O(1) - every gate-boundary case is built so that a
neighbour wrongly taken in or left out moves the result by more than 1e-4 (asserted on the CPU), fifty times the allowance."""
import ctypes

import numpy as np
import pytest
import torch

from tests import test_depth_edges_host as D

pytestmark = pytest.mark.gpu
f32 = np.float32
ATOL_EXPF = 2e-6
K = np.array([[61.7, 0, 17.4], [0, 60.3, 5.2], [0, 0, 1.0]])


@pytest.fixture(scope='module')
def U():
  from foundationpose_amd import Utils
  return Utils


def _xyz_oracle(depth, zfar):
  from oracle import geometry as G
  return G.depth2xyzmap_batch(torch.from_numpy(depth)[None], torch.as_tensor(K, dtype=torch.float32)[None], zfar=zfar)[0].numpy()


@pytest.mark.parametrize('name,d,kw', list(D.erode_cases()), ids=lambda v: v if isinstance(v, str) else '')
def test_erode_at_the_ratio_diff_and_zfar_boundaries(U, name, d, kw):
  from oracle import geometry as G
  for ratio in (0.8, 0.0, 1.0):
    np.testing.assert_array_equal(U.erode_depth(d, radius=2, ratio_thres=ratio, **kw), G.erode_depth(d, radius=2, ratio_thres=ratio, **kw), err_msg=f'{name} {ratio}')


@pytest.mark.parametrize('hw', [(9, 11), (13, 37)])
def test_bilateral_gate_zfar_and_empty_windows(U, hw):
  from oracle import geometry as G
  images = dict(on_gate=(D.gate_image(hw, D.M + D.E), 100.0), inside_gate=(D.gate_image(hw, np.nextafter(D.M + D.E, f32(0))), 100.0),
                at_zfar=(D.zfar_bilateral_image(hw), 2.0), split=(D.split_window_image(hw), 100.0), empty=(np.zeros(hw, np.float32), 100.0))
  for name, (d, zfar) in images.items():
    got, want = U.bilateral_filter_depth(d, radius=2, zfar=zfar), G.bilateral_filter_depth(d, radius=2, zfar=zfar)
    np.testing.assert_allclose(got, want, atol=ATOL_EXPF, rtol=0, err_msg=name)
    np.testing.assert_array_equal(got == 0, want == 0, err_msg=name)
    if name in ('on_gate', 'inside_gate', 'at_zfar'):                 # the contributing set at the boundary pixel is the oracle's (margin 1e-4)
      val, _ = D.bilateral_pixel(d, 4, 5, zfar=zfar)
      assert abs(float(got[4, 5]) - val) < ATOL_EXPF < D.MARGIN / 10
  assert U.bilateral_filter_depth(images['split'][0], radius=2)[4, 5] == 0 and not U.bilateral_filter_depth(images['empty'][0], radius=2).any()


def test_depth2xyz_keeps_a_pixel_equal_to_zfar(U):
  d = D.noise_image((13, 37), 1)
  above = np.nextafter(f32(2.0), f32(3))
  d[3, 4], d[3, 5], d[3, 6], d[3, 7] = f32(2.0), above, f32(0.001), np.nextafter(f32(0.001), f32(0))
  for zfar in (2.0, np.inf):
    got = U.depth2xyzmap_batch(torch.from_numpy(d)[None], torch.as_tensor(K, dtype=torch.float32)[None], zfar=zfar)[0].cpu().numpy()
    np.testing.assert_array_equal(got, _xyz_oracle(d, zfar))
  got = U.depth2xyzmap_batch(torch.from_numpy(d)[None], torch.as_tensor(K, dtype=torch.float32)[None], zfar=2.0)[0].cpu().numpy()
  assert got[3, 4, 2] == 2 and not got[3, 5].any() and got[3, 6, 2] == f32(0.001) and not got[3, 7].any()


def _all_images():
  for hw in D.NOISE_SIZES:
    yield f'noise_{hw[0]}x{hw[1]}', D.noise_image(hw, hw[0]), dict(depth_diff_thres=0.001, zfar=2.0)
  for name, d, kw in D.erode_cases():
    yield name, d, kw
  for hw in ((9, 11), (13, 37)):
    yield f'gate_{hw[0]}', D.gate_image(hw, D.M + D.E), dict(depth_diff_thres=0.05, zfar=100)
    yield f'zfar_{hw[0]}', D.zfar_bilateral_image(hw), dict(depth_diff_thres=0.05, zfar=2.0)


@pytest.mark.parametrize('radius', [1, 2, 3])
def test_three_kernels_at_every_radius(U, radius):
  from oracle import geometry as G
  for name, d, kw in _all_images():
    e_o = G.erode_depth(d, radius=radius, ratio_thres=0.8, **kw)
    np.testing.assert_array_equal(U.erode_depth(d, radius=radius, ratio_thres=0.8, **kw), e_o, err_msg=name)
    for src in (d, e_o):
      b_o = G.bilateral_filter_depth(src, radius=radius, zfar=kw['zfar'])
      b_g = U.bilateral_filter_depth(src, radius=radius, zfar=kw['zfar'])
      np.testing.assert_allclose(b_g, b_o, atol=ATOL_EXPF, rtol=0, err_msg=name)
      np.testing.assert_array_equal(b_g == 0, b_o == 0, err_msg=name)


def test_prefilter_equals_the_chain_and_the_oracle(U):
  """depth_prefilter (radius 2): bit-identical to the three kernels chained on the device and, judged by something other than its siblings,
  the oracle chain on the CPU: eroded pixels exactly where the oracle erodes, depth within the expf allowance, the xyz map exactly
  depth2xyzmap_batch of the depth it returns"""
  from oracle import geometry as G
  for name, d, kw in _all_images():
    dt = torch.from_numpy(d).cuda()
    zf = kw['zfar']
    chain_d = U.bilateral_filter_depth(U.erode_depth(dt, radius=2, **kw), radius=2, zfar=zf)
    chain_x = U.depth2xyzmap_batch(chain_d[None], K.astype(np.float32)[None], zfar=np.inf)[0]
    fused_d, fused_x = U.depth_prefilter(dt, K, radius=2, **kw)
    assert torch.equal(fused_d, chain_d) and torch.equal(fused_x, chain_x), name
    want_d = G.bilateral_filter_depth(G.erode_depth(d, radius=2, **kw), radius=2, zfar=zf)
    got_d = fused_d.cpu().numpy()
    np.testing.assert_allclose(got_d, want_d, atol=ATOL_EXPF, rtol=0, err_msg=name)
    np.testing.assert_array_equal(got_d == 0, want_d == 0, err_msg=name)
    np.testing.assert_array_equal(fused_x.cpu().numpy(), _xyz_oracle(got_d, np.inf), err_msg=name)


# ------------------------------------------------------------------------------------------------------------------------------------------
# radix-select median
# ------------------------------------------------------------------------------------------------------------------------------------------
def _single(depth, mask, min_depth=0.001):
  """fp_mask_depth_stats with the mask bytes as they are (Utils.mask_depth_stats would turn them into 0 / 1)"""
  from foundationpose_amd import _lib as L
  d, m = torch.from_numpy(depth).cuda().contiguous(), torch.from_numpy(mask).cuda().contiguous()
  st, med = (ctypes.c_int32 * 6)(), ctypes.c_float()
  L.check(L.lib().fp_mask_depth_stats(L.Context.get(d.device).handle, L.ptr(d), L.ptr(m), d.shape[0], d.shape[1], float(min_depth), st, ctypes.byref(med),
                                      L.stream_ptr(d.device)))
  return tuple(st), f32(med.value)


def _objects(depth, masks=None, label_image=None, labels=None, min_depth=0.001):
  from foundationpose_amd import _lib as L
  d = torch.from_numpy(depth).cuda().contiguous()
  H, W = d.shape
  if masks is not None:
    keep = [torch.from_numpy(m).cuda().contiguous() for m in masks]
    n, mptr, lptr, ids = len(keep), (ctypes.c_void_p * len(keep))(*[m.data_ptr() for m in keep]), None, None
  else:
    keep = torch.from_numpy(label_image.astype(np.int32)).cuda().contiguous()
    n, mptr, lptr, ids = len(labels), None, L.ptr(keep), (ctypes.c_int32 * len(labels))(*labels)
  st, med = (ctypes.c_int32 * (6 * n))(), (ctypes.c_float * n)()
  L.check(L.lib().fp_mask_depth_stats_objects(L.Context.get(d.device).handle, L.ptr(d), mptr, lptr, ids, n, H, W, float(min_depth), st, med, L.stream_ptr(d.device)))
  return [(tuple(st[6 * o:6 * o + 6]), f32(med[o])) for o in range(n)]


def _same(got, want, what):
  assert got[0] == want[0], (what, got, want)
  assert got[1].view(np.uint32) == want[1].view(np.uint32), (what, got[1], want[1])


MEDIAN_CASES = list(D.median_cases())


@pytest.mark.parametrize('name,depth,mask', MEDIAN_CASES, ids=lambda v: v if isinstance(v, str) else '')
def test_median_and_counts_equal_numpy(U, name, depth, mask):
  want = D.median_expected(depth, mask)
  _same(_single(depth, mask), want, name)
  _same(_objects(depth, masks=[mask])[0], want, name + ' objects')
  _same(_objects(depth, label_image=mask.astype(np.int32) * 7, labels=[7 * int(mask.max())])[0], want, name + ' labels')
  st = U.mask_depth_stats(depth, mask)                       # the Python wrappers
  assert (st['cmin'], st['cmax'], st['rmin'], st['rmax'], st['n_mask'], st['n_usable']) == want[0] and st['median'] == want[1]
  so = U.mask_depth_stats_objects(depth, [mask])[0]
  assert so == st


def test_objects_with_overlapping_boxes(U):
  """several objects in one launch: masks whose bounding boxes (and pixels) overlap, and a label image whose objects interleave"""
  by_size = [c for c in MEDIAN_CASES if c[1].shape == (25, 41)]
  depth = by_size[0][1].copy()
  masks = []
  for k, (name, d, m) in enumerate(by_size[:6]):             # values of six cases laid into one depth image; later cases overwrite shared pixels
    depth[m != 0] = d[m != 0]
    masks.append(m)
  got = _objects(depth, masks=masks)
  for m, g in zip(masks, got):
    _same(g, D.median_expected(depth, m), 'masks')
  boxes = [D.median_expected(depth, m)[0][:4] for m in masks[:2]]
  assert boxes[0][0] <= boxes[1][1] and boxes[1][0] <= boxes[0][1] and (masks[0].astype(bool) & masks[1].astype(bool)).any()
  rng = np.random.default_rng(9)
  labels = rng.integers(0, 4, (25, 41)).astype(np.int32) * 5          # 0 = background, objects 5, 10, 15 interleaved pixel by pixel
  depth2 = np.resize(D.median_value_sets()['duplicates'], 1025).reshape(25, 41).copy()
  depth2[rng.uniform(size=(25, 41)) < 0.1] = np.nextafter(f32(0.001), f32(0))
  got = _objects(depth2, label_image=labels, labels=[5, 10, 15, 999])
  for lab, g in zip((5, 10, 15), got):
    _same(g, D.median_expected(depth2, (labels == lab).astype(np.uint8)), f'label {lab}')
  assert got[3][0][4:] == (0, 0) and got[3][1] == 0                    # an absent label: nothing masked, median 0
