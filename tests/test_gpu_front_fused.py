"""The front end of encodeA as one launch (csrc/front.hip: the 7x7 stem and the 64 -> 128 stride-2 layer, the stem's output in LDS only)
against the two launches it replaces, through the public entry points fp_front_end_f16 and fp_conv2d_f16 only.

A. test_fused_equals_two_launches: fused == stem7x7_kernel followed by conv_igemm2_kernel<128, 3>, np.array_equal on a1 and on the stem's
   output as the fused kernel's tiles hold it, at 1, 2, 3 and 5 images (a persistent grid with fewer tiles than CUs, odd counts, tiles that end
   an image) x seeded normal inputs, all-zero images, images that are zero outside a disc, images whose only non-zero pixels are the border
   rows and columns.  The two-launch reference of a kind is computed ONCE, on the five images: a stand-alone fp_conv2d_f16 of one or two
   images of the stride-2 layer takes the few-image form (conv_small.hip, its own size class with its own last bits), which is not what the
   fused launch replaces; a pixel's arithmetic does not depend on its batch, so images [0, n) of the five-image reference are the two launches'
   result for n images.
B. test_exact_integers: small-integer inputs, sparse +-1 weights: every a0 and a1 value stays within 2048 (asserted on the reference), so
   every correct kernel gives the int64 numpy convolution of this file bit for bit.
C. test_whole_passes_do_not_change: the fused passes (tests/tools/variant_digest.py) under FP_FRONT_FUSED=0 and under the default print the
   same digests, one fresh process per knob set (the knobs are read once per process): 5, 8 and 56 hypotheses and 100 with a shared
   translation; again with the observed side per hypothesis and both sides as one chain (the branch that runs the two stems apart).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NMAX = 5
KINDS = ('normal', 'zeros', 'disc', 'border')
K0, K1 = 416, 576          # Kpad of the two layers: roundup(49 * 8, 32), 9 * 64


@pytest.fixture(scope='module')
def ctx():
  from foundationpose_amd import _lib
  return _lib.Context.get('cuda:0')


def pack_rows(w):
  """(Cout, KH, KW, Cin) -> [Cout][Kpad] fp16 rows, k = (ky * KW + kx) * Cin + ci, zero padded (include/foundationpose_amd.h: fp_conv2d_f16)"""
  co, kh, kw, ci = w.shape
  kpad = (kh * kw * ci + 31) // 32 * 32
  out = np.zeros((co, kpad), np.float16)
  out[:, :kh * kw * ci] = w.reshape(co, -1)
  return out


def make_weights(seed):
  r = np.random.default_rng(seed)
  w0 = (r.standard_normal((64, 7, 7, 8)) * 0.06).astype(np.float16)
  w0[..., 6:] = 0
  w1 = (r.standard_normal((128, 3, 3, 64)) * 0.04).astype(np.float16)
  return w0, (r.standard_normal(64) * 0.1).astype(np.float32), w1, (r.standard_normal(128) * 0.1).astype(np.float32)


def make_input(kind, seed):
  r = np.random.default_rng(seed)
  x = r.standard_normal((NMAX, 160, 160, 8)).astype(np.float16)
  x[..., 6:] = 0
  yy, xx = np.mgrid[0:160, 0:160]
  if kind == 'zeros':
    x[:] = 0
  elif kind == 'disc':           # rendered-like: zero outside a disc, another one per image (one touches the image edge)
    for i, (cy, cx, rad) in enumerate(((80, 80, 50), (30, 120, 45), (100, 60, 20), (159, 0, 70), (79.5, 79.5, 3))):
      x[i][(yy - cy) ** 2 + (xx - cx) ** 2 > rad * rad] = 0
  elif kind == 'border':         # only the border rows and columns (the four corners among them): padding and halo rows at every edge
    keep = (yy == 0) | (yy == 159) | (xx == 0) | (xx == 159)
    x[:, ~keep] = 0
  return x


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_two(ctx, x, w0p, b0, w1p, b1):
  """stem, then the stride-2 layer, as two stand-alone launches -> (a0, a1) on the CPU"""
  from foundationpose_amd._lib import check, lib, ptr, stream_ptr
  n = x.shape[0]
  a0 = torch.full((n, 80, 80, 64), float('nan'), dtype=torch.float16, device='cuda')
  a1 = torch.full((n, 40, 40, 128), float('nan'), dtype=torch.float16, device='cuda')
  check(lib().fp_conv2d_f16(ctx.handle, ptr(x), n, 160, 160, 8, ptr(w0p), ptr(b0), 64, 7, 7, 2, 3, None, 1, ptr(a0), 0, stream_ptr()))
  check(lib().fp_conv2d_f16(ctx.handle, ptr(a0), n, 80, 80, 64, ptr(w1p), ptr(b1), 128, 3, 3, 2, 1, None, 1, ptr(a1), 0, stream_ptr()))
  torch.cuda.synchronize()
  return a0.cpu().numpy(), a1.cpu().numpy()


def run_fused(ctx, x, w0p, b0, w1p, b1, with_a0=True):
  from foundationpose_amd._lib import check, lib, ptr, stream_ptr
  n = x.shape[0]
  a0 = torch.full((n, 80, 80, 64), float('nan'), dtype=torch.float16, device='cuda') if with_a0 else None
  a1 = torch.full((n, 40, 40, 128), float('nan'), dtype=torch.float16, device='cuda')
  check(lib().fp_front_end_f16(ctx.handle, ptr(x), n, ptr(w0p), ptr(b0), ptr(w1p), ptr(b1), ptr(a1), ptr(a0) if with_a0 else None, stream_ptr()))
  torch.cuda.synchronize()
  return (a0.cpu().numpy() if with_a0 else None), a1.cpu().numpy()


def first_diff(got, want):
  bad = np.argwhere(got.view(np.uint16) != want.view(np.uint16))
  if len(bad) == 0:
    return None
  i = tuple(bad[0])
  return f'{len(bad)} of {got.size} differ; first at (image, row, column, channel) = {i}: got {got[i]!r}, expected {want[i]!r}'


_two = {}


@pytest.fixture(scope='module')
def operands(ctx):
  w0, b0, w1, b1 = make_weights(7)
  return dict(w0p=dev(pack_rows(w0)), b0=dev(b0), w1p=dev(pack_rows(w1)), b1=dev(b1))


def two_launch_reference(ctx, operands, kind):
  """(x on the device, a0, a1) of the five images of `kind`: computed once, read by every image count"""
  if kind not in _two:
    x = dev(make_input(kind, 11 + KINDS.index(kind)))
    a0, a1 = run_two(ctx, x, **operands)
    assert not np.isnan(a0).any() and not np.isnan(a1).any()
    a0.setflags(write=False), a1.setflags(write=False)
    _two[kind] = (x, a0, a1)
  return _two[kind]


@pytest.mark.parametrize('n', (1, 2, 3, 5))
@pytest.mark.parametrize('kind', KINDS)
def test_fused_equals_two_launches(ctx, operands, kind, n):
  x, a0_ref, a1_ref = two_launch_reference(ctx, operands, kind)
  a0, a1 = run_fused(ctx, x[:n].contiguous(), **operands)
  assert not np.isnan(a0).any(), f'{int(np.isnan(a0).sum())} a0 values were not written or are NaN'
  assert not np.isnan(a1).any(), f'{int(np.isnan(a1).sum())} a1 values were not written or are NaN'
  if kind != 'zeros':
    assert np.count_nonzero(a1) > a1.size // 20
  msg = first_diff(a0, a0_ref[:n])
  assert msg is None, 'stem phase (a0): ' + msg
  msg = first_diff(a1, a1_ref[:n])
  assert msg is None, 'a1: ' + msg
  # the a0 image is an extra output: without it the launch writes the same a1
  _, a1_plain = run_fused(ctx, x[:n].contiguous(), with_a0=False, **operands)
  assert np.array_equal(a1_plain.view(np.uint16), a1.view(np.uint16))


def conv_int64(x, w, b, stride, pad):
  """x (n, H, W, Ci) int64, w (Co, KH, KW, Ci) int64, b (Co) int64 -> relu(conv + b), (n, Ho, Wo, Co) int64; one matrix product per tap"""
  n, H, W, ci = x.shape
  co, kh, kw, _ = w.shape
  ho, wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
  xp = np.zeros((n, H + 2 * pad, W + 2 * pad, ci), np.int64)
  xp[:, pad:pad + H, pad:pad + W] = x
  out = np.zeros((n, ho, wo, co), np.int64) + b
  for ky in range(kh):
    for kx in range(kw):
      out += xp[:, ky:ky + stride * ho:stride, kx:kx + stride * wo:stride] @ w[:, ky, kx].T
  return np.maximum(out, 0)


def test_exact_integers(ctx):
  r = np.random.default_rng(3)
  n = 2
  x = r.integers(-2, 3, (n, 160, 160, 8)).astype(np.int64)
  x[..., 6:] = 0
  x[1, 40:120, 40:120] = 0                                 # the second image: a frame of values around an empty middle
  w0 = (r.integers(0, 2, (64, 7, 7, 8)) * 2 - 1) * (r.random((64, 7, 7, 8)) < 0.1)
  w0[..., 6:] = 0
  w1 = (r.integers(0, 2, (128, 3, 3, 64)) * 2 - 1) * (r.random((128, 3, 3, 64)) < 0.04)
  b0, b1 = r.integers(-3, 4, 64), r.integers(-3, 4, 128)
  a0_ref = conv_int64(x, w0.astype(np.int64), b0, 2, 3)
  a1_ref = conv_int64(a0_ref, w1.astype(np.int64), b1, 2, 1)
  # every partial sum is bounded by the sum of the magnitudes: exact in fp32, and the results are exact in fp16
  m0 = int((conv_int64(np.abs(x), np.abs(w0).astype(np.int64), np.abs(b0), 2, 3)).max())
  m1 = int((conv_int64(a0_ref, np.abs(w1).astype(np.int64), np.abs(b1), 2, 1)).max())
  assert 0 < m0 <= 2048 and 0 < m1 <= 2048, (m0, m1)
  assert np.count_nonzero(a1_ref) > a1_ref.size // 10
  ops = dict(w0p=dev(pack_rows(w0.astype(np.float16))), b0=dev(b0.astype(np.float32)), w1p=dev(pack_rows(w1.astype(np.float16))), b1=dev(b1.astype(np.float32)))
  a0, a1 = run_fused(ctx, dev(x.astype(np.float16)), **ops)
  msg = first_diff(a0, a0_ref.astype(np.float16))
  assert msg is None, 'a0: ' + msg
  msg = first_diff(a1, a1_ref.astype(np.float16))
  assert msg is None, 'a1: ' + msg


def test_whole_passes_do_not_change():
  import json, os, subprocess, sys
  script = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools', 'variant_digest.py')

  def digests(knobs, sizes):
    r = subprocess.run([sys.executable, script] + [str(s) for s in sizes], env=dict(os.environ, **knobs), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f'{knobs}: {r.stdout[-1500:]}\n{r.stderr[-1500:]}'
    return json.loads([l for l in r.stdout.splitlines() if l.startswith('DIGEST ')][-1][7:])
  for knobs, sizes in (({}, (5, 8, 56, 100)), ({'FP_NO_SHARED_B': '1', 'FP_ONE_CHAIN': '1'}, (5, 8, 56))):
    fused = digests(knobs, sizes)
    assert len(set(fused.values())) == len(sizes)
    assert digests(dict(knobs, FP_FRONT_FUSED='0'), sizes) == fused, knobs
