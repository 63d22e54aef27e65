"""The convolution encoder's kernels against the references of tests/tools/conv_ref.py, through the public entry points fp_conv2d_f16 and
fp_conv3x3_band_f16 only.  Every output buffer is NaN-prefilled and must hold no NaN afterwards.

A. test_conv_exact_integers: small-integer operands, for which every correct form gives the integer reference BIT for bit (torch.equal), in
   fp16 and in fp32: a dropped, doubled or misplaced term of any size shows.  Each case runs dense and relu_like activations, each with
   (residual, ReLU) and with (no residual, no ReLU).
B. test_conv_against_float64: randn-like operands in four regimes against float64 with the per-element bound
   |got - o| <= 2^-11 |o| + 2^-25 + 62 x 2^-24 S (fp32 output: 2^-23 |o| + 62 x 2^-24 S): fp32 accumulation all the way, the residual added in
   fp32 before the one rounding, fp16 subnormals in and out.  Prints the largest |err| / tol per case and regime (pytest -s).
That the inputs are what they claim to be, that the integer reference is exact and that the bound tells four wrong kernels from a right one is
shown on the CPU by tests/test_conv_ref_host.py.

CASE -> KERNEL (rocprofv3 --kernel-trace --stats over this file on an MI355X; `form` is the first field of a case id).
  case form (residual)                          kernel(s) of the trace
  small<KS,HW,ST[,NW]> (with and without)       conv3x3_small_kernel<1,40,1,8> / <2,40,1,8> / <4,20,1,8> / <2,40,2,8> / <1,80,2,4>: each of the five
  halo-splitk (with and without)                conv3x3_halo_splitk_kernel<40> (2 x 40x40 x 256) or <20> (3, 4, 5 x 20x20 x 512) + splitk_finish_kernel
  halo-tail1..4, halo-round                     conv3x3_halo_dma_kernel<20 | 40, RES = true | false, false>: one kernel, the tile sizes by halo_plan (the
                                                host test restates it: 6 / 32 / 50 / 63 images at 512 channels give tiles of 1 / 2 / 3 / 4 x 128 pixels)
  fp32 output of all thirteen halo shapes       conv_igemm2_kernel<128, 3, false, false> (the residual is read directly in that output mode)
  s1b                                           conv3x3_s1_band_kernel<true | false>
  s2 without a residual                         conv3x3_s2_kernel<20, 8, 2> (256 -> 512), <20, 8, 1> (64 -> 128)
  s2 with one                                   conv_igemm2_kernel<128, 3, false, true>
  s2-splitk (with and without)                  conv_igemm2_splitk_kernel<128, 3> + splitk_finish_kernel
  stem without a residual                       stem7x7_kernel
  stem with one                                 conv_igemm2_kernel<64, 7, true, true>
  igemm2<BM,KW[,CIN8]> without / with           conv_igemm2_kernel<128, 3, false>, <64, 3, false>, <64, 7, true>, <128, 7, true>, <128, 1, false>, <64, 1, false>,
                                                each with RES = false / true: all twelve instantiations; fp32 output of the Linear shapes: <128 | 64, 1, false, false>
  All eight forms, the five conv_small and the twelve conv_igemm2 instantiations are reached; no case landed in a form other than the one it names.

LARGEST |err| / tol PER REGIME on an MI355X:
  fp16 output:  relu 0.970 (halo-tail1 3x40x40 128)   wide 0.982 (halo-round 83x40x40 128)   cancel 0.300 (igemm2<128,3> 1x33x9)   res_cancel 0.726 (halo-round)
  fp32 output:  relu 0.039   wide 0.230   cancel 0.004   res_cancel 0.149 (3x40x40 128 -> 128)
  relu and wide sit just below 1 in fp16 because the bound's first term IS the worst case of the one output rounding (half a step at the bottom of a
  binade); where that term is small beside the values handed on (cancel) or absent (fp32) the kernels use a third of the bound or less.
  All 45 exact-integer cases are bit-identical.  The whole file takes 14 s, its slowest test 1.2 s.
"""
import pytest
import torch

from tests.tools import conv_ref as R

pytestmark = pytest.mark.gpu

EXACT_IDS = [R.case_id(c) for c in R.EXACT_CASES]
NUM_PARAMS = R.num_params()
NUM_IDS = [f'{R.case_id(c)}-{r}' for c, r in NUM_PARAMS]


@pytest.fixture(scope='module')
def ctx():
  from foundationpose_amd import _lib
  return _lib.Context.get('cuda:0')


def run_conv(ctx, c, dev, use_res, relu, out_f32):
  """One launch of case c on the device operands `dev` (x, wp, b, res) -> (N, Ho, Wo, Cout) on the CPU, NaN-checked."""
  from foundationpose_amd._lib import check, lib, ptr, stream_ptr
  Ho, Wo = R.out_hw(c)
  out = torch.full((c.N, Ho, Wo, c.Cout), float('nan'), dtype=torch.float32 if out_f32 else torch.float16, device='cuda')
  res = ptr(dev['res']) if use_res else None
  h, s = ctx.handle, stream_ptr()
  if c.entry == 'band':
    assert c.H == c.W == 40 and c.Cin == c.Cout and not out_f32
    check(lib().fp_conv3x3_band_f16(h, ptr(dev['x']), c.N, c.Cin, ptr(dev['wp']), ptr(dev['b']), res, int(relu), ptr(out), s))
  else:
    check(lib().fp_conv2d_f16(h, ptr(dev['x']), c.N, c.H, c.W, R.cin_pad(c), ptr(dev['wp']), ptr(dev['b']), c.Cout, c.k, c.k, c.stride, (c.k - 1) // 2,
                              res, int(relu), ptr(out), int(out_f32), s))
  torch.cuda.synchronize()
  got = out.cpu()
  n_nan = int(torch.isnan(got).sum())
  assert n_nan == 0, f'{R.case_id(c)} out_f32={out_f32} residual={use_res}: {n_nan} of {got.numel()} outputs were not written or are NaN'
  return got


def to_device(d):
  dev = {k: d[k].cuda() for k in ('x', 'wp', 'b')}
  dev['res'] = None if d['res'] is None else d['res'].cuda()
  return dev


@pytest.mark.parametrize('c', R.EXACT_CASES, ids=EXACT_IDS)
def test_conv_exact_integers(ctx, c):
  """torch.equal with the integer reference, fp16 and (where the case lists it: every halo shape and the Linear layers) fp32 output.  On
  failure: the first mismatch as (image, row, column, channel, got, reference) and the number of mismatches."""
  for variant in R.VARIANTS:
    d = R.exact_case(c, variant)
    dev = to_device(d)
    for use_res, relu in ((True, True), (False, False)):
      want = R.exact_expected(d, use_res, relu)
      for out_f32 in c.outs:
        got = run_conv(ctx, c, dev, use_res, relu, out_f32)
        msg = R.first_mismatch(got.float(), want)
        assert msg == '', f'{R.case_id(c)} {variant} residual={use_res} relu={relu} out_f32={out_f32}: {msg}'


@pytest.mark.parametrize('c,regime', NUM_PARAMS, ids=NUM_IDS)
def test_conv_against_float64(ctx, c, regime):
  """|got - o| <= tol for every output element, tol the per-element bound of tests/tools/conv_ref.py from the float64 reference alone.
  Prints the largest |err| / tol with its element (pytest -s)."""
  d = R.num_case(c, regime)
  out_f32 = c.outs == (1,)
  got = run_conv(ctx, c, to_device(d), d['res'] is not None, d['relu'], out_f32).double()
  ratio = (got - d['o']).abs() / d['tol']
  i = tuple(int(v) for v in torch.nonzero(ratio == ratio.max())[0])
  line = (f'{R.case_id(c)} {regime}: max |err| / tol {float(ratio[i]):.3f} at (image {i[0]}, row {i[1]}, column {i[2]}, channel {i[3]}): '
          f'got {float(got[i]):.6g}, reference {float(d["o"][i]):.6g}, tol {float(d["tol"][i]):.2e}')
  print(line)
  assert float(ratio[i]) <= 1.0, line
