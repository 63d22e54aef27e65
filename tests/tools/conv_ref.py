"""References, inputs and bounds of the convolution encoder's tests (csrc/conv_small.hip, conv_halo.hip, conv_s1b.hip, conv_s2.hip, conv.hip,
stem.hip).  Plain torch / numpy, no GPU: tests/test_conv_ref_host.py checks what is here, tests/test_gpu_conv_numerics.py the
kernels against it.  Every reference reads the SAME fp16 operands the kernel reads.

A. EXACT-INTEGER PARITY (EXACT_CASES, exact_case).  Activations are integers in {-2, -1, 1, 2} (`dense`: no zeros, every product is nonzero and
every dropped, doubled or misplaced term shows) or the same with about half of them set to exact 0 (`relu_like`); weights in {-1, 0, 1}; bias and
residual integers in [-8, 8].  The stem's activations are integers in [-3, 3] in six channels, padded to eight: the two pad channels hold zero
ACTIVATIONS and nonzero garbage WEIGHTS.  Every partial sum is an integer below 2^24, so fp32 addition is exact in any order, and every result
with |value| <= 2048 is exact in fp16: whatever form runs - one launch, K split over waves, split-K with its finishing pass - has to give the integer reference bit for bit, in fp16 and in fp32.  The reference is
torch's float32 conv2d; the host test shows on every case that it equals the float64 one and that max |conv + bias + residual| <= 2048.

The form each case runs (`form` below) was worked out by hand for the 256 CUs of an MI355X, from the rules that csrc/conv_plan.h now states in
one place; tests/test_conv_plan_host.py plans every case with that header and asserts the form named here (the kernel names a profiler shows are
in the docstring of tests/test_gpu_conv_numerics.py):
  conv_small.hip takes a launch of at most 2 x 256 workgroups of 32 pixels x 32 couts: two images of every layer but 256 -> 256 (one).
  halo split-K: n_q = ceil(M / 128) (Cout / 128) quarter tiles with 4 n_q <= 256 and at least 8 chunks of 32 input channels.  512 channels at
    20x20: up to FIVE images (16 x 4 x 4 = 256) - so the smallest batch that runs one-launch tail tiles there is 6, not 5.
  halo tail tiles (halo_plan, cost 0.43 / 0.62 / 0.81 / 1.0 per round of 1 / 2 / 3 / 4 x 128-pixel tiles): 512 channels at 20x20, four cout
    tiles: 6 images 76 tiles of 128; 32: 200 of 256; 50: 212 of 384; 63: 200 of 512.  128 channels at 40x40: 3 images 38 of 128; 37: 232 of 256.
  halo whole round + tail: 83 x 400 pixels = 260 quarters = 256 tiles of 512 + 16 of 128; 42 x 1600 (two cout tiles): 256 + 26; 83 x 1600: 256 + 14.
  a residual keeps a layer out of conv_s2.hip and stem.hip (neither adds one): those cases run the generic kernel's RES variants when it is
    there, the fp32 output of the halo shapes the generic kernel's <128, 3> variant without.

B. FLOAT64 PARITY WITH A PER-ELEMENT BOUND (NUM_CASES, REGIMES, num_case).  o = [relu](sum x w + b [+ res]) in float64, S = sum |x w| + |b| +
|res| per element, and

    |got - o| <= 2^-11 |o| + 2^-25 + C_ACC 2^-24 S          (fp16 output: one rounding, half a subnormal step, fp32 accumulation)
    |got - o| <= 2^-23 |o| + C_ACC 2^-24 S                  (fp32 output)

C_ACC = 62.  It does not come from a GPU.  An honest fp32 accumulation of the same operands was simulated two ways on the CPU - torch's float32
conv2d (oneDNN: long chains per output element, every element of the tensor), and for 192 seeded elements per case a chain acc = fmaf(x_k, w_k,
acc) over k in the packed order (ky, kx, channel) - and |sim - o| / (2^-24 S) taken before any output rounding, over all 16 cases in every
regime (python -m tests.tools.conv_ref prints the table).  Largest values per regime, conv2d / chain:
    relu 6.09 / 3.20     wide 15.31 / 6.14     cancel 2.14 / 1.06     res_cancel 0.28 / 0.28
The largest of all is 15.31 (wide, conv2d, (3, 40x40, 128 -> 128); (83, 40x40, 128 -> 128) gives 15.01 over its 17 million elements).  These are
maxima of a long tail: in relu at (1, 40x40, 128 -> 128) the 99.99 % quantile is 3.0 beside a maximum of 4.7, and the same sums by im2col + GEMM
stay below 2.  Times 4 for the orders a kernel may choose: 61.2, rounded up to 62.  At K = 4608 this is 0.015 of the
worst-case bound K 2^-24 S of a sum of K terms.

Regimes:
  relu        x = randn.relu(), w = randn sqrt(2 / K), b = randn 0.1, residual randn, ReLU: the baseline (what the older tests draw).
  wide        per-input-channel scales of x and per-output-channel scales of w and b run from 2^-14 to 2^2 (evenly spaced exponents, shuffled);
              no residual, no ReLU.  Outputs span 20 binades; at least WIDE_SUBNORMAL_SHARE = 3 % of them are nonzero fp16 subnormals (expected
              ~ 8 %: an output channel of scale 2^e, e uniform in [-14, 2], holds values of std ~ 0.85 2^e), and so are a good part of the
              activations and weights.
  cancel      the second half of the input channels repeats the first (x > 0) and carries the weights -w + 2e-3 |w|: each output is the
              difference of two halves of size S / 2 that cancel to ~ 1e-3 S.  Whatever a kernel hands on between channel groups - the chunk
              loop, LDS between the waves of conv_small, the split-K scratch - is ~ S / 2 and has to be fp32.  No residual, no ReLU.
  res_cancel  conv + bias near +3e4 (the bias is 3e4 + randn 50), the residual near -2.9e4, the sum near 1e3; ReLU.  A kernel that rounds to
              fp16 before the residual add is off by up to 8 (half an fp16 step at 3e4); the bound allows ~ 0.75
              (2^-11 x 1e3 + 62 x 2^-24 x 6e4).
  Layers that take no residual in their own form (conv_s2.hip, stem.hip) run relu without one and have no res_cancel case.

Mutants of the reference the host test shows to lie OUTSIDE the bound (num_mutant): partial sums rounded to fp16 between 32-channel chunks
(cancel; cases with at least two chunks), conv + bias rounded to fp16 before the residual add (res_cancel), fp16 subnormal outputs flushed to
zero (wide), the residual added after the ReLU (relu).
"""
import collections
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

Case = collections.namedtuple('Case', 'form entry N H W Cin Cout k stride outs takes_res')
# outs: the output types the case runs (0 fp16, 1 fp32).  takes_res: the named form adds a residual itself


def _c(form, N, H, W, Cin, Cout, k=3, stride=1, entry='conv2d', outs=(0,), takes_res=True):
  return Case(form, entry, N, H, W, Cin, Cout, k, stride, outs, takes_res)


def case_id(c):
  hw = str(c.H) if c.H == c.W else f'{c.H}x{c.W}'
  return f'{c.form}-{c.N}x{hw}-{c.Cin}to{c.Cout}' + (f'-k{c.k}' if c.k != 3 else '') + (f'-s{c.stride}' if c.stride != 1 else '')


EXACT_CASES = (
  # conv_small.hip: one case per instantiation at one image and at the largest launch it takes
  _c('small<1,40,1>', 1, 40, 40, 128, 128), _c('small<1,40,1>', 2, 40, 40, 128, 128),
  _c('small<2,40,1>', 1, 40, 40, 256, 256), _c('small<2,40,1>', 1, 40, 40, 256, 128), _c('small<2,40,1>', 2, 40, 40, 256, 128),
  _c('small<4,20,1>', 1, 20, 20, 512, 512), _c('small<4,20,1>', 2, 20, 20, 512, 512),
  _c('small<2,40,2>', 1, 40, 40, 256, 512, stride=2), _c('small<2,40,2>', 2, 40, 40, 256, 512, stride=2),
  _c('small<1,80,2,4>', 1, 80, 80, 64, 128, stride=2), _c('small<1,80,2,4>', 2, 80, 80, 64, 128, stride=2),
  # conv_halo.hip: split-K + finishing pass
  _c('halo-splitk', 2, 40, 40, 256, 256, outs=(0, 1)), _c('halo-splitk', 3, 20, 20, 512, 512, outs=(0, 1)),
  _c('halo-splitk', 4, 20, 20, 512, 512, outs=(0, 1)), _c('halo-splitk', 5, 20, 20, 512, 512, outs=(0, 1)),
  # conv_halo.hip: tail tiles only, nt = 1, 2, 3, 4 x 128 pixels
  _c('halo-tail1', 6, 20, 20, 512, 512, outs=(0, 1)), _c('halo-tail2', 32, 20, 20, 512, 512, outs=(0, 1)),
  _c('halo-tail3', 50, 20, 20, 512, 512, outs=(0, 1)), _c('halo-tail4', 63, 20, 20, 512, 512, outs=(0, 1)),
  _c('halo-tail1', 3, 40, 40, 128, 128, outs=(0, 1)), _c('halo-tail2', 37, 40, 40, 128, 128, outs=(0, 1)),
  # conv_halo.hip: a whole round of 512-pixel tiles + tail
  _c('halo-round', 83, 20, 20, 512, 512, outs=(0, 1)), _c('halo-round', 42, 40, 40, 256, 256, outs=(0, 1)),
  _c('halo-round', 83, 40, 40, 128, 128, outs=(0, 1)),
  # conv_s1b.hip
  _c('s1b', 1, 40, 40, 128, 128, entry='band'), _c('s1b', 3, 40, 40, 128, 128, entry='band'), _c('s1b', 37, 40, 40, 128, 128, entry='band'),
  _c('s1b', 5, 40, 40, 256, 256, entry='band'),
  # conv_s2.hip (5 images: exactly S2_MIN_PIXELS output pixels)
  _c('s2', 5, 40, 40, 256, 512, stride=2, takes_res=False), _c('s2', 9, 40, 40, 256, 512, stride=2, takes_res=False),
  _c('s2', 9, 40, 40, 64, 128, stride=2, takes_res=False),
  # conv.hip: stride-2 split-K + finishing pass
  _c('s2-splitk', 3, 40, 40, 256, 512, stride=2), _c('s2-splitk', 4, 40, 40, 256, 512, stride=2),
  # stem.hip
  _c('stem', 1, 32, 32, 6, 64, k=7, stride=2, takes_res=False), _c('stem', 3, 32, 64, 6, 64, k=7, stride=2, takes_res=False),
  _c('stem', 2, 160, 160, 6, 64, k=7, stride=2, takes_res=False),
  # conv.hip: the generic implicit GEMM
  _c('igemm2<128,3>', 3, 80, 80, 64, 128, stride=2), _c('igemm2<64,3>', 2, 17, 23, 32, 64), _c('igemm2<128,3>', 1, 33, 9, 64, 128),
  _c('igemm2<64,3>', 2, 41, 37, 32, 64, stride=2), _c('igemm2<64,7,CIN8>', 1, 34, 30, 6, 64, k=7, stride=2),
  _c('igemm2<128,7,CIN8>', 1, 34, 30, 6, 128, k=7, stride=2),
  _c('igemm2<128,1>', 1, 1, 1000, 512, 1024, k=1, outs=(0, 1)), _c('igemm2<64,1>', 1, 1, 130, 512, 64, k=1, outs=(0, 1)),
  _c('igemm2<64,1>', 3, 7, 5, 32, 64, k=1),
)
VARIANTS = ('dense', 'relu_like')
EXACT_LIMIT = 2048

# one case per form, the smallest of A that reaches it
NUM_CASES = (
  _c('small<1,40,1>', 1, 40, 40, 128, 128), _c('small<2,40,1>', 1, 40, 40, 256, 128), _c('small<4,20,1>', 1, 20, 20, 512, 512),
  _c('small<2,40,2>', 1, 40, 40, 256, 512, stride=2), _c('small<1,80,2,4>', 1, 80, 80, 64, 128, stride=2),
  _c('halo-splitk', 3, 20, 20, 512, 512), _c('halo-tail1', 3, 40, 40, 128, 128), _c('halo-round', 83, 40, 40, 128, 128),
  _c('s1b', 3, 40, 40, 128, 128, entry='band'), _c('s2', 5, 40, 40, 256, 512, stride=2, takes_res=False),
  _c('s2-splitk', 3, 40, 40, 256, 512, stride=2), _c('stem', 1, 32, 32, 6, 64, k=7, stride=2, takes_res=False),
  _c('igemm2<128,3>', 1, 33, 9, 64, 128), _c('igemm2<64,7,CIN8>', 1, 34, 30, 6, 64, k=7, stride=2),
  _c('igemm2<64,1>', 1, 1, 130, 512, 64, k=1), _c('fp32-igemm2<128,3>', 3, 40, 40, 128, 128, outs=(1,)),
)
REGIMES = ('relu', 'wide', 'cancel', 'res_cancel')
C_ACC = 62.0
WIDE_SUBNORMAL_SHARE = 0.03
F16_MIN_NORMAL = 2.0 ** -14
N_CHAIN = 192                                  # elements per case of the k-ordered fmaf chain


def num_params():
  return tuple((c, r) for c in NUM_CASES for r in REGIMES if r != 'res_cancel' or c.takes_res)


def _seed(*what):
  return zlib.crc32('-'.join(str(w) for w in what).encode()) & 0x7fffffff


def out_hw(c):
  pad = (c.k - 1) // 2
  return (c.H + 2 * pad - c.k) // c.stride + 1, (c.W + 2 * pad - c.k) // c.stride + 1


def cin_pad(c):
  return 8 if c.Cin < 8 else c.Cin


def pack_weight(w):
  """w (Cout, cin_pad, k, k) float32 holding fp16 values -> [Cout][Kpad] fp16, k index (ky, kx, channel), zeros up to the next multiple of 32."""
  cout, cp, k, _ = w.shape
  kraw = k * k * cp
  p = torch.zeros((cout, (kraw + 31) // 32 * 32), dtype=torch.float16)
  p[:, :kraw] = w.permute(0, 2, 3, 1).reshape(cout, kraw).half()
  return p


def _nhwc(t):
  return t.permute(0, 2, 3, 1).contiguous()


def _conv(x_nhwc, w, c, dtype):
  """conv2d of the NHWC activations with w (Cout, cin_pad, k, k), in dtype -> NHWC."""
  return _nhwc(F.conv2d(x_nhwc.permute(0, 3, 1, 2).to(dtype), w.to(dtype), stride=c.stride, padding=(c.k - 1) // 2))


def _rb(rs, shape):
  """Seeded bytes (the fastest thing numpy draws: the largest case holds 17 million activations)."""
  return np.frombuffer(rs.bytes(int(np.prod(shape))), dtype=np.uint8).reshape(shape)


def _ri(rs, lo, hi, shape):
  return torch.from_numpy((_rb(rs, shape) % (hi - lo + 1)).astype(np.float32) + lo)


@functools.lru_cache(maxsize=2)
def exact_case(c, variant):
  """-> dict(x (N, H, W, cin_pad) fp16, w (Cout, cin_pad, k, k) fp32, wp its packed fp16 image, b (Cout,) fp32, res (N, Ho, Wo, Cout) fp16,
  conv = conv + b (N, Ho, Wo, Cout) fp32: integers all of them); seeded from (case, variant)."""
  rs = np.random.RandomState(_seed('exact', case_id(c), variant))
  cp = cin_pad(c)
  Ho, Wo = out_hw(c)
  bits = _rb(rs, (c.N, c.H, c.W, cp))
  if c.Cin < 8:
    x = torch.from_numpy((bits % 7).astype(np.float32) - 3)
    x[..., c.Cin:] = 0
  else:
    x = torch.from_numpy(np.array([-2, -1, 1, 2], dtype=np.float32)[bits & 3])
  if variant == 'relu_like':
    x = x * torch.from_numpy(((bits >> 4) & 1).astype(np.float32))
  w = _ri(rs, -1, 1, (c.Cout, cp, c.k, c.k))
  if c.Cin < 8:
    w[:, c.Cin:] = torch.from_numpy(np.array([-7, -5, 3, 6], dtype=np.float32)[_rb(rs, (c.Cout, cp - c.Cin, c.k, c.k)) & 3])
  b = _ri(rs, -8, 8, (c.Cout,))
  res = _ri(rs, -8, 8, (c.N, Ho, Wo, c.Cout)).half()
  conv = _conv(x, w, c, torch.float32) + b
  return dict(x=x.half(), w=w, wp=pack_weight(w), b=b, res=res, conv=conv)


def exact_expected(d, use_res, relu):
  ref = d['conv'] + d['res'].float() if use_res else d['conv']
  return torch.relu(ref) if relu else ref


def first_mismatch(got, ref):
  """'' when equal, else the first differing element as (image, row, column, channel, got, reference) and the number of them."""
  bad = (got != ref) | torch.isnan(got)
  n = int(bad.sum())
  if n == 0:
    return ''
  i = tuple(int(v) for v in torch.nonzero(bad)[0])
  return f'{n} of {ref.numel()} elements differ; the first at (image {i[0]}, row {i[1]}, column {i[2]}, channel {i[3]}): got {float(got[i])}, reference {float(ref[i])}'


# ------------------------------------------------------------------------------------------------------------------------
# B: float64 parity

def _spread(g, n):
  """n scales 2^e, e evenly spaced over [-14, 2], shuffled."""
  return (2.0 ** torch.linspace(-14, 2, n))[torch.randperm(n, generator=g)]


def num_uses_res(c, regime):
  return c.takes_res and regime in ('relu', 'res_cancel')


def num_inputs(c, regime):
  """-> dict(x (N, H, W, cin_pad) fp16, w (Cout, cin_pad, k, k) fp32 holding fp16 values, wp, b fp32, res fp16 or None, relu)."""
  g = torch.Generator().manual_seed(_seed('num', case_id(c), regime))
  cp = cin_pad(c)
  Ho, Wo = out_hw(c)
  K = c.k * c.k * c.Cin
  x = torch.randn((c.N, c.H, c.W, cp), generator=g)
  w = torch.randn((c.Cout, cp, c.k, c.k), generator=g) * (2.0 / K) ** 0.5
  b = torch.randn((c.Cout,), generator=g) * 0.1
  res = torch.randn((c.N, Ho, Wo, c.Cout), generator=g) if num_uses_res(c, regime) else None
  relu = regime in ('relu', 'res_cancel')
  if regime == 'cancel':
    h = c.Cin // 2
    x = x.abs() + 0.1
    x[..., h:2 * h] = x[..., :h]
    w1 = w[:, :h].half().float()
    w[:, :h], w[:, h:2 * h] = w1, -w1 + 2e-3 * w1.abs()
    b = b * 0.1
  else:
    x = x.relu()
  if regime == 'wide':
    x[..., :c.Cin] *= _spread(g, c.Cin)
    t = _spread(g, c.Cout)
    w, b = w * t[:, None, None, None], b * t
  if regime == 'res_cancel':
    b = 3e4 + torch.randn((c.Cout,), generator=g) * 50
    res = -2.9e4 + res * 50
  x[..., c.Cin:], w[:, c.Cin:] = 0, 0
  w = w.half().float()
  return dict(x=x.half(), w=w, wp=pack_weight(w), b=b.float(), res=None if res is None else res.half(), relu=relu)


def _finish(pre, inp, dtype):
  """+ bias [+ residual] [ReLU] in dtype."""
  y = pre + inp['b'].to(dtype)
  if inp['res'] is not None:
    y = y + inp['res'].to(dtype)
  return torch.relu(y) if inp['relu'] else y


@torch.no_grad()
def num_ref(c, inp):
  """-> o, S (N, Ho, Wo, Cout) float64."""
  o = _finish(_conv(inp['x'], inp['w'], c, torch.float64), inp, torch.float64)
  S = _conv(inp['x'].abs(), inp['w'].abs(), c, torch.float64) + inp['b'].double().abs()
  if inp['res'] is not None:
    S = S + inp['res'].double().abs()
  return o, S


def num_tol(o, S, out_f32=False):
  acc = C_ACC * 2.0 ** -24 * S
  return 2.0 ** -23 * o.abs() + acc if out_f32 else 2.0 ** -11 * o.abs() + 2.0 ** -25 + acc


@functools.lru_cache(maxsize=2)
def num_case(c, regime):
  inp = num_inputs(c, regime)
  o, S = num_ref(c, inp)
  return dict(inp, o=o, S=S, tol=num_tol(o, S, out_f32=c.outs == (1,)))


@torch.no_grad()
def sim_conv2d(c, inp):
  """An honest fp32 accumulation, blocked: torch's float32 conv2d, bias, residual and ReLU in fp32; not rounded to the output type."""
  return _finish(_conv(inp['x'], inp['w'], c, torch.float32), inp, torch.float32).double()


def sim_chain(c, inp, n=N_CHAIN):
  """An honest fp32 accumulation, the longest chain: acc = fmaf(x_k, w_k, acc) over k = (ky, kx, channel) from 0, then bias, residual and ReLU
  in fp32, for n seeded output elements.  (A product of two fp16 values is exact in fp32, so fmaf is multiply, then add.)
  -> (index tuple of the elements, their values as float64)"""
  rs = np.random.RandomState(_seed('chain', case_id(c)))
  Ho, Wo = out_hw(c)
  pad = (c.k - 1) // 2
  ni, yo, xo, co = (rs.randint(0, m, size=n) for m in (c.N, Ho, Wo, c.Cout))
  yo[:4], xo[:4] = (0, 0, Ho - 1, Ho - 1), (0, Wo - 1, 0, Wo - 1)            # the corners among them
  xp = np.pad(inp['x'].float().numpy(), ((0, 0), (pad, pad), (pad, pad), (0, 0)))
  kk = np.arange(c.k)
  patch = xp[ni[:, None, None], (yo * c.stride)[:, None, None] + kk[None, :, None], (xo * c.stride)[:, None, None] + kk[None, None, :]]
  prod = (patch * inp['w'].permute(0, 2, 3, 1).numpy()[co]).reshape(n, -1).astype(np.float32)
  acc = np.zeros(n, dtype=np.float32)
  for k in range(prod.shape[1]):
    acc = acc + prod[:, k]
  acc = acc + inp['b'].numpy()[co]
  if inp['res'] is not None:
    acc = acc + inp['res'].float().numpy()[ni, yo, xo, co]
  if inp['relu']:
    acc = np.maximum(acc, np.float32(0))
  assert acc.dtype == np.float32
  return (ni, yo, xo, co), torch.from_numpy(acc.astype(np.float64))


def _r16(t):
  return t.half().double()


@torch.no_grad()
def num_mutant(c, inp, which):
  """A subtly wrong kernel, in float64 apart from its one fault.  which: 'chunk16' partial sums rounded to fp16 between 32-channel chunks,
  'res16' conv + bias rounded to fp16 before the residual add, 'ftz' fp16 subnormal outputs flushed to zero, 'res_after_relu'."""
  b, res = inp['b'].double(), None if inp['res'] is None else inp['res'].double()
  if which == 'chunk16':
    acc = 0
    for c0 in range(0, c.Cin, 32):
      acc = _r16(acc + _conv(inp['x'][..., c0:c0 + 32], inp['w'][:, c0:c0 + 32], c, torch.float64))
    return _finish(acc, inp, torch.float64)
  conv = _conv(inp['x'], inp['w'], c, torch.float64)
  pre = conv + b
  if which == 'res16':
    y = _r16(pre) + res
    return torch.relu(y) if inp['relu'] else y
  if which == 'res_after_relu':
    return torch.relu(pre) + res
  if which == 'ftz':
    y = _finish(conv, inp, torch.float64)
    return torch.where(y.abs() < F16_MIN_NORMAL, torch.zeros_like(y), y)
  raise ValueError(which)


def sim_ratios(c, regime):
  """max |sim - o| / (2^-24 S) of the two simulations."""
  d = num_case(c, regime)
  unit = 2.0 ** -24 * d['S']
  r1 = float(((sim_conv2d(c, d) - d['o']).abs() / unit).max())
  idx, v = sim_chain(c, d)
  r2 = float(((v - d['o'][idx]).abs() / unit[idx]).max())
  return r1, r2


if __name__ == '__main__':
  worst = {r: [0.0, 0.0] for r in REGIMES}
  for c, r in num_params():
    r1, r2 = sim_ratios(c, r)
    print(f'{case_id(c):40s} {r:10s} conv2d {r1:6.2f}  chain {r2:6.2f}')
    worst[r] = [max(worst[r][0], r1), max(worst[r][1], r2)]
  print({r: [round(v, 2) for v in w] for r, w in worst.items()})
