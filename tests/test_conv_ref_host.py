"""CPU checks behind tests/test_gpu_conv_numerics.py: the exact-integer inputs of tests/tools/conv_ref.py are what they claim to be and their
float32 reference is exact (part A); the float64 inputs are in the regime they name, an honest fp32 accumulation lies inside the per-element
bound everywhere, and each of four subtly wrong kernels lies outside it in the regime built for it (part B) - so a failure on the GPU is never a
property of the inputs, and a pass is never a property of the bound."""
import numpy as np
import pytest
import torch

from tests.tools import conv_ref as R

EXACT_IDS = [R.case_id(c) for c in R.EXACT_CASES]
NUM_PARAMS = R.num_params()
NUM_IDS = [f'{R.case_id(c)}-{r}' for c, r in NUM_PARAMS]


# ---- part A ----
@pytest.mark.parametrize('c', R.EXACT_CASES, ids=EXACT_IDS)
def test_exact_inputs_are_small_integers_and_the_float32_reference_is_exact(c):
  for variant in R.VARIANTS:
    d = R.exact_case(c, variant)
    x, w = d['x'].float(), d['w']
    cp, (Ho, Wo) = R.cin_pad(c), R.out_hw(c)
    assert d['x'].dtype == torch.float16 and x.shape == (c.N, c.H, c.W, cp) and d['res'].shape == d['conv'].shape == (c.N, Ho, Wo, c.Cout)
    zeros = float((x[..., :c.Cin] == 0).float().mean())
    if c.Cin < 8:                                                           # the stem: [-3, 3]; zero activations under garbage weights in the pad channels
      assert torch.equal(x, x.round()) and float(x.max()) == 3 and float(x.min()) == -3
      assert float(x[..., c.Cin:].abs().max()) == 0 and float(w[:, c.Cin:].abs().min()) >= 3
    else:
      assert torch.equal(x, x.round()) and float(x.max()) == 2 and float(x.min()) == -2
      assert zeros == 0 if variant == 'dense' else 0.45 < zeros < 0.55, zeros
    if variant == 'relu_like':
      assert zeros > 0.45
    assert set(w[:, :c.Cin].unique().tolist()) == {-1.0, 0.0, 1.0}
    for t in (d['b'], d['res'].float()):
      assert float(t.abs().max()) <= 8 and torch.equal(t, t.round())
    kraw = c.k * c.k * cp
    assert d['wp'].shape == (c.Cout, (kraw + 31) // 32 * 32) and float(d['wp'][:, kraw:].abs().sum()) == 0
    assert torch.equal(d['wp'][:, :cp].float(), w[:, :, 0, 0])               # k index = (ky, kx, channel)
    if c.k > 1:
      assert torch.equal(d['wp'][:, cp:2 * cp].float(), w[:, :, 0, 1]) and torch.equal(d['wp'][:, c.k * cp:(c.k + 1) * cp].float(), w[:, :, 1, 0])
    # exact: float32 == float64, and whatever is rounded to fp16 is at most 2048
    ref64 = R._conv(d['x'], w, c, torch.float64) + d['b'].double()
    assert torch.equal(d['conv'].double(), ref64), f'{variant}: the float32 reference differs from float64'
    biggest = max(float(ref64.abs().max()), float((ref64 + d['res'].double()).abs().max()))
    assert biggest <= R.EXACT_LIMIT, f'{variant}: max |value| {biggest}'
    got = R.exact_expected(d, True, True)                                    # (the expected outputs: the same integers, exact in fp16)
    assert torch.equal(got.double(), torch.relu(ref64 + d['res'].double())) and torch.equal(got.half().float(), got)
    got = R.exact_expected(d, False, False)
    assert got is d['conv'] and torch.equal(got.half().float(), got)


def test_exact_cases_are_the_listed_ones_and_seeded():
  forms = {c.form for c in R.EXACT_CASES}
  assert {'small<1,40,1>', 'small<2,40,1>', 'small<4,20,1>', 'small<2,40,2>', 'small<1,80,2,4>', 'halo-splitk', 'halo-tail1', 'halo-tail2',
          'halo-tail3', 'halo-tail4', 'halo-round', 's1b', 's2', 's2-splitk', 'stem', 'igemm2<128,3>', 'igemm2<64,3>',
          'igemm2<64,7,CIN8>', 'igemm2<128,7,CIN8>', 'igemm2<128,1>', 'igemm2<64,1>'} == forms
  assert len(set(EXACT_IDS)) == len(EXACT_IDS)
  assert {c.form for c in R.NUM_CASES} >= {f for f in forms if f.startswith(('small', 's1b', 's2', 'stem'))}
  c = R.EXACT_CASES[0]
  a, b = R.exact_case(c, 'dense'), R.exact_case.__wrapped__(c, 'dense')
  assert torch.equal(a['x'], b['x']) and torch.equal(a['wp'], b['wp']) and not torch.equal(a['x'], R.exact_case(c, 'relu_like')['x'])
  got = a['conv'].clone()
  assert R.first_mismatch(got, a['conv']) == ''
  got[0, 3, 5, 7] += 1
  got[0, 9, 0, 0] = float('nan')
  msg = R.first_mismatch(got, a['conv'])
  assert msg.startswith('2 of ') and '(image 0, row 3, column 5, channel 7)' in msg, msg


def _model_form(c, out_f32, use_res, num_cu=256):
  """The dispatch of fp_conv2d_f16 / launch_conv restated (csrc/api.hip, conv.hip, conv_small.hip, conv_halo.hip) for a stand-alone call."""
  Ho, Wo = R.out_hw(c)
  M, cp, pad = c.N * Ho * Wo, R.cin_pad(c), (c.k - 1) // 2
  Kpad = (c.k * c.k * cp + 31) // 32 * 32
  sq = c.H == c.W
  if c.k == 3 and pad == 1 and sq and not out_f32 and c.Cout % 32 == 0 and Kpad == 9 * cp:
    s1 = c.stride == 1 and ((c.W == 40 and cp in (128, 256)) or (c.W == 20 and cp == 512))
    s2 = c.stride == 2 and ((c.W == 40 and cp == 256) or (c.W == 80 and cp == 64))
    if (s1 or s2) and -(-M // 32) * (c.Cout // 32) <= 2 * num_cu:
      return 'small<%s>' % {(128, 1): '1,40,1', (256, 1): '2,40,1', (512, 1): '4,20,1', (256, 2): '2,40,2', (64, 2): '1,80,2,4'}[(cp, c.stride)]
  halo = c.k == 3 and c.stride == 1 and sq and c.W in (40, 20) and cp % 32 == 0 and c.Cout % 128 == 0 and not out_f32
  if halo:
    n_ct, qm = c.Cout // 128, -(-M // 128)
    if qm * n_ct * 4 <= num_cu and cp // 32 >= 8:
      return 'halo-splitk'
    per_round = (num_cu // n_ct) * 4
    full, rem = divmod(qm, per_round)
    if full:
      return 'halo-round'
    cost = {nt: -(-(-(-rem // nt) * n_ct) // num_cu) * (0.0, 0.43, 0.62, 0.81, 1.0)[nt] for nt in (4, 3, 2, 1)}
    best = 4
    for nt in (3, 2, 1):
      if cost[nt] < cost[best] - 1e-9:
        best = nt
    return f'halo-tail{best}'
  nk = Kpad // 32
  if c.k == 3 and c.stride == 2 and not out_f32 and cp % 32 == 0 and c.Cout % 128 == 0 and M < 2000 and nk >= 36 and nk % 4 == 0 and \
     -(-M // 64) * (c.Cout // 128) * 4 <= 2 * num_cu:
    return 's2-splitk'
  if c.k == 3 and c.stride == 2 and not out_f32 and not use_res and sq and Ho == Wo == 20 and c.H == 40 and M >= 2000 and c.Cout % 128 == 0:
    return 's2'
  if c.k == 7 and c.stride == 2 and cp == 8 and c.Cout == 64 and not out_f32 and not use_res and Ho % 16 == 0 and Wo % 16 == 0 and \
     c.H == 2 * Ho and c.W == 2 * Wo:
    return 'stem'
  return 'igemm2<%d,%d%s>' % (128 if c.Cout % 128 == 0 else 64, c.k, ',CIN8' if cp == 8 else '')


@pytest.mark.parametrize('c', [c for c in R.EXACT_CASES if c.entry == 'conv2d'], ids=[R.case_id(c) for c in R.EXACT_CASES if c.entry == 'conv2d'])
def test_each_case_reaches_the_form_it_names_on_256_cus(c):
  """By the dispatch conditions of the sources, restated above: without a residual every case runs the form in its name, with one every form
  that adds a residual itself does, and the fp32 output of every halo shape runs the generic kernel."""
  assert _model_form(c, 0, False) == c.form
  assert _model_form(c, 0, True) == (c.form if c.takes_res else 'igemm2<%d,%d%s>' % (128 if c.Cout % 128 == 0 else 64, c.k, ',CIN8' if c.Cin < 8 else ''))
  if 1 in c.outs:
    assert _model_form(c, 1, False).startswith('igemm2<')
  if c.form.startswith('halo'):
    assert c.outs == (0, 1) and _model_form(c, 1, True) == 'igemm2<128,3>'
  if c.form == 'small<1,40,1>' and c.N == 2:                               # the largest launch conv_small takes: one image more runs another form
    assert not _model_form(c._replace(N=3), 0, False).startswith('small')


# ---- part B ----
def _outside(y, d):
  return bool(((y - d['o']).abs() > d['tol']).any())


@pytest.mark.parametrize('c,regime', NUM_PARAMS, ids=NUM_IDS)
def test_regime_bound_and_mutants(c, regime):
  d = R.num_case(c, regime)
  o, S, tol = d['o'], d['S'], d['tol']
  what = f'{R.case_id(c)} {regime}'
  cp = R.cin_pad(c)
  assert d['x'].dtype == torch.float16 and torch.equal(d['w'], d['w'].half().float()) and d['wp'].shape[0] == c.Cout
  assert float(d['x'][..., c.Cin:].abs().max() if cp > c.Cin else 0) == 0
  assert float(o.abs().max()) <= 6e4 and bool(torch.isfinite(o).all()) and bool((S >= o.abs() * (1 - 1e-12)).all()) and bool((tol > 0).all()), what
  assert (d['res'] is not None) == R.num_uses_res(c, regime)
  # an honest fp32 accumulation lies inside the bound, everywhere (rounded to the output type, as a kernel would)
  out_f32 = c.outs == (1,)
  sim = R.sim_conv2d(c, d)
  sim_out = sim.float().double() if out_f32 else sim.half().double()
  ratio = float(((sim_out - o).abs() / tol).max())
  assert ratio <= 1.0, f'{what}: float32 conv2d at {ratio:.3f} of the bound'
  idx, chain = R.sim_chain(c, d)
  chain_out = chain.float().double() if out_f32 else chain.half().double()
  ratio = float(((chain_out - o[idx]).abs() / tol[idx]).max())
  assert ratio <= 1.0, f'{what}: fmaf chain at {ratio:.3f} of the bound'
  unit = 2.0 ** -24 * S
  acc = max(float(((sim - o).abs() / unit).max()), float(((chain - o[idx]).abs() / unit[idx]).max()))
  assert 2 * acc <= R.C_ACC, f'{what}: accumulation error {acc:.2f} x 2^-24 S, more than half of C_ACC = {R.C_ACC}'
  # the regime, and the mutant it is built for
  if regime == 'relu':
    assert 0.3 < float((d['x'][..., :c.Cin] == 0).float().mean()) < 0.7 and d['relu']
    if d['res'] is not None:
      assert _outside(R.num_mutant(c, d, 'res_after_relu'), d), f'{what}: the residual after the ReLU passes'
  elif regime == 'wide':
    a = o.abs()
    sub = float(((a > 0) & (a < R.F16_MIN_NORMAL)).double().mean())
    assert sub >= R.WIDE_SUBNORMAL_SHARE, f'{what}: {sub:.4f} of the outputs are fp16 subnormals'
    assert float(torch.log2(a.max() / a[a > 0].min())) >= 20
    xs, ws = d['x'].float().abs(), d['w'].abs()
    assert float(((xs > 0) & (xs < R.F16_MIN_NORMAL)).float().mean()) > 0.01 and float(((ws > 0) & (ws < R.F16_MIN_NORMAL)).float().mean()) > 0.01
    assert _outside(R.num_mutant(c, d, 'ftz'), d), f'{what}: flushing subnormal outputs passes'
  elif regime == 'cancel':
    rel = (o.abs() / S).median()
    assert 3e-4 < float(rel) < 3e-3, f'{what}: |o| / S = {float(rel):.2e}'
    h = c.Cin // 2
    assert torch.equal(d['x'][..., :h], d['x'][..., h:2 * h]) and float(d['x'][..., :c.Cin].min()) > 0
    if c.Cin >= 64:                                                         # (one chunk of 32 channels: nothing is handed on)
      assert _outside(R.num_mutant(c, d, 'chunk16'), d), f'{what}: fp16 partial sums between chunks pass'
  else:
    pre = o - d['res'].double()
    assert 2.9e4 < float(pre.median()) < 3.1e4 and -3.0e4 < float(d['res'].float().median()) < -2.8e4 and 500 < float(o.median()) < 1500, what
    mut = R.num_mutant(c, d, 'res16')
    assert _outside(mut, d) and float((mut - o).abs().max()) > 4 and float(tol.max()) < 1.5, f'{what}: rounding before the residual add passes'


def test_bound_constants_and_cases():
  assert R.C_ACC == 62 and R.WIDE_SUBNORMAL_SHARE == 0.03 and R.REGIMES == ('relu', 'wide', 'cancel', 'res_cancel')
  assert len(NUM_PARAMS) == 4 * len(R.NUM_CASES) - sum(not c.takes_res for c in R.NUM_CASES)
  o, S = torch.tensor([1000.0, 0.0]).double(), torch.tensor([6e4, 1.0]).double()
  t16, t32 = R.num_tol(o, S), R.num_tol(o, S, out_f32=True)
  assert abs(float(t16[0]) - (1000 / 2048 + 2.0 ** -25 + 62 * 6e4 / 2 ** 24)) < 1e-12 and abs(float(t32[1]) - 62 / 2 ** 24) < 1e-15
  a, b = R.num_inputs(R.NUM_CASES[0], 'cancel'), R.num_inputs(R.NUM_CASES[0], 'cancel')
  assert torch.equal(a['x'], b['x']) and torch.equal(a['wp'], b['wp'])
