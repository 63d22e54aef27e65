"""The transformer heads' kernels against float64 references at the inputs their older tests never draw: the attention core (csrc/attn.hip:
attention_kernel and the split-K attention_small_kernel) with peaked, ascending, far-below-zero and uniform softmaxes at token counts that
end in nearly empty key and query blocks; the LayerNorm epilogues of the token Linear (csrc/tok_gemm.hip) and both forms of the fused head MLP
(csrc/head_mlp.hip) at rows whose mean is up to 64 standard deviations from zero and at rows whose variance is the LayerNorm epsilon.
References, inputs and bounds: tests/tools/heads_ref.py; that the inputs are what they claim to be is checked on the CPU by
tests/test_heads_ref_host.py.  Every output buffer is NaN-prefilled."""
import numpy as np
import pytest
import torch

from tests.tools import heads_ref as R

pytestmark = pytest.mark.gpu

ATT_IDS = [f'{r}-{T}' for r, T in R.att_cases()]
PERSISTENT = [(r, B, T) for r in R.PERSISTENT_REGIMES for B, T in R.PERSISTENT_SHAPES]


@pytest.fixture(scope='module')
def ctx():
  from foundationpose_amd import _lib
  return _lib.Context.get('cuda:0')


def run_attention(ctx, qk_d, vt_d, B, T):
  from foundationpose_amd._lib import check, lib, ptr, stream_ptr
  out = torch.full((B * T, 512), float('nan'), dtype=torch.float16, device='cuda')
  check(lib().fp_attention_f16(ctx.handle, ptr(qk_d), ptr(vt_d), B, T, ptr(out), stream_ptr()))
  torch.cuda.synchronize()
  return out


def worst_ratio(got16, o, tol, what):
  got = got16.cpu().numpy().astype(np.float64)
  assert not np.isnan(got).any(), f'{what}: NaN in the output'
  ratio = np.abs(got - o) / tol
  i = np.unravel_index(np.argmax(ratio), ratio.shape)
  line = f'{what}: max |err| / tol {ratio[i]:.3f} (row {i[0]}, column {i[1]}: got {got[i]:.6f}, reference {o[i]:.6f}, tol {tol[i]:.2e})'
  print(line)
  assert ratio[i] <= 1.0, line
  return float(ratio[i])


@pytest.mark.parametrize('regime,T', R.att_cases(), ids=ATT_IDS)
def test_attention_against_float64(ctx, regime, T):
  """|got - o| <= tol for every output element, tol the per-element bound of tests/tools/heads_ref.py (fp16 rounding of P and of the output,
  fp32 accumulation of a score, P below fp16's subnormals), from the float64 reference alone.  Hypotheses 0 (B = 1) and 1-2 (B = 2) through
  the split-K form, all three (B = 3) through the flash form.  uniform: also every query of a (hypothesis, head) gives the same bits.
  Prints the largest |err| / tol per case and form (pytest -s).  No MI355X figures are recorded here yet: the table of the largest ratio per
  regime belongs in this docstring once the test has run on one."""
  c = R.attention_case(regime, R.ATT_B, T)
  qk_d, vt_d = c['qk'].cuda(), c['vt'].cuda()
  for form, b0, nb in (('split-K', 0, 1), ('split-K', 1, 2), ('flash', 0, 3)):
    got = run_attention(ctx, qk_d[b0 * T:], vt_d[b0:], nb, T)
    rows = slice(b0 * T, (b0 + nb) * T)
    worst_ratio(got, c['o'][rows], c['tol'][rows], f'attention {regime} T={T} B={nb} ({form})')
    if regime == 'uniform':
      per_head = got.view(torch.int16).reshape(nb, T, 4, 128)
      n_diff = int((per_head != per_head[:, :1]).sum())
      assert n_diff == 0, f'uniform T={T} B={nb} ({form}): {n_diff} of {per_head.numel()} outputs differ from query 0 of their head'


@pytest.mark.parametrize('regime,B,T', PERSISTENT, ids=[f'{r}-{B}x{T}' for r, B, T in PERSISTENT])
def test_attention_persistent_walk_against_float64(ctx, regime, B, T):
  """More items than CUs - (70, 400): 560 items of seven key blocks, (130, 65): 520 items of two (KB0, then the tail with one key) - in the
  regimes that take the rescale-skip branch always (early_peak), never (ascending) or start far below zero (offset_neg): the same bound,
  and the batch equals launches of at most 256 items (one item per workgroup) bit for bit.
  Prints the largest |err| / tol per case.  No MI355X figures are recorded here yet."""
  c = R.attention_case(regime, B, T)
  qk_d, vt_d = c['qk'].cuda(), c['vt'].cuda()
  out = run_attention(ctx, qk_d, vt_d, B, T)
  worst_ratio(out, c['o'], c['tol'], f'attention walk {regime} {B}x{T}')
  nqb = -(-T // 224)
  step = max(3, 256 // (4 * nqb))
  while 0 < B % step <= 2:                # (launches of one or two hypotheses take the split-K form of a tracking frame: not this kernel)
    step -= 1
  single = torch.cat([run_attention(ctx, qk_d[b0 * T:], vt_d[b0:], min(step, B - b0), T) for b0 in range(0, B, step)])
  assert not bool(torch.isnan(single).any())
  assert torch.equal(out, single)


def _outside(other, ref, tol):
  return float((other - ref).abs().max()) > tol


@pytest.mark.parametrize('n_hyp', [1, 3])
@pytest.mark.parametrize('regime', R.LN_REGIMES)
def test_token_linear_layernorm_against_float64(ctx, regime, n_hyp):
  """Epilogues 2 (LayerNorm rows, fp16) and 3 (sums of the normalised rows over groups of 16 tokens, fp32) of fp_token_linear_f16 at
  tolerances of test_token_linear_epilogues_vs_fp32_reference: 2.5e-3 max |ref|, and 2e-4 max |ref| + 1e-4.  eps: a reference with eps =
  1e-6, and one with eps outside the square root, lie outside those tolerances - the test sees the epsilon.
  Prints both errors beside their tolerances per case.  No MI355X figures are recorded here yet."""
  from foundationpose_amd._lib import check, lib, ptr, stream_ptr
  inp = R.token_linear_inputs(regime, n_hyp)
  M = 400 * n_hyp
  ln, gs, _ = R.layernorm_ref(inp)
  x_d, res_d = inp['x'].cuda(), inp['res'].cuda()

  def run(epi, out, affine):
    check(lib().fp_token_linear_f16(ctx.handle, ptr(x_d), M, ptr(inp['w'].numpy()), ptr(inp['b'].numpy()), epi, 0, ptr(res_d),
                                    ptr(inp['gam'].numpy()) if affine else None, ptr(inp['bet'].numpy()) if affine else None, 400, ptr(out), stream_ptr()))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()), f'epilogue {epi}: NaN in the output'
    return out.double().cpu()
  rows = run(2, torch.full((M, 512), float('nan'), dtype=torch.float16, device='cuda'), True)
  sums = run(3, torch.full((M // 16, 512), float('nan'), dtype=torch.float32, device='cuda'), False)
  tol2, tol3 = 2.5e-3 * float(ln.abs().max()), 2e-4 * float(gs.abs().max()) + 1e-4
  e2, e3 = float((rows - ln).abs().max()), float((sums - gs).abs().max())
  line = f'token linear {regime} n={n_hyp}: rows {e2:.2e} (tol {tol2:.2e}), sums {e3:.2e} (tol {tol3:.2e}), max |ref| {float(ln.abs().max()):.2f} / {float(gs.abs().max()):.2f}'
  print(line)
  assert e2 <= tol2 and e3 <= tol3, line
  if regime == 'eps':
    for kw in (dict(eps=1e-6), dict(eps_outside=True)):
      ln_o, gs_o, _ = R.layernorm_ref(inp, **kw)
      assert _outside(ln_o, ln, tol2) and _outside(gs_o, gs, tol3), kw
      assert _outside(ln_o, rows, tol2) and _outside(gs_o, sums, tol3), kw


@pytest.mark.parametrize('n_hyp', [1, 3, 5, 7])
@pytest.mark.parametrize('regime', R.LN_REGIMES)
def test_head_mlp_against_float64(ctx, regime, n_hyp):
  """fp_head_mlp_f16 at the project's tolerance 2.5e-3 max |ref| + 1e-3: 1 and 3 hypotheses run head_mlp_kernel (two-pass LayerNorm
  variance), 5 and 7 head_mlp128_kernel (one pass: E[x^2] - mean^2 in fp32, whose relative error grows with (mean / sigma)^2).  eps: as above.
  Prints max |got - ref| / max |ref| per form and regime: the table that shows how the one-pass form degrades from centred to shift64 beside
  the two-pass form.  No MI355X figures are recorded here yet; a float32 simulation of the one-pass formula on the CPU puts its relative
  error in rstd at 1e-5 / 1.1e-4 / 1.7e-3 for mean / sigma = 4 / 16 / 64, inside the tolerance."""
  from foundationpose_amd._lib import check, lib, ptr, stream_ptr
  inp = R.head_mlp_inputs(regime, n_hyp)
  M = 400 * n_hyp
  ref, _, _ = R.head_mlp_ref(inp)
  att_d, tok_d = inp['att'].cuda(), inp['tok'].cuda()
  out = torch.full((M // 16, 512), float('nan'), dtype=torch.float32, device='cuda')
  args = [ptr(inp[k].numpy()) for k in ('w_out', 'b_out', 'g1', 'be1', 'w1', 'b1', 'w2', 'b2')]
  check(lib().fp_head_mlp_f16(ctx.handle, ptr(att_d), ptr(tok_d), M, *args, ptr(out), stream_ptr()))
  torch.cuda.synchronize()
  assert not bool(torch.isnan(out).any())
  got = out.double().cpu()
  scale = float(ref.abs().max())
  err, tol = float((got - ref).abs().max()), 2.5e-3 * scale + 1e-3
  line = f'head MLP {"64" if M <= 1600 else "128"}-token form {regime} n={n_hyp}: max |got - ref| / max |ref| = {err / scale:.2e} (max |ref| {scale:.2f}, tol {tol / scale:.2e})'
  print(line)
  assert err <= tol, line
  if regime == 'eps':
    for kw in (dict(eps=1e-6), dict(eps_outside=True)):
      other, _, _ = R.head_mlp_ref(inp, **kw)
      assert _outside(other, ref, tol) and _outside(other, got, tol), kw
