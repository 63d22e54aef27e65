"""CPU checks behind tests/test_gpu_heads_numerics.py: the float64 references of tests/tools/heads_ref.py are the textbook operations (Check A),
and every input set the GPU tests use is in the regime it names and keeps the conditions under which the bounds hold (Check B) - so a failure
on the GPU is never a property of the inputs."""
import math

import numpy as np
import pytest
import torch

from tests.tools import heads_ref as R

ATT_IDS = [f'{r}-{T}' for r, T in R.att_cases()]
PERSISTENT = [(r, B, T) for r in R.PERSISTENT_REGIMES for B, T in R.PERSISTENT_SHAPES]


# ---- Check A: the references ----
@pytest.mark.parametrize('regime', ['soft', 'last_key', 'offset_neg'])
def test_attention_ref_is_scaled_dot_product_attention(regime):
  B, T = 2, 65
  inp = R.attention_inputs(regime, B, T)
  o, s_abs, qk_abs = R.attention_ref(inp['qk'], inp['v'], B, T)
  q, k = R.split_qk(inp['qk'], B, T)
  want = torch.nn.functional.scaled_dot_product_attention(q, k, inp['v'].double())
  assert float((o - want.transpose(1, 2).reshape(B * T, 512)).abs().max()) <= 1e-12
  assert qk_abs.shape == (B, 4, T, T) and float((qk_abs[1, 2, 3, 5] - (q[1, 2, 3] * k[1, 2, 5]).abs().sum()).abs()) <= 1e-12
  assert bool((s_abs >= o.abs() - 1e-12).all())
  # the V image: token t of the rows in column vt_col(t), zeros behind
  col = R.vt_col(np.arange(T))
  assert sorted(col[:64]) == list(range(64)) and list(col[:16]) == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]
  assert torch.equal(inp['vt'][1, 2, :, col[37]], inp['v'][1, 2, 37]) and float(inp['vt'][..., 80:].abs().max()) == 0
  assert torch.equal(inp['qk'][T + 3, 512 + 2 * 128:512 + 3 * 128].double(), k[1, 2, 3])


@pytest.mark.parametrize('regime', R.LN_REGIMES)
def test_layernorm_ref_is_layer_norm(regime):
  inp = R.token_linear_inputs(regime, 1)
  ln, gs, y = R.layernorm_ref(inp)
  want = torch.nn.functional.layer_norm(y, (512,), inp['gam'].double(), inp['bet'].double(), 1e-5)
  assert float((ln - want).abs().max()) <= 1e-12
  nrm = torch.nn.functional.layer_norm(y, (512,), None, None, 1e-5)
  assert float((gs - nrm.reshape(25, 16, 512).sum(1)).abs().max()) <= 1e-12
  assert float((y - (inp['res'].double() + torch.nn.functional.linear(inp['x'].double(), inp['w'].double(), inp['b'].double()))).abs().max()) <= 1e-12
  assert inp['x'].dtype == torch.float16 and torch.equal(inp['w'], inp['w'].half().float())


@pytest.mark.parametrize('regime', R.LN_REGIMES)
def test_head_mlp_ref_is_a_post_norm_encoder_layer_tail(regime):
  """Without its two fp16 roundings: x = norm1(tok + out_proj(att)); x = norm2(x + linear2(relu(linear1(x)))), norm2 without affine
  parameters, summed over groups of 16 tokens - nn.TransformerEncoderLayer (norm_first=False) behind its attention core."""
  F = torch.nn.functional
  inp = R.head_mlp_inputs(regime, 1)
  d = {k: v.double() for k, v in inp.items()}
  x = F.layer_norm(d['tok'] + F.linear(d['att'], d['w_out'], d['b_out']), (512,), d['g1'], d['be1'], 1e-5)
  x = F.layer_norm(x + F.linear(F.relu(F.linear(x, d['w1'], d['b1'])), d['w2'], d['b2']), (512,), None, None, 1e-5)
  got, _, _ = R.head_mlp_ref(inp, round16=False)
  assert float((got - x.reshape(25, 16, 512).sum(1)).abs().max()) <= 1e-10 * max(1.0, float(got.abs().max()))
  rounded, _, _ = R.head_mlp_ref(inp)
  assert 0 < float((rounded - got).abs().max()) <= 2.5e-3 * float(got.abs().max()) + 1e-3          # (the roundings are there, and small)


# ---- Check B: the attention inputs ----
def _check_regime(regime, B, T, c):
  s = R.scaled_logits(c['qk'], B, T)                                      # (B, 4, T, T)
  nkb = -(-T // 64)
  what = f'{regime} {B}x{T}'
  if regime in ('early_peak', 'last_key', 'wave_alone'):
    top = torch.topk(s, 2, dim=-1) if T > 1 else None
    margin = top.values[..., 0] - top.values[..., 1]
    assert float(margin.min()) >= 30, f'{what}: margin {float(margin.min()):.1f}'
    win = top.indices[..., 0]
    if regime == 'early_peak':
      assert int(win.max()) < 64, what
      if T >= 128:                                                          # no running maximum moves after key block 0
        assert bool((s[..., :64].max(-1).values > s[..., 64:].max(-1).values + 30).all()), what
      assert len(torch.unique(win[0, 0])) == min(8, T)                      # (and the queries of a head do not share one winner)
    elif regime == 'last_key':
      assert bool((win == T - 1).all()), what
    else:
      assert T >= 128 and bool((win // 64 == (torch.arange(T) % nkb)).all()), what
      assert sorted(torch.unique(win // 64).tolist()) == list(range(nkb))
  elif regime == 'ascending':
    bmax = torch.stack([s[..., g * 64:(g + 1) * 64].max(-1).values for g in range(nkb)], -1)
    if nkb > 1:
      step = bmax[..., 1:] - bmax[..., :-1]
      assert float(step.min()) > 0, f'{what}: a block maximum does not move'
      full = step[..., :-1] if T % 64 else step                            # (a tail block of a few keys has a lower maximum of its noise)
      if full.numel():
        assert 8 < float(full.mean()) < 12, f'{what}: mean step {float(full.mean()):.2f}'
    noise = s[..., :min(64, T)].std(-1)
    assert 0.8 < float(noise.mean()) < 1.25, f'{what}: noise inside a block {float(noise.mean()):.2f}'
  elif regime == 'offset_neg':
    assert float(s.max()) < -40 and float(s.min()) > -80, f'{what}: logits in [{float(s.min()):.1f}, {float(s.max()):.1f}]'
    assert float(torch.softmax(s, -1).max(-1).values.median()) < 0.5       # (soft underneath)
  elif regime == 'uniform':
    assert float((s - s[..., :1]).abs().max()) == 0.0, what
    assert float((s - s[..., :1, :]).abs().max()) == 0.0 and float(s.abs().min()) > 0.01, what          # one score per head, not zero
    q, _ = R.split_qk(c['qk'], B, T)
    assert T == 1 or float((q[:, :, 1:] - q[:, :, :1]).abs().amax(-1).min()) > 0                        # yet no two queries alike
    p = torch.softmax(s, -1)
    assert float((p - 1.0 / T).abs().max()) <= 1e-15
    vmean = c['v'].double().mean(2, keepdim=True).expand(B, 4, T, 128).transpose(1, 2).reshape(B * T, 512)
    assert float(np.abs(c['o'] - vmean.numpy()).max()) <= 1e-14
  else:
    pm = torch.softmax(s, -1).max(-1).values
    assert float(s.max()) > 0 and (T < 64 or 1.5 / T < float(pm.median()) < 0.9), what
  # the conditions of the bound
  qmax = float(c['qk_abs_max'].max())
  assert qmax <= 2000, f'{what}: sum |q k| up to {qmax:.0f}'
  if regime != 'uniform':
    term1, term3 = 2.0 ** -11 * c['s_abs'], R.SCORE_TERM * c['qk_abs_max'] * c['s_abs']
    assert bool((term3 <= term1).all()) and qmax <= R.QK_ABS_LIMIT, f'{what}: sum |q k| up to {qmax:.0f}: the score term exceeds the P-rounding term'
  assert bool((c['tol'] > 0).all()) and np.isfinite(c['tol']).all() and np.isfinite(c['o']).all()
  assert float(c['tol'].max()) <= 5e-3 * max(1.0, c['vmax'])               # (and the bound is not vacuous)


@pytest.mark.parametrize('regime,T', R.att_cases(), ids=ATT_IDS)
def test_attention_inputs_are_in_their_regime(regime, T):
  _check_regime(regime, R.ATT_B, T, R.attention_case(regime, R.ATT_B, T))


@pytest.mark.parametrize('regime,B,T', PERSISTENT, ids=[f'{r}-{B}x{T}' for r, B, T in PERSISTENT])
def test_persistent_inputs_are_in_their_regime(regime, B, T):
  c = R.attention_case(regime, B, T)
  for b0 in range(0, B, 10):                                                # (the logits ten hypotheses at a time)
    nb = min(10, B - b0)
    part = dict(qk=c['qk'][b0 * T:(b0 + nb) * T], v=c['v'][b0:b0 + nb], vmax=c['vmax'],
                **{k: c[k][b0 * T:(b0 + nb) * T] for k in ('o', 's_abs', 'qk_abs_max', 'tol')})
    _check_regime(regime, nb, T, part)


def test_attention_cases_cover_the_kernels_edges():
  cases = R.att_cases()
  assert set(R.ATT_T) == {400, 399, 225, 224, 65, 64, 37} and set(R.ATT_REGIMES) == {r for r, _ in cases}
  assert {T for r, T in cases if r == 'wave_alone'} == {400, 399, 225, 224}
  assert len(cases) == 6 * 7 + 4
  assert abs(R.PEAK_A * R.PEAK_B * math.sqrt(128) - 40) < 0.1 and abs(R.QK_ABS_LIMIT - 2 ** 13 / math.sqrt(128)) < 1e-9
  a, b = R.attention_inputs('ascending', 2, 65), R.attention_inputs('ascending', 2, 65)
  assert torch.equal(a['qk'], b['qk']) and torch.equal(a['vt'], b['vt']) and a['qk'].dtype == torch.float16
  assert not torch.equal(a['qk'][:65], a['qk'][65:])


# ---- Check B: the LayerNorm inputs ----
def _check_ln_rows(regime, y, what):
  ratio, var = R.row_stats(y)
  if regime == 'centred':
    assert np.median(ratio) < 1 and 1 < np.median(var) < 10, what
  elif regime == 'eps':
    assert ((var >= 2e-6) & (var <= 2e-5)).mean() >= 0.9, f'{what}: variance {var.min():.2e} .. {var.max():.2e}'
    assert np.median(ratio) < 1, what
  else:
    r = int(regime[5:])
    assert (ratio >= r / 2).mean() >= 0.5, f'{what}: only {(ratio >= r / 2).mean():.3f} of the rows at |mean| / sigma >= {r / 2}'
    assert ratio.max() <= 1.25 * r and 0.5 < np.median(var) < 2.5, f'{what}: ratio up to {ratio.max():.1f}, variance {np.median(var):.2f}'


@pytest.mark.parametrize('regime', R.LN_REGIMES)
def test_layernorm_inputs_are_in_their_regime(regime):
  for n_hyp in (1, 3):
    inp = R.token_linear_inputs(regime, n_hyp)
    _, _, y = R.layernorm_ref(inp)
    _check_ln_rows(regime, y, f'token linear {regime} n={n_hyp}')
    if regime == 'eps':                                                     # a 512-term dot product of them stays clear of fp16's subnormals
      assert float(inp['x'].abs().median()) > 1e-3 and float(inp['w'].abs().median()) > 1e-3
    if regime.startswith('shift'):
      r = int(regime[5:])
      mean = y.mean(-1)
      assert float(mean.min()) < -0.9 * r and float(mean.max()) > 0.9 * r   # both signs, out to r sigma
  for n_hyp in (1, 3, 5, 7):
    inp = R.head_mlp_inputs(regime, n_hyp)
    _, y1, y2 = R.head_mlp_ref(inp)
    _check_ln_rows(regime, y1, f'head MLP LayerNorm1 {regime} n={n_hyp}')
    _check_ln_rows(regime, y2, f'head MLP LayerNorm2 {regime} n={n_hyp}')


@pytest.mark.parametrize('n_hyp', [1, 5])
def test_the_eps_regime_sees_the_epsilon(n_hyp):
  """With a variance of ~ 1e-5 a reference with eps = 1e-6, and one with eps added outside the square root, lie far outside the
  tolerances the GPU tests assert against the true one (the GPU tests assert this again for each of their cases)."""
  inp = R.token_linear_inputs('eps', 1)
  ln, gs, _ = R.layernorm_ref(inp)
  for kw in (dict(eps=1e-6), dict(eps_outside=True)):
    ln2, gs2, _ = R.layernorm_ref(inp, **kw)
    assert float((ln2 - ln).abs().max()) > 20 * 2.5e-3 * float(ln.abs().max())
    assert float((gs2 - gs).abs().max()) > 20 * (2e-4 * float(gs.abs().max()) + 1e-4)
  inp = R.head_mlp_inputs('eps', n_hyp)
  ref, _, _ = R.head_mlp_ref(inp)
  for kw in (dict(eps=1e-6), dict(eps_outside=True)):
    other, _, _ = R.head_mlp_ref(inp, **kw)
    assert float((other - ref).abs().max()) > 20 * (2.5e-3 * float(ref.abs().max()) + 1e-3)
