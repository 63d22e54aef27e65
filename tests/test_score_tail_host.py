"""CPU checks behind tests/test_gpu_score_tail.py: the two float64 references of the ScoreNet tail agree with each other where they must
(Check A), and every input set the GPU tests use is in the regime they name and leaves the bounds they assert attainable (Check B) - so a
failure on the GPU is never a property of the inputs."""
import numpy as np
import pytest

from tests.tools import score_tail_ref as R

CASE_IDS = [f'{g}x{L}-{r}' for g, L, r in R.CASES]


@pytest.mark.parametrize('groups,L,regime', R.CASES, ids=CASE_IDS)
def test_folded_value_path_equals_the_textbook_form(groups, L, regime):
  """Check A: without the float32 rounding of q and k, the folded form (four scalars per row, make_score_tail's algebra) is the textbook
  att_cross + linear up to float64 rounding: 1e-12 of the largest logit."""
  for tail in R.TAILS:
    c = R.case_refs(groups, L, regime, tail)
    emu, p = R.tail_emulation(R.tail_sd(tail), c['feats'], L, round_qk=False)
    _, p_ref = R.tail_reference(R.tail_sd(tail), c['feats'], L)
    err = float(np.abs(emu - c['ref']).max())
    assert err <= 1e-12 * np.abs(c['ref']).max(), f'tail {tail}: folded form off by {err:.2e}'
    np.testing.assert_allclose(p, p_ref, rtol=0, atol=1e-13)
    np.testing.assert_allclose(p_ref.sum(-1), 1.0, rtol=0, atol=1e-13)


@pytest.mark.parametrize('groups,L,regime', R.CASES, ids=CASE_IDS)
def test_inputs_are_in_their_regime(groups, L, regime):
  """Check B, on the reference alone.  Softmax windows: soft - the median over (query, head) of the largest weight in [0.03, 0.7] for L >= 64
  and no row uniform (minimum > 1/L); one-hot - median > 0.999; common offset - close to uniform (median <= 4/L for L >= 64) with a
  per-group logit spread of 5e-5 .. 5e-3.  Margins: at least 90 % of the groups have a top-1 / top-2 margin above 4 x the tight bound
  (their argmax is then decided for any implementation inside that bound), and in the soft and common-offset regimes at least 90 % of the
  groups have a spread the float32 output can resolve to 1e-3 (1e-3 x std >= 2 x (1 ulp + 2 d): what two logits inside the bounds of
  test_gpu_score_tail.py can differ by), as has the median group."""
  for tail in R.TAILS:
    c = R.case_refs(groups, L, regime, tail)
    pm, what = c['pmax'], f'{groups}x{L} {regime}, tail {tail}'
    assert np.isfinite(c['ref']).all() and np.isfinite(c['emu']).all()
    assert c['d'] <= 5e-9, f'{what}: the float32 q/k rounding moves a logit by {c["d"]:.2e}'
    if regime == 'soft':
      if L >= 64:
        assert 0.03 <= np.median(pm) <= 0.7, f'{what}: median largest weight {np.median(pm):.4f}'
      if L >= 2:
        assert pm.min() > 1.0 / L, what
    elif regime == 'onehot':
      assert np.median(pm) > 0.999, f'{what}: median largest weight {np.median(pm):.6f}'
      if L >= 2:
        assert np.abs(c['ref']).max() < 2.0          # (the logit itself stays O(1): only the attention scores are large)
    else:
      if L >= 64:
        assert np.median(pm) <= 4.0 / L, f'{what}: median largest weight {np.median(pm):.4f}'
      if L >= 2:
        assert 5e-5 <= np.median(c['std']) <= 5e-3, f'{what}: median logit spread {np.median(c["std"]):.2e}'
    assert c['decided'].mean() >= 0.9, f'{what}: only {c["decided"].mean():.2f} of the groups have a decided argmax'
    if regime != 'onehot' and L >= 2:
      floor = 2 * (c['ulp'] + 2 * c['d'])
      assert (1e-3 * c['std'] >= floor).mean() >= 0.9 and 1e-3 * np.median(c['std']) >= floor, f'{what}: float32 cannot resolve the spread'


def test_every_code_path_of_the_kernels_has_a_shape():
  """The shapes name the edges of score_tail.hip: a ragged last row block of cross_qk_kernel (M % 4 != 0), a ragged last query block
  (L % 4 != 0), one / two keys per lane, a second pass of the 256-key loop, and FP_TAIL_MAX_GROUPS groups."""
  shapes = set(R.SHAPES)
  assert {g * L for g, L in shapes} >= {9, 15, 21}
  assert any(L % 4 for _, L in shapes) and any(L % 4 == 0 for _, L in shapes)
  assert {L for _, L in shapes} >= {1, 63, 64, 65, 252, 256, 257, 513}
  assert (4096, 2) in shapes
  assert len(R.CASES) == 3 * len(R.SHAPES)


def test_case_inputs_are_reproducible_and_distinct():
  a = R.make_feats(3, 65, 'soft')
  np.testing.assert_array_equal(a, R.make_feats(3, 65, 'soft'))
  assert a.dtype == np.float32 and a.shape == (195, 512)
  assert not np.array_equal(a[:65], a[65:130])
  assert abs(R.make_feats(3, 65, 'offset').mean() - 0.2) < 1e-3
