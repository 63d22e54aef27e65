"""The ScoreNet tail (csrc/score_tail.hip: cross_qk_kernel, cross_logit_kernel) against float64 references at the sizes where its
structure changes: ragged row and query blocks, one / two / five keys per lane, a second pass of the 256-key loop, lanes without keys in
the merge, every arrival counter in use - each in a soft, a one-hot and a common-offset softmax regime, on the fixtures' tail weights and
on a tail seed nobody tuned.  References, inputs and bounds: tests/tools/score_tail_ref.py; that the inputs are what they claim to be is
checked on the CPU by tests/test_score_tail_host.py."""
import os
import re

import numpy as np
import pytest
import torch

from tests.tools import score_tail_ref as R

pytestmark = pytest.mark.gpu

CASE_IDS = [f'{g}x{L}-{r}' for g, L, r in R.CASES]


@pytest.fixture(scope='module')
def env():
  from foundationpose_amd import _lib, synthetic as S
  ctx = _lib.Context.get('cuda:0')
  base = S.make_score_state_dict(1)
  nets = {None: _lib.DeviceNet(ctx, _lib.FP_NET_SCORE, base, use_bn=True),
          5003: _lib.DeviceNet(ctx, _lib.FP_NET_SCORE, dict(base, **R.tail_sd(5003)), use_bn=True)}
  return dict(ctx=ctx, nets=nets)


def run_tail(env, feats, groups, L, tail=None, ld=512, score_offset=None, with_argmax=True):
  """One call of fp_score_tail (ld 512, no scores) or fp_score_tail_scores on NaN-prefilled outputs (argmax: -7).
  -> (logits (groups, L) float32, argmax (groups,) int32 or None, scores or None) as numpy arrays."""
  from foundationpose_amd._lib import check, lib, ptr, stream_ptr
  feats = feats if torch.is_tensor(feats) else torch.tensor(feats).cuda()
  assert feats.shape == (groups * L, ld)
  logits = torch.full((groups, L), float('nan'), device='cuda')
  am = torch.full((groups,), -7, dtype=torch.int32, device='cuda') if with_argmax else None
  scores = None
  ctx, net = env['ctx'].handle, env['nets'][tail].handle
  if ld == 512 and score_offset is None and with_argmax:
    check(lib().fp_score_tail(ctx, net, ptr(feats), groups, L, ptr(logits), ptr(am), stream_ptr()))
  else:
    scores = None if score_offset is None else torch.full((groups, L), float('nan'), device='cuda')
    check(lib().fp_score_tail_scores(ctx, net, ptr(feats), ld, groups, L, float(score_offset or 0.0), ptr(logits), ptr(scores), ptr(am), stream_ptr()))
  torch.cuda.synchronize()
  return logits.cpu().numpy(), None if am is None else am.cpu().numpy(), None if scores is None else scores.cpu().numpy()


def own_argmax(logits):
  """torch.argmax's rule on the kernel's own float32 logits: the first index of the maximum."""
  return np.argmax(logits, axis=-1).astype(np.int32)


@pytest.mark.parametrize('groups,L,regime', R.CASES, ids=CASE_IDS)
def test_logits_and_argmax_against_float64(env, groups, L, regime):
  """Per case and tail seed:
  tight        max |got - tail_emulation| <= 1 float32 ulp at max |logit| (0.5 ulp output rounding + float64 summation order + double rounding)
  textbook     max |got - tail_reference| <= 1 ulp + 2 d,  d = max |tail_emulation - tail_reference| of that case (the float32 q / k rows)
  differential soft and common-offset regimes, L >= 2: |(got - group mean) - (ref - group mean)| <= 1e-3 x the reference's standard
               deviation in the group: over the whole case against the median group, and group by group wherever float32 can resolve
               that (1e-3 x std >= 2 (ulp + 2 d), at least 90 % of the groups: test_score_tail_host.py; for a group of two the spread
               can be arbitrarily small and no float32 output can follow it to 1e-3)
  argmax       the first maximum of the kernel's own logits, always; the reference's argmax wherever its margin exceeds 4 x the tight bound
  Measured on an MI355X over all cases and both tail seeds (soft / one-hot / common offset): tight error at most 0.498 / 0.499 / 0.500 ulp;
  d at most 6.0e-10 / 1.5e-15 / 1.3e-9; worst differential error / spread 6.5e-7 (soft) and 5.8e-5 (common offset) over a case, 3.4e-5
  and 8.7e-5 group by group (both at 4096 x 2) - every one more than 10 x below the bound of 1e-3."""
  for tail in R.TAILS:
    c = R.case_refs(groups, L, regime, tail)
    got32, am, _ = run_tail(env, c['feats'], groups, L, tail)
    assert not np.isnan(got32).any() and (am >= 0).all() and (am < L).all()
    got = got32.astype(np.float64)
    e_tight, e_text = float(np.abs(got - c['emu']).max()), float(np.abs(got - c['ref']).max())
    line = f'score tail {groups}x{L} {regime} tail {tail}: ulp {c["ulp"]:.2e} tight {e_tight / c["ulp"]:.3f} ulp, d {c["d"]:.2e}, textbook {e_text:.2e}'
    ratios = None
    if regime != 'onehot' and L >= 2:
      derr = np.abs(R.differential(got) - R.differential(c['ref'])).max(-1)
      ok = 1e-3 * c['std'] >= 2 * (c['ulp'] + 2 * c['d'])
      ratios = float(derr.max() / np.median(c['std'])), float((derr[ok] / c['std'][ok]).max())
      line += f', differential / spread {ratios[0]:.2e} (case) {ratios[1]:.2e} (worst of {int(ok.sum())} groups)'
    print(line)
    assert e_tight <= c['ulp'], line
    assert e_text <= c['ulp'] + 2 * c['d'], line
    if ratios is not None:
      assert ratios[0] <= 1e-3 and ratios[1] <= 1e-3, line
    np.testing.assert_array_equal(am, own_argmax(got32), err_msg=line)
    want = c['ref'].argmax(-1)
    np.testing.assert_array_equal(am[c['decided']], want[c['decided']], err_msg=line)


def test_rows_with_stride_528_and_scores(env):
  """fp_score_tail_scores on the all-gather records [feature 512 | pose 16]: the 16 trailing columns (NaN here) never reach a result,
  the logits are those of the packed call bit for bit, scores = logits + float32(offset) exactly; the same without an argmax output."""
  for groups, L in ((3, 5), (3, 65), (1, 257)):
    for regime in ('soft', 'offset'):
      c = R.case_refs(groups, L, regime)
      base, am0, _ = run_tail(env, c['feats'], groups, L)
      rows = np.full((groups * L, 528), np.nan, dtype=np.float32)
      rows[:, :512] = c['feats']
      logits, am, scores = run_tail(env, rows, groups, L, ld=528, score_offset=0.37)
      assert not np.isnan(logits).any() and not np.isnan(scores).any()
      np.testing.assert_array_equal(logits, base)
      np.testing.assert_array_equal(scores, logits + np.float32(0.37))
      np.testing.assert_array_equal(am, am0)
      np.testing.assert_array_equal(am, own_argmax(logits))
      logits2, am2, scores2 = run_tail(env, rows, groups, L, ld=528, score_offset=0.37, with_argmax=False)
      assert am2 is None
      np.testing.assert_array_equal(logits2, base)
      np.testing.assert_array_equal(scores2, scores)
      logits3, _, scores3 = run_tail(env, rows, groups, L, ld=528, with_argmax=False)          # neither scores nor argmax
      assert scores3 is None
      np.testing.assert_array_equal(logits3, base)


def test_ties_go_to_the_lower_index(env):
  """torch.argmax returns the first maximum.  (a) 70 identical rows: 70 bitwise equal logits, argmax 0.  (b) [X; X] with 129 rows of X:
  row i and row i + 129 sit in different slots of their query blocks (129 % 4 = 1) and must still give the same bits - a query's
  arithmetic does not depend on its slot - so the maximum occurs twice and the argmax is the occurrence below 129."""
  for regime in ('soft', 'offset'):
    x = R.make_feats(1, 129, regime)
    same = np.repeat(x[5:6], 70, axis=0)
    logits, am, _ = run_tail(env, same, 1, 70)
    assert not np.isnan(logits).any()
    assert (logits.view(np.int32) == logits.view(np.int32)[0, 0]).all()
    assert am[0] == 0
    logits, am, _ = run_tail(env, np.concatenate([x, x]), 1, 258)
    assert not np.isnan(logits).any()
    np.testing.assert_array_equal(logits[0, :129].view(np.int32), logits[0, 129:].view(np.int32))
    assert len(np.unique(logits)) > 100          # (and they are not all the same number)
    assert am[0] == own_argmax(logits)[0] and am[0] < 129


def test_counters_return_to_zero(env):
  """The workgroup that arrives last at its group's counter takes the argmax and must leave the counter at zero: a counter left behind
  shows as an argmax that is never written (-7 stays) or taken early (of logits not yet there) in the next call.  Three grids that
  use the counters differently (4096 x 1 workgroup, 5 x 17, 1 x 63), each twice, on one context."""
  for groups, L in ((4096, 2), (5, 65), (1, 252)):
    feats = torch.tensor(R.make_feats(groups, L, 'soft')).cuda()
    first = None
    for run in range(2):
      logits, am, _ = run_tail(env, feats, groups, L)
      assert not np.isnan(logits).any()
      np.testing.assert_array_equal(am, own_argmax(logits), err_msg=f'{groups}x{L}, run {run}')
      if first is not None:
        np.testing.assert_array_equal(logits.view(np.int32), first[0].view(np.int32))
        np.testing.assert_array_equal(am, first[1])
      first = (logits, am)


def _tail_max_groups():
  common_h = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'foundationpose_amd', 'csrc', 'common.h')
  with open(common_h) as f:
    return int(re.search(r'#define\s+FP_TAIL_MAX_GROUPS\s+(\d+)', f.read()).group(1))


def test_group_limit(env):
  """One arrival counter per group, FP_TAIL_MAX_GROUPS of them: one group more is refused on the host (before any launch) with the limit
  in the message; no group at all is a call that does nothing; L = 0 is an error."""
  from foundationpose_amd._lib import FoundationPoseAmdError, check, lib, ptr, stream_ptr
  limit = _tail_max_groups()
  assert limit == max(g for g, _ in R.SHAPES)          # the largest case above uses every counter
  ctx, net = env['ctx'].handle, env['nets'][None].handle
  feats = torch.tensor(R.make_feats(limit + 1, 1, 'soft')).cuda()
  logits = torch.full((limit + 1,), float('nan'), device='cuda')
  am = torch.full((limit + 1,), -7, dtype=torch.int32, device='cuda')
  with pytest.raises(FoundationPoseAmdError, match=rf'\b{limit}\b'):
    check(lib().fp_score_tail(ctx, net, ptr(feats), limit + 1, 1, ptr(logits), ptr(am), stream_ptr()))
  check(lib().fp_score_tail(ctx, net, ptr(feats), 0, 1, ptr(logits), ptr(am), stream_ptr()))
  with pytest.raises(FoundationPoseAmdError):
    check(lib().fp_score_tail(ctx, net, ptr(feats), 1, 0, ptr(logits), ptr(am), stream_ptr()))
  torch.cuda.synchronize()
  assert torch.isnan(logits).all() and (am == -7).all()          # none of the three wrote anything
  check(lib().fp_score_tail(ctx, net, ptr(feats), limit, 1, ptr(logits), ptr(am), stream_ptr()))          # the limit itself is served
  torch.cuda.synchronize()
  assert not torch.isnan(logits[:limit]).any() and (am[:limit] == 0).all() and torch.isnan(logits[limit:]).all() and int(am[limit]) == -7


def test_a_group_does_not_depend_on_its_neighbours(env):
  """Group 1 of a 3 x 257 call is the same 257 rows run alone, bit for bit: logits and argmax."""
  for regime in R.REGIMES:
    c = R.case_refs(3, 257, regime)
    logits, am, _ = run_tail(env, c['feats'], 3, 257)
    alone, am1, _ = run_tail(env, c['feats'][257:514], 1, 257)
    np.testing.assert_array_equal(logits[1].view(np.int32), alone[0].view(np.int32))
    assert am[1] == am1[0]
    assert not np.array_equal(logits[0], logits[1])
