"""CPU checks behind tests/test_gpu_pose_arith.py: the plain reference (tests/tools/pose_ref.py) agrees with the float32 oracle where it
must, and the named cases can tell a subtly wrong kernel from a right one - every deliberately wrong variant (pose_ref.MUTANTS) differs
from the reference on the case KILLS names by more than the GPU test allows there.  So a pass on the GPU means something, and a failure
is never a property of the inputs.

One variant cannot be told apart, by these or any inputs: the so3 clamp 1e-6 in place of 1e-4.  See
test_so3_eps_mutant_is_below_float32_resolution."""
import numpy as np
import pytest
import torch

from tests.tools import pose_ref as R

f32 = np.float32
# mutant -> (family, case) that tells it from the reference at the GPU test's tolerance; None: cannot be told apart (see the module docstring)
KILLS = {
    'round_half_away': ('crop', 'half_ties'),
    'swap_ow_oh': ('crop', 'wide_160x96'),
    'u_extent_only': ('crop', 'fy_2fx'),
    'skew_ignored': ('crop', 'large_skew'),
    'so3_eps_1e-6': None,
    'so3_no_clamp': ('update', 'so3_tiny'),
    'swap_tn0_tn1': ('update', 'tanh_tn_n65'),
    'delta_on_the_right': ('update', 'raw_n64_inplace'),
    'so3_no_transpose': ('update', 'saturated'),
    'd6_no_second_clamp': ('update', 'd6_degenerate'),
    'inverse_transposed_cofactor': ('update', 'deepim_full'),
    'rank_unstable': ('rank', 'n2_tie'),
    'rank_plus_zero_above_minus_zero': ('rank', 'signed_zeros_64'),
    'rank_nan_last': ('rank', 'mixed_300'),
}
C = R.cases()


def _crop(case, mutant=None):
  outs = [R.crop_window(mutant=mutant, **call) for call in C['crop'][case]]
  return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])


def test_cases_are_pinned():
  assert {k: len(v) for k, v in C.items()} == R.N_CASES
  assert set(KILLS) == set(R.MUTANTS)
  again = R._update_cases()                              # seeded: a second build gives the same bits
  for name, c in C['update'].items():
    assert np.array_equal(c['rot'], again[name]['rot']) and np.array_equal(c['poseA'], again[name]['poseA'])
  assert sum(len(call['poses']) for call in C['crop']['half_ties']) == 8
  assert sorted(len(call['poses']) for name in ('n1', 'wide_160x96', 'fy_2fx', 'tall_96x160', 'fx_2fy') for call in C['crop'][name]) == [1, 63, 64, 65, 130]
  assert {len(s) for s in C['rank'].values()} >= {1, 2, 255, 256, 257, 300}
  assert max(len(c['poseA']) for c in C['update'].values()) <= 300


@pytest.mark.parametrize('case', list(C['crop']))
def test_crop_window_equals_the_oracle_bit_for_bit(case):
  from oracle import geometry as G
  for call in C['crop'][case]:
    tf, bbox = R.crop_window(**call)
    with np.errstate(all='ignore'):
      tf_o = G.compute_crop_window_tf_batch(torch.from_numpy(call['poses']), call['K'], call['ratio'], call['out_size'], call['diameter'])
    assert np.array_equal(tf.view(np.uint32), tf_o.numpy().view(np.uint32)) or np.array_equal(tf, tf_o.numpy(), equal_nan=True)
    if np.isfinite(tf).all():
      # the oracle inverts tf with LAPACK: the corners agree to a few float32 roundings of their magnitude, not bit for bit
      bb_o = G.crop_bbox2d_ori(tf_o, call['out_size']).numpy()
      np.testing.assert_allclose(bbox, bb_o, rtol=0, atol=4 * R.ulp32(max(1.0, np.abs(bb_o).max())))


def test_crop_cases_are_what_they_are_named():
  # half_ties: every border an exact half, odd and even integer parts on both axes and sides
  parities = set()
  for call in C['crop']['half_ties']:
    for left, right, top, bottom in R.window_borders(call['poses'], call['K'], call['ratio'], call['diameter']):
      for side, v in (('l', left), ('r', right), ('t', top), ('b', bottom)):
        assert v.denominator == 2, (side, v)
        parities.add((side, (v.numerator // 2) % 2))
  assert len(parities) == 8
  tf, _ = _crop('half_ties')
  k127 = C['crop']['half_ties'][0]                      # centre 320, rad 63.5: 256.5 -> 256 and 383.5 -> 384
  assert tf[0, 0, 0] == f32(1) / f32(128) * f32(160) and tf[0, 0, 2] == tf[0, 0, 0] * f32(-256) and k127['diameter'] == 2 * 127 / 1024
  # large_skew / fy_2fx: the largest extent is the skew term / a v extent
  for case, mutant in (('large_skew', 'skew_ignored'), ('fy_2fx', 'u_extent_only')):
    assert (_crop(case)[0][:, 0, 0] < _crop(case, mutant)[0][:, 0, 0]).all()        # (the right window is larger: a smaller scale)
  tf, bbox = _crop('off_image')
  assert (bbox[:, 0] < 0).any() and (bbox[:, 2] > 640).any() and (bbox[:, 2] < 0).any() and (bbox[:, 1] > 480).any() and np.isfinite(bbox).all()
  tf, bbox = _crop('collapsed')
  assert np.isinf(tf[:, 0, 0]).all() and np.isinf(tf[:, 1, 1]).all() and not np.isfinite(bbox[:, 0]).any()
  tf, bbox = _crop('tz_near_radius')
  assert np.isfinite(tf).all() and (bbox[:, 2] - bbox[:, 0] > 1000).all()
  assert C['crop']['wide_160x96'][0]['out_size'] == (160, 96) and C['crop']['tall_96x160'][0]['out_size'] == (96, 160)


@pytest.mark.parametrize('case', list(C['update']))
def test_pose_update64_agrees_with_the_float32_oracle(case):
  """e32 = max |oracle - reference| is a float32 evaluation's own error: a few ulp of the outputs (<= 1.6, so < 1e-6) on every case with a
  meaningful answer.  The bound the GPU test uses is derived from it (pose_ref.update_bound)."""
  c = C['update'][case]
  ref, ora = R.update_case_ref(c), R.oracle_update(c)
  assert ora.dtype == np.float32 and np.isfinite(ora).all()
  if c.get('degenerate'):
    assert np.isfinite(ref).all()
    return
  e32, bound = R.update_bound(c, ref, ora)
  print(f'{case}: e32 = {e32:.3e}, bound = {bound:.3e}, largest output {np.abs(ref).max():.3f}')
  if case == 'd6_near_parallel':
    assert e32 > 1e-3                                   # b2 keeps no digit in float32: the bound says so, and the case pins finiteness only
  else:
    assert e32 < 1.5e-6, f'{case}: the float32 oracle is {e32:.2e} from the float64 reference'
    assert bound < 6e-6


def test_update_cases_are_what_they_are_named():
  c = C['update']['so3_tiny']
  v = np.tanh(c['rot'].astype(np.float64)) * R.ROT_NORMALIZER
  norms = np.linalg.norm(v, axis=1)
  assert norms[0] == 0
  np.testing.assert_allclose(norms[1:].reshape(len(R.TINY_NORMS), len(R.TINY_DIRS)), np.repeat(np.array(R.TINY_NORMS)[:, None], len(R.TINY_DIRS), 1), rtol=2e-6)
  assert ((norms > 0) & (norms < 0.01)).sum() >= 15 and (norms > 0.01).sum() >= 10           # both sides of the clamp
  assert (np.count_nonzero(v, axis=1) == 1).sum() >= 3 * len(R.TINY_NORMS)                    # single-axis rows
  c = C['update']['saturated']
  assert (np.tanh(c['rot'].astype(np.float32)) == np.sign(c['rot'])).all() and (np.tanh(c['trans'].astype(np.float32)) == np.sign(c['trans'])).all()
  assert len({f32(t) for t in R.TN_DISTINCT}) == 3
  assert C['update']['deepim_full']['resize'] != 160 and (C['update']['deepim_full']['tf'][:, :2] != 0).all()
  K = C['update']['deepim_full']['K']
  assert K[1, 0] != 0 and K[0, 1] != 0 and np.linalg.cond(K) < 1e4
  assert max(np.linalg.cond(t.astype(np.float64)[:2, :2]) for t in C['update']['deepim_full']['tf']) < 10
  d = C['update']['d6_degenerate']['rot']
  assert len(d) <= 4 and not d[0, :3].any() and not d[1, 3:].any() and np.array_equal(d[2, 3:], 3 * d[2, :3]) and np.array_equal(d[3, 3:], 3 * d[3, :3])
  assert sorted(len(c['poseA']) for c in C['update'].values() if c['mode'] == 'raw' and c['rot'].shape[1] == 3)[:1] == [1]
  assert {1, 63, 64, 65} <= {len(c['poseA']) for c in C['update'].values()}


def test_rotation_block_stays_a_rotation():
  """R_delta is orthogonal, so R_out^T R_out = R_A^T R_A and det R_out = det R_A whatever float32 rounding left in R_A
  (pose_ref.rotation_defect).  The float64 reference keeps both to 1e-9 (below |v| = 0.01 the clamped
  formula is not exactly orthogonal: sin(t)/t is taken at t = 0.01, a defect of |v|^2 (1e-4 - |v|^2) / 3 < 1e-9); the float32 oracle to a few float32 ulp - the class the
  GPU test holds the kernel to (16 ulp of 1)."""
  for name, c in C['update'].items():
    if c.get('degenerate') or name == 'd6_near_parallel':
      continue
    for out, tol in ((R.update_case_ref(c), 1e-9), (R.oracle_update(c), R.ROTATION_TOL)):
      assert R.rotation_defect(out, c['poseA']) < tol, name


def test_chained_updates():
  """5 chained updates: the float32 oracle's chain stays within a few ulp of the float64 chain (errors add, they do not grow)"""
  ref, ora, e32, bound = R.chain_ref()
  print(f'chain of {R.CHAIN_DEPTH}: e32 = {e32:.3e}, bound = {bound:.3e}')
  assert e32 < 3e-6 and R.rotation_defect(ora, R.chain_inputs()[0]) < R.CHAIN_DEPTH * R.ROTATION_TOL


@pytest.mark.parametrize('case', list(C['rank']))
def test_rank_equals_torch_stable_sort(case):
  s = C['rank'][case]
  want = torch.sort(torch.from_numpy(s.copy()), descending=True, stable=True)
  got = R.rank(s)
  assert np.array_equal(got, want.indices.numpy())
  assert np.array_equal(s[got].view(np.uint32), want.values.numpy().view(np.uint32))
  assert sorted(got.tolist()) == list(range(len(s)))


def test_rank_issue_example():
  assert R.rank(C['rank']['issue_example']).tolist() == [3, 9, 4, 2, 8, 0, 1, 5, 6, 7]


def test_hypotheses_equal_guess_translation():
  from oracle import geometry as G
  h = C['hypotheses']['skewed']
  got = R.hypotheses(**h)
  off = 0
  for g, st, med in zip(h['rot_grids'], h['stats'], h['medians']):
    mask = np.zeros((480, 640), dtype=np.uint8)
    mask[st[2], st[0]] = mask[st[3], st[1]] = 1
    want = G.guess_translation(np.full((480, 640), med, dtype=np.float32), mask, h['K']) if med > 0 else np.zeros(3)
    rows = got[off:off + len(g)]
    assert np.array_equal(rows[:, :3, :3], g[:, :3, :3]) and (rows[:, 3] == [0, 0, 0, 1]).all()
    assert (rows[:, :3, 3] == want.astype(np.float32)).all()
    off += len(g)
  assert off == len(got) == 193
  assert (h['stats'][0, 0] + h['stats'][0, 1]) % 2 == 1 and (h['stats'][0, 2] + h['stats'][0, 3]) % 2 == 1
  assert [len(g) for g in h['rot_grids']] == [63, 1, 0, 64, 65] and np.linalg.inv(h['K'])[0, 1] != 0


def _pom_inputs():
  rng = np.random.default_rng(50)
  lattice = (rng.integers(-1023, 1024, (6, 4, 4)) / 256.0).astype(np.float32)
  lattice[:, 3] = [0, 0, 0, 1]
  centers_l = (rng.integers(-1023, 1024, (6, 3)) / 256.0).astype(np.float32)
  rand = R._pose_inputs(24, 51, 3)[0]
  centers_r = (rng.standard_normal((24, 3)) * 0.05).astype(np.float32)
  return (lattice, centers_l), (rand, centers_r)


def test_pose_of_mesh_orders():
  (lat, cl), (rnd, cr) = _pom_inputs()
  for p, c in zip(lat, cl):                             # on the lattice every product and sum is a float32: both orders give the exact value
    want = p.astype(np.float64) @ np.array([[1, 0, 0, -float(c[0])], [0, 1, 0, -float(c[1])], [0, 0, 1, -float(c[2])], [0, 0, 0, 1]])
    assert np.array_equal(R.pose_of_mesh_fma(p, c), want.astype(np.float32)) and np.array_equal(R.pose_of_mesh_plain(p, c), want)
  differ = 0
  for p, c in zip(rnd, cr):
    plain = R.pose_of_mesh_plain(p, c)
    cn = -c
    step = np.array([((p[r, 0] * cn[0] + p[r, 1] * cn[1]) + p[r, 2] * cn[2]) + p[r, 3] for r in range(4)], dtype=np.float32)   # np.float32 scalars round every op
    assert np.array_equal(plain[:, 3], step) and np.array_equal(plain[:, :3], p[:, :3])
    fma = R.pose_of_mesh_fma(p, c)
    exact = p.astype(np.float64)[:, :3] @ cn.astype(np.float64) + p[:, 3]
    assert np.abs(fma[:, 3] - exact).max() <= 2 * R.ulp32(np.abs(exact).max())
    differ += int((fma != plain).any())
  assert differ > 0                                     # the random case does tell the two orders apart


# ------------------------------------------------------------------------------------------------------------------------------------------
# the mutants
# ------------------------------------------------------------------------------------------------------------------------------------------
def _separation(mutant, family, case):
  """(how far the mutant is from the reference on the case, what the GPU test allows there)"""
  if family == 'crop':
    (tf, bb), (tf_m, bb_m) = _crop(case), _crop(case, mutant)
    return (0.0 if np.array_equal(tf, tf_m, equal_nan=True) and np.array_equal(bb, bb_m, equal_nan=True) else np.inf), 0.0
  if family == 'rank':
    s = C['rank'][case]
    return (0.0 if np.array_equal(R.rank(s), R.rank(s, mutant)) else np.inf), 0.0
  c = C['update'][case]
  ref, mut = R.update_case_ref(c), R.update_case_ref(c, mutant)
  if not np.isfinite(mut).all():
    return np.inf, 0.0                                  # the GPU test requires finite output everywhere
  return float(np.abs(ref - mut).max()), (2e-6 if c.get('degenerate') else R.update_bound(c, ref)[1])


@pytest.mark.parametrize('mutant', [m for m in R.MUTANTS if KILLS[m]])
def test_every_mutant_is_killed_by_its_named_case(mutant):
  family, case = KILLS[mutant]
  sep, allowed = _separation(mutant, family, case)
  print(f'{mutant}: {family}/{case} separates it by {sep:.3e}, allowed {allowed:.3e}')
  assert sep > 4 * allowed and sep > 0, f'{mutant}: {family}/{case} separates it by {sep:.2e}, the GPU test allows {allowed:.2e}'


def test_so3_eps_mutant_is_below_float32_resolution():
  """The clamp 1e-6 in place of 1e-4 changes sin(t)/t only for |v| < 0.01, by (1e-4 - |v|^2) / 6 at most, and that factor multiplies
  entries of size |v|: the rotation moves by |v| (1e-4 - |v|^2) / 6 <= 6.5e-8 (at |v| = 0.01 / sqrt 3), and the (1 - cos t) / t^2 term by
  |v|^2 1e-4 / 24 <= 5e-10.  Every output has the entry 1 (and a rotation block of unit rows), so 2 float32 ulp of the largest output is
  at least 2.4e-7: the variant is inside the float32 resolution of the result, for any input - scaling the pose scales both sides.  The
  test pins this, so that the table's `None` is a computed fact: the largest separation on so3_tiny is below a quarter of the bound."""
  c = C['update']['so3_tiny']
  ref, mut = R.update_case_ref(c), R.update_case_ref(c, 'so3_eps_1e-6')
  sep, bound = float(np.abs(ref - mut).max()), R.update_bound(c, ref)[1]
  assert 0 < sep < 6.5e-8 and bound >= 2 * R.ulp32(1.0) and sep < bound / 3
  v = np.linspace(0, 0.01, 2001)
  assert (v * (1e-4 - v * v) / 6).max() < 6.5e-8


def test_every_case_kills_a_mutant_or_adds_a_shape():
  """A case stays only if it is some mutant's named case or runs a size / path no other case has."""
  named = {fc for fc in KILLS.values() if fc}
  shape_only = {
      ('crop', 'tall_96x160'): 'N = 65, height > width', ('crop', 'fx_2fy'): 'N = 130: three blocks', ('crop', 'off_image'): 'negative and off-frame borders',
      ('crop', 'collapsed'): 'right == left: inf / nan', ('crop', 'tz_near_radius'): 'windows wider than the frame', ('crop', 'n1'): 'N = 1',
      ('update', 'raw_n1'): 'N = 1', ('update', 'd6_regular_n63'): 'N = 63, 6d at three scales', ('update', 'd6_inplace'): '6d in place',
      ('update', 'd6_near_parallel'): 'b2 just above its clamp', ('update', 'deepim_full_6d'): 'deepim with 6d and a translation scale',
      ('rank', 'issue_example'): 'the predicted signed-zero defect', ('rank', 'n1'): 'n = 1', ('rank', 'n1_nan'): 'n = 1, NaN winner',
      ('rank', 'all_equal_255'): 'n = 255, one run', ('rank', 'tie_runs_256'): 'n = 256', ('rank', 'increasing_257'): 'n = 257, reversed',
      ('rank', 'decreasing_300'): 'n = 300, identity', ('rank', 'denormals_40'): 'denormals', ('rank', 'negative_65'): 'negative scores',
      ('hypotheses', 'skewed'): 'the only hypotheses case',
  }
  every = {(fam, name) for fam, d in C.items() for name in d}
  assert named | set(shape_only) == every and not named & set(shape_only)
