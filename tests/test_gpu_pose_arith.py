"""GPU: the pose arithmetic every refinement pass ends in (csrc/pose_math.h) and the ranking and hypothesis kernels of a registration
(csrc/register.hip), through the C ABI, against the plain reference tests/tools/pose_ref.py on the named cases whose discriminating power
tests/test_pose_ref_host.py shows on the CPU.

  crop window     bit-equal (tf and bbox, NaN == NaN) to the float32 step-by-step reference: half-integer borders, non-square outputs,
                  fy = 2 fx and fx = 2 fy, a skew larger than fx, windows off the image, collapsed windows (inf / nan), N around the block size
  pose update     against float64.  Bound per case: 4 x e32 with a floor of 2 float32 ulp of the largest output, e32 = max |float32 oracle -
                  float64 reference| measured on the CPU when the test runs (the kernel runs the oracle's operation sequence; the factor 4
                  covers the device tanhf / sinf / cosf entering a chain of about 4 dependent products).  The four degenerate 6d rows
                  (a1 = 0, a2 = 0, a2 = 3 a1 twice) have no meaningful float64 answer: float32 oracle at 2e-6 and finite output.
  ranking         order, scores (bit patterns), permuted poses and the winner's pose of the mesh, all exact
  hypotheses      bit-equal to float64 inv(K) @ [uc, vc, 1] * median rounded once

Measured on an MI355X (case: e32, kernel error / bound):
  so3_tiny          6.4e-08  0.25      d6_regular_n63    6.9e-07  0.25      deepim_full       1.1e-07  0.41
  saturated         7.4e-08  0.25      d6_inplace        2.5e-07  0.25      deepim_full_6d    1.5e-07  0.31
  tanh_tn_n65       9.9e-08  0.27      d6_near_parallel  5.6e-01  0.16      chain of five     1.6e-07  0.37
  raw_n64_inplace   8.5e-08  0.29      raw_n1            4.6e-08  0.19      d6_degenerate     6.0e-08 from the float32 oracle (allowed 2e-6)
(0.25 = the kernel gave the oracle's bits and the bound is 4 e32.)  Crop window, ranking and hypotheses: every case bit-equal.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.tools import pose_ref as R

pytestmark = pytest.mark.gpu
C = R.cases()
f32 = np.float32
PAD = 3                                    # slots behind every ranking output that must keep their prefill


@pytest.fixture(scope='module')
def fp():
  from foundationpose_amd import _lib
  return dict(L=_lib, ctx=_lib.Context.get('cuda:0'))


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------------------------
# crop window
# ------------------------------------------------------------------------------------------------------------------------------------------
def _crop_window(fp, poses, K, ratio, out_size, diameter):
  L = fp['L']
  n = len(poses)
  d = _dev(poses)
  tf = torch.full((n + 1, 3, 3), -7.0, device='cuda')
  bbox = torch.full((n + 1, 4), -7.0, device='cuda')
  Kd, Kp = L.k_ptr(K)
  L.check(L.lib().fp_crop_window_tf(fp['ctx'].handle, L.ptr(d), n, Kp, float(ratio), float(diameter), int(out_size[0]), int(out_size[1]), L.ptr(tf),
                                    L.ptr(bbox), L.stream_ptr()))
  torch.cuda.synchronize()
  tf, bbox = tf.cpu().numpy(), bbox.cpu().numpy()
  assert (tf[n] == -7).all() and (bbox[n] == -7).all()            # nothing written behind row N - 1
  return tf[:n], bbox[:n]


@pytest.mark.parametrize('case', list(C['crop']))
def test_crop_window_bit_equal(fp, case):
  for call in C['crop'][case]:
    tf_r, bb_r = R.crop_window(**call)
    tf_g, bb_g = _crop_window(fp, **call)
    bad = [b for b in range(len(tf_r)) if not (np.array_equal(tf_r[b], tf_g[b], equal_nan=True) and np.array_equal(bb_r[b], bb_g[b], equal_nan=True))]
    assert not bad, f'{case}: rows {bad[:5]} differ, first: tf {tf_g[bad[0]].ravel()} vs {tf_r[bad[0]].ravel()}, bbox {bb_g[bad[0]]} vs {bb_r[bad[0]]}'


# ------------------------------------------------------------------------------------------------------------------------------------------
# pose update
# ------------------------------------------------------------------------------------------------------------------------------------------
def _pose_update(fp, c, poseA=None, trans=None, rot=None, inplace=False, n=None):
  """one fp_pose_update / fp_pose_update_deepim call on a case -> (n,4,4) float32 (in place: the pose buffer itself)"""
  L = fp['L']
  A = _dev(c['poseA'] if poseA is None else poseA)
  t, r = _dev(c['trans'] if trans is None else trans), _dev(c['rot'] if rot is None else rot)
  n = len(A) if n is None else n
  out = A if inplace else torch.full((len(A), 4, 4), float('nan'), device='cuda')
  rot_dim = r.shape[1]
  if c['mode'] == 'deepim':
    tf = _dev(c['tf'].reshape(-1, 9))
    Kd = np.ascontiguousarray(c['K'], dtype=np.float64)
    L.check(L.lib().fp_pose_update_deepim(fp['ctx'].handle, L.ptr(A), L.ptr(t), L.ptr(r), n, rot_dim, L.ptr(tf), Kd.ctypes.data, float(c['resize']),
                                          float(c['rot_normalizer']), float(c['trans_scale']), L.ptr(out), L.stream_ptr()))
  else:
    tn = np.asarray(c['tn'], dtype=np.float32)
    L.check(L.lib().fp_pose_update(fp['ctx'].handle, L.ptr(A), L.ptr(t), L.ptr(r), n, rot_dim, 1 if c['mode'] == 'tanh' else 0, L.ptr(tn),
                                   float(c['rot_normalizer']), float(c['trans_scale']), L.ptr(out), L.stream_ptr()))
  torch.cuda.synchronize()
  return out.cpu().numpy()


@pytest.mark.parametrize('case', list(C['update']))
def test_pose_update_against_float64(fp, case):
  c = C['update'][case]
  got = _pose_update(fp, c)
  assert np.isfinite(got).all(), f'{case}: non-finite output in rows {np.unique(np.nonzero(~np.isfinite(got))[0])}'
  assert (got[:, 3] == [0, 0, 0, 1]).all()
  if c.get('inplace'):
    assert np.array_equal(_pose_update(fp, c, inplace=True), got), f'{case}: the in-place update differs from the out-of-place one'
  ora = R.oracle_update(c)
  if c.get('degenerate'):
    err = float(np.abs(got - ora).max())
    print(f'{case}: |kernel - float32 oracle| = {err:.3e} (allowed 2e-6)')
    assert err <= 2e-6
    return
  ref = R.update_case_ref(c)
  e32, bound = R.update_bound(c, ref, ora)
  err = float(np.abs(got - ref).max())
  print(f'{case}: e32 = {e32:.3e}, bound = {bound:.3e}, kernel error = {err:.3e}, error / bound = {err / bound:.3f}')
  assert err <= bound, f'{case}: the kernel is {err:.3e} from the float64 reference, allowed {bound:.3e} (e32 = {e32:.3e})'
  if case != 'd6_near_parallel':
    defect = R.rotation_defect(got, c['poseA'])
    assert defect < R.ROTATION_TOL, f'{case}: the rotation block leaves SO(3) by {defect:.2e}'


def test_pose_update_n0_writes_nothing(fp):
  c = C['update']['raw_n1']
  got = _pose_update(fp, c, n=0)
  assert np.isnan(got).all()


def test_pose_update_chain_of_five(fp):
  """the tracker's depth: 5 in-place updates with seeded deltas stay within the bound of the chained float64 reference"""
  A, steps = R.chain_inputs()
  ref, _, e32, bound = R.chain_ref()
  c = dict(mode='raw', tn=(1.0, 1.0, 1.0), rot_normalizer=R.ROT_NORMALIZER, trans_scale=R.CHAIN_SCALE)
  pose = A
  for trans, rot in steps:
    pose = _pose_update(fp, c, poseA=pose, trans=trans, rot=rot, inplace=True)
  err = float(np.abs(pose - ref).max())
  print(f'chain5: e32 = {e32:.3e}, bound = {bound:.3e}, kernel error = {err:.3e}, error / bound = {err / bound:.3f}')
  assert np.isfinite(pose).all() and err <= bound
  assert R.rotation_defect(pose, A) < R.CHAIN_DEPTH * R.ROTATION_TOL


# ------------------------------------------------------------------------------------------------------------------------------------------
# ranking
# ------------------------------------------------------------------------------------------------------------------------------------------
PREFILL_BITS = 0x7fc0dead


def _rank_call(fp, scores, poses, centers):
  """one fp_register_rank call over the objects -> list of (order, scores, poses, pose_of_mesh); asserts the padding keeps its prefill"""
  L = fp['L']
  n_obj = len(scores)
  ns = [len(s) for s in scores]
  d_scores, d_poses = _dev(np.concatenate(scores).astype(np.float32)), _dev(np.concatenate(poses).astype(np.float32))
  fill = torch.tensor(np.array([PREFILL_BITS], dtype=np.uint32).view(np.float32), device='cuda')
  po = [fill.repeat((n + PAD) * 16).reshape(-1, 4, 4) for n in ns]
  so = [fill.repeat(n + PAD) for n in ns]
  oo = [torch.full((n + PAD,), -7, dtype=torch.int64, device='cuda') for n in ns]
  pm = [fill.repeat(16 + PAD) for n in ns]
  arr = lambda ts: (ctypes.c_void_p * n_obj)(*[t.data_ptr() for t in ts])
  cen = np.ascontiguousarray(centers, dtype=np.float32).reshape(n_obj, 3)
  L.check(L.lib().fp_register_rank(fp['ctx'].handle, L.ptr(d_poses), L.ptr(d_scores), (ctypes.c_int * n_obj)(*ns), n_obj, cen.ctypes.data, arr(po), arr(so), arr(oo),
                                   arr(pm), L.stream_ptr()))
  torch.cuda.synchronize()
  out = []
  for o, n in enumerate(ns):
    p, s, order, m = po[o].cpu().numpy(), so[o].cpu().numpy(), oo[o].cpu().numpy(), pm[o].cpu().numpy()
    assert (_bits(p[n:]) == PREFILL_BITS).all() and (_bits(s[n:]) == PREFILL_BITS).all() and (order[n:] == -7).all() and (_bits(m[16:]) == PREFILL_BITS).all()
    out.append((order[:n], s[:n], p[:n], m[:16].reshape(4, 4)))
  return out


def _rank_poses(n, seed):
  rng = np.random.default_rng(seed)
  p = rng.standard_normal((n, 4, 4)).astype(np.float32)
  p[:, 3] = [0, 0, 0, 1]
  return p


def _assert_ranked(got, scores, poses, center, what):
  order, s, p, m = got
  want = R.rank(scores)
  assert sorted(order.tolist()) == list(range(len(scores))), f'{what}: order is no permutation (a slot written twice or never)'
  assert np.array_equal(order, want), f'{what}: order differs first at rank {int(np.nonzero(order != want)[0][0])}: {order[:12]} vs {want[:12]}'
  assert np.array_equal(_bits(s), _bits(scores[want])), f'{what}: scores_out'
  assert np.array_equal(_bits(p), _bits(poses[want])), f'{what}: poses_out'
  assert np.array_equal(_bits(m), _bits(R.pose_of_mesh_fma(poses[want[0]], center))), f'{what}: pose_of_mesh'


@pytest.mark.parametrize('case', list(C['rank']))
def test_rank_exact(fp, case):
  scores = C['rank'][case]
  poses, center = _rank_poses(len(scores), 60), np.array([0.0123, -0.0456, 0.0789], dtype=np.float32)
  _assert_ranked(_rank_call(fp, [scores], [poses], [center])[0], scores, poses, center, case)


def test_rank_three_objects_in_one_call(fp):
  names = ('mixed_300', 'n1_nan', 'negative_65')
  scores = [C['rank'][k] for k in names]
  poses = [_rank_poses(len(s), 61 + i) for i, s in enumerate(scores)]
  centers = np.array([[0.01, 0.02, -0.03], [-0.5, 0.25, 0.125], [0.0, 0.0, 0.0]], dtype=np.float32)
  both = _rank_call(fp, scores, poses, centers)
  for o, name in enumerate(names):
    _assert_ranked(both[o], scores[o], poses[o], centers[o], f'{name} (object {o} of 3)')
    single = _rank_call(fp, [scores[o]], [poses[o]], [centers[o]])[0]
    for a, b in zip(both[o], single):
      assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), name


def test_rank_pose_of_mesh_lattice_and_random(fp):
  """the winner's pose @ translation(-center): a lattice (entries multiples of 2^-8 below 4: every step exact) and seeded random poses,
  one hypothesis per object, eight objects per call"""
  rng = np.random.default_rng(50)
  lattice = (rng.integers(-1023, 1024, (8, 4, 4)) / 256.0).astype(np.float32)
  lattice[:, 3] = [0, 0, 0, 1]
  sets = [(lattice, (rng.integers(-1023, 1024, (8, 3)) / 256.0).astype(np.float32))]
  sets.append((R._pose_inputs(8, 51, 3)[0], (rng.standard_normal((8, 3)) * 0.05).astype(np.float32)))
  sets.append((_rank_poses(8, 52), rng.standard_normal((8, 3)).astype(np.float32)))
  for poses, centers in sets:
    got = _rank_call(fp, [np.array([1.0], dtype=np.float32)] * 8, [p[None] for p in poses], centers)
    for o in range(8):
      want = R.pose_of_mesh_fma(poses[o], centers[o])
      assert np.array_equal(_bits(got[o][3]), _bits(want)), f'object {o}: {got[o][3][:, 3]} vs {want[:, 3]}'
  exact = lattice[0].astype(np.float64)[:3, :3] @ -sets[0][1][0].astype(np.float64) + lattice[0][:3, 3]
  assert np.array_equal(R.pose_of_mesh_fma(lattice[0], sets[0][1][0])[:3, 3], exact)


def test_track_frame_pose_of_mesh_is_the_plain_order(fp):
  """fp_track_frame's d_pose_of_mesh (pose_of_mesh_one, in the fused tail of the last refinement pass): separate multiplies and adds from
  the left, on whatever pose the refiner arrives at - the frame only has to give it one."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.config import REFINE_DEFAULT, SCORE_DEFAULT
  from foundationpose_amd.estimater import FoundationPose
  from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
  from foundationpose_amd.predict_score import ScorePredictor
  from tests import cases
  refiner = PoseRefinePredictor(state_dict=S.make_refine_state_dict(cases.REFINE_SEED, head_gain=cases.GAIN_CHAIN), cfg=REFINE_DEFAULT)
  mesh = S.make_mustard_mesh(seed=0)
  mesh.vertices = mesh.vertices + np.array([0.0123, -0.0456, 0.0789])      # the synthetic mesh comes centred: move it
  np.random.seed(0)
  est = FoundationPose(model_pts=mesh.vertices, model_normals=mesh.vertex_normals, mesh=mesh, refiner=refiner,
                       scorer=ScorePredictor(state_dict=S.make_score_state_dict(cases.SCORE_SEED), cfg=SCORE_DEFAULT))
  center = np.asarray(est.model_center, dtype=np.float32)
  assert np.abs(center).max() > 1e-3                      # (an uncentred mesh: the translation column has work to do)
  rng = np.random.default_rng(70)
  rgb = rng.integers(0, 256, (480, 640, 3)).astype(np.uint8)
  depth = (0.75 + rng.standard_normal((480, 640)) * 0.002).astype(np.float32)
  start = R._pose_inputs(1, 71, 3)[0][0]
  start[:3, 3] = [0.01, -0.02, 0.75]
  est.pose_last = torch.from_numpy(start).cuda()
  got = est.track_one(rgb, depth, S.YCB_K, iteration=2)
  pose = est.pose_last.reshape(4, 4).cpu().numpy()
  assert np.isfinite(pose).all() and not np.array_equal(pose, start)
  assert np.array_equal(_bits(got), _bits(R.pose_of_mesh_plain(pose, center)))


# ------------------------------------------------------------------------------------------------------------------------------------------
# hypotheses
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_register_hypotheses_bit_equal(fp):
  L = fp['L']
  h = C['hypotheses']['skewed']
  want = R.hypotheses(**h)
  grids = [_dev(g) for g in h['rot_grids']]
  n_obj, ns = len(grids), [len(g) for g in h['rot_grids']]
  total = sum(ns)
  out = torch.full((total + 1, 4, 4), float('nan'), device='cuda')
  st = np.ascontiguousarray(h['stats'], dtype=np.int32)
  med = np.ascontiguousarray(h['medians'], dtype=np.float32)
  Kinv = np.ascontiguousarray(np.linalg.inv(h['K']), dtype=np.float64)
  L.check(L.lib().fp_register_hypotheses(fp['ctx'].handle, (ctypes.c_void_p * n_obj)(*[g.data_ptr() if len(g) else None for g in grids]), (ctypes.c_int * n_obj)(*ns),
                                         n_obj, st.ctypes.data, med.ctypes.data, Kinv.ctypes.data, L.ptr(out), L.stream_ptr()))
  torch.cuda.synchronize()
  got = out.cpu().numpy()
  assert np.isnan(got[total]).all()                       # the row behind the last object keeps its prefill
  bad = np.unique(np.nonzero(_bits(got[:total]) != _bits(want))[0])
  assert len(bad) == 0, f'rows {bad[:8]} differ: {got[bad[0]]} vs {want[bad[0]]}'
  # the empty object in the middle: its neighbours' rows are exactly the rows before and after offset 64, all written (no NaN left)
  assert ns[2] == 0 and not np.isnan(got[:total]).any()
  zero_rows = got[64:128, :3, 3]                          # object 3: median 0
  assert (zero_rows == 0).all()


def test_register_hypotheses_empty_object_alone_writes_nothing(fp):
  """n = 0 for every object: no launch, the output keeps its NaN prefill"""
  L = fp['L']
  h = C['hypotheses']['skewed']
  out = torch.full((4, 4, 4), float('nan'), device='cuda')
  st = np.ascontiguousarray(h['stats'][:2], dtype=np.int32)
  med = np.ascontiguousarray(h['medians'][:2], dtype=np.float32)
  Kinv = np.ascontiguousarray(np.linalg.inv(h['K']), dtype=np.float64)
  L.check(L.lib().fp_register_hypotheses(fp['ctx'].handle, (ctypes.c_void_p * 2)(None, None), (ctypes.c_int * 2)(0, 0), 2, st.ctypes.data, med.ctypes.data,
                                         Kinv.ctypes.data, L.ptr(out), L.stream_ptr()))
  torch.cuda.synchronize()
  assert np.isnan(out.cpu().numpy()).all()
