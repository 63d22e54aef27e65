"""GPU: fp_box_extents (csrc/bounds.hip) bit for bit against its numpy restatement (tests/oriented_bounds_oracle.py), and
Utils.oriented_bounds end to end against the float64 calipers yardstick of the same file.

The end-to-end bound is derived, not tuned.  Both sides start from the same float64 points.  The search evaluates a candidate in fp32:
the frame and the centred point are rounded once (u = 2^-24 relative each), a product rounds once and the two sums once each, so a
projection r.p is off by at most (3u + 2u) sum_j |r_j p_j| <= 5 u rho with rho = max |p| (|r| = 1), and an extent hi - lo by at most
DELTA = 10 u rho.  The three fp32 operations of the volume add a relative 3u, twice (winner and rival): 6u.  fp32 can therefore only make
the search pick a nearly tied candidate: with e* the extents of the float64 optimum c* and e' the float64 extents of the winner c',
  prod (e'_k - DELTA) <= vol32(c') (1 + 3u) <= vol32(c*) (1 + 3u) <= prod (e*_k + DELTA) (1 + 6u),  so
  V = prod e'_k <= V_ref * prod (1 + DELTA / e*_k) / prod (1 - DELTA / e'_k) * (1 + 6u)
which is V_ref * prod (1 + 2 DELTA / e_k) to first order.  The yardstick merges hull normals at 9 decimals and the search at 10: two
frames of "one" face differ by a tilt below 1e-9 rad, a relative 1e-9 rho / e_k per extent, covered by a further factor (1 + 1e-8).  For
the mustard mesh (rho = 0.11, e = 0.061 .. 0.19) the whole factor is about 1 + 4e-6."""
import os

import numpy as np
import pytest
import torch

from tests import oriented_bounds_oracle as O

pytestmark = pytest.mark.gpu
T = 1024          # FP_BOX_EXTENTS_TILE: the points of an LDS tile
B = 1024          # FP_BOX_EXTENTS_CAND: the candidates of a workgroup (256 lanes x 4 frames)
U24 = 2.0 ** -24
# the float64 minimum a numpy prototype of the search found for the mustard mesh, m^3.  The yardstick reproduces it (1.1821185070665e-3,
# 6 720 distinct hull normals) on the vertices ROUNDED TO FLOAT32; on the float64 vertices, which the tests use, the hull has 3 456
# distinct normals and the minimum is 1.1821185143545e-3, a relative 6e-9 above it
PROTOTYPE_MUSTARD_MIN = 1.182118507e-3


def test_constants_are_the_librarys():
  from foundationpose_amd import _lib
  assert (T, B) == (_lib.FP_BOX_EXTENTS_TILE, _lib.FP_BOX_EXTENTS_CAND)


def _frames(C, seed):
  """C seeded rotations rounded to float32 (rows orthonormal to fp32's precision: the primitive does not ask for more)"""
  q = np.linalg.qr(np.random.RandomState(seed).randn(C, 3, 3))[0]
  return np.ascontiguousarray(q, dtype=np.float32)


def _cloud(n, seed, shift):
  p = np.random.RandomState(seed).randn(n, 3) * np.array([0.11, 0.06, 0.03])
  p += {'neg': -1.0, 'pos': 1.0, 'none': 0.0}[shift]                   # every coordinate below / above 0: a bound that starts at 0 shows
  p = p.astype(np.float32)
  if shift != 'none':
    assert ((p < 0).all() if shift == 'neg' else (p > 0).all())
  return p


def _same_bits(a, b):
  return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def _check(got, want, label):
  assert got['index'] == want['index'], f'{label}: winner {got["index"]}, oracle {want["index"]}'
  for k in ('lo', 'hi', 'volume', 'all_lohi', 'all_volume'):
    assert _same_bits(got[k], want[k]), f'{label}: {k} differs from the oracle'


# two point slices with a ragged last one: a launch of up to 3 candidate workgroups cuts the points into slices of one tile up to
# 342 tiles, so T + 3 points are two slices, the second of 3 points
N_POINTS = [1, 5, T - 1, T, T + 3, 2 * T + 7]
N_CAND = [1, 3, B - 1, B + 1, 2 * B + 5]


@pytest.mark.parametrize('shift', ['neg', 'pos'])
@pytest.mark.parametrize('C', N_CAND)
@pytest.mark.parametrize('n', N_POINTS)
def test_bits_against_the_oracle(n, C, shift):
  from foundationpose_amd import Utils as U
  pts, fr = _cloud(n, seed=n, shift=shift), _frames(C, seed=C)
  _check(U.box_extents(pts, fr, return_all=True), O.box_extents_f32(pts, fr), f'n={n} C={C} {shift}')


@pytest.mark.parametrize('C', [1, 3])
def test_slices_of_several_tiles(C):
  """Few candidates against many points: one candidate workgroup takes 1024 slices at most, so 1025 tiles and 5 points are 513 slices of
  two tiles, the last of T + 5 points - the loop over the tiles of a slice, and a ragged tile behind a full one."""
  from foundationpose_amd import Utils as U
  n = 1025 * T + 5
  pts, fr = _cloud(n, seed=9, shift='none'), _frames(C, seed=40 + C)
  _check(U.box_extents(pts, fr, return_all=True), O.box_extents_f32(pts, fr), f'n={n} C={C}')


@pytest.mark.parametrize('n', [T + 3, 2 * T + 7])
def test_extreme_point_is_the_very_last(n):
  from foundationpose_amd import Utils as U
  pts, fr = _cloud(n, seed=5, shift='none'), np.concatenate([np.eye(3, dtype=np.float32)[None], _frames(B + 1, seed=6)])
  pts[n - 1] = (7.0, -9.0, 11.0)
  got = U.box_extents(pts, fr, return_all=True)
  _check(got, O.box_extents_f32(pts, fr), f'n={n}')
  assert got['all_lohi'][0, 3] == 7.0 and got['all_lohi'][0, 1] == -9.0 and got['all_lohi'][0, 5] == 11.0


def _cube():
  return np.array([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], dtype=np.float32)


def test_ties_go_to_the_lowest_index():
  """The unit cube's corners; the identity at 0, B - 1, B and 2B + 4 (volume 1), twice the identity elsewhere (volume 8): every number
  is exact in fp32.  The ties lie in one lane's registers, across the lanes of a workgroup and across workgroups."""
  from foundationpose_amd import Utils as U
  eye = np.eye(3, dtype=np.float32)
  fr = np.tile(2 * eye, (2 * B + 5, 1, 1))
  fr[[0, B - 1, B, 2 * B + 4]] = eye
  got = U.box_extents(_cube(), fr, return_all=True)
  assert got['index'] == 0 and got['volume'] == 1.0
  np.testing.assert_array_equal(np.unique(got['all_volume']), [1.0, 8.0])
  np.testing.assert_array_equal(np.flatnonzero(got['all_volume'] == 1.0), [0, B - 1, B, 2 * B + 4])
  fr[0] = 2 * eye
  got = U.box_extents(_cube(), fr)
  assert got['index'] == B - 1 and got['volume'] == 1.0
  np.testing.assert_array_equal(np.r_[got['lo'], got['hi']], [0, 0, 0, 1, 1, 1])
  fr[[B - 1, B]] = 2 * eye
  assert U.box_extents(_cube(), fr)['index'] == 2 * B + 4
  # a NaN volume never wins, nor a candidate that saw no finite projection; none left: -1
  fr[:] = np.nan
  assert U.box_extents(_cube(), fr)['index'] == -1
  fr[B + 7] = eye
  _check(U.box_extents(_cube(), fr, return_all=True), O.box_extents_f32(_cube(), fr), 'NaN frames')
  assert U.box_extents(_cube(), fr)['index'] == B + 7


def test_null_outputs_tensors_and_batches():
  from foundationpose_amd import Utils as U
  n, C = T + 3, B + 1
  pts, fr = _cloud(n, seed=2, shift='neg'), _frames(C, seed=3)
  full = U.box_extents(pts, fr, return_all=True)
  lean = U.box_extents(pts, fr)                                        # null optional outputs
  assert lean['index'] == full['index'] and all(_same_bits(lean[k], full[k]) for k in ('lo', 'hi', 'volume'))
  assert 'all_lohi' not in lean
  dev = U.box_extents(torch.as_tensor(pts, device='cuda'), torch.as_tensor(fr, device='cuda'), return_all=True)
  assert torch.is_tensor(dev['all_lohi']) and dev['all_lohi'].is_cuda and dev['index'] == full['index']
  assert _same_bits(dev['all_lohi'].cpu().numpy(), full['all_lohi']) and _same_bits(dev['all_volume'].cpu().numpy(), full['all_volume'])
  # the same candidates inside a larger batch, at other indices, lanes and workgroups
  before, after = _frames(B + 37, seed=4), _frames(5, seed=5)
  big = U.box_extents(pts, np.concatenate([before, fr, after]), return_all=True)
  assert _same_bits(big['all_lohi'][len(before):len(before) + C], full['all_lohi'])
  assert _same_bits(big['all_volume'][len(before):len(before) + C], full['all_volume'])
  assert U.box_extents(pts, fr, return_all=True)['index'] == full['index']      # and again: the same


def _raw(ctx, pts, n, fr, C, idx, lohi, vol, all_lohi=None, all_vol=None):
  from foundationpose_amd import _lib
  return _lib.lib().fp_box_extents(ctx, _lib.ptr(pts), n, _lib.ptr(fr), C, _lib.ptr(idx), _lib.ptr(lohi), _lib.ptr(vol), _lib.ptr(all_lohi),
                                   _lib.ptr(all_vol), _lib.stream_ptr('cuda'))


def test_captured_in_a_graph_and_replayed():
  """fp_box_extents synchronises nothing: one linear chain of three launches, captured on a stream and replayed on new points."""
  from foundationpose_amd import _lib
  n, C = 3 * T + 11, B + 5
  ctx = _lib.Context.get('cuda')
  fr_h = _frames(C, seed=8)
  pts, fr = torch.as_tensor(_cloud(n, seed=1, shift='none'), device='cuda'), torch.as_tensor(fr_h, device='cuda')
  idx = torch.zeros(1, dtype=torch.int32, device='cuda')
  lohi, vol = torch.zeros(6, device='cuda'), torch.zeros(1, device='cuda')
  all_lohi, all_vol = torch.zeros((C, 6), device='cuda'), torch.zeros(C, device='cuda')
  call = lambda: _lib.check(_raw(ctx.handle, pts, n, fr, C, idx, lohi, vol, all_lohi, all_vol))
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    call()                                           # eager first: the context's arena is allocated outside the capture
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    call()
  for seed in (2, 3):
    fresh = _cloud(n, seed=seed, shift='pos' if seed == 2 else 'neg')
    pts.copy_(torch.as_tensor(fresh))
    for t in (idx, lohi, vol, all_lohi, all_vol):
      t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = dict(index=int(idx.item()), lo=lohi[:3].cpu().numpy(), hi=lohi[3:].cpu().numpy(), volume=vol.cpu().numpy()[0],
               all_lohi=all_lohi.cpu().numpy(), all_volume=all_vol.cpu().numpy())
    _check(got, O.box_extents_f32(fresh, fr_h), f'replay {seed}')


def test_rejects_bad_arguments_and_launches_nothing():
  from foundationpose_amd import _lib
  ctx = _lib.Context.get('cuda').handle
  pts, fr = torch.zeros((8, 3), device='cuda'), torch.zeros((4, 3, 3), device='cuda')
  idx = torch.full((1,), -77, dtype=torch.int32, device='cuda')
  lohi, vol = torch.full((6,), -77.0, device='cuda'), torch.full((1,), -77.0, device='cuda')
  E = _lib.FP_EINVAL
  assert _raw(None, pts, 8, fr, 4, idx, lohi, vol) == E
  assert _raw(ctx, None, 8, fr, 4, idx, lohi, vol) == E
  assert _raw(ctx, pts, 8, None, 4, idx, lohi, vol) == E
  assert _raw(ctx, pts, 8, fr, 4, None, lohi, vol) == E
  assert _raw(ctx, pts, 8, fr, 4, idx, None, vol) == E
  assert _raw(ctx, pts, 8, fr, 4, idx, lohi, None) == E
  assert _raw(ctx, pts, 0, fr, 4, idx, lohi, vol) == E
  assert _raw(ctx, pts, -1, fr, 4, idx, lohi, vol) == E
  assert _raw(ctx, pts, 8, fr, 0, idx, lohi, vol) == E
  assert _raw(ctx, pts, 8, fr, -3, idx, lohi, vol) == E
  assert _raw(ctx, pts, _lib.FP_BOX_EXTENTS_MAX_POINTS + 1, fr, 4, idx, lohi, vol) == E
  assert _raw(ctx, pts, 8, fr, _lib.FP_BOX_EXTENTS_MAX_FRAMES + 1, idx, lohi, vol) == E
  assert _raw(ctx, pts, 1 << 21, fr, 1 << 20, idx, lohi, vol) == E         # n C = 2^41 > FP_BOX_EXTENTS_MAX_EVALS
  assert (1 << 21) * (1 << 20) > _lib.FP_BOX_EXTENTS_MAX_EVALS
  torch.cuda.synchronize()
  assert int(idx.item()) == -77 and (lohi == -77).all() and (vol == -77).all()      # nothing ran
  assert _raw(ctx, pts, 8, fr, 4, idx, lohi, vol) == 0
  torch.cuda.synchronize()
  assert int(idx.item()) == 0 and float(vol.item()) == 0.0


# ---------------------------------------------------------------------------------------------- oriented_bounds end to end
def test_rotated_box_end_to_end():
  from foundationpose_amd import Utils as U
  pts = O.rotated_box()
  to_origin, extents, info = U.oriented_bounds(pts, return_info=True)
  print(f'extents {extents!r} volume {info["volume"]!r} candidates {info["n_candidates"]} hull vertices {info["hull_vertices"]}')
  np.testing.assert_allclose(extents, O.BOX, rtol=1e-6, atol=0)
  q = pts @ to_origin[:3, :3].T + to_origin[:3, 3]
  assert (np.abs(q) <= extents / 2 * (1 + 1e-12)).all() and abs(np.linalg.det(to_origin[:3, :3]) - 1) <= 1e-12
  # a device tensor and a mesh object give the same
  class Mesh:
    vertices = pts
  np.testing.assert_array_equal(U.oriented_bounds(torch.as_tensor(pts, device='cuda'))[0], to_origin)
  np.testing.assert_array_equal(U.model_box(Mesh(), oriented=True)[1], [-extents / 2, extents / 2])
  np.testing.assert_array_equal(U.model_box(Mesh(), oriented=True)[0], to_origin)


@pytest.fixture(scope='module')
def mustard():
  from foundationpose_amd import synthetic as S
  v = np.asarray(S.make_mustard_mesh(seed=0).vertices, dtype=np.float64)
  assert len(v) == 8066
  return v


@pytest.mark.parametrize('turned', [False, True])
def test_mustard_against_the_calipers_yardstick(mustard, turned):
  from foundationpose_amd import Utils as U
  pts = mustard @ O.rotvec_matrix(O.ROTVEC).T + O.SHIFT if turned else mustard
  to_origin, extents, info = U.oriented_bounds(pts, return_info=True)
  R = to_origin[:3, :3]
  q = pts @ R.T + to_origin[:3, 3]
  assert (np.abs(q) <= extents / 2 * (1 + 1e-12)).all()               # the box contains every vertex
  assert abs(np.linalg.det(R) - 1) <= 1e-12 and (np.diff(extents) >= 0).all()
  V = float(np.prod(extents))
  assert V == info['volume'] and V <= info['aabb_volume'] and V <= info['pca_volume']
  # (the vectorised form of the yardstick: tests/test_oriented_bounds_host.py holds it equal to the pointer-walking calipers)
  V_ref, rows, n_normals = O.calipers_min_volume(pts, brute=True)
  centred = pts - (pts.min(axis=0) + pts.max(axis=0)) / 2
  rho = float(np.linalg.norm(centred, axis=1).max())
  delta = 10 * U24 * rho
  e_ref = np.ptp(centred @ rows.T, axis=0)
  factor = float(np.prod(1 + delta / e_ref) / np.prod(1 - delta / extents) * (1 + 6 * U24) * (1 + 1e-8))
  print(f'turned={turned}: V={V!r} V_ref={V_ref!r} ratio={V / V_ref!r} derived factor={factor!r}; prototype minimum {PROTOTYPE_MUSTARD_MIN!r} '
        f'(V / prototype = {V / PROTOTYPE_MUSTARD_MIN!r}); aabb {info["aabb_volume"]:.6e} pca {info["pca_volume"]:.6e}; '
        f'{info["n_candidates"]} candidates, {info["hull_vertices"]} hull vertices, {n_normals} normals, extents {extents!r}')
  assert V <= V_ref * factor
  assert V >= V_ref * (1 - 1e-8)                                      # the yardstick is the minimum of the class


# ---------------------------------------------------------------------------------------------- wiring
@pytest.fixture(scope='module')
def nets():
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.config import REFINE_DEFAULT, SCORE_DEFAULT
  from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
  from foundationpose_amd.predict_score import ScorePredictor
  from tests import cases
  return (PoseRefinePredictor(state_dict=S.make_refine_state_dict(0, head_gain=cases.GAIN_CHAIN), cfg=REFINE_DEFAULT),
          ScorePredictor(state_dict=S.make_score_state_dict(1), cfg=SCORE_DEFAULT))


def _turned_mesh():
  """The small mustard mesh with its axes turned away from its box: the oriented and the axis-aligned box differ"""
  from foundationpose_amd import synthetic as S
  mesh = S.make_mustard_mesh(seed=0, n_theta=48, n_z=42)
  Rm = O.rotvec_matrix(O.ROTVEC)
  mesh.vertices = np.asarray(mesh.vertices) @ Rm.T + np.array([0.02, -0.01, 0.03])
  return mesh


def test_estimator_model_box_is_cached(nets, monkeypatch):
  from foundationpose_amd import Utils as U
  from foundationpose_amd.estimater import FoundationPose
  mesh = _turned_mesh()
  np.random.seed(0)
  est = FoundationPose(model_pts=mesh.vertices, model_normals=mesh.vertex_normals, mesh=mesh, refiner=nets[0], scorer=nets[1])
  calls = []
  real = U.oriented_bounds
  monkeypatch.setattr(U, 'oriented_bounds', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
  to_origin, bbox = est.model_box(oriented=True)
  again = est.model_box(oriented=True)
  assert len(calls) == 1
  np.testing.assert_array_equal(again[0], to_origin), np.testing.assert_array_equal(again[1], bbox)
  want = real(mesh.vertices)
  np.testing.assert_array_equal(to_origin, want[0]), np.testing.assert_array_equal(bbox, [-want[1] / 2, want[1] / 2])
  to_origin[:] = 0                                                    # a copy was returned: the cache is not the caller's to spoil
  np.testing.assert_array_equal(est.model_box(oriented=True)[0], want[0])
  assert est.instance().model_box(oriented=True)[1].shape == (2, 3) and len(calls) == 1      # instances share the object's box
  plain = est.model_box()
  np.testing.assert_array_equal(plain[0], U.model_box(mesh)[0]), np.testing.assert_array_equal(plain[1], U.model_box(mesh)[1])
  assert np.prod(bbox[1] - bbox[0]) < 0.6 * np.prod(plain[1][1] - plain[1][0])
  est.reset_object(mesh.vertices, mesh.vertex_normals, mesh=mesh)
  est.model_box(oriented=True)
  assert len(calls) == 2                                              # reset_object clears it


def test_pipeline_sets_center_pose_and_draws_the_oriented_box(nets):
  from foundationpose_amd import Utils as U
  from foundationpose_amd.pipeline import FoundationPoseEstimator, Pipeline, PipelineData, Processor
  from tests import util
  sc = util.scene(0)
  mesh = _turned_mesh()

  class Frame(Processor):
    def process(self, data):
      data.rgb, data.depth, data.K, data.mask = sc['rgb'], sc['depth'], sc['K'], sc['mask']
      return data
  stage = FoundationPoseEstimator(mesh=mesh, K=sc['K'], est_refine_iter=1, scorer=nets[1], refiner=nets[0], box='oriented')
  np.random.seed(0)
  data = Pipeline('demo', stop_on_error=True, visualize=True).add_processor(Frame()).add_processor(stage).run(PipelineData())
  assert not data.errors
  to_origin, extents = U.oriented_bounds(mesh)
  np.testing.assert_array_equal(data.center_pose, np.asarray(data.pose, dtype=np.float64).reshape(4, 4) @ np.linalg.inv(to_origin))
  want = U.draw_poses(data.rgb, sc['K'], np.asarray(data.pose, dtype=np.float64).reshape(1, 4, 4), bboxes=np.stack([-extents / 2, extents / 2]),
                      offsets=np.linalg.inv(to_origin), colors=(0, 255, 0))
  assert np.array_equal(data.vis, want) and not np.array_equal(data.vis, data.rgb)
  # the default stage leaves center_pose alone
  plain = FoundationPoseEstimator(mesh=mesh, K=sc['K'], est_refine_iter=1, scorer=nets[1], refiner=nets[0])
  assert plain.box == 'aabb' and PipelineData().center_pose is None


def test_draw_poses_with_the_oriented_pair_equals_the_draw_oracle():
  """The draw kernel is unchanged: this checks the plumbing of (to_origin, extents) into bboxes and offsets."""
  from foundationpose_amd import Utils as U, synthetic as S
  from tests import draw_oracle as D
  from tests import util
  from tests.test_gpu_draw_poses import _compare
  img = np.ascontiguousarray(util.scene(0)['rgb'])
  K = np.asarray(S.YCB_K, dtype=np.float64)
  mesh = _turned_mesh()
  to_origin, bbox = U.model_box(mesh, oriented=True)
  off = np.linalg.inv(to_origin)
  pose = np.eye(4, dtype=np.float32)
  pose[:3, :3] = S.random_rotation(np.random.RandomState(31))
  pose[:3, 3] = [0.03, -0.02, 0.62]
  obj = D.make_object(bbox.astype(np.float32), off.astype(np.float32), axis_scale=0.1, box_color=U.DRAW_PALETTE[0], axis_color=np.eye(3, dtype=np.uint8) * 255)
  want, touched, segs = D.draw(img, K, pose[None], [obj])
  assert D.endpoint_margin(segs) > 1e-6, 'pick another pose: an endpoint lies at a rounding tie'
  got = U.draw_poses(img, K, pose[None], bboxes=bbox, offsets=off)
  _compare(got, img, want, touched, 'oriented box')
  aabb = U.model_box(mesh)
  assert not np.array_equal(got, U.draw_poses(img, K, pose[None], bboxes=aabb[1], offsets=np.linalg.inv(aabb[0])))


def test_command_line_tool_prints_one_json_line(tmp_path, capsys, monkeypatch):
  """scripts/oriented_bounds.py MODEL --scale S, run in this process on the rotated box written as an OBJ in millimetres"""
  import json
  import runpy
  import sys
  from scipy.spatial import ConvexHull
  from foundationpose_amd import Utils as U, mesh_io, synthetic as S
  pts = O.rotated_box()
  mesh = S.SimpleMesh(pts * 1000.0, ConvexHull(pts).simplices.astype(np.int64))
  path = str(tmp_path / 'box.obj')
  mesh_io.save_obj(mesh, path)
  script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts', 'oriented_bounds.py')
  monkeypatch.setattr(sys, 'argv', [script, path, '--scale', '0.001'])
  runpy.run_path(script, run_name='__main__')
  lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')]
  assert len(lines) == 1
  rec = json.loads(lines[0])
  np.testing.assert_allclose(rec['extents'], O.BOX, rtol=1e-5)
  assert np.asarray(rec['to_origin']).shape == (4, 4) and rec['hull_vertices'] == 8 and rec['n_candidates'] >= 1
  assert rec['volume'] <= rec['pca_volume'] and rec['volume'] < rec['aabb_volume']
