"""GPU: posing views from depth alone (fp_depth_normals and fp_depth_pairs_align in csrc/depth_icp.hip; depth_normals, align_pairs_step,
joint_refine_view_poses and estimate_view_poses in foundationpose_amd/reconstruct.py) against the numpy restatement of the header's
rules (tests/depth_icp_oracle.py): normals and per-pixel rows bit for bit, the sums within the bound of any summation order of exact
terms, the two procedures against the restatement's recorded runs, and through reconstruct_object and the script.

Shapes: 5 views of 64 x 48 of the three spheres on an arc plus a pushed copy of the last (3 tiles of 1024 pixels per pair, 16 directed
pairs) and of 53 x 37 (1961 pixels: a ragged last tile, image rows that straddle tiles)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import depth_icp_oracle as D
from tests import tsdf_align_oracle as A
from tests import tsdf_oracle as O

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
  return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _case(*size):
  K, truth, depths, masks, query, pairs = D.row_case(*size)
  return dict(K=K, truth=truth, depths=depths, masks=masks, query=query, pairs=pairs)


@pytest.fixture(scope='module')
def case():
  return _case()


@pytest.fixture(scope='module')
def oracle_step(case):
  nrm = np.stack([D.normals(case['depths'][v], case['K'], case['masks'][v]) for v in range(6)])
  out = [D.pair_rows(case['depths'], nrm, case['K'], case['query'], s, t, *D.ROW_GATE, reasons=True) for s, t in case['pairs']]
  return nrm, np.stack([o[0] for o in out]), [{k: int(o[1][k].sum()) for k in D.SKIPS} for o in out]


@pytest.fixture(scope='module')
def device_step(case):
  from foundationpose_amd import reconstruct as R
  nrm = R.depth_normals(case['depths'], case['K'], case['masks'])
  depths = torch.as_tensor(case['depths'], device=nrm.device)
  sums, rows = R.align_pairs_step(depths, nrm, case['K'], case['query'], case['pairs'], *D.ROW_GATE, rows=True)
  return nrm, depths, sums, rows


def test_normals_are_bit_equal_with_masks_and_borders_are_zero(case, oracle_step, device_step):
  want, got = oracle_step[0], device_step[0].cpu().numpy()
  print(f'{int(want[..., 3].sum())} normals of {want[..., 3].size} pixels; differing words {(got.view(np.uint32) != want.view(np.uint32)).sum()}')
  assert all(want[v, ..., 3].sum() >= 300 for v in range(6))
  assert _same_bits(got, want)
  assert (got[:, 0] == 0).all() and (got[:, -1] == 0).all() and (got[:, :, 0] == 0).all() and (got[:, :, -1] == 0).all()
  assert (got[..., 2][got[..., 3] != 0] < 0).all()
  # 66 views (the 6 of the case 11 times) are cut into calls of 64 and 2: every copy gets the bits of its original
  from foundationpose_amd import reconstruct as R
  many = R.depth_normals(np.concatenate([case['depths']] * 11), case['K'], np.concatenate([case['masks']] * 11))
  assert torch.equal(many, torch.cat([device_step[0]] * 11))


def test_normals_on_a_ragged_image_with_zfar_nan_and_negative_depth():
  """53 x 37 pixels without masks; then a zfar that cuts part of the scene; then one NaN and one negative depth pixel inside a sphere:
  each takes the normals of itself and its four neighbours away and nothing else."""
  from foundationpose_amd import reconstruct as R
  c = _case(37, 53, 108.0)
  want = np.stack([D.normals(c['depths'][v], c['K']) for v in range(6)])
  assert all(want[v, ..., 3].sum() >= 200 for v in range(6))
  assert _same_bits(R.depth_normals(c['depths'], c['K']).cpu().numpy(), want)
  zfar = float(np.median(c['depths'][c['depths'] > 0]))
  cut = np.stack([D.normals(c['depths'][v], c['K'], zfar=zfar) for v in range(6)])
  assert all(20 <= cut[v, ..., 3].sum() < 0.8 * want[v, ..., 3].sum() for v in range(6))
  assert _same_bits(R.depth_normals(c['depths'], c['K'], zfar=zfar).cpu().numpy(), cut)
  bad = c['depths'].copy()
  r0, c0 = np.argwhere(want[0, ..., 3] != 0)[len(np.argwhere(want[0, ..., 3] != 0)) // 2]
  inner = [(r, cc) for r, cc in np.argwhere(want[1, ..., 3] != 0) if want[1, r - 1:r + 2, cc - 1:cc + 2, 3].all()]
  r1, c1 = inner[len(inner) // 2]
  bad[0, r0, c0], bad[1, r1, c1] = np.nan, -0.3
  hurt = np.stack([D.normals(bad[v], c['K']) for v in range(6)])
  assert hurt[1, ..., 3].sum() == want[1, ..., 3].sum() - 5 and hurt[0, ..., 3].sum() < want[0, ..., 3].sum()
  got = R.depth_normals(bad, c['K']).cpu().numpy()
  assert _same_bits(got, hurt) and np.isfinite(got).all()


def test_rows_are_bit_equal_and_counts_equal(case, oracle_step, device_step):
  _, want, why = oracle_step
  total = {k: sum(w[k] for w in why) for k in D.SKIPS}
  print(f'valid per pair {[int(w[..., 7].sum()) for w in want]}; skipped {total}')
  assert all(total[k] > 0 for k in D.SKIPS)
  got = device_step[3].cpu().numpy()
  print(f'differing words: {(got.view(np.uint32) != want.view(np.uint32)).sum()} of {want.size}')
  assert _same_bits(got, want)
  assert np.array_equal(device_step[2][:, 28], want[..., 7].reshape(len(want), -1).sum(1))


def test_rows_and_counts_on_a_ragged_image_without_masks():
  from foundationpose_amd import reconstruct as R
  c = _case(37, 53, 108.0)
  nrm = np.stack([D.normals(c['depths'][v], c['K']) for v in range(6)])
  want = np.stack([D.pair_rows(c['depths'], nrm, c['K'], c['query'], s, t, *D.ROW_GATE) for s, t in c['pairs']])
  assert sum(w[..., 7].sum() >= 90 for w in want) >= 12
  dn = R.depth_normals(c['depths'], c['K'])
  sums, got = R.align_pairs_step(torch.as_tensor(c['depths'], device=dn.device), dn, c['K'], c['query'], c['pairs'], *D.ROW_GATE, rows=True)
  assert _same_bits(got.cpu().numpy(), want)
  assert np.array_equal(sums[:, 28], want[..., 7].reshape(len(want), -1).sum(1))


def test_sums_are_within_the_bound_of_any_summation_order(oracle_step, device_step):
  """Every term is a product of two fp32 numbers, exact in double; n exact terms added in double in any order differ from the exactly
  rounded sum (math.fsum) by at most (n - 1) 2^-53 sum |terms| (1 + O(2^-53)) - the bound asserted is n 2^-52 sum |terms|, as in
  tests/test_gpu_tsdf_align.py.  The count is a sum of ones: exact."""
  worst = 0.0
  for k, rw in enumerate(oracle_step[1]):
    ref, scale = D.sums(rw)
    n = ref[28]
    err = np.abs(device_step[2][k] - ref)
    bound = n * 2.0 ** -52 * scale
    if n:
      worst = max(worst, (err[:28] / np.maximum(bound[:28], 1e-300)).max())
    assert (err <= bound).all(), (k, err, bound)
    assert device_step[2][k, 28] == n
  print(f'largest |sum - fsum| / bound: {worst:.3e}')


@pytest.mark.parametrize('make', [lambda: D.row_case(96, 100, 200.0), D.tiny_case, D.row_case, lambda: D.tiny_case(K=O.skew_camera(5, 7, 130.0))],
                         ids=['96x100', '5x7', 'masked 48x64', '5x7 fx != fy'])
def test_sums_have_the_bits_of_the_stated_order(make):
  """The device's sums against tests/gn_sums_oracle.py (the order stated in csrc/gn_sums.h) applied to the device's own rows, bit for
  bit.  96 x 100: 10 tiles - the fold's body of eight and a remainder of two - and a last tile of 384 pixels; 5 x 7: one tile of which
  three waves hold padding only (depth_icp_oracle.tiny_case); the masked row case of 48 x 64: whole waves without a source normal,
  which take the kernel's short cut."""
  from foundationpose_amd import reconstruct as R
  from tests import gn_sums_oracle as G
  c = dict(zip(('K', 'truth', 'depths', 'masks', 'query', 'pairs'), make()))
  nrm = R.depth_normals(c['depths'], c['K'], c['masks'])
  sums, rows = R.align_pairs_step(torch.as_tensor(c['depths'], device=nrm.device), nrm, c['K'], c['query'], c['pairs'], *D.ROW_GATE, rows=True)
  rows = rows.cpu().numpy()
  want = np.stack([G.device_sums(rows[p]) for p in range(len(c['pairs']))])
  print(f'{rows.shape[1:3]}: valid per pair {sums[:, 28]}; differing words {(sums.view(np.uint64) != want.view(np.uint64)).sum()} of {want.size}')
  assert sums[:, 28].sum() > 0
  assert np.array_equal(sums.view(np.uint64), want.view(np.uint64))


def test_normals_and_rows_under_a_camera_with_fx_not_fy():
  """The 5 x 7 case through tsdf_oracle.skew_camera (fy = 1.25 fx, cx and cy off the middle by different amounts): a kernel that takes
  fx for fy or cx for cy anywhere - the rays of the normals, the back-projections, the projection - differs from the restatement.
  Every pair has valid pixels."""
  from foundationpose_amd import reconstruct as R
  c = dict(zip(('K', 'truth', 'depths', 'masks', 'query', 'pairs'), D.tiny_case(K=O.skew_camera(5, 7, 130.0))))
  assert c['K'][0, 0] != c['K'][1, 1] and c['K'][0, 2] - 3.0 != c['K'][1, 2] - 2.0
  nrm = np.stack([D.normals(c['depths'][v], c['K'], c['masks'][v]) for v in range(6)])
  want = np.stack([D.pair_rows(c['depths'], nrm, c['K'], c['query'], s, t, *D.ROW_GATE) for s, t in c['pairs']])
  print(f'valid per pair {[int(w[..., 7].sum()) for w in want]}')
  assert all(w[..., 7].sum() > 0 for w in want)
  dn = R.depth_normals(c['depths'], c['K'], c['masks'])
  assert _same_bits(dn.cpu().numpy(), nrm)
  sums, got = R.align_pairs_step(torch.as_tensor(c['depths'], device=dn.device), dn, c['K'], c['query'], c['pairs'], *D.ROW_GATE, rows=True)
  assert _same_bits(got.cpu().numpy(), want)
  assert np.array_equal(sums[:, 28], want[..., 7].reshape(len(want), -1).sum(1))


def test_a_pair_does_not_depend_on_its_batch(case, device_step):
  from foundationpose_amd import _lib
  from foundationpose_amd import reconstruct as R
  nrm, depths, sums, rows = device_step
  step = lambda pr, **kw: R.align_pairs_step(depths, nrm, case['K'], case['query'], pr, *D.ROW_GATE, **kw)
  pairs = case['pairs']
  assert np.array_equal(step(pairs), sums)                                              # two runs
  assert np.array_equal(step(pairs[3:4])[0], sums[3])                                   # alone
  order = [3, 0, 1, 2] + list(range(4, 16))
  assert np.array_equal(step([pairs[i] for i in order]), sums[order])                   # at another index
  order = list(range(15, -1, -1))
  assert np.array_equal(step([pairs[i] for i in order]), sums[order])
  twice = step([pairs[0], pairs[7], pairs[0], pairs[0]])
  assert np.array_equal(twice, sums[[0, 7, 0, 0]])                                      # a repeated pair
  reps = 17
  assert 16 * reps > _lib.FP_DEPTH_ALIGN_MAX_PAIRS                                      # 272 pairs: calls of 256 and 16
  many = step(pairs * reps)
  assert np.array_equal(many, np.concatenate([sums] * reps))
  cut = _lib.FP_DEPTH_ALIGN_MAX_PAIRS
  _, tail = step((pairs * reps)[cut - 2:cut + 3], rows=True)                            # the rows of the same pairs in another, shorter batch
  assert torch.equal(tail, rows[[(cut - 2 + i) % 16 for i in range(5)]])
  assert (sums[:12, 28] >= 150).all() and len(np.unique(sums[:12, 27])) == 12


def test_zero_pairs_write_nothing(case, device_step):
  from foundationpose_amd import _lib
  from foundationpose_amd import reconstruct as R
  from foundationpose_amd._lib import lib, ptr, stream_ptr
  nrm, depths, _, _ = device_step
  ctx = _lib.Context.get(nrm.device)
  sums = np.full(29, 7.0)
  K, poses = np.ascontiguousarray(case['K']), np.ascontiguousarray(case['query'])
  rc = lib().fp_depth_pairs_align(ctx.handle, ptr(depths), ptr(nrm), 6, 48, 64, ptr(K), ptr(poses), None, 0, 0.01, 0.5, None, ptr(sums),
                                  stream_ptr(nrm.device))
  assert rc == 0 and (sums == 7.0).all()
  assert R.align_pairs_step(depths, nrm, K, poses, [], 0.01, 0.5).shape == (0, 29)
  keep = torch.full((1, 4, 4, 4), 3.0, device=nrm.device)
  rc = lib().fp_depth_normals(ctx.handle, ptr(depths), None, 0, 4, 4, ptr(K), 1.0, 0.01, ptr(keep), stream_ptr(nrm.device))
  assert rc == 0 and (keep == 3.0).all()


def test_misaligned_buffers_are_refused(case, device_step):
  from foundationpose_amd import _lib
  from foundationpose_amd._lib import lib, ptr, stream_ptr
  nrm, depths, sums0, _ = device_step
  dev = nrm.device
  ctx = _lib.Context.get(dev)
  K, poses = np.ascontiguousarray(case['K']), np.ascontiguousarray(case['query'])
  pr = np.array([case['pairs'][0]], dtype=np.int32)
  sums = np.zeros(29)
  buf = torch.zeros(48 * 64 * 8 + 4, device=dev)
  nbuf = torch.zeros(6 * 48 * 64 * 4 + 4, device=dev)
  assert buf.data_ptr() % 16 == 0 and nbuf.data_ptr() % 16 == 0
  nbuf[4:] = nrm.reshape(-1)                                                             # the normals at a 16-byte offset
  pairs_call = lambda n_off, r_off: lib().fp_depth_pairs_align(ctx.handle, ptr(depths), ctypes.c_void_p(nbuf.data_ptr() + n_off), 6, 48, 64, ptr(K),
                                                               ptr(poses), ptr(pr), 1, D.ROW_GATE[0], D.ROW_GATE[1],
                                                               ctypes.c_void_p(buf.data_ptr() + r_off), ptr(sums), stream_ptr(dev))
  assert pairs_call(16, 4) == _lib.FP_EINVAL and b'aligned' in lib().fp_last_error() and (buf == 0).all()
  assert pairs_call(4, 16) == _lib.FP_EINVAL and b'aligned' in lib().fp_last_error() and (buf == 0).all()
  assert pairs_call(16, 16) == 0 and np.array_equal(sums, sums0[0])
  out = torch.zeros(6 * 48 * 64 * 4 + 4, device=dev)
  normals_call = lambda off: lib().fp_depth_normals(ctx.handle, ptr(depths), None, 6, 48, 64, ptr(K), float('inf'), 0.01,
                                                    ctypes.c_void_p(out.data_ptr() + off), stream_ptr(dev))
  assert normals_call(8) == _lib.FP_EINVAL and b'aligned' in lib().fp_last_error() and (out == 0).all()
  assert normals_call(16) == 0
  torch.cuda.synchronize()
  assert out[4:].abs().sum() > 0


# ---- the procedures -------------------------------------------------------------------------------------------------------------------
def test_joint_refinement_end_to_end():
  """tsdf_align_oracle.refine_case(): 10 views of 96 x 72, view 0 true (the anchor), the others 4 mm / 1.5 degrees off.  After the first
  joint step the poses agree with the restatement's to 1e-9.  The rows are bit-equal, so the two 54 x 54 systems differ by the summation
  order of the 29 sums per pair only.  The system's condition number is 1.5e5 (computed on the CPU; view 8 is weakly constrained) and
  the largest twist of the first step is 0.16.  The worst case of any summation order, n 2^-52 = 1.5e-12 relative per sum, would allow
  1.5e5 x 1.5e-12 x 0.16 = 3.6e-8; the error of a pairwise or blocked order as the kernel's is of the order sqrt(n) 2^-53 = 1e-14 per
  sum, which allows 2.4e-10, so 1e-9 is kept (a relative perturbation of 1e-14 of every sum moved the CPU solution by 2.5e-14).
  The final mean displacement of views 1 .. 9 is at most 1.5 x the restatement's recorded 0.214 mm and below the start; the anchor
  keeps its bits."""
  from foundationpose_amd import reconstruct as R
  K, truth, depths, masks, given = A.refine_case()
  got, info = R.joint_refine_view_poses(dict(depths=depths, masks=masks, K=K, cam_in_obs=given), depth_filter=False)
  nrm = [D.normals(depths[v], K, masks[v]) for v in range(10)]
  pr = D.choose_pairs(given, 4, 100)
  assert info['pairs'][0] == pr
  sm = D.step_sums(depths, nrm, K, given, pr, *D.DEFAULT_STAGES[0][:2])
  xi, _ = D.solve_joint_step(sm, pr, 10, [0])
  want_first = np.stack([A.expm_se3(xi[v]) @ given[v] for v in range(10)])
  first = np.abs(info['after_first'] - want_first).max()
  print(f'after the first step: max |pose - restatement| {first:.3e}; valid {info["valid"][0]:.0f} (restatement {sm[:, 28].sum():.0f})')
  assert info['valid'][0] == sm[:, 28].sum()
  assert first <= 1e-9
  before = np.array([A.displacement(given[v], truth[v]) for v in range(10)]) * 1e3
  after = np.array([A.displacement(got[v], truth[v]) for v in range(10)]) * 1e3
  print(f'before mean {before[1:].mean():.3f} mm; after {np.round(after, 3)} mean {after[1:].mean():.3f} mm (restatement {D.RECORDED_JOINT_MEAN_MM}); '
        f'rms {np.round(1e3 * info["rms"], 3)}; eig ratio {info["eig_ratio"]}')
  assert np.array_equal(got[0], given[0])                                      # the anchor: the same bits
  assert after[1:].mean() <= 1.5 * D.RECORDED_JOINT_MEAN_MM and after[1:].mean() < before[1:].mean()
  assert info['stopped'] == {} and len(info['rms']) == 21 and len(info['pairs']) == 3
  assert np.nanargmin(info['eig_ratio']) == 8
  # a view that sees nothing keeps its pose and is named
  blind = depths.copy()
  blind[4] = 0
  got2, info2 = R.joint_refine_view_poses(dict(depths=blind, masks=masks, K=K, cam_in_obs=given), depth_filter=False, stages=((0.02, 0.5, 2),))
  assert np.array_equal(got2[4], given[4]) and info2['stopped'] == {4: 'no valid residual'} and np.isnan(info2['eig_ratio'][4])
  with pytest.raises(ValueError):
    R.joint_refine_view_poses(dict(depths=depths, masks=masks, K=K, cam_in_obs=given), anchor=10, depth_filter=False)


def test_unposed_orbit():
  """depth_icp_oracle.orbit_case(): 24 frames, only frame 0's pose given.  The restatement's recorded run loses track at frame 5 (mean
  over frames 1 .. 23: odometry 25.123 mm, final 24.654 mm - tests/test_depth_icp_host.py).  Asserted as the issue states it: the final
  mean is at most 1.5 x the recorded one and below the mean of the run's own odometry poses."""
  from foundationpose_amd import reconstruct as R
  K, truth, depths, masks = D.orbit_case()
  got, info = R.estimate_view_poses(dict(depths=depths, masks=masks, K=K), first_pose=truth[0], depth_filter=False)
  odo = np.array([A.displacement(info['odometry'][v], truth[v]) for v in range(24)]) * 1e3
  fin = np.array([A.displacement(got[v], truth[v]) for v in range(24)]) * 1e3
  print(f'odometry {np.round(odo, 3)} mean {odo[1:].mean():.3f} mm; final {np.round(fin, 3)} mean {fin[1:].mean():.3f} mm '
        f'(restatement {D.RECORDED_ORBIT_ODOMETRY_MM[0]} / {D.RECORDED_ORBIT_FINAL_MM[0]})')
  assert np.array_equal(got[0], truth[0])
  assert fin[1:].mean() <= 1.5 * D.RECORDED_ORBIT_FINAL_MM[0]
  assert fin[1:].mean() < odo[1:].mean()
  assert odo[1:5].max() < 0.1 and info['joint']['stopped'] == {}


# ---- through reconstruct_object: rendered views of the mustard bottle ----------------------------------------------------------------------
(MH, MW), MVOXEL, MK = O.MUSTARD_HW, O.MUSTARD_VOXEL, O.MUSTARD_K
MUSTARD_KEEP = list(range(10))


@pytest.fixture(scope='module')
def mustard_views():
  from foundationpose_amd import Utils as U
  from tests import util
  sc = util.scene(0)
  cams = np.stack([O.look_at(e) for e in O.mustard_eyes()])
  ob_in_cams = np.linalg.inv(cams).astype(np.float32)
  color, depth, _ = U.nvdiffrast_render(K=MK, H=MH, W=MW, ob_in_cams=ob_in_cams, mesh_tensors=util.to_dev(sc['mt']))
  mm = np.round(depth.cpu().numpy().astype(np.float64) * 1e3).astype(np.uint16)       # what a 16-bit PNG in millimetres holds
  depths = (mm.astype(np.float64) / 1e3).astype(np.float32)
  rgbs = np.clip(np.round(color.cpu().numpy() * 255), 0, 255).astype(np.uint8)
  return dict(depths=depths, rgbs=rgbs, masks=(mm > 0).astype(np.uint8), K=MK, cam_in_obs=cams), sc


def test_jointly_refined_poses_give_a_better_mesh(mustard_views):
  """The mustard views of tests/test_gpu_tsdf_align.py, rendered the same way, every pose but the first perturbed by 4 mm / 1.5 degrees
  (seed 31) - WITHOUT the two views from below (MUSTARD_KEEP: the ring of eight and the two from above).  The fraction of the fused
  vertices beyond the radial bound is lower with refine_poses='joint' than with the given poses; the TSDF-refined value is printed.
  CPU experiment with the checker's renderer and the restatements alone (raw maps rounded to millimetres, fused by tsdf_oracle.Volume;
  DESIGN.md section 5), views 0 .. 9: true poses 0.0091, given 0.0300, TSDF-refined 0.0102, jointly refined 0.0120; mean displacement of
  views 1 .. 9: 4.06 mm given, 1.94 mm TSDF, 1.52 mm joint.  With all 12 views the joint refinement does NOT improve the scene on the
  CPU (given 0.0360, TSDF 0.0092, joint 0.0917): the two views from below see the flat bottom and a rim, which constrain neither the
  sliding in the plane nor the rotation about its normal, and they drift by 77 mm, while the TSDF procedure aligns them to a volume
  that already holds the sides.  The schedule is the default one in both."""
  from foundationpose_amd.reconstruct import reconstruct_object
  views, sc = mustard_views
  rs = np.random.RandomState(31)
  given = views['cam_in_obs'].copy()
  for v in range(1, len(given)):
    given[v] = A.perturb(given[v], 0.004, 1.5, rs)
  off = {k: (a if k == 'K' else a[MUSTARD_KEEP]) for k, a in dict(views, cam_in_obs=given).items()}
  frac = lambda m: O.fraction_beyond_bound(m.vertices, sc['mesh'].vertices, sc['mesh'].faces, MVOXEL)
  plain = reconstruct_object(off, voxel_size=MVOXEL)
  tsdf = reconstruct_object(off, voxel_size=MVOXEL, refine_poses=True)
  joint = reconstruct_object(off, voxel_size=MVOXEL, refine_poses='joint')
  (f_plain, _), (f_tsdf, _), (f_joint, far) = frac(plain), frac(tsdf), frac(joint)
  print(f'beyond {O.RADIAL_BOUND_VOXELS:.2f} voxels: given poses {f_plain:.4f}, TSDF-refined {f_tsdf:.4f}, jointly refined {f_joint:.4f} (max {far:.2f} voxels)')
  assert len(joint.faces) > 5000
  assert f_joint < f_plain
  with pytest.raises(ValueError):
    reconstruct_object(off, voxel_size=MVOXEL, refine_poses='both')


def test_false_and_true_are_unchanged(mustard_views):
  """refine_poses=False is the default's bits; refine_poses=True is the fusion at the poses refine_view_poses returns"""
  from foundationpose_amd.reconstruct import reconstruct_object, refine_view_poses
  views = mustard_views[0]
  same = lambda a, b: (np.array_equal(a.vertices, b.vertices) and np.array_equal(a.faces, b.faces) and np.array_equal(a.vertex_normals, b.vertex_normals)
                       and np.array_equal(a.visual.vertex_colors, b.visual.vertex_colors))
  a, b = reconstruct_object(views, voxel_size=MVOXEL), reconstruct_object(views, voxel_size=MVOXEL, refine_poses=False, estimate_poses=False)
  assert same(a, b) and len(a.faces) > 5000
  poses, _ = refine_view_poses(views, voxel_size=MVOXEL)
  c, d = reconstruct_object(views, voxel_size=MVOXEL, refine_poses=True), reconstruct_object(dict(views, cam_in_obs=poses), voxel_size=MVOXEL)
  assert same(c, d) and not np.array_equal(poses[1:], views['cam_in_obs'][1:])


def test_script_estimates_poses_for_a_folder_without_them(tmp_path, monkeypatch):
  """scripts/reconstruct_object.py DIR on a folder without cam_in_ob/ (the first 5 frames of the orbit, depth in millimetres): the mesh,
  and DIR/cam_in_ob_estimated/NAME.txt - frame 0 with the identity rotation, the others such that G^-1 pose_k is within 1 mm of the
  truth, where G = pose_0 truth_0^-1 is the change of object frame (the restatement's odometry holds these frames to 0.06 mm).
  load_reference_views still insists on cam_in_ob/ by default, and reconstruct_object(estimate_poses=True) takes the same folder."""
  import importlib.util
  import os
  from PIL import Image
  from foundationpose_amd.reconstruct import load_reference_views, reconstruct_object
  K, truth, depths, masks = D.orbit_case()
  n = 5
  for sub in ('rgb', 'depth', 'mask'):
    os.makedirs(tmp_path / sub)
  np.savetxt(tmp_path / 'K.txt', K, fmt='%.18e')
  for k in range(n):
    name = f'{k:04d}'
    Image.fromarray(np.full(depths[k].shape + (3,), 128, dtype=np.uint8)).save(tmp_path / 'rgb' / f'{name}.png')
    Image.fromarray(np.round(depths[k].astype(np.float64) * 1e3).astype(np.uint16)).save(tmp_path / 'depth' / f'{name}.png')
    Image.fromarray(masks[k] * 255).save(tmp_path / 'mask' / f'{name}.png')
  with pytest.raises(OSError):
    load_reference_views(str(tmp_path))
  assert 'cam_in_obs' not in load_reference_views(str(tmp_path), poses=False)
  repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  spec = importlib.util.spec_from_file_location('reconstruct_object_script', os.path.join(repo, 'scripts', 'reconstruct_object.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  monkeypatch.setattr('sys.argv', ['reconstruct_object.py', str(tmp_path), '--voxel', '0.003', '--no-depth-filter'])
  mod.main()
  assert os.path.getsize(tmp_path / 'model' / 'model.obj') > 10000
  out = [np.loadtxt(tmp_path / 'cam_in_ob_estimated' / f'{k:04d}.txt').reshape(4, 4) for k in range(n)]
  assert np.array_equal(out[0][:3, :3], np.eye(3)) and np.linalg.norm(out[0][:3, 3]) > 0.3
  G = out[0] @ np.linalg.inv(truth[0])
  err = [A.displacement(np.linalg.inv(G) @ out[k], truth[k]) * 1e3 for k in range(1, n)]
  print(f'displacement of frames 1 .. {n - 1} in the first frame\'s object frame: {np.round(err, 3)} mm')
  assert max(err) < 1.0
  mesh = reconstruct_object(str(tmp_path), voxel_size=0.003, depth_filter=False, estimate_poses=True)
  assert len(mesh.faces) > 1000
