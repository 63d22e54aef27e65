"""GPU: the photometric term of pairwise depth ICP (fp_view_intensity and fp_depth_pairs_align_photo in csrc/depth_icp.hip; view_intensity,
align_pairs_step(intensity=), combine_sums and the photometric option of joint_refine_view_poses, estimate_view_poses and
reconstruct_object in foundationpose_amd/reconstruct.py) against the numpy restatement of the header's rules (tests/photo_icp_oracle.py):
intensity maps and 16-float rows bit for bit, the geometric sums bit for bit those of fp_depth_pairs_align, the photometric sums within
the bound of any summation order of exact terms, the two procedures against the restatement's recorded runs, and through
reconstruct_object and the script.

Shapes: the textured row case of 6 views of 64 x 48 (3 tiles of 1024 pixels per pair, 16 directed pairs, masks cutting every view) and
of 37 x 29 (1073 pixels: a last tile of 49, image rows that straddle the tiles); 8 views of 96 x 72 of a textured sphere; the
24-frame orbit of 96 x 72."""
import ctypes

import numpy as np
import pytest
import torch

from tests import depth_icp_oracle as D
from tests import photo_icp_oracle as P
from tests import tsdf_align_oracle as A
from tests import tsdf_oracle as O

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
  return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _case(*size):
  K, truth, depths, masks, query, pairs, rgbs = P.row_case(*size)
  return dict(K=K, truth=truth, depths=depths, masks=masks, query=query, pairs=pairs, rgbs=rgbs)


@pytest.fixture(scope='module')
def case():
  return _case()


@pytest.fixture(scope='module')
def oracle_step(case):
  """normals, intensity maps (of the row case's tighter max_jump), the 16-float rows of the 16 pairs and the skipped pixels per reason"""
  nrm = np.stack([D.normals(case['depths'][v], case['K'], case['masks'][v]) for v in range(6)])
  inten = np.stack(P.row_intensity(case['depths'], case['masks'], case['rgbs'], case['K']))
  out = [P.pair_rows(case['depths'], nrm, inten, case['K'], case['query'], s, t, *D.ROW_GATE, P.ROW_I_MAX, reasons=True) for s, t in case['pairs']]
  return nrm, inten, np.stack([o[0] for o in out]), [{k: int(o[1][k].sum()) for k in P.SKIPS} for o in out]


@pytest.fixture(scope='module')
def device_step(case):
  from foundationpose_amd import reconstruct as R
  nrm = R.depth_normals(case['depths'], case['K'], case['masks'])
  inten = R.view_intensity(case['rgbs'], R.depth_normals(case['depths'], case['K'], case['masks'], max_jump=P.ROW_INTENSITY_MAX_JUMP))
  depths = torch.as_tensor(case['depths'], device=nrm.device)
  sums, rows = R.align_pairs_step(depths, nrm, case['K'], case['query'], case['pairs'], *D.ROW_GATE, rows=True, intensity=inten, i_max=P.ROW_I_MAX)
  return nrm, depths, inten, sums, rows


def test_intensity_is_bit_equal_and_zero_where_there_is_no_normal(case, oracle_step, device_step):
  from foundationpose_amd import reconstruct as R
  nrm, want = oracle_step[0], oracle_step[1]
  got = device_step[2].cpu().numpy()
  print(f'{int(want[..., 3].sum())} records of {want[..., 3].size} pixels; differing words {(got.view(np.uint32) != want.view(np.uint32)).sum()}')
  assert all(want[v, ..., 3].sum() >= 100 for v in range(6))
  assert _same_bits(got, want)
  # from the alignment's own normals: a record exactly where a normal is, four zeros elsewhere
  own = R.view_intensity(case['rgbs'], device_step[0]).cpu().numpy()
  assert _same_bits(own, np.stack([P.intensity(case['rgbs'][v], nrm[v]) for v in range(6)]))
  assert np.array_equal(own[..., 3] != 0, nrm[..., 3] != 0) and (own[nrm[..., 3] == 0] == 0).all() and own[..., 3].sum() > 2500
  # three different channels
  rgb = np.random.RandomState(3).randint(0, 256, size=case['rgbs'].shape).astype(np.uint8)
  assert _same_bits(R.view_intensity(rgb, device_step[0]).cpu().numpy(), np.stack([P.intensity(rgb[v], nrm[v]) for v in range(6)]))
  # 66 views (the 6 of the case 11 times) are cut into calls of 64 and 2: every copy gets the bits of its original
  many = R.view_intensity(np.concatenate([case['rgbs']] * 11), torch.cat([device_step[0]] * 11))
  assert torch.equal(many, torch.cat([torch.as_tensor(own, device=many.device)] * 11))
  # a map that claims normals on the border: the neighbours outside the view are not read, the border stays empty
  edge = R.view_intensity(rgb, torch.ones_like(device_step[0])).cpu().numpy()
  assert _same_bits(edge, np.stack([P.intensity(rgb[v], np.ones_like(nrm[v])) for v in range(6)])) and edge[..., 3].sum() == 6 * 46 * 62


def _ragged():
  """37 x 29 without masks, the intensity maps from the alignment's own normals: (case, normals, intensity maps, rows)"""
  c = _case(*P.RAGGED)
  nrm = np.stack([D.normals(c['depths'][v], c['K']) for v in range(6)])
  inten = np.stack([P.intensity(c['rgbs'][v], nrm[v]) for v in range(6)])
  want = np.stack([P.pair_rows(c['depths'], nrm, inten, c['K'], c['query'], s, t, *D.ROW_GATE, P.ROW_I_MAX) for s, t in c['pairs']])
  return c, nrm, inten, want


def test_intensity_rows_and_counts_on_a_ragged_image_without_masks():
  from foundationpose_amd import reconstruct as R
  c, nrm, inten, want = _ragged()
  assert c['depths'].shape[1:] == (29, 37) and all(inten[v, ..., 3].sum() >= 100 for v in range(6))
  assert sum(w[..., 15].sum() >= 50 for w in want) >= 10
  dn = R.depth_normals(c['depths'], c['K'])
  di = R.view_intensity(c['rgbs'], dn)
  assert _same_bits(di.cpu().numpy(), inten)
  sums, got = R.align_pairs_step(torch.as_tensor(c['depths'], device=dn.device), dn, c['K'], c['query'], c['pairs'], *D.ROW_GATE, rows=True, intensity=di,
                                 i_max=P.ROW_I_MAX)
  assert _same_bits(got.cpu().numpy(), want)
  assert np.array_equal(sums[:, 28], want[..., 7].reshape(len(want), -1).sum(1))
  assert np.array_equal(sums[:, 57], want[..., 15].reshape(len(want), -1).sum(1))


def test_rows_are_bit_equal_and_counts_equal(case, oracle_step, device_step):
  _, _, want, why = oracle_step
  total = {k: sum(w[k] for w in why) for k in P.SKIPS}
  print(f'photometric rows per pair {[int(w[..., 15].sum()) for w in want]}; skipped {total}')
  assert all(total[k] > 0 for k in P.SKIPS), total
  got = device_step[4].cpu().numpy()
  print(f'differing words: {(got.view(np.uint32) != want.view(np.uint32)).sum()} of {want.size}')
  assert got.shape == (16, 48, 64, 16) and _same_bits(got, want)
  assert np.array_equal(device_step[3][:, 28], want[..., 7].reshape(len(want), -1).sum(1))
  assert np.array_equal(device_step[3][:, 57], want[..., 15].reshape(len(want), -1).sum(1))


def test_geometric_half_is_the_geometric_call_bit_for_bit(case, device_step):
  from foundationpose_amd import reconstruct as R
  nrm, depths, inten, sums, rows = device_step
  geo, geo_rows = R.align_pairs_step(depths, nrm, case['K'], case['query'], case['pairs'], *D.ROW_GATE, rows=True)
  assert geo.shape == (16, 29) and sums.shape == (16, 58)
  assert np.array_equal(sums[:, :29].copy().view(np.uint64), geo.view(np.uint64))
  assert torch.equal(rows[..., :8].contiguous().view(torch.int32), geo_rows.view(torch.int32))
  assert (geo[:12, 28] >= 150).all()


def test_photometric_sums_are_within_the_bound_of_any_summation_order(oracle_step, device_step):
  """As tests/test_gpu_depth_icp.py: every term is a product of two fp32 numbers, exact in double; n exact terms added in double in any
  order differ from the exactly rounded sum (math.fsum) by at most (n - 1) 2^-53 sum |terms| (1 + O(2^-53)) - the bound asserted is
  n 2^-52 sum |terms|, for both halves.  The counts are sums of ones: exact."""
  worst = 0.0
  for k, rw in enumerate(oracle_step[2]):
    ref, scale = P.sums(rw)
    err = np.abs(device_step[3][k] - ref)
    for half in (0, 29):
      n = ref[half + 28]
      bound = n * 2.0 ** -52 * scale[half:half + 29]
      if n:
        worst = max(worst, (err[half:half + 28] / np.maximum(bound[:28], 1e-300)).max())
      assert (err[half:half + 29] <= bound).all(), (k, half, err, bound)
      assert device_step[3][k, half + 28] == n
  print(f'largest |sum - fsum| / bound: {worst:.3e}')
  assert (device_step[3][:10, 57] >= 60).all()


@pytest.mark.parametrize('make', [lambda: P.row_case(96, 100, 200.0), P.tiny_case, P.row_case, lambda: P.tiny_case(K=O.skew_camera(5, 7, 130.0))],
                         ids=['96x100', '5x7', 'masked 48x64', '5x7 fx != fy'])
def test_sums_have_the_bits_of_the_stated_order(make):
  """All 58 of the device's sums against tests/gn_sums_oracle.py (the order stated in csrc/gn_sums.h) applied to the device's own
  rows, floats 0 .. 7 for terms 0 .. 28 and floats 8 .. 15 for terms 29 .. 57, bit for bit.  The shapes of the same test of
  tests/test_gpu_depth_icp.py: 10 tiles with a ragged last one, one partial tile, and the masked row case with its empty waves."""
  from foundationpose_amd import reconstruct as R
  from tests import gn_sums_oracle as G
  c = dict(zip(('K', 'truth', 'depths', 'masks', 'query', 'pairs', 'rgbs'), make()))
  nrm = R.depth_normals(c['depths'], c['K'], c['masks'])
  inten = R.view_intensity(c['rgbs'], R.depth_normals(c['depths'], c['K'], c['masks'], max_jump=P.ROW_INTENSITY_MAX_JUMP))
  sums, rows = R.align_pairs_step(torch.as_tensor(c['depths'], device=nrm.device), nrm, c['K'], c['query'], c['pairs'], *D.ROW_GATE, rows=True,
                                  intensity=inten, i_max=P.ROW_I_MAX)
  rows = rows.cpu().numpy()
  want = np.stack([np.concatenate([G.device_sums(np.ascontiguousarray(rows[p, ..., :8])), G.device_sums(np.ascontiguousarray(rows[p, ..., 8:]))])
                   for p in range(len(c['pairs']))])
  print(f'{rows.shape[1:3]}: valid per pair {sums[:, 28]}, photometric {sums[:, 57]}; differing words '
        f'{(sums.view(np.uint64) != want.view(np.uint64)).sum()} of {want.size}')
  assert sums[:, 28].sum() > 0 and sums[:, 57].sum() > 0
  assert sums.shape == (len(c['pairs']), 58) and np.array_equal(sums.view(np.uint64), want.view(np.uint64))


def test_rows_under_a_camera_with_fx_not_fy():
  """The 5 x 7 case through tsdf_oracle.skew_camera (fy = 1.25 fx, cx and cy off the middle by different amounts): the photometric row
  takes fx and fy themselves (the image gradient through the projection), the geometric one the rays and the projection.  Every pair has
  geometric and photometric rows."""
  from foundationpose_amd import reconstruct as R
  c = dict(zip(('K', 'truth', 'depths', 'masks', 'query', 'pairs', 'rgbs'), P.tiny_case(K=O.skew_camera(5, 7, 130.0))))
  nrm = np.stack([D.normals(c['depths'][v], c['K'], c['masks'][v]) for v in range(6)])
  inten = np.stack(P.row_intensity(c['depths'], c['masks'], c['rgbs'], c['K']))
  want = np.stack([P.pair_rows(c['depths'], nrm, inten, c['K'], c['query'], s, t, *D.ROW_GATE, P.ROW_I_MAX) for s, t in c['pairs']])
  print(f'rows per pair: geometric {[int(w[..., 7].sum()) for w in want]}, photometric {[int(w[..., 15].sum()) for w in want]}')
  assert all(w[..., 7].sum() > 0 and w[..., 15].sum() > 0 for w in want)
  dn = R.depth_normals(c['depths'], c['K'], c['masks'])
  di = R.view_intensity(c['rgbs'], R.depth_normals(c['depths'], c['K'], c['masks'], max_jump=P.ROW_INTENSITY_MAX_JUMP))
  assert _same_bits(di.cpu().numpy(), inten)
  sums, got = R.align_pairs_step(torch.as_tensor(c['depths'], device=dn.device), dn, c['K'], c['query'], c['pairs'], *D.ROW_GATE, rows=True,
                                 intensity=di, i_max=P.ROW_I_MAX)
  assert _same_bits(got.cpu().numpy(), want)
  assert np.array_equal(sums[:, 28], want[..., 7].reshape(len(want), -1).sum(1))
  assert np.array_equal(sums[:, 57], want[..., 15].reshape(len(want), -1).sum(1))


def test_a_pair_does_not_depend_on_its_batch(case, device_step):
  from foundationpose_amd import _lib
  from foundationpose_amd import reconstruct as R
  nrm, depths, inten, sums, rows = device_step
  step = lambda pr, **kw: R.align_pairs_step(depths, nrm, case['K'], case['query'], pr, *D.ROW_GATE, intensity=inten, i_max=P.ROW_I_MAX, **kw)
  pairs = case['pairs']
  assert np.array_equal(step(pairs), sums)                                              # two runs
  assert np.array_equal(step(pairs[3:4])[0], sums[3])                                   # alone
  order = list(range(15, -1, -1))
  assert np.array_equal(step([pairs[i] for i in order]), sums[order])                   # at another index
  reps = 17
  assert 16 * reps > _lib.FP_DEPTH_ALIGN_MAX_PAIRS                                      # 272 pairs: calls of 256 and 16
  many = step(pairs * reps)
  assert np.array_equal(many, np.concatenate([sums] * reps))
  cut = _lib.FP_DEPTH_ALIGN_MAX_PAIRS
  _, tail = step((pairs * reps)[cut - 2:cut + 3], rows=True)                            # the rows of the same pairs in another, shorter batch
  assert torch.equal(tail, rows[[(cut - 2 + i) % 16 for i in range(5)]])
  assert len(np.unique(sums[:10, 56])) == 10


def test_zero_pairs_misaligned_buffers_and_an_infinite_i_max(case, oracle_step, device_step):
  from foundationpose_amd import _lib
  from foundationpose_amd import reconstruct as R
  from foundationpose_amd._lib import lib, ptr, stream_ptr
  nrm, depths, inten, sums0, _ = device_step
  dev = nrm.device
  ctx = _lib.Context.get(dev)
  K, poses = np.ascontiguousarray(case['K']), np.ascontiguousarray(case['query'])
  sums = np.full(58, 7.0)
  rc = lib().fp_depth_pairs_align_photo(ctx.handle, ptr(depths), ptr(nrm), ptr(inten), 6, 48, 64, ptr(K), ptr(poses), None, 0, 0.01, 0.5, 0.2, None,
                                        ptr(sums), stream_ptr(dev))
  assert rc == 0 and (sums == 7.0).all()                                                 # zero pairs write nothing
  assert R.align_pairs_step(depths, nrm, K, poses, [], 0.01, 0.5, intensity=inten).shape == (0, 58)
  keep = torch.full((1, 4, 4, 4), 3.0, device=dev)
  rc = lib().fp_view_intensity(ctx.handle, ptr(torch.zeros(48, dtype=torch.uint8, device=dev)), ptr(nrm), 0, 4, 4, ptr(keep), stream_ptr(dev))
  assert rc == 0 and (keep == 3.0).all()                                                 # zero views write nothing
  # misaligned buffers
  pr = np.array([case['pairs'][2]], dtype=np.int32)                                      # the pair with the most residuals above i_max
  buf = torch.zeros(48 * 64 * 16 + 4, device=dev)
  ibuf = torch.zeros(6 * 48 * 64 * 4 + 4, device=dev)
  assert buf.data_ptr() % 16 == 0 and ibuf.data_ptr() % 16 == 0
  ibuf[4:] = inten.reshape(-1)                                                           # the intensity maps at a 16-byte offset
  one = np.zeros(58)
  pairs_call = lambda i_off, r_off, i_max=P.ROW_I_MAX: lib().fp_depth_pairs_align_photo(
      ctx.handle, ptr(depths), ptr(nrm), ctypes.c_void_p(ibuf.data_ptr() + i_off), 6, 48, 64, ptr(K), ptr(poses), ptr(pr), 1, D.ROW_GATE[0], D.ROW_GATE[1],
      i_max, ctypes.c_void_p(buf.data_ptr() + r_off), ptr(one), stream_ptr(dev))
  assert pairs_call(16, 4) == _lib.FP_EINVAL and b'aligned' in lib().fp_last_error() and (buf == 0).all()
  assert pairs_call(4, 16) == _lib.FP_EINVAL and b'aligned' in lib().fp_last_error() and (buf == 0).all()
  assert pairs_call(16, 16) == 0 and np.array_equal(one, sums0[2])
  out = torch.zeros(6 * 48 * 64 * 4 + 4, device=dev)
  rgb = torch.as_tensor(case['rgbs'], device=dev).contiguous()
  map_call = lambda off: lib().fp_view_intensity(ctx.handle, ptr(rgb), ptr(nrm), 6, 48, 64, ctypes.c_void_p(out.data_ptr() + off), stream_ptr(dev))
  assert map_call(8) == _lib.FP_EINVAL and b'aligned' in lib().fp_last_error() and (out == 0).all()
  assert map_call(16) == 0
  torch.cuda.synchronize()
  assert out[4:].abs().sum() > 0
  # i_max = inf is a value: nothing is skipped for its residual
  assert pairs_call(16, 16, float('inf')) == 0
  s, t = case['pairs'][2]
  want, why = P.pair_rows(case['depths'], oracle_step[0], oracle_step[1], case['K'], case['query'], s, t, *D.ROW_GATE, np.inf, reasons=True)
  assert why['i_max'].sum() == 0 and one[57] == want[..., 15].sum() > sums0[2, 57]
  assert _same_bits(buf[4:].reshape(48, 64, 16).cpu().numpy(), want)


# ---- the procedures -------------------------------------------------------------------------------------------------------------------
def _errors(poses, truth):
  n = len(truth)
  return (np.array([A.displacement(poses[v], truth[v]) for v in range(n)]) * 1e3, np.array([P.rotation_deg(poses[v], truth[v]) for v in range(n)]))


def test_textured_sphere_end_to_end():
  """photo_icp_oracle.sphere_case(): 8 views of 96 x 72 of one textured sphere, view 0 true (the anchor), the others 4 mm / 1.5 degrees
  off.  After the first joint step the poses agree with the restatement's to 1e-9.  The rows are bit-equal, so the two 42 x 42 systems
  differ by the summation order of the 58 sums per pair only.  The combined system's condition number is 3.2e5 (computed on the CPU;
  the geometric system's alone is 5.0e6) and the largest twist entry of the first step is 0.091.  The worst case of any summation order,
  n 2^-52 = 6.6e-13 relative per sum of n = 3000 pixels, would allow 3.2e5 x 6.6e-13 x 0.091 = 1.9e-8; the error of a pairwise or blocked
  order as the kernel's is of the order sqrt(n) 2^-53 = 6e-15 per sum, which allows 1.8e-10, so 1e-9 is kept (a relative perturbation of
  1e-14 of every sum moved the CPU solution by 2.7e-14, one of 5e-13 by 2.0e-13).
  The final mean displacement of views 1 .. 7 is at most 1.5 x the restatement's recorded 0.048 mm and at most 0.5 mm; the anchor keeps
  its bits; photometric=False returns the bits of the call without the argument, and that geometric run's mean rotation error is above
  the 1.5 degrees it started with."""
  from foundationpose_amd import reconstruct as R
  K, truth, depths, masks, given, rgbs = P.sphere_case()
  views = dict(depths=depths, masks=masks, rgbs=rgbs, K=K, cam_in_obs=given)
  got, info = R.joint_refine_view_poses(views, depth_filter=False, photometric=True)
  nrm = [D.normals(depths[v], K, masks[v]) for v in range(8)]
  inten = [P.intensity(rgbs[v], nrm[v]) for v in range(8)]
  pr = D.choose_pairs(given, 4, 100)
  assert info['pairs'][0] == pr
  sm = P.step_sums(depths, nrm, inten, K, given, pr, *D.DEFAULT_STAGES[0][:2], P.I_MAX)
  xi, _ = D.solve_joint_step(P.combine(sm, P.PHOTO_WEIGHT), pr, 8, [0])
  want_first = np.stack([A.expm_se3(xi[v]) @ given[v] for v in range(8)])
  first = np.abs(info['after_first'] - want_first).max()
  print(f'after the first step: max |pose - restatement| {first:.3e}; valid {info["valid"][0]:.0f} / {info["photo_valid"][0]:.0f} '
        f'(restatement {sm[:, 28].sum():.0f} / {sm[:, 57].sum():.0f})')
  assert info['valid'][0] == sm[:, 28].sum() and info['photo_valid'][0] == sm[:, 57].sum()
  assert first <= 1e-9
  disp, rot = _errors(got, truth)
  print(f'after {np.round(disp, 3)} mean {disp[1:].mean():.3f} mm (restatement {P.RECORDED_SPHERE_PHOTO[0]}), rotation {np.round(rot, 3)} degrees; '
        f'photometric rms {np.round(info["photo_rms"], 4)}; eig ratio {info["eig_ratio"]}')
  assert np.array_equal(got[0], given[0])                                      # the anchor: the same bits
  assert disp[1:].mean() <= 1.5 * P.RECORDED_SPHERE_PHOTO[0] and disp[1:].mean() <= 0.5
  assert info['stopped'] == {} and len(info['rms']) == len(info['photo_rms']) == len(info['photo_valid']) == 21 and len(info['pairs']) == 3
  # a float is the weight itself
  same, _ = R.joint_refine_view_poses(views, depth_filter=False, photometric=P.PHOTO_WEIGHT, stages=D.DEFAULT_STAGES[:1])
  assert np.array_equal(same, R.joint_refine_view_poses(views, depth_filter=False, photometric=True, stages=D.DEFAULT_STAGES[:1])[0])
  # geometry only: today's bits, and the rotation drifts
  plain, pinfo = R.joint_refine_view_poses(dict(depths=depths, masks=masks, K=K, cam_in_obs=given), depth_filter=False)
  off, oinfo = R.joint_refine_view_poses(views, depth_filter=False, photometric=False)
  assert np.array_equal(plain, off) and np.array_equal(pinfo['rms'], oinfo['rms']) and len(oinfo['photo_rms']) == 0
  gdisp, grot = _errors(plain, truth)
  print(f'geometry only: {np.round(gdisp, 3)} mean {gdisp[1:].mean():.3f} mm, rotation {np.round(grot, 3)} mean {grot[1:].mean():.3f} degrees')
  assert grot[1:].mean() > 1.5
  with pytest.raises(ValueError):
    R.joint_refine_view_poses(dict(depths=depths, masks=masks, K=K, cam_in_obs=given), depth_filter=False, photometric=True)      # no rgbs
  with pytest.raises(ValueError):
    R.joint_refine_view_poses(views, depth_filter=False, photometric=-0.03)


def test_textured_unposed_orbit():
  """photo_icp_oracle.orbit_case(): 24 textured frames, only frame 0's pose given.  The restatement's recorded run with the term holds
  every frame (mean over frames 1 .. 23: odometry 0.086 mm, final 0.052 mm - tests/test_photo_icp_host.py) where the geometric run
  loses track at frame 5 (24.654 mm).  The final mean is at most 1.5 x the recorded one and at most 1 mm; frame 0 keeps its bits."""
  from foundationpose_amd import reconstruct as R
  K, truth, depths, masks, rgbs = P.orbit_case()
  got, info = R.estimate_view_poses(dict(depths=depths, masks=masks, rgbs=rgbs, K=K), first_pose=truth[0], depth_filter=False, photometric=True)
  odo, _ = _errors(info['odometry'], truth)
  fin, _ = _errors(got, truth)
  print(f'odometry {np.round(odo, 3)} mean {odo[1:].mean():.3f} mm; final {np.round(fin, 3)} mean {fin[1:].mean():.3f} mm '
        f'(restatement {P.RECORDED_ORBIT_PHOTO_ODOMETRY_MM[0]} / {P.RECORDED_ORBIT_PHOTO_FINAL_MM[0]})')
  assert np.array_equal(got[0], truth[0])
  assert fin[1:].mean() <= 1.5 * P.RECORDED_ORBIT_PHOTO_FINAL_MM[0] and fin[1:].mean() <= 1.0
  assert info['joint']['stopped'] == {} and len(info['joint']['photo_rms']) == 17
  with pytest.raises(ValueError):
    R.estimate_view_poses(dict(depths=depths, masks=masks, K=K), first_pose=truth[0], depth_filter=False, photometric=True)      # no rgbs


# ---- through reconstruct_object: rendered views of the mustard bottle ----------------------------------------------------------------------
(MH, MW), MVOXEL, MK = O.MUSTARD_HW, O.MUSTARD_VOXEL, O.MUSTARD_K
MUSTARD_KEEP = list(range(10))


@pytest.fixture(scope='module')
def mustard_views():
  """as tests/test_gpu_depth_icp.py renders them: unlit, 160 x 120, depth rounded to millimetres"""
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


def test_photometric_joint_refinement_through_reconstruct_object(mustard_views):
  """The mustard views of tests/test_gpu_depth_icp.py - unlit, so that a surface point has one colour in every view -, every pose but
  the first perturbed by 4 mm / 1.5 degrees (seed 31), views 0 .. 9.  The fraction of the fused vertices beyond the radial bound is
  lower with refine_poses='joint', photometric=True than with the given poses: the form of the geometric test's assertion.  The
  geometry-only value and the values with all 12 views are printed; nobody had measured them before, so they are not asserted.  Measured
  on an MI355X: views 0 .. 9 given 0.0361, geometry only 0.0093, with the term 0.0280 - better than given, worse
  than geometry alone, whose poses this object already determines -; all 12 views given 0.0569, geometry only 0.8093, with the term
  0.0797.  photometric is refused where nothing takes it."""
  from foundationpose_amd.reconstruct import reconstruct_object
  views, sc = mustard_views
  rs = np.random.RandomState(31)
  given = views['cam_in_obs'].copy()
  for v in range(1, len(given)):
    given[v] = A.perturb(given[v], 0.004, 1.5, rs)
  every = dict(views, cam_in_obs=given)
  off = {k: (a if k == 'K' else a[MUSTARD_KEEP]) for k, a in every.items()}
  frac = lambda m: O.fraction_beyond_bound(m.vertices, sc['mesh'].vertices, sc['mesh'].faces, MVOXEL)
  plain = reconstruct_object(off, voxel_size=MVOXEL)
  joint = reconstruct_object(off, voxel_size=MVOXEL, refine_poses='joint')
  photo = reconstruct_object(off, voxel_size=MVOXEL, refine_poses='joint', photometric=True)
  (f_plain, _), (f_joint, _), (f_photo, far) = frac(plain), frac(joint), frac(photo)
  print(f'views 0 .. 9, beyond {O.RADIAL_BOUND_VOXELS:.2f} voxels: given poses {f_plain:.4f}, jointly refined {f_joint:.4f}, with the photometric term '
        f'{f_photo:.4f} (max {far:.2f} voxels)')
  f12 = [frac(reconstruct_object(every, voxel_size=MVOXEL, **kw))[0] for kw in (dict(), dict(refine_poses='joint'), dict(refine_poses='joint', photometric=True))]
  print(f'all 12 views: given poses {f12[0]:.4f}, jointly refined {f12[1]:.4f}, with the photometric term {f12[2]:.4f}')
  assert len(photo.faces) > 5000
  assert f_photo < f_plain
  for kw in (dict(refine_poses=True), dict(), dict(refine_poses=dict(rounds=1)), dict(refine_poses=True, estimate_poses=True)):
    with pytest.raises(ValueError):
      reconstruct_object(off, voxel_size=MVOXEL, photometric=True, **kw)
  no_rgb = {k: a for k, a in off.items() if k != 'rgbs'}
  with pytest.raises(ValueError):
    reconstruct_object(no_rgb, voxel_size=MVOXEL, refine_poses='joint', photometric=True)


def test_script_estimates_poses_with_the_photometric_term(tmp_path, monkeypatch):
  """scripts/reconstruct_object.py DIR --estimate-poses --photometric on a written folder without cam_in_ob/ (the first 5 textured frames
  of the orbit, depth in millimetres): the mesh, and DIR/cam_in_ob_estimated/NAME.txt such that G^-1 pose_k is within 1 mm of the truth,
  G = pose_0 truth_0^-1 being the change of object frame.  The poses are those of estimate_view_poses(photometric=True) on the folder
  and not those of the call without the term; --photometric with --refine-poses is refused."""
  import importlib.util
  import os
  from PIL import Image
  from foundationpose_amd.reconstruct import estimate_view_poses
  K, truth, depths, masks, rgbs = P.orbit_case()
  n = 5
  for sub in ('rgb', 'depth', 'mask'):
    os.makedirs(tmp_path / sub)
  np.savetxt(tmp_path / 'K.txt', K, fmt='%.18e')
  for k in range(n):
    name = f'{k:04d}'
    Image.fromarray(rgbs[k]).save(tmp_path / 'rgb' / f'{name}.png')
    Image.fromarray(np.round(depths[k].astype(np.float64) * 1e3).astype(np.uint16)).save(tmp_path / 'depth' / f'{name}.png')
    Image.fromarray(masks[k] * 255).save(tmp_path / 'mask' / f'{name}.png')
  repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  spec = importlib.util.spec_from_file_location('reconstruct_object_script', os.path.join(repo, 'scripts', 'reconstruct_object.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  monkeypatch.setattr('sys.argv', ['reconstruct_object.py', str(tmp_path), '--voxel', '0.003', '--no-depth-filter', '--estimate-poses', '--photometric'])
  mod.main()
  assert os.path.getsize(tmp_path / 'model' / 'model.obj') > 10000
  out = np.stack([np.loadtxt(tmp_path / 'cam_in_ob_estimated' / f'{k:04d}.txt').reshape(4, 4) for k in range(n)])
  G = out[0] @ np.linalg.inv(truth[0])
  err = [A.displacement(np.linalg.inv(G) @ out[k], truth[k]) * 1e3 for k in range(1, n)]
  print(f'displacement of frames 1 .. {n - 1} in the first frame\'s object frame: {np.round(err, 3)} mm')
  assert max(err) < 1.0
  with_term, _ = estimate_view_poses(str(tmp_path), depth_filter=False, photometric=True)
  without, _ = estimate_view_poses(str(tmp_path), depth_filter=False)
  assert np.array_equal(out, with_term) and not np.array_equal(out[1:], without[1:])
  monkeypatch.setattr('sys.argv', ['reconstruct_object.py', str(tmp_path), '--refine-poses', '--photometric'])
  with pytest.raises(SystemExit):
    mod.main()
