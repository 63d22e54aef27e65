"""GPU: frame-to-model alignment of depth maps to the fused volume (fp_tsdf_align in csrc/tsdf.hip, TsdfVolume.align_step / align and
refine_view_poses in foundationpose_amd/reconstruct.py) against the numpy restatement of the header's rule (tests/tsdf_align_oracle.py):
the per-pixel rows bit for bit, the sums within the bound of any summation order of exact terms, the solver and the sequential procedure
against the restatement's own runs, and through reconstruct_object on rendered views of the mustard bottle.

Shapes: 40 x 36 x 33 points at 4 mm; 5 views of 64 x 48 of three spheres (3 tiles of 1024 pixels per view) and of 50 x 37 (1850 pixels: a
ragged last tile, rows that straddle tiles), masks on every view, view 4 pushed 3.8 cm so that part of it leaves the volume and part lies in
observed free space (truncated samples), and a second volume fused from 2 views only (unobserved corners)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import tsdf_align_oracle as A
from tests import tsdf_oracle as O

pytestmark = pytest.mark.gpu
DIMS, VOXEL = (40, 36, 33), 0.004
ORIGIN = np.array([-0.004, -0.006, 0.004]) - (np.array(DIMS) - 1) * VOXEL / 2 + np.array([0.0007, -0.0011, 0.0013])


def _case(H, W, focal):
  """`focal`: the focal length of a centred camera, or a camera matrix"""
  K = np.array([[focal, 0, W / 2 - 0.5], [0, focal, H / 2 - 0.5], [0, 0, 1.0]]) if np.ndim(focal) == 0 else focal
  poses = np.stack([O.look_at(e) for e in O.fibonacci_eyes(5, 0.4)])
  depths = np.stack([A.scene_depth(p, K, H, W) for p in poses])
  masks = (depths > 0).astype(np.uint8)
  masks[0, :H // 6], masks[1, :, :W // 3], masks[2, :, W - W // 3:], masks[3, H // 2 + H // 8:], masks[4, :H // 5] = 0, 0, 0, 0, 0
  rs = np.random.RandomState(7)
  query = np.stack([A.perturb(p, 0.003, 1.0, rs) for p in poses])
  query[4] = A.expm_se3([0.03, -0.012, 0.02, 0, 0, 0.05]) @ poses[4]
  return dict(K=K, poses=poses, depths=depths, masks=masks, query=query, H=H, W=W)


@pytest.fixture(scope='module')
def case():
  return _case(48, 64, 130.0)


@pytest.fixture(scope='module')
def oracle_volumes(case):
  full, two = O.Volume(ORIGIN, VOXEL, DIMS), O.Volume(ORIGIN, VOXEL, DIMS)
  full.integrate(case['depths'], case['K'], case['poses'])
  two.integrate(case['depths'][:2], case['K'], case['poses'][:2])
  return full, two


@pytest.fixture(scope='module')
def device_volumes(case):
  from foundationpose_amd.reconstruct import TsdfVolume
  full, two = TsdfVolume(ORIGIN, VOXEL, DIMS), TsdfVolume(ORIGIN, VOXEL, DIMS)
  full.integrate(case['depths'], case['K'], case['poses'])
  two.integrate(case['depths'][:2], case['K'], case['poses'][:2])
  return full, two


@pytest.fixture(scope='module')
def oracle_rows(case, oracle_volumes):
  """the restated rows of the 5 query views against the full volume, and which condition skipped how many pixels of each view"""
  out = [A.rows(oracle_volumes[0], case['depths'][v], case['K'], case['query'][v], case['masks'][v], reasons=True) for v in range(5)]
  return np.stack([o[0] for o in out]), [{k: int(m.sum()) for k, m in o[1].items()} for o in out]


@pytest.fixture(scope='module')
def device_step(case, device_volumes):
  return device_volumes[0].align_step(case['depths'], case['K'], case['query'], masks=case['masks'], rows=True)


def _same_bits(a, b):
  return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_rows_are_bit_equal_to_the_restatement(case, oracle_volumes, device_volumes, oracle_rows, device_step):
  want, why = oracle_rows
  for v in range(5):
    print(f'view {v}: {int(want[v, ..., 7].sum())} valid; skipped {why[v]}')
    assert want[v, ..., 7].sum() >= 200
  for kind in ('depth', 'mask', 'outside', 'unobserved', 'truncated'):
    assert sum(w[kind] for w in why) > 0, f'no pixel is skipped for: {kind}'
  got = device_step[1].cpu().numpy()
  print(f'differing words: {(got.view(np.uint32) != want.view(np.uint32)).sum()} of {want.size}')
  assert _same_bits(got, want)
  # the volume fused from two views: most cells around the far side have an unobserved corner
  out = [A.rows(oracle_volumes[1], case['depths'][v], case['K'], case['query'][v], case['masks'][v], reasons=True) for v in range(5)]
  assert sum(int(o[1]['unobserved'].sum()) for o in out) >= 1000 and all(o[0][..., 7].sum() >= 50 for o in out)
  _, got2 = device_volumes[1].align_step(case['depths'], case['K'], case['query'], masks=case['masks'], rows=True)
  assert _same_bits(got2.cpu().numpy(), np.stack([o[0] for o in out]))


def test_rows_and_sums_on_a_ragged_image_without_masks(oracle_volumes, device_volumes):
  """50 x 37 pixels: 1850 = 1024 + 826, image rows straddle the tile border and the last tile is not full; no mask; a zfar that cuts"""
  c = _case(37, 50, 100.0)
  zfar = float(np.median(c['depths'][c['depths'] > 0]))
  want = np.stack([A.rows(oracle_volumes[0], c['depths'][v], c['K'], c['query'][v], None, zfar=zfar) for v in range(5)])
  assert all(20 <= want[v, ..., 7].sum() < (c['depths'][v] > 0).sum() * 0.9 for v in range(5))
  sums, got = device_volumes[0].align_step(c['depths'], c['K'], c['query'], zfar=zfar, rows=True)
  assert _same_bits(got.cpu().numpy(), want)
  assert np.array_equal(sums[:, 28], want[..., 7].reshape(5, -1).sum(1))


def test_sums_are_within_the_bound_of_any_summation_order(oracle_rows, device_step):
  """Every term is a product of two fp32 numbers, exact in double; n exact terms added in double in any order differ from the exactly
  rounded sum (math.fsum) by at most (n - 1) 2^-53 sum |terms| (1 + O(2^-53)) - the bound asserted is n 2^-52 sum |terms|.  The count
  is a sum of ones: exact."""
  want, _ = oracle_rows
  worst = 0.0
  for v in range(5):
    ref, scale = A.sums(want[v])
    n = ref[28]
    err = np.abs(device_step[0][v] - ref)
    bound = n * 2.0 ** -52 * scale
    worst = max(worst, (err[:28] / np.maximum(bound[:28], 1e-300)).max())
    assert (err <= bound).all(), (v, err / bound)
    assert device_step[0][v, 28] == n
  print(f'largest |sum - fsum| / bound: {worst:.3e}')


SKEW = O.skew_camera(5, 7, 130.0)      # fy = 1.25 fx, cx and cy off the middle by different amounts


@pytest.mark.parametrize('H,W,focal', [(96, 100, 200.0), (5, 7, 130.0), (48, 64, 130.0), pytest.param(5, 7, SKEW, id='5-7-fx != fy')])
def test_sums_have_the_bits_of_the_stated_order(H, W, focal, device_volumes):
  """The device's sums against tests/gn_sums_oracle.py (the order stated in csrc/gn_sums.h) applied to the device's own rows, bit for
  bit.  96 x 100: 10 tiles - the fold's body of eight and a remainder of two - and a last tile of 384 pixels; 5 x 7: one tile of which
  three waves hold padding only; 48 x 64: the masked case of this file, 3 whole tiles."""
  from tests import gn_sums_oracle as G
  c = _case(H, W, focal)
  sums, rows = device_volumes[0].align_step(c['depths'], c['K'], c['query'], masks=c['masks'], rows=True)
  rows = rows.cpu().numpy()
  want = np.stack([G.device_sums(rows[v]) for v in range(5)])
  print(f'{H} x {W}: valid per view {sums[:, 28]}; differing words {(sums.view(np.uint64) != want.view(np.uint64)).sum()} of {want.size}')
  assert sums[:, 28].sum() > 0
  assert np.array_equal(sums.view(np.uint64), want.view(np.uint64))


def test_rows_under_a_camera_with_fx_not_fy(oracle_volumes, device_volumes):
  """5 x 7 pixels through SKEW, without masks (a mask of the case would cut all of so small a view): a kernel that takes fx for fy or
  cx for cy in the back-projection differs from the restatement.  Every view has valid pixels."""
  c = _case(5, 7, SKEW)
  want = np.stack([A.rows(oracle_volumes[0], c['depths'][v], c['K'], c['query'][v], None) for v in range(5)])
  print(f'valid per view {[int(w[..., 7].sum()) for w in want]}')
  assert all(w[..., 7].sum() > 0 for w in want)
  sums, got = device_volumes[0].align_step(c['depths'], c['K'], c['query'], rows=True)
  assert _same_bits(got.cpu().numpy(), want)
  assert np.array_equal(sums[:, 28], want[..., 7].reshape(5, -1).sum(1))


def test_a_view_does_not_depend_on_its_batch(case, device_volumes, device_step):
  vol = device_volumes[0]
  d, m, q, K = case['depths'], case['masks'], case['query'], case['K']
  again = vol.align_step(d, K, q, masks=m)
  assert np.array_equal(again, device_step[0])                                         # two runs
  alone = vol.align_step(d[3:4], K, q[3:4], masks=m[3:4])
  assert np.array_equal(alone[0], device_step[0][3])                                    # alone
  order = [3, 0, 1, 2, 4]
  first = vol.align_step(d[order], K, q[order], masks=m[order])
  assert np.array_equal(first[0], device_step[0][3])                                    # at index 0 of 5
  order = [0, 1, 2, 4, 3]
  last = vol.align_step(d[order], K, q[order], masks=m[order])
  assert np.array_equal(last[4], device_step[0][3]) and np.array_equal(last[3], device_step[0][4])      # at index 4 of 5
  singles = np.stack([vol.align_step(d[v:v + 1], K, q[v:v + 1], masks=m[v:v + 1])[0] for v in range(5)])
  assert np.array_equal(singles, device_step[0])                                        # one batched step = five single steps
  assert (device_step[0][:, 28] >= 200).all() and len(np.unique(device_step[0][:, 27])) == 5


def test_zero_views_write_nothing(case, device_volumes):
  from foundationpose_amd._lib import lib, ptr, stream_ptr
  vol = device_volumes[0]
  sums = np.full(29, 7.0)
  depth = torch.zeros((1, 48, 64), device=vol.device)
  K = np.ascontiguousarray(case['K'])
  rc = lib().fp_tsdf_align(vol.ctx.handle, vol.handle, ptr(depth), None, 0, 48, 64, ptr(K), ptr(np.ascontiguousarray(case['poses'][:1])), 1.0, 1.0,
                           None, ptr(sums), stream_ptr(vol.device))
  assert rc == 0 and (sums == 7.0).all()
  assert vol.align_step(np.zeros((0, 48, 64), dtype=np.float32), K, np.zeros((0, 4, 4))).shape == (0, 29)


def test_parameter_errors(case, device_volumes):
  from foundationpose_amd import _lib
  from foundationpose_amd._lib import lib, ptr, stream_ptr
  vol = device_volumes[0]
  dev = vol.device
  depth = torch.as_tensor(case['depths'][:1], device=dev).contiguous()
  K0, pose0, sums = np.ascontiguousarray(case['K']), np.ascontiguousarray(case['poses'][:1]), np.zeros(29)

  def call(ctx=vol.ctx.handle, v=vol.handle, d=ptr(depth), n=1, H=48, W=64, K=K0, pose=pose0, zfar=1.0, mw=1.0, out=sums):
    return lib().fp_tsdf_align(ctx, v, d, None, n, H, W, ptr(K), ptr(pose), zfar, mw, None, ptr(out), stream_ptr(dev))
  assert call() == 0 and sums[28] > 0
  for kw in (dict(ctx=None), dict(v=None), dict(d=None), dict(K=None), dict(pose=None), dict(out=None), dict(n=-1), dict(n=_lib.FP_TSDF_MAX_VIEWS + 1),
             dict(H=0), dict(W=-3), dict(zfar=0.0), dict(zfar=-1.0), dict(mw=0.0), dict(mw=float('nan'))):
    assert call(**kw) == _lib.FP_EINVAL, kw
  for i, val in ((0, 0.0), (4, -5.0), (4, float('nan'))):
    Kb = K0.copy()
    Kb.reshape(-1)[i] = val
    assert call(K=Kb) == _lib.FP_EINVAL, (i, val)
  for idx, val in (((0, 3, 3), 0.0), ((0, 3, 0), 1e-9), ((0, 1, 1), np.nan), ((0, 2, 3), np.inf)):
    pb = pose0.copy()
    pb[idx] = val
    assert call(pose=pb) == _lib.FP_EINVAL, (idx, val)
  assert call(zfar=float('inf')) == 0
  torch.cuda.synchronize()


def test_a_volume_never_integrated_into_skips_everything(case):
  from foundationpose_amd.reconstruct import TsdfVolume
  vol = TsdfVolume(ORIGIN, VOXEL, DIMS)
  sums, rows = vol.align_step(case['depths'], case['K'], case['query'], masks=case['masks'], rows=True)
  assert (sums == 0).all() and (rows == 0).all()
  got, info = vol.align(case['depths'], case['K'], case['query'], masks=case['masks'])
  assert np.array_equal(got, case['query']) and info['stopped'] == {v: 'too few valid pixels' for v in range(5)}


# ---- the solver against the restatement's loop ------------------------------------------------------------------------------------------
N, H2, W2, FOCAL, VOXEL2 = 8, 72, 96, 220.0, 0.003      # the scene of tests/test_tsdf_align_host.py


@pytest.fixture(scope='module')
def scene():
  K, poses, depths, masks = A.scene_views(N, H2, W2, FOCAL)
  origin, dims = A.volume_for(depths, masks, K, poses, VOXEL2, 5 * VOXEL2 + 0.01)
  ref = O.Volume(origin, VOXEL2, dims)
  ref.integrate(depths, K, poses, masks=masks)
  return dict(K=K, poses=poses, depths=depths, masks=masks, origin=origin, dims=dims, ref=ref)


def test_align_follows_the_restatement(scene):
  """Views 2 and 5 from seeded 3 mm / 1 degree perturbations, both in one batch, against the same loop on the restatement.  After the first
  step the poses agree to 1e-9: the 6 x 6 systems differ by the summation order only (relative 1e-13 in the sums, a condition number
  of 1e3 - 1e4 with rotations in radians and translations in metres).  At the end the mean displacement over the 5 cm ball is at most
  1.5 x the restatement's own final value (view 2: 0.464 mm, tests/test_tsdf_align_host.py) and below the start."""
  from foundationpose_amd.reconstruct import TsdfVolume
  vs = [2, 5]
  rs = np.random.RandomState(3)
  start = np.stack([A.perturb(scene['poses'][v], 0.003, 1.0, rs) for v in vs])
  want, winfo = A.align(scene['ref'], scene['depths'][vs], scene['K'], start, scene['masks'][vs])
  vol = TsdfVolume(scene['origin'], VOXEL2, scene['dims'])
  vol.integrate(scene['depths'], scene['K'], scene['poses'], masks=scene['masks'])
  got, info = vol.align(scene['depths'][vs], scene['K'], start, masks=scene['masks'][vs])
  first = np.abs(info['after_first'] - winfo['after_first']).max()
  print(f'after the first step: max |pose - restatement| {first:.3e}')
  assert first <= 1e-9
  assert np.array_equal(info['valid'][0], winfo['valid'][0])
  for k, v in enumerate(vs):
    d0, dw, dg = (A.displacement(p, scene['poses'][v]) for p in (start[k], want[k], got[k]))
    print(f'view {v}: {1e3 * d0:.3f} mm -> {1e3 * dg:.3f} mm (restatement {1e3 * dw:.3f} mm); stopped: {info["stopped"].get(k)}; '
          f'rms {1e3 * info["rms"][0, k]:.3f} -> {1e3 * info["rms"][-1, k]:.3f} mm')
    assert dg <= 1.5 * dw and dg < d0
  assert info['rms'].shape[1] == 2 and set(info['stopped']) <= {0, 1}


def test_refine_view_poses_end_to_end():
  """10 views of 96 x 72 of the three spheres, 3 mm voxels, view 0 true (the anchor), the others perturbed by 4 mm / 1.5 degrees (seeded).
  The restatement's sequential procedure (tsdf_align_oracle.refine_view_poses, greedy order 0 3 2 5 8 6 9 7 4 1), mean displacement over
  the 5 cm ball in mm, views 1 .. 9:   before 4.061 4.084 4.052 4.074 4.063 4.072 4.071 4.050 4.050 (mean 4.064)
                                       after  0.111 0.278 0.133 0.249 0.246 0.174 0.245 2.738 0.253 (mean 0.492)
  View 8 is the weakly constrained one: it sees the spheres nearly in line.  The GPU mean must be within 1.5 x the recorded mean and
  below the start; no per-view maximum is asserted."""
  from foundationpose_amd.reconstruct import refine_view_poses
  K, truth, depths, masks, given = A.refine_case()
  got, info = refine_view_poses(dict(depths=depths, masks=masks, K=K, cam_in_obs=given), voxel_size=VOXEL2, depth_filter=False)
  before = np.array([A.displacement(given[v], truth[v]) for v in range(10)]) * 1e3
  after = np.array([A.displacement(got[v], truth[v]) for v in range(10)]) * 1e3
  print(f'order {info["order"]}; stopped {info["stopped"]}')
  print(f'before {np.round(before, 3)} mean {before[1:].mean():.3f} mm; after {np.round(after, 3)} mean {after[1:].mean():.3f} mm')
  assert np.array_equal(got[0], given[0])                                      # the anchor: the same bits
  assert after[1:].mean() <= 1.5 * A.RECORDED_MEAN_MM and after[1:].mean() < before[1:].mean()
  assert sorted(info['order']) == list(range(10)) and info['order'][0] == 0
  assert all(0 < v < 10 and isinstance(why, str) and why for v, why in info['stopped'].items())
  assert (info['valid'][1:] >= 100).all() and (info['rms'][1:] > 0).all()
  # a view that cannot be aligned is fused at its given pose and named
  blind = depths.copy()
  blind[4] = 0
  got2, info2 = refine_view_poses(dict(depths=blind, masks=masks, K=K, cam_in_obs=given), voxel_size=VOXEL2, depth_filter=False, iterations=2)
  assert np.array_equal(got2[4], given[4]) and info2['stopped'][4] == 'too few valid pixels'


# ---- through reconstruct_object: rendered views of the mustard bottle ----------------------------------------------------------------------
(MH, MW), MVOXEL, MK = O.MUSTARD_HW, O.MUSTARD_VOXEL, O.MUSTARD_K


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


def test_refined_poses_give_a_better_mesh(mustard_views):
  """The 12 mustard views of tests/test_gpu_tsdf.py with every pose but the first perturbed by 4 mm / 1.5 degrees (seeded): the fraction of
  the fused vertices beyond the radial bound from the source surface is lower with refine_poses=True than without.  A CPU experiment with the checker's renderer and filters
  (160 x 120 pixels, 4 mm voxels, depth filter on): true poses 0.0053, given poses 0.0555, refined 0.0227 (on an MI355X:
  true 0.0040, given 0.0569; the test prints given and refined); the mean displacement
  of views 1 .. 11 goes from 4.06 mm to 2.67 mm.  DESIGN.md section 5 has the table, and what the refinement needs for that: a
  2-voxel band and depth maps that are eroded but not filled."""
  from foundationpose_amd.reconstruct import reconstruct_object
  views, sc = mustard_views
  rs = np.random.RandomState(31)
  given = views['cam_in_obs'].copy()
  for v in range(1, len(given)):
    given[v] = A.perturb(given[v], 0.004, 1.5, rs)
  off = dict(views, cam_in_obs=given)
  plain = reconstruct_object(off, voxel_size=MVOXEL)
  refined = reconstruct_object(off, voxel_size=MVOXEL, refine_poses=True)
  f_plain, far_plain = O.fraction_beyond_bound(plain.vertices, sc['mesh'].vertices, sc['mesh'].faces, MVOXEL)
  f_ref, far_ref = O.fraction_beyond_bound(refined.vertices, sc['mesh'].vertices, sc['mesh'].faces, MVOXEL)
  print(f'beyond {O.RADIAL_BOUND_VOXELS:.2f} voxels: given poses {f_plain:.4f} (max {far_plain:.2f} voxels), refined {f_ref:.4f} (max {far_ref:.2f} voxels)')
  assert len(refined.faces) > 5000
  assert f_ref < f_plain


def test_the_default_is_unchanged(mustard_views):
  from foundationpose_amd.reconstruct import reconstruct_object
  views = mustard_views[0]
  a, b = reconstruct_object(views, voxel_size=MVOXEL), reconstruct_object(views, voxel_size=MVOXEL, refine_poses=False)
  assert np.array_equal(a.vertices, b.vertices) and np.array_equal(a.faces, b.faces) and len(a.faces) > 5000
  assert np.array_equal(a.vertex_normals, b.vertex_normals) and np.array_equal(a.visual.vertex_colors, b.visual.vertex_colors)


# ---- the options of the procedure, the cut into calls, the script ------------------------------------------------------------------------
def test_more_views_than_one_call(case, device_volumes, device_step):
  """65 views (the 5 of the case 13 times) are cut into calls of FP_TSDF_MAX_VIEWS = 64 and 1: every copy gets the bits of its original"""
  from foundationpose_amd import _lib
  reps = 13
  assert 5 * reps == _lib.FP_TSDF_MAX_VIEWS + 1
  tile = lambda a: np.concatenate([a] * reps)
  sums, rows = device_volumes[0].align_step(tile(case['depths']), case['K'], tile(case['query']), masks=tile(case['masks']), rows=True)
  assert np.array_equal(sums, tile(device_step[0]))
  assert torch.equal(rows, torch.cat([device_step[1]] * reps))


def test_misaligned_rows_are_refused(case, device_volumes):
  from foundationpose_amd import _lib
  from foundationpose_amd._lib import lib, ptr, stream_ptr
  vol = device_volumes[0]
  depth = torch.as_tensor(case['depths'][:1], device=vol.device).contiguous()
  buf = torch.zeros(48 * 64 * 8 + 4, device=vol.device)
  assert buf.data_ptr() % 16 == 0
  K, pose, sums = np.ascontiguousarray(case['K']), np.ascontiguousarray(case['query'][:1]), np.zeros(29)
  call = lambda off: lib().fp_tsdf_align(vol.ctx.handle, vol.handle, ptr(depth), None, 1, 48, 64, ptr(K), ptr(pose), 1.0, 1.0,
                                         ctypes.c_void_p(buf.data_ptr() + off), ptr(sums), stream_ptr(vol.device))
  assert call(4) == _lib.FP_EINVAL and b'aligned' in lib().fp_last_error() and (buf == 0).all()
  assert call(16) == 0 and sums[28] > 0
  torch.cuda.synchronize()


def test_max_step_limits_a_step(scene):
  """max_step = (0.5 mm, 0.002 rad) on a view that is 3 mm / 1 degree off: the first step exp(xi) has a rotation of at most 0.002 rad and
  a translation part of at most 0.5 mm (xi is scaled as a whole, so one of the two is met with equality)"""
  from foundationpose_amd.reconstruct import TsdfVolume
  vol = TsdfVolume(scene['origin'], VOXEL2, scene['dims'])
  vol.integrate(scene['depths'], scene['K'], scene['poses'], masks=scene['masks'])
  start = A.perturb(scene['poses'][2], 0.003, 1.0, np.random.RandomState(3))[None]
  free, _ = vol.align(scene['depths'][2:3], scene['K'], start, masks=scene['masks'][2:3], iterations=1)
  held, info = vol.align(scene['depths'][2:3], scene['K'], start, masks=scene['masks'][2:3], iterations=1, max_step=(0.0005, 0.002))
  E = held[0] @ np.linalg.inv(start[0])
  angle = np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1))
  shift = np.linalg.norm(E[:3, 3])                  # |V u| with V = I + O(angle): within 0.2 % of |u|
  print(f'limited step: {angle:.6f} rad, {1e3 * shift:.4f} mm; free step moves {1e3 * A.displacement(free[0], start[0]):.3f} mm')
  assert angle <= 0.002 * 1.002 and shift <= 0.0005 * 1.002
  assert max(angle / 0.002, shift / 0.0005) >= 0.99
  assert A.displacement(held[0], start[0]) < A.displacement(free[0], start[0])


def test_order_and_rounds_of_refine_view_poses():
  """On the 10 views of the end-to-end case: order='index' and an explicit sequence are followed, a wrong sequence or word is refused, and
  rounds=1 (fuse everything again, align all views but the anchor in ONE batched call) keeps the anchor's bits, reports every view and
  stays below the start - it moves the poses (the sequential result is not its fixed point) but is not asserted to improve them: on
  this scene whole-model rounds add little (the issue's prototype)."""
  from foundationpose_amd.reconstruct import refine_view_poses
  K, truth, depths, masks, given = A.refine_case()
  views = dict(depths=depths, masks=masks, K=K, cam_in_obs=given)
  mean = lambda ps: float(np.mean([A.displacement(ps[v], truth[v]) for v in range(1, 10)])) * 1e3
  _, info = refine_view_poses(views, voxel_size=VOXEL2, depth_filter=False, order='index', iterations=2)
  assert info['order'] == list(range(10))
  seq = [9, 8, 7, 6, 5, 4, 3, 2, 1]
  _, info = refine_view_poses(views, voxel_size=VOXEL2, depth_filter=False, order=seq, iterations=2)
  assert info['order'] == [0] + seq
  for bad in ([1, 2, 3], seq + [9], 'nearest'):
    with pytest.raises(ValueError):
      refine_view_poses(views, voxel_size=VOXEL2, depth_filter=False, order=bad)
  with pytest.raises(ValueError):
    refine_view_poses(views, voxel_size=VOXEL2, depth_filter=False, anchor=10)
  plain, _ = refine_view_poses(views, voxel_size=VOXEL2, depth_filter=False)
  got, info = refine_view_poses(views, voxel_size=VOXEL2, depth_filter=False, rounds=1)
  print(f'mean displacement: given {mean(given):.3f} mm, sequential {mean(plain):.3f} mm, with one whole-model round {mean(got):.3f} mm')
  assert np.array_equal(got[0], given[0]) and mean(got) < mean(given)
  assert not np.array_equal(got[1:], plain[1:])
  assert (info['valid'][1:] >= 100).all() and (info['rms'][1:] > 0).all() and info['valid'][0] == 0


def test_script_writes_refined_poses(tmp_path, monkeypatch):
  """scripts/reconstruct_object.py DIR --refine-poses on a folder in the reference's layout (4 views of the three spheres, depth in
  millimetres): the mesh, and DIR/cam_in_ob_refined/NAME.txt with the anchor as given and the other views moved towards the truth"""
  import importlib.util
  import os
  from PIL import Image
  K, truth, depths, masks, given = A.refine_case()
  keep = [0, 3, 2, 5]                                # the first views of the greedy order: neighbours of the anchor
  for sub in ('rgb', 'depth', 'mask', 'cam_in_ob'):
    os.makedirs(tmp_path / sub)
  np.savetxt(tmp_path / 'K.txt', K, fmt='%.18e')
  for k, v in enumerate(keep):
    name = f'{k:04d}'
    Image.fromarray(np.full(depths[v].shape + (3,), 128, dtype=np.uint8)).save(tmp_path / 'rgb' / f'{name}.png')
    Image.fromarray(np.round(depths[v].astype(np.float64) * 1e3).astype(np.uint16)).save(tmp_path / 'depth' / f'{name}.png')
    Image.fromarray(masks[v] * 255).save(tmp_path / 'mask' / f'{name}.png')
    np.savetxt(tmp_path / 'cam_in_ob' / f'{name}.txt', given[v], fmt='%.18e')
  repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  spec = importlib.util.spec_from_file_location('reconstruct_object_script', os.path.join(repo, 'scripts', 'reconstruct_object.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  monkeypatch.setattr('sys.argv', ['reconstruct_object.py', str(tmp_path), '--voxel', '0.003', '--no-depth-filter', '--refine-poses'])
  mod.main()
  assert os.path.getsize(tmp_path / 'model' / 'model.obj') > 10000
  out = [np.loadtxt(tmp_path / 'cam_in_ob_refined' / f'{k:04d}.txt').reshape(4, 4) for k in range(4)]
  assert np.array_equal(out[0], given[0])
  before = np.mean([A.displacement(given[v], truth[v]) for v in keep[1:]])
  after = np.mean([A.displacement(out[k], truth[v]) for k, v in enumerate(keep) if k])
  print(f'mean displacement {1e3 * before:.3f} -> {1e3 * after:.3f} mm')
  assert after < before
