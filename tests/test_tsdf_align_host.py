"""CPU: the numpy restatement of the alignment rule (tests/tsdf_align_oracle.py) against analytic truth - three ray-cast spheres seen from
known poses - and the argument checks of fp_tsdf_align that need no GPU.  The GPU tests (tests/test_gpu_tsdf_align.py) hold the kernel to
this restatement bit for bit, so what is shown here about the rule holds for it."""
import ctypes

import numpy as np
import pytest

from tests import tsdf_align_oracle as A
from tests import tsdf_oracle as O

N, H, W, FOCAL, VOXEL = 8, 72, 96, 220.0, 0.003


@pytest.fixture(scope='module')
def scene():
  K, poses, depths, masks = A.scene_views(N, H, W, FOCAL)
  origin, dims = A.volume_for(depths, masks, K, poses, VOXEL, 5 * VOXEL + 0.01)
  vol = O.Volume(origin, VOXEL, dims)
  vol.integrate(depths, K, poses, masks=masks)
  return dict(K=K, poses=poses, depths=depths, masks=masks, vol=vol)


def _ratio(s):
  diag = np.array([s[e] for e, (i, j) in enumerate(A.PAIRS) if i == j])
  return np.abs(s[21:27]) / np.sqrt(diag * s[27])


def test_truth_is_nearly_stationary(scene):
  """At the true poses, against the model fused from them: b_k^2 / A_kk is the part of sum r^2 that the best step along axis k alone
  removes (Cauchy-Schwarz: at most all of it).  It stays under a half for every axis and view - the residual is the fusion's own
  discretisation (RMS 1.05 - 1.30 mm at 3 mm voxels), not a pose error - and under its value at a pose that is 3 mm / 1 degree off.
  The full Gauss-Newton step from truth moves the 5 cm ball by less than a voxel (measured: 0.31 - 0.47 mm)."""
  s = A.step_sums(scene['vol'], scene['depths'], scene['K'], scene['poses'], scene['masks'])
  rs = np.random.RandomState(1)
  off = np.stack([A.perturb(p, 0.003, 1.0, rs) for p in scene['poses']])
  s_off = A.step_sums(scene['vol'], scene['depths'], scene['K'], off, scene['masks'])
  for v in range(N):
    rho, rho_off = _ratio(s[v]).max(), _ratio(s_off[v]).max()
    moved = A.displacement(A.expm_se3(A.solve_step(s[v])) @ scene['poses'][v], scene['poses'][v])
    print(f'view {v}: {int(s[v, 28])} valid, rms {1e3 * np.sqrt(s[v, 27] / s[v, 28]):.3f} mm, max b/sqrt(A rr) {rho:.3f} (off pose {rho_off:.3f}), '
          f'step from truth {1e3 * moved:.3f} mm')
    assert s[v, 28] >= 1000
    assert rho ** 2 < 0.5 and rho < rho_off
    assert moved < VOXEL


def test_analytic_jacobian_is_the_derivative_of_the_residual(scene):
  """J of a pixel against the central difference of r under exp(eps e_k), both of the same trilinear interpolant, the difference in
  float64, on valid pixels at least a tenth of a cell from every cell face (eps moves a point by 1e-6 m at most: 3e-4 cells).
  Tolerance 3e-4: J is fp32 - the point's coordinates carry up to 4 roundings of 2^-24 x 0.5 m, 4e-5 cells at 3 mm; the gradient
  changes by at most 2 (the second difference of T in [-1, 1]) x trunc / v = 4 per cell - and rotation entries are scaled by |x| < 1.
  A wrong sign, axis or corner is an error of order 1."""
  vol, K, v = scene['vol'], scene['K'], 3
  rs = np.random.RandomState(2)
  pose = A.perturb(scene['poses'][v], 0.002, 0.5, rs)
  rw = A.rows(vol, scene['depths'][v], K, pose, scene['masks'][v])
  pix = np.argwhere(rw[..., 7] > 0)
  _, f = A.residual64(vol, scene['depths'][v], K, pose, pix)
  pix = pix[((f > 0.1) & (f < 0.9)).all(1)]
  assert len(pix) >= 200
  r0, _ = A.residual64(vol, scene['depths'][v], K, pose, pix)
  assert np.abs(r0 - rw[pix[:, 0], pix[:, 1], 6]).max() < 1e-6
  worst = 0.0
  for k in range(6):
    eps = 1e-6 * np.eye(6)[k]
    rp, _ = A.residual64(vol, scene['depths'][v], K, A.expm_se3(eps) @ pose, pix)
    rm, _ = A.residual64(vol, scene['depths'][v], K, A.expm_se3(-eps) @ pose, pix)
    worst = max(worst, np.abs((rp - rm) / 2e-6 - rw[pix[:, 0], pix[:, 1], k].astype(np.float64)).max())
  print(f'{len(pix)} pixels: max |J - finite difference| {worst:.3e}')
  assert worst < 3e-4
  assert np.abs(rw[pix[:, 0], pix[:, 1], :3]).max() > 0.5      # the gradient of a distance field: of order 1


def test_single_view_converges_from_a_perturbed_pose(scene):
  """View 2 from a seeded 3 mm / 1 degree perturbation against the model fused from the true poses: mean displacement over the 5 cm ball
  3.051 mm -> 0.464 mm (96 x 72 pixels, 3 mm voxels: 0.15 voxels), the RMS residual 3.877 mm -> 0.958 mm; at the true pose it is 1.120 mm
  (the refined pose fits this view's own discretisation better than truth does).  The loop stops when the residual no longer falls."""
  v = 2
  start = A.perturb(scene['poses'][v], 0.003, 1.0, np.random.RandomState(3))
  got, info = A.align(scene['vol'], scene['depths'][v:v + 1], scene['K'], start[None], scene['masks'][v:v + 1])
  d0, d1 = A.displacement(start, scene['poses'][v]), A.displacement(got[0], scene['poses'][v])
  d_first = A.displacement(info['after_first'][0], scene['poses'][v])
  print(f'displacement {1e3 * d0:.3f} -> {1e3 * d_first:.3f} (one step) -> {1e3 * d1:.3f} mm; rms {1e3 * info["rms"][:, 0]} mm; {info["stopped"]}')
  assert d1 < d_first < d0
  assert d1 < VOXEL / 2
  assert (np.diff(info['rms'][:-1, 0]) < 0).all() and info['valid'][0, 0] >= 1000


def test_a_view_that_sees_nothing_keeps_its_pose(scene):
  empty = O.Volume(scene['vol'].origin, VOXEL, scene['vol'].dims)
  got, info = A.align(empty, scene['depths'][:1], scene['K'], scene['poses'][:1], scene['masks'][:1])
  assert np.array_equal(got, scene['poses'][:1]) and info['stopped'] == {0: 'too few valid pixels'} and info['valid'][0, 0] == 0


def test_sequential_refinement_reproduces_its_record():
  """The restatement's run of the sequential procedure on refine_case(): the displacements recorded in tsdf_align_oracle (to a micrometre),
  which the GPU test of refine_view_poses is judged against.  Mean over views 1 .. 9: 4.064 mm -> 0.492 mm; view 8, which sees the three
  spheres nearly in line, stays at 2.7 mm."""
  K, truth, depths, masks, given = A.refine_case()
  got, info = A.refine_view_poses(depths, masks, K, given, VOXEL, 5 * VOXEL + 0.01)
  before = np.array([A.displacement(given[v], truth[v]) for v in range(10)]) * 1e3
  after = np.array([A.displacement(got[v], truth[v]) for v in range(10)]) * 1e3
  print(f'order {info["order"]}; before {np.round(before, 3)}; after {np.round(after, 3)} mean {after[1:].mean():.3f} mm')
  assert np.abs(before - A.RECORDED_BEFORE_MM).max() < 1e-3 and np.abs(after - A.RECORDED_AFTER_MM).max() < 1e-3
  assert abs(after[1:].mean() - A.RECORDED_MEAN_MM) < 1e-3 and np.array_equal(got[0], given[0])


def test_expm_against_scipy():
  from scipy.linalg import expm
  rs = np.random.RandomState(4)
  for scale in (1e-7, 1e-3, 0.3, 2.5):
    xi = rs.randn(6) * scale
    tw = np.zeros((4, 4))
    tw[:3, :3] = [[0, -xi[5], xi[4]], [xi[5], 0, -xi[3]], [-xi[4], xi[3], 0]]
    tw[:3, 3] = xi[:3]
    assert np.abs(A.expm_se3(xi) - expm(tw)).max() < 1e-13 * max(1.0, scale)


@pytest.fixture(scope='module')
def built():
  import __graft_entry__ as g
  g.build()
  from foundationpose_amd import _lib
  return _lib


def test_product_expm_and_solve_equal_the_restatement(built):
  from foundationpose_amd import reconstruct as R
  rs = np.random.RandomState(5)
  for scale in (1e-6, 0.01, 1.0):
    xi = rs.randn(6) * scale
    assert np.abs(R.expm_se3(xi) - A.expm_se3(xi)).max() < 1e-15
  J, r = rs.randn(50, 6), rs.randn(50)
  s = A.sums(np.concatenate([J, r[:, None], np.ones((50, 1))], 1).astype(np.float32))[0]
  assert np.allclose(R.solve_step(s), A.solve_step(s), rtol=1e-12, atol=0)


def test_argument_checks_need_no_gpu(built):
  L, EINVAL = built.lib(), built.FP_EINVAL
  K = (ctypes.c_double * 9)(100, 0, 4, 0, 100, 4, 0, 0, 1)
  pose = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
  sums = (ctypes.c_double * 29)()
  fake = ctypes.c_void_p(64)                     # never dereferenced: the null and range checks come first
  call = lambda ctx=fake, vol=fake, depth=fake, n=1, Hh=8, Ww=8, Kk=K, p=pose, zfar=1.0, mw=1.0, out=sums: \
      L.fp_tsdf_align(ctx, vol, depth, None, n, Hh, Ww, Kk, p, zfar, mw, None, out, None)
  for kw in (dict(ctx=None), dict(vol=None), dict(depth=None), dict(Kk=None), dict(p=None), dict(out=None)):
    assert call(**kw) == EINVAL and b'null' in L.fp_last_error(), kw
  for kw in (dict(n=-1), dict(n=built.FP_TSDF_MAX_VIEWS + 1), dict(Hh=0), dict(Ww=0), dict(zfar=0.0), dict(zfar=float('nan')), dict(mw=0.0),
             dict(mw=float('nan')), dict(Kk=(ctypes.c_double * 9)(0, 0, 4, 0, 100, 4, 0, 0, 1)),
             dict(Kk=(ctypes.c_double * 9)(100, 0, 4, 0, -1, 4, 0, 0, 1))):
    assert call(**kw) == EINVAL, kw
  bad = np.eye(4)
  bad[3, 3] = 2
  assert call(p=(ctypes.c_double * 16)(*bad.reshape(-1))) == EINVAL and b'last row' in L.fp_last_error()
  bad = np.eye(4)
  bad[1, 2] = np.inf
  assert call(p=(ctypes.c_double * 16)(*bad.reshape(-1))) == EINVAL and b'finite' in L.fp_last_error()
  assert L.fp_tsdf_align(fake, fake, fake, None, 1, 8, 8, K, pose, 1.0, 1.0, ctypes.c_void_p(68), sums, None) == EINVAL and b'aligned' in L.fp_last_error()
  assert built.FP_TSDF_ALIGN_TERMS == 29
