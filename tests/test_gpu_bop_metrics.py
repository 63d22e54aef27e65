"""GPU: BOP pose errors - MSSD and MSPD (fp_pose_errors_bop through Utils.bop_pose_errors) and VSD (fp_vsd through Utils.vsd_errors) -
against float64 restatements of bop_toolkit's definitions, written here from the contract in include/foundationpose_amd.h and fed the
same float32 inputs the kernels read.  VSD is defined on this library's depth renders, so the restatement takes its depths from
nvdiffrast_render and its counts must be EQUAL.  Tolerances of MSSD (2e-6 m + 1e-5 x value) and MSPD (1e-3 px + 1e-5 x value) are what
float32 camera-frame points allow; they are not fitted to measurements."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu


def f64(x):
  return np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float64)


def rot(w):
  w = np.asarray(w, dtype=np.float64)
  th = np.linalg.norm(w)
  if th == 0:
    return np.eye(3)
  Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
  return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def around(gt, n, seed, ang=0.1, trans=0.015):
  """n float32 poses near gt: a random small rotation (left-multiplied) and translation."""
  rs = np.random.RandomState(seed)
  out = np.repeat(np.asarray(gt, dtype=np.float64)[None], n, 0)
  for p in out:
    p[:3, :3] = rot(rs.randn(3) * ang) @ p[:3, :3]
    p[:3, 3] += rs.randn(3) * trans
  return out.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ MSSD / MSPD
def cam(T, pts):
  T = f64(T)
  return pts @ T[..., :3, :3].swapaxes(-1, -2) + T[..., None, :3, 3]


def ref_mssd(pred, gt, pts, sym):
  GS = f64(gt)[None] @ f64(sym)                                                  # (S,4,4)
  return float(np.linalg.norm(cam(pred, pts)[None] - cam(GS, pts), axis=-1).max(1).min())


def proj(X, K):
  return np.stack([K[0, 0] * X[..., 0] / X[..., 2] + K[0, 2], K[1, 1] * X[..., 1] / X[..., 2] + K[1, 2]], -1)


def ref_mspd(pred, gt, pts, sym, K):
  GS = f64(gt)[None] @ f64(sym)
  P, Q = cam(pred, pts), cam(GS, pts)
  d = np.linalg.norm(proj(P, K)[None] - proj(Q, K), axis=-1).max(1)
  d[(P[None, :, 2] <= 0).any(-1) | (Q[..., 2] <= 0).any(-1)] = np.inf
  return float(d.min())


def assert_close(got, ref, abs_tol, what):
  got, ref = f64(got), f64(ref)
  bad = np.abs(got - ref) > abs_tol + 1e-5 * np.abs(ref)
  assert not bad.any(), f'{what}: {bad.sum()} of {bad.size} out of tolerance, worst |diff| {np.abs(got - ref).max():.3e}'


def sym_z73():
  from foundationpose_amd import Utils as U
  return U.symmetry_tfs_from_info({'symmetries_continuous': [{'axis': [0, 0, 1], 'offset': [0, 0, 0]}]}).astype(np.float32)


@pytest.fixture(scope='module')
def mustard():
  sc = util.scene(0)
  hyp = util.hypotheses(sc, 252, jitter_seed=1)
  rs = np.random.RandomState(7)
  for h in hyp:                        # + a small rotation jitter, so no hypothesis is exactly a grid rotation
    h[:3, :3] = (rot(rs.randn(3) * 0.02) @ h[:3, :3]).astype(np.float32)
  return dict(pts=sc['mesh'].vertices.astype(np.float32), hyp=hyp, gt=sc['gt_pose'].astype(np.float32), K=sc['K'])


@pytest.mark.parametrize('n_sym', [0, 73])
@pytest.mark.parametrize('per_pose_gt', [False, True])
def test_mssd_mspd_values(mustard, n_sym, per_pose_gt):
  from foundationpose_amd import Utils as U
  m = mustard
  sym = sym_z73() if n_sym else None
  assert sym is None or len(sym) == 73
  gt = np.repeat(m['gt'][None], 252, 0) if per_pose_gt else m['gt']
  out = U.bop_pose_errors(m['hyp'], gt, m['pts'], K=m['K'], symmetry_tfs=sym)
  assert all(v.shape == (252,) and v.dtype == torch.float for v in out.values())
  pts = m['pts'].astype(np.float64)
  S = np.eye(4)[None] if sym is None else sym
  assert_close(out['mssd'].cpu(), [ref_mssd(h, m['gt'], pts, S) for h in m['hyp']], 2e-6, 'MSSD')
  assert_close(out['mspd'].cpu(), [ref_mspd(h, m['gt'], pts, S, m['K']) for h in m['hyp']], 1e-3, 'MSPD')
  if n_sym:        # the symmetry set helps some poses and never hurts
    plain = U.bop_pose_errors(m['hyp'], gt, m['pts'], K=m['K'])
    assert (out['mssd'] <= plain['mssd']).all() and (out['mssd'] < plain['mssd'] - 1e-3).any()
    assert (out['mspd'] <= plain['mspd']).all()


def test_exact_zeros(mustard):
  from foundationpose_amd import Utils as U
  m = mustard
  poses = np.stack([m['gt'], m['hyp'][0], m['hyp'][200]])
  for sym in (None, sym_z73()):
    out = U.bop_pose_errors(poses, poses, m['pts'], K=m['K'], symmetry_tfs=sym)
    for k, v in out.items():
      assert (v.cpu().numpy() == 0).all(), (k, v)


def box_points(a=0.04, b=0.025, c=0.06, n=9):
  g = np.linspace(-1, 1, n)
  X, Y, Z = np.meshgrid(g * a, g * b, g * c, indexing='ij')
  P = np.stack([X, Y, Z], -1).reshape(-1, 3)
  on_face = (np.abs(P) >= np.array([a, b, c]) - 1e-12).any(1)       # the surface grid, corners included
  return P[on_face].astype(np.float32), (a, b, c)


def test_symmetry_box():
  from foundationpose_amd import Utils as U
  pts, (a, b, c) = box_points()
  S = np.diag([-1.0, -1.0, 1.0, 1.0])
  gt = np.eye(4)
  gt[:3, :3] = rot([0.3, -0.5, 0.2])
  gt[:3, 3] = [0.02, -0.03, 0.7]
  pred = (gt @ S).astype(np.float32)
  gt = gt.astype(np.float32)
  K = np.array([[600.0, 0, 320], [0, 600, 240], [0, 0, 1]])
  with_sym = U.bop_pose_errors(pred[None], gt, pts, K=K, symmetry_tfs=np.stack([np.eye(4), S]))
  assert float(with_sym['mssd'][0]) <= 1e-6
  assert float(with_sym['mspd'][0]) <= 1e-3
  without = float(U.bop_pose_errors(pred[None], gt, pts, K=K, metrics=('mssd',))['mssd'][0])
  want = 2 * np.sqrt(a * a + b * b)                                  # the box's diagonal in the xy plane
  assert abs(without - want) <= 2e-6 + 1e-5 * want, (without, want)


def test_mspd_behind_camera(mustard):
  from foundationpose_amd import Utils as U
  m = mustard
  behind = m['gt'].copy()
  behind[2, 3] = 0.01                                                # the mesh straddles the camera plane
  poses = np.stack([m['hyp'][3], behind])
  out = U.bop_pose_errors(poses, m['gt'], m['pts'], K=m['K'])
  mspd, mssd = out['mspd'].cpu().numpy(), out['mssd'].cpu().numpy()
  assert np.isfinite(mspd[0]) and np.isposinf(mspd[1])
  assert np.isfinite(mssd).all()
  # the ground truth behind the camera: every pose fails
  g = m['gt'].copy()
  g[2, 3] = -0.5
  assert np.isposinf(U.bop_pose_errors(m['hyp'][:4], g, m['pts'], K=m['K'], metrics=('mspd',))['mspd'].cpu().numpy()).all()


# ------------------------------------------------------------------------------------------------------------------------------- VSD
FULL_HD_K = np.array([[1600.0, 0, 955.5], [0, 1600.0, 603.2], [0, 0, 1]])
VSD_DEPTH_BUDGET = 512 << 20          # fp_vsd's bytes of depth images per render chunk (api.hip)


def ref_dist(d, K):
  """bop_toolkit misc.depth_im_to_dist_im_fast, float64"""
  d = np.asarray(d, dtype=np.float64)
  H, W = d.shape
  xs, ys = np.meshgrid(np.arange(W), np.arange(H))
  X = ((xs - K[0, 2]) * d) * (1.0 / K[0, 0])
  Y = ((ys - K[1, 2]) * d) * (1.0 / K[1, 1])
  return np.sqrt(X * X + Y * Y + d * d)


def ref_vsd(dt, dg, de, K, diameter, delta, taus):
  """(counts [|union|, |inter|, cost_tau ..], e) of one pose: bop_toolkit pose_error.vsd, visib_mode='bop19'"""
  Dt, Dg, De = ref_dist(dt, K), ref_dist(dg, K), ref_dist(de, K)
  ft = Dt.astype(np.float32)
  vis = lambda Dm: (Dm > 0) & (((Dm.astype(np.float32) - ft).astype(np.float64) <= delta) | (Dt == 0))
  vg = vis(Dg)
  ve = vis(De) | (vg & (De > 0))
  inter, union = vg & ve, vg | ve
  c = np.abs(Dg[inter] - De[inter]) / diameter
  n_u, n_i = int(union.sum()), int(inter.sum())
  cost = [int((c >= t).sum()) for t in taus]
  e = [1.0] * len(taus) if n_u == 0 else [(k + n_u - n_i) / float(n_u) for k in cost]
  return np.array([n_u, n_i] + cost), np.array(e)


@pytest.fixture(scope='module')
def obj():
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  mesh = S.make_mustard_mesh(seed=0)
  mesh.vertices = mesh.vertices - (mesh.vertices.min(0) + mesh.vertices.max(0)) / 2
  mt = make_mesh_tensors(mesh)
  pts = np.asarray(mesh.vertices)
  diam = float(np.linalg.norm(pts[None] - pts[:, None], axis=-1).max())
  return dict(mesh=mesh, mt=mt, diameter=diam)


def render_depth(obj, poses, K, H, W):
  from foundationpose_amd import Utils as U
  _, d, _ = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=torch.as_tensor(np.asarray(poses, dtype=np.float32)).reshape(-1, 4, 4).cuda(),
                                mesh_tensors=obj['mt'])
  return d.cpu().numpy()


def make_frame(obj, K, H, W, gt_pose, seed):
  from foundationpose_amd import synthetic as S

  def rf(K_, H_, W_, pose):
    return np.zeros((H_, W_, 3), np.float32), render_depth(obj, pose, K_, H_, W_)[0]
  return S.make_scene(rf, obj['mt'], seed=seed, H=H, W=W, K=K, gt_pose=gt_pose)


@pytest.fixture(scope='module')
def vga(obj):
  from foundationpose_amd import synthetic as S
  K = S.YCB_K
  sc = make_frame(obj, K, 480, 640, None, seed=0)
  gt = sc['gt_pose']
  hyp = around(gt, 64, seed=3)
  hyp[5, :3, 3] += [0.2, 0.0, 0.0]                                   # one pose off to the side: no overlap
  return dict(K=K, depth=sc['depth'], gt=gt, hyp=hyp)


def check_counts(obj, got_e, got_c, depths, dg, de, K, taus, delta=0.015):
  got_e, got_c = got_e.cpu().numpy(), got_c.cpu().numpy()
  assert got_c.dtype == np.int32 and got_c.shape == (len(de), 2 + len(taus)) and got_e.shape == (len(de), len(taus))
  for b in range(len(de)):
    c, e = ref_vsd(depths[b], dg[b], de[b], K, obj['diameter'], delta, taus)
    assert np.array_equal(got_c[b], c), (b, got_c[b], c)
    assert np.array_equal(got_e[b], e.astype(np.float32)), (b, got_e[b], e)


def test_vsd_counts_exact(obj, vga):
  from foundationpose_amd import Utils as U
  v = vga
  taus = U.BOP19_VSD_TAUS
  e, c = U.vsd_errors(v['hyp'], v['gt'], v['depth'], v['K'], mesh_tensors=obj['mt'], diameter=obj['diameter'], return_counts=True)
  de = render_depth(obj, v['hyp'], v['K'], 480, 640)
  dg = render_depth(obj, v['gt'], v['K'], 480, 640)
  check_counts(obj, e, c, [v['depth']] * 64, [dg[0]] * 64, de, v['K'], taus)
  cn = c.cpu().numpy()
  assert (cn[:, 0] > 1000).all() and (cn[:, 1] > 0).sum() >= 60          # the poses overlap the object: a real test
  assert cn[5, 1] == 0 and (e[5] == 1).all()


def test_vsd_per_pose_trajectory(obj):
  from foundationpose_amd import Utils as U
  from foundationpose_amd import synthetic as S
  K = S.YCB_K
  gts = S.trajectory(10)
  depths = np.stack([make_frame(obj, K, 480, 640, g, seed=20 + f)['depth'] for f, g in enumerate(gts)])
  preds = np.stack([around(g, 1, seed=40 + f)[0] for f, g in enumerate(gts)])
  taus = np.array([0.3, 0.05, 0.2])                                  # any order
  e, c = U.vsd_errors(torch.as_tensor(preds).cuda(), torch.as_tensor(gts).cuda(), torch.as_tensor(depths).cuda(), K, mesh_tensors=obj['mt'],
                      diameter=obj['diameter'], taus=taus, return_counts=True)
  check_counts(obj, e, c, depths, render_depth(obj, gts, K, 480, 640), render_depth(obj, preds, K, 480, 640), K, taus)
  # frame f alone against its own frame and ground truth: the same bits
  f = 6
  alone = U.vsd_errors(preds[f:f + 1], gts[f], depths[f], K, mesh_tensors=obj['mt'], diameter=obj['diameter'], taus=taus)
  assert np.array_equal(alone.cpu().numpy()[0], e.cpu().numpy()[f])


def test_vsd_full_hd(obj):
  """1920x1200: vertices beyond 1024 px from the origin take the rasteriser's second face list, and the frame needs more strips."""
  from foundationpose_amd import Utils as U
  K = FULL_HD_K
  gt = np.eye(4)
  gt[:3, :3] = rot([0.4, 1.1, -0.3])
  gt[:3, 3] = [0.11, 0.04, 0.8]
  sc = make_frame(obj, K, 1200, 1920, gt, seed=5)
  hyp = around(sc['gt_pose'], 4, seed=9)
  taus = U.BOP19_VSD_TAUS
  e, c = U.vsd_errors(hyp, sc['gt_pose'], sc['depth'], K, mesh_tensors=obj['mt'], diameter=obj['diameter'], return_counts=True)
  de = render_depth(obj, hyp, K, 1200, 1920)
  dg = render_depth(obj, sc['gt_pose'], K, 1200, 1920)
  assert (de > 0).any(axis=(0, 1))[1040:].any()                      # the object reaches past column 1024
  check_counts(obj, e, c, [sc['depth']] * 4, [dg[0]] * 4, de, K, taus)
  assert (c.cpu().numpy()[:, 1] > 0).all()


def render_depth_batched(obj, poses, K, H, W, batch=16):
  return np.concatenate([render_depth(obj, poses[i:i + batch], K, H, W) for i in range(0, len(poses), batch)])


def noisy_frames(dg, seed):
  """depth frames from ground-truth renders: a background plane at 1.2 m, 1 mm noise, 2 % dropout (as synthetic.make_scene)"""
  rs = np.random.RandomState(seed)
  d = np.where(dg > 0, dg, 1.2).astype(np.float32) + (rs.randn(*dg.shape) * 0.001).astype(np.float32)
  d[rs.uniform(size=dg.shape) < 0.02] = 0
  return d


@pytest.mark.parametrize('per_pose', [False, True])
def test_vsd_several_render_chunks(obj, per_pose):
  """More poses than one render chunk holds at 1920x1200: the per-chunk offsets into the depth frames, the ground truth and the
  counts, the smaller last chunk and the reuse of the chunk buffers.  Shared: 60 poses in chunks of 58 + 2; per pose (depth frame
  and ground truth of a trajectory): 31 poses in chunks of 29 + 2."""
  from foundationpose_amd import Utils as U
  from foundationpose_amd import synthetic as S
  H, W, K = 1200, 1920, FULL_HD_K
  B = 31 if per_pose else 60
  chunk = VSD_DEPTH_BUDGET // (H * W * 4 * (2 if per_pose else 1))
  assert chunk < B < 2 * chunk and B % chunk > 1
  taus = U.BOP19_VSD_TAUS
  if per_pose:
    gts = S.trajectory(B, seed=3)
    preds = np.stack([around(g, 1, seed=60 + f)[0] for f, g in enumerate(gts)])
    dg = render_depth_batched(obj, gts, K, H, W)
    depths = noisy_frames(dg, seed=8)
    e, c = U.vsd_errors(preds, gts, depths, K, mesh_tensors=obj['mt'], diameter=obj['diameter'], taus=taus, return_counts=True)
  else:
    gt = S.trajectory(1, seed=4)[0]
    preds = around(gt, B, seed=12)
    dg0 = render_depth(obj, gt, K, H, W)
    d0 = noisy_frames(dg0, seed=9)[0]
    dg, depths = [dg0[0]] * B, [d0] * B
    e, c = U.vsd_errors(preds, gt, d0, K, mesh_tensors=obj['mt'], diameter=obj['diameter'], taus=taus, return_counts=True)
  check_counts(obj, e, c, depths, dg, render_depth_batched(obj, preds, K, H, W), K, taus)
  assert (c.cpu().numpy()[:, 1] > 0).all()


def test_full_hd_render_matches_oracle(obj):
  """The 1920x1200 full frame beside the 8k-vertex mesh needs more than 255 strips with the vertex records in LDS, so render_plan keeps
  them in global memory.  Which pixels are covered and which face wins each is integer work on both sides: compared exactly with the
  CPU oracle's rasteriser; the depth is the same fp32 interpolation (2e-6 abs, as the other render parity tests)."""
  from foundationpose_amd import Utils as U
  from oracle.render import nvdiffrast_render as orender
  H, W, K = 1200, 1920, FULL_HD_K
  gt = np.eye(4)
  gt[:3, :3] = rot([0.4, 1.1, -0.3])
  gt[:3, 3] = [0.11, 0.04, 0.8]
  poses = np.stack([gt, around(gt, 1, seed=2)[0]]).astype(np.float32)
  mt_cpu = {k: v.cpu() for k, v in obj['mt'].items()}
  eo, eg = {}, {'rast': None}
  _, do, _ = orender(K=K, H=H, W=W, ob_in_cams=poses, mesh_tensors=mt_cpu, extra=eo)
  _, dg, _ = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=torch.from_numpy(poses).cuda(), mesh_tensors=obj['mt'], extra=eg)
  id_o, id_g = eo['rast'][..., 3].numpy().astype(np.int64), eg['rast'][..., 3].cpu().numpy().astype(np.int64)
  assert (id_o > 0).sum(axis=(1, 2)).min() > 10000 and (id_o[:, :, 1025:] > 0).any()
  assert np.array_equal(id_o > 0, id_g > 0) and np.array_equal(id_o, id_g)
  frac, mx, _ = util.mismatch_report(do.numpy(), dg.cpu().numpy(), 2e-6)
  assert frac <= 2e-4, f'depth: {frac:.2e} of values differ by > 2e-6 (max {mx:.2e})'


def test_vsd_analytic(obj, vga):
  from foundationpose_amd import Utils as U
  v, K, mt, diam = vga, vga['K'], obj['mt'], obj['diameter']
  taus = U.BOP19_VSD_TAUS
  dg = render_depth(obj, v['gt'], K, 480, 640)[0]
  # pred = gt against its own render: every pixel visible and no cost
  e, c = U.vsd_errors(np.stack([v['gt']] * 3), v['gt'], dg, K, mesh_tensors=mt, diameter=diam, return_counts=True)
  assert (e.cpu().numpy() == 0).all() and (c.cpu().numpy()[:, 0] == (dg > 0).sum()).all()
  # no overlap
  far = v['gt'].copy()
  far[:3, 3] += [0.2, 0.0, 0.0]
  e = U.vsd_errors(far[None], v['gt'], v['depth'], K, mesh_tensors=mt, diameter=diam)
  assert (e.cpu().numpy() == 1).all()
  # a wall at 0.3 m in front of both poses: nothing is visible, the union is empty
  wall = np.full((480, 640), 0.3, np.float32)
  e, c = U.vsd_errors(v['hyp'][:8], v['gt'], wall, K, mesh_tensors=mt, diameter=diam, return_counts=True)
  assert (e.cpu().numpy() == 1).all() and (c.cpu().numpy() == 0).all()
  # no depth at all: silhouettes only
  zero = np.zeros((480, 640), np.float32)
  e, c = U.vsd_errors(v['hyp'][:16], v['gt'], zero, K, mesh_tensors=mt, diameter=diam, return_counts=True)
  de = render_depth(obj, v['hyp'][:16], K, 480, 640)
  Dg = ref_dist(dg, K)
  for b in range(16):
    De = ref_dist(de[b], K)
    both, either = (Dg > 0) & (De > 0), (Dg > 0) | (De > 0)
    d = np.abs(Dg - De)[both] / diam
    want = np.array([((d >= t).sum() + either.sum() - both.sum()) / either.sum() for t in taus])
    assert np.array_equal(e.cpu().numpy()[b], want.astype(np.float32)), b
    assert c.cpu().numpy()[b, 0] == either.sum() and c.cpu().numpy()[b, 1] == both.sum()
  # e is non-increasing in tau
  e = U.vsd_errors(v['hyp'], v['gt'], v['depth'], K, mesh_tensors=mt, diameter=diam, taus=np.linspace(0.01, 1.0, 32)).cpu().numpy()
  assert (np.diff(e, axis=1) <= 0).all() and (e[:, 0] > e[:, -1]).any()


def test_bit_identity(obj, vga, mustard):
  from foundationpose_amd import Utils as U
  m, v = mustard, vga
  sym = sym_z73()
  full = U.bop_pose_errors(m['hyp'], m['gt'], m['pts'], K=m['K'], symmetry_tfs=sym)
  for b in (0, 200):
    alone = U.bop_pose_errors(m['hyp'][b:b + 1], m['gt'], m['pts'], K=m['K'], symmetry_tfs=sym)
    for k in ('mssd', 'mspd'):
      assert full[k].cpu().numpy()[b].view(np.int32) == alone[k].cpu().numpy()[0].view(np.int32), (k, b)
  target = v['hyp'][7]
  batch = around(v['gt'], 201, seed=11)
  batch[0] = target
  batch[200] = target
  kw = dict(mesh_tensors=obj['mt'], diameter=obj['diameter'])
  e_batch = U.vsd_errors(batch, v['gt'], v['depth'], v['K'], **kw).cpu().numpy()
  e_alone = U.vsd_errors(target[None], v['gt'], v['depth'], v['K'], **kw).cpu().numpy()
  assert np.array_equal(e_batch[0], e_alone[0]) and np.array_equal(e_batch[200], e_alone[0])


def test_diameter_from_mesh(obj, vga):
  from foundationpose_amd import Utils as U
  v = vga
  np.random.seed(0)
  e = U.vsd_errors(v['hyp'][:4], v['gt'], v['depth'], v['K'], mesh=obj['mesh'])
  np.random.seed(0)
  d = U.compute_mesh_diameter(model_pts=obj['mesh'].vertices, n_sample=10000)
  want = U.vsd_errors(v['hyp'][:4], v['gt'], v['depth'], v['K'], mesh_tensors=obj['mt'], diameter=d)
  assert torch.equal(e, want)


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_invalid_arguments_bop(mustard):
  from foundationpose_amd import Utils as U
  from foundationpose_amd import _lib
  from foundationpose_amd._lib import FP_EINVAL, k_ptr, lib, ptr, stream_ptr
  ctx = _lib.Context.get('cuda:0')
  dev = torch.device('cuda', 0)
  pts = torch.ones((10, 3), device=dev)
  pose = torch.eye(4, device=dev)[None].contiguous()
  pose[0, 2, 3] = 1.0
  sym = torch.eye(4, device=dev)[None].contiguous()
  o1, o2 = torch.empty(1, device=dev), torch.empty(1, device=dev)
  Kd, Kp = k_ptr(np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]))
  M, P = _lib.FP_BOP_MSSD, _lib.FP_BOP_MSPD
  good = dict(ctx=ctx.handle, pts=pts, n=10, pred=pose, gt=pose, per=0, B=1, sym=sym, S=1, K=Kp, which=M | P, mssd=o1, mspd=o2)

  def call(**kw):
    a = dict(good, **kw)
    rc = lib().fp_pose_errors_bop(a['ctx'], ptr(a['pts']), a['n'], ptr(a['pred']), ptr(a['gt']), a['per'], a['B'], ptr(a['sym']), a['S'],
                                  a['K'], a['which'], ptr(a['mssd']), ptr(a['mspd']), stream_ptr(dev))
    torch.cuda.synchronize()
    return rc

  assert call() == 0
  for bad in (dict(ctx=None), dict(pts=None), dict(pred=None), dict(gt=None), dict(n=0), dict(n=-1), dict(B=-1), dict(S=-1),
              dict(sym=None), dict(per=2), dict(per=-1), dict(which=4), dict(which=M | 8), dict(mssd=None), dict(mspd=None), dict(K=None)):
    assert call(**bad) == FP_EINVAL, bad
  assert call(B=0) == 0 and call(which=0) == 0                          # nothing to do
  assert call(sym=None, S=0) == 0                                       # the identity only
  assert call(which=M, mspd=None, K=None) == 0 and call(which=P, mssd=None) == 0      # outputs not requested may be null
  with pytest.raises(ValueError):
    U.bop_pose_errors(np.eye(4)[None], np.eye(4), np.zeros((5, 3), np.float32), metrics=('vsd',))
  with pytest.raises(ValueError):
    U.bop_pose_errors(np.eye(4)[None], np.eye(4), np.zeros((5, 3), np.float32))           # mspd without K
  with pytest.raises(_lib.FoundationPoseAmdError):
    U.bop_pose_errors(np.eye(4)[None], np.eye(4), np.zeros((0, 3), np.float32), metrics=('mssd',))


def test_invalid_arguments_vsd(obj, vga):
  from foundationpose_amd import Utils as U
  from foundationpose_amd import _lib
  from foundationpose_amd._lib import FP_EINVAL, k_ptr, lib, ptr, stream_ptr
  ctx = _lib.Context.get('cuda:0')
  dev = torch.device('cuda', 0)
  dm = _lib.device_mesh(ctx, obj['mt'])
  H, W = 48, 64
  depth = torch.zeros((H, W), device=dev)
  pose = torch.as_tensor(vga['gt'], device=dev)[None].contiguous()
  Kd, Kp = k_ptr(np.array([[100.0, 0, 32], [0, 100, 24], [0, 0, 1]]))
  taus = np.array([0.1, 0.2])
  err = torch.empty((1, 2), device=dev)
  cnt = torch.empty((1, 4), dtype=torch.int32, device=dev)
  good = dict(ctx=ctx.handle, mesh=dm.handle, depth=depth, dpp=0, H=H, W=W, K=Kp, pred=pose, gt=pose, gpp=0, B=1, diam=0.2, delta=0.015,
              taus=taus, T=2, err=err, cnt=cnt)

  def call(**kw):
    a = dict(good, **kw)
    rc = lib().fp_vsd(a['ctx'], a['mesh'], ptr(a['depth']), a['dpp'], a['H'], a['W'], a['K'], ptr(a['pred']), ptr(a['gt']), a['gpp'], a['B'],
                      a['diam'], a['delta'], ptr(a['taus']), a['T'], ptr(a['err']), ptr(a['cnt']), stream_ptr(dev))
    torch.cuda.synchronize()
    return rc

  assert call() == 0 and call(cnt=None) == 0
  assert call(B=0) == 0                                                 # a no-op
  for bad in (dict(ctx=None), dict(mesh=None), dict(depth=None), dict(K=None), dict(pred=None), dict(gt=None), dict(taus=None),
              dict(err=None), dict(T=0), dict(T=33), dict(T=-1), dict(H=0), dict(W=0), dict(H=-5), dict(diam=0.0), dict(diam=-0.1),
              dict(diam=float('nan')), dict(dpp=2), dict(dpp=-1), dict(gpp=2), dict(B=-1)):
    assert call(**bad) == FP_EINVAL, bad
  with pytest.raises(ValueError):
    U.vsd_errors(np.stack([vga['gt']] * 3), vga['gt'], np.zeros((2, H, W), np.float32), Kd, mesh_tensors=obj['mt'], diameter=0.2)
  with pytest.raises(_lib.FoundationPoseAmdError):
    U.vsd_errors(vga['gt'][None], vga['gt'], np.zeros((H, W), np.float32), Kd, mesh_tensors=obj['mt'], diameter=0.2, taus=np.zeros(33))
