"""GPU: masks, visible masks, the z-buffer composite and BOP's gt_info of the object instances of a frame from their poses
(Utils.scene_instances, fp_scene_instances).

Every comparison is exact.  The expected values are restated here in numpy float64 from the library's own per-instance depth renders
(Utils.nvdiffrast_render on the same padded canvas with K'), the way tests/test_gpu_bop_metrics.py restates VSD; the kernel shares no
code with the restatement.  No pixel and no instance is left out."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu
H, W = 480, 640
FULL_HD_K = np.array([[1600.0, 0, 955.5], [0, 1600.0, 603.2], [0, 0, 1]])
DELTA = 0.015
OCC = {'depth': 1, 'instances': 2, 'both': 3}


def _pose(t, rot_seed=None, R=None):
  from foundationpose_amd import synthetic as S
  p = np.eye(4, dtype=np.float32)
  p[:3, :3] = S.random_rotation(np.random.RandomState(rot_seed)) if R is None else R
  p[:3, 3] = t
  return p


def _centred(mesh):
  mesh.vertices = mesh.vertices - (mesh.vertices.min(0) + mesh.vertices.max(0)) / 2
  return mesh


def pads(pad, h, w):
  return (w, h) if pad == 'bop' else ((pad, pad) if isinstance(pad, int) else tuple(pad))


def canvas_K(K, pad_x, pad_y):
  Kc = np.array(K, dtype=np.float64)
  Kc[0, 2] = Kc[0, 2] + float(pad_x)
  Kc[1, 2] = Kc[1, 2] + float(pad_y)
  return Kc


def render_layers(mts, poses, K, h, w, pad_x, pad_y):
  """(n, h + 2 pad_y, w + 2 pad_x) float32: every instance alone on the padded canvas, by the library's public render"""
  from foundationpose_amd import Utils as U
  Kc = canvas_K(K, pad_x, pad_y)
  out = []
  for mt, p in zip(mts, poses):
    _, d, _ = U.nvdiffrast_render(K=Kc, H=h + 2 * pad_y, W=w + 2 * pad_x, ob_in_cams=torch.as_tensor(p, device='cuda').reshape(1, 4, 4), mesh_tensors=mt)
    out.append(d[0].cpu().numpy())
  return np.stack(out)


def ref_dist(d, K):
  """bop_toolkit misc.depth_im_to_dist_im_fast, float64"""
  d = np.asarray(d, dtype=np.float64)
  h, w = d.shape
  xs, ys = np.meshgrid(np.arange(w), np.arange(h))
  X = ((xs - K[0, 2]) * d) * (1.0 / K[0, 0])
  Y = ((ys - K[1, 2]) * d) * (1.0 / K[1, 1])
  return np.sqrt(X * X + Y * Y + d * d)


def _box(m, pad_x, pad_y):
  if not m.any():
    return [-1, -1, -1, -1]
  r, c = np.nonzero(m)
  return [int(c.min()) - pad_x, int(r.min()) - pad_y, int(c.max()) - pad_x, int(r.max()) - pad_y]


def ref_scene(layers, depth, K, h, w, pad_x, pad_y, occ, delta=DELTA):
  """The contract of fp_scene_instances in numpy float64, instance by instance: dict(mask, mask_visib (n,h,w) bool, rows (n,12) int,
  Dt_zero_under_mask: does a pixel without depth lie under a mask)."""
  n = len(layers)
  Kc = canvas_K(K, pad_x, pad_y)
  hc, wc = h + 2 * pad_y, w + 2 * pad_x
  frame = np.zeros((hc, wc), dtype=bool)
  frame[pad_y:pad_y + h, pad_x:pad_x + w] = True
  dt = np.zeros((hc, wc), dtype=np.float32)
  if depth is not None:
    dt[pad_y:pad_y + h, pad_x:pad_x + w] = depth
  Dt = ref_dist(dt, Kc) if occ & 1 else np.zeros((hc, wc))
  Docc = Dt
  if occ & 2:
    Dmin = np.full((hc, wc), np.inf)
    for l in layers:
      Dm = ref_dist(l, Kc)
      Dmin = np.where((Dm > 0) & (Dm < Dmin), Dm, Dmin)
    Dmin[np.isinf(Dmin)] = 0
    Docc = np.where((Dt > 0) & (Dmin > 0), np.minimum(Dt, Dmin), np.where(Dt > 0, Dt, Dmin)) if occ & 1 else Dmin
  focc = Docc.astype(np.float32)
  masks, visibs, rows, holes = [], [], [], False
  for l in layers:
    Dm = ref_dist(l, Kc)
    m = Dm > 0
    vis = m & (((Dm.astype(np.float32) - focc).astype(np.float64) <= delta) | (Docc == 0)) & frame
    holes |= bool((m & frame & (dt == 0)).any())
    rows.append([int(m.sum()), int((m & frame & (dt > 0)).sum()), int(vis.sum()), int((m & frame).sum())] + _box(m, pad_x, pad_y) + _box(vis, pad_x, pad_y))
    masks.append(m[pad_y:pad_y + h, pad_x:pad_x + w])
    visibs.append(vis[pad_y:pad_y + h, pad_x:pad_x + w])
  return dict(mask=np.stack(masks), mask_visib=np.stack(visibs), rows=np.array(rows, dtype=np.int64).reshape(n, 12), holes=holes)


def ref_composite(layers_frame):
  """owner / depth as the loop of tests/test_gpu_bop_run.py::_frame composes them: the first index wins a tie"""
  d_all = torch.as_tensor(layers_frame, device='cuda')
  depth = torch.full(d_all.shape[1:], float('inf'), device='cuda')
  owner = torch.full(d_all.shape[1:], -1, device='cuda', dtype=torch.int32)
  for o, d in enumerate(d_all):
    near = (d > 0) & (d < depth)
    depth = torch.where(near, d, depth)
    owner = torch.where(near, torch.full_like(owner, o), owner)
  depth = torch.where(owner >= 0, depth, torch.zeros_like(depth))
  return owner.cpu().numpy(), depth.cpu().numpy()


def run(K, h, w, mts, poses, depth, occ, pad, **kw):
  from foundationpose_amd import Utils as U
  out = U.scene_instances(K, h, w, mts, poses, depth=depth, occluders=occ, delta=DELTA, pad=pad, **kw)
  torch.cuda.synchronize()
  return out


def check(out, ref, what):
  from foundationpose_amd import Utils as U
  # every int32 column through the host conversion that tests/test_scene_info_host.py pins: equal dicts = equal rows (an empty set has
  # count 0 and a box of four -1 on both sides)
  assert out['info'] == U.scene_info_rows(ref['rows']), (what, out['info'], ref['rows'])
  m, v = out['mask'].cpu().numpy(), out['mask_visib'].cpu().numpy()
  assert m.dtype == np.uint8 and set(np.unique(m)) <= {0, 255} and set(np.unique(v)) <= {0, 255}
  assert np.array_equal(m > 0, ref['mask']), (what, int(((m > 0) != ref['mask']).sum()))
  assert np.array_equal(v > 0, ref['mask_visib']), (what, int(((v > 0) != ref['mask_visib']).sum()))
  assert (v > 0).reshape(len(v), -1).sum(1).tolist() == [e['px_count_visib'] for e in out['info']]      # == count(mask_visib), always


@pytest.fixture(scope='module')
def world():
  """Six instances of two models at 640 x 480 over a make_scene frame (object 0 in it, plane at 1.2 m, 2 % holes): 0 the frame's object;
  1 partly behind it; 2 behind the plane (seen through its holes only); 3 behind 0 and inside its silhouette; 4 cut by the left border;
  5 right of the frame, on the 'bop' canvas only."""
  from foundationpose_amd import synthetic as S
  from foundationpose_amd import Utils as U
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  A = make_mesh_tensors(_centred(S.make_mustard_mesh(seed=0)))
  B = make_mesh_tensors(_centred(S.make_mustard_mesh(seed=1, n_theta=80, n_z=70)))

  def rf(K_, H_, W_, pose):
    _, d, _ = U.nvdiffrast_render(K=K_, H=H_, W=W_, ob_in_cams=torch.as_tensor(pose, device='cuda').reshape(-1, 4, 4), mesh_tensors=A)
    return np.zeros((H_, W_, 3), np.float32), d[0].cpu().numpy()
  sc = S.make_scene(rf, A, seed=0)
  gt = sc['gt_pose']
  t0 = gt[:3, 3]
  poses = [gt, _pose((t0[0] + 0.05, t0[1], 0.95), rot_seed=3), _pose((-0.25, -0.25, 1.5), rot_seed=4), _pose(t0 * (1.05 / 0.75), R=gt[:3, :3]),
           _pose((-0.2, 0.08, 0.7), rot_seed=5), _pose((0.6, 0.0, 0.7), rot_seed=6)]
  return dict(K=S.YCB_K, depth=sc['depth'], mts=[A, B, A, A, B, B], poses=np.stack(poses).astype(np.float32), A=A, B=B)


@pytest.mark.parametrize('pad', [0, 'bop'])
@pytest.mark.parametrize('occ', ['depth', 'instances', 'both'])
def test_masks_and_info_exact(world, occ, pad):
  from foundationpose_amd import Utils as U
  w = world
  pad_x, pad_y = pads(pad, H, W)
  layers = render_layers(w['mts'], w['poses'], w['K'], H, W, pad_x, pad_y)
  ref = ref_scene(layers, w['depth'], w['K'], H, W, pad_x, pad_y, OCC[occ])
  names = {'depth': 'depth', 'instances': 'instances', 'both': ('depth', 'instances')}[occ]
  out = run(w['K'], H, W, w['mts'], w['poses'], w['depth'], names, pad)
  print('info', occ, pad, out['info'])
  check(out, ref, (occ, pad))
  # the cases the scene was built for really occur in the restatement
  r = ref['rows']
  assert ref['holes'], 'no pixel without depth under a mask'
  assert r[0, 0] > 5000 and r[0, 0] == r[0, 3]                                         # the frame's own object, wholly inside
  assert 0 < r[1, 2] < r[1, 3], 'instance 1 is not partly hidden'
  assert r[5, 3] == 0 and list(r[5, 8:]) == [-1] * 4, 'instance 5 is not wholly outside the frame'
  if pad == 'bop':
    assert r[4, 0] > r[4, 3] > 0 and r[4, 4] < 0, 'instance 4 is not cut by the left border'
    assert r[5, 0] > 0 and r[5, 4] > W - 1
  else:
    assert r[4, 0] == r[4, 3] and r[4, 4] == 0
    assert r[5, 0] == 0 and list(r[5, 4:8]) == [-1] * 4
  if occ == 'depth':
    assert 0 < r[2, 2] < 0.05 * r[2, 3], 'instance 2 should show through the holes of the plane only'
    assert r[0, 2] == r[0, 3]                                                            # what the depth image shows is visible
  if occ in ('instances', 'both'):
    assert r[3, 0] > 1000 and r[3, 2] == 0 and list(r[3, 8:]) == [-1] * 4, 'instance 3 is not wholly hidden behind instance 0'
  if occ == 'instances':
    assert r[2, 2] == r[2, 3] > 0                                                        # nothing but instances occludes: the plane does not
  # the dicts of the public call
  info = U.scene_info_rows(r)
  assert out['info'] == info and info[3]['visib_fract'] == (0.0 if occ != 'depth' else info[3]['visib_fract'])
  assert info[0]['bbox_obj'][2] == r[0, 6] - r[0, 4] + 1


@pytest.mark.parametrize('pad', [0, (8, 4), (3, 5)])
def test_owner_and_depth_equal_the_composite_loop(world, pad):
  """(pad (3, 5) and the odd frame below take the one-pixel-per-lane form of the kernel)"""
  from foundationpose_amd import Utils as U
  w = world
  pad_x, pad_y = pads(pad, H, W)
  layers = render_layers(w['mts'], w['poses'], w['K'], H, W, pad_x, pad_y)
  owner, depth = ref_composite(layers[:, pad_y:pad_y + H, pad_x:pad_x + W])
  out = run(w['K'], H, W, w['mts'], w['poses'], w['depth'], 'both', pad)
  assert out['owner'].dtype == torch.int32 and np.array_equal(out['owner'].cpu().numpy(), owner)
  assert np.array_equal(out['depth'].cpu().numpy(), depth)
  assert set(np.unique(owner)) >= {-1, 0, 1, 4}
  check(out, ref_scene(layers, w['depth'], w['K'], H, W, pad_x, pad_y, 3), pad)


def test_odd_frame_size(world):
  w = world
  h, ww = 241, 323
  depth = np.ascontiguousarray(w['depth'][:h, :ww])
  for pad in (0, (2, 1)):
    pad_x, pad_y = (pad, pad) if isinstance(pad, int) else pad
    layers = render_layers(w['mts'], w['poses'], w['K'], h, ww, pad_x, pad_y)
    out = run(w['K'], h, ww, w['mts'], w['poses'], depth, 'both', pad)
    check(out, ref_scene(layers, depth, w['K'], h, ww, pad_x, pad_y, 3), pad)
    owner, comp = ref_composite(layers[:, pad_y:pad_y + h, pad_x:pad_x + ww])
    assert np.array_equal(out['owner'].cpu().numpy(), owner) and np.array_equal(out['depth'].cpu().numpy(), comp)


def test_two_instances_at_one_pose(world):
  w = world
  poses = np.stack([w['poses'][0], w['poses'][0]])
  out = run(w['K'], H, W, w['A'], poses, None, 'instances', 0)
  owner, m, v = out['owner'].cpu().numpy(), out['mask'].cpu().numpy() > 0, out['mask_visib'].cpu().numpy() > 0
  assert m[0].sum() > 5000 and np.array_equal(m[0], m[1])
  assert np.array_equal(owner >= 0, m[0]) and (owner[m[0]] == 0).all()                  # the smaller index owns every pixel
  assert np.array_equal(v[0], m[0]) and np.array_equal(v[1], m[1])                      # both visible masks are full
  assert [r['visib_fract'] for r in out['info']] == [1.0, 1.0]


def test_more_instances_than_one_chunk(world):
  """60 instances at 1920 x 1200: 58 depth layers fit the 512 MB of a chunk.  With the instances as occluders the minimum runs over both
  chunks (a second pass); without them every row equals the instance run alone."""
  from foundationpose_amd import _lib, synthetic as S
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  h, ww, K = 1200, 1920, FULL_HD_K
  n = 60
  chunk = _lib.SCENE_DEPTH_BUDGET // (h * ww * 4)
  assert chunk < n < 2 * chunk
  small = make_mesh_tensors(_centred(S.make_mustard_mesh(seed=2, n_theta=24, n_z=20)))
  poses = np.stack([_pose((-0.45 + 0.1 * (i % 10), min(-0.25 + 0.1 * (i // 10), 0.2), 1.0 + 0.03 * ((i + i // 10) % 5)), rot_seed=100 + i) for i in range(n)])
  rs = np.random.RandomState(5)
  depth = np.full((h, ww), 1.08, dtype=np.float32) + (rs.randn(h, ww) * 0.001).astype(np.float32)
  depth[rs.uniform(size=(h, ww)) < 0.02] = 0
  layers = render_layers([small] * n, poses, K, h, ww, 0, 0)
  for occ in ('instances', 'both'):
    ref = ref_scene(layers, depth, K, h, ww, 0, 0, OCC[occ])
    out = run(K, h, ww, small, poses, depth, {'instances': 'instances', 'both': ('depth', 'instances')}[occ], 0)
    check(out, ref, occ)
    owner, comp = ref_composite(layers)
    assert np.array_equal(out['owner'].cpu().numpy(), owner) and np.array_equal(out['depth'].cpu().numpy(), comp)
    hidden = ref['rows'][:, 2] < ref['rows'][:, 3]
    assert hidden[chunk:].any() and hidden[:chunk].any(), 'no occlusion across the chunk boundary'
    del out
  out = run(K, h, ww, small, poses, depth, 'depth', 0)
  check(out, ref_scene(layers, depth, K, h, ww, 0, 0, 1), 'depth')
  info, v = out['info'], out['mask_visib']
  for i in range(n):
    alone = run(K, h, ww, small, poses[i:i + 1], depth, 'depth', 0, want=('mask_visib', 'info'))
    assert alone['info'][0] == info[i], i
    assert torch.equal(alone['mask_visib'][0], v[i]), i
  # every output alone over two chunks, with the instances as occluders (the default) and with the depth image alone: what is not asked
  # for is not there, in the call's workspace either (a running minimum nobody reads)
  for occ in (None, 'depth'):
    full = run(K, h, ww, small, poses, depth, occ, 0)
    for k in ('mask', 'mask_visib', 'owner', 'depth', 'info'):
      one = run(K, h, ww, small, poses, depth, occ, 0, want=(k,))
      assert set(one) == {k}
      assert one[k] == full[k] if k == 'info' else torch.equal(one[k], full[k]), (occ, k)
      del one
    assert np.array_equal(full['mask'].cpu().numpy() > 0, layers > 0)
    del full


def test_bit_identity_optional_outputs_and_no_instances(world):
  from foundationpose_amd import Utils as U
  w = world
  a = run(w['K'], H, W, w['mts'], w['poses'], w['depth'], None, 'bop')
  b = run(w['K'], H, W, w['mts'], w['poses'], w['depth'], None, 'bop')
  for k in ('mask', 'mask_visib', 'owner', 'depth'):
    assert torch.equal(a[k], b[k]), k
  assert a['info'] == b['info']
  for k in ('mask', 'mask_visib', 'owner', 'depth', 'info'):
    one = run(w['K'], H, W, w['mts'], w['poses'], w['depth'], None, 'bop', want=(k,))
    assert set(one) == {k}
    assert one[k] == a[k] if k == 'info' else torch.equal(one[k], a[k]), k
  none = U.scene_instances(w['K'], H, W, [], np.zeros((0, 4, 4), np.float32), depth=w['depth'])
  torch.cuda.synchronize()
  assert none['mask'].shape == (0, H, W) and none['info'] == []
  assert (none['owner'] == -1).all() and (none['depth'] == 0).all()


def test_invalid_arguments_leave_the_arena_alone(world):
  from foundationpose_amd import _lib
  from foundationpose_amd._lib import lib, ptr, stream_ptr
  w = world
  before = run(w['K'], H, W, w['mts'], w['poses'], w['depth'], None, 4)
  ctx = _lib.Context.get()
  dm = [_lib.device_mesh(ctx, m) for m in w['mts']]
  handles = (ctypes.c_void_p * 6)(*[m.handle for m in dm])
  P = torch.as_tensor(w['poses'], device='cuda').contiguous()
  D = torch.as_tensor(w['depth'], device='cuda').contiguous()
  Kd, Kp = _lib.k_ptr(w['K'])
  rows = torch.empty((6, _lib.FP_SCENE_INFO_COLS), dtype=torch.int32, device='cuda')

  def call(**kw):
    a = dict(ctx=ctx.handle, meshes=handles, poses=ptr(P), n=6, K=Kp, H=H, W=W, pad_x=0, pad_y=0, depth=ptr(D), occ=3, delta=DELTA)
    a.update(kw)
    rc = lib().fp_scene_instances(a['ctx'], a['meshes'], a['poses'], a['n'], a['K'], a['H'], a['W'], a['pad_x'], a['pad_y'], a['depth'], a['occ'],
                                  a['delta'], None, None, None, None, ptr(rows), stream_ptr())
    return rc, lib().fp_last_error().decode()
  assert call()[0] == 0
  one_null = (ctypes.c_void_p * 6)(*([dm[0].handle] * 5 + [None]))
  bad = [dict(ctx=None), dict(K=None), dict(meshes=None), dict(meshes=one_null), dict(poses=None), dict(n=-1), dict(n=_lib.FP_SCENE_MAX_INSTANCES + 1),
         dict(H=0), dict(W=0), dict(pad_x=-1), dict(pad_y=-1), dict(occ=0), dict(occ=4), dict(occ=7), dict(occ=1, depth=None), dict(occ=3, depth=None),
         dict(delta=-1e-9), dict(delta=float('nan')), dict(pad_x=2960), dict(pad_x=8, pad_y=40000)]
  for kw in bad:
    rc, msg = call(**kw)
    assert rc == _lib.FP_EINVAL, (kw, rc, msg)
    if kw == dict(pad_x=2960):
      assert 'reduce pad_x' in msg, msg
  # a canvas within the width limit that needs more strips than the rasteriser has is refused before anything is queued; the hint
  # about the pad comes with a pad only
  rc, msg = call(H=1200, W=1920, pad_x=1920, pad_y=1200, occ=2, depth=None)
  assert rc == _lib.FP_EINVAL and 'reduce pad' in msg, (rc, msg)
  rc, msg = call(H=3600, W=5760, occ=2, depth=None)
  assert rc == _lib.FP_EINVAL and 'strips' in msg and 'reduce pad' not in msg, (rc, msg)
  after = run(w['K'], H, W, w['mts'], w['poses'], w['depth'], None, 4)
  for k in ('mask', 'mask_visib', 'owner', 'depth'):
    assert torch.equal(before[k], after[k]), k
  assert before['info'] == after['info']
  from foundationpose_amd import Utils as U
  for kw, msg in ((dict(want=('masks',)), 'unknown output'), (dict(occluders='plane'), 'unknown occluder'), (dict(pad='bob'), 'pad must be')):
    with pytest.raises(ValueError, match=msg):
      U.scene_instances(w['K'], H, W, w['mts'], w['poses'], depth=w['depth'], **kw)
  with pytest.raises(ValueError, match='meshes for'):
    U.scene_instances(w['K'], H, W, w['mts'][:4], w['poses'], depth=w['depth'])


def test_tracker_instance_masks():
  """MultiObjectTracker.instance_masks() after register equals Utils.scene_instances by hand on the estimators' poses; before it, it
  raises."""
  from foundationpose_amd import Utils as U
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.tracking import MultiObjectTracker
  from tests.test_gpu_register_objects import GT, SCORE_GAIN, _estimator, _frame, _instance
  from tests.test_gpu_register_objects import _pose as reg_pose
  from foundationpose_amd.config import REFINE_DEFAULT, SCORE_DEFAULT
  from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
  from foundationpose_amd.predict_score import ScorePredictor
  refiner = PoseRefinePredictor(state_dict=S.make_refine_state_dict(cases.REFINE_SEED, head_gain=cases.GAIN_CHAIN), cfg=REFINE_DEFAULT)
  ssd = S.make_score_state_dict(cases.SCORE_SEED)
  ssd['linear.weight'] = ssd['linear.weight'] * SCORE_GAIN
  ssd['linear.bias'] = ssd['linear.bias'] * SCORE_GAIN - SCORE_GAIN * 0.0795
  scorer = ScorePredictor(state_dict=ssd, cfg=SCORE_DEFAULT)
  base = [_estimator(S.make_mustard_mesh(seed=0), refiner, scorer), _estimator(S.make_mustard_mesh(seed=1, n_theta=80, n_z=70), refiner, scorer)]
  ests = base + [_instance(base[0])]
  gt = [reg_pose(t, s) for t, s in GT[:3]]
  rgb, depth, owner = _frame(ests, gt)
  tracker = MultiObjectTracker(ests)
  with pytest.raises(ValueError, match='no pose yet'):
    tracker.instance_masks()
  tracker.register(rgb, depth, S.YCB_K, [owner == o for o in range(3)], iteration=1)
  poses = torch.stack([e.pose_last.reshape(4, 4) for e in ests])
  for kw in (dict(), dict(depth=depth)):
    got = tracker.instance_masks(**kw)
    want = U.scene_instances(S.YCB_K, H, W, [e.mesh_tensors for e in ests], poses, want=('mask_visib', 'owner', 'info'), **kw)
    torch.cuda.synchronize()
    assert torch.equal(got['owner'], want['owner']) and torch.equal(got['mask_visib'], want['mask_visib'])
    assert got['mask_visib'].shape == (3, H, W) and got['visib_fract'].shape == (3,)
    assert np.array_equal(got['visib_fract'], np.array([r['visib_fract'] for r in want['info']]))
    assert (got['visib_fract'] > 0).all() and int((got['owner'] >= 0).sum()) > 5000
