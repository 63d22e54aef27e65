"""CPU checks of the observed crop's plain reference (tests/tools/crop_ref.py), so that tests/test_gpu_crop_exact.py is not its own judge:
the reference equals the project's oracle (oracle/warp.py, oracle/geometry.py, oracle/predict.py) on every case, the cases hold what they claim
(ties, borders, thresholds - by count, so a later edit cannot thin them out), the lattice colours make every bilinear sum exact, and two
deliberately wrong references are told apart.

Tolerances: none on the lattice cases.  On the non-lattice case rgb is compared with the float64 sum under crop_ref.bilinear_f64's bound; against
oracle/warp.py:warp_perspective the coordinate term of that bound uses the oracle's OWN deviation from the exact coordinate (its float32 kornia
chain carries several ulps, computed here from its sampling grid, not assumed) plus two ulps for grid_sample's own un-normalisation; the arithmetic
term is unchanged."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests.tools import crop_ref as R


def _oracle(name, mode, normalize_xyz):
  """side B of make_crop_data_batch_refine / _score rebuilt from the oracle's pieces (no renderer)"""
  from oracle import geometry as G
  from oracle.predict import _xyz_transform
  from oracle.warp import warp_perspective, warp_perspective_nearest
  c = R.case(name)
  B, size = len(c['tf']), (c['Ho'], c['Wo'])
  tf, poses = torch.from_numpy(c['tf']), torch.from_numpy(c['poses'])
  rgb = torch.from_numpy(c['rgb'])
  rgbBs = warp_perspective(rgb.permute(2, 0, 1)[None].expand(B, -1, -1, -1), tf, dsize=size, mode='bilinear', align_corners=False) / 255.0
  diam = torch.ones((B,), dtype=torch.float32) * c['diameter']
  if mode == 0:
    xyz = torch.from_numpy(c['xyz'])
    xyzBs = warp_perspective_nearest(xyz.permute(2, 0, 1)[None].expand(B, -1, -1, -1).contiguous(), tf, size)
    xyzBs = _xyz_transform(xyzBs, poses, diam, normalize_xyz, 0.001, False)
  else:
    depth = torch.from_numpy(c['depth'])
    depthBs = warp_perspective_nearest(depth[None, None].expand(B, -1, -1, -1).contiguous(), tf, size)
    Ks = torch.as_tensor(np.asarray(c['K']), dtype=torch.float32).reshape(1, 3, 3).expand(B, 3, 3)
    ori = warp_perspective_nearest(depthBs, torch.linalg.inv(tf), (c['H'], c['W']))
    xyz_full = G.depth2xyzmap_batch(ori[:, 0], Ks, zfar=np.inf).permute(0, 3, 1, 2)
    xyzBs = warp_perspective_nearest(xyz_full, tf, size)
    xyzBs = _xyz_transform(xyzBs, poses, diam, normalize_xyz, 0.1, True)
  return rgbBs.numpy(), xyzBs.numpy()


def _oracle_rgb_coords(c):
  """the pixel coordinates grid_sample derives from the oracle's float32 sampling grid: x (B,Wo), y (B,Ho) as float64 values of float32 numbers"""
  from oracle.warp import warp_grid
  g = warp_grid(torch.from_numpy(c['tf']), (c['H'], c['W']), (c['Ho'], c['Wo']))
  x = ((g[..., 0] + 1) * c['W'] - 1) / 2
  y = ((g[..., 1] + 1) * c['H'] - 1) / 2
  return x[:, 0, :].double().numpy(), y[:, :, 0].double().numpy()


@pytest.mark.parametrize('normalize_xyz', [True, False])
@pytest.mark.parametrize('name,mode', R.RUNS)
def test_reference_equals_the_oracle(name, mode, normalize_xyz):
  c = R.case(name)
  want, _ = R.expected(name, mode, normalize_xyz)
  rgb_o, xyz_o = _oracle(name, mode, normalize_xyz)
  np.testing.assert_array_equal(want[:, 3:], xyz_o)                    # nearest channels, scorer round trip, batch transform: exact
  if name == 'band_probes':
    return                                                              # (its rgb is not what the case is about)
  # rgb.  The oracle's bilinear warp runs kornia's chain in float32, and linspace / the normalisation by (size - 1) round there unless
  # (Ho - 1) and (Wo - 1) are powers of two: where its coordinate IS the exact one the values must be equal bit for bit, and that is every pixel
  # of the power-of-two lattice cases; elsewhere they agree within the derived bound, with the oracle's own deviation as the coordinate term.
  ox, oy = _oracle_rgb_coords(c)
  pow2 = all(v & (v - 1) == 0 for v in (c['Ho'] - 1, c['Wo'] - 1))
  for b in range(len(c['tf'])):
    xs = R.source_coords(c['tf'][b, 0, 0], c['tf'][b, 0, 2], c['Wo'], c['W'])
    ys = R.source_coords(c['tf'][b, 1, 1], c['tf'][b, 1, 2], c['Ho'], c['H'])
    dx = np.array([float(Fraction(float(a)) - e) for a, e in zip(ox[b], xs)])
    dy = np.array([float(Fraction(float(a)) - e) for a, e in zip(oy[b], ys)])
    same = (dy == 0)[:, None] & (dx == 0)[None, :]
    if c['lattice']:
      assert same.all() or not pow2, (name, b)
      np.testing.assert_array_equal(want[b, :3][:, same], rgb_o[b][:, same])
    assert max(np.abs(dx).max(), np.abs(dy).max()) < 1e-4              # (the chain's noise: far below a pixel)
    # (+ 2 float32 ulps of the coordinate: F.grid_sample un-normalises the grid itself, two more float32 operations at the coordinate's
    # magnitude whose order and fusing the definition does not fix, so the deviation reconstructed above is known only that well)
    ulps = lambda v: 2 * np.spacing(np.maximum(np.abs(v), 1).astype(np.float32)).astype(np.float64)
    val, bound = R.bilinear_f64(c['rgb'], xs, ys, dx=np.abs(dx) + ulps(ox[b]), dy=np.abs(dy) + ulps(oy[b]))
    assert np.all(np.abs(rgb_o[b].transpose(1, 2, 0) - val) <= bound), (name, b)
  val, bound = R.rgb_f64_and_bound(name)                                # the reference's own float32 sum against float64: the derived bound
  assert np.all(np.abs(want[:, :3] - val) <= bound) and float(bound.max()) < 1e-5


def test_depth2xyz_equals_the_oracle():
  from oracle import geometry as G
  for name in ('r17x33', 'big_frame', 'non_lattice'):
    c = R.case(name)
    want = G.depth2xyzmap_batch(torch.from_numpy(c['depth'])[None], torch.as_tensor(c['K'], dtype=torch.float32)[None], zfar=np.inf)[0].numpy()
    np.testing.assert_array_equal(R.depth2xyz_f32(c['depth'], c['K']), want)


def test_warp_nearest_equals_the_oracle():
  from oracle.warp import warp_perspective_nearest
  for name, src, tf, Ho, Wo in warp_cases():
    n = len(tf)
    full = np.broadcast_to(src, (n,) + src.shape[1:]) if len(src) == 1 else src
    want = warp_perspective_nearest(torch.from_numpy(np.ascontiguousarray(full.transpose(0, 3, 1, 2))), torch.from_numpy(tf), (Ho, Wo)).numpy()
    got = R.warp_nearest(src, tf, Ho, Wo)
    np.testing.assert_array_equal(got, want, err_msg=name)
    assert 0.05 < float((got != 0).mean()) < 0.99, name


def warp_cases():
  """(name, src (1 or N,Hs,Ws,C), tf, Ho, Wo) for fp_warp_nearest: the lattice transforms, C in {1, 3, 4}, broadcast and per-item sources, ragged
  Ho * Wo, and a 2 x 2 source on which every other output pixel is an exact tie"""
  out = []
  tf = R.make_tf(R.FAMILY_33x65)
  for C, per_item, (Ho, Wo) in ((1, False, (17, 33)), (3, True, (12, 40)), (4, False, (20, 24)), (3, False, (9, 17)), (4, True, (17, 33))):
    rng = np.random.default_rng(100 + C + 10 * per_item)
    src = rng.integers(1, 1000, (len(tf) if per_item else 1, 33, 65, C)).astype(np.float32)
    out.append((f'c{C}_{"items" if per_item else "bcast"}_{Ho}x{Wo}', src, tf, Ho, Wo))
  tiny = R.make_tf(R.LATTICE['tiny_frame'][5])
  out.append(('tiny_source', np.arange(1, 2 * 2 * 2 * 3 + 1, dtype=np.float32).reshape(2, 2, 2, 3), tiny, 9, 17))
  return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# what the cases hold
# ------------------------------------------------------------------------------------------------------------------------------------------
def _all_infos(lattice_only=True):
  for name, mode in R.RUNS:
    c = R.case(name)
    if lattice_only and not c['lattice']:
      continue
    for b, info in enumerate(R.expected(name, mode, True)[1]):
      yield c, mode, b, info


def _is_tie(v):
  return v - math.floor(v) == R.HALF


def test_lattice_coordinates_are_exact_in_float32():
  for c, mode, b, info in _all_infos():
    for v in info['xs'] + info['ys'] + info.get('bx', []) * (c['name'] != 'production') + info.get('by', []) * (c['name'] != 'production'):
      assert Fraction(float(np.float32(float(v)))) == v, (c['name'], b, v)


def test_cases_hold_ties_borders_and_windows():
  n = dict.fromkeys(('x_even', 'x_odd', 'y_even', 'y_odd', 'neg_floor', 'm0.5', 'm1.5', 'W-0.5', 'H-0.5', 'left', 'right', 'top', 'bottom', 'outside',
                     'neg_x', 'back_ties', 'taps2', 'taps3', 'taps4', 'taps0'), 0)
  for c, mode, b, info in _all_infos():
    H, W = c['H'], c['W']
    for axis, vs, size in (('x', info['xs'], W), ('y', info['ys'], H)):
      for v in vs:
        if _is_tie(v):
          f = math.floor(v)
          n[f'{axis}_even' if f % 2 == 0 else f'{axis}_odd'] += 1
          n['neg_floor'] += f < 0
          n['m0.5'] += v == -R.HALF and R.nearest_index(v) == 0
          n['m1.5'] += v == Fraction(-3, 2) and R.nearest_index(v) == -2
          n['W-0.5' if axis == 'x' else 'H-0.5'] += v == size - R.HALF and R.nearest_index(v) == size - 1
    n['neg_x'] += sum(v < 0 for v in info['xs'])
    n['back_ties'] += sum(_is_tie(v) for v in info.get('bx', []) + info.get('by', []))
    qx, qy = np.array(info['qx']), np.array(info['qy'])
    inx, iny = (qx >= 0) & (qx < W), (qy >= 0) & (qy < H)
    if inx.any() and iny.any():                       # a window that crosses an edge: pixels on both sides of it
      n['left'] += (qx < 0).any()
      n['right'] += (qx >= W).any()
      n['top'] += (qy < 0).any()
      n['bottom'] += (qy >= H).any()
    else:
      n['outside'] += bool(c['poses'][b, :3, 3].any())
      for norm in (True, False):                      # all zero but the xyz of normalize_xyz = False, which is -t
        out = R.expected(c['name'], mode, norm)[0][b]
        assert not out[:3].any()
        want = np.zeros(3, np.float32) if norm else -c['poses'][b, :3, 3]
        assert (out[3:] == want.reshape(3, 1, 1)).all()
    t = R.taps_outside(info['xs'], info['ys'], H, W)
    for k in (0, 2, 3, 4):
      n[f'taps{k}'] += int((t == k).sum())
    assert not (t == 1).any()                         # (one tap outside cannot happen on a rectangle)
  print(n)
  assert min(n['x_even'], n['x_odd'], n['y_even'], n['y_odd']) >= 4, n
  assert n['neg_floor'] >= 4 and n['m0.5'] >= 4 and n['m1.5'] >= 2 and n['W-0.5'] >= 2 and n['H-0.5'] >= 2, n
  assert min(n['left'], n['right'], n['top'], n['bottom']) >= 2 and n['outside'] >= 4, n
  assert n['neg_x'] >= 150 and n['back_ties'] >= 4, n
  assert n['taps0'] >= 1000 and n['taps2'] >= 50 and n['taps3'] >= 4 and n['taps4'] >= 100, n


def test_band_probes_sit_where_they_claim():
  c = R.case('band_probes')
  _, infos = R.expected('band_probes', 0, True)
  seen = set()
  for (kx, ky, d), info in zip(c['probes'], infos):
    for v, k, q in ((info['xs'][R.PROBE_I], kx, info['qx'][R.PROBE_I]), (info['ys'][R.PROBE_J], ky, info['qy'][R.PROBE_J])):
      off = float(v - (k + R.HALF))
      assert abs(off - d) < 1e-5 and abs(float(v)) < 100          # float32 offsets land within 1e-5 of the target: clear of the band's edge
      snapped = abs(d) < 1e-4
      naive = math.floor(v + R.HALF)
      assert q == ((k if k % 2 == 0 else k + 1) if snapped else naive)
      seen.add((k % 2, d > 0, snapped, q != naive))
  # both parities, both sides, inside and outside the band; the snap changes the index on one side per parity, and never outside the band
  assert {(p, s, sn) for p, s, sn, _ in seen} == {(p, s, sn) for p in (0, 1) for s in (True, False) for sn in (True, False)}
  assert {(p, s) for p, s, sn, ch in seen if ch} == {(0, True), (1, False)} and not any(ch for _, _, sn, ch in seen if not sn)
  wide = R.crop_observed(c['rgb'], c['xyz'], c['K'], c['tf'], c['poses'], c['Ho'], c['Wo'], 0, c['diameter'], True, eps=Fraction(1, 1000))
  none = R.crop_observed(c['rgb'], c['xyz'], c['K'], c['tf'], c['poses'], c['Ho'], c['Wo'], 0, c['diameter'], True, eps=Fraction(0))
  want = R.expected('band_probes', 0, True)[0]
  assert (wide != want).any() and (none != want).any()            # a band ten times wider, or no band at all, is seen


def test_cases_hold_the_threshold_values():
  two, below2 = np.float32(2), np.nextafter(np.float32(2), np.float32(0))
  n = dict.fromkeys(('z001_0', 'z001b_0', 'z001_1', 'z001b_1', 'z01', 'z01b', 'two_0', 'below2_0', 'two_1', 'below2_1', 'mtwo'), 0)
  for c, mode, b, info in _all_infos():
    z, pre = info['xyz'][..., 2], info['pre']
    src = z if mode == 0 else info['depth_frame']
    n[f'z001_{mode}'] += int((src == np.float32(0.001)).sum())
    n[f'z001b_{mode}'] += int((src == R.BELOW(0.001)).sum())
    if mode == 1:
      n['z01'] += int((z == np.float32(0.1)).sum())
      n['z01b'] += int((z == R.BELOW(0.1)).sum())
    live = ~np.broadcast_to(info['invalid'], pre.shape)
    n[f'two_{mode}'] += int(((pre == two) & live).sum())
    n[f'below2_{mode}'] += int(((pre == below2) & live).sum())
    n['mtwo'] += int(((pre == -two) & live).sum())
    # the same pixels with normalize_xyz = 0: nothing is zeroed; an empty scorer pixel is -t
    plain = R.expected(c['name'], mode, False)[0][b]
    np.testing.assert_array_equal(plain[3:], (info['xyz'] - c['poses'][b, :3, 3]).transpose(2, 0, 1))
  print(n)
  assert all(v >= 3 for v in n.values()), n


def test_lattice_bilinear_sums_are_exact_in_float32():
  """Every weight, every tap product and every partial sum of the lattice cases is a float32 number: evaluated in Fractions and pushed through
  float32, nothing moves.  The rgb of the reference (and of the kernel) then carries one rounding, the IEEE division by 255."""
  exact = lambda v: Fraction(float(np.float32(float(v)))) == v
  checked = 0
  for c, mode, b, info in _all_infos():
    if mode != c['modes'][0] or c['name'] == 'production':            # (same coordinates in both modes; the production size repeats r17x33's family)
      continue
    H, W, rgb = c['H'], c['W'], c['rgb']
    px = lambda y, x, ch: Fraction(float(rgb[y, x, ch])) if 0 <= y < H and 0 <= x < W else Fraction(0)
    out = R.expected(c['name'], mode, True)[0][b]
    for j, y in enumerate(info['ys']):
      y0 = math.floor(y)
      for i, x in enumerate(info['xs']):
        x0 = math.floor(x)
        wx1, wy1, wx0, wy0 = x - x0, y - y0, x0 + 1 - x, y0 + 1 - y
        assert all(map(exact, (wx0, wx1, wy0, wy1)))
        for ch in range(3):
          acc = Fraction(0)
          for tap, w in ((px(y0, x0, ch), wx0 * wy0), (px(y0, x0 + 1, ch), wx1 * wy0), (px(y0 + 1, x0, ch), wx0 * wy1), (px(y0 + 1, x0 + 1, ch), wx1 * wy1)):
            assert exact(w) and exact(tap * w)
            acc += tap * w
            assert exact(acc)
          assert out[ch, j, i] == np.float32(float(acc)) / np.float32(255)
          checked += 1
  assert checked > 20000


@pytest.mark.parametrize('broken', ['ties_half_up', 'gt_instead_of_ge'])
def test_broken_references_are_told_apart(broken):
  kw = dict(tie='up') if broken == 'ties_half_up' else dict(ge2=False)
  differing = 0
  for name, mode in R.RUNS:
    c = R.case(name)
    if not c['lattice'] or name == 'production':
      continue
    bad = R.crop_observed(c['rgb'], c['xyz'] if mode == 0 else c['depth'], c['K'], c['tf'], c['poses'], c['Ho'], c['Wo'], mode, c['diameter'], True, **kw)
    differing += int((bad != R.expected(name, mode, True)[0]).sum())
  assert differing >= 20, differing


def test_half_form_is_the_rounded_float32_form():
  want, _ = R.expected('r17x33', 0, True)
  h = R.to_nhwc8_half(want)
  assert h.shape == (len(want), 17, 33, 8) and h.dtype == np.float16 and not h[..., 6:].any()
  np.testing.assert_array_equal(h[..., :6].transpose(0, 3, 1, 2), want.astype(np.float16))
