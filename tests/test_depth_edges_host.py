"""Crafted inputs for the depth prelude (erode_depth, bilateral_filter_depth, depth2xyzmap_batch, depth_prefilter) and the radix-select median
(mask_depth_stats), with the CPU checks that they sit on the thresholds they name.  tests/test_gpu_depth_edges.py runs the kernels on them.
The reference is the oracle's float32 CPU code (oracle/geometry.py); nothing here needs a GPU.

Images are 9 x 11 and 13 x 37 (the 32 x 8 workgroup tiles are cut on both axes) and 5 x 3 (smaller than the radius-2 window)."""
import numpy as np
import pytest

f32 = np.float32
E = f32(0.01)                        # the bilateral filter's 1 cm gate: 0x3C23D70A, a multiple of 2^-29
M = f32(2.0 ** -7)                   # window mean of the gate cases


def window(H, W, h, w, radius=2):
  """pixels of the (2 radius + 1)^2 window of (h, w) inside the image, in the kernels' order (columns outer, rows inner), centre excluded"""
  return [(v, u) for u in range(w - radius, w + radius + 1) for v in range(h - radius, h + radius + 1)
          if 0 <= u < W and 0 <= v < H and (v, u) != (h, w)]


def bad_total(depth, h, w, radius, diff_thres, zfar):
  """erode_depth's counts at one pixel, from its definition (src/Utils.py:359-385)"""
  H, W = depth.shape
  cells = window(H, W, h, w, radius) + [(h, w)]
  bad = sum(1 for v, u in cells if depth[v, u] < f32(0.001) or depth[v, u] >= f32(zfar) or abs(f32(depth[v, u] - depth[h, w])) > f32(diff_thres))
  return bad, len(cells)


# (h, w, number of bad neighbours) per image size: windows do not overlap.  total = 25 inside, 15 on an edge, 9 in a corner; with
# ratio_thres = 0.8 the pixel is kept at bad / total = 20/25 = 12/15 (not > 0.8) and at 7/9, eroded at 21/25, 13/15 and 8/9
ERODE_TARGETS = {
    (13, 37): [(0, 0, 7), (12, 36, 8), (0, 18, 12), (12, 18, 13), (5, 25, 20), (5, 31, 21), (6, 0, 12), (6, 36, 13)],
    (9, 11): [(0, 0, 8), (4, 5, 20), (8, 10, 7)],
}
KEPT = {(25, 20), (15, 12), (9, 7)}


def erode_image(hw, good, bad_value):
  """background and centres `good`; the first `n` window pixels of every target `bad_value`"""
  H, W = hw
  d = np.full((H, W), good, dtype=np.float32)
  for h, w, n in ERODE_TARGETS[hw]:
    for v, u in window(H, W, h, w)[:n]:
      d[v, u] = bad_value
  return d


# name: (good, bad value, the same value made harmless, dict(depth_diff_thres, zfar))
ERODE_KINDS = {
    'invalid': (f32(1.0), f32(0.0), f32(1.0), dict(depth_diff_thres=0.001, zfar=100)),
    # |cur - d_ori| > diff_thres with diff_thres = 2^-10: exactly 2^-10 is not bad, one ulp more is
    'diff': (f32(1.0), f32(1.0) + f32(2.0 ** -10) + f32(2.0 ** -23), f32(1.0) + f32(2.0 ** -10), dict(depth_diff_thres=2.0 ** -10, zfar=100)),
    # cur >= zfar: a pixel EQUAL to zfar is bad, its nextafter below is not (diff_thres out of the way)
    'zfar': (f32(1.5), f32(2.0), np.nextafter(f32(2.0), f32(0)), dict(depth_diff_thres=10.0, zfar=2.0)),
}


def erode_cases():
  """(name, depth, kwargs of erode_depth) - every kind at both sizes, with the bad value and with its harmless neighbour"""
  for hw in ERODE_TARGETS:
    for kind, (good, bad, harmless, kw) in ERODE_KINDS.items():
      yield f'{kind}_{hw[0]}x{hw[1]}', erode_image(hw, good, bad), kw
      if kind != 'invalid':
        yield f'{kind}_harmless_{hw[0]}x{hw[1]}', erode_image(hw, good, harmless), kw


def noise_image(hw, seed):
  """quantised depths around 0.8 m with holes, sub-millimetre values, values at and beyond zfar = 2: every branch of the three kernels"""
  rng = np.random.default_rng(seed)
  pool = np.array([0, 0.0005, 0.001, 0.8, 0.8005, 0.801, 0.802, 0.805, 0.8098, 0.81, 0.82, 2.0, np.nextafter(f32(2.0), f32(0)), 150.0], dtype=np.float32)
  p = np.array([6, 1, 1, 20, 10, 10, 10, 8, 4, 6, 4, 2, 2, 1], dtype=np.float64)
  return pool[rng.choice(len(pool), size=hw, p=p / p.sum())]


NOISE_SIZES = ((9, 11), (13, 37), (5, 3))


def gate_image(hw, probe):
  """One window around (4, 5) in an otherwise empty image: q, q in the window's first column, the centre M, the probe in its last column, with
  q = M - E/2 and probe = M + E.  All four are multiples of 2^-30 below 2^-5 and their partial sums in the kernels' order are float32 numbers, so
  the window mean is exactly M and |probe - mean| = E: the 1 cm gate `< 0.01f` leaves it out.  probe = nextafter(M + E, 0) is just inside."""
  d = np.zeros(hw, dtype=np.float32)
  q = M - E / f32(2)
  d[3, 3], d[5, 3], d[4, 5], d[4, 7] = q, q, M, probe
  return d


def bilateral_pixel(depth, h, w, radius=2, zfar=100.0, sigmaD=2.0, sigmaR=100000.0, gate=lambda a: a < float(E), below_zfar=lambda c, z: c < z):
  """bilateral_filter_depth at one pixel in float64 with the float32 window mean, with exchangeable comparisons: what a kernel with `<=` at the
  gate or at zfar would give.  Returns (value, contributing pixels)."""
  H, W = depth.shape
  cells = [(v, u) for u in range(w - radius, w + radius + 1) for v in range(h - radius, h + radius + 1) if 0 <= u < W and 0 <= v < H]
  valid = [(v, u) for v, u in cells if depth[v, u] >= f32(0.001) and below_zfar(float(depth[v, u]), zfar)]
  if not valid:
    return 0.0, []
  mean = f32(0)
  for v, u in valid:
    mean = f32(mean + depth[v, u])
  mean = f32(mean / f32(len(valid)))
  used = [(v, u) for v, u in valid if gate(float(abs(f32(depth[v, u] - mean))))]
  ws = [np.exp(-((u - w) ** 2 + (v - h) ** 2) / (2.0 * sigmaD * sigmaD) - (float(depth[h, w]) - float(depth[v, u])) ** 2 / (2.0 * sigmaR * sigmaR)) for v, u in used]
  return (sum(wt * float(depth[v, u]) for wt, (v, u) in zip(ws, used)) / sum(ws) if used else 0.0), used


def zfar_bilateral_image(hw):
  """values 5 mm under zfar = 2 and pixels EQUAL to zfar around (4, 5): `cur < zfar` leaves those out; taken in, they would pass the 1 cm gate"""
  d = np.zeros(hw, dtype=np.float32)
  d[2:7, 3:8] = f32(1.995)
  d[3, 4], d[5, 6], d[4, 7] = f32(2.0), f32(2.0), f32(2.0)
  return d


def split_window_image(hw):
  """num_valid > 0 but nothing passes the gate (1.0 and 1.5 around a mean of 1.25): sum_w == 0 gives 0"""
  d = np.zeros(hw, dtype=np.float32)
  d[4, 5], d[4, 6] = f32(1.0), f32(1.5)
  return d


MARGIN = 1e-4                        # a wrongly included or excluded neighbour moves the result by more than this; the comparison allows 2e-6


# ------------------------------------------------------------------------------------------------------------------------------------------
# CPU checks
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_erode_targets_sit_on_the_ratio_boundary():
  from oracle import geometry as G
  seen = set()
  for name, d, kw in erode_cases():
    hw = d.shape
    out = G.erode_depth(d, radius=2, ratio_thres=0.8, **kw)
    for h, w, n in ERODE_TARGETS[hw]:
      bad, total = bad_total(d, h, w, 2, kw['depth_diff_thres'], kw['zfar'])
      if 'harmless' in name:
        assert bad == 0 and out[h, w] == d[h, w], (name, h, w)
        continue
      assert (bad, total) == (n, len(window(hw[0], hw[1], h, w)) + 1), (name, h, w, bad, total)
      assert (out[h, w] == d[h, w]) == ((total, bad) in KEPT) and (out[h, w] == 0) == ((total, bad) not in KEPT), (name, h, w)
      seen.add((total, bad))
    # ratio_thres 0: any bad neighbour erodes; 1: nothing is ever eroded
    np.testing.assert_array_equal(G.erode_depth(d, radius=2, ratio_thres=1.0, **kw), d)
    if 'harmless' not in name:
      assert (G.erode_depth(d, radius=2, ratio_thres=0.0, **kw)[[t[0] for t in ERODE_TARGETS[hw]], [t[1] for t in ERODE_TARGETS[hw]]] == 0).all()
  assert seen == {(25, 20), (25, 21), (15, 12), (15, 13), (9, 7), (9, 8)}


def test_gate_and_zfar_cases_sit_on_their_boundaries():
  from oracle import geometry as G
  for hw in ((9, 11), (13, 37)):
    on, inside = gate_image(hw, M + E), gate_image(hw, np.nextafter(M + E, f32(0)))
    assert float(M + E) == float(M) + float(E)                      # (representable: the probe is exactly 1 cm above the mean)
    for d, n_used in ((on, 3), (inside, 4)):
      val, used = bilateral_pixel(d, 4, 5)
      assert len(used) == n_used
      got = float(G.bilateral_filter_depth(d, radius=2)[4, 5])
      assert abs(got - val) < 2e-6
      other, used2 = bilateral_pixel(d, 4, 5, gate=(lambda a: a <= float(E)) if n_used == 3 else (lambda a: a < 0.999 * float(E)))
      assert len(used2) != n_used and abs(other - val) > MARGIN      # `<=` at the gate (resp. a gate 0.1 % tighter) is told apart
    z = zfar_bilateral_image(hw)
    val, used = bilateral_pixel(z, 4, 5, zfar=2.0)
    other, used2 = bilateral_pixel(z, 4, 5, zfar=2.0, below_zfar=lambda c, zf: c <= zf)
    assert len(used) == 22 and len(used2) == 25 and abs(other - val) > MARGIN
    assert abs(float(G.bilateral_filter_depth(z, radius=2, zfar=2.0)[4, 5]) - val) < 2e-6
    s = split_window_image(hw)
    assert bilateral_pixel(s, 4, 5) == (0.0, []) and G.bilateral_filter_depth(s, radius=2)[4, 5] == 0 and G.bilateral_filter_depth(s, radius=2)[4, 6] == 0


# ------------------------------------------------------------------------------------------------------------------------------------------
# radix-select median: crafted values
# ------------------------------------------------------------------------------------------------------------------------------------------
def bits(*patterns):
  return np.array(patterns, dtype=np.uint32).view(np.float32)


def median_value_sets():
  """name -> float32 usable values (all >= 0.001)"""
  rng = np.random.default_rng(3)
  quant = np.array([0.731, 0.732, 0.733], dtype=np.float32)
  dup = np.concatenate([quant[rng.integers(0, 3, 360)], rng.uniform(0.4, 1.2, 40).astype(np.float32)])
  sets = {
      'n1': bits(0x3F000001), 'n2': bits(0x3F000001, 0x3F7FFFFF), 'n3': bits(0x3F000001, 0x3F7FFFFF, 0x3E800000),
      'n4': bits(0x3F000001, 0x3F7FFFFF, 0x3E800000, 0x40000000),
      # an even count whose two middle values part in the top byte (0x3F | 0x40), in byte 2 (0x7F | 0x80) and in byte 1 (0x00FF | 0x0100)
      'straddle_byte3': bits(*([0x3F000000] * 7 + [0x3FFFFFFF, 0x40000000] + [0x40400000] * 7)),
      'straddle_byte2': bits(*([0x3F000000] * 7 + [0x3F7FFFFF, 0x3F800000] + [0x40400000] * 7)),
      'straddle_byte1': bits(*([0x3F000000] * 7 + [0x3F8000FF, 0x3F800100] + [0x40400000] * 7)),
      'all_equal': np.full(300, 0.8125, dtype=np.float32),
      'duplicates': dup,
      # the selected statistic has 0xFF in its three low bytes: the last bucket of the scan, three passes running
      'ff_selected': bits(*([0x3F000000] * 5 + [0x3FFFFFFF] + [0x40400000] * 5)),
      'ff_even': bits(*([0x3F000000] * 5 + [0x3FFFFFFF, 0x3FFFFFFF] + [0x40400000] * 5)),
      'at_min_depth': np.array([0.001, 0.001, 0.5], dtype=np.float32),
  }
  return sets


def median_case(hw, values, layout='scatter', mask_byte=1, seed=0):
  """(depth, mask uint8): the values at masked pixels; further masked pixels just under min_depth (not usable); unmasked pixels hold large and
  tiny junk.  layout: scatter | row | column | full (the bounding box: some rows / one row / one column / the whole image)."""
  H, W = hw
  rng = np.random.default_rng(seed)
  depth = np.where(rng.uniform(size=hw) < 0.5, f32(7.5), f32(0.25)).astype(np.float32)
  mask = np.zeros(hw, dtype=np.uint8)
  if layout == 'row':
    cells = [(H // 2, u) for u in range(W)]
  elif layout == 'column':
    cells = [(v, W // 3) for v in range(H)]
  elif layout == 'full':
    cells = [(v, u) for v in range(H) for u in range(W)]
  else:
    cells = [(v, u) for v in range(H // 8, H - H // 8) for u in range(W // 8, W - W // 8)]
  if layout != 'full':
    cells = [cells[i] for i in rng.permutation(len(cells))]
  n = min(len(values), len(cells))
  n_mask = min(len(cells), n + n // 3 + 1) if layout == 'scatter' else len(cells)
  below = np.nextafter(f32(0.001), f32(0))
  for k, (v, u) in enumerate(cells[:n_mask]):
    mask[v, u] = mask_byte
    depth[v, u] = values[k] if k < n else (below if k % 2 else f32(0))
  return depth, mask


def median_cases():
  """(name, depth, mask)"""
  sets = median_value_sets()
  yield '1x1', *median_case((1, 1), sets['n1'], 'full')
  for k in ('n1', 'n2', 'n3', 'n4'):
    yield f'3x5_{k}', *median_case((3, 5), sets[k], 'scatter', seed=1)
  for k, v in sets.items():
    yield f'25x41_{k}', *median_case((25, 41), v, 'scatter', mask_byte=2 if 'straddle' in k else 255 if 'ff' in k else 1, seed=2)
  yield '25x41_row', *median_case((25, 41), sets['duplicates'], 'row', seed=3)
  yield '25x41_column', *median_case((25, 41), sets['straddle_byte3'], 'column', mask_byte=255, seed=4)
  yield '25x41_full', *median_case((25, 41), np.resize(sets['duplicates'], 1025), 'full', seed=5)


def median_expected(depth, mask, min_depth=0.001):
  """numpy's statistics: (cmin, cmax, rmin, rmax, n_mask, n_usable), np.median of the float32 usable values"""
  vs, us = np.where(mask != 0)
  usable = depth[(mask != 0) & (depth >= f32(min_depth))]
  assert usable.dtype == np.float32
  med = np.median(usable) if len(usable) else f32(0)
  return (int(us.min()), int(us.max()), int(vs.min()), int(vs.max()), len(us), len(usable)), f32(med)


def test_median_cases_hold_what_they_name():
  cases = {name: (d, m) for name, d, m in median_cases()}
  counts = {name: median_expected(d, m)[0][5] for name, (d, m) in cases.items()}
  assert [counts[f'3x5_n{k}'] for k in (1, 2, 3, 4)] == [1, 2, 3, 4] and counts['1x1'] == 1 and counts['25x41_full'] == 1025
  for b, (lo, hi) in ((3, (0x3FFFFFFF, 0x40000000)), (2, (0x3F7FFFFF, 0x3F800000)), (1, (0x3F8000FF, 0x3F800100))):
    d, m = cases[f'25x41_straddle_byte{b}']
    u = np.sort(d[(m != 0) & (d >= f32(0.001))])
    assert len(u) == 16 and list(u[7:9].view(np.uint32)) == [lo, hi] and median_expected(d, m)[1] == f32((u[7] + u[8]) / f32(2))
    assert (lo >> (8 * b)) != (hi >> (8 * b)) and (b == 3 or (lo >> (8 * b + 8)) == (hi >> (8 * b + 8)))
  d, m = cases['25x41_ff_selected']
  assert median_expected(d, m)[1].view(np.uint32) == 0x3FFFFFFF and median_expected(*cases['25x41_ff_even'])[1].view(np.uint32) == 0x3FFFFFFF
  d, m = cases['25x41_duplicates']
  u = d[(m != 0) & (d >= f32(0.001))]
  assert len(u) == 400 and len(np.unique(u)) <= 43
  d, m = cases['25x41_at_min_depth']
  assert (d[m != 0] == f32(0.001)).sum() == 2 and (d[m != 0] == np.nextafter(f32(0.001), f32(0))).sum() >= 1 and median_expected(d, m)[0][5] == 3
  assert {int(m.max()) for _, m in cases.values()} == {1, 2, 255}
  for name, (rows, cols) in (('25x41_row', (1, 41)), ('25x41_column', (25, 1)), ('25x41_full', (25, 41))):
    st = median_expected(*cases[name])[0]
    assert (st[3] - st[2] + 1, st[1] - st[0] + 1) == (rows, cols)
