"""Depth from a rectified stereo pair (fp_stereo_sgm) restated in numpy, rule for rule as include/foundationpose_amd.h states it: grey,
9 x 7 census, Hamming cost, the eight-path semi-global recurrence with constant P1 / P2, the lowest minimal disparity, the left-right
check, the parabola and fb / disparity.  Everything up to the winning disparity is integer, so the GPU has to match it bit for bit; the
two float32 steps are single correctly rounded operations in the written order.  A checker: never imported by the product."""
import numpy as np

# bit b of `paths`: the step r = (dy, dx) of a walk; the recurrence at p looks back at q = p - r
DIRS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))
_POP8 = np.array([bin(i).count('1') for i in range(256)], np.uint8)


def popcount64(a):
  a = np.ascontiguousarray(a, dtype=np.uint64)
  return _POP8[a.view(np.uint8).reshape(a.shape + (8,))].sum(-1, dtype=np.int32)


def grey(img):
  img = np.asarray(img)
  assert img.dtype == np.uint8 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)), (img.dtype, img.shape)
  if img.ndim == 2:
    return img
  c = img.astype(np.uint32)
  return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def census(g):
  """(H,W) uint8 -> (H,W) uint64: 62 neighbours row-major, the first in bit 61, coordinates clamped, bit = neighbour < centre."""
  H, W = g.shape
  pad = np.pad(g, ((3, 3), (4, 4)), mode='edge')
  code = np.zeros((H, W), np.uint64)
  for dy in range(-3, 4):
    for dx in range(-4, 5):
      if dy == 0 and dx == 0:
        continue
      nb = pad[3 + dy:3 + dy + H, 4 + dx:4 + dx + W]
      code = (code << np.uint64(1)) | (nb < g).astype(np.uint64)
  return code


def cost(cl, cr, D):
  """(H,W,D) uint8: popcount(cl(y,x) ^ cr(y,x-d)), 64 where x - d < 0."""
  H, W = cl.shape
  C = np.full((H, W, D), 64, np.uint8)
  for d in range(min(D, W)):
    C[:, d:, d] = popcount64(cl[:, d:] ^ cr[:, :W - d])
  return C


def _step(prev, c, P1, P2):
  """One pixel of the recurrence for a stack of lines: prev = L_r(q, .), c = C(p, .), both (N, D) int32."""
  m = prev.min(1, keepdims=True)
  best = np.minimum(prev, m + P2)
  best[:, 1:] = np.minimum(best[:, 1:], prev[:, :-1] + P1)
  best[:, :-1] = np.minimum(best[:, :-1], prev[:, 1:] + P1)
  return c + best - m


def path(C, r, P1=8, P2=32):
  """L_r (H,W,D) int32 of direction bit r."""
  dy, dx = DIRS[r]
  H, W, D = C.shape
  C = C.astype(np.int32)
  L = C.copy()
  if dy == 0:
    for x in (range(1, W) if dx > 0 else range(W - 2, -1, -1)):
      L[:, x] = _step(L[:, x - dx], C[:, x], P1, P2)
  else:
    lo, hi = max(0, dx), W + min(0, dx)      # the columns whose q = (y - dy, x - dx) is inside
    for y in (range(1, H) if dy > 0 else range(H - 2, -1, -1)):
      if hi > lo:
        L[y, lo:hi] = _step(L[y - dy, lo - dx:hi - dx], C[y, lo:hi], P1, P2)
  return L


def aggregate(C, paths=0xFF, P1=8, P2=32):
  S = np.zeros(C.shape, np.int64)
  for r in range(8):
    if paths >> r & 1:
      S += path(C, r, P1, P2)
  assert S.max() <= 65535
  return S.astype(np.uint16)


def winners(S):
  """(d* (H,W) int32, d_R (H,W) int32): lowest minimising d of S(y,x,.) and of S(y,x+d,d) over x + d < W."""
  H, W, D = S.shape
  ds = S.argmin(2).astype(np.int32)
  SR = np.full((H, W, D), 1 << 20, np.int64)
  for d in range(min(D, W)):
    SR[:, :W - d, d] = S[:, d:, d]
  return ds, SR.argmin(2).astype(np.int32)


def sgm(left, right, max_disparity=128, p1=8, p2=32, paths=0xFF, lr_max=1, min_disparity=1, subpixel=True, fx=None, baseline=None,
        zfar=np.inf):
  """One pair.  A dict of every stage: grey_l, grey_r, census_l, census_r, cost, sum, dstar, dright, valid, disparity and, with fx and
  baseline, depth."""
  D = int(max_disparity)
  gl, gr = grey(left), grey(right)
  H, W = gl.shape
  cl, cr = census(gl), census(gr)
  C = cost(cl, cr, D)
  S = aggregate(C, paths, p1, p2)
  ds, dr = winners(S)
  xs = np.arange(W)[None, :] - ds
  valid = (xs >= 0) & (ds >= min_disparity)
  if lr_max >= 0:
    valid &= np.abs(np.take_along_axis(dr, np.clip(xs, 0, W - 1), 1) - ds) <= lr_max
  disp = ds.astype(np.float32)
  if subpixel:
    Si = S.astype(np.int32)
    dc = np.clip(ds, 1, D - 2)[..., None]
    a, b, c = (np.take_along_axis(Si, dc + o, 2)[..., 0] for o in (-1, 0, 1))
    den = a - 2 * b + c
    ok = (ds > 0) & (ds < D - 1) & (den > 0)
    off = (a - c).astype(np.float32) / np.where(ok, 2 * den, 1).astype(np.float32)
    disp = np.where(ok, disp + off, disp).astype(np.float32)
  disp = np.where(valid, disp, np.float32(-1)).astype(np.float32)
  out = dict(grey_l=gl, grey_r=gr, census_l=cl, census_r=cr, cost=C, sum=S, dstar=ds, dright=dr, valid=valid, disparity=disp)
  if fx is not None:
    fb = np.float32(float(fx) * float(baseline))
    with np.errstate(divide='ignore', invalid='ignore'):
      z = (fb / disp).astype(np.float32)
    out['depth'] = np.where(valid & (disp > 0) & ~(z > np.float32(zfar)), z, np.float32(0)).astype(np.float32)
  return out


def stereogram(seed, H=40, W=176, D=64, bg=6, fg=41):
  """The random-dot pair of tests/test_stereo_host.py: (left, right, truth (H,W) int32, occluded (H,W) bool)."""
  rng = np.random.default_rng(seed)
  tex = rng.integers(0, 256, (H, W + D + 8)).astype(np.uint8)
  texf = rng.integers(0, 256, (H, W + D + 8)).astype(np.uint8)
  right = tex[:, D:D + W].copy()
  left = tex[:, D - bg:D - bg + W].copy()
  y0, y1, x0, x1 = H // 4, 3 * H // 4, W // 3, 2 * W // 3
  left[y0:y1, x0:x1] = texf[y0:y1, x0:x1]
  right[y0:y1, x0 - fg:x1 - fg] = texf[y0:y1, x0:x1]
  truth = np.full((H, W), bg, np.int32)
  truth[y0:y1, x0:x1] = fg
  occ = np.zeros((H, W), bool)
  occ[y0:y1, x0 - fg + bg:x1 - fg + bg] = True      # background whose partner the foreground covers in the right image
  occ[y0:y1, x0:x1] = False
  return left, right, truth, occ
