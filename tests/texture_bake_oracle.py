"""numpy restatement of the texture-baking rule of include/foundationpose_amd.h (fp_texture_bake): the per-face atlas and the colour of
every texel in np.float32, operation for operation in the stated order.  It imports nothing from foundationpose_amd - the product cannot
check itself.  Also here, because the host and the GPU tests both need it: the rasteriser's bilinear texel indices and weights
(csrc/raster.hip, the texture fetch) in float32."""
import numpy as np

from tests.tsdf_oracle import invert_view

F32 = np.float32


def grid(n_faces):
  """the smallest g with g * g >= ceil(n_faces / 2)"""
  cells = (int(n_faces) + 1) // 2
  g = 1
  while g * g < cells:
    g += 1
  return g


def cell(T, n_faces):
  return int(T) // grid(n_faces)


def owners(T, n_faces):
  """(face (T,T) int64 or -1, i (T,T), j (T,T)): the owner of every texel [row, column] and its position inside the owner's patch,
  counted from the patch's corner 0 (for B: c-1-i, c-1-j)."""
  g, c = grid(n_faces), cell(T, n_faces)
  assert c >= 4
  Y, X = np.meshgrid(np.arange(T), np.arange(T), indexing='ij')
  col, row = X // c, Y // c
  i, j = X - col * c, Y - row * c
  inside = (col < g) & (row < g)
  k = row * g + col
  A, B = inside & (i + j <= c - 2), inside & (i + j >= c)
  face = np.where(A, 2 * k, np.where(B, 2 * k + 1, -1))
  face = np.where(face >= n_faces, -1, face)
  i, j = np.where(B, c - 1 - i, i), np.where(B, c - 1 - j, j)
  return face.astype(np.int64), i, j


def atlas_uv(T, n_faces):
  """(3F,2) float32 in the rasteriser's convention: the texel centres of the corners of every face's patch"""
  g, c = grid(n_faces), cell(T, n_faces)
  m = c - 3
  f = np.arange(n_faces)
  k, B = f // 2, (f % 2) == 1
  col, row = k % g, k // g
  ci = np.stack([np.where(B, c - 1, 0), np.where(B, c - 1 - m, m), np.where(B, c - 1, 0)], 1)
  cj = np.stack([np.where(B, c - 1, 0), np.where(B, c - 1, 0), np.where(B, c - 1 - m, m)], 1)
  u = ((col[:, None] * c + ci).astype(F32) + F32(0.5)) / F32(T)
  v = ((row[:, None] * c + cj).astype(F32) + F32(0.5)) / F32(T)
  return np.stack([u, v], -1).reshape(-1, 2).astype(F32)


def bilinear_taps(u, v, T):
  """The rasteriser's fetch at uv (float32 arrays): ((x0, y0), (x1, y0), (x0, y1), (x1, y1)) texel indices and their weights, float32."""
  u, v = np.asarray(u, dtype=F32), np.asarray(v, dtype=F32)
  x, y = u * F32(T) - F32(0.5), v * F32(T) - F32(0.5)
  fx0, fy0 = np.floor(x), np.floor(y)
  fx, fy = x - fx0, y - fy0
  x0, y0 = np.mod(fx0.astype(np.int64), T), np.mod(fy0.astype(np.int64), T)
  x1, y1 = (x0 + 1) % T, (y0 + 1) % T
  one = F32(1)
  taps = ((x0, y0, (one - fx) * (one - fy)), (x1, y0, fx * (one - fy)), (x0, y1, (one - fx) * fy), (x1, y1, fx * fy))
  assert all(w.dtype == F32 for _, _, w in taps)
  return taps


def texel_points(pos, faces, T):
  """float64, for the tests' own expectations: (own (T,T) bool, face (N,), clamped barycentrics (N,3), surface point (N,3)) of the N
  owned texels in row-major order"""
  pos, faces = np.asarray(pos, dtype=np.float64), np.asarray(faces, dtype=np.int64)
  face, i, j = owners(T, len(faces))
  own = face >= 0
  m = cell(T, len(faces)) - 3
  b1, b2 = i[own] / m, j[own] / m
  b0 = 1 - b1 - b2
  neg = b0 < 0
  s = np.where(neg, b1 + b2, 1)
  b = np.stack([np.where(neg, 0, b0), b1 / s, b2 / s], 1)
  return own, face[own], b, (b[:, :, None] * pos[faces[face[own]]]).sum(1)


def _to_u8(x):
  return np.clip(np.floor(x + F32(0.5)), 0, 255).astype(np.uint8)


def bake(pos, faces, vertex_colors, rgbs, depths, masks, K, cam_in_obs, tex_size, top_n=4, depth_tol=0.005, cos_min=np.cos(np.deg2rad(75.0)),
         zfar=np.inf):
  """-> (texture (T,T,3) uint8, uv (3F,2) float32, used (T,T) int8)"""
  T = int(tex_size)
  pos, faces = np.asarray(pos, dtype=F32), np.asarray(faces, dtype=np.int64)
  n_faces = len(faces)
  face, ii, jj = owners(T, n_faces)
  c = cell(T, n_faces)
  tex = np.zeros((T, T, 3), dtype=np.uint8)
  used = np.full((T, T), -1, dtype=np.int8)
  own = face >= 0
  f, i, j = face[own], ii[own], jj[own]
  N = len(f)
  mf = F32(c - 3)
  with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
    b1, b2 = i.astype(F32) / mf, j.astype(F32) / mf
    b0 = (F32(1) - b1) - b2
    neg = b0 < 0
    s = b1 + b2
    b0, b1, b2 = np.where(neg, F32(0), b0), np.where(neg, b1 / s, b1), np.where(neg, b2 / s, b2)
    P = pos[faces[f]]                                     # (N,3 corners,3)
    p = [(b0 * P[:, 0, a] + b1 * P[:, 1, a]) + b2 * P[:, 2, a] for a in range(3)]
    e, h = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    n = [e[:, 1] * h[:, 2] - e[:, 2] * h[:, 1], e[:, 2] * h[:, 0] - e[:, 0] * h[:, 2], e[:, 0] * h[:, 1] - e[:, 1] * h[:, 0]]
    nl = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    n = [x / nl for x in n]
    tw = np.full((N, 4), -1, dtype=F32)
    tc = np.zeros((N, 4, 3), dtype=F32)
    cnt = np.zeros(N, dtype=np.int64)
    n_views = 0 if depths is None else len(depths)
    if n_views:
      depths = np.asarray(depths, dtype=F32)
      _, H, W = depths.shape
      Kd = np.asarray(K, dtype=np.float64)
      fx, fy, cx, cy = F32(Kd[0, 0]), F32(Kd[1, 1]), F32(Kd[0, 2]), F32(Kd[1, 2])
    for v in range(n_views):
      R, t = invert_view(cam_in_obs[v])
      q = [((R[a, 0] * p[0] + R[a, 1] * p[1]) + R[a, 2] * p[2]) + t[a] for a in range(3)]
      ok = q[2] >= F32(0.001)
      x, y = fx * (q[0] / q[2]) + cx, fy * (q[1] / q[2]) + cy
      x0, y0 = np.floor(x), np.floor(y)
      ok &= (x0 >= 0) & (x0 < F32(W - 1)) & (y0 >= 0) & (y0 < F32(H - 1))
      cn, rn = np.floor(x + F32(0.5)), np.floor(y + F32(0.5))
      xi, yi = np.where(ok, x0, 0).astype(np.int64), np.where(ok, y0, 0).astype(np.int64)
      ci, ri = np.where(ok, cn, 0).astype(np.int64), np.where(ok, rn, 0).astype(np.int64)
      d = depths[v][ri, ci]
      ok &= (d >= F32(0.001)) & (d < F32(zfar))
      if masks is not None:
        ok &= np.asarray(masks[v])[ri, ci] != 0
      ok &= np.abs(d - q[2]) <= F32(depth_tol)
      o = [-((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2]) for a in range(3)]
      w = [o[a] - p[a] for a in range(3)]
      wl = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
      cosang = ((n[0] * w[0] + n[1] * w[1]) + n[2] * w[2]) / wl
      ok &= cosang >= F32(cos_min)
      wx, wy = x - x0, y - y0
      img = np.asarray(rgbs[v])
      t00, t10, t01, t11 = (img[yi + dy, xi + dx].astype(F32) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)))
      ta, tb = t00 + wx[:, None] * (t10 - t00), t01 + wx[:, None] * (t11 - t01)
      smp = ta + wy[:, None] * (tb - ta)
      cnt = np.where(ok, np.minimum(cnt + 1, top_n), cnt)
      for sl in range(top_n - 1, -1, -1):
        shift = ok & (cosang > tw[:, sl - 1]) if sl > 0 else np.zeros(N, dtype=bool)
        place = ok & ~shift & (cosang > tw[:, sl])
        if sl > 0:
          tc[:, sl] = np.where(shift[:, None], tc[:, sl - 1], tc[:, sl])
          tw[:, sl] = np.where(shift, tw[:, sl - 1], tw[:, sl])
        tc[:, sl] = np.where(place[:, None], smp, tc[:, sl])
        tw[:, sl] = np.where(place, cosang, tw[:, sl])
    sw, sc = np.zeros(N, dtype=F32), np.zeros((N, 3), dtype=F32)
    for sl in range(4):
      take = sl < cnt
      sw = np.where(take, sw + tw[:, sl], sw)
      sc = np.where(take[:, None], sc + tw[:, sl, None] * tc[:, sl], sc)
    blend = sc / sw[:, None]
    if vertex_colors is not None:
      C = np.asarray(vertex_colors)[:, :3][faces[f]].astype(F32)
      fall = (b0[:, None] * C[:, 0] + b1[:, None] * C[:, 1]) + b2[:, None] * C[:, 2]
    else:
      fall = np.full((N, 3), 128, dtype=F32)
    assert blend.dtype == F32 and fall.dtype == F32 and all(a.dtype == F32 for a in p + n)
    tex[own] = _to_u8(np.where((cnt > 0)[:, None], blend, fall))
  used[own] = cnt.astype(np.int8)
  return tex, atlas_uv(T, n_faces), used
