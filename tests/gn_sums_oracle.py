"""The 29 Gauss-Newton sums of one item (a view of fp_tsdf_align, a pair of fp_depth_pairs_align, either half of a pair of
fp_depth_pairs_align_photo) in the device's summation order, from the rows the device wrote.  The order is stated in
foundationpose_amd/csrc/gn_sums.h; this is its restatement in numpy, and the GPU tests compare the device's sums with it bit for bit."""
import numpy as np

TERMS = 29


def device_sums(rows, threads=256, pix=4):
  """rows: the (H, W, 8) or (n, 8) float32 of one item in d_rows (J0 .. J5, r, valid); for the photometric half pass floats 8 .. 15.
  threads, pix: the kernel's workgroup size and pixels per lane.  Returns the 29 float64 sums."""
  rows = np.asarray(rows)
  assert rows.dtype == np.float32 and rows.shape[-1] == 8
  rows = rows.reshape(-1, 8)
  tile = threads * pix
  n_tiles = -(-len(rows) // tile)
  # 1. zero rows up to whole tiles; pixel tile * 1024 + q * 256 + tid belongs to lane tid
  x = np.zeros((n_tiles * tile, 8), dtype=np.float32)
  x[:len(rows)] = rows
  x = x.astype(np.float64).reshape(n_tiles, pix, threads, 8)
  J, r = x[..., :6], x[..., 6]
  terms = [J[..., i] * J[..., j] for i in range(6) for j in range(i, 6)] + [J[..., i] * r for i in range(6)] + [r * r, np.where(x[..., 7] != 0, 1.0, 0.0)]
  terms = np.stack(terms, -1)                                      # (tile, q, lane, 29): products of widened fp32 values, no contraction
  # 2. a lane starts at +0.0 and adds q = 0 .. pix - 1 in order
  v = np.zeros((n_tiles, threads, TERMS))
  for q in range(pix):
    v = v + terms[:, q]
  # 3. the butterfly over each wave of 64: partner distance 32, 16, .. 1; every lane ends equal
  v = v.reshape(n_tiles, threads // 64, 64, TERMS)
  lane = np.arange(64)
  for o in (32, 16, 8, 4, 2, 1):
    v = v + v[:, :, lane ^ o]
  assert (v == v[:, :, :1]).all()
  red = v[:, :, 0]
  # 4. the waves, left to right
  slot = red[:, 0]
  for w in range(1, threads // 64):
    slot = slot + red[:, w]
  # 5. the tiles from 0.0 in tile order
  s = np.zeros(TERMS)
  for k in range(n_tiles):
    s = s + slot[k]
  return s
