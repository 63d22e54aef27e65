"""Device time of fp_tsdf_integrate (16 views of 640 x 480 into 256^3 points) and of fp_tsdf_extract_count + fp_tsdf_extract_write on the
same volume, filled from rendered views of the synthetic mustard mesh: HIP events around the calls, after a warm-up the minimum and the
median of --reps timed calls.  Beside each: the bytes the call must move (integrate: the six planes read and written once, the depth and
colour images once; extraction: tsdf and weight read, the 8-byte count word and the mask byte written, the scan's read-modify-write, and
the mesh) and the resulting GB/s next to the HBM peak of the MI355X (8 TB/s).  A numpy float32 restatement of the integration at 64^3 and
4 views in the same process gives the scale of a host implementation.  Prints one JSON line.
usage: python scripts/bench_tsdf.py [--reps R] [--out profiles/bench_tsdf.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from foundationpose_amd import Utils as U
from foundationpose_amd import synthetic as S
from foundationpose_amd._lib import check, lib, ptr, stream_ptr
from foundationpose_amd.mesh_tensors import make_mesh_tensors
from foundationpose_amd.reconstruct import TsdfVolume

HBM_PEAK_GBS = 8000.0
H, W, N_VIEWS, DIM = 480, 640, 16, 256


def look_at(eye):
  z = -eye / np.linalg.norm(eye)
  up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.99 else np.array([0.0, 1.0, 0.0])
  x = np.cross(z, up)
  x /= np.linalg.norm(x)
  m = np.eye(4)
  m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, eye
  return m


def timed(run, reps):
  for _ in range(3):
    run()
  torch.cuda.synchronize()
  times = []
  for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1))
  return float(np.min(times)), float(np.median(times))


def host_integrate_ms(origin, vs, dim, depths, K, poses):
  """numpy float32, the same rule (no colours), one pass over the views"""
  F = np.float32
  g = [F(origin[a]) + F(vs) * np.arange(dim, dtype=F) for a in range(3)]
  sx, sy, sz = g[0][None, None, :], g[1][None, :, None], g[2][:, None, None]
  T, Wt = np.zeros((dim,) * 3, F), np.zeros((dim,) * 3, F)
  trunc = F(4 * vs)
  t0 = time.perf_counter()
  with np.errstate(all='ignore'):
    for v in range(len(depths)):
      m = np.linalg.inv(poses[v]).astype(F)
      q = [((m[a, 0] * sx + m[a, 1] * sy) + m[a, 2] * sz) + m[a, 3] for a in range(3)]
      col = np.floor((F(K[0, 0]) * (q[0] / q[2]) + F(K[0, 2])) + F(0.5))
      row = np.floor((F(K[1, 1]) * (q[1] / q[2]) + F(K[1, 2])) + F(0.5))
      ok = (q[2] >= F(0.001)) & (col >= 0) & (col < W) & (row >= 0) & (row < H)
      d = depths[v][np.where(ok, row, 0).astype(np.int64), np.where(ok, col, 0).astype(np.int64)]
      sdf = d - q[2]
      ok &= (d >= F(0.001)) & ~(sdf < -trunc)
      T = np.where(ok, (T * Wt + np.minimum(F(1), sdf / trunc)) / (Wt + F(1)), T)
      Wt = np.where(ok, Wt + F(1), Wt)
  return (time.perf_counter() - t0) * 1e3


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_tsdf needs an MI355X'
  dev = torch.device('cuda', 0)
  mesh = S.make_mustard_mesh(seed=0)
  mesh.vertices = mesh.vertices - (mesh.vertices.min(0) + mesh.vertices.max(0)) / 2
  mt = make_mesh_tensors(mesh, device=dev)
  K = np.array([[800.0, 0, 319.5], [0, 800.0, 239.5], [0, 0, 1.0]])
  i = np.arange(N_VIEWS) + 0.5
  z = 1 - 2 * i / N_VIEWS
  phi = i * np.pi * (3 - np.sqrt(5))
  eyes = 0.6 * np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
  cams = np.stack([look_at(e) for e in eyes])
  color, depth, _ = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=np.linalg.inv(cams).astype(np.float32), mesh_tensors=mt)
  rgb = (color * 255).round().clamp(0, 255).to(torch.uint8).contiguous()
  depth = depth.contiguous()
  vs = 0.2 / (DIM - 1)
  origin = np.full(3, -0.1)
  vol = TsdfVolume(origin, vs, (DIM,) * 3, device=dev)
  n = DIM ** 3
  res = dict(reps=args.reps, hbm_peak_GBs=HBM_PEAK_GBS, dims=[DIM] * 3, views=N_VIEWS, image=[H, W])

  t_min, t_med = timed(lambda: vol.integrate(depth, K, cams, rgbs=rgb), args.reps)
  nbytes = n * 6 * 4 * 2 + N_VIEWS * H * W * (4 + 3)
  res['integrate'] = dict(ms_min=t_min, ms_median=t_med, bytes=nbytes, GBs=nbytes / (t_min * 1e-3) / 1e9, hbm_fraction=nbytes / (t_min * 1e-3) / 1e9 / HBM_PEAK_GBS)

  vol.reset()
  vol.integrate(depth, K, cams, rgbs=rgb)
  counts = (ctypes.c_int64 * 2)()
  count = lambda: check(lib().fp_tsdf_extract_count(vol.ctx.handle, vol.handle, 1.0, counts, stream_ptr(dev)))
  count()
  nv, nf = int(counts[0]), int(counts[1])
  bv, bn = torch.empty((nv, 3), device=dev), torch.empty((nv, 3), device=dev)
  bc, bf = torch.empty((nv, 3), dtype=torch.uint8, device=dev), torch.empty((nf, 3), dtype=torch.int32, device=dev)
  write = lambda: check(lib().fp_tsdf_extract_write(vol.ctx.handle, vol.handle, ptr(bv), ptr(bn), ptr(bc), ptr(bf), nv, nf, stream_ptr(dev)))
  c_min, c_med = timed(count, args.reps)
  w_min, w_med = timed(write, args.reps)
  c_bytes = n * (4 + 4 + 8 + 1) + n * 8 * 3                    # count pass; scan: reduce reads, scan reads and writes
  w_bytes = n * (1 + 16 + 1) + nv * 27 + nf * 12                # mask per point (vertex pass), base pair + mask (face pass), the mesh
  res['extract_count'] = dict(ms_min=c_min, ms_median=c_med, bytes=c_bytes, GBs=c_bytes / (c_min * 1e-3) / 1e9, hbm_fraction=c_bytes / (c_min * 1e-3) / 1e9 / HBM_PEAK_GBS)
  res['extract_write'] = dict(ms_min=w_min, ms_median=w_med, bytes=w_bytes, GBs=w_bytes / (w_min * 1e-3) / 1e9, hbm_fraction=w_bytes / (w_min * 1e-3) / 1e9 / HBM_PEAK_GBS,
                              vertices=nv, faces=nf)
  hd = 64
  res['host_numpy_integrate_64'] = dict(dims=[hd] * 3, views=4, ms=host_integrate_ms(origin, 0.2 / (hd - 1), hd, depth[:4].cpu().numpy(), K, cams[:4]))
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
