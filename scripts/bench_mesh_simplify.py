"""Device time of fp_mesh_simplify_count and fp_mesh_simplify_write on two meshes - the mesh fused from 16 rendered views of the synthetic
mustard bottle in a 256^3 volume (the case of scripts/bench_tsdf.py) at a cell of 2 voxels, and the composite mesh of the tests (22 365
vertices) at 3 mm - with HIP events around the calls: after a warm-up the minimum and the median of --reps timed calls.  Beside each: the
bytes the call must move and the resulting GB/s next to the HBM peak (8 TB/s); the table passes issue one to three atomics per vertex or
face, and those execute at the memory side, so a small fraction of the peak here means the atomics, not the bytes, set the time.  Then the
wall time of the whole Utils.simplify_mesh(max_vertices=8192) search on the fused mesh (20 counts and one write, uploads and read-back
included), and what it buys: one 252-hypothesis 160 x 160 fused render (fp_render_net, the path of scripts/bench_render.py) of the fused
mesh before and after.  Prints one JSON line.
usage: python scripts/bench_mesh_simplify.py [--reps R] [--out profiles/bench_mesh_simplify.json]"""
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
from foundationpose_amd import _lib
from foundationpose_amd import synthetic as S
from foundationpose_amd._lib import check, k_ptr, lib, ptr, stream_ptr
from foundationpose_amd.mesh_tensors import make_mesh_tensors
from foundationpose_amd.reconstruct import TsdfVolume
from scripts.bench_tsdf import DIM, H, N_VIEWS, W, look_at, timed
from tests import mesh_simplify_oracle as M

HBM_PEAK_GBS = 8000.0


def table_slots(n):
  cap = 1024
  while cap < 2 * n:
    cap <<= 1
  return cap


def count_bytes(V, F):
  """bounding box and insert read the positions; the tables are cleared (12 bytes a slot) and touched once per vertex (key, lowest member)
  plus the slot written; flags written, scanned (reduce read, scan read and write); ids resolved; the same for the faces, and the
  referenced flags cleared, set and scanned."""
  b = V * 12 * 2 + table_slots(V) * 12 + V * (8 + 4 + 4) + (V + 1) * 8 * 4 + V * (4 + 4 + 8 + 4)
  if F:
    b += table_slots(F) * 12 + (V + 1) * 8 + F * (12 + 12 + 8 + 4 + 4) + F * (4 + 4 + 12 + 12 + 8 + 24) + (F + 1) * 8 * 3 + (V + 1) * 8 * 3
  return b


def write_bytes(V, F, nv, nf):
  """sums cleared (80 bytes an output vertex); accumulate: attributes read (27), id and referenced pair read, 10 atomics of 8 or 4 bytes,
  the map written; vertex write: scan pair, sums, the output; face write: scan pair, face, three ids, three new ids, the output."""
  return nv * 80 + V * (27 + 4 + 16 + 7 * 8 + 3 * 4 + 4) + V * 16 + nv * (80 + 27) + F * 16 + nf * (12 + 12 + 24 + 12)


def time_pair(ctx, dev, pos, nrm, col, faces, cell, reps):
  V, F = len(pos), len(faces)
  counts = (ctypes.c_int64 * 2)()
  count = lambda: check(lib().fp_mesh_simplify_count(ctx.handle, ptr(pos), V, ptr(faces), F, cell, counts, stream_ptr(dev)))
  count()
  nv, nf = int(counts[0]), int(counts[1])
  o_pos, o_nrm = torch.empty((nv, 3), device=dev), torch.empty((nv, 3), device=dev)
  o_col, o_f = torch.empty((nv, 3), dtype=torch.uint8, device=dev), torch.empty((nf, 3), dtype=torch.int32, device=dev)
  vmap = torch.empty((V,), dtype=torch.int32, device=dev)
  write = lambda: check(lib().fp_mesh_simplify_write(ctx.handle, ptr(pos), ptr(nrm), ptr(col), V, ptr(faces), F, cell, ptr(o_pos), ptr(o_nrm), ptr(o_col),
                                                     ptr(o_f), ptr(vmap), nv, nf, stream_ptr(dev)))
  c_min, c_med = timed(count, reps)
  w_min, w_med = timed(write, reps)
  cb, wb = count_bytes(V, F), write_bytes(V, F, nv, nf)
  rate = lambda b, ms: dict(bytes=b, GBs=b / (ms * 1e-3) / 1e9, hbm_fraction=b / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS)
  return dict(vertices_in=V, faces_in=F, cell=float(cell), vertices=nv, faces=nf, count=dict(ms_min=c_min, ms_median=c_med, **rate(cb, c_min)),
              write=dict(ms_min=w_min, ms_median=w_med, **rate(wb, w_min)))


def render_us(ctx, dev, mesh, K, reps, n_hyp=252):
  mt = make_mesh_tensors(mesh, device=dev)
  dm = _lib.device_mesh(ctx, mt)
  ext = mesh.vertices.max(0) - mesh.vertices.min(0)
  diameter = float(np.linalg.norm(ext))
  rs = np.random.RandomState(0)
  poses = np.tile(np.eye(4, dtype=np.float32), (n_hyp, 1, 1))
  for p in poses:
    p[:3, :3] = S.random_rotation(rs)
    p[:3, 3] = (0.0, 0.0, 0.6)
  poses = torch.as_tensor(poses, device=dev).contiguous()
  Kd, Kp = k_ptr(K)
  tf, bbox = torch.empty((n_hyp, 3, 3), device=dev), torch.empty((n_hyp, 4), device=dev)
  net = torch.empty((n_hyp, 160, 160, 8), device=dev, dtype=torch.float16)
  check(lib().fp_crop_window_tf(ctx.handle, ptr(poses), n_hyp, Kp, 1.2, diameter, 160, 160, ptr(tf), ptr(bbox), stream_ptr(dev)))
  run = lambda: check(lib().fp_render_net(ctx.handle, dm.handle, ptr(poses), n_hyp, Kp, H, W, ptr(bbox), 160, 160, diameter, 1, 0.001, ptr(net),
                                          stream_ptr(dev)))
  t_min, t_med = timed(run, reps)
  return dict(vertices=len(mesh.vertices), faces=len(mesh.faces), us_min=t_min * 1e3, us_median=t_med * 1e3,
              covered=float((net[..., 5] != 0).float().mean()))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_mesh_simplify needs an MI355X'
  dev = torch.device('cuda', 0)
  ctx = _lib.Context.get(dev)
  src = S.make_mustard_mesh(seed=0)
  src.vertices = src.vertices - (src.vertices.min(0) + src.vertices.max(0)) / 2
  K = np.array([[800.0, 0, 319.5], [0, 800.0, 239.5], [0, 0, 1.0]])
  i = np.arange(N_VIEWS) + 0.5
  z = 1 - 2 * i / N_VIEWS
  phi = i * np.pi * (3 - np.sqrt(5))
  eyes = 0.6 * np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
  cams = np.stack([look_at(e) for e in eyes])
  color, depth, _ = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=np.linalg.inv(cams).astype(np.float32), mesh_tensors=make_mesh_tensors(src, device=dev))
  rgb = (color * 255).round().clamp(0, 255).to(torch.uint8).contiguous()
  vs = 0.2 / (DIM - 1)
  vol = TsdfVolume(np.full(3, -0.1), vs, (DIM,) * 3, device=dev)
  vol.integrate(depth.contiguous(), K, cams, rgbs=rgb)
  pos, nrm, col, faces = vol.extract_arrays(1)
  del vol
  res = dict(reps=args.reps, hbm_peak_GBs=HBM_PEAK_GBS)
  res['fused'] = time_pair(ctx, dev, pos, nrm, col, faces, float(np.float32(2 * vs)), args.reps)
  cp, cf, cn, cc = M.composite_mesh()
  t = lambda a: torch.as_tensor(a, device=dev).contiguous()
  res['composite'] = time_pair(ctx, dev, t(cp), t(cn), t(cc), t(cf), float(np.float32(0.003)), args.reps)

  fused = S.SimpleMesh(pos.cpu().numpy(), faces.cpu().numpy(), vertex_normals=nrm.cpu().numpy(),
                       vertex_colors=np.concatenate([col.cpu().numpy(), np.full((len(col), 1), 255, dtype=np.uint8)], 1))
  U.simplify_mesh((pos, faces, nrm, col), max_vertices=8192)                 # warm-up
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  small, info = U.simplify_mesh((pos, faces, nrm, col), max_vertices=8192)
  torch.cuda.synchronize()
  res['search_8192'] = dict(wall_ms=(time.perf_counter() - t0) * 1e3, **info)
  res['render_252x160x160'] = dict(before=render_us(ctx, dev, fused, K, args.reps), after=render_us(ctx, dev, small, K, args.reps))
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
