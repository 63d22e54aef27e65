"""Device time of fp_mesh_components_count and fp_mesh_components_write on two meshes - the mesh fused from 16 rendered views of the
synthetic mustard bottle in a 256^3 volume (the case of scripts/bench_tsdf.py) and the composite mesh of the tests (22 365 vertices, 4
components) - with HIP events around the calls: after a warm-up the minimum and the median of --reps timed calls.  Beside each: the bytes
the call must move and the resulting GB/s next to the HBM peak (8 TB/s); the hooks are scattered 4-byte atomics that execute at the memory
side, so a small fraction of the peak here means the atomics and the launches, not the bytes, set the time.  In the same process and
interleaved with the device calls, the wall time of the host path they replace: device -> host copy of the mesh, reconstruct.
largest_component (scipy), the cumsum re-index, host -> device copy.  Then the wall time of a whole reconstruct_object(...,
max_vertices=8192) of the 16 views with the clean-up on the device and with the host path of the previous version (kept callable here
through largest_component).  Prints one JSON line.
usage: python scripts/bench_mesh_clean.py [--reps R] [--out profiles/bench_mesh_clean.json]"""
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
from foundationpose_amd import reconstruct as R
from foundationpose_amd import synthetic as S
from foundationpose_amd._lib import check, lib, ptr, stream_ptr
from foundationpose_amd.mesh_tensors import make_mesh_tensors
from scripts.bench_tsdf import DIM, H, N_VIEWS, W, look_at
from tests import mesh_simplify_oracle as M

HBM_PEAK_GBS = 8000.0


def count_bytes(V, F):
  """init writes the parents and the counts (12 a vertex); the hooks read the faces (12) and, per union, at least two parents and one
  compare-and-swap (2 x 12); flatten reads and writes a parent and writes a flag (16); three scans (reduce read, scan read and write) over
  V + 1, V + 1 and F + 1 words; the face count reads an index and a label (8); maximum and lowest label read a label and a count (2 x 8 a
  vertex); the flags read a label and a count and write a word (16 a vertex; 4 + 8 + 8 a face)."""
  return V * 12 + F * (12 + 24) + V * 16 + (2 * (V + 1) + (F + 1)) * 8 * 3 + F * 8 + V * 16 + V * 16 + F * 20


def write_bytes(V, F, nv, nf):
  """per vertex the label (4) and a scan pair (16), the map written (4); per kept vertex 27 bytes read and written; per face a scan pair (16);
  per kept face the face (12), three new ids (24), the output (12)."""
  return V * 24 + nv * 54 + F * 16 + nf * 48


def host_path(pos, nrm, col, faces, dev):
  """What reconstruct_object did between the extraction and the simplification: the mesh to the host, the largest component, the re-index,
  the mesh back to the device."""
  p, n, c, f = pos.cpu().numpy(), nrm.cpu().numpy(), col.cpu().numpy(), faces.cpu().numpy()
  keep = R.largest_component(f, len(p))
  if len(keep) and not keep.all():
    f = f[keep]
    used = np.zeros(len(p), dtype=bool)
    used[f.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    p, n, c, f = p[used], n[used], c[used], new_id[f].astype(np.int32)
  out = [torch.as_tensor(a, device=dev) for a in (p, n, c, f)]
  torch.cuda.synchronize()
  return out


def time_pair(ctx, dev, pos, nrm, col, faces, reps):
  V, F = len(pos), len(faces)
  counts = (ctypes.c_int64 * 4)()
  count = lambda: check(lib().fp_mesh_components_count(ctx.handle, ptr(faces), F, V, 1, 0.0, 1, counts, stream_ptr(dev)))
  count()
  C, kept, nv, nf = (int(c) for c in counts)
  o_pos, o_nrm = torch.empty((nv, 3), device=dev), torch.empty((nv, 3), device=dev)
  o_col, o_f = torch.empty((nv, 3), dtype=torch.uint8, device=dev), torch.empty((nf, 3), dtype=torch.int32, device=dev)
  vmap = torch.empty((V,), dtype=torch.int32, device=dev)
  write = lambda: check(lib().fp_mesh_components_write(ctx.handle, ptr(pos), ptr(nrm), ptr(col), V, ptr(faces), F, ptr(o_pos), ptr(o_nrm), ptr(o_col),
                                                       ptr(o_f), ptr(vmap), None, None, nv, nf, stream_ptr(dev)))
  ev = lambda: torch.cuda.Event(enable_timing=True)
  for _ in range(3):
    count(), write(), host_path(pos, nrm, col, faces, dev)
  torch.cuda.synchronize()
  t_count, t_write, t_host = [], [], []
  for _ in range(reps):                      # interleaved: device pair, then the host path, reps times
    e0, e1, e2 = ev(), ev(), ev()
    e0.record()
    count()
    e1.record()
    write()
    e2.record()
    torch.cuda.synchronize()
    t_count.append(e0.elapsed_time(e1)), t_write.append(e1.elapsed_time(e2))
    t0 = time.perf_counter()
    host = host_path(pos, nrm, col, faces, dev)
    t_host.append((time.perf_counter() - t0) * 1e3)
  same = all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(host, (o_pos, o_nrm, o_col, o_f))) if nf != F else None
  cb, wb = count_bytes(V, F), write_bytes(V, F, nv, nf)
  rate = lambda b, ms: dict(bytes=b, GBs=b / (ms * 1e-3) / 1e9, hbm_fraction=b / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS)
  stat = lambda t: dict(ms_min=float(np.min(t)), ms_median=float(np.median(t)))
  return dict(vertices_in=V, faces_in=F, components=C, kept_components=kept, vertices=nv, faces=nf, count=dict(**stat(t_count), **rate(cb, np.min(t_count))),
              write=dict(**stat(t_write), **rate(wb, np.min(t_write))), host_path=dict(**stat(t_host), pcie_bytes=(V * 27 + F * 12) + (nv * 27 + nf * 12)),
              host_equals_device=same)


def reconstruct_before(views, voxel, dev, max_vertices):
  """reconstruct_object as it was before the clean-up moved to the device: the same fusion, then the host tail."""
  eroded = R._eroded_depths(views, True, dev)
  depths = R._fusion_depths(eroded, True, dev)
  origin, dims = R.volume_from_views(depths, views.get('masks'), views['K'], views['cam_in_obs'], voxel, device=dev)
  vol = R.TsdfVolume(origin, voxel, dims, device=dev)
  vol.integrate(depths, views['K'], views['cam_in_obs'], rgbs=views.get('rgbs'), masks=views.get('masks'))
  return R._finish_on_host(*vol.extract_arrays(1), dev, max_vertices, None)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_mesh_clean needs an MI355X'
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
  vol = R.TsdfVolume(np.full(3, -0.1), vs, (DIM,) * 3, device=dev)
  vol.integrate(depth.contiguous(), K, cams, rgbs=rgb)
  pos, nrm, col, faces = vol.extract_arrays(1)
  del vol
  res = dict(reps=args.reps, hbm_peak_GBs=HBM_PEAK_GBS)
  res['fused'] = time_pair(ctx, dev, pos, nrm, col, faces, args.reps)
  t = lambda a: torch.as_tensor(a, device=dev).contiguous()
  cp, cf, cn, cc = M.composite_mesh()
  res['composite'] = time_pair(ctx, dev, t(cp), t(cn), t(cc), t(cf), args.reps)

  views = dict(depths=depth.contiguous(), rgbs=rgb, masks=(depth > 0).to(torch.uint8).contiguous(), K=K, cam_in_obs=cams)
  runs = dict(device=lambda: R.reconstruct_object(views, voxel_size=vs, max_vertices=8192, device=dev),
              host=lambda: reconstruct_before(views, vs, dev, 8192))
  wall = {k: [] for k in runs}
  meshes = {}
  for k, run in runs.items():                # warm-up
    meshes[k] = run()
  for _ in range(5):
    for k, run in runs.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      run()
      torch.cuda.synchronize()
      wall[k].append((time.perf_counter() - t0) * 1e3)
  a, b = meshes['device'], meshes['host']
  res['reconstruct_object_8192'] = dict(after_ms_min=float(np.min(wall['device'])), after_ms_median=float(np.median(wall['device'])),
                                        before_ms_min=float(np.min(wall['host'])), before_ms_median=float(np.median(wall['host'])),
                                        vertices=len(a.vertices), faces=len(a.faces),
                                        same_mesh=bool(a.vertices.tobytes() == b.vertices.tobytes() and a.faces.tobytes() == b.faces.tobytes()))
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
