"""Device time of fp_point_mesh_distance - brute force, every point against every triangle - with HIP events around the call: after a
warm-up the minimum and the median of --reps timed calls, and the point-triangle tests per second that makes.  Three cases:
  fused_to_simplified   the vertices of the mesh fused from 16 rendered views of the synthetic mustard bottle in a 256^3 volume (the case of
                        scripts/bench_tsdf.py) against its Utils.simplify_mesh(max_vertices=8192) simplification
  simplified_to_fused   100 000 surface samples of the simplification against the fused mesh's faces
  icosphere_80          4096 points against the 80-face icosphere of the tests (launch-bound)
Beside each, interleaved in the same process, the host path it replaces (tests/tsdf_oracle.py fraction_beyond_bound): 400 000 random
samples of the target surface and a scipy cKDTree query - an upper bound of the distance, not the distance; its largest excess over the
exact distance is reported.  `valu_per_pair` is the count of vector instructions per pair in surfdist_kernel's inner loop (from the
disassembly: the per-record loop body divided by the 4 queries a lane holds); with it the achieved rate is set against the fp32 vector
issue peak (256 CUs x 4 SIMD-32 x 2.4 GHz lane-instructions per second; an FMA counts 2 FLOP in the 157 TFLOP/s figure).
Then Utils.mesh_distance(fused, simplified): the Chamfer, Hausdorff and F-score numbers that max_vertices=8192 costs, and its wall time.
Prints one JSON line.
usage: python scripts/bench_mesh_distance.py [--reps R] [--valu-per-pair 100] [--out profiles/bench_mesh_distance.json]"""
import argparse
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
from foundationpose_amd._lib import check, lib, ptr, stream_ptr
from foundationpose_amd.mesh_tensors import make_mesh_tensors
from foundationpose_amd.reconstruct import TsdfVolume
from scripts.bench_tsdf import DIM, H, N_VIEWS, W, look_at, timed
from tests import surface_distance_oracle as SO
from tests import tsdf_oracle as TO

LANE_INSTR_PEAK = 256 * 4 * 32 * 2.4e9      # fp32 vector lane-instructions per second: 157 TFLOP/s at 2 FLOP per FMA


def fused_mesh(dev):
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
  vol = TsdfVolume(np.full(3, -0.1), 0.2 / (DIM - 1), (DIM,) * 3, device=dev)
  vol.integrate(depth.contiguous(), K, cams, rgbs=rgb)
  return vol.extract_arrays(1)


def case(ctx, dev, pts, pos, faces, reps, host_reps, valu_per_pair):
  n, V, F = len(pts), len(pos), len(faces)
  dist, face = torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
  run = lambda: check(lib().fp_point_mesh_distance(ctx.handle, ptr(pts), n, ptr(pos), V, ptr(faces), F, ptr(dist), ptr(face), None, stream_ptr(dev)))
  p_h, v_h, f_h = pts.cpu().numpy().astype(np.float64), pos.cpu().numpy(), faces.cpu().numpy()
  from scipy.spatial import cKDTree
  dev_ms, host_ms, nn = [], [], None
  for _ in range(host_reps):                 # interleaved: device, host, device, host, ..
    dev_ms.append(timed(run, max(1, reps // host_reps)))
    t0 = time.perf_counter()
    nn, _ = cKDTree(TO.surface_samples(v_h, f_h)).query(p_h)
    host_ms.append((time.perf_counter() - t0) * 1e3)
  ms_min, ms_med = min(m[0] for m in dev_ms), float(np.median([m[1] for m in dev_ms]))
  pairs = float(n) * F
  d = dist.cpu().numpy().astype(np.float64)
  out = dict(points=n, faces=F, pairs=pairs, ms_min=ms_min, ms_median=ms_med, pairs_per_s=pairs / (ms_min * 1e-3),
             host_samples=400000, host_ms_min=float(np.min(host_ms)), host_ms_median=float(np.median(host_ms)),
             host_excess_max=float((nn - d).max()), host_excess_mean=float((nn - d).mean()), host_below_exact=int((nn < d - 1e-6 * max(d.max(), 1e-9)).sum()),
             dist_mean=float(d.mean()), dist_max=float(d.max()))
  if valu_per_pair:
    out.update(valu_per_pair=valu_per_pair, vector_issue_fraction=out['pairs_per_s'] * valu_per_pair / LANE_INSTR_PEAK)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--host-reps', type=int, default=2)
  ap.add_argument('--valu-per-pair', type=float, default=100.0)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_mesh_distance needs an MI355X'
  dev = torch.device('cuda', 0)
  ctx = _lib.Context.get(dev)
  pos, nrm, col, faces = fused_mesh(dev)
  small, info = U.simplify_mesh((pos, faces, nrm, col), max_vertices=8192)
  s_pos, s_faces = torch.as_tensor(small.vertices, dtype=torch.float, device=dev), torch.as_tensor(small.faces, dtype=torch.int32, device=dev)
  res = dict(reps=args.reps, lane_instr_peak=LANE_INSTR_PEAK, tile=_lib.FP_SURFDIST_TILE, chunk=_lib.FP_SURFDIST_CHUNK,
             fused=dict(vertices=len(pos), faces=len(faces)), simplified=dict(vertices=len(s_pos), faces=len(s_faces), cell=info['cell']))
  res['fused_to_simplified'] = case(ctx, dev, pos, s_pos, s_faces, args.reps, args.host_reps, args.valu_per_pair)
  samples = U.sample_surface((s_pos, s_faces), 100_000, seed=0)
  res['simplified_to_fused'] = case(ctx, dev, samples, pos, faces, args.reps, args.host_reps, args.valu_per_pair)
  iv, jf = SO.icosphere(1, radius=0.05)
  q = torch.as_tensor(np.random.default_rng(0).uniform(-0.08, 0.08, (4096, 3)).astype(np.float32), device=dev)
  res['icosphere_80'] = case(ctx, dev, q, torch.as_tensor(iv, device=dev), torch.as_tensor(jf, device=dev), args.reps, args.host_reps, args.valu_per_pair)
  U.mesh_distance((pos, faces), (s_pos, s_faces), n_samples=100_000)        # warm-up
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  md = U.mesh_distance((pos, faces), (s_pos, s_faces), n_samples=100_000)
  res['mesh_distance_fused_vs_simplified'] = dict(wall_ms=(time.perf_counter() - t0) * 1e3, n_samples=100_000, **md)
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
