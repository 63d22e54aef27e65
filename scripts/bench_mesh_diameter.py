"""Device time of fp_mesh_diameter (HIP events around the launches, points already on the device; after a warm-up, the minimum and the
median of --reps timed calls) beside the host time of compute_mesh_diameter in the same process: the 8 066-vertex mustard mesh (host:
every pair, n_sample=None), a 65 538-point and a 2^18-point cloud (host: the reference's 10 000-point random sample).  Prints one JSON
line.
usage: python scripts/bench_mesh_diameter.py [--reps R] [--out profiles/bench_mesh_diameter.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from foundationpose_amd import Utils as U
from foundationpose_amd import _lib, synthetic as S
from foundationpose_amd._lib import check, lib, ptr, stream_ptr


def device_ms(ctx, dev, pts, reps):
  out = torch.empty(1, device=dev)
  pair = torch.empty(2, dtype=torch.int32, device=dev)
  run = lambda: check(lib().fp_mesh_diameter(ctx.handle, ptr(pts), len(pts), ptr(out), ptr(pair), stream_ptr(dev)))
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
  return float(np.min(times)), float(np.median(times)), float(out.item())


def host_ms(pts, n_sample, reps):
  times = []
  for _ in range(reps):
    np.random.seed(0)
    t0 = time.perf_counter()
    d = U.compute_mesh_diameter(model_pts=pts, n_sample=n_sample)
    times.append((time.perf_counter() - t0) * 1e3)
  return float(np.min(times)), float(np.median(times)), d


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_mesh_diameter needs an MI355X'
  dev = torch.device('cuda', 0)
  ctx = _lib.Context.get(dev)
  cloud = lambda n: (np.random.RandomState(n).randn(n, 3) * np.array([0.11, 0.06, 0.03])).astype(np.float32)
  cases = [('mustard', np.asarray(S.make_mustard_mesh(seed=0).vertices, dtype=np.float32), None),
           ('cloud_65538', cloud(65538), 10000), ('cloud_2p18', cloud(1 << 18), 10000)]
  res = {}
  for name, pts, n_sample in cases:
    d_min, d_med, d = device_ms(ctx, dev, torch.as_tensor(pts, device=dev), args.reps)
    h_min, h_med, h = host_ms(pts.astype(np.float64), n_sample, max(args.reps // 10, 2))
    res[name] = dict(n=len(pts), device_ms_min=d_min, device_ms_median=d_med, diameter=d, pairs_per_s=len(pts) * (len(pts) - 1) / 2 / (d_min * 1e-3),
                     host_ms_min=h_min, host_ms_median=h_med, host_n_sample=n_sample, host_diameter=h)
  res['reps'] = args.reps
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
