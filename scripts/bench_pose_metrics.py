"""Device time of fp_pose_errors (HIP events around the launches, inputs already on the device): ADD-S and ADD of 252 poses on the
mustard mesh (96 x 84 grid, 8 066 vertices), and ADD-S of 16 poses on a 65 538-point mesh.  Prints one JSON line; pairs_per_s counts
the B x N x N point pairs of ADD-S.
usage: python scripts/bench_pose_metrics.py [--reps R]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from foundationpose_amd import _lib, synthetic as S
from foundationpose_amd._lib import check, lib, ptr, stream_ptr


def case(dev, n_theta, n_z, B, seed):
  mesh = S.make_mustard_mesh(seed=seed, n_theta=n_theta, n_z=n_z)
  pts = mesh.vertices - (mesh.vertices.min(0) + mesh.vertices.max(0)) / 2
  rs = np.random.RandomState(seed)
  gt = np.eye(4)
  gt[:3, :3] = S.random_rotation(rs)
  gt[:3, 3] = (0.02, -0.03, 0.75)
  poses = np.repeat(np.eye(4)[None], B, 0)
  for p in poses:
    p[:3, :3] = S.random_rotation(rs)
    p[:3, 3] = gt[:3, 3] + rs.randn(3) * 0.01
  t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float, device=dev)
  return t(pts), t(poses), t(gt)


def time_ms(ctx, dev, pts, poses, gt, which, reps):
  B = len(poses)
  out = torch.empty((3, B), device=dev)
  run = lambda: check(lib().fp_pose_errors(ctx.handle, ptr(pts), len(pts), ptr(poses), ptr(gt), 0, B, None, 0, which, ptr(out[0]),
                                           ptr(out[1]), None, stream_ptr(dev)))
  for _ in range(3):
    run()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(reps):
    run()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / reps


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_pose_metrics needs an MI355X'
  dev = torch.device('cuda', 0)
  ctx = _lib.Context.get(dev)
  res = {}
  pts, poses, gt = case(dev, 96, 84, 252, 0)
  res['mustard_B252_N'] = len(pts)
  res['mustard_B252_adds_ms'] = time_ms(ctx, dev, pts, poses, gt, _lib.FP_ERR_ADDS, args.reps)
  res['mustard_B252_add_ms'] = time_ms(ctx, dev, pts, poses, gt, _lib.FP_ERR_ADD, args.reps)
  res['mustard_B252_adds_pairs_per_s'] = len(poses) * len(pts) ** 2 / (res['mustard_B252_adds_ms'] * 1e-3)
  pts, poses, gt = case(dev, 256, 256, 16, 1)
  res['large_B16_N'] = len(pts)
  res['large_B16_adds_ms'] = time_ms(ctx, dev, pts, poses, gt, _lib.FP_ERR_ADDS, max(args.reps // 4, 3))
  res['large_B16_adds_pairs_per_s'] = len(poses) * len(pts) ** 2 / (res['large_B16_adds_ms'] * 1e-3)
  res['reps'] = args.reps
  print(json.dumps(res))


if __name__ == '__main__':
  main()
