"""Device time of fp_box_extents (HIP events around the three launches, points and frames already on the device; after a warm-up, the
minimum and the median of --reps timed calls) for the candidates of the 8 066-vertex mustard mesh, the rotated 0.05 x 0.12 x 0.2 m box
and one frame against 2^18 points; beside it, in the same process, the wall time of a whole Utils.oriented_bounds on the mustard mesh
with the hull and the frame building shown separately, and a float64 host path written here: per distinct hull normal the
minimum-area rectangle of the projected hull (every 2-D hull edge as the flush side), times the height.

An evaluation is one point projected on one frame: 9 products, 6 sums, 6 min / max = 21 fp32 vector operations per lane; the share of
the fp32 vector issue rate is evaluations/s x 21 over 256 CUs x 128 lanes/clock x 2.4 GHz = 7.86e13 lane-operations/s.  No counters
are taken.  Prints one JSON line.
usage: python scripts/bench_oriented_bounds.py [--reps R] [--out profiles/bench_oriented_bounds.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from foundationpose_amd import Utils as U
from foundationpose_amd import _lib, bounds as B, synthetic as S
from foundationpose_amd._lib import check, lib, ptr, stream_ptr

OPS_PER_EVAL = 21
ISSUE_RATE = 256 * 128 * 2.4e9      # fp32 vector lane-operations per second


def device_ms(ctx, dev, pts, frames, reps):
  idx = torch.empty(1, dtype=torch.int32, device=dev)
  rec = torch.empty(7, device=dev)
  n, C = len(pts), len(frames)
  run = lambda: check(lib().fp_box_extents(ctx.handle, ptr(pts), n, ptr(frames), C, ptr(idx), ptr(rec[:6]), ptr(rec[6:]), None, None, stream_ptr(dev)))
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
  return float(np.min(times)), float(np.median(times)), int(idx.item()), float(rec[6].item())


def host_calipers(pts):
  """float64: (volume, seconds) of the best box with one face flush with a hull face"""
  from scipy.spatial import ConvexHull
  t0 = time.perf_counter()
  hull = ConvexHull(pts)
  P = pts[hull.vertices]
  nrm = hull.equations[:, :3] / np.linalg.norm(hull.equations[:, :3], axis=1, keepdims=True)
  nrm = nrm[np.unique(np.round(nrm, 10), axis=0, return_index=True)[1]]
  best = np.inf
  for m in nrm:
    a = np.eye(3)[np.argmin(np.abs(m))]
    a = a - (a @ m) * m
    a /= np.linalg.norm(a)
    xy = np.stack([P @ a, P @ np.cross(m, a)], axis=1)
    H = xy[ConvexHull(xy).vertices]
    E = np.roll(H, -1, axis=0) - H
    E /= np.linalg.norm(E, axis=1, keepdims=True)
    area = np.ptp(H @ E.T, axis=0) * np.ptp(H @ np.stack([-E[:, 1], E[:, 0]], axis=1).T, axis=0)
    best = min(best, float(area.min()) * float(np.ptp(P @ m)))
  return best, time.perf_counter() - t0


def rotated_box():
  rv = np.array([0.3, -0.7, 0.5])
  t = np.linalg.norm(rv)
  k = rv / t
  K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
  R = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
  box = np.array([0.05, 0.12, 0.2])
  corners = np.array([[(-1, 1)[(i >> 2) & 1], (-1, 1)[(i >> 1) & 1], (-1, 1)[i & 1]] for i in range(8)], dtype=np.float64) * box / 2
  inside = (np.random.RandomState(0).rand(500, 3) - 0.5) * box * 0.98
  return np.concatenate([corners, inside]) @ R.T + np.array([0.4, -0.25, 0.9])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_oriented_bounds needs an MI355X'
  from scipy.spatial import ConvexHull
  dev = torch.device('cuda', 0)
  ctx = _lib.Context.get(dev)
  mustard = np.asarray(S.make_mustard_mesh(seed=0).vertices, dtype=np.float64)
  cm, cb = B.hull_candidates(mustard - (mustard.min(0) + mustard.max(0)) / 2), B.hull_candidates(rotated_box())
  cloud = (np.random.RandomState(18).randn(1 << 18, 3) * np.array([0.11, 0.06, 0.03])).astype(np.float32)
  cases = [('mustard', cm['points'], cm['frames']), ('rotated_box', cb['points'], cb['frames']), ('one_frame_2p18', cloud, np.eye(3)[None])]
  res = {}
  for name, pts, frames in cases:
    p, f = torch.as_tensor(pts, dtype=torch.float, device=dev).contiguous(), torch.as_tensor(frames, dtype=torch.float, device=dev).contiguous()
    d_min, d_med, winner, vol = device_ms(ctx, dev, p, f, args.reps)
    evals = len(p) * len(f)
    res[name] = dict(points=len(p), frames=len(f), device_ms_min=d_min, device_ms_median=d_med, winner=winner, volume_fp32=vol,
                     evals_per_s=evals / (d_min * 1e-3), share_of_fp32_issue_rate=evals * OPS_PER_EVAL / (d_min * 1e-3) / ISSUE_RATE,
                     bytes_read=12 * len(p) + 36 * len(f))
  # the whole call on the mustard mesh: wall clock, the read-back of the winner ends it
  whole = []
  for _ in range(3):
    t0 = time.perf_counter()
    to_origin, extents, info = U.oriented_bounds(mustard, return_info=True)
    whole.append(time.perf_counter() - t0)
  t0 = time.perf_counter()
  ConvexHull(mustard)
  t_hull = time.perf_counter() - t0
  t0 = time.perf_counter()
  B.hull_candidates(mustard)
  t_cand = time.perf_counter() - t0
  host_vol, host_s = host_calipers(mustard)
  res['oriented_bounds_mustard'] = dict(wall_s_min=float(np.min(whole)), wall_s_median=float(np.median(whole)), hull_s=t_hull,
                                        hull_and_frames_s=t_cand, volume=info['volume'], aabb_volume=info['aabb_volume'],
                                        pca_volume=info['pca_volume'], n_candidates=info['n_candidates'], hull_vertices=info['hull_vertices'],
                                        host_float64_calipers_s=host_s, host_float64_volume=host_vol)
  res['reps'] = args.reps
  res['counters'] = 'none taken'
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
