"""Device time of the masks-from-depth calls - fp_plane_score (512 hypotheses), fp_plane_moments, fp_depth_segment_count and
fp_depth_segment_write - with HIP events around the calls: after a warm-up the minimum and the median of --reps timed calls, at 640 x 480,
1920 x 1200 and a batch of 16 views of 640 x 480, on two scenes: a synthetic table top with 8 spheres, and the worst case of the
union-find, a frame that is ONE foreground component.  Beside each: the bytes the call must move and the resulting share of the HBM peak
(8 TB/s) - the plane score is arithmetic over registers and the hooks are scattered 4-byte atomics that execute at the memory side, so a
small share means that launches, atomics or arithmetic set the time, not bytes.  In the same process and interleaved with the device
calls, the wall time of the host path they replace, device -> host copy of the depth included: the numpy inlier count over the same
triplets (planes taken from the device) and scipy.sparse.csgraph.connected_components on the explicit pixel graph
(tests/segment_oracle.py builds it).  The host path runs --host-reps times (once above 640 x 480: it takes seconds).  Also checks
that the device's best hypothesis, component counts and labels equal the host's.  Prints one JSON line.
usage: python scripts/bench_segment.py [--reps R] [--host-reps R] [--out profiles/bench_segment.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy.sparse.csgraph import connected_components

from foundationpose_amd import _lib
from foundationpose_amd._lib import check, lib, ptr, stream_ptr
from tests import segment_oracle as O

HBM_PEAK_GBS = 8000.0
N_HYP = 512
RULE = dict(h_min=0.01, h_max=0.5, max_jump=0.01, min_pixels=200)
TOL = 0.005


def table_scene(H, W):
  """A table seen from 40 degrees above the horizon with 8 spheres on it, ray-cast in float64: (depth float32, K, plane)."""
  f = 0.9 * W
  K = np.array([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1.0]])
  a = np.deg2rad(40.0)
  n, p0 = np.array([0.0, -np.cos(a), -np.sin(a)]), np.array([0.0, 0.05, 0.9])
  dd = -float(n @ p0)
  e1, e2 = np.array([1.0, 0, 0]), np.array([0.0, -np.sin(a), np.cos(a)])
  col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
  ray = np.stack([(col - K[0, 2]) / f, (row - K[1, 2]) / f, np.ones_like(col)], -1)
  best = -dd / (ray @ n)
  rs = np.random.RandomState(0)
  for k in range(8):
    rad = rs.uniform(0.03, 0.06)
    c = p0 + (-0.35 + 0.1 * k) * e1 + (0.12 * (k % 2) - 0.06) * e2 + rad * n
    A, B, C = (ray * ray).sum(-1), ray @ c, c @ c - rad * rad
    disc = B * B - A * C
    with np.errstate(invalid='ignore'):
      ts = (B - np.sqrt(disc)) / A
    best = np.where((disc > 0) & (ts > 0) & (ts < best), ts, best)
  return best.astype(np.float32), K, np.array([n[0], n[1], n[2], dd])


def one_component_scene(H, W):
  """Every pixel half a metre above a fronto-parallel plane: one component of H W pixels."""
  f = 0.9 * W
  return np.full((H, W), 0.5, np.float32), np.array([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1.0]]), np.array([0.0, 0, -1, 1.0])


def host_plane_count(depth_dev, K, planes, tol):
  """The inlier counts of `planes` (n_hyp,4) over one view in numpy, from the device depth; the best index."""
  depth = depth_dev.cpu().numpy()
  x, y, z = (a.ravel() for a in O.points(depth, K))
  ok = O.ok_map(depth).ravel()
  x, y, z = x[ok], y[ok], z[ok]
  counts = np.zeros(len(planes), np.int64)
  for h, g in enumerate(planes):
    if g[0] != 0 or g[1] != 0 or g[2] != 0:
      counts[h] = int((np.abs(((g[0] * x + g[1] * y) + g[2] * z) + g[3]) < np.float32(tol)).sum())
  return counts, (int(np.argmax(counts)) if counts.max() > 0 else -1)


def host_components(depth_dev, K, plane):
  depth = depth_dev.cpu().numpy()
  fg = O.foreground(depth, K, plane, RULE['h_min'], RULE['h_max'])
  n, comp = connected_components(O.pixel_graph(depth, fg, RULE['max_jump']), directed=False)
  size = np.bincount(comp[fg.ravel()], minlength=n)
  return int((size > 0).sum()), int((size >= RULE['min_pixels']).sum())


def bench(ctx, dev, name, depth, K, plane, n_views, reps, host_reps):
  H, W = depth.shape
  N = n_views * H * W
  depths = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(depth, (n_views, H, W))), device=dev)
  Kd, Kp = _lib.k_ptr(K)
  planes = np.ascontiguousarray(np.tile(np.asarray(plane, dtype=np.float64), (n_views, 1)))
  trip = np.ascontiguousarray(np.tile(np.random.RandomState(0).randint(0, H * W, (1, N_HYP, 3)).astype(np.int32), (n_views, 1, 1)))
  hp, hc, hb = np.zeros((n_views, N_HYP, 4), np.float32), np.zeros((n_views, N_HYP), np.int32), np.zeros((n_views,), np.int32)
  sums, counts = np.zeros((n_views, 10)), np.zeros((n_views, 2), np.int32)
  labels = torch.empty((n_views, H, W), dtype=torch.int32, device=dev)
  st = stream_ptr(dev)
  score = lambda: check(lib().fp_plane_score(ctx.handle, ptr(depths), None, n_views, H, W, Kp, 100.0, ptr(trip), N_HYP, TOL, ptr(hp), ptr(hc), ptr(hb), st))
  moments = lambda: check(lib().fp_plane_moments(ctx.handle, ptr(depths), None, n_views, H, W, Kp, 100.0, ptr(planes), TOL, ptr(sums), st))
  count = lambda: check(lib().fp_depth_segment_count(ctx.handle, ptr(depths), None, n_views, H, W, Kp, 100.0, ptr(planes), RULE['h_min'], RULE['h_max'],
                                                     RULE['max_jump'], RULE['min_pixels'], ptr(counts), st))
  count()
  kept = int(counts[:, 1].sum())
  rows = torch.empty((max(kept, 1), _lib.FP_SEGMENT_STATS), dtype=torch.int64, device=dev)
  write = lambda: check(lib().fp_depth_segment_write(ctx.handle, ptr(depths), n_views, H, W, ptr(labels), ptr(rows) if kept else None, kept, st))
  calls = dict(plane_score=score, plane_moments=moments, segment_count=count, segment_write=write)
  for _ in range(3):
    for c in calls.values():
      c()
  torch.cuda.synchronize()
  ms = {k: [] for k in calls}
  host = dict(plane_count=[], components=[])
  ev = lambda: torch.cuda.Event(enable_timing=True)
  same = []
  for r in range(reps):                      # interleaved: the four device calls, then (the first host_reps times) the host path
    for k, c in calls.items():
      e0, e1 = ev(), ev()
      e0.record()
      c()
      e1.record()
      torch.cuda.synchronize()
      ms[k].append(e0.elapsed_time(e1))
    if r < host_reps:
      t0 = time.perf_counter()
      hcounts, hbest = host_plane_count(depths[0], K, hp[0], TOL)
      host['plane_count'].append((time.perf_counter() - t0) * 1e3 * n_views)      # the views are copies: one is timed, all are charged
      t0 = time.perf_counter()
      hcomp = host_components(depths[0], K, plane)
      host['components'].append((time.perf_counter() - t0) * 1e3 * n_views)
      same.append(bool(np.array_equal(hcounts, hc[0]) and hbest == hb[0] and hcomp == tuple(counts[0].tolist())))
  # bytes that must move: the score reads the depth once per chunk of 256 hypotheses and nothing else of size; the moments read it once;
  # the count reads the depth twice (init, hooks) and writes / reads parent (4), count (4) and the scan word (8) over init, hooks, flatten,
  # flags and the scan's three passes; the write reads depth, label, count and scan word and writes the label image
  need = dict(plane_score=N * 4 * (N_HYP // 256), plane_moments=N * 4, segment_count=N * (4 + 8 + 4 + 4 + 12 + 16 + 24), segment_write=N * (4 + 4 + 4 + 8 + 4))
  out = dict(scene=name, n_views=n_views, H=H, W=W, components=counts[0].tolist(), best=int(hb[0]), plane_tests=int(N) * N_HYP,
             host_equals_device=all(same) if same else None)
  for k in calls:
    t = float(np.min(ms[k]))
    out[k] = dict(ms_min=t, ms_median=float(np.median(ms[k])), bytes=int(need[k]), GBs=need[k] / (t * 1e-3) / 1e9,
                  hbm_fraction=need[k] / (t * 1e-3) / 1e9 / HBM_PEAK_GBS)
  out['plane_score']['plane_tests_per_s'] = N * N_HYP / (out['plane_score']['ms_min'] * 1e-3)
  out['host_path'] = {k: dict(ms_min=float(np.min(v)), ms_median=float(np.median(v)), reps=len(v)) for k, v in host.items() if v}
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--host-reps', type=int, default=3)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_segment needs an MI355X'
  dev = torch.device('cuda', 0)
  ctx = _lib.Context.get(dev)
  res = dict(reps=args.reps, hbm_peak_GBs=HBM_PEAK_GBS, n_hyp=N_HYP, tol=TOL, rule=RULE, labelling='union-find hooks in global memory, wave runs pre-joined',
             runs=[])
  for H, W, n_views in ((480, 640, 1), (1200, 1920, 1), (480, 640, 16)):
    for name, make in (('table_8_objects', table_scene), ('one_component', one_component_scene)):
      depth, K, plane = make(H, W)
      res['runs'].append(bench(ctx, dev, name, depth, K, plane, n_views, args.reps, args.host_reps if (H, n_views) == (480, 1) else 1))
  line = json.dumps(res)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
