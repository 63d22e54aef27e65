"""Device time of registering depth into another camera (fp_depth_reproject) with HIP events around the call: after a warm-up the minimum
and the median of --reps timed calls, for 640 x 480 -> 1280 x 720 and 848 x 480 -> 1920 x 1080 with one view (an RGB-D sensor's depth into
its colour camera) and 640 x 480 -> 640 x 480 with four views (a rig merged into one view), and for 8 x 8 -> 8 x 8: the fixed cost of the
memset node and the two launches.  Beside each case, interleaved call by call in the same process, what a user of torch has today:
the projection written in torch (rays precomputed outside the timed part) and scatter_reduce_('amin') of the CENTRE pixel only - it has
no footprint, so a magnified target is left with holes, and no winner index; it is the lower bound of a torch path, not an equivalent.
graph_ms is the memset and the two launches alone, without the host work of the Python call: the call captured into a graph, events
around its replay; node_ms is each node between the context's own events (mean of --reps calls; a node's figure includes its launch).  Beside each: the bytes that must move - the source read once, the key buffer filled, every atomic's 8 bytes, the keys read
back and the two outputs written - and the rates they amount to against the median graph_ms.  Every case runs in a child process of its own under
a time limit; the first one that fails ends the run.  Prints one JSON line.
usage: python scripts/bench_depth_reproject.py [--reps R] [--out profiles/bench_depth_reproject.json]"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

HBM_PEAK_GBS = 8000.0
# name, (Hs, Ws), (Hd, Wd), V
CASES = [('floor_8x8', (8, 8), (8, 8), 1), ('640x480_to_1280x720_v1', (480, 640), (720, 1280), 1), ('848x480_to_1920x1080_v1', (480, 848), (1080, 1920), 1),
         ('640x480_to_640x480_v4', (480, 640), (480, 640), 4)]
CASE_LIMIT_S = 150


def rodrigues(w):
  w = np.asarray(w, np.float64)
  a = np.linalg.norm(w)
  k = w / a
  Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
  return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def rig(src, dst, V):
  """V depth cameras of one size beside a target camera that sees the same field of view: each a few centimetres off and turned by 1.5 degrees."""
  (Hs, Ws), (Hd, Wd) = src, dst
  f = 0.9 * Ws
  Ks = [np.array([[f * (1 + 0.01 * s), 0, Ws / 2 - 0.5 + s], [0, f * (1 - 0.01 * s), Hs / 2 - 0.5 - s], [0, 0, 1]]) for s in range(V)]
  K_dst = np.array([[0.9 * Wd, 0, Wd / 2 - 0.5], [0, 0.9 * Wd, Hd / 2 - 0.5], [0, 0, 1]])
  Ts = []
  for s in range(V):
    T = np.eye(4)
    T[:3, :3] = rodrigues(np.deg2rad(1.5) * np.array([0.3 - 0.2 * s, 0.9, 0.1 * s]))
    T[:3, 3] = [0.05 - 0.03 * s, 0.004 * s, 0.002]
    Ts.append(T)
  return np.stack(Ks), np.stack(Ts), K_dst


def scene(V, Hs, Ws):
  """Smooth surfaces between 0.7 and 1.3 m with a step across the middle and 5 % missing pixels."""
  rng = np.random.default_rng(0)
  y, x = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing='ij')
  d = np.stack([1.0 + 0.2 * np.sin(x / (40.0 + 3 * s)) * np.cos(y / 30.0) + 0.1 * (x > Ws // 2) for s in range(V)]).astype(np.float32)
  d[rng.random(d.shape) < 0.05] = 0
  return d


def time_interleaved(calls, reps):
  """[ms list per call]: the calls take turns, each timed with its own pair of events."""
  import torch
  for _ in range(3):
    for c in calls:
      c()
  torch.cuda.synchronize()
  ms = [[] for _ in calls]
  for _ in range(reps):
    for i, c in enumerate(calls):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      c()
      e1.record()
      torch.cuda.synchronize()
      ms[i].append(e0.elapsed_time(e1))
  return ms


def run_case(name, reps):
  import torch
  from foundationpose_amd import Utils as U
  from foundationpose_amd import _lib
  _, src, dst, V = next(c for c in CASES if c[0] == name)
  (Hs, Ws), (Hd, Wd) = src, dst
  dev = torch.device('cuda', 0)
  Ks, Ts, K_dst = rig(src, dst, V)
  depth = torch.as_tensor(scene(V, Hs, Ws), device=dev)
  ours = lambda: U.reproject_depth(depth, Ks, Ts, K_dst, dst, return_source=True)

  # the torch path: fp32, the rays of every view precomputed
  row, col = torch.meshgrid(torch.arange(Hs, device=dev, dtype=torch.float32), torch.arange(Ws, device=dev, dtype=torch.float32), indexing='ij')
  rays = [torch.stack([(col - float(K[0, 2])) / float(K[0, 0]), (row - float(K[1, 2])) / float(K[1, 1]), torch.ones_like(col)], -1).reshape(-1, 3) for K in Ks]
  Rt = [(torch.as_tensor(T[:3, :3].T.copy(), device=dev, dtype=torch.float32), torch.as_tensor(T[:3, 3].copy(), device=dev, dtype=torch.float32)) for T in Ts]
  fx, fy, cx, cy = (float(K_dst[0, 0]), float(K_dst[1, 1]), float(K_dst[0, 2]), float(K_dst[1, 2]))

  def torch_path():
    out = torch.full((Hd * Wd,), float('inf'), device=dev)
    for s in range(V):
      d = depth[s].reshape(-1)
      q = (rays[s] * d[:, None]) @ Rt[s][0] + Rt[s][1]
      z = q[:, 2]
      u, v = torch.floor(fx * (q[:, 0] / z) + cx + 0.5), torch.floor(fy * (q[:, 1] / z) + cy + 0.5)
      ok = (d >= 0.001) & (z >= 0.001) & (u >= 0) & (u <= Wd - 1) & (v >= 0) & (v <= Hd - 1)
      idx = (v * Wd + u)[ok].long()
      out.scatter_reduce_(0, idx, z[ok], 'amin')
    return torch.where(torch.isinf(out), torch.zeros_like(out), out).reshape(Hd, Wd)

  ms_ours, ms_torch = time_interleaved([ours, torch_path], reps)
  # the three nodes alone, without the host work of the Python call: the call captured into a graph, events around its replay
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    ours()
  ms_graph = time_interleaved([graph.replay], reps)[0]
  kernel_ms = float(np.median(ms_graph))
  ctx = _lib.Context.get(dev)      # each node between the context's own events (which put gaps of their own between the nodes)
  ctx.prof_enable(True)
  ctx.prof_reset()
  for _ in range(reps):
    ours()
  torch.cuda.synchronize()
  node_ms = {k: ctx.prof_read('reproject_' + k)['total_ms'] / reps for k in ('fill', 'scatter', 'finalise')}
  ctx.prof_enable(False)
  got, source = ours()
  ref = torch_path()
  filled, ref_filled = got > 0, ref > 0
  # the atomics of a call: the winners' footprints cannot be counted from the output, so the range rule is evaluated once more in torch
  # fp32 (the kernel's order of operations; a pixel on a rounding boundary may count differently, which moves the figure by a few in a million)
  atomics = 0
  for s in range(V):
    d = depth[s].reshape(-1)
    K = Ks[s]
    pts = []
    for off in (0.0, -0.5, 0.5):
      ray = torch.stack([(col + off - float(K[0, 2])) / float(K[0, 0]), (row + off - float(K[1, 2])) / float(K[1, 1]), torch.ones_like(col)], -1).reshape(-1, 3)
      q = (ray * d[:, None]) @ Rt[s][0] + Rt[s][1]
      pts.append((fx * (q[:, 0] / q[:, 2]) + cx, fy * (q[:, 1] / q[:, 2]) + cy, q[:, 2]))
    (uc, vc, z), (u0, v0, z0), (u1, v1, z1) = pts
    ok = (d >= 0.001) & (z >= 0.001) & (z0 > 0) & (z1 > 0)
    rng_ = lambda e0, e1, c: (torch.minimum(torch.ceil(torch.minimum(e0, e1)), torch.floor(c + 0.5)), torch.maximum(torch.ceil(torch.maximum(e0, e1)) - 1, torch.floor(c + 0.5)))
    (xl, xh), (yl, yh) = rng_(u0, u1, uc), rng_(v0, v1, vc)
    cap = ((xh - xl) + 1 > 8) | ((yh - yl) + 1 > 8)
    pcx, pcy = torch.floor(uc + 0.5), torch.floor(vc + 0.5)
    xl, xh, yl, yh = torch.where(cap, pcx, xl), torch.where(cap, pcx, xh), torch.where(cap, pcy, yl), torch.where(cap, pcy, yh)
    nx = (torch.clamp(xh, max=Wd - 1) - torch.clamp(xl, min=0) + 1).clamp(min=0)
    ny = (torch.clamp(yh, max=Hd - 1) - torch.clamp(yl, min=0) + 1).clamp(min=0)
    atomics += int((nx * ny)[ok].sum().item())
  need = dict(source_read=V * Hs * Ws * 4, key_fill=Hd * Wd * 8, atomics=atomics * 8, key_read=Hd * Wd * 8, outputs=Hd * Wd * 8)
  total = sum(need.values())
  return dict(case=name, src=[Hs, Ws], dst=[Hd, Wd], views=V, nodes=3, reps=reps, ms_min=float(np.min(ms_ours)), ms_median=float(np.median(ms_ours)),
              graph_ms_min=float(np.min(ms_graph)), graph_ms_median=kernel_ms, node_ms=node_ms, torch_centre_only_ms_min=float(np.min(ms_torch)), torch_centre_only_ms_median=float(np.median(ms_torch)),
              bytes=need, bytes_total=total, GBs=total / (kernel_ms * 1e-3) / 1e9, hbm_fraction=total / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
              atomics=atomics, atomics_per_us=atomics / (kernel_ms * 1e3), filled_fraction=float(filled.float().mean()),
              torch_filled_fraction=float(ref_filled.float().mean()),
              max_abs_difference_where_both_filled=float((got - ref).abs()[filled & ref_filled].max()) if (filled & ref_filled).any() else None)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  ap.add_argument('--case', default=None, help='run this one case in this process and print its JSON (what the driver starts)')
  args = ap.parse_args()
  if args.case:
    print('RESULT ' + json.dumps(run_case(args.case, args.reps)))
    return
  res = dict(reps=args.reps, hbm_peak_GBs=HBM_PEAK_GBS,
             kernel_form='a memset node, a scatter launch (one thread a source pixel, 64-bit atomicMin without a return value) and a finalise launch', runs=[])
  for name in [c[0] for c in CASES]:
    # a fresh process per case, under its own time limit; a case that fails or hangs ends the run: nothing more is started on the device
    try:
      p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', name, '--reps', str(args.reps)], capture_output=True, text=True,
                         timeout=CASE_LIMIT_S)
      status, text = p.returncode, p.stdout[-2000:] + p.stderr[-4000:]
      line = next((l for l in p.stdout.splitlines() if l.startswith('RESULT ')), None)
    except subprocess.TimeoutExpired:
      status, text, line = 124, f'no result within {CASE_LIMIT_S} s', None
    if status != 0 or line is None:
      sys.stderr.write(text + '\n')
      res['stopped_at'] = dict(case=name, exit_status=status)
      break
    res['runs'].append(json.loads(line[7:]))
  line = json.dumps(res)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(line + '\n')
  if 'stopped_at' in res:
    raise SystemExit(f"bench_depth_reproject: case {res['stopped_at']['case']} failed; nothing was started after it")


if __name__ == '__main__':
  main()
