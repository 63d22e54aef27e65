"""Device time of the warp through a camera model (fp_remap) with HIP events around the call: after a warm-up the minimum and the median
of --reps timed calls, for a stereo pair (two plans, one launch) at 640 x 480 and 1920 x 1200, grey and RGB, and for one depth map at
640 x 480.  Beside each case, interleaved call by call in the same process, the path a user of torch has today:
torch.nn.functional.grid_sample on a PRECOMPUTED grid (the map of this library's own debug output, normalised once outside the timed
part), with the uint8 -> float -> uint8 conversions and the layout change that it needs included (depth: mode='nearest', no conversions).
kernel_ms is the launch alone between the context's own events (mean of --reps calls), without the host work of the Python call, and
the rates are formed with it.  Beside each: the bytes the call must move (every source and destination byte once) and the share of the
HBM peak (8 TB/s) they amount to.  Also: the cost of stereo_depth(rectify=rect) over stereo_depth on an already rectified pair of the same size.
Every case runs in a child process of its own under a time limit; the first one that fails ends the run.  Prints one JSON line.
usage: python scripts/bench_rectify.py [--reps R] [--out profiles/bench_rectify.json]"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

HBM_PEAK_GBS = 8000.0
CASES = [('pair_640x480_grey', 480, 640, 1, 'colour'), ('pair_640x480_rgb', 480, 640, 3, 'colour'), ('pair_1920x1200_grey', 1200, 1920, 1, 'colour'),
         ('pair_1920x1200_rgb', 1200, 1920, 3, 'colour'), ('depth_640x480', 480, 640, 1, 'depth')]
STEREO_CASES = [('stereo_depth_640x480_d128', 480, 640, 128), ('stereo_depth_1920x1200_d128', 1200, 1920, 128)]
CASE_LIMIT_S = 150


def calibration(H, W):
  """A raw pair of that size: mild five-term distortions, the right camera 0.12 m away and rotated by 1.5 degrees."""
  f = 0.9 * W
  K1 = np.array([[f, 0, W / 2 - 3.0], [0, 1.002 * f, H / 2 + 2.0], [0, 0, 1]])
  K2 = np.array([[0.995 * f, 0, W / 2 + 4.0], [0, 0.997 * f, H / 2 - 1.5], [0, 0, 1]])
  rvec = np.deg2rad(1.5) * np.array([0.6, -0.64, 0.48])
  th = np.linalg.norm(rvec)
  k = rvec / th
  Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
  Q = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
  c2 = np.array([0.12, 0.002, -0.001])
  return K1, [-0.08, 0.02, 4e-4, -3e-4, 0.003], K2, [-0.07, 0.015, -2e-4, 5e-4, 0.002], Q.T, -Q.T @ c2


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


def grid_of(uv, Hs, Ws):
  """The (u, v) map as grid_sample's normalised grid (align_corners=True); refused rays (NaN) point far outside."""
  import torch
  g = torch.nan_to_num(uv, nan=-1e6)
  return torch.stack([2 * g[..., 0] / (Ws - 1) - 1, 2 * g[..., 1] / (Hs - 1) - 1], -1).contiguous()


def warp_case(name, H, W, channels, mode, reps):
  import torch
  import torch.nn.functional as F
  from foundationpose_amd import Utils as U
  from foundationpose_amd import _lib, rectify
  dev = torch.device('cuda', 0)
  rng = np.random.default_rng(0)
  rect = U.rectify_stereo(*calibration(H, W), (H, W))
  if mode == 'colour':
    shape = (1, H, W) + ((3,) if channels == 3 else ())
    srcs = [torch.as_tensor(rng.integers(0, 256, shape).astype(np.uint8), device=dev) for _ in range(2)]
    plans = [rect.left, rect.right]
  else:
    srcs = [torch.as_tensor(rng.uniform(0.3, 3.0, (1, H, W)).astype(np.float32), device=dev)]
    plans = [U.undistort_plan(calibration(H, W)[0], calibration(H, W)[1], (H, W))]
  outs, valids, maps = rectify.remap(srcs, plans, mode, want_valid=True, want_map=True)
  grid = grid_of(torch.cat(maps), H, W)
  stacked = torch.cat(srcs)
  ours = lambda: rectify.remap(srcs, plans, mode)

  def torch_path():
    if mode == 'depth':
      return F.grid_sample(stacked[:, None], grid, mode='nearest', padding_mode='zeros', align_corners=True)[:, 0]
    x = stacked[..., None] if channels == 1 else stacked
    y = F.grid_sample(x.permute(0, 3, 1, 2).float(), grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    return (y + 0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

  ms_ours, ms_torch = time_interleaved([ours, torch_path], reps)
  ctx = _lib.Context.get(dev)      # the kernel alone: the context's own events around the launch, without the host work of the call
  ctx.prof_enable(True)
  ctx.prof_reset()
  for _ in range(reps):
    ours()
  torch.cuda.synchronize()
  kernel_ms = ctx.prof_read('remap')['total_ms'] / reps
  ctx.prof_enable(False)
  got, ref = torch.cat(outs), torch_path()
  if mode == 'colour':
    inside = torch.cat(valids).bool()
    diff = (got.reshape(ref.shape).int() - ref.int()).abs()[inside]
    agreement = dict(max_abs_difference_where_valid=int(diff.max()), share_equal_where_valid=float((diff == 0).float().mean()))
  else:
    agreement = dict(share_equal=float((got == ref).float().mean()))
  elem = 1 if mode == 'colour' else 4
  need = len(srcs) * 2 * H * W * channels * elem
  t = float(np.min(ms_ours))
  return dict(case=name, H=H, W=W, channels=channels, mode=mode, images=len(srcs), launches=1, ms_min=t, ms_median=float(np.median(ms_ours)),
              kernel_ms=kernel_ms,               grid_sample_ms_min=float(np.min(ms_torch)), grid_sample_ms_median=float(np.median(ms_torch)), reps=reps, bytes=int(need),
              GBs=need / (kernel_ms * 1e-3) / 1e9, hbm_fraction=need / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
              valid_fraction=float(torch.cat(valids).float().mean()), **agreement)


def stereo_case(name, H, W, D, reps):
  import torch
  from foundationpose_amd import Utils as U
  dev = torch.device('cuda', 0)
  rng = np.random.default_rng(0)
  rect = U.rectify_stereo(*calibration(H, W), (H, W))
  tex = rng.integers(0, 256, (H, W + 24)).astype(np.uint8)
  left, right = torch.as_tensor(tex[:, :W].copy(), device=dev), torch.as_tensor(tex[:, 24:].copy(), device=dev)
  plain = lambda: U.stereo_depth(left, right, rect.K_new, rect.baseline, max_disparity=D)
  warped = lambda: U.stereo_depth(left, right, rectify=rect, max_disparity=D)
  ms_plain, ms_warped = time_interleaved([plain, warped], reps)
  return dict(case=name, H=H, W=W, max_disparity=D, stereo_depth_ms_min=float(np.min(ms_plain)), stereo_depth_ms_median=float(np.median(ms_plain)),
              with_rectify_ms_min=float(np.min(ms_warped)), with_rectify_ms_median=float(np.median(ms_warped)),
              added_ms_median=float(np.median(ms_warped) - np.median(ms_plain)), reps=reps)


def run_case(name, reps):
  for c in CASES:
    if c[0] == name:
      return warp_case(*c, reps)
  return stereo_case(*next(c for c in STEREO_CASES if c[0] == name), reps)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  ap.add_argument('--case', default=None, help='run this one case in this process and print its JSON (what the driver starts)')
  args = ap.parse_args()
  if args.case:
    print('RESULT ' + json.dumps(run_case(args.case, args.reps)))
    return
  res = dict(reps=args.reps, hbm_peak_GBs=HBM_PEAK_GBS, kernel_form='one launch a call; a thread owns four destination pixels and writes whole dwords', runs=[])
  for name in [c[0] for c in CASES] + [c[0] for c in STEREO_CASES]:
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
    raise SystemExit(f"bench_rectify: case {res['stopped_at']['case']} failed; nothing was started after it")


if __name__ == '__main__':
  main()
