"""Device time of Utils.draw_poses (fp_draw_poses: the boxes, axes and silhouettes of 8 objects drawn on the frame in two launches) beside
the Utils.scene_instances call that makes its owner map, in the same process and interleaved call by call: the scene of
scripts/bench_scene_instances.py at 640 x 480 and 1920 x 1200; box + axes, and box + axes + fill + contour.  HIP events around each call,
after a warm-up the minimum and the median of --reps calls.  A second, profiled run splits the draw into its set-up launch and its tiled
pass (fp_prof classes 'draw_setup', 'draw'), gives the pass' GB/s over the bytes it must move (the frame in and out, the owner map once)
and the scene pass of fp_scene_instances ('scene_pass') on the same scene.  Prints one JSON line.
The gate: exits non-zero when the median of the box + axes + fill + contour draw is above the median of the whole scene_instances call
that produced its owner map, at either size - drawing on a segmentation must not cost more than making it.
usage: python scripts/bench_draw_poses.py [--reps R] [--out profiles/bench_draw_poses.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from foundationpose_amd import Utils as U
from foundationpose_amd import _lib
from scripts.bench_scene_instances import FULL_HD_K, VGA_K, scene, timed


def frame(H, W):
  vs, us = torch.meshgrid(torch.arange(H, device='cuda'), torch.arange(W, device='cuda'), indexing='ij')
  rgb = torch.stack([0.5 + 0.3 * torch.sin(us * 0.07) * torch.cos(vs * 0.05), 0.45 + 0.3 * torch.sin(us * 0.031 + vs * 0.043),
                     0.4 + 0.25 * torch.cos(vs * 0.09 - us * 0.02)], -1)
  return (rgb * 255).clamp(0, 255).to(torch.uint8).contiguous()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=50)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_draw_poses needs an MI355X'
  torch.cuda.set_device(0)
  ctx = _lib.Context.get(torch.device('cuda', 0))
  ctx.reserve(8)
  res = dict(reps=args.reps, n_objects=8)
  for name, K, H, W in (('640x480', VGA_K, 480, 640), ('1920x1200', FULL_HD_K, 1200, 1920)):
    mts, poses, depth = scene(K, H, W)
    img, out = frame(H, W), torch.empty((H, W, 3), dtype=torch.uint8, device='cuda')
    boxes = np.stack([np.stack([m['pos'].min(0).values.cpu().numpy(), m['pos'].max(0).values.cpu().numpy()]) for m in mts])
    seg = lambda: U.scene_instances(K, H, W, mts, poses, depth=depth, want=('owner',))
    owner = seg()['owner']
    lines = lambda: U.draw_poses(img, K, poses, bboxes=boxes, out=out)
    full = lambda: U.draw_poses(img, K, poses, bboxes=boxes, owner=owner, fill_alpha=0.35, contour=True, out=out)
    for _ in range(5):
      lines(), full(), seg()
    torch.cuda.synchronize()
    t_lines, t_full, t_seg = [], [], []
    for _ in range(args.reps):
      t_lines.append(timed(lines))
      t_full.append(timed(full))
      t_seg.append(timed(seg))
    prof = {}
    ctx.prof_enable(True)
    for key, fn in (('lines', lines), ('full', full), ('seg', seg)):
      ctx.prof_reset()
      for _ in range(10):
        fn()
      torch.cuda.synchronize()
      prof[key] = {c: ctx.prof_read(c) for c in ('draw_setup', 'draw', 'scene_pass', 'render')}
    ctx.prof_enable(False)
    per = lambda key, c: prof[key][c]['total_ms'] / max(prof[key][c]['launches'], 1)
    gbps = lambda key: prof[key]['draw']['flops'] / (prof[key]['draw']['total_ms'] * 1e-3) / 1e9 if prof[key]['draw']['total_ms'] > 0 else None
    res[name] = dict(
      lines_ms_min=float(np.min(t_lines)), lines_ms_median=float(np.median(t_lines)), full_ms_min=float(np.min(t_full)),
      full_ms_median=float(np.median(t_full)), scene_instances_ms_min=float(np.min(t_seg)), scene_instances_ms_median=float(np.median(t_seg)),
      lines_setup_ms=per('lines', 'draw_setup'), lines_pass_ms=per('lines', 'draw'), lines_pass_bytes=6 * H * W, lines_pass_GBps=gbps('lines'),
      full_setup_ms=per('full', 'draw_setup'), full_pass_ms=per('full', 'draw'), full_pass_bytes=10 * H * W, full_pass_GBps=gbps('full'),
      scene_pass_ms=per('seg', 'scene_pass'), scene_render_ms=prof['seg']['render']['total_ms'] / 10,
      not_slower=bool(np.median(t_full) <= np.median(t_seg)))
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')
  slower = [k for k, v in res.items() if isinstance(v, dict) and v.get('not_slower') is False]
  if slower:
    raise SystemExit(f'draw_poses with fill and contour is slower than the scene_instances call that makes its owner map for {slower}')


if __name__ == '__main__':
  main()
