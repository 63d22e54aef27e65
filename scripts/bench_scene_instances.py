"""Device time of Utils.scene_instances (fp_scene_instances: masks, visible masks, owner, depth and gt_info of 8 instances in one call)
beside the loop the project used for the same answer, in the same process and interleaved call by call: per object one
nvdiffrast_render depth + torch.where into the composite (tests/test_gpu_bop_run.py::_frame), extended by the visibility test against the
frame's depth and per-object sum / nonzero min-max for the counts and boxes.  HIP events around each call, after a warm-up the minimum
and the median of --reps calls; 640 x 480 and 1920 x 1200, pad 0 and 'bop'.  A second, profiled call splits the new one into render time
and fused-pass time (fp_prof classes 'render', 'scene_pass') and gives the pass' GB/s over the bytes it must read and write.  A canvas
the rasteriser refuses is reported as such.  Prints one JSON line; exits non-zero when the new call's median is above the loop's.
usage: python scripts/bench_scene_instances.py [--reps R] [--out profiles/bench_scene_instances.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from foundationpose_amd import Utils as U
from foundationpose_amd import _lib, synthetic as S
from foundationpose_amd.mesh_tensors import make_mesh_tensors

VGA_K = S.YCB_K
FULL_HD_K = np.array([[1600.0, 0, 955.5], [0, 1600.0, 603.2], [0, 0, 1]])


def scene(K, H, W, n=8):
  """n instances of two models spread over the frame at 0.7 .. 1.0 m, and a depth image: their composite over a plane at 1.2 m"""
  meshes = []
  for seed, (nt, nz) in ((0, (96, 84)), (1, (80, 70))):
    m = S.make_mustard_mesh(seed=seed, n_theta=nt, n_z=nz)
    m.vertices = m.vertices - (m.vertices.min(0) + m.vertices.max(0)) / 2
    meshes.append(make_mesh_tensors(m))
  mts = [meshes[i % 2] for i in range(n)]
  poses = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
  span_x, span_y = 0.35 * W / K[0, 0], 0.3 * H / K[1, 1]
  for i in range(n):
    poses[i, :3, :3] = S.random_rotation(np.random.RandomState(40 + i))
    z = 0.7 + 0.04 * i
    poses[i, :3, 3] = [(-1 + 2 * (i % 4) / 3.0) * span_x * z, (-0.5 + (i // 4)) * span_y * z, z]
  out = U.scene_instances(K, H, W, mts, poses, occluders='instances', want=('depth',))
  depth = torch.where(out['depth'] > 0, out['depth'], torch.full_like(out['depth'], 1.2))
  return mts, torch.as_tensor(poses, device='cuda'), depth


def baseline(K, H, W, mts, poses, depth, pad_x, pad_y, delta=0.015):
  """The per-object loop: render, composite, visibility against the frame's depth and the other instances, counts and boxes"""
  Kc = np.array(K, dtype=np.float64)
  Kc[0, 2] += pad_x
  Kc[1, 2] += pad_y
  Hc, Wc = H + 2 * pad_y, W + 2 * pad_x
  comp = torch.full((H, W), float('inf'), device='cuda')
  owner = torch.full((H, W), -1, device='cuda', dtype=torch.int32)
  layers = []
  for o, (mt, p) in enumerate(zip(mts, poses)):
    _, d, _ = U.nvdiffrast_render(K=Kc, H=Hc, W=Wc, ob_in_cams=p.reshape(1, 4, 4), mesh_tensors=mt)
    layers.append(d[0])
    f = d[0, pad_y:pad_y + H, pad_x:pad_x + W]
    near = (f > 0) & (f < comp)
    comp = torch.where(near, f, comp)
    owner = torch.where(near, torch.full_like(owner, o), owner)
  occ = torch.minimum(comp, torch.where(depth > 0, depth, torch.full_like(depth, float('inf'))))
  rows, masks, visibs = [], [], []
  for d in layers:
    m = d > 0
    f = d[pad_y:pad_y + H, pad_x:pad_x + W]
    vis = (f > 0) & (f - occ <= delta)
    masks.append(m[pad_y:pad_y + H, pad_x:pad_x + W])
    visibs.append(vis)
    row = [m.sum(), (masks[-1] & (depth > 0)).sum(), vis.sum(), masks[-1].sum()]
    for s in (m, vis):
      nz = s.nonzero()
      row += [nz[:, 1].min(), nz[:, 0].min(), nz[:, 1].max(), nz[:, 0].max()] if len(nz) else [torch.tensor(-1, device='cuda')] * 4
    rows.append(torch.stack(row))
  return torch.stack(masks), torch.stack(visibs), owner, comp, torch.stack(rows).cpu()


def timed(fn):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_scene_instances needs an MI355X'
  torch.cuda.set_device(0)
  ctx = _lib.Context.get(torch.device('cuda', 0))
  res = dict(reps=args.reps, n_instances=8)
  for name, K, H, W in (('640x480', VGA_K, 480, 640), ('1920x1200', FULL_HD_K, 1200, 1920)):
    mts, poses, depth = scene(K, H, W)
    for pad in (0, 'bop'):
      pad_x, pad_y = (W, H) if pad == 'bop' else (pad, pad)
      new = lambda: U.scene_instances(K, H, W, mts, poses, depth=depth, pad=pad)
      old = lambda: baseline(K, H, W, mts, poses, depth, pad_x, pad_y)
      key = f'{name}_pad_{pad}'
      try:
        new()
      except _lib.FoundationPoseAmdError as e:
        res[key] = dict(refused=str(e)[:200])
        continue
      for _ in range(3):
        new(), old()
      torch.cuda.synchronize()
      t_new, t_old = [], []
      for _ in range(args.reps):
        t_new.append(timed(new))
        t_old.append(timed(old))
      ctx.prof_enable(True)
      ctx.prof_reset()
      new()
      torch.cuda.synchronize()
      render, fused = ctx.prof_read('render'), ctx.prof_read('scene_pass')
      ctx.prof_enable(False)
      res[key] = dict(new_ms_min=float(np.min(t_new)), new_ms_median=float(np.median(t_new)), loop_ms_min=float(np.min(t_old)),
                      loop_ms_median=float(np.median(t_old)), speedup_median=float(np.median(t_old) / np.median(t_new)),
                      render_ms=render['total_ms'], render_launches=render['launches'], pass_ms=fused['total_ms'], pass_bytes=fused['flops'],
                      pass_GBps=fused['flops'] / (fused['total_ms'] * 1e-3) / 1e9 if fused['total_ms'] > 0 else None,
                      not_slower=bool(np.median(t_new) <= np.median(t_old)))
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')
  # the condition of the measurement: the one call is not slower than the loop it replaces, wherever both ran
  slower = [k for k, v in res.items() if isinstance(v, dict) and v.get('not_slower') is False]
  if slower:
    raise SystemExit(f'scene_instances is slower than the per-object loop for {slower}')


if __name__ == '__main__':
  main()
