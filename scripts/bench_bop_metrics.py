"""Device time of the BOP errors (HIP events around the calls, inputs already on the device): MSSD + MSPD of 252 poses on the mustard
mesh (96 x 84 grid, 8 066 vertices) with 1 and 73 symmetry transforms (fp_pose_errors_bop), and VSD of 252 poses against one ground
truth at 640x480 and at 1920x1200 (fp_vsd: the depth renders of every pose and the counting pass).  Prints one JSON line.
usage: python scripts/bench_bop_metrics.py [--reps R]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from foundationpose_amd import Utils as U, _lib, synthetic as S
from foundationpose_amd._lib import check, k_ptr, lib, ptr, stream_ptr
from foundationpose_amd.mesh_tensors import make_mesh_tensors


def poses_around(gt, B, rs):
  poses = np.repeat(gt[None], B, 0)
  for p in poses:
    p[:3, :3] = S.random_rotation(rs) if rs.uniform() < 0.5 else p[:3, :3]
    p[:3, 3] = gt[:3, 3] + rs.randn(3) * 0.01
  return poses


def time_ms(run, reps):
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
  assert torch.cuda.is_available(), 'bench_bop_metrics needs an MI355X'
  dev = torch.device('cuda', 0)
  ctx = _lib.Context.get(dev)
  mesh = S.make_mustard_mesh(seed=0)
  mesh.vertices = mesh.vertices - (mesh.vertices.min(0) + mesh.vertices.max(0)) / 2
  rs = np.random.RandomState(0)
  gt = np.eye(4)
  gt[:3, :3] = S.random_rotation(rs)
  gt[:3, 3] = (0.02, -0.03, 0.75)
  B = 252
  t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float, device=dev)
  pts, poses, G = t(mesh.vertices), t(poses_around(gt, B, rs)), t(gt)
  res = {'B': B, 'N': len(pts)}

  Kd, Kp = k_ptr(S.YCB_K)
  out = torch.empty((2, B), device=dev)
  for n_sym in (1, 73):
    sym = t(U.symmetry_tfs_from_info({'symmetries_continuous': [{'axis': [0, 0, 1], 'offset': [0, 0, 0]}]})[:n_sym])
    run = lambda: check(lib().fp_pose_errors_bop(ctx.handle, ptr(pts), len(pts), ptr(poses), ptr(G), 0, B, ptr(sym), n_sym, Kp,
                                                 _lib.FP_BOP_MSSD | _lib.FP_BOP_MSPD, ptr(out[0]), ptr(out[1]), stream_ptr(dev)))
    res[f'mssd_mspd_sym{n_sym}_ms'] = time_ms(run, args.reps)

  mt = make_mesh_tensors(mesh)
  dm = _lib.device_mesh(ctx, mt)
  taus = np.ascontiguousarray(U.BOP19_VSD_TAUS, dtype=np.float64)
  for name, H, W, K in (('vga', 480, 640, S.YCB_K), ('1920x1200', 1200, 1920, np.array([[1600.0, 0, 955.5], [0, 1600.0, 603.2], [0, 0, 1]]))):
    Kd, Kp = k_ptr(K)
    _, d, _ = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=G[None], mesh_tensors=mt)
    depth = (torch.where(d[0] > 0, d[0], torch.full_like(d[0], 1.2)) + 0.001 * torch.randn((H, W), device=dev)).contiguous()
    err = torch.empty((B, len(taus)), device=dev)
    run = lambda: check(lib().fp_vsd(ctx.handle, dm.handle, ptr(depth), 0, H, W, Kp, ptr(poses), ptr(G), 0, B, 0.2, U.BOP19_VSD_DELTA,
                                     ptr(taus), len(taus), ptr(err), None, stream_ptr(dev)))
    res[f'vsd_{name}_ms'] = time_ms(run, max(args.reps // 4, 3))
    res[f'vsd_{name}_mean_e'] = float(err.mean())
  res['reps'] = args.reps
  print(json.dumps(res))


if __name__ == '__main__':
  main()
