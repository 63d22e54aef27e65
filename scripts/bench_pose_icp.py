"""Device time of polishing poses against depth on one 640 x 480 frame of the synthetic mustard mesh, crop 160, for N = 1, 8 and 252
poses (4 mm / 1.5 degrees off the frame's pose, seeded): one fp_pose_depth_align call alone (its maps rendered beforehand; nothing
synchronises) and a whole fp_pose_polish at the default iterations (8 + the closing round).  HIP events around the call, after a warm-up
the minimum and the median of --reps timed calls.  Beside them, call by call in the same process, track_one (2 iterations) on the same
scene, host clock with the device synchronised.
Bytes that must move, from the shapes.  Align: the two maps once (24 bytes per map pixel), the partial-sum slab written and read once
(232 bytes per workgroup of 1024 pixels, twice), and the gathers: 20 bytes per rendered pixel at most (neighbouring map pixels land on
the same or neighbouring frame pixels - a crop of 160 magnifies the object - so the caches serve nearly all of them).  Polish: per round
that, plus the two maps written by the rasteriser (another 24 bytes per pixel); the rasteriser's own traffic (vertices, face lists) is
not counted.  The share of the 8 TB/s HBM peak says what bounds the call: at N = 1 a round is five launches of a few microseconds each and
the call is bound by launches; at N = 252 the bytes begin to count.
Prints one JSON line.
usage: python scripts/bench_pose_icp.py [--reps R] [--out profiles/bench_pose_icp.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from foundationpose_amd import Utils as U
from foundationpose_amd import _lib
from foundationpose_amd import pose_icp as PI
from foundationpose_amd.reconstruct import depth_normals, expm_se3

HBM_PEAK_GBS = 8000.0
H, W, CROP = 480, 640, 160


def timed(run, reps, dev):
  for _ in range(3):
    run()
  torch.cuda.synchronize(dev)
  ms = []
  for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run()
    b.record()
    b.synchronize()
    ms.append(a.elapsed_time(b))
  return float(np.min(ms)), float(np.median(ms))


def perturbed(truth, n, rs, trans=0.004, rot_deg=1.5):
  out = []
  for _ in range(n):
    u, w = rs.randn(3), rs.randn(3)
    p = np.array(truth, dtype=np.float64)
    p[:3, :3] = expm_se3(np.concatenate([np.zeros(3), w / np.linalg.norm(w) * np.deg2rad(rot_deg)]))[:3, :3] @ p[:3, :3]
    p[:3, 3] += u / np.linalg.norm(u) * trans
    out.append(p)
  return np.stack(out).astype(np.float32)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  dev = torch.device('cuda', 0)
  est, objects = bench.build_job(dev, n_objects=1, rank=0)
  ob = objects[0]
  ctx = est.refiner.ctx
  ctx.reserve(256)
  K = ob['K']
  from foundationpose_amd import synthetic as S
  truth = np.eye(4)
  rs0 = np.random.RandomState(1000)                                 # make_scene(seed=0)'s pose
  truth[:3, :3] = S.random_rotation(rs0)
  truth[:3, 3] = (0.02, -0.03, 0.75)
  depth = ob['depth']
  mask = torch.as_tensor(ob['mask'], device=dev)
  normals = depth_normals(depth, K, mask[None], device=dev)[0]
  Kd, Kp = _lib.k_ptr(K)
  dm = _lib.device_mesh(ctx, est.mesh_tensors)
  rs = np.random.RandomState(3)
  res = dict(reps=args.reps, hbm_peak_GBs=HBM_PEAK_GBS, image=[H, W], crop=CROP, iterations=PI.DEFAULT_ITERATIONS, dist_max=PI.DEFAULT_DIST_MAX,
             cos_min=PI.DEFAULT_COS_MIN, observed_normals=int((normals[..., 3] != 0).sum()), cases=[])
  # track_one on the same scene: pose_last is put back before every call
  start = torch.as_tensor(perturbed(truth, 1, rs), device=dev)
  rgb_u8 = torch.as_tensor(ob['rgb_np'], device=dev)

  def track():
    est.pose_last = start.clone()
    est.track_one(rgb_u8, depth, K, iteration=2)
  for _ in range(3):
    track()
  track_ms = []
  for N in (1, 8, 252):
    given = torch.as_tensor(perturbed(truth, N, rs), device=dev).contiguous()
    poses = given.clone()
    state = PI.new_pose_state(N, dev)
    sums = torch.zeros((N, 29), dtype=torch.float64, device=dev)
    counts = torch.zeros((N, 2), dtype=torch.int32, device=dev)
    # the maps of the given poses, for the align call alone
    tf, bb = torch.empty((N, 9), device=dev), torch.empty((N, 4), device=dev)
    _lib.check(_lib.lib().fp_crop_window_tf(ctx.handle, _lib.ptr(given), N, Kp, 1.2, float(est.diameter), CROP, CROP, _lib.ptr(tf), _lib.ptr(bb),
                                           _lib.stream_ptr(dev)))
    ex = {}
    _, _, nm = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=given, get_normal=True, mesh_tensors=est.mesh_tensors, bbox2d=bb, output_size=(CROP, CROP),
                                   glctx=U.RasterizeContext(dev), extra=ex)
    xyz = ex['xyz_map']

    def align():
      _lib.check(_lib.lib().fp_pose_depth_align(ctx.handle, _lib.ptr(xyz), _lib.ptr(nm), N, CROP, CROP, _lib.ptr(depth), _lib.ptr(normals), H, W, Kp,
                                               _lib.ptr(given), PI.DEFAULT_DIST_MAX, PI.DEFAULT_COS_MIN, None, _lib.ptr(sums), _lib.ptr(counts), None,
                                               _lib.stream_ptr(dev)))

    def polish():
      poses.copy_(given)
      PI.enqueue_polish(ctx, dm.handle, poses, Kp, H, W, depth, normals, CROP, 1.2, float(est.diameter), PI.DEFAULT_ITERATIONS, PI.DEFAULT_DIST_MAX,
                        PI.DEFAULT_COS_MIN, PI.DEFAULT_DAMPING, PI.DEFAULT_MIN_PIXELS, state, sums, counts)
    a_min, a_med = timed(align, args.reps, dev)
    c = counts.cpu().numpy()
    valid = sums.cpu().numpy()[:, 28]
    p_min, p_med = timed(polish, args.reps, dev)
    # interleaved: polish, track_one, polish, ... on the host clock
    pw, tw = [], []
    for _ in range(args.reps):
      torch.cuda.synchronize(dev)
      t0 = time.perf_counter()
      polish()
      torch.cuda.synchronize(dev)
      t1 = time.perf_counter()
      track()
      torch.cuda.synchronize(dev)
      pw.append((t1 - t0) * 1e3)
      tw.append((time.perf_counter() - t1) * 1e3)
    track_ms += tw
    info = PI.polish_info(state, counts)
    px = N * CROP * CROP
    tiles = N * ((CROP * CROP + 1023) // 1024)
    align_bytes = px * 24 + 2 * tiles * 232 + int(c[:, 0].sum()) * 20
    rounds = PI.DEFAULT_ITERATIONS + 1
    polish_bytes = rounds * (align_bytes + px * 24)
    res['cases'].append(dict(
      N=N, rendered_pixels=int(c[:, 0].sum()), observed_pixels=int(c[:, 1].sum()), valid_pixels=int(valid.sum()), workgroups=tiles,
      align=dict(ms_min=a_min, ms_median=a_med, bytes=align_bytes, GBs=align_bytes / a_min / 1e6, hbm_fraction=align_bytes / a_min / 1e6 / HBM_PEAK_GBS,
                 launches=3),
      polish=dict(ms_min=p_min, ms_median=p_med, rounds=rounds, launches_at_least=rounds * 6, bytes=polish_bytes, GBs=polish_bytes / p_min / 1e6,
                  hbm_fraction=polish_bytes / p_min / 1e6 / HBM_PEAK_GBS, us_per_round=p_min / rounds * 1e3, wall_ms_min=float(np.min(pw)),
                  wall_ms_median=float(np.median(pw)), steps=[int(x) for x in info['steps'][:8]], stopped=info['stopped'][:8],
                  rms_mm_median=float(np.median(info['rms']) * 1e3))))
  res['track_one'] = dict(iterations=2, wall_ms_min=float(np.min(track_ms)), wall_ms_median=float(np.median(track_ms)))
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
