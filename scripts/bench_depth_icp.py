"""Device time of fp_depth_normals and of one fp_depth_pairs_align call (16 views of 640 x 480 of the synthetic mustard mesh, the poses
3 mm / 1 degree off, every view paired with its 4 nearest views by optical axis: 64 directed pairs): HIP events around the call, after a
warm-up the minimum and the median of --reps timed calls (the pairs call synchronises: the copy of the sums to the host is inside).
Beside them the bytes each call must move and their share of the HBM peak of the MI355X (8 TB/s).  Normals: every depth and mask byte
once (the four neighbours come from the caches), 16 bytes written per pixel.  Pairs: per pair the source view's normals and depth once
(20 bytes per pixel - the 16 views are read 4 times each, from L2 / MALL after the first), the partial-sum slab written and read once,
and the gathers: 20 bytes per source pixel that projects into the target (neighbouring pixels project to neighbouring pixels, so most
of these are served by the caches).  The photometric term beside them: fp_view_intensity (the normals and 3 bytes of rgb read, 16 bytes written
per pixel), and one fp_depth_pairs_align_photo call with fp_depth_pairs_align calls in between, call by call, in the same process -
it adds one 16-byte source read and one 16-byte gather per pixel to the 20 + 20 bytes, and its slab holds 58 numbers.  Then the wall time of a whole joint_refine_view_poses beside a whole refine_view_poses on the same
views with every pose but the anchor's 2 mm / 0.75 degrees off, and of joint_refine_view_poses(photometric=True) on them (the unlit
render of the mesh is their rgb), interleaved in one process (host clock, device synchronised).
Prints one JSON line.
usage: python scripts/bench_depth_icp.py [--reps R] [--refine-voxel 0.002] [--refine-mm 2] [--refine-deg 0.75] [--out profiles/bench_depth_icp.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from foundationpose_amd import Utils as U
from foundationpose_amd import synthetic as S
from foundationpose_amd import reconstruct as R
from foundationpose_amd.mesh_tensors import make_mesh_tensors

HBM_PEAK_GBS = 8000.0
H, W, N_VIEWS = 480, 640, 16


def look_at(eye):
  """camera-to-object pose: z looks from eye to the origin, x right, y down"""
  z = -np.asarray(eye, dtype=np.float64)
  z /= np.linalg.norm(z)
  up = np.array([0.0, 1.0, 0.0]) if abs(z[2]) > 0.99 else np.array([0.0, 0.0, 1.0])
  x = np.cross(z, up)
  x /= np.linalg.norm(x)
  m = np.eye(4)
  m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, eye
  return m


def fibonacci_eyes(n, radius):
  i = np.arange(n) + 0.5
  z = 1 - 2 * i / n
  phi = i * np.pi * (3 - np.sqrt(5))
  r = np.sqrt(1 - z * z)
  return radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def displacement(pose, truth, ball):
  E = pose @ np.linalg.inv(truth)
  return float(np.linalg.norm(ball @ E[:3, :3].T + E[:3, 3] - ball, axis=1).mean())


def timed(run, reps):
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
  return float(np.min(times)), float(np.median(times))


def timed_interleaved(runs, reps):
  """{name: (min, median)} of the calls of `runs` {name: callable}, timed one after the other in every repetition"""
  for _ in range(3):
    for run in runs.values():
      run()
  torch.cuda.synchronize()
  times = {name: [] for name in runs}
  for _ in range(reps):
    for name, run in runs.items():
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      run()
      e1.record()
      torch.cuda.synchronize()
      times[name].append(e0.elapsed_time(e1))
  return {name: (float(np.min(t)), float(np.median(t))) for name, t in times.items()}


def perturbed(cams, trans, rot_deg, seed, keep_first=False):
  rs = np.random.RandomState(seed)
  out = cams.copy()
  for v in range(1 if keep_first else 0, len(cams)):
    u, w = rs.randn(3), rs.randn(3)
    out[v] = R.expm_se3(np.concatenate([u / np.linalg.norm(u) * trans, w / np.linalg.norm(w) * np.deg2rad(rot_deg)])) @ cams[v]
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--refine-voxel', type=float, default=0.002)
  ap.add_argument('--refine-mm', type=float, default=2.0)
  ap.add_argument('--refine-deg', type=float, default=0.75)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_depth_icp needs an MI355X'
  dev = torch.device('cuda', 0)
  mesh = S.make_mustard_mesh(seed=0)
  mesh.vertices = mesh.vertices - (mesh.vertices.min(0) + mesh.vertices.max(0)) / 2
  mt = make_mesh_tensors(mesh, device=dev)
  K = np.array([[800.0, 0, 319.5], [0, 800.0, 239.5], [0, 0, 1.0]])
  cams = np.stack([look_at(e) for e in fibonacci_eyes(N_VIEWS, 0.6)])
  color, depth, _ = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=np.linalg.inv(cams).astype(np.float32), mesh_tensors=mt)
  depth = depth.contiguous()
  rgb = (color.clamp(0, 1) * 255).round().to(torch.uint8).contiguous()
  mask = (depth > 0).to(torch.uint8).contiguous()
  off = perturbed(cams, 0.003, 1.0, 0)
  res = dict(reps=args.reps, hbm_peak_GBs=HBM_PEAK_GBS, views=N_VIEWS, image=[H, W])

  normals = R.depth_normals(depth, K, mask)
  t_min, t_med = timed(lambda: R.depth_normals(depth, K, mask), args.reps)
  nbytes = N_VIEWS * H * W * (4 + 1 + 16)
  res['depth_normals'] = dict(ms_min=t_min, ms_median=t_med, bytes=nbytes, GBs=nbytes / (t_min * 1e-3) / 1e9, hbm_fraction=nbytes / (t_min * 1e-3) / 1e9 / HBM_PEAK_GBS,
                              normals=int((normals[..., 3] != 0).sum()))

  pairs = R.choose_pairs(off, 4, 100)
  sums = R.align_pairs_step(depth, normals, K, off, pairs, 0.02, 0.5)
  t_min, t_med = timed(lambda: R.align_pairs_step(depth, normals, K, off, pairs, 0.02, 0.5), args.reps)
  tiles = (H * W + 1023) // 1024
  P = len(pairs)
  sources = sum(int((normals[s, ..., 3] != 0).sum()) for s, _ in pairs)
  nbytes = P * H * W * 20 + 2 * P * tiles * 29 * 8
  valid = int(sums[:, 28].sum())
  res['pairs_align'] = dict(pairs=P, ms_min=t_min, ms_median=t_med, bytes=nbytes, GBs=nbytes / (t_min * 1e-3) / 1e9, hbm_fraction=nbytes / (t_min * 1e-3) / 1e9 / HBM_PEAK_GBS,
                            unique_bytes=N_VIEWS * H * W * 20 + 2 * P * tiles * 29 * 8, source_pixels=sources, valid_pixels=valid, gathered_bytes_at_most=sources * 20,
                            workgroups=P * tiles, rms_mm=float(1e3 * np.sqrt(sums[:, 27].sum() / max(valid, 1))))

  intensity = R.view_intensity(rgb, normals)
  t_min, t_med = timed(lambda: R.view_intensity(rgb, normals), args.reps)
  nbytes = N_VIEWS * H * W * (16 + 3 + 16)
  res['view_intensity'] = dict(ms_min=t_min, ms_median=t_med, bytes=nbytes, GBs=nbytes / (t_min * 1e-3) / 1e9, hbm_fraction=nbytes / (t_min * 1e-3) / 1e9 / HBM_PEAK_GBS,
                               records=int((intensity[..., 3] != 0).sum()))
  sums58 = R.align_pairs_step(depth, normals, K, off, pairs, 0.02, 0.5, intensity=intensity)
  assert np.array_equal(sums58[:, :29], sums)
  both = timed_interleaved(dict(geometric=lambda: R.align_pairs_step(depth, normals, K, off, pairs, 0.02, 0.5),
                                photometric=lambda: R.align_pairs_step(depth, normals, K, off, pairs, 0.02, 0.5, intensity=intensity)), args.reps)
  nbytes = P * H * W * 36 + 2 * P * tiles * 58 * 8
  (t_min, t_med), (g_min, g_med) = both['photometric'], both['geometric']
  pvalid = int(sums58[:, 57].sum())
  res['pairs_align_photo'] = dict(pairs=P, ms_min=t_min, ms_median=t_med, bytes=nbytes, GBs=nbytes / (t_min * 1e-3) / 1e9,
                                  hbm_fraction=nbytes / (t_min * 1e-3) / 1e9 / HBM_PEAK_GBS, unique_bytes=N_VIEWS * H * W * 36 + 2 * P * tiles * 58 * 8,
                                  bytes_over_geometric=nbytes / res['pairs_align']['bytes'], gathered_bytes_at_most=sources * 36, valid_pixels=pvalid,
                                  rms_intensity=float(np.sqrt(sums58[:, 56].sum() / max(pvalid, 1))), geometric_interleaved_ms_min=g_min,
                                  geometric_interleaved_ms_median=g_med, ms_over_geometric=t_min / g_min)

  ball = np.random.RandomState(11).randn(2000, 3)
  ball = ball / np.linalg.norm(ball, axis=1, keepdims=True) * 0.05 * np.random.RandomState(12).rand(2000, 1) ** (1 / 3)
  views = dict(depths=depth, masks=mask, rgbs=rgb, K=K, cam_in_obs=perturbed(cams, args.refine_mm * 1e-3, args.refine_deg, 1, keep_first=True))
  runs = dict(joint=lambda: R.joint_refine_view_poses(views, depth_filter=False, device=dev),
              tsdf=lambda: R.refine_view_poses(views, voxel_size=args.refine_voxel, depth_filter=False, device=dev),
              photo=lambda: R.joint_refine_view_poses(views, depth_filter=False, device=dev, photometric=True))
  times, got = dict(joint=[], tsdf=[], photo=[]), {}
  for _ in range(4):
    for name, run in runs.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      got[name] = run()
      torch.cuda.synchronize()
      times[name].append((time.perf_counter() - t0) * 1e3)
  before = [displacement(views['cam_in_obs'][v], cams[v], ball) for v in range(1, N_VIEWS)]
  for name, key in (('joint', 'joint_refine_view_poses'), ('tsdf', 'refine_view_poses'), ('photo', 'joint_refine_view_poses_photometric')):
    after = [displacement(got[name][0][v], cams[v], ball) for v in range(1, N_VIEWS)]
    res[key] = dict(ms_first=times[name][0], ms_min=float(np.min(times[name][1:])), ms_median=float(np.median(times[name][1:])),
                    perturbation_mm=args.refine_mm, perturbation_deg=args.refine_deg, views_improved=int(np.sum(np.array(after) < np.array(before))),
                    mean_displacement_mm_before=float(1e3 * np.mean(before)), mean_displacement_mm_after=float(1e3 * np.mean(after)),
                    max_displacement_mm_after=float(1e3 * np.max(after)), stopped={str(k): v for k, v in got[name][1]['stopped'].items()})
  info = got['joint'][1]
  res['joint_refine_view_poses'].update(evaluations=int(len(info['rms'])), pairs=int(len(info['pairs'][0])), rms_mm_first=float(1e3 * info['rms'][0]),
                                        rms_mm_last=float(1e3 * info['rms'][-1]), eig_ratio_min=float(np.nanmin(info['eig_ratio'])))
  info = got['photo'][1]
  res['joint_refine_view_poses_photometric'].update(evaluations=int(len(info['rms'])), weight=R.PHOTO_WEIGHT, i_max=R.I_MAX, rms_mm_last=float(1e3 * info['rms'][-1]),
                                                    photo_rms_first=float(info['photo_rms'][0]), photo_rms_last=float(info['photo_rms'][-1]),
                                                    eig_ratio_min=float(np.nanmin(info['eig_ratio'])))
  res['refine_view_poses'].update(voxel=args.refine_voxel, band=2 * args.refine_voxel)
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
