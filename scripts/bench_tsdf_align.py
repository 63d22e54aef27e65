"""Device time of one fp_tsdf_align call (16 views of 640 x 480 against a 256^3 volume fused from the same rendered views of the synthetic
mustard mesh, the poses 3 mm / 1 degree off): HIP events around the call, after a warm-up the minimum and the median of --reps timed calls
(the call synchronises: the copy of the sums to the host is inside).  Beside it: the bytes the call must move - every depth map once and
the partial-sum slab written and read once - and their share of the HBM peak of the MI355X (8 TB/s), and the bytes its gathers ask for
(64 per valid pixel: tsdf and weight at the 8 corners; neighbouring pixels share cells, so most of these are served by the caches).  Then a
whole refine_view_poses of those views at 2 mm voxels with every pose but the anchor's 2 mm / 0.75 degrees off - half the 2-voxel band
the alignment runs in, a case it is built for (host clock around it, device synchronised: 15 sequential alignments, their 6 x 6 solves on
the host, 16 integrations), and the numpy float32 restatement of one step (tests/tsdf_align_oracle.py) at 4 views of 160 x 120 against 64^3 points in
the same process for the scale of a host implementation.  Prints one JSON line.
usage: python scripts/bench_tsdf_align.py [--reps R] [--refine-voxel 0.002] [--refine-mm 2] [--refine-deg 0.75] [--out profiles/bench_tsdf_align.json]"""
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
from foundationpose_amd.mesh_tensors import make_mesh_tensors
from foundationpose_amd.reconstruct import TsdfVolume, expm_se3, refine_view_poses
from tests import tsdf_align_oracle as A
from tests import tsdf_oracle as O

HBM_PEAK_GBS = 8000.0
H, W, N_VIEWS, DIM = 480, 640, 16, 256


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


def perturbed(cams, trans, rot_deg, seed, keep_first=False):
  rs = np.random.RandomState(seed)
  out = cams.copy()
  for v in range(1 if keep_first else 0, len(cams)):
    u, w = rs.randn(3), rs.randn(3)
    out[v] = expm_se3(np.concatenate([u / np.linalg.norm(u) * trans, w / np.linalg.norm(w) * np.deg2rad(rot_deg)])) @ cams[v]
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--refine-voxel', type=float, default=0.002)
  ap.add_argument('--refine-mm', type=float, default=2.0)
  ap.add_argument('--refine-deg', type=float, default=0.75)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_tsdf_align needs an MI355X'
  dev = torch.device('cuda', 0)
  mesh = S.make_mustard_mesh(seed=0)
  mesh.vertices = mesh.vertices - (mesh.vertices.min(0) + mesh.vertices.max(0)) / 2
  mt = make_mesh_tensors(mesh, device=dev)
  K = np.array([[800.0, 0, 319.5], [0, 800.0, 239.5], [0, 0, 1.0]])
  cams = np.stack([O.look_at(e) for e in O.fibonacci_eyes(N_VIEWS, 0.6)])
  _, depth, _ = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=np.linalg.inv(cams).astype(np.float32), mesh_tensors=mt)
  depth = depth.contiguous()
  mask = (depth > 0).to(torch.uint8).contiguous()
  vs = 0.2 / (DIM - 1)
  vol = TsdfVolume(np.full(3, -0.1), vs, (DIM,) * 3, device=dev)
  vol.integrate(depth, K, cams, masks=mask)
  off = perturbed(cams, 0.003, 1.0, 0)
  res = dict(reps=args.reps, hbm_peak_GBs=HBM_PEAK_GBS, dims=[DIM] * 3, views=N_VIEWS, image=[H, W])

  sums = vol.align_step(depth, K, off, masks=mask)
  t_min, t_med = timed(lambda: vol.align_step(depth, K, off, masks=mask), args.reps)
  tiles = (H * W + 1023) // 1024
  nbytes = N_VIEWS * H * W * (4 + 1) + 2 * N_VIEWS * tiles * 29 * 8
  valid = int(sums[:, 28].sum())
  res['align_step'] = dict(ms_min=t_min, ms_median=t_med, bytes=nbytes, GBs=nbytes / (t_min * 1e-3) / 1e9, hbm_fraction=nbytes / (t_min * 1e-3) / 1e9 / HBM_PEAK_GBS,
                           valid_pixels=valid, gathered_bytes=valid * 64, gathered_GBs=valid * 64 / (t_min * 1e-3) / 1e9,
                           rms_mm=float(1e3 * np.sqrt(sums[:, 27].sum() / max(valid, 1))))

  views = dict(depths=depth, masks=mask, K=K, cam_in_obs=perturbed(cams, args.refine_mm * 1e-3, args.refine_deg, 1, keep_first=True))
  times, got = [], None
  for _ in range(4):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got, info = refine_view_poses(views, voxel_size=args.refine_voxel, depth_filter=False, device=dev)
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) * 1e3)
  before = [A.displacement(views['cam_in_obs'][v], cams[v]) for v in range(1, N_VIEWS)]
  after = [A.displacement(got[v], cams[v]) for v in range(1, N_VIEWS)]
  res['refine_view_poses'] = dict(ms_first=times[0], ms_min=float(np.min(times[1:])), ms_median=float(np.median(times[1:])), voxel=args.refine_voxel, band=2 * args.refine_voxel,
                                  perturbation_mm=args.refine_mm, perturbation_deg=args.refine_deg, views_improved=int(np.sum(np.array(after) < np.array(before))),
                                  mean_displacement_mm_before=float(1e3 * np.mean(before)), mean_displacement_mm_after=float(1e3 * np.mean(after)),
                                  max_displacement_mm_after=float(1e3 * np.max(after)), stopped={str(k): v for k, v in info['stopped'].items()})

  hd, hn = 64, 4
  small = torch.nn.functional.interpolate(depth[:hn, None], size=(120, 160), mode='nearest')[:, 0].cpu().numpy()
  Ks = np.array([[200.0, 0, 79.5], [0, 200.0, 59.5], [0, 0, 1.0]])
  ref = O.Volume(np.full(3, -0.1), 0.2 / (hd - 1), (hd,) * 3)
  ref.integrate(small, Ks, cams[:hn])
  t0 = time.perf_counter()
  host = A.step_sums(ref, small, Ks, off[:hn])
  res['host_numpy_step_64'] = dict(dims=[hd] * 3, views=hn, image=[120, 160], ms=(time.perf_counter() - t0) * 1e3, valid_pixels=int(host[:, 28].sum()))
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
