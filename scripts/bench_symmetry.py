"""Device time of fp_symmetry_residuals with HIP events around the call: after a warm-up the minimum and the median of --reps timed calls,
and the point-triangle tests per second that makes.  The case is the first stage of Utils.find_symmetries on the mesh fused from 16
rendered views of the synthetic mustard bottle and simplified to 8192 vertices (the mesh of scripts/bench_mesh_distance.py): all of its
candidates (1752 at the defaults) on n_coarse = 512 surface samples, and the second-stage shape beside it (64 transforms on 4096 samples).
Beside each, interleaved call by call in the same process, the path it replaces: the T n transformed points formed by torch (one
baddbmm), fp_point_mesh_distance on them, and the per-transform maximum, mean and mean square by torch reductions over the (T, n)
distances.  Then the wall time of a whole Utils.find_symmetries on that mesh, and what it finds.  Prints one JSON line.
usage: python scripts/bench_symmetry.py [--reps 20] [--out profiles/bench_symmetry.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from foundationpose_amd import Utils as U
from foundationpose_amd import _lib
from foundationpose_amd import symmetry as SY
from scripts.bench_mesh_distance import fused_mesh


def event_ms(run):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  run()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1)


def case(pts, tfs, pos, faces, reps):
  T, n, F = len(tfs), len(pts), len(faces)
  tfs_d = U._tfs_f32_on(tfs, pos.device)
  rot, trans = tfs_d[:, :, :3].contiguous(), tfs_d[:, :, 3].contiguous()
  fused = lambda: U._symmetry_residuals_on(pts, tfs_d, pos, faces)[0]

  def replaced():
    q = torch.baddbmm(trans[:, None, :], pts[None].expand(T, n, 3), rot.transpose(1, 2)).reshape(T * n, 3)
    d = U._point_mesh_distance_on(q, pos, faces)[0].reshape(T, n).double()
    return torch.stack([d.max(1).values, d.mean(1), (d * d).mean(1)], 1)
  for _ in range(3):
    a, b = fused(), replaced()
  torch.cuda.synchronize()
  ms = dict(fused=[], replaced=[])
  for _ in range(reps):                       # interleaved: fused, replaced, fused, replaced, ..
    ms['fused'].append(event_ms(fused))
    ms['replaced'].append(event_ms(replaced))
  s = a.cpu().numpy()
  b = b.cpu().numpy()
  pairs = float(T) * n * F
  return dict(transforms=T, samples=n, faces=F, pairs=pairs, ms_min=float(np.min(ms['fused'])), ms_median=float(np.median(ms['fused'])),
              pairs_per_s=pairs / (float(np.min(ms['fused'])) * 1e-3), replaced_ms_min=float(np.min(ms['replaced'])),
              replaced_ms_median=float(np.median(ms['replaced'])),
              max_abs_difference_of_max=float(np.abs(s[:, _lib.FP_SURFDIST_STATS_MAX] - b[:, 0]).max()))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_symmetry needs an MI355X'
  dev = torch.device('cuda', 0)
  pos, nrm, col, faces = fused_mesh(dev)
  small, info = U.simplify_mesh((pos, faces, nrm, col), max_vertices=8192)
  s_pos, s_faces = torch.as_tensor(small.vertices, dtype=torch.float, device=dev), torch.as_tensor(small.faces, dtype=torch.int32, device=dev)
  v = s_pos.cpu().numpy().astype(np.float64)
  _, centroid, cov = SY.surface_moments(v, small.faces)
  eigenvalues, axes = SY.principal_axes(cov)
  cands = SY.candidates()
  tfs = np.stack([SY.candidate_transform(c, axes, centroid) for c in cands])
  res = dict(reps=args.reps, mesh=dict(vertices=len(s_pos), faces=len(s_faces)), tile=_lib.FP_SURFDIST_TILE, chunk=_lib.FP_SURFDIST_CHUNK)
  res['coarse_stage'] = case(U.sample_surface((s_pos, s_faces), 512, seed=0), tfs, s_pos, s_faces, args.reps)
  res['verify_stage'] = case(U.sample_surface((s_pos, s_faces), 4096, seed=0), tfs[:64], s_pos, s_faces, args.reps)
  try:
    U.find_symmetries(small)                  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    found = U.find_symmetries(small)
    res['find_symmetries'] = dict(wall_ms=(time.perf_counter() - t0) * 1e3, tol=found['tol'], n_candidates=found['n_candidates'],
                                  n_transforms=len(found['symmetry_tfs']), n_discrete=len(found['symmetries_discrete']),
                                  n_continuous=len(found['symmetries_continuous']), eigenvalues=found['eigenvalues'].tolist(),
                                  max_residual=float(found['max'].max()), closed=found['closed'])
  except ValueError as e:                     # more than max_group elements at the default tol: reported, not hidden
    res['find_symmetries'] = dict(error=str(e))
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
