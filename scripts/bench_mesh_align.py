"""Device time of fp_points_mesh_align with HIP events around the call: after a warm-up the minimum and the median of --reps timed calls and
the point-triangle tests per second that makes, for N = 1 and N = 24 starts x 4096 samples against the mesh fused from 16 rendered views
of the synthetic mustard bottle (the mesh of scripts/bench_mesh_distance.py) and against that mesh simplified to 8192 vertices.  Beside
each, interleaved call by call in the same process, the path it replaces: fp_symmetry_residuals for the moved points,
fp_point_mesh_distance with the closest points on them, and the rows' sums by torch (a point-to-plane J^T J and J^T r per pose with the
host-supplied face normals left out: the closest-point direction stands in, which is what a user without the kernel would have).  The
share of everything but the search - the fill of the keys, the rows, the fold - is the same call against a ONE-triangle mesh.  Then the
wall time of a whole Utils.align_to_mesh (24 starts, the default stages) of the simplified mesh under a rigid transform onto itself.
Prints one JSON line.
usage: python scripts/bench_mesh_align.py [--reps 20] [--out profiles/bench_mesh_align.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from foundationpose_amd import Utils as U
from foundationpose_amd import mesh_align as MA
from scripts.bench_mesh_distance import fused_mesh
from scripts.bench_symmetry import event_ms


def case(pts, poses, pos, faces, reps):
  N, n, F = len(poses), len(pts), len(faces)
  dev = pos.device
  keys = torch.empty(N * n, dtype=torch.int64, device=dev)
  tfs = poses[:, :3, :].contiguous()
  one_pos, one_face = pos[faces[0].long()].contiguous(), torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
  fused = lambda: MA.align_step_on(pts, poses, pos, faces, 'plane', 0.02, keys=keys)[0]
  rest = lambda: MA.align_step_on(pts, poses, one_pos, one_face, 'plane', 0.02, keys=keys)[0]

  def replaced():
    q = U._symmetry_residuals_on(pts, tfs, pos, faces, want_q=True)[1]
    dist, _, closest = U._point_mesh_distance_on(q, pos, faces, want_closest=True)
    e = (q - closest).double()
    nrm = e / dist.double().clamp_min(1e-12)[:, None]
    X = (q.reshape(N, n, 3) - poses[:, None, :3, 3]).reshape(-1, 3).double()
    J = torch.cat([nrm, torch.linalg.cross(X, nrm)], 1) * (dist <= 0.02)[:, None]
    r = (nrm * e).sum(1) * (dist <= 0.02)
    J, r = J.reshape(N, n, 6), r.reshape(N, n)
    return torch.cat([(J.transpose(1, 2) @ J).reshape(N, 36), (J * r[..., None]).sum(1), (r * r).sum(1, keepdim=True)], 1)
  for _ in range(3):
    a, b, c = fused(), replaced(), rest()
  torch.cuda.synchronize()
  ms = dict(fused=[], replaced=[], rest=[])
  for _ in range(reps):                       # interleaved: fused, replaced, rest, fused, ..
    ms['fused'].append(event_ms(fused))
    ms['replaced'].append(event_ms(replaced))
    ms['rest'].append(event_ms(rest))
  pairs = float(N) * n * F
  return dict(poses=N, samples=n, faces=F, pairs=pairs, ms_min=float(np.min(ms['fused'])), ms_median=float(np.median(ms['fused'])),
              pairs_per_s=pairs / (float(np.min(ms['fused'])) * 1e-3), replaced_ms_min=float(np.min(ms['replaced'])),
              replaced_ms_median=float(np.median(ms['replaced'])), without_search_ms_min=float(np.min(ms['rest'])),
              without_search_ms_median=float(np.median(ms['rest'])), valid_points=float(a[:, 28].sum().item()))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_mesh_align needs an MI355X'
  dev = torch.device('cuda', 0)
  pos, nrm, col, faces = fused_mesh(dev)
  small, _ = U.simplify_mesh((pos, faces, nrm, col), max_vertices=8192)
  s_pos, s_faces = torch.as_tensor(small.vertices, dtype=torch.float, device=dev), torch.as_tensor(small.faces, dtype=torch.int32, device=dev)
  pts = U.sample_surface((s_pos, s_faces), 4096, seed=0)
  rs = np.random.RandomState(0)
  w = rs.normal(size=(24, 3))
  w = w / np.linalg.norm(w, axis=1, keepdims=True) * np.radians(1.5)
  poses = np.tile(np.eye(4), (24, 1, 1))
  for k in range(24):
    K = np.array([[0, -w[k, 2], w[k, 1]], [w[k, 2], 0, -w[k, 0]], [-w[k, 1], w[k, 0], 0]])
    poses[k, :3, :3] = np.eye(3) + K + 0.5 * K @ K
    poses[k, :3, 3] = rs.normal(size=3) * 0.002
  poses = torch.as_tensor(poses.astype(np.float32), device=dev)
  res = dict(reps=args.reps, simplified=dict(vertices=len(s_pos), faces=len(s_faces)), fused=dict(vertices=len(pos), faces=len(faces)))
  for name, (p, f) in (('simplified', (s_pos, s_faces)), ('fused', (pos.float().contiguous(), faces.to(torch.int32).contiguous()))):
    for N in (1, 24):
      res[f'{name}_N{N}'] = case(pts, poses[:N].contiguous(), p, f, args.reps)
  move = np.eye(4)
  move[:3, :3] = np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])
  move[:3, 3] = (0.3, -0.2, 0.1)
  moved = U.transform_mesh((small.vertices, small.faces), np.linalg.inv(move))
  U.align_to_mesh(moved, small)               # warm-up
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  T, info = U.align_to_mesh(moved, small)
  res['align_to_mesh'] = dict(wall_ms=(time.perf_counter() - t0) * 1e3, starts=len(info['rms']), samples=info['n_points'], chosen=info['chosen'],
                              ambiguous=info['ambiguous'], rms=float(info['rms'][info['chosen']]),
                              max_abs_error_of_transform=float(np.abs(T - move).max()), stages=[list(s) for s in info['stages']])
  line = json.dumps(res)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
