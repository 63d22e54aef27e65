"""How far apart two meshes are: Chamfer and Hausdorff distance and precision / recall / F-score at thresholds, measured on the GPU with
exact point-to-triangle distances (foundationpose_amd.Utils.mesh_distance).  A is the mesh under test (a reconstruction, a
simplification), B the one it is compared to (the CAD model): precision is the share of A's points within tau of B, recall the share of
B's points within tau of A.  Prints one JSON line; distances are in the unit of the files.
usage: python scripts/mesh_distance.py A B [--samples 100000] [--tau 0.001 0.002 0.005] [--seed 0] [--no-vertices] [--scale-a S] [--scale-b S] [--align]
--align first lays A onto B rigidly (Utils.align_to_mesh: for two meshes of one object in different frames; A the partial surface, B the
complete one) and adds the transform `B from A`, the start that was chosen and the starts that fit nearly as well (a symmetric B).
A and B: OBJ or PLY (foundationpose_amd.mesh_io.load_mesh)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_amd import Utils as U
from foundationpose_amd import mesh_io


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('a')
  ap.add_argument('b')
  ap.add_argument('--samples', type=int, default=100_000)
  ap.add_argument('--tau', type=float, nargs='+', default=[0.001, 0.002, 0.005])
  ap.add_argument('--seed', type=int, default=0)
  ap.add_argument('--no-vertices', action='store_true')
  ap.add_argument('--scale-a', type=float, default=1.0)
  ap.add_argument('--scale-b', type=float, default=1.0)
  ap.add_argument('--align', action='store_true')
  args = ap.parse_args()
  a, b = mesh_io.load_mesh(args.a, scale=args.scale_a), mesh_io.load_mesh(args.b, scale=args.scale_b)
  res = U.mesh_distance(a, b, n_samples=args.samples, seed=args.seed, taus=args.tau, use_vertices=not args.no_vertices, align=args.align)
  if args.align:
    info = res.pop('align_info')
    res.update(a_to_b_transform=res['a_to_b_transform'].tolist(), align_chosen=info['chosen'], align_ambiguous=info['ambiguous'],
               align_rms=float(info['rms'][info['chosen']]))
  print(json.dumps(dict(a=args.a, b=args.b, **res)))


if __name__ == '__main__':
  main()
