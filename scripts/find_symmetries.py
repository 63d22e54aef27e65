"""The rotational symmetries of a model, found on the GPU (foundationpose_amd.Utils.find_symmetries): prints one JSON line with the
models_info.json keys (symmetries_discrete with translations in mm, symmetries_continuous), the number of transforms FoundationPose would
take, the largest residual of an accepted element, the centroid, the eigenvalues of the surface's covariance (three nearly equal ones: the
axes are arbitrary and the group may be incomplete) and tol.
usage: python scripts/find_symmetries.py MODEL [--tol T] [--scale S] [--max-order 12] [--angle-step 1.0] [--samples 4096] [--seed 0]
MODEL: OBJ or PLY (foundationpose_amd.mesh_io.load_mesh); --scale 0.001 for a BOP model in millimetres; T in the scaled unit (default 2 % of
the exact diameter)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_amd import Utils as U
from foundationpose_amd import mesh_io


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('model')
  ap.add_argument('--tol', type=float, default=None)
  ap.add_argument('--scale', type=float, default=1.0)
  ap.add_argument('--max-order', type=int, default=12)
  ap.add_argument('--angle-step', type=float, default=1.0)
  ap.add_argument('--samples', type=int, default=4096)
  ap.add_argument('--seed', type=int, default=0)
  args = ap.parse_args()
  mesh = mesh_io.load_mesh(args.model, scale=args.scale)
  info = U.find_symmetries(mesh, tol=args.tol, max_order=args.max_order, angle_step_deg=args.angle_step, n_samples=args.samples, seed=args.seed)
  print(json.dumps(dict(model=args.model, n_transforms=len(info['symmetry_tfs']), symmetries_discrete=info['symmetries_discrete'],
                        symmetries_continuous=info['symmetries_continuous'], max_residual=float(info['max'].max()), tol=info['tol'],
                        closed=info['closed'], centroid=info['centroid'].tolist(), eigenvalues=info['eigenvalues'].tolist(),
                        n_candidates=info['n_candidates'])))


if __name__ == '__main__':
  main()
