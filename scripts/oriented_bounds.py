"""The minimum-volume oriented box of a model, searched on the GPU (foundationpose_amd.Utils.oriented_bounds): prints one JSON line with
the extents (ascending), to_origin (4x4, row-major: it moves the model so that its box is centred at the origin and axis-aligned), the
box's volume beside the volumes of the axis-aligned box and of the box in the PCA frame, the number of candidate frames and of hull
vertices.  The box is the smallest with one face flush with a face of the convex hull; axis order and signs are this project's convention.
usage: python scripts/oriented_bounds.py MODEL [--scale S]
MODEL: OBJ or PLY (foundationpose_amd.mesh_io.load_mesh); --scale 0.001 for a BOP model in millimetres."""
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
  ap.add_argument('--scale', type=float, default=1.0)
  args = ap.parse_args()
  mesh = mesh_io.load_mesh(args.model, scale=args.scale)
  to_origin, extents, info = U.oriented_bounds(mesh, return_info=True)
  print(json.dumps(dict(model=args.model, extents=extents.tolist(), to_origin=to_origin.tolist(), volume=info['volume'],
                        aabb_volume=info['aabb_volume'], pca_volume=info['pca_volume'], n_candidates=info['n_candidates'],
                        hull_vertices=info['hull_vertices'], rank=info['rank'])))


if __name__ == '__main__':
  main()
