"""Where a model may be in a depth frame, without a mask, on the command line:
  python scripts/detect_object.py MODEL DEPTH --K FILE [--top-k 4] [--stride 4] [--depth-scale 0.001] [--views 42] [--out FILE.json] [--mask FILE.png]
MODEL: an OBJ or PLY file in metres.  DEPTH: a .npy of float32 metres, or a 16-bit image file whose values times --depth-scale are metres.
--K: a text file with the 3 x 3 camera matrix.  Depth templates of the model are matched against the whole frame on the GPU
(foundationpose_amd/detect.py; geometry only - see its limits), after register's depth prelude (erode + bilateral).  Prints one line per
detection - the centre of the model's bounding box in the camera frame, the pass fractions, the anchor pixel - and writes, with --out, the
records as JSON (pose: 4 x 4 ob_in_cam of the model as the file holds it, a rough rotation with the detected centre) and, with --mask, what
the model shows at the best record's pose in front of the frame's depth: a mask for register."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('model')
  ap.add_argument('depth')
  ap.add_argument('--K', required=True)
  ap.add_argument('--top-k', type=int, default=4)
  ap.add_argument('--stride', type=int, default=4)
  ap.add_argument('--views', type=int, default=42)
  ap.add_argument('--anchors', type=int, default=1)
  ap.add_argument('--depth-scale', type=float, default=0.001, help='metres per unit of a 16-bit depth image (a .npy is metres already)')
  ap.add_argument('--out', default=None)
  ap.add_argument('--mask', default=None)
  args = ap.parse_args()
  from foundationpose_amd import Utils as U
  from foundationpose_amd.mesh_io import load_intrinsics, load_mesh
  mesh = load_mesh(args.model)
  K = load_intrinsics(args.K)
  if args.depth.endswith('.npy'):
    depth = np.ascontiguousarray(np.load(args.depth), dtype=np.float32)
  else:
    from PIL import Image
    depth = (np.asarray(Image.open(args.depth)).astype(np.float64) * args.depth_scale).astype(np.float32)
  centre = (mesh.vertices.min(axis=0) + mesh.vertices.max(axis=0)) / 2
  centred = mesh.copy()
  centred.vertices = centred.vertices - centre
  mt = U.make_mesh_tensors(centred)
  ts = U.build_templates(mesh_tensors=mt, n_views=args.views, anchors=args.anchors)
  filtered = U.bilateral_filter_depth(U.erode_depth(depth, radius=2, device='cuda'), radius=2, device='cuda')
  found = U.detect(filtered, K, ts, top_k=args.top_k, stride=args.stride)
  to_centred = np.eye(4)
  to_centred[:3, 3] = -centre
  rows = []
  for d in found:
    print(f"centre {d['centre'][0]:+.4f} {d['centre'][1]:+.4f} {d['centre'][2]:+.4f} m   in {d['in_fraction']:.2f} out {d['out_fraction']:.2f}   "
          f"pixel (row {d['pixel'][0]}, col {d['pixel'][1]})   template {d['template']}")
    rows.append(dict(pose=(d['ob_in_cam'] @ to_centred).tolist(), centre=d['centre'].tolist(), in_fraction=d['in_fraction'], out_fraction=d['out_fraction'],
                     pixel=list(d['pixel']), template=d['template'], score=d['score']))
  if not found:
    print('no candidate: no depth inside the range of centres')
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(dict(templates=ts.n_templates, dropped=len(ts.dropped), detections=rows), f, indent=1)
  if args.mask and found:
    from PIL import Image
    H, W = depth.shape
    visib = U.scene_instances(K, H, W, mt, found[0]['ob_in_cam'][None], depth=depth, occluders='depth', want=('mask_visib',))['mask_visib']
    Image.fromarray(visib[0].cpu().numpy()).save(args.mask)


if __name__ == '__main__':
  main()
