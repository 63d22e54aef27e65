"""An RGB-D frame of a camera whose depth and colour come from two sensors, brought onto one pixel grid on the command line:
  python scripts/align_depth.py RGB DEPTH --calibration FILE --out DIR [--depth-scale 0.001] [--zfar M] [--source]
RGB: an image file of the colour sensor.  DEPTH: the depth sensor's map, a .npy of float32 metres, or a 16-bit image file whose values
times --depth-scale are metres (0.001: millimetres).  --calibration: this project's RGB-D calibration file (JSON with K_depth,
dist_depth, K_colour, dist_colour, T_colour_depth, size_depth, size_colour; INTEGRATION.md, "Aligning depth to the colour camera";
mesh_io.load_rgbd_calibration).  Written to DIR: rgb.png (undistorted when the colour sensor has distortion), depth.npy (float32 metres in
the colour camera, 0 where the depth sensor saw nothing), cam_K.txt (the camera matrix that belongs to both: what register takes) and,
with --source, source.npy (int32: per pixel the index row * W + col of the depth pixel that won, -1 where none)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('rgb')
  ap.add_argument('depth')
  ap.add_argument('--calibration', required=True)
  ap.add_argument('--out', required=True, help='directory')
  ap.add_argument('--depth-scale', type=float, default=0.001, help='metres per unit of a 16-bit depth image (a .npy is metres already)')
  ap.add_argument('--zfar', type=float, default=np.inf)
  ap.add_argument('--source', action='store_true', help='also write source.npy')
  args = ap.parse_args()
  from PIL import Image
  from foundationpose_amd import Utils as U
  from foundationpose_amd.mesh_io import load_rgbd_calibration
  rig = U.rgbd_rig(**load_rgbd_calibration(args.calibration))
  rgb = np.ascontiguousarray(np.asarray(Image.open(args.rgb).convert('RGB')))
  if args.depth.endswith('.npy'):
    depth = np.ascontiguousarray(np.load(args.depth), dtype=np.float32)
  else:
    depth = (np.asarray(Image.open(args.depth)).astype(np.float64) * args.depth_scale).astype(np.float32)
  if rgb.shape[:2] != rig.size or depth.shape != rig.size_depth:
    ap.error(f'the calibration is for a colour image of {rig.size} and a depth map of {rig.size_depth} (H, W); got {rgb.shape[:2]} and {depth.shape}')
  res = U.align_frame(rgb, depth, rig, zfar=args.zfar, return_source=args.source)
  os.makedirs(args.out, exist_ok=True)
  Image.fromarray(res[0]).save(os.path.join(args.out, 'rgb.png'))
  np.save(os.path.join(args.out, 'depth.npy'), res[1])
  np.savetxt(os.path.join(args.out, 'cam_K.txt'), rig.K)
  if args.source:
    np.save(os.path.join(args.out, 'source.npy'), res[2])
  filled = res[1] > 0
  print(f'{args.out}: {rig.size[1]} x {rig.size[0]}, {filled.mean():.1%} of the pixels have a depth' +
        (f', {res[1][filled].min():.3f} .. {res[1][filled].max():.3f} m' if filled.any() else ''))


if __name__ == '__main__':
  main()
