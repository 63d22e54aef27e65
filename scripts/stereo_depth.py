"""Depth from a rectified stereo pair on the command line: two image files -> a float32 depth map in metres (.npy), 0 where there is none.
  python scripts/stereo_depth.py LEFT RIGHT --K FILE --baseline M [-o depth.npy]
--K: a nine-number cam_K.txt or a stereo camera's sectioned calibration file (then --camera-section picks the section, and without
--baseline the [STEREO] Baseline of that file is used, times --baseline-scale).  The pair must already be rectified and undistorted."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('left')
  ap.add_argument('right')
  ap.add_argument('--K', required=True, help='intrinsics file of the left camera')
  ap.add_argument('--camera-section', default='LEFT_CAM_FHD1200')
  ap.add_argument('--baseline', type=float, default=None, help='metres')
  ap.add_argument('--baseline-scale', type=float, default=0.001, help='unit of Baseline= in a sectioned file, in metres')
  ap.add_argument('--max-disparity', type=int, default=128)
  ap.add_argument('--p1', type=int, default=8)
  ap.add_argument('--p2', type=int, default=32)
  ap.add_argument('--paths', type=lambda v: int(v, 0), default=0xFF)
  ap.add_argument('--lr-max', type=int, default=1)
  ap.add_argument('--min-disparity', type=int, default=1)
  ap.add_argument('--no-subpixel', action='store_true')
  ap.add_argument('--zfar', type=float, default=np.inf)
  ap.add_argument('-o', '--out', default='depth.npy')
  args = ap.parse_args()
  from PIL import Image
  from foundationpose_amd import Utils as U
  from foundationpose_amd.mesh_io import load_intrinsics, load_stereo_baseline
  K = load_intrinsics(args.K, camera_section=args.camera_section)
  baseline = args.baseline if args.baseline is not None else load_stereo_baseline(args.K, scale=args.baseline_scale)

  def load(path):      # a grey file stays one channel, anything else becomes RGB
    img = Image.open(path)
    return np.ascontiguousarray(np.asarray(img.convert('L' if img.mode in ('L', '1') else 'RGB')))

  left, right = load(args.left), load(args.right)
  depth = U.stereo_depth(left, right, K, baseline, zfar=args.zfar, max_disparity=args.max_disparity, p1=args.p1, p2=args.p2, paths=args.paths,
                         lr_max=args.lr_max, min_disparity=args.min_disparity, subpixel=not args.no_subpixel)
  np.save(args.out, depth)
  valid = depth > 0
  print(f'{args.out}: {depth.shape[1]} x {depth.shape[0]}, {valid.mean():.1%} of the pixels have a depth' +
        (f', {depth[valid].min():.3f} .. {depth[valid].max():.3f} m' if valid.any() else ''))


if __name__ == '__main__':
  main()
