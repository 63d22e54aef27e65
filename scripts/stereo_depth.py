"""Depth from a stereo pair on the command line: two image files -> a float32 depth map in metres (.npy), 0 where there is none.
  python scripts/stereo_depth.py LEFT RIGHT --K FILE --baseline M [-o depth.npy]
  python scripts/stereo_depth.py RAW_LEFT RAW_RIGHT --calibration FILE [--left-section S] [-o depth.npy]
--K: a nine-number cam_K.txt or a stereo camera's sectioned calibration file (then --camera-section picks the section, and without
--baseline the [STEREO] Baseline of that file is used, times --baseline-scale).  With --K the pair must already be rectified and
undistorted.  --calibration: the sectioned calibration file of a RAW pair - both cameras, their distortion and their relative pose are
read from it (mesh_io.load_stereo_calibration, which states how it reads the [STEREO] section: an assumption), the pair is rectified
and undistorted on the device in front of the matching, and the depth belongs to the rectified left camera, whose matrix is written
beside the depth as <out>.K.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('left')
  ap.add_argument('right')
  ap.add_argument('--K', default=None, help='intrinsics file of the left camera (a rectified pair)')
  ap.add_argument('--calibration', default=None, help='sectioned calibration file of a raw pair: rectify before matching')
  ap.add_argument('--left-section', default='LEFT_CAM_FHD1200', help='camera section of the left image with --calibration')
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
  if (args.K is None) == (args.calibration is None):
    ap.error('give --K (a rectified pair) or --calibration (a raw pair)')

  def load(path):      # a grey file stays one channel, anything else becomes RGB
    img = Image.open(path)
    return np.ascontiguousarray(np.asarray(img.convert('L' if img.mode in ('L', '1') else 'RGB')))

  left, right = load(args.left), load(args.right)
  rect = None
  if args.calibration is not None:
    from foundationpose_amd.mesh_io import load_stereo_calibration
    c = load_stereo_calibration(args.calibration, left_section=args.left_section, scale=args.baseline_scale)
    rect = U.rectify_stereo(c['K1'], c['dist1'], c['K2'], c['dist2'], c['R'], c['T'], left.shape[:2])
    K, baseline = rect.K_new, rect.baseline if args.baseline is None else args.baseline
    np.savetxt(args.out + '.K.txt', K)
  else:
    K = load_intrinsics(args.K, camera_section=args.camera_section)
    baseline = args.baseline if args.baseline is not None else load_stereo_baseline(args.K, scale=args.baseline_scale)
  depth = U.stereo_depth(left, right, K, baseline, zfar=args.zfar, rectify=rect, max_disparity=args.max_disparity, p1=args.p1, p2=args.p2, paths=args.paths,
                         lr_max=args.lr_max, min_disparity=args.min_disparity, subpixel=not args.no_subpixel)
  np.save(args.out, depth)
  valid = depth > 0
  print(f'{args.out}: {depth.shape[1]} x {depth.shape[0]}, {valid.mean():.1%} of the pixels have a depth' +
        (f', {depth[valid].min():.3f} .. {depth[valid].max():.3f} m' if valid.any() else ''))


if __name__ == '__main__':
  main()
