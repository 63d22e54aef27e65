"""Write the masks and scene_gt_info.json that a BOP-format split with ground-truth poses still lacks (foundationpose_amd.bop.annotate_scene:
bop_toolkit's calc_gt_masks.py + calc_gt_info.py on the device), one JSON line per scene.
usage: python scripts/bop_annotate.py DATASET SPLIT [--scenes 1 2 ..] [--delta 0.015] [--pad bop | N | X Y] [--overwrite]
Afterwards scripts/run_bop.py DATASET --split SPLIT runs and scores the split."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('dataset')
  ap.add_argument('split')
  ap.add_argument('--scenes', type=int, nargs='+', default=None, help='scene ids (default: every scene of the split)')
  ap.add_argument('--delta', type=float, default=0.015, help='visibility tolerance in metres (BOP: 0.015)')
  ap.add_argument('--pad', nargs='+', default=['bop'], metavar='PAD',
                  help="canvas around the frame: 'bop' (one frame a side; frames up to 640 x 480), N pixels, or X Y pixels")
  ap.add_argument('--overwrite', action='store_true', help='replace existing mask files and scene_gt_info.json')
  args = ap.parse_args(argv)
  if not args.delta >= 0:
    ap.error(f'--delta must be >= 0, got {args.delta}')
  if args.pad == ['bop']:
    args.pad = 'bop'
  else:
    if len(args.pad) > 2 or not all(p.isdigit() for p in args.pad):
      ap.error(f"--pad takes 'bop', one pixel count or two (x y), got {' '.join(args.pad)}")
    args.pad = (int(args.pad[0]), int(args.pad[-1]))
  return args


def main(argv=None):
  args = parse_args(argv)
  from foundationpose_amd import bop
  models = bop.BopModels(os.path.join(args.dataset, 'models'))
  dirs = bop._scene_dirs(args.dataset, args.split)
  missing = [s for s in (args.scenes or []) if s not in dirs]
  if missing:
    raise SystemExit(f'no scene {missing} under {os.path.join(args.dataset, args.split)} (found {sorted(dirs)})')
  for scene_id in (args.scenes or sorted(dirs)):
    info = bop.annotate_scene(dirs[scene_id], models, delta=args.delta, pad=args.pad, overwrite=args.overwrite)
    inst = [e for entries in info.values() for e in entries]
    print(json.dumps(dict(scene_id=scene_id, n_images=len(info), n_instances=len(inst),
                          n_counted=sum(e['visib_fract'] >= bop.VISIB_GT_MIN for e in inst),
                          mean_visib_fract=float(sum(e['visib_fract'] for e in inst) / len(inst)) if inst else None)))


if __name__ == '__main__':
  main()
