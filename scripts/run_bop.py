"""Register every target of a BOP-format split, write the BOP results CSV and print the BOP-19 recalls as one JSON line
(foundationpose_amd.bop: run_bop + write_results + evaluate_results).
usage: python scripts/run_bop.py DATASET_DIR [--split test] [--weights-root DIR] [--out-csv est.csv] [--out-json scores.json]
                                 [--iteration 5] [--diameter info|exact|sampled] [--max-objects 8] [--no-eval]
The refiner's and the scorer's weights are the run directories config.load_run_dir finds under --weights-root."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_amd import bop
from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
from foundationpose_amd.predict_score import ScorePredictor


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('dataset_dir')
  ap.add_argument('--split', default='test')
  ap.add_argument('--weights-root', default=None)
  ap.add_argument('--out-csv', default='bop_results.csv')
  ap.add_argument('--out-json', default=None)
  ap.add_argument('--iteration', type=int, default=5)
  ap.add_argument('--diameter', choices=['info', 'exact', 'sampled'], default='info')
  ap.add_argument('--max-objects', type=int, default=None)
  ap.add_argument('--no-eval', action='store_true')
  ap.add_argument('--polish', action='store_true', help='move the registered poses onto the depth by geometry alone (fp_pose_polish)')
  args = ap.parse_args()
  models = bop.BopModels(os.path.join(args.dataset_dir, 'models'))
  refiner, scorer = PoseRefinePredictor(weights_root=args.weights_root), ScorePredictor(weights_root=args.weights_root)
  rows = bop.run_bop(args.dataset_dir, args.split, models, refiner, scorer, iteration=args.iteration,
                     diameter=None if args.diameter == 'sampled' else args.diameter, max_objects=args.max_objects, polish=args.polish)
  bop.write_results(args.out_csv, rows)
  res = dict(n_rows=len(rows), csv=args.out_csv)
  if not args.no_eval:
    ev = bop.evaluate_results(args.dataset_dir, args.split, models, args.out_csv)
    res.update({k: v for k, v in ev.items() if k not in ('recalls', 'per_object')})
    res['per_object'] = {str(o): {k: v for k, v in r.items() if k != 'recalls'} for o, r in ev['per_object'].items()}
  line = json.dumps(res)
  print(line)
  if args.out_json:
    with open(args.out_json, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
