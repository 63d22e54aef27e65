"""Render lattice cases of tests/tools/raster_ref.py at 1, 2 and 5 hypotheses and print one JSON line {case: {N: sha1 of every output}} (used by
tests/test_gpu_raster_exact.py in child processes whose FP_RENDER_* knobs - read once per process - select another launch form)."""
import hashlib, json, os, sys
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..', '..')))
import numpy as np


def digests(names):
  from foundationpose_amd import Utils as U
  from tests.tools import raster_ref as R
  from tests.test_raster_ref_host import render_case
  out = {}
  for name in names:
    c = R.lattice_case(name)
    out[name] = {}
    for n in (1, 2, 5):
      g = render_case(U.nvdiffrast_render, c, n, dev='cuda')
      h = hashlib.sha1()
      for k in ('rast', 'xyz', 'depth', 'color'):
        h.update(np.ascontiguousarray(g[k]).tobytes())
      out[name][str(n)] = h.hexdigest()
  return out


if __name__ == '__main__':
  print('DIGESTS ' + json.dumps(digests(sys.argv[1:])))
