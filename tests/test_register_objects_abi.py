"""CPU: the exports of the multi-object registration are declared in the header, bound in _lib.py with matching argument counts and
structure sizes, and exported by the library; MultiObjectTracker.register's argument checks that need no GPU."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
NEW = ('fp_register_objects', 'fp_mask_depth_stats_objects', 'fp_register_hypotheses', 'fp_register_rank')


def _header():
  src = open(os.path.join(REPO, 'include', 'foundationpose_amd.h')).read()
  return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


@pytest.fixture(scope='module')
def built():
  import __graft_entry__ as g
  g.build()
  from foundationpose_amd import _lib
  return _lib


def test_new_exports_are_declared_bound_and_exported(built):
  src = _header()
  L = ctypes.CDLL(built.LIB_PATH)
  exports = open(os.path.join(REPO, 'foundationpose_amd', 'csrc', 'exports.map')).read()
  assert re.search(r'global:\s*fp_\*;', exports)                      # (the version script exports the fp_ prefix, nothing else)
  for name in NEW:
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', src, flags=re.S)
    assert m, f'{name} is not declared in include/foundationpose_amd.h'
    n_args = len([a for a in m.group(1).split(',') if a.strip()])
    assert name in built._PROTOS and len(built._PROTOS[name][1]) == n_args, f'{name}: header has {n_args} arguments'
    assert hasattr(L, name), f'{name} missing from libfoundationpose_amd.so'


def test_structures_match_the_header(built, tmp_path):
  """sizeof of the argument structures as a C compiler lays them out == the ctypes mirrors."""
  prog = tmp_path / 'sizes.c'
  prog.write_text('#include <stdio.h>\n#include "foundationpose_amd.h"\nint main(void) { printf("%zu %zu %d %d\\n", sizeof(fp_register_object), '
                  'sizeof(fp_register_objects_args), FP_REGISTER_PASS_HYP, FP_REGISTER_MIN_VALID); return 0; }\n')
  exe = tmp_path / 'sizes'
  subprocess.run(['cc', '-I', os.path.join(REPO, 'include'), str(prog), '-o', str(exe)], check=True)
  got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
  assert got == [ctypes.sizeof(built.FpRegisterObject), ctypes.sizeof(built.FpRegisterObjectsArgs), built.FP_REGISTER_PASS_HYP,
                 built.FP_REGISTER_MIN_VALID]


def _fake_estimator(ctx, refine_handle=1, score_handle=2):
  net = lambda h: types.SimpleNamespace(ctx=ctx, model=types.SimpleNamespace(handle=ctypes.c_void_p(h)))
  return types.SimpleNamespace(refiner=net(refine_handle), scorer=net(score_handle), dist_group=None, pose_last=None)


def test_register_argument_checks_need_no_gpu():
  from foundationpose_amd.tracking import MultiObjectTracker
  ctx = types.SimpleNamespace()
  tracker = MultiObjectTracker([_fake_estimator(ctx), _fake_estimator(ctx)])
  H, W = 6, 8
  rgb, depth = np.zeros((H, W, 3), dtype=np.uint8), np.ones((H, W), dtype=np.float32)
  mask, image = np.ones((H, W), dtype=bool), np.zeros((H, W), dtype=np.int32)
  K = np.eye(3)
  for kw, msg in ((dict(masks=[mask]), '1 masks for 2 objects'), (dict(masks=[mask, mask[:, :-1]]), 'mask 1 is .* shapes differ'),
                  (dict(masks=image), 'needs labels='), (dict(masks=[mask, mask], labels=[1, 2]), 'not with a list of masks'),
                  (dict(masks=image, labels=[3, 3]), 'label is repeated'), (dict(masks=image, labels=[3]), '1 labels for 2 objects'),
                  (dict(masks=image[1:], labels=[1, 2]), 'label image is .* shapes differ')):
    with pytest.raises(ValueError, match=msg):
      tracker.register(rgb, depth, K, **kw)
  with pytest.raises(ValueError, match="estimator 1 does not share estimator 0's scorer"):
    MultiObjectTracker([_fake_estimator(ctx), _fake_estimator(ctx, score_handle=3)]).register(rgb, depth, K, [mask, mask])
  # the constructor still accepts estimators with different scorers: tracking needs only the refiner
  assert len(MultiObjectTracker([_fake_estimator(ctx), _fake_estimator(ctx, score_handle=3)]).estimators) == 2
