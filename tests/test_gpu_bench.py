"""GPU: bench.py's plain run - exactly --steps timed steps, the headline keys and none of what --full adds - and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def test_plain_run_and_dump_outputs(tmp_path):
  r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--dump-outputs', str(tmp_path)],
                     capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stderr[-3000:]
  line = json.loads(r.stdout.strip().splitlines()[-1])
  for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'roofline'):
    assert k in line, k
  assert line['steps'] == 2 and line['warmup'] == 1
  assert line['value'] == pytest.approx(252 * 1e3 / line['ms_per_step'], rel=1e-9)
  assert not {'kernel_classes', 'ms_per_step_events_off', 'phases_ms_per_rank', 'configs3_4x252', 'tracking_configs4', 'cpu_baseline'} & set(line)
  poses, am = np.load(tmp_path / 'poses.npy'), np.load(tmp_path / 'argmax.npy')
  assert poses.shape == (252, 4, 4) and poses.dtype == np.float32 and np.isfinite(poses).all()
  assert am.shape == (1,) and am.dtype == np.float64 and am[0] == int(am[0]) and 0 <= am[0] < 252
