"""CPU: the host part of foundationpose_amd/csrc/view_geom.h - the camera and the rigid transforms every depth toolkit and aligner hands
to its kernels - computed by a stand-alone program that is compiled against the header alone: no HIP, no GPU.

The expected bit patterns are a numpy restatement of the header's rules: fx, fy, cx, cy are K[0][0], K[1][1], K[0][2], K[1][2] rounded to
float32; rigid_of is the upper 3 x 4 of the matrix rounded to float32; rigid_inverse_of is the transposed rotation and
t[i] = -((m[0][i] m[0][3] + m[1][i] m[1][3]) + m[2][i] m[2][3]) in float64 in that order, rounded once.  The matrices have no zero entry
in the rotation and translations of mixed signs between 1e-3 and 10, and fx != fy, cx != cy: a swapped index shows.  The same program is
built once more with the address and undefined-behaviour sanitizers and run as its own process."""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CSRC = os.path.join(REPO, 'foundationpose_amd', 'csrc')

PROGRAM = r'''
#include <stdio.h>
#include <string.h>
#include "view_geom.h"
static void put(const float *f, int n) {
  for (int i = 0; i < n; ++i) {
    unsigned u;
    memcpy(&u, &f[i], 4);
    printf(" %08x", u);
  }
}
int main() {
  double K[9], m[FP_TSDF_MAX_VIEWS * 16];
  int H, W, n;
  for (int i = 0; i < 9; ++i)
    if (scanf("%lf", &K[i]) != 1) return 1;
  if (scanf("%d %d %d", &H, &W, &n) != 3 || n < 0 || n > FP_TSDF_MAX_VIEWS) return 1;
  for (int i = 0; i < n * 16; ++i)
    if (scanf("%lf", &m[i]) != 1) return 1;
  const Pinhole c = pinhole_of(K, H, W);
  printf("P");
  put(&c.fx, 1), put(&c.fy, 1), put(&c.cx, 1), put(&c.cy, 1);
  printf(" %d %d\n", c.H, c.W);
  const Rigids fw = rigids_of(m, n, false), inv = rigids_of(m, n, true);
  for (int v = 0; v < FP_TSDF_MAX_VIEWS; ++v) {
    const Rigid a = v < n ? rigid_of(m + v * 16) : Rigid{}, b = v < n ? rigid_inverse_of(m + v * 16) : Rigid{};
    if (memcmp(&a, &fw.v[v], sizeof(Rigid)) || memcmp(&b, &inv.v[v], sizeof(Rigid))) return 2;      // the filler is the two functions, then zeros
    if (v >= n) continue;
    printf("F"), put(a.r, 9), put(a.t, 3), printf("\nI"), put(b.r, 9), put(b.t, 3), printf("\n");
  }
  return 0;
}
'''

K = np.array([[412.3456789, 0, 17.30517578125 + 1e-9], [0, 515.43209876, 11.7091064453125 - 1e-9], [0, 0, 1.0]])
H, W = 31, 33


def _matrices():
  """camera-to-object matrices: rotations about skew axes by angles that leave no zero entry, translations of mixed signs, 1e-3 .. 10"""
  out = []
  for axis, angle, t in (((0.3, -0.5, 0.81), 0.7, (1.25e-3, -9.7531, 0.31)), ((-0.6, 0.2, 0.4), 2.1, (-3.4567, 2.5e-3, 7.1253)),
                         ((0.1, 0.9, -0.3), -1.3, (0.0421, -0.77, -1.0e-2))):
    a = np.array(axis) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx
    m[:3, 3] = t
    assert (m[:3, :3] != 0).all() and (np.abs(m[:3, 3]) >= 1e-3).all() and (np.abs(m[:3, 3]) <= 10).all()
    out.append(m)
  return np.stack(out)


def _hex(x):
  return ' '.join(f'{w:08x}' for w in np.asarray(x, np.float32).reshape(-1).view(np.uint32))


def _want(K, H, W, ms):
  lines = ['P ' + _hex([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]) + f' {H} {W}']
  for m in ms:
    lines.append('F ' + _hex(m[:3, :3]) + ' ' + _hex(m[:3, 3]))
    t = [-((m[0, i] * m[0, 3] + m[1, i] * m[1, 3]) + m[2, i] * m[2, 3]) for i in range(3)]      # float64, rounded once by _hex
    lines.append('I ' + _hex(m[:3, :3].T) + ' ' + _hex(t))
  return lines


def _build(d, *flags):
  """The compiler beside the hipcc the Makefile names (ROCm's clang++), on view_geom.h alone; not contracted, like the library."""
  hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC \?= (\S+)', open(os.path.join(CSRC, 'Makefile')).read(), flags=re.M).group(1)
  cxx = os.path.join(os.path.dirname(hipcc), 'amdclang++')
  src, exe = d / 'geom.cc', d / ('geom' + ''.join(flags).replace('=', '_').replace(',', '_'))
  src.write_text(PROGRAM)
  subprocess.run([cxx, '-std=c++17', '-O1', '-ffp-contract=off', '-Wall', '-Werror', *flags, '-I', CSRC, str(src), '-o', str(exe)], check=True)
  return str(exe)


def _run(exe, K, H, W, ms):
  text = ' '.join(repr(float(x)) for x in K.reshape(-1)) + f'\n{H} {W} {len(ms)}\n' + ' '.join(repr(float(x)) for x in ms.reshape(-1)) + '\n'
  p = subprocess.run([exe], input=text, capture_output=True, text=True)
  assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
  return p.stdout.split('\n')[:-1]


@pytest.fixture(scope='module')
def build_dir(tmp_path_factory):
  return tmp_path_factory.mktemp('view_geom')


def test_camera_and_transforms_have_the_restated_bits(build_dir):
  ms = _matrices()
  assert K[0, 0] != K[1, 1] and K[0, 2] != K[1, 2]
  # every number asked of the program needs its rounding: none is a float32 already
  assert all(float(np.float32(x)) != x for x in (K[0, 0], K[1, 1], K[0, 2], K[1, 2])) and (ms[:, :3].astype(np.float32) != ms[:, :3]).all()
  got = _run(_build(build_dir), K, H, W, ms)
  assert got == _want(K, H, W, ms)
  # the inverse is the inverse: R^T (R p + t) + t' = p to rounding
  for m, line in zip(ms, got[2::2]):
    w = np.array([int(x, 16) for x in line.split()[1:]], np.uint32).view(np.float32).astype(np.float64)
    inv = np.eye(4)
    inv[:3, :3], inv[:3, 3] = w[:9].reshape(3, 3), w[9:]
    assert np.abs(inv @ m - np.eye(4)).max() < 1e-5


def test_no_views_and_the_full_table(build_dir):
  exe = _build(build_dir)
  assert _run(exe, K, H, W, np.zeros((0, 4, 4))) == _want(K, H, W, [])
  ms = np.concatenate([_matrices()] * 22)[:64]
  assert _run(exe, K, 5, 7, ms) == _want(K, 5, 7, ms)


def test_the_program_is_clean_under_the_sanitizers(build_dir):
  ms = np.concatenate([_matrices()] * 22)[:64]
  exe = _build(build_dir, '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g')
  assert _run(exe, K, H, W, ms) == _want(K, H, W, ms)
