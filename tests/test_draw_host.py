"""CPU: the host side of drawing poses on the frame - project_3d_to_2d and model_box, the numpy restatement of the drawing rule
(tests/draw_oracle.py) on cases whose answer is known by hand, and the ctypes mirrors of fp_draw_object / fp_draw_args against the
header as a C compiler lays them out."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import draw_oracle as O

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
K = np.array([[600.0, 0.5, 320.0], [0, 610.0, 240.0], [0, 0, 1]])


@pytest.fixture(scope='module')
def built():
  import __graft_entry__ as g
  g.build()
  from foundationpose_amd import _lib
  return _lib


def test_project_3d_to_2d_is_the_formula():
  from foundationpose_amd import Utils as U, synthetic as S
  rs = np.random.RandomState(0)
  for i in range(50):
    pose = np.eye(4)
    pose[:3, :3] = S.random_rotation(np.random.RandomState(i))
    pose[:3, 3] = [rs.uniform(-0.2, 0.2), rs.uniform(-0.2, 0.2), rs.uniform(0.4, 1.5)]
    pt = np.array([*rs.uniform(-0.1, 0.1, 3), 1.0])
    cam = pose @ pt
    u = (K[0, 0] * cam[0] + K[0, 1] * cam[1] + K[0, 2] * cam[2]) / cam[2]
    v = (K[1, 1] * cam[1] + K[1, 2] * cam[2]) / cam[2]
    got = U.project_3d_to_2d(pt, K, pose)
    assert got.dtype.kind == 'i' and got.shape == (2,)
    assert abs(got[0] - u) <= 0.5 + 1e-9 and abs(got[1] - v) <= 0.5 + 1e-9
  # ties go to even, as np.round
  assert list(U.project_3d_to_2d(np.array([0.5, 1.5, 1.0, 1.0]), np.eye(3), np.eye(4))) == [0, 2]


def test_model_box_on_the_mustard_mesh():
  from foundationpose_amd import Utils as U, synthetic as S
  mesh = S.make_mustard_mesh(seed=0, n_theta=48, n_z=42)
  v = np.asarray(mesh.vertices, dtype=np.float64)
  to_origin, bbox = U.model_box(mesh)
  assert to_origin.shape == (4, 4) and bbox.shape == (2, 3)
  moved = v @ to_origin[:3, :3].T + to_origin[:3, 3]
  np.testing.assert_allclose(moved.min(0), bbox[0], atol=1e-12)
  np.testing.assert_allclose(moved.max(0), bbox[1], atol=1e-12)
  np.testing.assert_allclose(bbox[0], -bbox[1], atol=0)
  np.testing.assert_allclose(bbox[1] - bbox[0], v.max(0) - v.min(0), atol=1e-12)
  np.testing.assert_array_equal(to_origin[:3, :3], np.eye(3))
  to2, bbox2 = U.model_box(v)                                   # the vertices alone give the same
  np.testing.assert_array_equal(to2, to_origin), np.testing.assert_array_equal(bbox2, bbox)


def _one_segment(p0, p1, thickness=2.0, H=32, W=48, Kc=None):
  """The oracle on a frame of 7s with ONE segment: the x axis of an object whose origin is p0 and whose x axis ends at p1 (same z)"""
  Kc = np.array([[100.0, 0, 0], [0, 100.0, 0], [0, 0, 1]]) if Kc is None else Kc
  p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
  pose = np.eye(4)
  pose[:3, 3] = p0
  d = p1 - p0
  scale = np.linalg.norm(d)
  x = d / scale
  y = np.cross([0, 0, 1.0], x) if abs(x[2]) < 0.9 else np.cross([0, 1.0, 0], x)
  y /= np.linalg.norm(y)
  pose[:3, :3] = np.stack([x, y, np.cross(x, y)], axis=1)
  ob = O.make_object(np.zeros((2, 3)), axis_scale=scale, axis_color=((200, 100, 50), (7, 7, 7), (7, 7, 7)))
  img = np.full((H, W, 3), 7, dtype=np.uint8)
  out, _, segs = O.draw(img, Kc, pose[None], [ob], flags=O.AXES, axis_thickness=thickness)
  # the y and z axes are drawn in the colour of the frame; what the x axis touches, and the x axis alone of the segments
  touched = np.zeros((H, W), dtype=bool)
  segs = [s for s in segs if list(s['color']) == [200, 100, 50]]
  for s in segs:
    O._blend_segment(img.astype(np.float64), touched, s, 1.0)
  return out, touched, segs


def test_oracle_horizontal_two_pixel_line_covers_the_expected_rows():
  # from pixel (10, 12) to (30, 12) at z = 1
  out, touched, segs = _one_segment([0.10, 0.12, 1.0], [0.30, 0.12, 1.0], thickness=2.0)
  assert [list(s['xy'].reshape(-1)) for s in segs][0] == [10, 12, 30, 12]
  rows = np.nonzero(touched.any(axis=1))[0]
  assert list(rows) == [11, 12, 13]                             # thickness / 2 + 0.5 = 1.5: d = 0 -> 1, d = 1 -> 0.5, d = 2 -> 0
  assert list(out[12, 20]) == [200, 100, 50]
  assert list(out[11, 20]) == list(out[13, 20]) == [int(np.rint(7 + 0.5 * (c - 7))) for c in (200, 100, 50)]
  assert list(out[10, 20]) == list(out[14, 20]) == [7, 7, 7]
  assert list(np.nonzero(touched[12])[0]) == list(range(9, 32)) # the round caps reach one pixel beyond the ends
  assert (out[~touched] == 7).all()


def test_oracle_segment_behind_the_camera_draws_nothing():
  out, touched, segs = _one_segment([0.10, 0.12, -1.0], [0.30, 0.12, -1.0])
  assert segs == [] and not touched.any() and (out == 7).all()
  out, touched, segs = _one_segment([0.10, 0.12, 0.005], [0.30, 0.12, 0.009])      # in front of the camera but nearer than FP_DRAW_ZNEAR
  assert segs == [] and not touched.any()


def test_oracle_clipping_keeps_the_visible_end():
  # from (0.1, 0.12, 1) back through the near plane to z = -1: the visible end projects to (10, 12) and stays
  out, touched, segs = _one_segment([0.10, 0.12, 1.0], [0.10, 0.12, -1.0])
  assert len(segs) == 1
  np.testing.assert_array_equal(segs[0]['xy'][0], [10, 12])
  # the cut end lies on z = FP_DRAW_ZNEAR: (0.1, 0.12, 0.01) -> (1000, 1200)
  np.testing.assert_array_equal(segs[0]['xy'][1], [1000, 1200])
  assert touched[12, 10] and touched[24, 20] and list(out[24, 20]) == [200, 100, 50]      # ((12, 10) itself lies under the other two axes)
  assert touched[31, 26] or touched[31, 25]                     # it leaves the frame along the direction (10, 12) -> (1000, 1200)
  # and the other way round: the far end is the second point
  out2, touched2, segs2 = _one_segment([0.10, 0.12, -1.0], [0.10, 0.12, 1.0])
  np.testing.assert_array_equal(segs2[0]['xy'][1], [10, 12])
  np.testing.assert_array_equal(touched2, touched)
  assert list(out2[24, 20]) == [200, 100, 50]


def test_oracle_segment_order_and_far_endpoints():
  ob = O.make_object([[0.3, -0.2, 0.1], [-0.1, 0.2, 0.5]])      # (min / max are taken per component)
  segs = O.object_segments(ob)
  assert len(segs) == 15
  np.testing.assert_allclose(segs[0][0], [-0.1, -0.2, 0.1]), np.testing.assert_allclose(segs[0][1], [0.3, -0.2, 0.1])
  np.testing.assert_allclose(segs[1][0], [-0.1, -0.2, 0.5])     # x-edges: y outer, z inner
  np.testing.assert_allclose(segs[2][0], [-0.1, 0.2, 0.1])
  np.testing.assert_allclose(segs[5][0], [-0.1, -0.2, 0.5]), np.testing.assert_allclose(segs[5][1], [-0.1, 0.2, 0.5])
  np.testing.assert_allclose(segs[11][0], [0.3, 0.2, 0.1]), np.testing.assert_allclose(segs[11][1], [0.3, 0.2, 0.5])
  assert [s[3] for s in segs] == [False] * 12 + [True] * 3
  # a rounded coordinate beyond 2^20 drops the segment whole
  assert O.project_segment(np.array([0.0, 0, 1]), np.array([30.0, 0, 0.011]), np.eye(4), K) is None


def _header():
  src = open(os.path.join(REPO, 'include', 'foundationpose_amd.h')).read()
  return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_draw_export_is_declared_bound_and_exported(built):
  src = _header()
  m = re.search(r'\bint\s+fp_draw_poses\s*\(([^;]*?)\)\s*;', src, flags=re.S)
  assert m, 'fp_draw_poses is not declared in include/foundationpose_amd.h'
  n_args = len([a for a in m.group(1).split(',') if a.strip()])
  assert len(built._PROTOS['fp_draw_poses'][1]) == n_args
  assert hasattr(ctypes.CDLL(built.LIB_PATH), 'fp_draw_poses')


def test_draw_structures_match_the_header(built, tmp_path):
  """sizeof and every field offset of the two structures, and the constants, as a C compiler sees the header == the ctypes mirrors"""
  structs = (('fp_draw_object', built.FpDrawObject), ('fp_draw_args', built.FpDrawArgs))
  lines = []
  for cname, mirror in structs:
    lines.append(f'printf("%zu\\n", sizeof({cname}));')
    lines += [f'printf("%zu\\n", offsetof({cname}, {f[0]}));' for f in mirror._fields_]
  consts = ('FP_DRAW_MAX_OBJECTS', 'FP_DRAW_BOX', 'FP_DRAW_AXES', 'FP_DRAW_FILL', 'FP_DRAW_CONTOUR')
  lines += [f'printf("%d\\n", (int){c});' for c in consts] + ['printf("%.17g\\n", (double)FP_DRAW_ZNEAR);']
  prog = tmp_path / 'draw_sizes.c'
  prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "foundationpose_amd.h"\nint main(void) {\n' + '\n'.join(lines) + '\nreturn 0; }\n')
  exe = tmp_path / 'draw_sizes'
  subprocess.run(['cc', '-I', os.path.join(REPO, 'include'), str(prog), '-o', str(exe)], check=True)
  got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
  want = []
  for _, mirror in structs:
    want.append(ctypes.sizeof(mirror))
    want += [getattr(mirror, f[0]).offset for f in mirror._fields_]
  want += [getattr(built, c) for c in consts]
  assert [int(x) for x in got[:-1]] == want
  assert float(got[-1]) == built.FP_DRAW_ZNEAR == O.ZNEAR
  assert (O.BOX, O.AXES, O.FILL, O.CONTOUR) == (built.FP_DRAW_BOX, built.FP_DRAW_AXES, built.FP_DRAW_FILL, built.FP_DRAW_CONTOUR)
