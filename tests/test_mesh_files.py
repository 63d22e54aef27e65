"""CPU: model files - Stanford PLY (ascii / binary), OBJ with its .mtl texture, load_mesh - and the angle-weighted vertex normals
against analytic ones."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from foundationpose_amd import mesh_io as M
from foundationpose_amd import synthetic as S

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

QUAD_PLY = """ply
format ascii 1.0
comment a unit square with colours and normals
element vertex 4
property float x
property float y
property float z
property float nx
property float ny
property float nz
property uchar red
property uchar green
property uchar blue
element face 1
property list uchar int vertex_indices
end_header
0 0 0 0 0 1 255 0 0
1 0 0 0 0 1 0 255 0
1 1 0.5 0 0 1 0 0 255
0 1 0 0 0 1 10 20 30
4 0 1 2 3
"""


def _write(path, text):
  with open(path, 'w') as f:
    f.write(text)
  return str(path)


def test_import_does_not_load_pil():
  code = 'import sys, foundationpose_amd, foundationpose_amd.mesh_io, foundationpose_amd.bop; assert "PIL" not in sys.modules'
  subprocess.run([sys.executable, '-c', code], check=True, cwd=REPO)


def test_handwritten_ascii_ply(tmp_path):
  mesh = M.load_ply(_write(tmp_path / 'quad.ply', QUAD_PLY))
  assert np.array_equal(mesh.vertices, [[0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, 0]]) and mesh.vertices.dtype == np.float64
  assert np.array_equal(mesh.faces, [[0, 1, 2], [0, 2, 3]]) and mesh.faces.dtype == np.int64        # the quad as a fan, as load_obj does
  assert np.array_equal(mesh.vertex_normals, np.tile([0.0, 0.0, 1.0], (4, 1)))
  assert np.array_equal(mesh.visual.vertex_colors, [[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255], [10, 20, 30, 255]])
  assert mesh.visual.vertex_colors.dtype == np.uint8


@pytest.mark.parametrize('binary', [True, False])
def test_round_trip_coloured(tmp_path, binary):
  mesh = S.make_mustard_mesh(seed=0)
  path = str(tmp_path / 'm.ply')
  M.save_ply(mesh, path, binary=binary)
  back = M.load_ply(path)
  assert np.array_equal(back.vertices, mesh.vertices.astype(np.float32).astype(np.float64))
  assert np.array_equal(back.faces, mesh.faces)
  assert np.array_equal(back.visual.vertex_colors, mesh.visual.vertex_colors)
  assert np.array_equal(back.vertex_normals, mesh.vertex_normals.astype(np.float32).astype(np.float64))
  # without normals in the file they are computed from the geometry that was read
  M.save_ply(mesh, path, binary=binary, normals=False)
  back = M.load_ply(path)
  assert np.array_equal(back.vertex_normals, S.angle_weighted_vertex_normals(back.vertices, back.faces))


@pytest.mark.parametrize('binary', [True, False])
def test_round_trip_textured_through_texture_file_comment(tmp_path, binary):
  from PIL import Image
  mesh = S.make_mustard_mesh(seed=0, textured=True)
  Image.fromarray(mesh.visual.image).save(str(tmp_path / 'tex.png'))
  path = str(tmp_path / 'm.ply')
  M.save_ply(mesh, path, binary=binary, texture_file='tex.png')
  assert b'comment TextureFile tex.png' in open(path, 'rb').read(400)
  back = M.load_ply(path)
  assert np.array_equal(back.vertices, mesh.vertices.astype(np.float32).astype(np.float64)) and np.array_equal(back.faces, mesh.faces)
  assert np.array_equal(back.visual.uv, mesh.visual.uv.astype(np.float32).astype(np.float64))
  assert np.array_equal(back.visual.image, mesh.visual.image) and back.visual.image.dtype == np.uint8
  # an explicit image wins; a missing file leaves the grey default
  other = np.full((4, 4, 3), 7, np.uint8)
  assert np.array_equal(M.load_ply(path, texture_image=other).visual.image, other)
  os.remove(str(tmp_path / 'tex.png'))
  plain = M.load_ply(path)
  assert not hasattr(plain.visual, 'uv') and np.array_equal(plain.visual.vertex_colors, np.tile([128, 128, 128, 255], (len(mesh.vertices), 1)))


def _binary_ply(path, order, count_type, index_type, faces, extra_vertex_prop=False, unknown_element=False):
  """A tetrahedron-like 5-point PLY written by hand with struct."""
  names = {'B': 'uchar', 'H': 'ushort', 'i': 'int', 'I': 'uint', 'h': 'short'}
  verts = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 1.0)]
  head = ['ply', 'format binary_%s_endian 1.0' % ('little' if order == '<' else 'big')]
  if unknown_element:
    head += ['element material 2', 'property int id', 'property list uchar float params']
  head += ['element vertex 5', 'property float x', 'property double y', 'property float32 z']
  if extra_vertex_prop:
    head += ['property float quality', 'property int16 flags']
  head += ['element face %d' % len(faces), 'property list %s %s vertex_index' % (names[count_type], names[index_type]), 'end_header']
  body = b''
  if unknown_element:
    body += struct.pack(order + 'iB2f', 7, 2, 0.5, 0.25) + struct.pack(order + 'iB', 8, 0)
  for k, (x, y, z) in enumerate(verts):
    body += struct.pack(order + 'fdf', x, y, z)
    if extra_vertex_prop:
      body += struct.pack(order + 'fh', 0.1 * k, k)
  for f in faces:
    body += struct.pack(order + count_type + index_type * len(f), len(f), *f)
  with open(path, 'wb') as fh:
    fh.write(('\n'.join(head) + '\n').encode('ascii') + body)
  return str(path)


@pytest.mark.parametrize('order', ['<', '>'])
@pytest.mark.parametrize('count_type,index_type', [('B', 'i'), ('B', 'I'), ('H', 'I'), ('H', 'i')])
def test_binary_index_and_count_types(tmp_path, order, count_type, index_type):
  tris = [(0, 1, 2), (0, 2, 3), (1, 4, 2)]
  mesh = M.load_ply(_binary_ply(tmp_path / 't.ply', order, count_type, index_type, tris))
  assert np.array_equal(mesh.vertices, [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]])
  assert np.array_equal(mesh.faces, tris)
  # a quad among triangles: rows of different lengths
  mesh = M.load_ply(_binary_ply(tmp_path / 'q.ply', order, count_type, index_type, [(0, 1, 2), (0, 1, 4, 2), (1, 4, 2)]))
  assert np.array_equal(mesh.faces, [(0, 1, 2), (0, 1, 4), (0, 4, 2), (1, 4, 2)])


def test_unknown_element_and_unknown_vertex_property_are_skipped(tmp_path):
  tris = [(0, 1, 2), (0, 2, 3)]
  mesh = M.load_ply(_binary_ply(tmp_path / 'u.ply', '<', 'B', 'i', tris, extra_vertex_prop=True, unknown_element=True))
  assert np.array_equal(mesh.vertices[4], [1, 1, 1]) and np.array_equal(mesh.faces, tris)
  text = QUAD_PLY.replace('element face 1', 'property float quality\nelement face 1')
  text = text.replace('element vertex 4', 'element material 1\nproperty float shininess\nelement vertex 4')
  lines = text.split('\n')
  h = lines.index('end_header')
  body = ['0.5'] + [ln + ' 0.25' for ln in lines[h + 1:h + 5]] + lines[h + 5:]
  mesh = M.load_ply(_write(tmp_path / 'u_ascii.ply', '\n'.join(lines[:h + 1] + body)))
  assert np.array_equal(mesh.vertices[2], [1, 1, 0.5]) and np.array_equal(mesh.faces, [[0, 1, 2], [0, 2, 3]])


def test_malformed_files_raise_value_error(tmp_path):
  mesh = S.make_mustard_mesh(seed=0, n_theta=16, n_z=12)
  path = str(tmp_path / 'm.ply')
  M.save_ply(mesh, path, binary=True)
  raw = open(path, 'rb').read()
  for cut in (7, 5000):                                   # inside the face rows, inside the vertex rows
    with open(path, 'wb') as f:
      f.write(raw[:-cut])
    with pytest.raises(ValueError, match='truncated'):
      M.load_ply(path)
  with pytest.raises(ValueError, match='truncated'):
    M.load_ply(_write(tmp_path / 'short.ply', QUAD_PLY.rsplit('\n', 3)[0] + '\n'))
  with pytest.raises(ValueError, match='format'):
    M.load_ply(_write(tmp_path / 'fmt.ply', QUAD_PLY.replace('format ascii 1.0', 'format binary_middle_endian 1.0')))
  with pytest.raises(ValueError, match='x, y, z'):
    M.load_ply(_write(tmp_path / 'noz.ply', QUAD_PLY.replace('property float z\n', 'property float w\n')))
  with pytest.raises(ValueError, match='outside'):
    M.load_ply(_write(tmp_path / 'idx.ply', QUAD_PLY.replace('4 0 1 2 3', '4 0 1 2 9')))
  with pytest.raises(ValueError):
    M.load_ply(_write(tmp_path / 'not.ply', 'solid\n'))


# ---------------------------------------------------------------------------------------------- OBJ + MTL
TEXTURED_OBJ = """mtllib a.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0 0
vt 1 0
vt 1 1
vt 0 1
usemtl m
f 1/1 2/2 3/3 4/4
"""
MTL = """newmtl other
Kd 1 1 1
map_Kd missing.png
newmtl m
Kd 0.8 0.8 0.8
map_Kd -s 1 1 1 tex.png
"""


def _texture():
  rs = np.random.RandomState(3)
  return (rs.uniform(0, 255, (16, 8, 3))).astype(np.uint8)


def test_obj_follows_mtllib_to_the_texture(tmp_path):
  from PIL import Image
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  tex = _texture()
  Image.fromarray(tex).save(str(tmp_path / 'tex.png'))
  _write(tmp_path / 'a.mtl', MTL)
  path = _write(tmp_path / 'a.obj', TEXTURED_OBJ)
  mesh = M.load_obj(path)
  assert np.array_equal(mesh.visual.image, tex)
  want = M.load_obj(path, texture_image=tex)
  a, b = make_mesh_tensors(mesh, device='cpu'), make_mesh_tensors(want, device='cpu')
  assert sorted(a) == sorted(b) == ['faces', 'pos', 'tex', 'uv', 'uv_idx', 'vnormals']
  for k in a:
    assert a[k].dtype == b[k].dtype and np.array_equal(a[k].numpy(), b[k].numpy()), k
  # an explicit image still wins
  other = np.zeros((2, 2, 3), np.uint8)
  assert np.array_equal(M.load_obj(path, texture_image=other).visual.image, other)
  # load_mesh dispatches on the extension, any case, and scales
  os.rename(path, str(tmp_path / 'B.OBJ'))
  scaled = M.load_mesh(str(tmp_path / 'B.OBJ'), scale=1e-3)
  assert np.array_equal(scaled.vertices, mesh.vertices * 1e-3) and np.array_equal(scaled.visual.image, tex)
  with pytest.raises(ValueError, match='extension'):
    M.load_mesh(str(tmp_path / 'a.stl'))


@pytest.mark.parametrize('missing', ['image', 'mtl', 'material_map'])
def test_obj_with_missing_texture_parts_is_untextured_not_an_error(tmp_path, missing):
  from PIL import Image
  if missing != 'image':
    Image.fromarray(_texture()).save(str(tmp_path / 'tex.png'))
  if missing != 'mtl':
    _write(tmp_path / 'a.mtl', MTL if missing != 'material_map' else 'newmtl m\nKd 1 1 1\n')
  mesh = M.load_obj(_write(tmp_path / 'a.obj', TEXTURED_OBJ))
  assert not hasattr(mesh.visual, 'uv')
  assert np.array_equal(mesh.vertices, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]) and np.array_equal(mesh.faces, [[0, 1, 2], [0, 2, 3]])
  assert np.array_equal(mesh.visual.vertex_colors, np.tile([128, 128, 128, 255], (4, 1)))


def test_obj_without_mtllib_is_what_it_was(tmp_path):
  """The values load_obj returned before it knew about mtllib, written out."""
  coloured = 'v 0 0 0 1 0 0\nv 1 0 0 0 0.5 0\nv 0 1 0 0 0 1\nv 0 0 1 0.25 0.25 0.25\nf 1 2 3\nf -4 -2 -1\n'
  mesh = M.load_obj(_write(tmp_path / 'c.obj', coloured))
  assert np.array_equal(mesh.vertices, [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]) and mesh.vertices.dtype == np.float64
  assert np.array_equal(mesh.faces, [[0, 1, 2], [0, 2, 3]]) and mesh.faces.dtype == np.int64
  assert np.array_equal(mesh.visual.vertex_colors, [[255, 0, 0, 255], [0, 127, 0, 255], [0, 0, 255, 255], [63, 63, 63, 255]])
  assert mesh.visual.vertex_colors.dtype == np.uint8 and mesh._vn is None
  # texture coordinates without a library: vertices split per (v, vt) pair, no texture, grey
  uv_obj = 'v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nvt 1 1\nf 1/1 2/2 3/3\nf 1/4 3/3 2/2\n'
  mesh = M.load_obj(_write(tmp_path / 'u.obj', uv_obj))
  assert np.array_equal(mesh.vertices, [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0]])
  assert np.array_equal(mesh.faces, [[0, 1, 2], [3, 2, 1]])
  assert not hasattr(mesh.visual, 'uv') and np.array_equal(mesh.visual.vertex_colors, np.tile([128, 128, 128, 255], (4, 1)))
  tex = _texture()
  mesh = M.load_obj(str(tmp_path / 'u.obj'), texture_image=tex)
  assert np.array_equal(mesh.visual.uv, [[0, 0], [1, 0], [0, 1], [1, 1]]) and mesh.visual.image is not None
  assert np.array_equal(mesh.visual.image, tex)


# ---------------------------------------------------------------------------------------------- vertex normals
def _uv_sphere(n, radius=0.7):
  """n meridians, n / 2 - 1 rings between the poles."""
  rings = n // 2 - 1
  verts = [(0.0, 0.0, radius)]
  for r in range(1, rings + 1):
    phi = np.pi * r / (rings + 1)
    verts += [(radius * np.sin(phi) * np.cos(2 * np.pi * k / n), radius * np.sin(phi) * np.sin(2 * np.pi * k / n), radius * np.cos(phi))
              for k in range(n)]
  verts.append((0.0, 0.0, -radius))
  ring = lambda r, k: 1 + (r - 1) * n + k % n
  faces = [(0, ring(1, k), ring(1, k + 1)) for k in range(n)]
  for r in range(1, rings):
    for k in range(n):
      faces += [(ring(r, k), ring(r + 1, k), ring(r + 1, k + 1)), (ring(r, k), ring(r + 1, k + 1), ring(r, k + 1))]
  last = len(verts) - 1
  faces += [(last, ring(rings, k + 1), ring(rings, k)) for k in range(n)]
  return np.array(verts), np.array(faces)


@pytest.mark.parametrize('n', [16, 48])
def test_vertex_normals_of_a_sphere_are_radial_within_the_facet_half_angle(n):
  """On a sphere the normal is position / radius.  Every facet around a vertex of the tessellation spans at most one step of
  2 pi / n in longitude and latitude, so each facet normal - and with it any positive combination of them - lies within the facet
  half-angle pi / n of the radial direction at that vertex."""
  v, f = _uv_sphere(n)
  got = S.angle_weighted_vertex_normals(v, f)
  want = v / np.linalg.norm(v, axis=1, keepdims=True)
  assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-12)
  angle = np.arccos(np.clip((got * want).sum(1), -1, 1))
  print(f'n={n}: max angle {angle.max():.4f} rad, bound {np.pi / n:.4f}')
  assert angle.max() < np.pi / n
  assert angle[[0, -1]].max() < 1e-9                     # (the poles: radial by symmetry)


def test_vertex_normal_of_an_asymmetric_fan_by_hand():
  """Three triangles around the origin, angle weights pi/4, pi/2, pi/4:
     (o, a, b): a = (1,0,0), b = (1,1,0)   normal (0,0,1),         angle(a, b) = pi/4
     (o, b, c): c = (0,0,2)                normal (1,-1,0)/sqrt2,  angle(b, c) = pi/2
     (o, c, d): d = (-1,0,1)               normal (0,-1,0),        angle(c, d) = pi/4"""
  v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 0, 2], [-1, 0, 1]], dtype=np.float64)
  f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4]])
  s = np.pi / 4 * np.array([0, 0, 1.0]) + np.pi / 2 * np.array([1.0, -1.0, 0]) / np.sqrt(2) + np.pi / 4 * np.array([0, -1.0, 0])
  got = S.angle_weighted_vertex_normals(v, f)
  assert np.allclose(got[0], s / np.linalg.norm(s), atol=1e-14)
  # vertex 1 belongs to the first triangle only: its normal, whatever the weight
  assert np.allclose(got[1], [0, 0, 1], atol=1e-14)
  # SimpleMesh computes them lazily with the same function
  assert np.array_equal(S.SimpleMesh(v, f).vertex_normals, got)
