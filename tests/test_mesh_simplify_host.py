"""CPU: the numpy restatement of the vertex-clustering rule (tests/mesh_simplify_oracle.py) alone, on the composite mesh - a UV sphere, two
lattice sheets 0.9 mm apart with opposite faces, one isolated vertex: 22 365 vertices, above the rasteriser's 8192.  The GPU tests compare
the library with this restatement bit for bit; here the restatement is held against the consequences the header lists."""
import numpy as np
import pytest

from tests import mesh_simplify_oracle as M


@pytest.fixture(scope='module')
def mesh():
  return M.composite_mesh()


@pytest.mark.parametrize('cell', [0.0005, 0.003, 0.004, 0.010])
def test_consequences_on_the_composite_mesh(mesh, cell):
  pos, faces, normals, colors = mesh
  out = M.simplify(pos, faces, cell, normals, colors)
  ratio = M.check_consequences(pos, faces, out, cell)
  print(f"cell {cell * 1e3:g} mm: {len(out['pos'])} vertices, {len(out['faces'])} faces; dropped: {out['degenerate']} degenerate, "
        f"{out['duplicate']} duplicate faces, {out['unreferenced']} unreferenced clusters; largest displacement {ratio:.2f} cells")
  assert len(out['pos']) < len(pos) and len(out['faces']) < len(faces)
  assert len(out['faces']) == len(faces) - out['degenerate'] - out['duplicate']
  assert len(out['pos']) == out['clusters'] - out['unreferenced']
  assert out['unreferenced'] >= 1                      # the isolated vertex
  assert out['vertex_map'][-1] == -1
  assert out['normals'].shape == out['pos'].shape and out['colors'].shape == out['pos'].shape
  ln = np.linalg.norm(out['normals'].astype(np.float64), axis=1)
  assert np.all((np.abs(ln - 1) < 1e-6) | (ln == 0))
  again = M.simplify(pos, faces, cell, normals, colors)
  for k in ('pos', 'normals', 'colors', 'faces', 'vertex_map'):
    assert out[k].tobytes() == again[k].tobytes()


def test_every_branch_occurs_at_3mm(mesh):
  pos, faces, normals, colors = mesh
  out = M.simplify(pos, faces, 0.003, normals, colors)
  assert out['degenerate'] > 0 and out['duplicate'] > 0 and out['unreferenced'] > 0


def test_a_cell_below_the_spacing_returns_the_input_bits(mesh):
  pos, faces, normals, colors = mesh
  out = M.simplify(pos, faces, 1e-6, normals, colors)
  # every vertex is its own cluster; the isolated one (the last) is referenced by no face and goes
  assert out['clusters'] == len(pos) and out['degenerate'] == 0 and out['duplicate'] == 0 and out['unreferenced'] == 1
  assert out['pos'].tobytes() == pos[:-1].tobytes()
  assert out['normals'].tobytes() == normals[:-1].tobytes()
  assert out['colors'].tobytes() == colors[:-1].tobytes()
  assert out['faces'].tobytes() == faces.tobytes()
  assert (out['vertex_map'][:-1] == np.arange(len(pos) - 1)).all() and out['vertex_map'][-1] == -1


def test_point_cloud_equals_per_cell_means(mesh):
  pos = mesh[0]
  cell = np.float32(0.004)
  out = M.simplify(pos, None, cell)
  assert len(out['faces']) == 0 and out['unreferenced'] == 0 and (out['vertex_map'] >= 0).all()
  o, c, dims = M.cells(pos, cell)
  groups = {}
  for v, k in enumerate(map(tuple, c)):
    groups.setdefault(k, []).append(v)        # insertion order: by lowest member
  assert len(groups) == len(out['pos'])
  means = np.stack([pos[m].astype(np.float64).mean(0) for m in groups.values()])
  # one float32 rounding of the result and 2^-31 of fixed-point rounding per member
  tol = np.abs(pos).max() * 2.0 ** -23 + 2.0 ** -31
  assert np.abs(out['pos'].astype(np.float64) - means).max() <= tol
  assert [m[0] for m in groups.values()] == sorted(m[0] for m in groups.values())
  expect = np.empty(len(pos), dtype=np.int32)
  for g, m in enumerate(groups.values()):
    expect[m] = g
  assert (out['vertex_map'] == expect).all()


def test_search_brackets_the_budget(mesh):
  pos, faces = mesh[0], mesh[1]
  cell, lo, hi = M.search_cell(pos, faces, 2048)
  n_hi, n_lo = M.count_vertices(pos, faces, cell), M.count_vertices(pos, faces, np.float32(lo))
  print(f'max_vertices 2048: cell {float(cell) * 1e3:.4f} mm -> {n_hi} vertices; lo {lo * 1e3:.4f} mm -> {n_lo}')
  assert n_hi <= 2048 < n_lo
  assert cell == np.float32(hi) and lo < hi


def test_dims_above_2_21_are_refused(mesh):
  with pytest.raises(ValueError, match='dims'):
    M.simplify(mesh[0], mesh[1], 1e-8)
