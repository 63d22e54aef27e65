"""CPU: the numpy / scipy restatement of the connected-components rule (tests/mesh_components_oracle.py) against a pure-Python union-find,
against reconstruct.largest_component, and at the tie and threshold boundaries of the selection."""
import numpy as np
import pytest

from tests import mesh_components_oracle as C
from tests import mesh_simplify_oracle as M


@pytest.mark.parametrize('name', sorted(C.small_cases()))
def test_labels_agree_with_a_plain_union_find(name):
  V, faces = C.small_cases()[name]
  label, number = C.labels(faces, V)
  assert label.tobytes() == C.union_find_labels(faces, V).tobytes()
  roots = np.nonzero(label == np.arange(V))[0]
  assert (number[roots] == np.arange(len(roots))).all()          # numbered by the lowest member, ascending
  assert (label[label] == label).all() and (label <= np.arange(V)).all()


def test_small_cases_by_hand():
  cases = C.small_cases()
  V, f = cases['bow_tie']
  out = C.components(np.zeros((V, 3)), f, keep='all')
  assert out['labels'].tolist() == [0] * 5 and out['stats'].tolist() == [[5, 2]] and out['counts'] == (1, 1, 5, 2)
  V, f = cases['isolated']
  out = C.components(np.zeros((V, 3)), f, keep='all')
  assert out['labels'].tolist() == [0, 1, 1, 1, 4, 5, 5, 5, 8]
  assert out['stats'].tolist() == [[1, 0], [3, 1], [1, 0], [3, 1], [1, 0]]
  assert out['vertex_map'].tolist() == [-1, 0, 1, 2, -1, 3, 4, 5, -1] and out['faces'].tolist() == [[0, 1, 2], [5, 3, 4]]
  assert out['counts'] == (5, 2, 6, 2)
  V, f = cases['degenerate']
  out = C.components(np.zeros((V, 3)), f, keep='all')
  # 0-1, 2-3, 3-0 -> {0,1,2,3} with faces [0,1,1], [2,2,3], [3,0,0]; {4,6} with [6,4,6]; {5} with [5,5,5]; {7} without a face
  assert out['labels'].tolist() == [0, 0, 0, 0, 4, 5, 4, 7]
  assert out['stats'].tolist() == [[4, 3], [2, 1], [1, 1], [1, 0]]
  assert out['kept'].tolist() == [True, True, True, False] and len(out['faces']) == 5
  V, f = cases['repeated']
  out = C.components(np.zeros((V, 3)), f)
  assert out['stats'].tolist() == [[3, 3], [1, 0], [3, 2]] and out['kept'].tolist() == [True, False, False]
  assert out['faces'].tolist() == [[0, 1, 2], [2, 1, 0], [0, 1, 2]]
  V, f = cases['no_faces']
  out = C.components(np.zeros((V, 3)), f)
  assert out['counts'] == (V, 0, 0, 0) and out['labels'].tolist() == [0, 1, 2, 3] and (out['vertex_map'] == -1).all()
  assert out['pos'].shape == (0, 3) and out['faces'].shape == (0, 3) and out['stats'].tolist() == [[1, 0]] * 4
  assert C.components(np.zeros((0, 3)), None)['counts'] == (0, 0, 0, 0)


@pytest.mark.parametrize('permute', [False, True])
def test_largest_agrees_with_reconstruct_largest_component(permute):
  from foundationpose_amd.reconstruct import largest_component
  pos, faces, normals, colors = M.composite_mesh()
  if permute:
    perm = np.random.RandomState(5).permutation(len(pos))         # new index of every vertex
    inv = np.argsort(perm)
    pos, normals, colors, faces = pos[inv], normals[inv], colors[inv], perm[faces].astype(np.int32)
  out = C.components(pos, faces, normals, colors, keep='largest')
  mask = largest_component(faces, len(pos))
  assert mask.sum() == 2 * 95 * 200 and out['counts'] == (4, 1, 95 * 200 + 2, 2 * 95 * 200)
  assert (out['vertex_map'][faces[:, 0]] >= 0).tolist() == mask.tolist()
  # ... and the re-index of reconstruct_object
  used = np.zeros(len(pos), dtype=bool)
  used[faces[mask].reshape(-1)] = True
  new_id = np.cumsum(used) - 1
  assert out['faces'].tobytes() == new_id[faces[mask]].astype(np.int32).tobytes()
  assert out['pos'].tobytes() == pos[used].tobytes() and out['normals'].tobytes() == normals[used].tobytes()
  assert out['colors'].tobytes() == colors[used].tobytes()
  assert (out['vertex_map'] >= 0).tolist() == used.tolist()


def test_tie_goes_to_the_lower_component_number_not_the_earlier_face():
  V, faces = C.tie_case()
  out = C.components(np.zeros((V, 3)), faces, keep='largest')
  assert out['stats'].tolist() == [[5, 3], [5, 3]] and out['kept'].tolist() == [True, False]
  assert out['labels'].tolist() == [0, 1] * 5
  assert (out['vertex_map'] >= 0).tolist() == [True, False] * 5      # the component of vertex 0: the LATER faces
  assert out['faces'].tolist() == [[0, 1, 2], [1, 2, 3], [2, 3, 4]]
  assert C.components(np.zeros((V, 3)), faces, keep='all')['counts'] == (2, 2, 10, 6)


def test_threshold_at_the_exact_boundary():
  # 0.25 * 8 == 2.0 exactly in double: a component of 2 faces is kept, the next float32 above 0.25 drops it
  n = np.array([8, 2, 1])
  assert C.select(n, 'all', 1, 0.25).tolist() == [True, True, False]
  assert C.select(n, 'all', 1, np.nextafter(np.float32(0.25), np.float32(1))).tolist() == [True, False, False]
  assert C.select(n, 'all', 1, np.nextafter(np.float32(0.25), np.float32(0))).tolist() == [True, True, False]
  # the fraction is the float32 the device receives: 0.1 as float32 is ABOVE 1/10, so 3 of 30 is below the bound
  assert np.float64(np.float32(0.1)) * 30.0 > 3.0
  assert C.select(np.array([30, 3]), 'all', 1, 0.1).tolist() == [True, False]
  assert C.select(np.array([30, 3]), 'all', 3, 0.0).tolist() == [True, True]
  assert C.select(np.array([30, 3]), 'all', 4, 0.0).tolist() == [True, False]
  assert C.select(n, 'largest', 9, 0.0).tolist() == [False, False, False]      # the largest is no candidate: nothing is kept
  assert C.select(n, 'all', 1, 1.0).tolist() == [True, False, False]
  assert C.select(np.array([0, 0]), 'largest').tolist() == [False, False]
  with pytest.raises(ValueError):
    C.select(n, 'biggest')
