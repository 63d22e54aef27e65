"""CPU: finding an object without a mask - the numpy restatement tests/detect_oracle.py on a case in which every condition of the match
rule occurs, on a scene rendered exactly at a template's pose and on seeded clutter scenes (templates from the CPU rasteriser); the
properties of the template builder; the suppression of foundationpose_amd/detect.py against the oracle's; the table limits and the
refusals of fp_template_match, which need no GPU."""
import ctypes

import numpy as np
import pytest

from foundationpose_amd import detect as Dt
from foundationpose_amd import synthetic as S
from foundationpose_amd.mesh_tensors import make_mesh_tensors
from tests import detect_oracle as O

F = np.float32
Z0, RENDER = 0.7, 96


@pytest.fixture(scope='module')
def model():
  """The centred mustard model on the CPU and its render camera."""
  mesh = S.make_mustard_mesh(seed=0, n_theta=48, n_z=42)
  mesh.vertices = mesh.vertices - (mesh.vertices.min(axis=0) + mesh.vertices.max(axis=0)) / 2
  extent = 2.0 * float(np.linalg.norm(mesh.vertices, axis=1).max())
  f, K = Dt.render_camera(extent, RENDER, Z0)
  return dict(mesh=mesh, mt=make_mesh_tensors(mesh, device='cpu'), extent=extent, f=f, K=K)


def template_depths(model, rot):
  from oracle.render import nvdiffrast_render
  poses = np.tile(np.eye(4), (len(rot), 1, 1))
  poses[:, :3, :3] = rot
  poses[:, 2, 3] = Z0
  return nvdiffrast_render(K=model['K'], H=RENDER, W=RENDER, ob_in_cams=poses.astype(F), mesh_tensors=model['mt'])[1].numpy()


@pytest.fixture(scope='module')
def rendered(model):
  """The 504 depth maps (42 views x 12 rolls) of the clutter recipe and their rotations, rendered once."""
  rot = Dt.template_rotations(42, 30)
  return rot, template_depths(model, rot)


@pytest.fixture(scope='module')
def templates(model, rendered):
  return Dt.templates_from_depths(rendered[1], model['f'], Z0, rendered[0], model['extent'])


def host_instances(model):
  from oracle.render import nvdiffrast_render

  def render(K, H, W, shapes, poses):
    out = []
    for s, p in zip(shapes, poses):
      mt = model['mt'] if isinstance(s, str) else make_mesh_tensors(S.SimpleMesh(s[0], s[1]), device='cpu')
      out.append(nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=p[None].astype(F), mesh_tensors=mt)[1][0].numpy())
    return np.asarray(out)
  return render


def test_every_condition_of_the_rule_occurs_in_the_small_case():
  c = O.small_case()
  total = dict.fromkeys(O.REASONS, 0)
  for frame in c['frames']:
    keys, counts, why = O.match(frame, c['K'], c['table'], c['ranges'], c['n_in'], c['n_out'], c['anchors'], 2, 0, 0, c['z_min'], c['z_max'], c['zfar'],
                                c['tol_in'], c['tol_out'])
    for k, v in why.items():
      total[k] += v
    assert keys.shape == (2, 36, 48) and (keys[counts == 0] & 0xFFFF0000 == 0).all()
    score, _, _ = Dt.decode_keys(keys)
    assert (score == (counts >> 16) * (counts & 0xFFFF)).all()
  assert all(total[k] > 0 for k in O.REASONS), total
  # the duplicated template never wins: equal keys cannot occur, and the lower index has the higher key at an equal score
  keys, _, _ = O.match(c['frames'][0], c['K'], c['table'], c['ranges'], 12, 9, 2, 2, 0, 0, c['z_min'], c['z_max'], c['zfar'], c['tol_in'], c['tol_out'])
  _, t_local, _ = Dt.decode_keys(keys[0])
  assert (t_local[keys[0] > 0] != 5).all() and (t_local[keys[0] > 0] == 2).any()


def test_a_scene_at_a_templates_pose_scores_every_sample(model, rendered, templates):
  rot, depths = rendered
  for t in (0, 100, 333):
    one = Dt.templates_from_depths(depths[t:t + 1], model['f'], Z0, rot[t:t + 1], model['extent'])
    keys, counts, _ = O.match(depths[t], model['K'], one.table, one.ranges, one.n_in, one.n_out, 1, stride=1, tol_in=0.001, tol_out=0.03)
    A = one.table[0, 0, :3].astype(np.float64) + [0, 0, Z0]      # the anchor sample's pixel is the centre's anchor pixel
    r, c = int(round(model['f'] * A[1] / A[2] + model['K'][1, 2])), int(round(model['f'] * A[0] / A[2] + model['K'][0, 2]))
    assert keys[0, r, c] >> 16 == one.n_in * one.n_out == 3072 and counts[0, r, c] == (64 << 16 | 48)
    top = O.nms(keys, depths[t], model['K'], one.table, one.ranges, one.rotations, [model['extent'] / 2], top_k=1, stride=1)[0][0]
    assert np.abs(top[3] - [0, 0, Z0]).max() < 1e-5      # the centre in closed form: float32 samples, float64 arithmetic


def test_builder_anchors_first_distinct_samples_same_bits(model, rendered, templates):
  rot, depths = rendered
  assert templates.n_templates == 504 and templates.dropped == [] and templates.table.shape == (504, 112, 4)
  assert (templates.table[:, :, 3] == 0).all() and np.isfinite(templates.table).all()
  tab = templates.table.astype(np.float64)
  off_axis = tab[:, :64, 0] ** 2 + tab[:, :64, 1] ** 2
  assert (off_axis.argmin(axis=1) == 0).all()                           # the anchor is the in-sample nearest the centre ray
  for t in range(0, 504, 7):
    assert len(np.unique(tab[t, :, :3], axis=0)) == 112                # distinct samples
  again = Dt.templates_from_depths(depths, model['f'], Z0, rot, model['extent'])
  assert (again.table.view(np.uint32) == templates.table.view(np.uint32)).all()
  # further anchors: farthest-point sampling among the in-samples, moved to the front, the other samples in their order
  three = Dt.templates_from_depths(depths[:40], model['f'], Z0, rot[:40], model['extent'], anchors=3)
  for t in range(40):
    a, b = three.table[t, :64, :3].astype(np.float64), templates.table[t, :64, :3].astype(np.float64)
    assert (a[0] == b[0]).all() and sorted(map(tuple, a)) == sorted(map(tuple, b))
    gap = np.linalg.norm(b - b[0], axis=1)
    assert (a[1] == b[gap.argmax()]).all()
    gap2 = np.minimum(gap, np.linalg.norm(b - a[1], axis=1))
    assert (a[2] == b[gap2.argmax()]).all()
  # out-samples lie outside the in-samples' extent, at the depth of the silhouette's rim
  assert (np.abs(tab[:, 64:, :2]).max(axis=(1, 2)) > np.abs(tab[:, :64, :2]).max(axis=(1, 2))).all()


def test_builder_drops_and_reports(model, rendered):
  rot, depths = rendered
  d = depths[:4].copy()
  d[1] = 0                                   # an empty render
  small = np.zeros_like(d[3])
  small[40:46, 40:46] = 0.7                  # 36 pixels, 16 after the erosion
  d[3] = small
  ts = Dt.templates_from_depths(d, model['f'], Z0, rot[:4], model['extent'])
  assert ts.n_templates == 2 and [i for i, _ in ts.dropped] == [1, 3]
  assert 'empty' in ts.dropped[0][1] and 'fewer than n_in' in ts.dropped[1][1]
  assert (ts.rotations == rot[[0, 2]]).all()
  edge = np.zeros_like(d[0])
  edge[0:30, 30:60] = 0.7                    # touches the border: the ring would leave the render
  ts = Dt.templates_from_depths(edge[None], model['f'], Z0, rot[:1], model['extent'])
  assert ts.n_templates == 0 and 'does not fit' in ts.dropped[0][1]


def test_table_limits_and_concat(templates):
  with pytest.raises(ValueError, match='65535'):
    Dt.check_table_limits(256, 256, 1, [1])
  Dt.check_table_limits(255, 257, 1, [1])
  with pytest.raises(ValueError, match='samples a template'):
    Dt.check_table_limits(1, 1024, 1, [1])
  for anchors in (0, 5):
    with pytest.raises(ValueError, match='anchors'):
      Dt.check_table_limits(12, 9, anchors, [1])
  with pytest.raises(ValueError, match='anchors'):
    Dt.check_table_limits(2, 9, 3, [1])
  with pytest.raises(ValueError, match='16384'):
    Dt.check_table_limits(12, 9, 1, [16385])
  Dt.check_table_limits(12, 9, 4, [16384])
  with pytest.raises(ValueError, match='objects'):
    Dt.check_table_limits(12, 9, 1, [1] * 65)
  both = Dt.TemplateSet.concat([templates, templates])
  assert both.n_obj == 2 and list(both.ranges) == [0, 504, 1008] and both.table.shape[0] == 1008 and len(both.diameters) == 2
  other = Dt.TemplateSet(templates.table[:, :100], templates.rotations, 64, 36, 1, templates.ranges, templates.diameters, [])
  with pytest.raises(ValueError, match='cannot be concatenated'):
    Dt.TemplateSet.concat([templates, other])
  with pytest.raises(ValueError, match='do not hold'):
    Dt.TemplateSet(templates.table[:10], templates.rotations, 64, 48, 1, templates.ranges, templates.diameters, [])


def test_host_suppression_equals_the_oracles(model, templates):
  sc = O.clutter_scene(O.SCENE_SEEDS[0], host_instances(model))
  sub = Dt.TemplateSet(templates.table[::6], templates.rotations[::6], 64, 48, 1, [0, 84], templates.diameters, [])
  keys, counts, _ = O.match(sc['depth'], sc['K'], sub.table, sub.ranges, 64, 48, 1, stride=4, tol_in=0.015, tol_out=0.06)
  want = O.nms(keys, sc['depth'], sc['K'], sub.table, sub.ranges, sub.rotations, sub.diameters / 2, top_k=5, stride=4)[0]
  got = Dt.detections_from_keys(keys, counts, sc['depth'], sc['K'], sub, top_k=5, stride=4)[0]
  assert len(got) == len(want) == 5
  for g, w in zip(got, want):
    assert g['template'] == w[1] and g['anchor'] == w[2] and np.abs(g['centre'] - w[3]).max() < 1e-12
    assert g['pixel'] == (4 * (w[0] // 40), 4 * (w[0] % 40)) and (g['ob_in_cam'][:3, :3] == sub.rotations[w[1]]).all()
    assert g['score'] == round(g['in_fraction'] * 64) * round(g['out_fraction'] * 48)
  centres = np.array([g['centre'] for g in got])
  gaps = np.linalg.norm(centres[:, None] - centres[None], axis=2) + np.eye(5)
  assert gaps.min() > sub.diameters[0] / 2
  few = Dt.detections_from_keys(keys, counts, sc['depth'], sc['K'], sub, top_k=5, stride=4, min_score=got[2]['score'] / 3072.0 + 1e-9)[0]
  assert [f['template'] for f in few] == [g['template'] for g in got if g['score'] > got[2]['score']]


@pytest.mark.parametrize('seed', O.SCENE_SEEDS)
def test_clutter_scene_top1_is_the_object_and_beats_the_mask_path(model, templates, seed):
  """The oracle's best detection in a seeded clutter scene (160 x 120, f = 150, the mustard model at 0.55 - 0.8 m, a tilted plane, four
  spheres, mm rounding, 1 mm noise, 2 % dropout; 504 templates, 64 + 48 samples, stride 2) on register's filtered depth: it projects into
  the object's visible mask, and its centre is no farther from the truth than guess_translation's from the PERFECT visible mask of the
  same depth.  Measured (mm, detect / guess_translation): seed 1: 17.5 / 34.7, seed 8: 38.7 / 66.0, seed 28: 19.9 / 29.8."""
  from oracle import geometry as G
  sc = O.clutter_scene(seed, host_instances(model))
  assert sc['visible_fraction'] >= 0.9
  filtered = np.asarray(G.bilateral_filter_depth(G.erode_depth(sc['depth'], radius=2), radius=2), dtype=F)
  keys, _, _ = O.match(filtered, sc['K'], templates.table, templates.ranges, 64, 48, 1, stride=2, tol_in=0.015, tol_out=0.06)
  top = O.nms(keys, filtered, sc['K'], templates.table, templates.ranges, templates.rotations, templates.diameters / 2, top_k=1, stride=2)[0][0]
  truth = sc['pose'][:3, 3]
  uv = sc['K'] @ top[3] / top[3][2]
  err = np.linalg.norm(top[3] - truth)
  err_mask = np.linalg.norm(np.asarray(G.guess_translation(filtered, sc['mask'], sc['K'])) - truth)
  print(f'seed {seed}: detect {err * 1000:.1f} mm, guess_translation {err_mask * 1000:.1f} mm')
  assert sc['mask'][int(round(uv[1])), int(round(uv[0]))]
  assert err <= err_mask


@pytest.fixture(scope='module')
def built():
  import __graft_entry__ as g
  g.build()
  from foundationpose_amd import _lib
  return _lib


def test_argument_checks_need_no_gpu(built):
  L = built.lib()
  fake = ctypes.c_void_p(64)      # never dereferenced: every check of a value comes first
  K = np.array([[50.0, 0, 8], [0, 50.0, 6], [0, 0, 1]])

  def call(ctx=fake, depth=fake, n=1, H=12, W=16, K_on=True, table=fake, ranges=(0, 3, 5), n_in=12, n_out=9, anchors=2, stride=2, r0=0, c0=0, z_min=0.1,
           z_max=2.0, zfar=float('inf'), tol_in=0.01, tol_out=0.03, keys=fake, counts=None, k_entry=None):
    k = K.copy()
    if k_entry is not None:
      k.reshape(-1)[k_entry[0]] = k_entry[1]
    rg = None if ranges is None else np.asarray(ranges, np.int32)
    return L.fp_template_match(ctx, depth, n, H, W, built.ptr(k) if K_on else None, table, built.ptr(rg), 0 if rg is None else len(rg) - 1, n_in, n_out, anchors,
                               stride, r0, c0, z_min, z_max, zfar, tol_in, tol_out, keys, counts, None)

  nan, inf = float('nan'), float('inf')
  bad = [dict(ctx=None), dict(depth=None), dict(K_on=False), dict(table=None), dict(ranges=None), dict(keys=None),
         dict(n=-1), dict(n=1 << 16), dict(H=0), dict(W=0), dict(H=(1 << 14) + 1), dict(stride=0), dict(stride=-2),
         dict(r0=-1), dict(r0=12), dict(c0=-1), dict(c0=16), dict(tol_in=0.0), dict(tol_in=nan), dict(tol_out=-1.0), dict(tol_out=nan),
         dict(z_min=2.5), dict(z_min=nan), dict(z_max=nan), dict(zfar=0.0), dict(zfar=nan),
         dict(k_entry=(0, nan)), dict(k_entry=(2, inf)), dict(k_entry=(4, 0.0)), dict(k_entry=(0, -5.0)), dict(k_entry=(5, 1e300)), dict(k_entry=(1, nan)),
         dict(n_in=0), dict(n_out=0), dict(n_in=256, n_out=256), dict(n_in=1, n_out=1024), dict(anchors=0), dict(anchors=5), dict(n_in=1, anchors=2),
         dict(ranges=(0,)), dict(ranges=tuple(range(66))), dict(ranges=(1, 3)), dict(ranges=(0, 3, 2)), dict(ranges=(0, 16385)),
         dict(table=ctypes.c_void_p(72))]
  for kw in bad:
    assert call(**kw) == built.FP_EINVAL, kw
    assert L.fp_last_error()
  assert call(ranges=(0, 16385)) == built.FP_EINVAL and b'16384' in L.fp_last_error()
  assert call(n_in=256, n_out=256) == built.FP_EINVAL and b'65535' in L.fp_last_error()
  assert call(r0=12) == built.FP_EINVAL and b'outside' in L.fp_last_error()
  assert call(table=ctypes.c_void_p(72)) == built.FP_EINVAL and b'16-byte aligned' in L.fp_last_error()
  # the staged chunk: a host function
  assert Dt.staged_templates(12, 9) == 1024 // 21 and Dt.staged_templates(64, 48) == 1024 // 112 and Dt.staged_templates(1, 1023) == 1
  out = ctypes.c_int()
  assert L.fp_template_match_info(1025, ctypes.byref(out)) == built.FP_EINVAL and L.fp_template_match_info(21, None) == built.FP_EINVAL


def test_refusals_on_the_host(templates):
  d = np.zeros((12, 16), F)
  K = np.array([[50.0, 0, 8], [0, 50.0, 6], [0, 0, 1]])
  with pytest.raises(ValueError, match='float32'):
    Dt.match_templates(d.astype(np.float64), K, templates, device='cpu')
  with pytest.raises(ValueError, match=r'\(H, W\)'):
    Dt.match_templates(d[None, None], K, templates, device='cpu')
  with pytest.raises(ValueError, match='stride'):
    Dt.match_templates(d, K, templates, stride=0, device='cpu')
  with pytest.raises(ValueError, match='offset'):
    Dt.match_templates(d, K, templates, offset=(12, 0), device='cpu')
  with pytest.raises(ValueError, match='must be > 0'):
    Dt.match_templates(d, K, templates, tol_in=0.0, device='cpu')
  with pytest.raises(ValueError, match='z_range'):
    Dt.match_templates(d, K, templates, z_range=(2.0, 1.0), device='cpu')
  with pytest.raises(ValueError, match='anchors'):
    Dt.match_templates(d, K, templates, anchors=2, device='cpu')
  with pytest.raises(ValueError, match='focal'):
    Dt.match_templates(d, np.diag([0.0, 1.0, 1.0]), templates, device='cpu')
  with pytest.raises(ValueError, match='one frame'):
    Dt.detect(d[None], K, templates, device='cpu')
  assert Dt.lattice_shape(72, 96, 3, (1, 2)) == (24, 32) and Dt.lattice_shape(480, 640, 4) == (120, 160)
