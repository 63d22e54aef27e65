"""CPU checks of the rasteriser's exact reference (tests/tools/raster_ref.py): that every lattice case is what it says it is, that the reference's
fill rule equals the literal top-left statement and a concrete-epsilon evaluation in Python integers, that the CPU mirror (oracle/raster_c.c) equals
the reference - winner exactly, floats within the derived tolerance -, and that seven deliberately wrong rasterisers are told apart from it."""
import numpy as np
import pytest

from tests.tools import raster_ref as R


def _hyps(c):
  return range(len(c['shifts']))


@pytest.mark.parametrize('name', R.ALL_CASES)
def test_transform_is_exact(name):
  c = R.lattice_case(name)
  assert len(R.transform_check(c)) == 5
  assert len(c['real']) <= 370 and np.all(np.diff(c['real']) > 0)


@pytest.mark.parametrize('name', R.BASE_CASES)
def test_case_reaches_the_paths_it_names(name):
  c = R.lattice_case(name)
  cl = c['claims']
  for N, h in ((1, 0), (2, 1), (5, 4)):
    got = set(R.face_classes(c, h, N)) - {'none'}
    assert cl['classes'] <= got, (name, N, got)
    if cl.get('only_classes'):
      assert got == cl['classes'], (name, N, got)
    cov = R.coverage_exact(c, h)
    covered = cov['face'] >= 0
    assert covered.sum() >= 100
    e, dx, dy, a = R._edges(c, h)
    on_edge = ((e == 0).any(0) & (np.abs(e).max(0) > 0))          # a pixel centre exactly on an edge line of a face ...
    near = on_edge & (np.sign(a)[:, None, None] * e >= 0).all(0)   # ... and on the face's closed boundary
    if 'on_edge' in cl and h == 0:
      assert near.sum() >= cl['on_edge'], (name, int(near.sum()))
      assert (near & cov['claims']).sum() > 0 and (near & ~cov['claims']).sum() > 0        # both outcomes of the fill rule occur
    if 'ties' in cl:
      k = np.sort(cov['key'], 0)
      assert ((k[0] == k[1]) & np.isfinite(k[0])).sum() >= cl['ties']
    if len(c['real']) < len(c['faces']):           # the faces the reference leaves out claim nothing
      allf = dict(c, real=np.arange(len(c['faces'])))
      rest = np.setdiff1d(allf['real'], c['real'])
      assert not R.claims_exact(allf, h)[rest].any()
    if cl.get('dropped'):
      assert (cov['claims'] & ~cov['ok']).any() and ((np.abs(cov['key']) == 1) & cov['ok']).any()       # one ulp outside is dropped, exactly +-1 kept
    if cl.get('band'):
      f = c['faces'][c['real']]
      for t in range(len(f)):
        n = int(cov['claims'][t].sum())
        if n >= 20:                      # (the parallax of a translation shrinks the small one to a pixel or two)
          assert (cov['claims'][t] & ~cov['ok'][t]).any() and cov['ok'][t].any()                       # the triangle is cut inside the window
      band = cov['band']
      assert band.sum() <= R.ZCLIP_CAP * cov['claims'].any(0).sum()
    else:
      assert not cov['band'].any()


@pytest.mark.parametrize('name', R.BASE_CASES)
def test_competing_depths_are_exact_or_far_apart(name):
  """Where two faces compete for a pixel, the kernel's float32 depths decide as the exact ones do: either both are exact in float32 (z = 0; every
  barycentric 0, 1/2 or 1; a power-of-two area with a few-bit constant z) or they differ by at least DEPTH_GAP, 2000 times the tolerance."""
  c = R.lattice_case(name)
  for h in _hyps(c):
    cov = R.coverage_exact(c, h)
    e, dx, dy, a = R._edges(c, h)
    z = c['zw'][c['faces'][c['real']]]
    const = (z[:, 0] == z[:, 1]) & (z[:, 0] == z[:, 2])
    half = ((2 * e) % np.where(a == 0, 1, a)[None, :, None, None] == 0).all(0)
    pow2 = (np.abs(a) & (np.abs(a) - 1)) == 0
    fewbits = np.array([float(np.float32(v * 2.0 ** 6).item()).is_integer() or v == 1 or v == -1 for v in z[:, 0] * 1.0])       # |z| <= 1 in steps of 2^-6
    exact = const[:, None, None] & ((z[:, 0] == 0)[:, None, None] | half | (pow2 & fewbits)[:, None, None])
    cl = cov['claims']
    # depth of every claiming face (not only the in-range ones: a face just outside +-1 must not slip in)
    lam = e.astype(np.float64) / np.where(a == 0, 1, a)[None, :, None, None]
    zw = np.where(const[:, None, None], z[:, 0][:, None, None], (lam * z.T[:, :, None, None]).sum(0))
    for t in range(len(z)):
      others = cl & cl[t][None] & (np.arange(len(z)) != t)[:, None, None]
      close = others & (np.abs(zw - zw[t][None]) < R.DEPTH_GAP)
      assert not (close & ~(exact & exact[t][None])).any(), (name, h, t)
      edge = cl[t] & ~exact[t] & (np.abs(np.abs(zw[t]) - 1) < R.DEPTH_GAP) & ~cov['band'][::-1]
      if not c['claims'].get('band'):
        assert not edge.any(), (name, h, t)


def _literal(c, h, edge='tl', winding=True, snap='rint', tie='low', key='ordered', interp='persp'):
  """A plain rasteriser after the documented rules, with switches that break one rule each.  Returns (face, u, v), top-down."""
  dx_, dy_ = c['shifts'][h]
  Xf, Yf = c['Xq'] + dx_ / c['w'], c['Yq'] + dy_ / c['w']
  X, Y = (np.rint(Xf), np.rint(Yf)) if snap == 'rint' else (np.trunc(Xf), np.trunc(Yf))
  e, dx, dy, a = R._edges(c, h, (X.astype(np.int64), Y.astype(np.int64)))
  s = np.sign(a) if winding else np.ones_like(a)
  e, dx, dy, area = e * s[None, :, None, None], dx * s, dy * s, a * s
  tl = (dy > 0) | ((dy == 0) & (dx < 0))
  if edge == 'tl':
    ins = (e > 0) | ((e == 0) & tl[:, :, None, None])
  else:
    ins = (e >= 0) if edge == 'ge' else (e > 0)
  ins = ins.all(0) & (area != 0)[:, None, None]
  f = c['faces'][c['real']]
  lam = e.astype(np.float64) / np.where(area == 0, 1, area)[None, :, None, None]
  z = c['zw'][f]
  const = (z[:, 0] == z[:, 1]) & (z[:, 0] == z[:, 2])
  zw = np.where(const[:, None, None], z[:, 0][:, None, None], (lam * z.T[:, :, None, None]).sum(0))
  ok = ins & (zw >= -1) & (zw <= 1)
  if key == 'raw':                      # the float's bits compared as an unsigned integer
    k = zw.astype(np.float32).view(np.uint32).astype(np.float64)
  else:
    k = zw
  k = np.where(ok, k, np.inf)
  win = k.argmin(0) if tie == 'low' else len(f) - 1 - k[::-1].argmin(0)
  face = np.where(ok.any(0), c['real'][win], -1)
  lw = np.stack([np.take_along_axis(lam[i], win[None], 0)[0] for i in range(3)], -1)
  q = lw / (c['w'][f][win] if interp == 'persp' else 1.0)
  qs = q.sum(-1, keepdims=True)
  uv = np.where(ok.any(0)[..., None], q / np.where(qs == 0, 1, qs), 0)
  return face[::-1], uv[::-1, :, 0], uv[::-1, :, 1]


def _differs(c, h, **kw):
  cov = R.coverage_exact(c, h)
  ref = R.interp_float64(c, h, cov)
  face, u, v = _literal(c, h, **kw)
  return bool((face != cov['face']).any() or np.abs(u - ref['rast'][..., 0]).max() > 1e-3 or np.abs(v - ref['rast'][..., 1]).max() > 1e-3)


@pytest.mark.parametrize('name', R.BASE_CASES)
def test_symbolic_displacement_equals_the_literal_top_left_rule(name):
  c = R.lattice_case(name)
  for h in _hyps(c):
    assert not _differs(c, h), (name, h)
  # the displacement with a concrete rational eps = 2^-40 in Python integers: e + eps dy - eps^2 dx, scaled by 2^80
  e, dx, dy, a = R._edges(c, 0)
  E = e.astype(object) * (1 << 80) + (dy.astype(object) * (1 << 40) - dx.astype(object))[:, :, None, None]
  sg = np.sign(a).astype(object)[None, :, None, None]
  inside = ((E * sg) > 0).all(0) & (a != 0)[:, None, None]
  assert np.array_equal(inside, R.claims_exact(c, 0))


MUTANTS = [('ge', dict(edge='ge'), 'centres_small'), ('gt', dict(edge='gt'), 'centres_small'), ('no_winding', dict(winding=False), 'centres_small'),
           ('trunc_snap', dict(snap='trunc'), 'degenerate'), ('tie_high', dict(tie='high'), 'ties_zero'), ('raw_bits_key', dict(key='raw'), 'depth_signs_mixed'),
           ('affine_uv', dict(interp='affine'), 'zclip_slant')]


@pytest.mark.parametrize('what,kw,name', MUTANTS, ids=[m[0] for m in MUTANTS])
def test_wrong_rasterisers_are_rejected(what, kw, name):
  c = R.lattice_case(name)
  assert _differs(c, 0, **kw), (what, name)
  if what in ('ge', 'gt'):                # ... and on the tilings: a shared edge claimed twice / not at all
    assert _differs(R.lattice_case('large32'), 0, **kw)
  if what == 'raw_bits_key':
    assert _differs(R.lattice_case('depth_signs_ulp_neg'), 0, **kw) and _differs(R.lattice_case('depth_signs_tiny'), 0, **kw)


def test_tilings_claim_every_interior_pixel_once():
  masks = []
  for kind in ('fan', 'strip', 'ear'):
    for perm in ('', '_perm'):
      c = R.lattice_case('tiling_' + kind + perm)
      for h in _hyps(c):
        cov = R.coverage_exact(c, h)
        n = cov['claims'].sum(0)
        assert n.max() == 1 and n.sum() > 2500
        masks.append((h, n[::-1] > 0))
        assert np.array_equal(n[::-1] > 0, cov['face'] >= 0)
  for h, m in masks:
    assert np.array_equal(m, masks[h][1]), 'the mask depends on the tessellation'
  c = R.lattice_case('large32')
  combs = np.all(c['w'][c['faces']] == 1, axis=1)
  for h in _hyps(c):
    n = R.coverage_exact(c, h)['claims'][combs].sum(0)
    assert n.min() == 1 and n.max() == 1, 'the combs tile the window'
  for far in (16383, 16384, 1600008):
    c = R.lattice_case('far64_%d' % far)
    assert (R.coverage_exact(c, 0)['face'] >= 0).all()


def test_far_variants_differ_little_inside_the_window():
  """the far vertex one unit further out (16383 -> 16384: the other record form) moves an edge by less than a unit inside the window"""
  f0, f1, f2 = [R.coverage_exact(R.lattice_case('far64_%d' % far), 0)['face'] for far in (16383, 16384, 1600008)]
  assert (f0 == f1).mean() > 0.99 and (f0 == f2).mean() > 0.5


@pytest.mark.parametrize('name', R.PADDED_CASES)
def test_padded_cases_reach_the_launch_forms(name):
  c = R.lattice_case(name)
  b = R.lattice_case(c['claims']['base'])
  F, V, ids = len(c['faces']), len(c['X']), c['claims']['remap']
  assert np.array_equal(c['faces'][ids], b['faces']) and F - 1 in ids
  p5, p1 = R.plan_restated(5, V, F, 64, 64), R.plan_restated(1, V, F, 64, 64)
  if name == 'padded_solo_max':
    assert p1['solo'] and not R.plan_restated(1, V, F + 1, 64, 64)['solo']
  elif name == 'padded_solo_over':
    assert not p1['solo'] and R.plan_restated(1, V, F - 1, 64, 64)['solo']
  else:
    want = 8 if F >= 8192 else 4 if F >= 4096 else 2
    assert p5['G'] == want and not p5['solo'], p5
    assert p5['lds_verts'] == (V <= 8192) and (V <= 8192 or not p1['solo'])
    for g in range(1, want):
      assert g * p5['Fg'] - 1 in ids and g * p5['Fg'] in ids
  # the padding covers nothing and the real faces are the base's, so the exact images are the base's with ids remapped
  for h in (0, 4):
    cp, cb = R.coverage_exact(c, h), R.coverage_exact(b, h)
    assert np.array_equal(cp['face'] >= 0, cb['face'] >= 0)
    assert np.array_equal(cp['face'][cp['face'] >= 0], ids[cb['face'][cb['face'] >= 0]])
  pad = np.ones(F, bool)
  pad[ids] = False
  X, Y = R.hyp_lattice(c, 0)
  fx, fy = X[c['faces'][pad]], Y[c['faces'][pad]]
  area = (fx[:, 1] - fx[:, 0]) * (fy[:, 2] - fy[:, 0]) - (fx[:, 2] - fx[:, 0]) * (fy[:, 1] - fy[:, 0])
  assert np.all((area == 0) | (fx.max(1) < -2000))


def test_float32_emulation_lies_inside_the_tolerance():
  mu = ma = 0.0
  for name in R.BASE_CASES:
    c = R.lattice_case(name)
    for h in _hyps(c):
      cov = R.coverage_exact(c, h)
      u, a = R.float_errors(R.emulate_f32(c, h, cov), R.interp_float64(c, h, cov), cov['band'])
      mu, ma = max(mu, u * R.TOL_UVZ), max(ma, a * R.TOL_ATTR)
  print('emulated max error: u, v, z/w %.3e (recorded %.3e), attributes %.3e (recorded %.3e)' % (mu, R.EMU_UVZ, ma, R.EMU_ATTR))
  assert 0.5 * R.EMU_UVZ < mu <= R.EMU_UVZ and 0.5 * R.EMU_ATTR < ma <= R.EMU_ATTR
  assert R.TOL_UVZ == 4 * R.EMU_UVZ and R.TOL_ATTR == 4 * R.EMU_ATTR
  assert R.TOL_UVZ >= 7 * 2.0 ** -24          # not below the count of roundings


def render_case(render, c, n, dev=None, **kw):
  """the case's n first hypotheses through a nvdiffrast_render (the CPU mirror's or the HIP one): dict of numpy arrays like interp_float64's"""
  import torch
  to = (lambda x: torch.as_tensor(x)) if dev is None else (lambda x: torch.as_tensor(x).to(dev))
  mt = {k: to(v) for k, v in c['mesh_tensors'].items()}
  extra = {'rast': None}
  color, depth, _ = render(K=c['K'], H=c['H'], W=c['W'], ob_in_cams=to(c['poses'][:n]), mesh_tensors=mt, projection_mat=c['projection_mat'],
                           bbox2d=None if c['bbox2d'] is None else to(c['bbox2d'][:n]), output_size=(c['Ho'], c['Wo']), use_light=False, extra=extra, **kw)
  return dict(rast=extra['rast'].cpu().numpy(), xyz=extra['xyz_map'].cpu().numpy(), depth=depth.cpu().numpy(), color=color.cpu().numpy())


def compare_with_reference(c, got, n, what):
  """winner exactly (no exclusions but zclip's stated band), floats within the tolerance; returns the largest |err| / tol (uvz, attr)"""
  worst = [0.0, 0.0]
  for h in range(n):
    cov = R.coverage_exact(c, h)
    ref = R.interp_float64(c, h, cov)
    keep = ~cov['band']
    ids = got['rast'][h][..., 3].astype(np.int64)
    bad = (ids != cov['face'] + 1) & keep
    assert not bad.any(), '%s %s hypothesis %d: triangle id differs on %d pixels, first (row, col) %s: got %d, reference %d' % (
        what, c['name'], h, bad.sum(), np.argwhere(bad)[0], ids[tuple(np.argwhere(bad)[0])], cov['face'][tuple(np.argwhere(bad)[0])] + 1)
    u, a = R.float_errors({k: v[h] for k, v in got.items()}, ref, cov['band'] | (ids != cov['face'] + 1))
    worst = [max(worst[0], u), max(worst[1], a)]
  print('%s %s: largest |err| / tol: u, v, z/w %.3f, attributes %.3f' % (what, c['name'], worst[0], worst[1]))
  assert worst[0] <= 1 and worst[1] <= 1, (what, c['name'], worst)
  return worst


@pytest.mark.parametrize('name', R.ALL_CASES)
def test_cpu_mirror_equals_the_reference(name):
  from oracle.render import nvdiffrast_render
  c = R.lattice_case(name)
  compare_with_reference(c, render_case(nvdiffrast_render, c, 5), 5, 'mirror')
