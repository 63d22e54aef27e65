"""CPU checks of the rasteriser's exact reference (tests/tools/raster_ref.py): that every lattice case is what it says it is, that the reference's
fill rule equals the literal top-left statement and a concrete-epsilon evaluation in Python integers, that the CPU mirror (oracle/raster_c.c) equals
the reference - winner exactly, floats within the derived tolerance -, and that seven deliberately wrong rasterisers are told apart from it.
Texture fetch and lighting (R.SHADE_CASES): the float64 reference against closed forms that do not go through its fetch, the float32 emulation inside
EMU_TEX, wrong fetches told apart, and the CPU mirror against float64 under every light setting."""
import functools

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


# ---------------------------------------------------------------------------------------------------------------------------------------
# texture fetch and lighting (R.SHADE_CASES)
# ---------------------------------------------------------------------------------------------------------------------------------------
def shade_light(var):
  """nvdiffrast_render's light arguments of a variant name (None: use_light = False)"""
  return {} if var is None else dict(R.LIGHTS[var], use_light=True)


@pytest.mark.parametrize('name', R.SHADE_CASES + ['tex_wrap_shifted'])
def test_shade_case_is_what_it_says(name):
  c = R.lattice_case(name)
  assert len(R.transform_check(c)) == 5
  mt = c['mesh_tensors']
  for h in _hyps(c):
    cl = R.claims_exact(c, h)
    assert cl.sum(0).max() == 1 and cl.any((1, 2)).all()                       # no two faces compete, every face shows
  if 'tex' in mt:
    assert 'vertex_color' not in mt and max(mt['tex'].shape[1:3]) <= 16
    assert not (mt['uv_idx'] == mt['faces']).any() and len(mt['uv']) > len(mt['pos'])
    assert np.abs(mt['uv'][mt['uv_idx']]).max() <= 3
    wrong = mt['uv'][mt['faces']] - mt['uv'][mt['uv_idx']]                     # what indexing uv through `faces` would change
    assert (np.abs(wrong).max((1, 2)) >= 1 / 16).all()
  if name == 'tex_perspective':
    assert 'slow' in R.face_classes(c, 0, 1) and 'slow' in R.face_classes(c, 4, 5)
    assert c['w'].min() == 1 and c['w'].max() == 4
  if name in R.LIT_CASES:
    n = mt['vnormals'].astype(np.float64)
    assert len(np.unique(n, axis=0)) == len(n) and not np.array_equal(c['poses'][0][:3, :3], np.eye(3))
    for var in R.shade_variants(name):
      clipped0 = clipped1 = 0
      for h in _hyps(c):
        s = R.shade_float64(c, h, **shade_light(var))
        clipped0 += int((s['dvert'] < -0.05).sum())
        clipped1 += int((s['preclip'] > 1.01).sum())
        g = R.interp_float64(c, h)                   # |sum uvw_k n_k| against sum uvw_k |n_k|: how much the interpolation shortens the normal
        short = np.linalg.norm((g['uvw'][..., None] * n[g['vid']]).sum(-2), axis=-1) / (g['uvw'] * np.linalg.norm(n, axis=1)[g['vid']]).sum(-1)
        assert short[g['covered']].min() > 0.68
      assert clipped0 >= 5, (var, clipped0)                                   # some normals face away: the clip at 0 acts (5 hypotheses x vertices)
      if var == 'bright':
        assert clipped1 >= 100, clipped1                                      # ... and the final clip at 1


def _grid_expected(c, h):
  """closed form of tex_identity / tex_identity_5x7 / tex_corners in integers: (rows, cols, value) of every pixel inside the quad"""
  i0, j0, pw, ph, half = c['claims']['grid']
  tex = c['mesh_tensors']['tex'][0].astype(np.float64)
  Ht, Wt = tex.shape[:2]
  dx, dy = c['shifts'][h]
  assert dx % 16 == 0 and dy % 16 == 0
  out = {}
  for j in range(64):
    for i in range(64):
      ti, tj = i - i0 - dx // 16, (j0 + dy // 16 + ph - 1) - j            # texel steps right of the quad's left edge / below its top edge (rows bottom-up)
      if half == 0:
        if 0 <= ti < pw and 0 <= tj < ph:
          out[(63 - j, i)] = tex[tj % Ht, ti % Wt]
      elif 0 <= ti <= pw and 0 <= tj + 1 <= ph:                # (the closed box: the fill rule keeps one of each pair of opposite boundary lines)
        # corners on pixel centres: the centre (i, j) sits on the corner between texel columns ti - 1, ti and rows tj, tj + 1 counted from the top vertex row
        tj += 1
        out[(63 - j, i)] = (tex[(tj - 1) % Ht, (ti - 1) % Wt] + tex[(tj - 1) % Ht, ti % Wt] + tex[tj % Ht, (ti - 1) % Wt] + tex[tj % Ht, ti % Wt]) / 4
  return out


@pytest.mark.parametrize('name', ['tex_identity', 'tex_identity_5x7', 'tex_corners'])
def test_reference_fetch_equals_the_texel_and_the_four_texel_mean(name):
  """closed forms that do not go through fetch_float64: where every pixel centre is a texel centre the colour IS the texel (row 0 of the texture at the
  top of the quad, column 0 at its left: no flip, no transposition), half a texel further it is the mean of the four texels around the corner"""
  c = R.lattice_case(name)
  for h in _hyps(c):
    cov = R.coverage_exact(c, h)
    s = R.shade_float64(c, h, cov)
    want = _grid_expected(c, h)
    inside = np.zeros((64, 64), bool)
    for (r, i), v in want.items():
      inside[r, i] = True
      if cov['face'][r, i] >= 0:
        assert np.abs(s['color'][r, i] - v).max() <= (0 if c['claims']['exact'] else 1e-13), (name, h, r, i)
    assert not (s['covered'] & ~inside).any() and s['covered'].sum() == c['claims']['grid'][2] * c['claims']['grid'][3]


def test_reference_fetch_wraps_periodically():
  """tex_wrap in closed form from integers (2 x = k - 21, 4 y = l - 22 for the k-th column / l-th row of the quad), the blend of the last with the
  first column where u = 0 and u = 1 fall on pixel centres, the period of 16 px, and whole periods added to every uv (tex_wrap_shifted)"""
  c, c2 = R.lattice_case('tex_wrap'), R.lattice_case('tex_wrap_shifted')
  tex = c['mesh_tensors']['tex'][0].astype(np.float64)
  Ht, Wt = tex.shape[:2]
  for h in _hyps(c):
    cov = R.coverage_exact(c, h)
    s, s2 = R.shade_float64(c, h, cov), R.shade_float64(c2, h)
    assert np.array_equal(s['covered'], s2['covered']) and np.abs(s['color'] - s2['color']).max() <= 1e-13
    both = s['covered'][:, 16:] & s['covered'][:, :-16]
    assert both.sum() > 1500 and np.abs(s['color'][:, 16:] - s['color'][:, :-16])[both].max() <= 1e-13
    both = s['covered'][16:] & s['covered'][:-16]
    assert both.sum() > 1500 and np.abs(s['color'][16:] - s['color'][:-16])[both].max() <= 1e-13
    dx, dy = c['shifts'][h]
    seen = set()
    for r in range(64):
      for i in range(64):
        if not s['covered'][r, i]:
          continue
        k, l = i - 4 - dx // 16, (60 + dy // 16) - (63 - r)          # pixel steps right of the left edge (u = -1.25) / below the top edge (v = -1.25)
        assert 0 <= k <= 56 and 0 <= l <= 56
        xf, xr, yf, yr = (k - 21) // 2, (k - 21) % 2, (l - 22) // 4, (l - 22) % 4
        a = tex[yf % Ht, xf % Wt] * (2 - xr) / 2 + tex[yf % Ht, (xf + 1) % Wt] * xr / 2
        b = tex[(yf + 1) % Ht, xf % Wt] * (2 - xr) / 2 + tex[(yf + 1) % Ht, (xf + 1) % Wt] * xr / 2
        assert np.abs(s['color'][r, i] - (a * (4 - yr) / 4 + b * yr / 4)).max() <= 1e-13, (h, r, i)
        if k in (20, 36):                     # u = 0, u = 1: x = -0.5 and Wt - 0.5, half the last column and half the first
          assert xf % Wt == Wt - 1 and xr == 1
          seen.add(k)
    assert seen == {20, 36}


def test_reference_lambert_term_of_a_flat_quad():
  """One normal for the whole quad: colour = base (w_ambient + w_diffuse d) (or base w_ambient + d light_color w_diffuse) with d from Pythagorean
  triples by hand; the point light's per-vertex d = p_z / |p| for a light at the camera and a normal along -z."""
  def flat(ncam):
    m = R._Mesh()
    R._quad(m, R._c(8), R._c(8), R._c(40), R._c(40))
    return R._finish('flat', m, {}, normals_cam=np.tile(np.asarray(ncam, np.float32), (4, 1)), rot=R.LIT_ROT)
  c = flat((0, 0.75, -1))
  base = R.interp_float64(c, 0)['color']
  for light_dir, d in (((0, 0, 1), 0.8), ((0, -3, 4), 1.0), ((0, 4, 3), 0.0), ((0, 3, -4), 0.0), ((3, 0, 4), 0.64)):
    s = R.shade_float64(c, 0, use_light=True, light_dir=light_dir)
    np.testing.assert_allclose(s['color'], np.clip(base * (0.8 + 0.5 * d), 0, 1), atol=1e-14)
    s = R.shade_float64(c, 0, use_light=True, light_dir=light_dir, light_color=(1.0, 0.5, 0.25), w_ambient=0.5, w_diffuse=0.25)
    want = np.clip(base * 0.5 + d * np.array([1.0, 0.5, 0.25]) * 0.25, 0, 1) * s['covered'][..., None]
    np.testing.assert_allclose(s['color'], want, atol=1e-14)
    assert np.abs(s['normal'][s['covered']] - np.array([0, 0.6, -0.8])).max() <= 1e-14 and not s['normal'][~s['covered']].any()
  c = flat((0, 0, -1))
  s = R.shade_float64(c, 1, use_light=True, light_dir=None, light_pos=(0, 0, 0))
  p = R._cam64(c, 1)
  assert np.all(p[:, 2] == 1) and np.abs(p[:, :2]).max() > 0.2
  np.testing.assert_allclose(s['dvert'], 1 / np.sqrt(1 + p[:, 0] ** 2 + p[:, 1] ** 2), atol=1e-14)


def _wrong_fetch(c, h, what):
  """the reference's colour with one rule broken"""
  g = R.interp_float64(c, h)
  mt = c['mesh_tensors']
  tex = mt['tex'][0].astype(np.float64)
  Ht, Wt = tex.shape[:2]
  uvw = g['uvw']
  idx = mt['faces'][g['tri']] if what == 'uv_through_faces' else mt['uv_idx'][g['tri']]
  if what == 'affine_uv':
    lam = np.moveaxis(R.coverage_exact(c, h)['lam'], 0, -1)
    uvw = lam / np.where(g['covered'], lam.sum(-1), 1.0)[..., None]
  t = (uvw[..., None] * mt['uv'].astype(np.float64)[idx]).sum(-2)
  u, v = t[..., 0], t[..., 1]
  if what == 'no_half_texel':
    u, v = u + 0.5 / Wt, v + 0.5 / Ht
  elif what == 'v_flip':
    v = 1 - v
  elif what == 'swap_uv':
    u, v = v, u
  elif what == 'swapped_stride':                          # rows addressed with the height as the stride
    flat = tex.reshape(-1, 3)
    x, y = u * Wt - 0.5, v * Ht - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    c0, r0 = np.mod(x0, Wt).astype(int), np.mod(y0, Ht).astype(int)
    c1, r1 = (c0 + 1) % Wt, (r0 + 1) % Ht
    at = lambda r, cc: flat[(r * Ht + cc) % len(flat)]
    col = (1 - fy) * ((1 - fx) * at(r0, c0) + fx * at(r0, c1)) + fy * ((1 - fx) * at(r1, c0) + fx * at(r1, c1))
    return np.where(g['covered'][..., None], col, 0.0)
  elif what == 'clamp':
    u, v = np.clip(u, 0.5 / Wt, 1 - 0.5 / Wt), np.clip(v, 0.5 / Ht, 1 - 0.5 / Ht)
  elif what == 'nearest':
    u, v = (np.floor(u * Wt) + 0.5) / Wt, (np.floor(v * Ht) + 0.5) / Ht
  return np.where(g['covered'][..., None], R.fetch_float64(tex, u, v), 0.0)


WRONG_FETCHES = [('no_half_texel', 'tex_identity'), ('no_half_texel', 'tex_corners'), ('v_flip', 'tex_identity'), ('swap_uv', 'tex_identity'),
                 ('swapped_stride', 'tex_identity'), ('swapped_stride', 'tex_identity_5x7'), ('uv_through_faces', 'tex_charts'), ('uv_through_faces', 'tex_atlas'),
                 ('affine_uv', 'tex_perspective'), ('clamp', 'tex_wrap'), ('nearest', 'tex_corners'), ('nearest', 'tex_wrap')]


@pytest.mark.parametrize('what,name', WRONG_FETCHES, ids=['%s-%s' % w for w in WRONG_FETCHES])
def test_wrong_fetches_are_rejected(what, name):
  """each broken rule moves some pixel of its case by more than a hundred tolerances"""
  c = R.lattice_case(name)
  err = np.abs(_wrong_fetch(c, 0, what) - R.shade_float64(c, 0)['color']).max()
  assert err > 100 * R.shade_tol(c), (what, name, err)


def test_shade_emulation_lies_inside_the_tolerance():
  worst = worst_n = 0.0
  for name in R.SHADE_CASES:
    c = R.lattice_case(name)
    for var in R.shade_variants(name):
      ec = 0.0
      for h in _hyps(c):
        cov = R.coverage_exact(c, h)
        ref, emu = R.shade_float64(c, h, cov, **shade_light(var)), R.emulate_shade_f32(c, h, cov, **shade_light(var))
        ec = max(ec, float(np.abs(emu['color'] - ref['color']).max()))
        worst_n = max(worst_n, float(np.abs(emu['normal'] - ref['normal']).max()))
        if c['claims'].get('exact') and var is None:
          assert np.array_equal(emu['color'].astype(np.float64), ref['color']), (name, h)
      scale = R.shade_tol(c, **shade_light(var)) / R.TOL_TEX
      print('%-18s %-14s emulated colour error %.3e = %.3e x scale %.2f' % (name, var, ec, ec / scale, scale))
      worst = max(worst, ec / scale)
  print('emulated max error / scale %.3e (recorded %.3e); normal map %.3e (EMU_ATTR %.3e)' % (worst, R.EMU_TEX, worst_n, R.EMU_ATTR))
  assert 0.5 * R.EMU_TEX < worst <= R.EMU_TEX and worst_n <= R.EMU_ATTR
  assert R.TOL_TEX == 4 * R.EMU_TEX


def render_shaded(render, c, n, dev=None, **light):
  """the case's n first hypotheses with nvdiffrast_render's light arguments: dict(color, normal, rast) of numpy arrays"""
  import torch
  to = (lambda x: torch.as_tensor(x)) if dev is None else (lambda x: torch.as_tensor(x).to(dev))
  mt = {k: to(v) for k, v in c['mesh_tensors'].items()}
  extra = {'rast': None}
  color, depth, normal = render(K=c['K'], H=c['H'], W=c['W'], ob_in_cams=to(c['poses'][:n]), mesh_tensors=mt, projection_mat=c['projection_mat'],
                                bbox2d=None if c['bbox2d'] is None else to(c['bbox2d'][:n]), output_size=(c['Ho'], c['Wo']), get_normal=True, extra=extra,
                                **light)
  return dict(color=color.cpu().numpy(), normal=normal.cpu().numpy(), rast=extra['rast'].cpu().numpy())


@functools.lru_cache(maxsize=None)
def _shade_reference(name, h, var):
  """(coverage, float64 images) of a SHADE case, computed once and shared by everything that compares with it; never modified"""
  c = R.lattice_case(name)
  cov = R.coverage_exact(c, h)
  return cov, R.shade_float64(c, h, cov, **shade_light(var))


def compare_shaded(c, got, n, what, var=None):
  """winner exactly on every pixel; colour within shade_tol - bit for bit where the case is exact -, normal map within TOL_ATTR, both exactly 0 outside
  coverage; tex_atlas: within 1e-5 of a colour step of the face's own colour.  Returns the largest |err| / tol (colour, normal)."""
  light = shade_light(var)
  tol = R.shade_tol(c, **light)
  worst = [0.0, 0.0]
  for h in range(n):
    cov, ref = _shade_reference(c['name'], h, var)
    ids = got['rast'][h][..., 3].astype(np.int64)
    assert np.array_equal(ids, cov['face'] + 1), (what, c['name'], h)
    col, nrm = got['color'][h].astype(np.float64), got['normal'][h].astype(np.float64)
    assert not col[~ref['covered']].any() and not nrm[~ref['covered']].any(), (what, c['name'], h)
    ec, en = np.abs(col - ref['color']).max(), np.abs(nrm - ref['normal']).max()
    worst = [max(worst[0], ec / tol), max(worst[1], en / R.TOL_ATTR)]
    if c['claims'].get('exact') and var is None:
      assert np.array_equal(col, ref['color']), (what, c['name'], h, ec)
    if c['claims'].get('atlas'):
      own = R.atlas_face_colors().astype(np.float64)[cov['face']]
      step = float(c['mesh_tensors']['tex'].max())
      bleed = np.abs(col - own)[ref['covered']].max()
      assert bleed <= 1e-5 * step, (what, h, bleed)
  print('%s %-18s %-14s largest |err| / tol: colour %.3f (tol %.2e), normal %.3f' % (what, c['name'], var, worst[0], tol, worst[1]))
  assert worst[0] <= 1 and worst[1] <= 1, (what, c['name'], var, worst)
  return worst


@pytest.mark.parametrize('name', R.SHADE_CASES)
def test_cpu_mirror_shades_like_the_float64_reference(name):
  """oracle/render.py (the mirror the kernel is compared with on real meshes) on the independent footing of shade_float64"""
  from oracle.render import nvdiffrast_render
  c = R.lattice_case(name)
  for var in R.shade_variants(name):
    compare_shaded(c, render_shaded(nvdiffrast_render, c, 5, **shade_light(var)), 5, 'mirror', var)


def far_uv_case(U, V):
  """tex_identity's quad (power-of-two legs: barycentrics of at most 6 bits) with a 5 x 7 texture and ONE uv, of few bits, for all corners, so that the
  interpolated uv is (U, V) exactly at every pixel; and the colour the contract gives it: x = u Wt - 0.5 and y = v Ht - 0.5 as float32 computes them
  (the product, then the difference), the indices floor(.) modulo the size in Python integers, the weights the fractional parts."""
  m = R._Mesh()
  R._quad(m, 256, 384, 256 + 512, 384 + 256)
  tex = R._distinct_texture(5, 7, 507)
  uv = np.array([U, V], np.float32)
  assert uv[0] == U and uv[1] == V
  c = R._finish('far_uv', m, {}, tex=tex, corner_uv=np.tile(uv.astype(np.float64), (2, 3, 1)))
  tex = tex.astype(np.float64)
  x, y = np.float32(uv[0] * np.float32(7)) - np.float32(0.5), np.float32(uv[1] * np.float32(5)) - np.float32(0.5)
  x0, y0 = int(np.floor(float(x))), int(np.floor(float(y)))
  fx, fy = float(x) - x0, float(y) - y0
  a = tex[y0 % 5, x0 % 7] * (1 - fx) + tex[y0 % 5, (x0 + 1) % 7] * fx
  b = tex[(y0 + 1) % 5, x0 % 7] * (1 - fx) + tex[(y0 + 1) % 5, (x0 + 1) % 7] * fx
  return c, a * (1 - fy) + b * fy


FAR_UV = [(1e6, -1e6), (-1e6, 1e6), (3 * 2.0 ** 30, -5 * 2.0 ** 30), (-2.0 ** 40, 3 * 2.0 ** 36), (2.0 ** 31, -2.0 ** 31)]


@pytest.mark.parametrize('U,V', FAR_UV)
def test_cpu_mirror_fetch_far_from_the_origin(U, V):
  """uv = +-1e6 (a million periods away: x = 7e6 - 0.5, exact in float32) and |uv size| beyond the int range, where x is a whole number and the index
  its residue - reduced in float, since the conversion to int alone cannot hold it: the float32 result equals the contract's exactly"""
  from oracle.render import nvdiffrast_render
  c, want = far_uv_case(U, V)
  got = render_shaded(nvdiffrast_render, c, 1)
  covered = got['rast'][0][..., 3] > 0
  assert covered.sum() == 512 and np.array_equal(got['color'][0][covered].astype(np.float64), np.tile(want, (512, 1))), (got['color'][0][covered][0], want)
