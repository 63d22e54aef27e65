"""Mesh / intrinsics ingestion for the estimator: Wavefront OBJ (with its .mtl texture) and Stanford PLY (ascii and
binary, the form of the BOP object models) -> SimpleMesh with angle-weighted vertex normals and vertex colours or a uv-mapped
texture array.  Images are decoded with PIL, imported only where one is decoded."""
import logging
import os
import re

import numpy as np

from .synthetic import SimpleMesh, TextureVisual


def _read_image(path):
  """An image file as (H,W,3) uint8 RGB."""
  from PIL import Image
  with Image.open(path) as im:
    return np.array(im.convert('RGB'), dtype=np.uint8)


def _mtl_texture(obj_path, mtllib, usemtl):
  """The decoded `map_Kd` image of material `usemtl` (None: the library's first material) of the .mtl file `mtllib` beside the OBJ, or
  None - with a logging line - when the library, the material, its map or the image file is missing."""
  base = os.path.dirname(os.path.abspath(obj_path))
  mtl_path = os.path.join(base, mtllib)
  if not os.path.isfile(mtl_path):
    logging.info(f'{obj_path}: material library {mtllib} not found, no texture')
    return None
  maps, order, cur = {}, [], None
  with open(mtl_path) as f:
    for line in f:
      p = line.split()
      if not p or p[0].startswith('#'):
        continue
      if p[0] == 'newmtl' and len(p) > 1:
        cur = p[1]
        order.append(cur)
      elif p[0] == 'map_Kd' and cur is not None and len(p) > 1:
        maps[cur] = p[-1]                     # (options such as -s 1 1 1 come before the file name)
  name = usemtl if usemtl in order else (order[0] if order else None)
  if name is None or name not in maps:
    logging.info(f'{obj_path}: material {usemtl!r} of {mtllib} has no map_Kd, no texture')
    return None
  img_path = os.path.join(os.path.dirname(mtl_path), maps[name].replace('\\', '/'))
  if not os.path.isfile(img_path):
    logging.info(f'{obj_path}: texture {maps[name]} of material {name!r} not found, no texture')
    return None
  return _read_image(img_path)


def load_obj(path, texture_image=None, split_uv=True):
  """Triangles and polygons (fan-triangulated); `v/vt/vn` index forms; negative (relative) indices.
  Vertices are split per (v, vt) pair when texture coordinates are present, so faces index uv directly
  (make_mesh_tensors uses `mesh.faces` as `uv_idx`, src/Utils.py:115).  split_uv=False keeps the file's vertices and faces instead and
  returns the `vt` entries as they stand with the faces' vt indices as `visual.uv_idx` - the form of a per-face atlas
  (Utils.bake_texture), which splitting would triple in vertices.  The texture is `texture_image` when given, else the `map_Kd`
  image of the material the first `usemtl` names (or the first material) in the `mtllib` file beside the OBJ - the YCB
  textured.obj + .mtl + .png form; a missing library or image leaves the mesh untextured."""
  v, vc, vt, corners = [], [], [], []
  mtllib = usemtl = None
  with open(path) as f:
    for line in f:
      p = line.split()
      if not p or p[0].startswith('#'):
        continue
      if p[0] == 'v':
        v.append([float(x) for x in p[1:4]])
        vc.append([float(x) for x in p[4:7]] if len(p) >= 7 else None)
      elif p[0] == 'vt':
        vt.append([float(p[1]), float(p[2]) if len(p) > 2 else 0.0])
      elif p[0] == 'mtllib' and mtllib is None and len(p) > 1:
        mtllib = line.split(None, 1)[1].strip()
      elif p[0] == 'usemtl' and usemtl is None and len(p) > 1:
        usemtl = p[1]
      elif p[0] == 'f':
        idx = []
        for tok in p[1:]:
          parts = tok.split('/')
          vi = int(parts[0])
          ti = int(parts[1]) if len(parts) > 1 and parts[1] else 0
          idx.append((vi - 1 if vi > 0 else len(v) + vi, (ti - 1 if ti > 0 else len(vt) + ti) if ti else -1))
        for k in range(1, len(idx) - 1):
          corners.append((idx[0], idx[k], idx[k + 1]))
  if not v or not corners:
    raise ValueError(f'{path}: no geometry')
  v = np.asarray(v, dtype=np.float64)
  use_uv = bool(vt) and all(c[1] >= 0 for tri in corners for c in tri)
  if use_uv and not split_uv:
    mesh = SimpleMesh(v, np.asarray([[c[0] for c in tri] for tri in corners], dtype=np.int64))
    if texture_image is None and mtllib is not None:
      texture_image = _mtl_texture(path, mtllib, usemtl)
    if texture_image is not None:
      mesh.visual = TextureVisual(uv=np.asarray(vt, dtype=np.float64), image=np.asarray(texture_image),
                                  uv_idx=np.asarray([[c[1] for c in tri] for tri in corners], dtype=np.int64))
    return mesh
  if use_uv:
    remap, verts, uvs, faces = {}, [], [], []
    for tri in corners:
      face = []
      for key in tri:
        if key not in remap:
          remap[key] = len(verts)
          verts.append(v[key[0]])
          uvs.append(vt[key[1]])
        face.append(remap[key])
      faces.append(face)
    mesh = SimpleMesh(np.asarray(verts), np.asarray(faces))
    if texture_image is None and mtllib is not None:
      texture_image = _mtl_texture(path, mtllib, usemtl)
    if texture_image is not None:
      mesh.visual = TextureVisual(uv=np.asarray(uvs, dtype=np.float64), image=np.asarray(texture_image))
    return mesh
  faces = np.asarray([[c[0] for c in tri] for tri in corners], dtype=np.int64)
  colors = None
  if all(c is not None for c in vc):
    rgb = np.clip(np.asarray(vc) * 255.0, 0, 255).astype(np.uint8)
    colors = np.concatenate([rgb, np.full((len(rgb), 1), 255, np.uint8)], 1)
  return SimpleMesh(v, faces, vertex_colors=colors)


def save_obj(mesh, path):
  """`v` (with colours when the mesh has vertex colours) and `f`.  A mesh whose visual carries `uv_idx` (a per-face atlas,
  Utils.bake_texture) is written with `vt`, `f v/vt`, and beside the OBJ NAME.mtl and NAME.png (the image as it stands, rows top-down,
  for uv in the OBJ convention); uv with 9 significant digits, which a float32 survives unchanged."""
  if getattr(mesh.visual, 'uv_idx', None) is not None:
    return _save_obj_atlas(mesh, path)
  colors = np.asarray(mesh.visual.vertex_colors)[:, :3] / 255.0 if hasattr(mesh.visual, 'vertex_colors') else None
  with open(path, 'w') as f:
    for i, p in enumerate(mesh.vertices):
      c = '' if colors is None else ' %.6f %.6f %.6f' % tuple(colors[i])
      f.write('v %.9g %.9g %.9g%s\n' % (p[0], p[1], p[2], c))
    for t in mesh.faces:
      f.write('f %d %d %d\n' % (t[0] + 1, t[1] + 1, t[2] + 1))


def _save_obj_atlas(mesh, path):
  from PIL import Image
  stem = os.path.splitext(os.path.basename(path))[0]
  base = os.path.dirname(os.path.abspath(path))
  Image.fromarray(np.ascontiguousarray(np.asarray(mesh.visual.image)[..., :3].astype(np.uint8))).save(os.path.join(base, stem + '.png'))
  with open(os.path.join(base, stem + '.mtl'), 'w') as f:
    f.write('newmtl material_0\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nmap_Kd %s.png\n' % stem)
  uv_idx = np.asarray(mesh.visual.uv_idx).reshape(-1, 3)
  with open(path, 'w') as f:
    f.write('mtllib %s.mtl\nusemtl material_0\n' % stem)
    for p in mesh.vertices:
      f.write('v %.9g %.9g %.9g\n' % (p[0], p[1], p[2]))
    for t in np.asarray(mesh.visual.uv):
      f.write('vt %.9g %.9g\n' % (t[0], t[1]))
    for t, u in zip(mesh.faces, uv_idx):
      f.write('f %d/%d %d/%d %d/%d\n' % (t[0] + 1, u[0] + 1, t[1] + 1, u[1] + 1, t[2] + 1, u[2] + 1))


# ---------------------------------------------------------------------------------------------- Stanford PLY
_PLY_TYPES = {'char': 'i1', 'uchar': 'u1', 'short': 'i2', 'ushort': 'u2', 'int': 'i4', 'uint': 'u4', 'float': 'f4', 'double': 'f8',
              'int8': 'i1', 'uint8': 'u1', 'int16': 'i2', 'uint16': 'u2', 'int32': 'i4', 'uint32': 'u4', 'float32': 'f4', 'float64': 'f8'}


def _ply_header(path, f):
  """-> (format, [(element name, count, [property, ...])], texture file name or None); a property is (name, type) or
  (name, count type, item type) for a list."""
  if f.readline().strip() != b'ply':
    raise ValueError(f'{path}: not a PLY file')
  fmt, elements, texture = None, [], None
  while True:
    raw = f.readline()
    if not raw:
      raise ValueError(f'{path}: the header has no end_header')
    p = raw.decode('ascii', 'replace').split()
    if not p:
      continue
    if p[0] == 'end_header':
      break
    if p[0] == 'format':
      fmt = p[1]
    elif p[0] == 'comment' and len(p) > 2 and p[1] == 'TextureFile':
      texture = raw.decode('ascii', 'replace').split(None, 2)[2].strip()
    elif p[0] == 'element':
      elements.append((p[1], int(p[2]), []))
    elif p[0] == 'property':
      if not elements:
        raise ValueError(f'{path}: a property before any element')
      try:
        prop = (p[4], _PLY_TYPES[p[2]], _PLY_TYPES[p[3]]) if p[1] == 'list' else (p[2], _PLY_TYPES[p[1]])
      except (KeyError, IndexError):
        raise ValueError(f'{path}: unknown property declaration {" ".join(p)!r}') from None
      elements[-1][2].append(prop)
  if fmt not in ('ascii', 'binary_little_endian', 'binary_big_endian'):
    raise ValueError(f'{path}: unknown PLY format {fmt!r}')
  return fmt, elements, texture


def _ply_element_binary(path, buf, off, name, count, props, order):
  """One element of a binary body -> ({scalar property: (count,) array}, {list property: list of arrays}, new offset)."""
  short = ValueError(f'{path}: the body ends inside element {name!r} (truncated file)')
  lists = [p for p in props if len(p) == 3]
  if not lists:
    dt = np.dtype([(p[0], order + p[1]) for p in props])
    if off + count * dt.itemsize > len(buf):
      raise short
    rec = np.frombuffer(buf, dtype=dt, count=count, offset=off)
    return {p[0]: rec[p[0]] for p in props}, {}, off + count * dt.itemsize
  if count == 0:
    return {p[0]: np.zeros(0, p[1]) for p in props if len(p) == 2}, {p[0]: [] for p in lists}, off
  # every row of one length (a mesh of triangles, the usual case): the rows are one record array; else row by row
  if len(lists) == 1:
    ct = np.dtype(order + lists[0][1])
    if off + ct.itemsize > len(buf):
      raise short
    n0 = int(np.frombuffer(buf, dtype=ct, count=1, offset=off + sum(np.dtype(p[1]).itemsize for p in props[:props.index(lists[0])]))[0])
    dt = np.dtype([(p[0], order + p[1]) if len(p) == 2 else (p[0], [('n', order + p[1]), ('i', order + p[2], (n0,))]) for p in props])
    if off + count * dt.itemsize <= len(buf):
      rec = np.frombuffer(buf, dtype=dt, count=count, offset=off)
      if (rec[lists[0][0]]['n'] == n0).all():
        return ({p[0]: rec[p[0]] for p in props if len(p) == 2}, {lists[0][0]: list(rec[lists[0][0]]['i'])}, off + count * dt.itemsize)
  scal = {p[0]: np.zeros(count, p[1]) for p in props if len(p) == 2}
  out = {p[0]: [] for p in lists}
  for r in range(count):
    for p in props:
      if len(p) == 2:
        dt = np.dtype(order + p[1])
        if off + dt.itemsize > len(buf):
          raise short
        scal[p[0]][r] = np.frombuffer(buf, dtype=dt, count=1, offset=off)[0]
        off += dt.itemsize
      else:
        ct, it = np.dtype(order + p[1]), np.dtype(order + p[2])
        if off + ct.itemsize > len(buf):
          raise short
        n = int(np.frombuffer(buf, dtype=ct, count=1, offset=off)[0])
        off += ct.itemsize
        if n < 0 or off + n * it.itemsize > len(buf):
          raise short
        out[p[0]].append(np.frombuffer(buf, dtype=it, count=n, offset=off))
        off += n * it.itemsize
  return scal, out, off


def _ply_element_ascii(path, lines, pos, name, count, props):
  if pos + count > len(lines):
    raise ValueError(f'{path}: the body ends inside element {name!r} (truncated file)')
  scal = {p[0]: np.zeros(count, p[1]) for p in props if len(p) == 2}
  out = {p[0]: [] for p in props if len(p) == 3}
  try:
    if not out:
      rows = np.array([ln.split()[:len(props)] for ln in lines[pos:pos + count]], dtype=np.float64).reshape(count, len(props))
      for c, p in enumerate(props):
        scal[p[0]] = rows[:, c].astype(p[1])
    else:
      for r in range(count):
        tok, k = lines[pos + r].split(), 0
        for p in props:
          if len(p) == 2:
            scal[p[0]][r] = float(tok[k])
            k += 1
          else:
            n = int(tok[k])
            if len(tok) < k + 1 + n:
              raise IndexError
            out[p[0]].append(np.array(tok[k + 1:k + 1 + n], dtype=np.float64).astype(p[2]))
            k += 1 + n
  except (ValueError, IndexError):
    raise ValueError(f'{path}: malformed row in element {name!r}') from None
  return scal, out, pos + count


def load_ply(path, texture_image=None):
  """Stanford PLY -> SimpleMesh: `format ascii 1.0`, `binary_little_endian 1.0` and `binary_big_endian 1.0`; the scalar types char ..
  double and their int8 .. float64 aliases.  Element `vertex`: x y z (required); nx ny nz -> vertex_normals (else angle-weighted,
  computed when first read); red green blue [alpha] -> (V,4) uint8 colours; texture_u texture_v (also u v, s t) -> uv.  Element `face`:
  the list property vertex_indices / vertex_index, polygons fan-triangulated as load_obj does.  Other elements and other properties are
  skipped.  With uv, the texture is `texture_image` when given, else the file a `comment TextureFile NAME` header line names, beside the
  PLY; a mesh without either shows its vertex colours, or SimpleMesh's grey.  ValueError for a malformed header, a body that ends
  early, or a vertex index out of range."""
  with open(path, 'rb') as f:
    fmt, elements, texture = _ply_header(path, f)
    body = f.read()
  data = {}
  if fmt == 'ascii':
    lines = [ln for ln in body.decode('ascii', 'replace').splitlines() if ln.strip()]
    pos = 0
    for name, count, props in elements:
      scal, lst, pos = _ply_element_ascii(path, lines, pos, name, count, props)
      data.setdefault(name, (scal, lst))
  else:
    off, order = 0, '<' if fmt == 'binary_little_endian' else '>'
    for name, count, props in elements:
      scal, lst, off = _ply_element_binary(path, body, off, name, count, props, order)
      data.setdefault(name, (scal, lst))
  if 'vertex' not in data or not all(k in data['vertex'][0] for k in 'xyz'):
    raise ValueError(f'{path}: no vertex element with x, y, z')
  vs = data['vertex'][0]
  verts = np.stack([vs['x'], vs['y'], vs['z']], 1).astype(np.float64)
  faces = []
  if 'face' in data:
    lst = data['face'][1]
    rows = lst.get('vertex_indices', lst.get('vertex_index'))
    if rows is None:
      raise ValueError(f'{path}: the face element has no vertex_indices / vertex_index list')
    if rows and all(len(r) == 3 for r in rows):
      faces = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    else:
      faces = np.asarray([(r[0], r[k], r[k + 1]) for r in rows for k in range(1, len(r) - 1)], dtype=np.int64).reshape(-1, 3)
  faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
    raise ValueError(f'{path}: a face indexes a vertex outside 0 .. {len(verts) - 1}')
  normals = np.stack([vs['nx'], vs['ny'], vs['nz']], 1).astype(np.float64) if all(k in vs for k in ('nx', 'ny', 'nz')) else None
  colors = None
  if all(k in vs for k in ('red', 'green', 'blue')):
    chans = [vs['red'], vs['green'], vs['blue'], vs['alpha'] if 'alpha' in vs else None]
    to_u8 = lambda c: np.clip(c * 255.0 if c.dtype.kind == 'f' else c, 0, 255).astype(np.uint8)
    colors = np.stack([np.full(len(verts), 255, np.uint8) if c is None else to_u8(c) for c in chans], 1)
  uv = next((np.stack([vs[a], vs[b]], 1).astype(np.float64) for a, b in (('texture_u', 'texture_v'), ('u', 'v'), ('s', 't'))
             if a in vs and b in vs), None)
  mesh = SimpleMesh(verts, faces, vertex_normals=normals, vertex_colors=colors)
  if uv is not None:
    if texture_image is None and texture is not None:
      tex_path = os.path.join(os.path.dirname(os.path.abspath(path)), texture)
      if os.path.isfile(tex_path):
        texture_image = _read_image(tex_path)
      else:
        logging.info(f'{path}: texture file {texture} not found, no texture')
    if texture_image is not None:
      mesh.visual = TextureVisual(uv=uv, image=np.asarray(texture_image))
  return mesh


def save_ply(mesh, path, binary=True, texture_file=None, normals=True):
  """Write what load_ply reads: float32 positions (and normals), then uv (float32) for a textured mesh - with `comment TextureFile
  <texture_file>` when a name is given; the image itself is not written - or uchar red green blue alpha for a coloured one, and the
  triangles as `list uchar int vertex_indices`.  binary=True: binary_little_endian; else ascii with 9 significant digits, which a
  float32 survives unchanged."""
  if getattr(mesh.visual, 'uv_idx', None) is not None:
    raise ValueError('save_ply: the mesh carries a per-face texture atlas (visual.uv_idx); a PLY holds one uv per vertex - use save_obj')
  v = np.asarray(mesh.vertices, dtype=np.float32)
  cols = [('x', v[:, 0]), ('y', v[:, 1]), ('z', v[:, 2])]
  if normals:
    n = np.asarray(mesh.vertex_normals, dtype=np.float32)
    cols += [('nx', n[:, 0]), ('ny', n[:, 1]), ('nz', n[:, 2])]
  if hasattr(mesh.visual, 'uv'):
    uv = np.asarray(mesh.visual.uv, dtype=np.float32)
    cols += [('texture_u', uv[:, 0]), ('texture_v', uv[:, 1])]
  elif getattr(mesh.visual, 'vertex_colors', None) is not None:
    c = np.asarray(mesh.visual.vertex_colors, dtype=np.uint8)
    if c.shape[1] == 3:
      c = np.concatenate([c, np.full((len(c), 1), 255, np.uint8)], 1)
    cols += [(k, c[:, i]) for i, k in enumerate(('red', 'green', 'blue', 'alpha'))]
  faces = np.asarray(mesh.faces, dtype=np.int32).reshape(-1, 3)
  names = {'f': 'float', 'u': 'uchar'}
  head = ['ply', 'format %s 1.0' % ('binary_little_endian' if binary else 'ascii')]
  if texture_file is not None and hasattr(mesh.visual, 'uv'):
    head.append(f'comment TextureFile {texture_file}')
  head += [f'element vertex {len(v)}'] + [f'property {names[a.dtype.kind]} {k}' for k, a in cols]
  head += [f'element face {len(faces)}', 'property list uchar int vertex_indices', 'end_header']
  with open(path, 'wb') as f:
    f.write(('\n'.join(head) + '\n').encode('ascii'))
    if binary:
      rec = np.zeros(len(v), dtype=[(k, '<' + a.dtype.str[1:]) for k, a in cols])
      for k, a in cols:
        rec[k] = a
      f.write(rec.tobytes())
      fr = np.zeros(len(faces), dtype=[('n', 'u1'), ('i', '<i4', (3,))])
      fr['n'], fr['i'] = 3, faces
      f.write(fr.tobytes())
    else:
      fmt = lambda x: '%.9g' % x if isinstance(x, (float, np.floating)) else '%d' % x
      for r in range(len(v)):
        f.write((' '.join(fmt(a[r]) for _, a in cols) + '\n').encode('ascii'))
      for t in faces:
        f.write(('3 %d %d %d\n' % tuple(t)).encode('ascii'))


def load_mesh(path, scale=1.0, split_uv=True):
  """A model file by its extension (.obj, .ply; any case), its vertices multiplied by `scale` - BOP models are in millimetres:
  scale=1e-3 (src/datareader.py:322).  split_uv: load_obj's (an OBJ with a per-face atlas keeps its vertex count with False)."""
  ext = os.path.splitext(path)[1].lower()
  if ext == '.obj':
    mesh = load_obj(path, split_uv=split_uv)
  elif ext == '.ply':
    mesh = load_ply(path)
  else:
    raise ValueError(f'{path}: unknown model file extension {ext!r} (.obj or .ply)')
  if scale != 1.0:
    mesh.vertices = mesh.vertices * float(scale)
  return mesh


_NUMBER = r'([-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?)'


def _calibration_section(path, text, section):
  """The text between `[section]` and the next `[` of a sectioned calibration file."""
  m = re.search(r'^[ \t]*\[' + re.escape(section) + r'\][ \t]*$(.*?)(?=^[ \t]*\[|\Z)', text, re.S | re.M)
  if m is None:
    raise ValueError(f'{path}: no section [{section}]')
  return m.group(1)


def _calibration_value(path, body, section, key):
  m = re.search(r'^[ \t]*' + re.escape(key) + r'[ \t]*=[ \t]*' + _NUMBER + r'[ \t]*$', body, re.M)
  if m is None:
    raise ValueError(f'{path}: no {key}= in section [{section}]')
  return float(m.group(1))


def _is_sectioned(text):
  first = next((l for l in text.splitlines() if l.strip()), '')
  return first.lstrip().startswith('[')


def load_intrinsics(path, camera_section='LEFT_CAM_FHD1200'):
  """3x3 matrix as 9 whitespace/comma separated numbers (the cam_K.txt convention).  A file whose first non-blank line starts with `[`
  is a stereo camera's sectioned calibration file instead (src/file_processing.py:36-81): the fx=, fy=, cx=, cy= of `[camera_section]`
  become [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]."""
  text = open(path).read()
  if _is_sectioned(text):
    body = _calibration_section(path, text, camera_section)
    fx, fy, cx, cy = (_calibration_value(path, body, camera_section, k) for k in ('fx', 'fy', 'cx', 'cy'))
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=np.float64)
  vals = np.fromstring(text.replace(',', ' '), sep=' ')
  if vals.size != 9:
    raise ValueError(f'{path}: expected 9 numbers, got {vals.size}')
  return vals.reshape(3, 3).astype(np.float64)


def load_stereo_baseline(path, scale=0.001):
  """`Baseline=` of the `[STEREO]` section of a sectioned calibration file, times `scale`, as metres.  The reference reads only the
  camera sections of that file and never says in which unit the baseline is written; cameras of this kind write millimetres, hence the
  default 0.001 - `scale` is a parameter because that is an assumption: pass 1.0 for a file in metres."""
  text = open(path).read()
  if not _is_sectioned(text):
    raise ValueError(f'{path}: not a sectioned calibration file (its first non-blank line does not start with "[")')
  return _calibration_value(path, _calibration_section(path, text, 'STEREO'), 'STEREO', 'Baseline') * float(scale)



def _calibration_optional(path, body, section, key):
  return _calibration_value(path, body, section, key) if re.search(r'^[ \t]*' + re.escape(key) + r'[ \t]*=', body, re.M) else 0.0


def _rotation_of_vector(rvec):
  """Rodrigues: the rotation by |rvec| radians about rvec, float64."""
  rvec = np.asarray(rvec, dtype=np.float64)
  theta = float(np.linalg.norm(rvec))
  if theta == 0.0:
    return np.eye(3)
  k = rvec / theta
  Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
  return np.eye(3) + np.sin(theta) * Kx + (1.0 - np.cos(theta)) * (Kx @ Kx)


def load_stereo_calibration(path, left_section='LEFT_CAM_FHD1200', right_section=None, scale=0.001):
  """Both cameras and their relative pose from a stereo camera's sectioned calibration file, as plain arrays: a dict with K1, K2 (3x3),
  dist1, dist2 (k1 k2 p1 p2 k3 of each camera section, absent keys = 0), R (3x3) and T (3) in the convention of rectify.rectify_stereo,
  x2 = R x1 + T, T in metres.  right_section defaults to left_section with LEFT replaced by RIGHT.
  **The reading of the [STEREO] section is an ASSUMPTION.**  The reference reads fx, fy, cx, cy of the camera sections only
  (src/file_processing.py:36-81) and never the [STEREO] keys, so their meaning cannot be taken from it.  Assumed here: the right camera's
  centre lies at (Baseline, TY, TZ) * scale in the left camera's frame (scale 0.001: a file in millimetres), and its orientation in that
  frame is the rotation vector (RX_<res>, CV_<res>, RZ_<res>) in radians, <res> being the resolution suffix of the section name
  (FHD1200 for LEFT_CAM_FHD1200); absent keys are 0.  With that orientation Q and centre c: R = Q^T, T = -Q^T c.  Only arrays are
  returned: a caller whose camera follows another convention builds R and T themselves from the same numbers."""
  text = open(path).read()
  if not _is_sectioned(text):
    raise ValueError(f'{path}: not a sectioned calibration file (its first non-blank line does not start with "[")')
  if right_section is None:
    if 'LEFT' not in left_section:
      raise ValueError(f'right_section must be given: "{left_section}" does not contain LEFT')
    right_section = left_section.replace('LEFT', 'RIGHT')
  out = {}
  for i, section in ((1, left_section), (2, right_section)):
    body = _calibration_section(path, text, section)
    fx, fy, cx, cy = (_calibration_value(path, body, section, k) for k in ('fx', 'fy', 'cx', 'cy'))
    out[f'K{i}'] = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=np.float64)
    out[f'dist{i}'] = np.array([_calibration_optional(path, body, section, k) for k in ('k1', 'k2', 'p1', 'p2', 'k3')], dtype=np.float64)
  stereo = _calibration_section(path, text, 'STEREO')
  res = left_section.rsplit('_', 1)[-1]
  centre = np.array([_calibration_value(path, stereo, 'STEREO', 'Baseline'), _calibration_optional(path, stereo, 'STEREO', 'TY'),
                     _calibration_optional(path, stereo, 'STEREO', 'TZ')]) * float(scale)
  Q = _rotation_of_vector([_calibration_optional(path, stereo, 'STEREO', f'{k}_{res}') for k in ('RX', 'CV', 'RZ')])
  out['R'], out['T'] = Q.T, -Q.T @ centre
  return out


RGBD_CALIBRATION_KEYS = ('K_depth', 'dist_depth', 'K_colour', 'dist_colour', 'T_colour_depth', 'size_depth', 'size_colour')


def load_rgbd_calibration(path):
  """The calibration of an RGB-D sensor whose depth and colour come from two sensors, from this project's own small JSON file (written
  down in INTEGRATION.md, "Aligning depth to the colour camera"): a dict with K_depth, K_colour (3x3), dist_depth, dist_colour (0, 4, 5
  or 8 coefficients k1 k2 p1 p2 [k3 [k4 k5 k6]]; an absent key is no distortion), T_colour_depth (4x4, metres: x_colour = T x_depth),
  size_depth and size_colour ((H, W) tuples) - the arguments of Utils.rgbd_rig, in its order.  save_rgbd_calibration writes one."""
  import json
  with open(path) as f:
    raw = json.load(f)
  if not isinstance(raw, dict):
    raise ValueError(f'{path}: expected a JSON object with the keys {", ".join(RGBD_CALIBRATION_KEYS)}')
  unknown = sorted(set(raw) - set(RGBD_CALIBRATION_KEYS))
  if unknown:
    raise ValueError(f'{path}: unknown key(s) {", ".join(unknown)} (known: {", ".join(RGBD_CALIBRATION_KEYS)})')
  out = {}
  for key in RGBD_CALIBRATION_KEYS:
    if key not in raw:
      if key.startswith('dist_'):
        out[key] = np.zeros(0)
        continue
      raise ValueError(f'{path}: the key "{key}" is missing')
    v = np.asarray(raw[key], dtype=np.float64)
    if key.startswith('K_'):
      if v.size != 9:
        raise ValueError(f'{path}: {key} must hold 3x3 numbers, got {v.size}')
      out[key] = v.reshape(3, 3)
    elif key == 'T_colour_depth':
      if v.size != 16:
        raise ValueError(f'{path}: T_colour_depth must hold 4x4 numbers, got {v.size}')
      out[key] = v.reshape(4, 4)
    elif key.startswith('size_'):
      if v.size != 2 or (v != np.round(v)).any():
        raise ValueError(f'{path}: {key} must be [H, W], got {raw[key]}')
      out[key] = (int(v.reshape(-1)[0]), int(v.reshape(-1)[1]))
    else:
      out[key] = v.reshape(-1)
  return out


def save_rgbd_calibration(path, K_depth, dist_depth, K_colour, dist_colour, T_colour_depth, size_depth, size_colour):
  """Writes the file load_rgbd_calibration reads; float64 values survive the round trip bit for bit (JSON numbers are written with repr)."""
  import json
  lists = lambda a: np.asarray(a, dtype=np.float64).tolist()
  rec = dict(K_depth=lists(np.reshape(K_depth, (3, 3))), dist_depth=lists(np.reshape([] if dist_depth is None else dist_depth, -1)),
             K_colour=lists(np.reshape(K_colour, (3, 3))), dist_colour=lists(np.reshape([] if dist_colour is None else dist_colour, -1)),
             T_colour_depth=lists(np.reshape(T_colour_depth, (4, 4))), size_depth=[int(v) for v in size_depth], size_colour=[int(v) for v in size_colour])
  with open(path, 'w') as f:
    json.dump(rec, f, indent=1)
    f.write('\n')
