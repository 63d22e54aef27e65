"""Device time of fp_texture_bake on the mesh reconstruct_object(..., max_vertices=8192) makes of 16 rendered views of 640 x 480 of the
synthetic mustard bottle (the views of scripts/bench_tsdf.py), at tex_size 1024 and 2048, with HIP events around the call: after a
warm-up the minimum and the median of --reps timed calls.  Beside each: the texels owned and coloured, the view tests a second (owned
texels x views / time) and the bytes the call must move at least - the atlas written once (3 bytes a texel, 1 for `used`), every view's
depth and colour read once (7 bytes a pixel) - as GB/s next to the HBM peak (8 TB/s): the kernel is a gather with a few dozen flops per
view test, so a small fraction of the peak means the dependent loads of the view loop, not the bytes, set the time.  Then the small
case of tests/test_gpu_texture_bake.py (80 faces, tex_size 128, five views of 64 x 48) on the device and through the numpy
restatement (tests/texture_bake_oracle.py, wall time).  Prints one JSON line.
usage: python scripts/bench_texture_bake.py [--reps R] [--out profiles/bench_texture_bake.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from foundationpose_amd import Utils as U
from foundationpose_amd import reconstruct as R
from foundationpose_amd import synthetic as S
from foundationpose_amd.mesh_tensors import make_mesh_tensors
from scripts.bench_tsdf import DIM, H, N_VIEWS, W, look_at
from tests import texture_bake_oracle as O

HBM_PEAK_GBS = 8000.0


def timed_bake(reps, **kw):
  run = lambda: U.bake_texture_arrays(**kw)
  for _ in range(3):
    tex, uv, used = run()
  torch.cuda.synchronize()
  ms = []
  for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
  T, n = int(kw['tex_size']), len(kw['cam_in_obs'])
  owned, coloured = int((used >= 0).sum().item()), int((used >= 1).sum().item())
  hw = int(np.prod(kw['depths'].shape[1:]))
  bytes_min = T * T * 4 + n * hw * 7
  best = float(np.min(ms)) * 1e-3
  return dict(tex_size=T, cell=U.texture_cell(T, len(kw['faces'])), faces=len(kw['faces']), views=n, ms_min=float(np.min(ms)),
              ms_median=float(np.median(ms)), texels_owned=owned, coverage=coloured / max(owned, 1), view_tests_per_s=owned * n / best,
              bytes_min=bytes_min, GBs=bytes_min / best / 1e9, hbm_fraction=bytes_min / best / 1e9 / HBM_PEAK_GBS), (tex, uv, used)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_texture_bake needs an MI355X'
  dev = torch.device('cuda', 0)
  src = S.make_mustard_mesh(seed=0)
  src.vertices = src.vertices - (src.vertices.min(0) + src.vertices.max(0)) / 2
  K = np.array([[800.0, 0, 319.5], [0, 800.0, 239.5], [0, 0, 1.0]])
  i = np.arange(N_VIEWS) + 0.5
  z = 1 - 2 * i / N_VIEWS
  phi = i * np.pi * (3 - np.sqrt(5))
  eyes = 0.6 * np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
  cams = np.stack([look_at(e) for e in eyes])
  color, depth, _ = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=np.linalg.inv(cams).astype(np.float32), mesh_tensors=make_mesh_tensors(src, device=dev))
  rgb = (color * 255).round().clamp(0, 255).to(torch.uint8).contiguous()
  depth = depth.contiguous()
  masks = (depth > 0).to(torch.uint8).contiguous()
  vs = 0.2 / (DIM - 1)
  mesh = R.reconstruct_object(dict(depths=depth, rgbs=rgb, masks=masks, K=K, cam_in_obs=cams), voxel_size=vs, max_vertices=8192, device=dev)
  pos = torch.as_tensor(mesh.vertices, device=dev).float().contiguous()
  faces = torch.as_tensor(mesh.faces, device=dev).int().contiguous()
  col = torch.as_tensor(mesh.visual.vertex_colors[:, :3].copy(), device=dev).contiguous()
  res = dict(reps=args.reps, hbm_peak_GBs=HBM_PEAK_GBS, image=[H, W], vertices=len(pos))
  for T in (1024, 2048):
    res[f'fused_{T}'], _ = timed_bake(args.reps, pos=pos, faces=faces, rgbs=rgb, depths=depth, K=K, cam_in_obs=cams, tex_size=T, colors=col, masks=masks,
                                      depth_tol=2 * vs)

  from tests import test_gpu_texture_bake as G             # the small case of the tests: its mesh and its five rendered views
  v, f, c = G._mesh(80)
  vw = G._views()
  small, got = timed_bake(args.reps, pos=v, faces=f, rgbs=torch.as_tensor(vw['rgbs'], device=dev), depths=torch.as_tensor(vw['depths'], device=dev), K=G.K,
                          cam_in_obs=vw['cam_in_obs'], tex_size=128, colors=c)
  wall = []
  for _ in range(5):
    t0 = time.perf_counter()
    want = O.bake(v, f, c, vw['rgbs'], vw['depths'], None, G.K, vw['cam_in_obs'], 128)
    wall.append((time.perf_counter() - t0) * 1e3)
  small['numpy_ms_min'], small['numpy_ms_median'] = float(np.min(wall)), float(np.median(wall))
  small['same_bits'] = bool(np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[2].cpu().numpy(), want[2]))
  res['small_128'] = small
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
