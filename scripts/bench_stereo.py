"""Device time of depth from a stereo pair (fp_stereo_sgm) with HIP events around the call: after a warm-up the minimum and the median of
--reps timed calls, at 640 x 480 with 64 and 128 disparities and at 1920 x 1200 with 128, with all 8 paths and with the 4 axis-aligned
ones, on a random-dot pair with a disparity ramp.  Beside each: the bytes the call must move (the census images, S written once and
read-modified-written by every further direction, S read by the winner pass, the outputs) and the share of the HBM peak (8 TB/s) they
amount to - a path walk is a chain of dependent steps per wave, so a small share means that the chain's latency sets the time, not
bytes.  The time per stage comes from the context's own profiling events (stereo_census, stereo_paths, stereo_winner) over further
calls of the same kind.  Also: the numpy restatement (tests/stereo_oracle.py) at the largest size it finishes in a few seconds, checked
equal to the device; and one textured model over a textured plane rendered by this library's rasteriser from two cameras one baseline
apart: the share of valid pixels and the median and 90th percentile of |disparity - fx b / z| against the left render's depth.
Every case runs in a child process of its own under a time limit; the first one that fails ends the run.  Prints one JSON line.
usage: python scripts/bench_stereo.py [--reps R] [--out profiles/bench_stereo.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

HBM_PEAK_GBS = 8000.0
CASES = [('640x480_d64_p8', 480, 640, 64, 0xFF), ('640x480_d64_p4', 480, 640, 64, 0x0F), ('640x480_d128_p8', 480, 640, 128, 0xFF),
         ('640x480_d128_p4', 480, 640, 128, 0x0F), ('1920x1200_d128_p8', 1200, 1920, 128, 0xFF), ('1920x1200_d128_p4', 1200, 1920, 128, 0x0F)]
HOST_CASE = (480, 640, 64)      # the restatement takes about 4 s there
CASE_LIMIT_S = 150


def ramp_pair(H, W, D, seed=0):
  """Random dots, smoothed a little; the disparity of row y is 4 + (D - 12) y / H, so every part of the range is used."""
  rng = np.random.default_rng(seed)
  tex = rng.integers(0, 256, (H, W + D)).astype(np.float32)
  tex = ((tex + np.roll(tex, 1, 1) + np.roll(tex, 1, 0) + np.roll(np.roll(tex, 1, 0), 1, 1)) / 4).astype(np.uint8)
  left, right = np.empty((H, W), np.uint8), np.empty((H, W), np.uint8)
  for y in range(H):
    d = 4 + (D - 12) * y // H
    right[y] = tex[y, D:D + W]
    left[y] = tex[y, D - d:D - d + W]
  return left, right


def bytes_needed(H, W, D, n_paths):
  px = H * W
  return px * (2 + 16 + 16 * n_paths) + px * D * 2 * (2 * n_paths - 1) + px * D * 2 + px * (8 + 8 + 6 + 8)


def timed_case(name, H, W, D, paths, reps):
  import torch
  from foundationpose_amd import _lib, stereo
  dev = torch.device('cuda', 0)
  ctx = _lib.Context.get(dev)
  left, right = (torch.as_tensor(a, device=dev) for a in ramp_pair(H, W, D))
  call = lambda: stereo.sgm(left, right, max_disparity=D, paths=paths, fx=0.9 * W, baseline=0.12)
  for _ in range(3):
    call()
  torch.cuda.synchronize()
  ms = []
  for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    disparity, depth, _ = call()
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
  ctx.prof_enable(True)
  ctx.prof_reset()
  n_prof = 5
  for _ in range(n_prof):
    call()
  torch.cuda.synchronize()
  stages = {k: ctx.prof_read(k)['total_ms'] / n_prof for k in ('stereo_census', 'stereo_paths', 'stereo_winner')}
  ctx.prof_enable(False)
  n_paths = bin(paths).count('1')
  need = bytes_needed(H, W, D, n_paths)
  t = float(np.min(ms))
  d = disparity[0].cpu().numpy()
  truth = (4 + (D - 12) * np.arange(H) // H)[:, None]
  ok = (d >= 0) & (np.arange(W)[None, :] >= D)
  return dict(case=name, H=H, W=W, max_disparity=D, paths=n_paths, ms_min=t, ms_median=float(np.median(ms)), reps=reps, bytes=int(need),
              GBs=need / (t * 1e-3) / 1e9, hbm_fraction=need / (t * 1e-3) / 1e9 / HBM_PEAK_GBS, cells_per_s=H * W * D * n_paths / (t * 1e-3),
              stage_ms=stages, valid_fraction=float((d >= 0).mean()),
              within_one_of_truth=float((np.abs(d - truth)[ok] <= 1).mean()) if ok.any() else None)


def host_case():
  import torch
  from foundationpose_amd import stereo
  from tests import stereo_oracle as O
  H, W, D = HOST_CASE
  left, right = ramp_pair(H, W, D)
  t0 = time.perf_counter()
  ref = O.sgm(left, right, max_disparity=D)
  host_s = time.perf_counter() - t0
  dev = torch.device('cuda', 0)
  l, r = torch.as_tensor(left, device=dev), torch.as_tensor(right, device=dev)
  for _ in range(3):
    got = stereo.sgm(l, r, max_disparity=D)[0]
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  got = stereo.sgm(l, r, max_disparity=D)[0]
  e1.record()
  torch.cuda.synchronize()
  same = bool((got[0].cpu().numpy().view(np.uint32) == ref['disparity'].view(np.uint32)).all())
  return dict(case='numpy_restatement', H=H, W=W, max_disparity=D, paths=8, host_ms=host_s * 1e3, device_ms=e0.elapsed_time(e1), host_equals_device=same)


def render_case():
  """The textured mustard bottle 0.75 m in front of a noise-textured plane at 1.2 m, rendered from two cameras 0.12 m apart."""
  import torch
  from foundationpose_amd import Utils as U
  from foundationpose_amd import stereo, synthetic as S
  from foundationpose_amd.mesh_tensors import make_mesh_tensors
  H, W, D, b = 480, 640, 128, 0.12
  K = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])
  rs = np.random.RandomState(0)
  obj = S.make_mustard_mesh(seed=0, textured=True)
  hw = 1.0      # the plane's half width in metres: wider than both frusta at 1.2 m
  plane = S.SimpleMesh(np.array([[-hw, -hw, 0], [hw, -hw, 0], [hw, hw, 0], [-hw, hw, 0.0]]), np.array([[0, 1, 2], [0, 2, 3]]),
                       vertex_normals=np.tile([0.0, 0, -1], (4, 1)))
  img = np.kron((rs.uniform(0, 1, size=(256, 256, 3)) * 255).astype(np.uint8), np.ones((2, 2, 1), np.uint8))      # 4 mm texels, ~2 pixels at 1.2 m
  plane.visual = S.TextureVisual(uv=np.array([[0, 0], [1, 0], [1, 1], [0, 1.0]]), image=img)
  pose_obj = np.eye(4)
  pose_obj[:3, :3] = S.random_rotation(np.random.RandomState(1000))
  pose_obj[:3, 3] = [0.02, -0.03, 0.75]
  pose_plane = np.eye(4)
  pose_plane[2, 3] = 1.2
  views = []
  for shift in (0.0, b):      # the right camera sits at x = +b: everything moves by -b in its frame
    col, dep = None, None
    for mesh, pose in ((obj, pose_obj), (plane, pose_plane)):
      p = pose.copy()
      p[0, 3] -= shift
      c, d, _ = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=p[None].astype(np.float32), mesh_tensors=make_mesh_tensors(mesh))
      c, d = c[0], d[0]
      if col is None:
        col, dep = c, d
      else:
        front = (d > 0) & ((dep <= 0) | (d < dep))
        col, dep = torch.where(front[..., None], c, col), torch.where(front, d, dep)
    views.append(((col.clamp(0, 1) * 255).round().to(torch.uint8).contiguous(), dep))
  (left, z), (right, _) = views
  disparity = stereo.sgm(left, right, max_disparity=D)[0][0].cpu().numpy()
  z = z.cpu().numpy()
  seen = z > 0
  valid = (disparity >= 0) & seen
  err = np.abs(disparity - K[0, 0] * b / np.where(seen, z, 1))[valid]
  return dict(case='rendered_pair', H=H, W=W, max_disparity=D, paths=8, fx=K[0, 0], baseline=b, valid_fraction=float((disparity >= 0).mean()),
              valid_fraction_right_of_band=float((disparity[:, D:] >= 0).mean()), disparity_error_median=float(np.median(err)),
              disparity_error_p90=float(np.percentile(err, 90)), object_pixels=int((z < 1.0)[seen].sum()),
              object_valid_fraction=float(valid[seen & (z < 1.0)].mean()))


def run_case(name, reps):
  if name == 'numpy_restatement':
    return host_case()
  if name == 'rendered_pair':
    return render_case()
  return timed_case(*next(c for c in CASES if c[0] == name), reps)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  ap.add_argument('--case', default=None, help='run this one case in this process and print its JSON (what the driver starts)')
  args = ap.parse_args()
  if args.case:
    print('RESULT ' + json.dumps(run_case(args.case, args.reps)))
    return
  res = dict(reps=args.reps, hbm_peak_GBs=HBM_PEAK_GBS, kernel_form='one wave per path line, disparities on the lanes; eight launches add into S', runs=[])
  for name in [c[0] for c in CASES] + ['numpy_restatement', 'rendered_pair']:
    # a fresh process per case, under its own time limit; a case that fails or hangs ends the run: nothing more is started on the device
    try:
      p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', name, '--reps', str(args.reps)], capture_output=True, text=True,
                         timeout=CASE_LIMIT_S)
      status, text = p.returncode, p.stdout[-2000:] + p.stderr[-4000:]
      line = next((l for l in p.stdout.splitlines() if l.startswith('RESULT ')), None)
    except subprocess.TimeoutExpired:
      status, text, line = 124, f'no result within {CASE_LIMIT_S} s', None
    if status != 0 or line is None:
      sys.stderr.write(text + '\n')
      res['stopped_at'] = dict(case=name, exit_status=status)
      break
    res['runs'].append(json.loads(line[7:]))
  line = json.dumps(res)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(line + '\n')
  if 'stopped_at' in res:
    raise SystemExit(f"bench_stereo: case {res['stopped_at']['case']} failed; nothing was started after it")


if __name__ == '__main__':
  main()
