"""Device time of finding objects in a depth frame by template matching (fp_template_match) with HIP events around the call: after a warm-up
the minimum and the median of --reps timed calls, for a 640 x 480 and a 1920 x 1200 frame at stride 4 with 1944 templates (162 views x 12
rolls) of 64 + 48 samples of the mustard model, one and eight objects (the same set eight times), anchors 1 and 2, and for one object
with the default set of 504 templates (42 views).  graph_ms is the launch
alone, without the host work of the Python call: the call captured into a graph, events around its replay.  Beside each case, interleaved
call by call in the same process, the same rule written with torch gathers on the same device over the first --torch-templates templates
of the set (the whole set would take seconds a call); torch_ms_scaled is that time times T / torch_templates, and `torch_equal` says
whether its map over that subset has the kernel's bits.  sample_tests is live anchor pixels x templates x anchors x samples, the work without
the prune, and the rate is that over the median graph_ms - a nominal rate: the exact prune skips part of it.  Every case runs in a child
process of its own under a time limit; the first one that fails ends the run.  Prints one JSON line.
usage: python scripts/bench_detect.py [--reps R] [--out profiles/bench_detect.json]"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

# name, (H, W), objects, anchors, views
CASES = [(f'{W}x{H}_obj{n}_anchors{a}', (H, W), n, a, 162) for (H, W) in ((480, 640), (1200, 1920)) for n in (1, 8) for a in (1, 2)]
CASES += [(f'{W}x{H}_obj1_anchors1_views42', (H, W), 1, 1, 42) for (H, W) in ((480, 640), (1200, 1920))]      # the default set: 504 templates
CASE_LIMIT_S = 240
STRIDE, TOL_IN, TOL_OUT, Z_RANGE = 4, 0.015, 0.06, (0.05, 20.0)
# from scripts/kernel_resources.sh on template_match_kernel (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)
RESOURCES = dict(vgprs=140, scratch=0, lds_bytes=16384, threads=64, waves_per_simd=3, waves_per_simd_by_lds=2.5)


def frame(H, W, mesh_tensors):
  """The mustard model at 0.7 m in front of a tilted plane with blocks on it, 2 % of the pixels missing; K with a 56 degree field of view."""
  import torch
  from foundationpose_amd import Utils as U
  f = 0.94 * W
  K = np.array([[f, 0, W / 2 - 0.5], [0, f, H / 2 - 0.5], [0, 0, 1.0]])
  pose = np.eye(4)
  pose[:3, :3] = U.euler_matrix(0.4, -0.7, 1.1)[:3, :3]
  pose[:3, 3] = [0.05, -0.02, 0.7]
  obj = U.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=pose[None], mesh_tensors=mesh_tensors)[1][0].cpu().numpy()
  rng = np.random.default_rng(0)
  y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
  d = 1.1 + 0.15 * (x / W - 0.5) - 0.1 * (y / H - 0.5)
  for _ in range(12):
    r, c, s = rng.integers(0, H), rng.integers(0, W), rng.integers(W // 40, W // 10)
    d[max(r - s, 0):r + s, max(c - s, 0):c + s] = rng.uniform(0.5, 1.0)
  d = np.where(obj > 0, obj, d) + rng.normal(0, 0.001, (H, W))
  d[rng.random((H, W)) < 0.02] = 0
  return d.astype(np.float32), K


def torch_match(D, K, table, n_in, n_out, anchors, stride, tol_in, tol_out, z_range, chunk=6):
  """fp_template_match for one object in torch: fp32 in the kernel's order of operations, gathers over (templates, pixels, samples)."""
  import torch
  H, W = D.shape
  fx, fy, cx, cy = (float(np.float32(K[0, 0])), float(np.float32(K[1, 1])), float(np.float32(K[0, 2])), float(np.float32(K[1, 2])))
  rows, cols = torch.arange(0, H, stride, device=D.device), torch.arange(0, W, stride, device=D.device)
  d = D[rows][:, cols].reshape(-1)
  live = (d >= 0.001)
  bx = ((cols.float()[None, :].expand(len(rows), -1).reshape(-1) - cx) / fx) * d
  by = ((rows.float()[:, None].expand(-1, len(cols)).reshape(-1) - cy) / fy) * d
  best = torch.zeros(len(d), dtype=torch.int64, device=D.device)
  flat = D.reshape(-1)
  is_in = (torch.arange(n_in + n_out, device=D.device) < n_in)[None, None, :]
  for t0 in range(0, len(table), chunk):
    S = table[t0:t0 + chunk]                                    # (c, ns, 4)
    for a in range(anchors):
      A = S[:, a]                                               # (c, 4)
      zc = d[None, :] - A[:, 2:3]                               # (c, P)
      ok = live[None, :] & (zc >= z_range[0]) & (zc <= z_range[1])
      X = (bx[None, :] - A[:, 0:1])[:, :, None] + S[:, None, :, 0]
      Y = (by[None, :] - A[:, 1:2])[:, :, None] + S[:, None, :, 1]
      Z = zc[:, :, None] + S[:, None, :, 2]
      cf, rf = torch.floor((fx * X) / Z + cx + 0.5), torch.floor((fy * Y) / Z + cy + 0.5)
      inside = (Z >= 0.001) & (cf >= 0) & (cf <= W - 1) & (rf >= 0) & (rf <= H - 1)
      o = flat[(torch.where(inside, rf, 0.0) * W + torch.where(inside, cf, 0.0)).long()]
      read, gap = o >= 0.001, (o - Z).abs()
      n_i = (inside & is_in & read & (gap <= tol_in)).sum(-1)
      n_o = (inside & ~is_in & (~read | (gap > tol_out))).sum(-1)
      low = 0xFFFF - (4 * torch.arange(t0, t0 + len(S), device=D.device) + a)
      key = torch.where(ok, ((n_i * n_o) << 16) | low[:, None], 0)
      best = torch.maximum(best, key.max(dim=0).values)
  return best.reshape(len(rows), len(cols))


def time_interleaved(calls, reps):
  """[ms list per call]: the calls take turns, each timed with its own pair of events; reps may differ per call (reps[i] <= max)."""
  import torch
  for c in calls:
    c(), c()
  torch.cuda.synchronize()
  ms = [[] for _ in calls]
  for r in range(max(reps)):
    for i, c in enumerate(calls):
      if r >= reps[i]:
        continue
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      c()
      e1.record()
      torch.cuda.synchronize()
      ms[i].append(e0.elapsed_time(e1))
  return ms


def run_case(name, reps, torch_templates):
  import torch
  from foundationpose_amd import Utils as U
  from foundationpose_amd import detect as Dt
  from foundationpose_amd import synthetic as S
  _, (H, W), n_obj, anchors, views = next(c for c in CASES if c[0] == name)
  dev = torch.device('cuda', 0)
  mesh = S.make_mustard_mesh(seed=0, n_theta=48, n_z=42)
  mesh.vertices = mesh.vertices - (mesh.vertices.min(axis=0) + mesh.vertices.max(axis=0)) / 2
  mt = U.make_mesh_tensors(mesh)
  one = U.build_templates(mesh_tensors=mt, anchors=2, n_views=views)
  ts = Dt.TemplateSet.concat([one] * n_obj)
  depth_np, K = frame(H, W, mt)
  depth = torch.as_tensor(depth_np, device=dev)
  kw = dict(stride=STRIDE, tol_in=TOL_IN, tol_out=TOL_OUT, z_range=Z_RANGE, anchors=anchors)
  ours = lambda: Dt.match_templates(depth, K, ts, **kw)
  sub = torch.as_tensor(one.table[:torch_templates], device=dev)
  theirs = lambda: torch_match(depth, K, sub, one.n_in, one.n_out, anchors, STRIDE, TOL_IN, TOL_OUT, Z_RANGE)
  ms_ours, ms_torch = time_interleaved([ours, theirs], [reps, min(reps, 5)])
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    ours()
  ms_graph = time_interleaved([graph.replay], [reps])[0]
  # the same bits: the kernel over the same subset of templates against the torch formulation
  sub_set = Dt.TemplateSet(one.table[:torch_templates], one.rotations[:torch_templates], one.n_in, one.n_out, one.anchors, [0, torch_templates],
                           one.diameters, [])
  equal = bool((torch.as_tensor(Dt.match_templates(depth, K, sub_set, **kw)[0].cpu().numpy().astype(np.int64)) == theirs().cpu()).all())
  Hs, Ws = Dt.lattice_shape(H, W, STRIDE)
  live = int((depth[::STRIDE, ::STRIDE] >= 0.001).sum())
  T = one.n_templates
  tests = live * T * n_obj * anchors * (one.n_in + one.n_out)
  g = float(np.median(ms_graph))
  t_med = float(np.median(ms_torch))
  return dict(case=name, frame=[H, W], lattice=[Hs, Ws], live_anchor_pixels=live, objects=n_obj, templates_per_object=T, samples=[one.n_in, one.n_out],
              anchors=anchors, stride=STRIDE, reps=reps, ms_min=float(np.min(ms_ours)), ms_median=float(np.median(ms_ours)), graph_ms_min=float(np.min(ms_graph)),
              graph_ms_median=g, sample_tests=tests, nominal_sample_tests_per_s=tests / (g * 1e-3), workgroups=((Hs + 7) // 8) * ((Ws + 7) // 8) * n_obj,
              torch_templates=torch_templates, torch_ms_min=float(np.min(ms_torch)), torch_ms_median=t_med,
              torch_ms_scaled=t_med * T * n_obj / torch_templates, torch_equal=equal)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--torch-templates', type=int, default=54)
  ap.add_argument('--out', default=None)
  ap.add_argument('--case', default=None, help='run this one case in this process and print its JSON (what the driver starts)')
  args = ap.parse_args()
  if args.case:
    print('RESULT ' + json.dumps(run_case(args.case, args.reps, args.torch_templates)))
    return
  res = dict(reps=args.reps, resources=RESOURCES, register_ms=35.2,
             not_measured=['hardware counters (which unit bounds the kernel is reasoned from times and instruction counts)',
                           'an LDS window for the depth gathers', 'other tile shapes, strides and sample counts', 'build_templates',
                           'detect / register_detected end to end', 'a real sensor'],
             kernel_form='one launch: a wave per 8 x 8 tile of the anchor lattice and object, templates staged through 16 KB of LDS, depth gathers '
                         'through the vector cache, exact prune', runs=[])
  for name in [c[0] for c in CASES]:
    # a fresh process per case, under its own time limit; a case that fails or hangs ends the run: nothing more is started on the device
    try:
      p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', name, '--reps', str(args.reps), '--torch-templates',
                          str(args.torch_templates)], capture_output=True, text=True, timeout=CASE_LIMIT_S)
      status, text = p.returncode, p.stdout[-2000:] + p.stderr[-4000:]
      line = next((l for l in p.stdout.splitlines() if l.startswith('RESULT ')), None)
    except subprocess.TimeoutExpired:
      status, text, line = 124, f'no result within {CASE_LIMIT_S} s', None
    if status != 0 or line is None:
      sys.stderr.write(text + '\n')
      res['stopped_at'] = dict(case=name, exit_status=status)
      break
    res['runs'].append(json.loads(line[7:]))
    sys.stderr.write(line[:400] + '\n')
  line = json.dumps(res)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(line + '\n')
  if 'stopped_at' in res:
    raise SystemExit(f"bench_detect: case {res['stopped_at']['case']} failed; nothing was started after it")


if __name__ == '__main__':
  main()
