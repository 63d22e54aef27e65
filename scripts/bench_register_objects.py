"""Registering several objects of one frame: (a) four sequential FoundationPose.register() calls against (b) ONE
MultiObjectTracker.register() (fp_register_objects) for the same four objects - four distinct meshes, one 480x640 RGB-D frame
z-composited from their renders, numpy frame in, numpy poses out, iteration=5.  One process, the same frame; after warm-up the two forms
alternate (a, b, a, b, ...) so that clock and power drift hit both alike.  (b1) is (b) with every object in a network pass of its own
(max_pass_hyp=1) instead of one pass of 4 x 252.  Prints one JSON line: min / median / max of each form in ms, the per-object figure and
whether the results agree.  REPS=n sets the number of repetitions (at least 20)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main():
  from foundationpose_amd import synthetic as S
  from foundationpose_amd.Utils import nvdiffrast_render
  from foundationpose_amd.config import REFINE_DEFAULT, SCORE_DEFAULT
  from foundationpose_amd.estimater import FoundationPose
  from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
  from foundationpose_amd.predict_score import ScorePredictor
  from foundationpose_amd.tracking import MultiObjectTracker
  dev = torch.device('cuda', 0)
  reps = max(20, int(os.environ.get('REPS', '24')))
  refiner = PoseRefinePredictor(state_dict=S.make_refine_state_dict(0), cfg=REFINE_DEFAULT, device=dev)
  scorer = ScorePredictor(state_dict=S.make_score_state_dict(1), cfg=SCORE_DEFAULT, device=dev)
  ests = []
  for o, (nt, nz) in enumerate([(96, 84), (80, 70), (88, 76), (64, 60)]):
    mesh = S.make_mustard_mesh(seed=o, n_theta=nt, n_z=nz)
    np.random.seed(0)
    ests.append(FoundationPose(model_pts=mesh.vertices, model_normals=mesh.vertex_normals, mesh=mesh, refiner=refiner, scorer=scorer))
  H, W, K = 480, 640, S.YCB_K
  g = torch.Generator(device=dev).manual_seed(7)
  vs, us = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing='ij')
  rgb = torch.stack([0.5 + 0.3 * torch.sin(us * 0.07) * torch.cos(vs * 0.05), 0.45 + 0.3 * torch.sin(us * 0.031 + vs * 0.043),
                     0.4 + 0.25 * torch.cos(vs * 0.09 - us * 0.02)], -1)
  depth = torch.full((H, W), 1.2, device=dev)
  owner = torch.full((H, W), -1, device=dev, dtype=torch.int32)
  for o, e in enumerate(ests):
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = S.random_rotation(np.random.RandomState(o + 1))
    pose[:3, 3] = (-0.09 + 0.06 * o, -0.05 + 0.04 * o, 0.72 + 0.04 * o)
    c, d, _ = nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=torch.as_tensor(pose, device=dev).reshape(1, 4, 4), mesh_tensors=e.mesh_tensors, use_light=True)
    near = (d[0] > 0) & (d[0] < depth)
    depth, rgb, owner = torch.where(near, d[0], depth), torch.where(near[..., None], c[0], rgb), torch.where(near, torch.full_like(owner, o), owner)
  rgb = (rgb * 255 + torch.randn(rgb.shape, device=dev, generator=g) * 1.5).clamp(0, 255).to(torch.uint8).cpu().numpy()
  depth = (depth + torch.randn(depth.shape, device=dev, generator=g) * 0.001).cpu().numpy()
  owner = owner.cpu().numpy()
  masks = [owner == o for o in range(4)]
  tracker = MultiObjectTracker(ests)
  refiner.ctx.reserve(1008)

  def separate():
    return np.stack([e.register(K, rgb, depth, m, iteration=5) for e, m in zip(ests, masks)])

  forms = {'a_register_x4': separate, 'b_register_objects': lambda: tracker.register(rgb, depth, K, masks, iteration=5),
           'b1_register_objects_pass_per_object': lambda: tracker.register(rgb, depth, K, masks, iteration=5, max_pass_hyp=1)}
  results = {}
  for _ in range(3):
    for name, fn in forms.items():
      results[name] = fn()
  torch.cuda.synchronize()
  times = {name: [] for name in forms}
  for _ in range(reps):
    for name, fn in forms.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn()
      times[name].append((time.perf_counter() - t0) * 1e3)
  out = {'reps': reps, 'iteration': 5, 'objects': 4, 'hypotheses': [len(e.rot_grid) for e in ests],
         'frame': '480x640 uint8 RGB + float32 depth + 4 boolean masks, numpy in, numpy poses out', 'order': 'interleaved a, b, b1 per repetition'}
  for name, ts in times.items():
    out[name + '_ms'] = {'min': min(ts), 'median': float(np.median(ts)), 'max': max(ts)}
  out['per_object_ms'] = {name: float(np.median(ts)) / 4 for name, ts in times.items()}
  out['b_over_a'] = out['b_register_objects_ms']['median'] / out['a_register_x4_ms']['median']
  out['b_not_slower_than_a'] = out['b_register_objects_ms']['median'] <= out['a_register_x4_ms']['max']
  out['results_equal'] = all(np.array_equal(results['a_register_x4'], r) for r in results.values())
  ctx = refiner.ctx
  ctx.prof_reset()
  ctx.prof_enable(2)
  forms['b_register_objects']()
  torch.cuda.synchronize()
  ctx.prof_enable(False)
  out['b_launches'] = {c: ctx.prof_read(c)['launches'] for c in ('prelude', 'mask_stats', 'render', 'crop')}
  ctx.prof_reset()
  print(json.dumps(out))


if __name__ == '__main__':
  main()
