"""A mesh from a folder of posed RGB-D reference views (the reference's model-free layout: rgb/, depth_enhanced/ or depth/, mask/,
cam_in_ob/, K.txt), by TSDF fusion and marching tetrahedra on the GPU (foundationpose_amd.reconstruct).
usage: python scripts/reconstruct_object.py DIR [--voxel 0.002] [--trunc T] [--min-weight 1] [--no-depth-filter] [--refine-poses | --joint-refine] [--estimate-poses]
       [--photometric [WEIGHT]]
       [--max-vertices N | --simplify-cell C] [--min-component-fraction X] [--texture [SIZE]] [--out DIR/model/model.obj]
       [--compare-to MODEL [--align]] [--align-to MODEL] [--symmetries [--symmetry-tol T]] [--segment]
The output format follows the extension: .obj or .ply.  --refine-poses aligns every view but the first to the geometry fused so far before the
fusion (reconstruct.refine_view_poses) and also writes the poses it used to DIR/cam_in_ob_refined/NAME.txt.  --joint-refine refines all poses
together from depth alone instead (reconstruct.joint_refine_view_poses: pairwise ICP, view 0 the anchor) and writes cam_in_ob_refined/ too.
--estimate-poses is for a folder WITHOUT cam_in_ob/ - a masked RGB-D sequence whose neighbouring frames overlap: the poses come from
reconstruct.estimate_view_poses (the object frame is the first camera's, moved to the object) and are written to DIR/cam_in_ob_estimated/;
it is also what happens without the flag when DIR has no cam_in_ob/.  --photometric [WEIGHT] adds the grey-value residual of the views' rgb to
--joint-refine and to the pose estimation (WEIGHT: metres per unit of intensity, default 0.03; brightness constancy is assumed - a camera
moving round a static object under fixed light); it is refused with --refine-poses, which has no such term.  --max-vertices N (8192: the
rasteriser's on-chip vertex limit) or --simplify-cell C (metres) reduces the mesh by vertex clustering (Utils.simplify_mesh).  By default
only the connected component with the most faces is kept; --min-component-fraction X (0 .. 1) keeps EVERY component with at least X of
the largest one's faces (Utils.clean_mesh: an object of several parts).  --texture bakes a texture atlas from the views' rgb onto the
finished mesh (Utils.bake_texture; SIZE: a power of two, 64 .. 4096, default: the smallest with cells of 8 texels) and writes
model.obj with model.mtl and model.png beside it; OBJ only - a PLY holds one uv per vertex, the atlas three per face.  --compare-to MODEL
(OBJ or PLY, e.g. the CAD model, in the frame and unit of the views' poses) adds one JSON line: the Chamfer and Hausdorff distance and
precision / recall / F-score of the written model against MODEL (Utils.mesh_distance; scripts/mesh_distance.py has more options).
With estimated poses the model's frame is the first camera's, not MODEL's, and those numbers describe the frame offset: --align lays the
model onto MODEL first (Utils.align_to_mesh) and they describe the surface.  --align-to MODEL goes further: the model is WRITTEN in
MODEL's frame, the poses in that frame go to DIR/cam_in_ob_aligned/NAME.txt, and the transform (`MODEL from reconstruction`, the chosen
start and the starts that fit nearly as well - a symmetric MODEL has several equivalent answers) to DIR/model/model_from_reconstruction.json.
--symmetries finds the model's rotational symmetries (Utils.find_symmetries; --symmetry-tol T in metres, default 2 % of the diameter) and
writes DIR/model/models_info.json with object id 1 (bop.write_models_info: diameter, bounds and the symmetry keys, in millimetres).
--segment is for a folder WITHOUT mask/, of an object standing on a plane (a turntable): the masks come from the depth maps
(reconstruct.segment_views: the supporting plane, what stands above it, the segment nearest the image centre) and are written to
DIR/mask/NAME.png; whatever touches the object without a depth step is part of its mask."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_amd import mesh_io
from foundationpose_amd.reconstruct import (estimate_view_poses, joint_refine_view_poses, load_reference_views, reconstruct_object, refine_view_poses,
                                            segment_views)


def load_views(args, poses):
  if not args.segment:
    return load_reference_views(args.dir, poses=poses)
  from PIL import Image
  views, info = segment_views(load_reference_views(args.dir, poses=poses, masks=False))
  os.makedirs(os.path.join(args.dir, 'mask'), exist_ok=True)
  for name, m in zip(views['names'], views['masks']):
    Image.fromarray((np.asarray(m) != 0).astype(np.uint8) * 255).save(os.path.join(args.dir, 'mask', name + '.png'))
  for v in info['empty']:
    print(f'view {views["names"][v]}: no segment above the plane, its mask is empty')
  return views


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('dir')
  ap.add_argument('--voxel', type=float, default=0.002)
  ap.add_argument('--trunc', type=float, default=None)
  ap.add_argument('--min-weight', type=float, default=1)
  ap.add_argument('--no-depth-filter', action='store_true')
  ap.add_argument('--refine-poses', action='store_true')
  ap.add_argument('--joint-refine', action='store_true')
  ap.add_argument('--estimate-poses', action='store_true')
  ap.add_argument('--photometric', type=float, nargs='?', const=True, default=False, metavar='WEIGHT')
  ap.add_argument('--max-vertices', type=int, default=None)
  ap.add_argument('--simplify-cell', type=float, default=None)
  ap.add_argument('--min-component-fraction', type=float, default=None)
  ap.add_argument('--texture', type=int, nargs='?', const=0, default=None, metavar='SIZE')
  ap.add_argument('--out', default=None)
  ap.add_argument('--compare-to', default=None, metavar='MODEL')
  ap.add_argument('--align', action='store_true')
  ap.add_argument('--align-to', default=None, metavar='MODEL')
  ap.add_argument('--symmetries', action='store_true')
  ap.add_argument('--symmetry-tol', type=float, default=None)
  ap.add_argument('--segment', action='store_true')
  args = ap.parse_args()
  out = args.out or os.path.join(args.dir, 'model', 'model.obj')
  if args.texture is not None and out.lower().endswith('.ply'):
    ap.error('--texture writes an OBJ with its .mtl and .png: give --out a name ending in .obj')
  if args.align and args.compare_to is None:
    ap.error('--align goes with --compare-to MODEL (--align-to MODEL writes the model in MODEL\'s frame)')
  if args.refine_poses and args.joint_refine:
    ap.error('give --refine-poses or --joint-refine, not both')
  estimate = args.estimate_poses or not os.path.isdir(os.path.join(args.dir, 'cam_in_ob'))
  if args.photometric is not False and (args.refine_poses or not (estimate or args.joint_refine)):
    ap.error('--photometric goes with --joint-refine or --estimate-poses (--refine-poses has no photometric term)')
  if estimate:
    views = load_views(args, poses=False)
    poses, _ = estimate_view_poses(views, depth_filter=not args.no_depth_filter, photometric=args.photometric)
    os.makedirs(os.path.join(args.dir, 'cam_in_ob_estimated'), exist_ok=True)
    for name, pose in zip(views['names'], poses):
      np.savetxt(os.path.join(args.dir, 'cam_in_ob_estimated', name + '.txt'), pose, fmt='%.18e')
    views = dict(views, cam_in_obs=poses)
  else:
    views = load_views(args, poses=True)
  if args.refine_poses or args.joint_refine:
    if args.joint_refine:
      poses, info = joint_refine_view_poses(views, depth_filter=not args.no_depth_filter, photometric=args.photometric)
    else:
      poses, info = refine_view_poses(views, voxel_size=args.voxel, depth_filter=not args.no_depth_filter)
    os.makedirs(os.path.join(args.dir, 'cam_in_ob_refined'), exist_ok=True)
    for name, pose in zip(views['names'], poses):
      np.savetxt(os.path.join(args.dir, 'cam_in_ob_refined', name + '.txt'), pose, fmt='%.18e')
    for v, why in sorted(info['stopped'].items()):
      print(f'view {views["names"][v]}: alignment stopped ({why})')
    views = dict(views, cam_in_obs=poses)
  mesh = reconstruct_object(views, voxel_size=args.voxel, trunc=args.trunc, min_weight=args.min_weight, depth_filter=not args.no_depth_filter,
                            max_vertices=args.max_vertices, simplify_cell=args.simplify_cell,
                            texture=None if args.texture is None else (args.texture or True),
                            components='largest' if args.min_component_fraction is None else dict(keep='all', min_fraction=args.min_component_fraction),
                            align_to=None if args.align_to is None else mesh_io.load_mesh(args.align_to))
  if args.align_to is not None:
    mesh, ainfo = mesh
    T, al = ainfo['model_from_reconstruction'], ainfo['align']
    os.makedirs(os.path.join(args.dir, 'cam_in_ob_aligned'), exist_ok=True)
    for name, pose in zip(views['names'], views['cam_in_obs']):
      np.savetxt(os.path.join(args.dir, 'cam_in_ob_aligned', name + '.txt'), T @ np.asarray(pose, dtype=np.float64), fmt='%.18e')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(os.path.join(os.path.dirname(os.path.abspath(out)), 'model_from_reconstruction.json'), 'w') as fh:
      json.dump(dict(aligned_to=args.align_to, model_from_reconstruction=T.tolist(), chosen=al['chosen'], ambiguous=al['ambiguous'],
                     rms=float(al['rms'][al['chosen']]), ambiguous_transforms=[al['poses'][k].tolist() for k in al['ambiguous']]), fh)
    print(f'aligned to {args.align_to}: rms {al["rms"][al["chosen"]]:.6f}, start {al["chosen"]}' +
          (f'; starts {al["ambiguous"]} fit nearly as well (a symmetric model: the answers are equivalent)' if al['ambiguous'] else ''))
  os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
  if out.lower().endswith('.ply'):
    mesh_io.save_ply(mesh, out)
  else:
    mesh_io.save_obj(mesh, out)
  tex = f', texture {mesh.visual.image.shape[1]} x {mesh.visual.image.shape[0]}' if args.texture is not None else ''
  print(f'{out}: {len(mesh.vertices)} vertices, {len(mesh.faces)} faces{tex}')
  if args.symmetries:
    from foundationpose_amd import Utils as U
    from foundationpose_amd import bop
    info = U.find_symmetries(mesh, tol=args.symmetry_tol)
    models_dir = os.path.join(args.dir, 'model')
    bop.write_models_info(models_dir, {1: mesh}, symmetries={1: info})
    print(f'{os.path.join(models_dir, "models_info.json")}: {len(info["symmetries_discrete"])} discrete symmetries, '
          f'{len(info["symmetries_continuous"])} continuous axes, {len(info["symmetry_tfs"])} transforms (tol {info["tol"]:.3g})')
  if args.compare_to is not None:
    from foundationpose_amd import Utils as U
    res = U.mesh_distance(mesh, mesh_io.load_mesh(args.compare_to), align=args.align)
    if args.align:
      al = res.pop('align_info')
      res.update(a_to_b_transform=res['a_to_b_transform'].tolist(), align_chosen=al['chosen'], align_ambiguous=al['ambiguous'])
    print(json.dumps(dict(compared_to=args.compare_to, **res)))


if __name__ == '__main__':
  main()
