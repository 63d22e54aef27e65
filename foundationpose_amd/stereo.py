"""Depth from a rectified stereo pair: semi-global matching on census costs (csrc/stereo.hip; the rule is stated in
include/foundationpose_amd.h and restated in numpy by tests/stereo_oracle.py).

    disparity = stereo_disparity(left, right)                    # float32 pixels, -1 where no match is accepted
    depth = stereo_depth(left, right, K, baseline)               # float32 metres, 0 where there is none: what register / track_one take

The reference reads a depth image that its camera vendor's SDK computed (src/file_processing.py:99-138); this is the library's own rule
in that place, integer up to the winning disparity and therefore the same on every run and in any batch.  **The pair must already be
rectified and undistorted - rectify.rectify_pair does that for a raw pair with a calibration, stereo_depth(..., rectify=rect) in one
chain; textureless and specular surfaces are not matched; the band x < d has no partner; one disparity step is z^2 / (fx b) of depth;
P2 is constant.**
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr


def _pair_on(left, right, device):
  """(device, left, right as contiguous uint8 device tensors (n,H,W) or (n,H,W,3), channels, batch, on_device).  (H,W) is one grey
  image, (H,W,3) one RGB image, (n,H,W) with W != 3 a grey batch, (n,H,W,3) an RGB batch."""
  on_device = torch.is_tensor(left) and left.is_cuda
  dev = left.device if on_device else torch.device(device)
  out = []
  for name, img in (('left', left), ('right', right)):
    t = torch.as_tensor(img)
    if t.dtype != torch.uint8:
      raise ValueError(f'{name} must be uint8, got {t.dtype}')
    out.append(t.to(dev).contiguous())
  l, r = out
  if l.shape != r.shape:
    raise ValueError(f'left {tuple(l.shape)} and right {tuple(r.shape)} differ in shape')
  if l.dim() == 2:
    channels, batch = 1, False
  elif l.dim() == 3 and l.shape[2] == 3:
    channels, batch = 3, False
  elif l.dim() == 3:
    channels, batch = 1, True
  elif l.dim() == 4 and l.shape[3] == 3:
    channels, batch = 3, True
  else:
    raise ValueError(f'images must be (H,W), (H,W,3), (n,H,W) or (n,H,W,3), got {tuple(l.shape)}')
  if not batch:
    l, r = l[None], r[None]
  return dev, l, r, channels, batch, on_device


def sgm(left, right, max_disparity=128, p1=8, p2=32, paths=0xFF, lr_max=1, min_disparity=1, subpixel=True, fx=None, baseline=None, zfar=np.inf,
        want_disparity=True, return_debug=False, device='cuda'):
  """One fp_stereo_sgm call on images as stereo_disparity takes them: (disparity or None, depth or None, stages or None) as device tensors
  with the leading n.  depth is made when fx and baseline are given.  Queues on the current stream; does not synchronise."""
  dev, l, r, channels, _, _ = _pair_on(left, right, device)
  return _sgm(dev, l, r, channels, max_disparity, p1, p2, paths, lr_max, min_disparity, subpixel, fx, baseline, zfar, want_disparity, return_debug)


def _sgm(dev, l, r, channels, max_disparity=128, p1=8, p2=32, paths=0xFF, lr_max=1, min_disparity=1, subpixel=True, fx=None, baseline=None,
         zfar=np.inf, want_disparity=True, return_debug=False):
  n, H, W = l.shape[:3]
  D = int(max_disparity)
  o = _lib.FpStereoOpts(struct_size=ctypes.sizeof(_lib.FpStereoOpts), max_disparity=D, p1=int(p1), p2=int(p2), paths=int(paths) & 0xFFFFFFFF,
                        lr_max=int(lr_max), min_disparity=int(min_disparity), subpixel=int(bool(subpixel)),
                        fx=0.0 if fx is None else float(fx), baseline=0.0 if baseline is None else float(baseline), zfar=float(zfar))
  want_depth = fx is not None and baseline is not None
  disparity = torch.empty((n, H, W), dtype=torch.float32, device=dev) if want_disparity else None
  depth = torch.empty((n, H, W), dtype=torch.float32, device=dev) if want_depth else None
  dbg, stages = None, None
  if return_debug:
    if not (1 <= D <= _lib.FP_STEREO_MAX_DISPARITY):      # the library refuses it below; do not size an allocation by it
      raise ValueError(f'max_disparity must be a multiple of 64 in 64 .. {_lib.FP_STEREO_MAX_DISPARITY}, got {D}')
    stages = dict(census_left=torch.empty((n, H, W), dtype=torch.int64, device=dev), census_right=torch.empty((n, H, W), dtype=torch.int64, device=dev),
                  cost=torch.empty((n, H, W, D), dtype=torch.uint8, device=dev), sum=torch.empty((n, H, W, D), dtype=torch.int16, device=dev),
                  dstar=torch.empty((n, H, W), dtype=torch.int32, device=dev), dright=torch.empty((n, H, W), dtype=torch.int32, device=dev))
    dbg = _lib.FpStereoDebug(struct_size=ctypes.sizeof(_lib.FpStereoDebug), **{'d_' + k: v.data_ptr() for k, v in stages.items()})
  check(lib().fp_stereo_sgm(_lib.Context.get(dev).handle, ptr(l), ptr(r), n, H, W, channels, ctypes.byref(o), ptr(disparity), ptr(depth),
                            ctypes.byref(dbg) if dbg is not None else None, stream_ptr(dev)))
  return disparity, depth, stages


def _debug_numpy(stages):
  """The stages as numpy with their own types: the census codes uint64, S uint16 (torch has no such device types)."""
  out = {k: v.cpu().numpy() for k, v in stages.items()}
  out['census_left'], out['census_right'] = out['census_left'].view(np.uint64), out['census_right'].view(np.uint64)
  out['sum'] = out['sum'].view(np.uint16)
  return out


def _finish(x, batch, on_device):
  x = x if batch else x[0]
  return x if on_device else x.cpu().numpy()


def stereo_disparity(left, right, max_disparity=128, p1=8, p2=32, paths=0xFF, lr_max=1, min_disparity=1, subpixel=True, return_debug=False,
                     device='cuda'):
  """Disparity of a rectified pair, float32 pixels, -1 where no match is accepted: left pixel (y, x) shows what right pixel
  (y, x - disparity) shows.  left, right: uint8 (H,W) grey or (H,W,3) RGB, or a batch (n,H,W) / (n,H,W,3) of pairs of one size; numpy
  arrays give numpy, device tensors give a device tensor without a host copy (and without a synchronisation).  max_disparity: a multiple
  of 64 in 64 .. 256, the disparities 0 .. max_disparity - 1 are searched.  p1 <= p2: the constant penalties of a disparity step of one
  and of a jump; paths: one bit per direction (0xFF all eight, 0x0F the four axis-aligned ones: about half the time, more streaks);
  lr_max: the largest difference the left-right check accepts (negative: no check); min_disparity: smaller winners are invalid;
  subpixel: the parabola through the three sums around the winner.  return_debug: (disparity, stages) with the stages as numpy arrays of
  the leading n - census_left, census_right (uint64), cost (uint8), sum (uint16), dstar, dright (int32); this synchronises.
  **Rectified, undistorted input only (rectify.rectify_pair makes one from a raw pair); textureless and specular surfaces are not
  matched; the band x < d has no partner.**"""
  dev, l, r, channels, batch, on_device = _pair_on(left, right, device)
  disparity, _, stages = _sgm(dev, l, r, channels, max_disparity, p1, p2, paths, lr_max, min_disparity, subpixel, return_debug=return_debug)
  out = _finish(disparity, batch, on_device)
  return (out, _debug_numpy(stages)) if return_debug else out


def stereo_depth(left, right, K=None, baseline=None, zfar=np.inf, *, rectify=None, **kw):
  """Metric depth of a rectified pair: float32 metres, (H,W) or (n,H,W), 0 where there is none (no accepted match, or farther than
  zfar) - the depth image register, track_one, depth_prefilter and segment_on_plane take.  K: the 3x3 matrix of the (rectified) left
  camera, of which fx is used; baseline: the distance of the two cameras in metres; depth = (float)(fx baseline) / disparity.  **One
  disparity step is z^2 / (fx baseline) of depth: the error grows with the square of the distance.**  The other arguments are those of
  stereo_disparity (return_debug gives (depth, stages)).  Numpy in gives numpy out, device tensors give a device tensor without a host copy.
  rectify: a rectify.StereoRectification (rectify_stereo) for a RAW pair - both images are first warped into its rectified cameras
  (one fp_remap launch in front of the matching, on the same stream) and K, baseline default to rectify.K_new, rectify.baseline; the
  depth then belongs to the rectified left camera rectify.K_new, size rectify.size_new.  Without it the pair must already be rectified
  and undistorted, and K and baseline are required."""
  return_debug = bool(kw.pop('return_debug', False))
  device = kw.pop('device', 'cuda')
  if rectify is not None:
    K = rectify.K_new if K is None else K
    baseline = rectify.baseline if baseline is None else baseline
  if K is None or baseline is None:
    raise ValueError('stereo_depth: K and baseline are required (or rectify=...)')
  Kh = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float64).reshape(3, 3)
  dev, l, r, channels, batch, on_device = _pair_on(left, right, device)
  if rectify is not None:
    from .rectify import remap
    (l, r), _, _ = remap([l, r], [rectify.left, rectify.right], 'colour')
  _, depth, stages = _sgm(dev, l, r, channels, fx=float(Kh[0, 0]), baseline=float(baseline), zfar=zfar, want_disparity=False, return_debug=return_debug, **kw)
  out = _finish(depth, batch, on_device)
  return (out, _debug_numpy(stages)) if return_debug else out
