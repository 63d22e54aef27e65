"""Host: the layout of a frame buffer (frame.frame_sections) and the test for an already packed [depth | rgb] frame (frame.is_packed).
Neither needs a device."""
import itertools

import pytest
import torch

from foundationpose_amd.frame import frame_sections, is_packed

H, W = 5, 7                    # an odd pixel count: H * W * 3 is odd, so a mask section behind uint8 colours starts at an odd offset
HW = H * W


@pytest.mark.parametrize('rgb_u8, labels, n_masks', list(itertools.product([True, False], [False, True], [0, 1, 8])))
def test_sections_are_contiguous_ordered_and_aligned(rgb_u8, labels, n_masks):
  sec = frame_sections(H, W, rgb_u8, labels, n_masks)
  want = ['depth'] + (['labels'] if labels else []) + ['rgb'] + (['masks'] if n_masks else [])
  assert list(sec) == want                                     # the stated order; an absent section is not listed
  at = 0
  for name in want:
    assert sec[name][0] == at, name                            # no gap, no overlap
    at += sec[name][1]
  n_rgb = HW * 3 * (1 if rgb_u8 else 4)
  assert sec['depth'] == (0, HW * 4) and sec['rgb'][1] == n_rgb
  assert at == HW * 4 + (HW * 4 if labels else 0) + n_rgb + n_masks * HW      # the buffer's size
  for name in ['depth', 'labels'] + ([] if rgb_u8 else ['rgb']):
    if name in sec:
      assert sec[name][0] % 4 == 0, name                      # float32 / int32 views need it
  if labels:
    assert sec['labels'] == (HW * 4, HW * 4)
  if n_masks:
    assert sec['masks'] == (at - n_masks * HW, n_masks * HW)
    if rgb_u8:
      assert sec['masks'][0] % 2 == 1                          # (the odd offset this frame size was chosen for)


@pytest.mark.parametrize('rgb_u8', [True, False])
def test_tracking_layout_is_depth_then_rgb(rgb_u8):
  sec = frame_sections(H, W, rgb_u8)
  assert list(sec) == ['depth', 'rgb'] and sec['rgb'][0] == HW * 4


def _carve(buf, at_depth, at_rgb, rgb_u8):
  """depth (H,W) float32 and rgb (H,W,3) as views of the byte buffer `buf` at the two byte offsets."""
  n_rgb = HW * 3 * (1 if rgb_u8 else 4)
  depth = buf[at_depth:at_depth + HW * 4].view(torch.float).reshape(H, W)
  rgb = buf[at_rgb:at_rgb + n_rgb]
  return depth, (rgb if rgb_u8 else rgb.view(torch.float)).reshape(H, W, 3)


@pytest.mark.parametrize('rgb_u8', [True, False])
def test_is_packed(rgb_u8):
  n_rgb = HW * 3 * (1 if rgb_u8 else 4)
  buf = torch.zeros(2 * (HW * 4 + n_rgb) + 64, dtype=torch.uint8)
  assert is_packed(*_carve(buf, 0, HW * 4, rgb_u8))
  assert is_packed(*_carve(buf, 8, 8 + HW * 4, rgb_u8))                             # not at the start of the storage
  depth, rgb = _carve(buf, 0, HW * 4, rgb_u8)
  assert not is_packed(depth.clone(), rgb.clone())                                  # two separate tensors
  assert not is_packed(depth, rgb.clone()) and not is_packed(depth.clone(), rgb)
  assert not is_packed(*_carve(buf, 0, HW * 4 + 4, rgb_u8))                         # one buffer, a gap between them
  assert not is_packed(*_carve(buf, (n_rgb + 3) // 4 * 4, 0, rgb_u8))               # one buffer, rgb first
  wide = buf[HW * 4:HW * 4 + 2 * n_rgb]
  wide = (wide if rgb_u8 else wide.view(torch.float)).reshape(H, W, 6)
  assert wide.data_ptr() == rgb.data_ptr() and not is_packed(depth, wide[..., :3])   # the right address, but not contiguous
