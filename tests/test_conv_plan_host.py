"""CPU: which kernel form a convolution launch runs (foundationpose_amd/csrc/conv_plan.h), planned by a stand-alone program that is compiled
against the header alone - no HIP, no GPU - for the 256 CUs of an MI355X and the default knobs.

The oracle is the `form` column of tests/tools/conv_ref.py (EXACT_CASES, NUM_CASES), written by hand before the plan existed: every case of
tests/test_gpu_conv_numerics.py is thereby shown to reach the kernel it names.  The named cases below state what the network passes take,
where they differ from a stand-alone call, and what the knobs FP_SMALL and FP_C128_BAND move."""
import os
import re
import subprocess

import pytest

from tests.tools import conv_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CSRC = os.path.join(REPO, 'foundationpose_amd', 'csrc')

SMALL, S2, S1B, SPLITK, FORCE_S1B = 1, 2, 4, 8, 16        # ConvOffer
STANDALONE = SMALL | S2 | SPLITK                         # what fp_conv2d_f16 offers for an fp16 output (nothing for fp32)
NET = -1                                                 # the network's offer: the layer's conv_packings, scratch up to CONV_NET_SPLITK_MAX_HYP hypotheses

PROGRAM = r'''
#include <stdio.h>
#include "conv_plan.h"
int main() {
  static const f16 some_residual = 0;
  int N, H, W, Cin, Cout, k, stride, out_mode, res, hyp, offer, small, band;
  while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d", &N, &H, &W, &Cin, &Cout, &k, &stride, &out_mode, &res, &hyp, &offer, &small, &band) == 13) {
    const int Kpad = conv_kpad(k, k, Cin);
    ConvArgs a = conv_args(nullptr, N, H, W, Cin, nullptr, nullptr, Cout, k, k, stride, (k - 1) / 2, Kpad, nullptr);
    a.out_mode = out_mode, a.hyp = hyp;
    if (res) a.res = &some_residual;
    const unsigned packings = conv_packings(Cin, Cout, k, stride, Kpad);
    const unsigned o = offer >= 0 ? (unsigned)offer : packings | (hyp <= CONV_NET_SPLITK_MAX_HYP ? CONV_OFFER_SPLITK : 0u);
    ConvKnobs knobs;
    knobs.small = small, knobs.c128_band = band;
    const ConvPlan p = conv_plan(a, 256, o, knobs);
    printf("%s %d %u\n", conv_form_name(p, a), p.ksplit, packings);
  }
  return 0;
}
'''


@pytest.fixture(scope='module')
def planner(tmp_path_factory):
  """The compiler beside the hipcc the Makefile names (ROCm's clang++), on conv_plan.h alone."""
  hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC \?= (\S+)', open(os.path.join(CSRC, 'Makefile')).read(), flags=re.M).group(1)
  cxx = os.path.join(os.path.dirname(hipcc), 'amdclang++')
  d = tmp_path_factory.mktemp('conv_plan')
  src, exe = d / 'plan.cc', d / 'plan'
  src.write_text(PROGRAM)
  subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', CSRC, str(src), '-o', str(exe)], check=True)

  def plan(rows):
    """rows of (N, H, W, Cin, Cout, k, stride, out_f32, residual, hyp, offer[, FP_SMALL, FP_C128_BAND]) -> [(form, ksplit, packings)]"""
    text = ''.join(' '.join(str(int(v)) for v in (tuple(r) + (1, 1))[:13]) + '\n' for r in rows)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split('\n')[:-1]
    assert len(out) == len(rows)
    return [(f, int(k), int(p)) for f, k, p in (l.split() for l in out)]
  return plan


def _igemm2(c):
  return f'igemm2<{128 if c.Cout % 128 == 0 else 64},{c.k}' + (',CIN8>' if c.Cin < 8 else '>')


def _row(c, out_f32, res, offer):
  return (c.N, c.H, c.W, R.cin_pad(c), c.Cout, c.k, c.stride, out_f32, res, 0, offer)


def _table():
  """(id, row, expected form) of every case x output type x with / without a residual, as tests/test_gpu_conv_numerics.py runs them"""
  t = []
  for c in dict.fromkeys(R.EXACT_CASES + R.NUM_CASES):
    for out_f32 in c.outs:
      for res in (0, 1):
        if c.entry == 'band':
          offer, want = FORCE_S1B, c.form
        elif out_f32:
          offer, want = 0, _igemm2(c)                         # fp32 output: the generic kernel of the shape, whatever form the fp16 output names
          if c.form.startswith('fp32-') or c.form.startswith('igemm2'):
            assert c.form in (want, 'fp32-' + want), R.case_id(c)
        else:
          # a form that adds no residual itself (s2, stem) hands the launch to the generic kernel when there is one
          offer, want = STANDALONE, c.form if (c.takes_res or not res) else _igemm2(c)
        t.append((f'{R.case_id(c)}-out{out_f32}-res{res}', _row(c, out_f32, res, offer), want))
  return t


def test_every_case_of_conv_ref_runs_the_form_it_names(planner):
  table = _table()
  assert len(table) >= 2 * (len(R.EXACT_CASES) + 1)
  got = planner([row for _, row, _ in table])
  wrong = [f'{i}: plan {g[0]}, table {want}' for (i, _, want), g in zip(table, got) if g[0] != want]
  assert not wrong, '\n'.join(wrong)
  assert {'fp32-igemm2<128,3>'} <= {c.form for c in R.NUM_CASES}      # the fp32 entry of NUM_CASES is among them


# the 3x3 layers of the trunks: (input map, Cin, Cout, stride)
SMALL_LAYERS = ((40, 128, 128, 1), (40, 256, 256, 1), (20, 512, 512, 1), (40, 256, 512, 2), (80, 64, 128, 2))
SMALL_NAMES = ('small<1,40,1>', 'small<2,40,1>', 'small<4,20,1>', 'small<2,40,2>', 'small<1,80,2,4>')


def _net(n_img, layer, hyp, **kw):
  hw, cin, cout, stride = layer
  return (n_img, hw, hw, cin, cout, 3, stride, 0, kw.get('res', 0), hyp, kw.get('offer', NET), kw.get('small', 1), kw.get('band', 1))


def test_network_passes_of_one_and_two_hypotheses_take_the_small_form(planner):
  """by the hypotheses of the pass, whatever the launch's image count (one side of encodeA, both, the shared crops of several objects)"""
  rows = [_net(n, l, hyp) for hyp in (1, 2) for l in SMALL_LAYERS for n in (1, 2, 4, 8)]
  assert [g[0] for g in planner(rows)] == [name for _ in (1, 2) for name in SMALL_NAMES for _ in range(4)]


def test_network_passes_of_three_and_four_hypotheses_split_k(planner):
  """the 512-channel stride-1 layers on 20x20 maps (4 shares) and the long-K stride-2 layer.  The 256-channel layers on 40x40 maps do NOT: three
  images are 38 x 2 quarter tiles, and 4 x 76 > 256 CUs (conv_halo_ksplit), so they run the one-launch kernel's 128-pixel tiles - they split at
  one and two hypotheses with FP_SMALL=0 only.  The 128-channel layers have too few chunks to split at any size."""
  for hyp in (3, 4):
    got = planner([_net(hyp, SMALL_LAYERS[2], hyp), _net(hyp, SMALL_LAYERS[3], hyp), _net(hyp, SMALL_LAYERS[1], hyp), _net(2 * hyp, SMALL_LAYERS[0], hyp)])
    assert [g[:2] for g in got] == [('halo-splitk', 4), ('s2-splitk', 4), ('halo-tail1', 0), ('halo-tail1', 0)], (hyp, got)
  got = planner([_net(2, SMALL_LAYERS[1], 2, small=0), _net(1, SMALL_LAYERS[1], 1, small=0)])
  assert [g[:2] for g in got] == [('halo-splitk', 4), ('halo-splitk', 4)], got


def test_network_pass_of_five_hypotheses_splits_nowhere(planner):
  """the networks offer scratch up to four hypotheses; the stand-alone call at the same sizes still splits the 20x20 512 -> 512 layer"""
  rows = [_net(n, l, 5) for l in SMALL_LAYERS for n in (5, 10)]
  got = planner(rows)
  assert all('splitk' not in g[0] and 'small' not in g[0] and g[1] == 0 for g in got), got
  assert planner([_net(5, SMALL_LAYERS[2], 0, offer=STANDALONE)])[0][:2] == ('halo-splitk', 4)


def test_s1b_starts_above_512_pixels_per_cu(planner):
  """The 128 -> 128 layers with the network's offer (s1b packing): the boundary is M > 512 x 256 = 131 072 pixels.  81 images of 40x40 are
  129 600 pixels and stay on the halo kernel (less than a round: tiles of 512 pixels), 82 are 131 200 and take the band form - the first batch at which the general kernel needs
  more than one round of its 512-pixel tiles (launch_conv has always put it there: `M > num_cu * 512`), and so does 83."""
  got = planner([_net(81, SMALL_LAYERS[0], 41), _net(82, SMALL_LAYERS[0], 41), _net(83, SMALL_LAYERS[0], 42)])
  assert [g[0] for g in got] == ['halo-tail4', 's1b', 's1b'], got


def test_knobs_move_the_cases_they_are_said_to(planner):
  # FP_SMALL=0 (tests/test_gpu_kernels.py: the one-hypothesis shapes fall back to the split-K forms)
  got = planner([_net(1, SMALL_LAYERS[2], 0, offer=STANDALONE, res=1, small=0), _net(1, SMALL_LAYERS[1], 0, offer=STANDALONE, small=0),
                 _net(1, SMALL_LAYERS[3], 0, offer=STANDALONE, small=0)])
  assert [g[:2] for g in got] == [('halo-splitk', 8), ('halo-splitk', 4), ('s2-splitk', 4)], got
  # FP_C128_BAND=0 (tests/test_gpu_pipeline.py): the 128 -> 128 layers on the general 3x3 kernel; 2: the 256 -> 256 layers on the band form too
  got = planner([_net(200, SMALL_LAYERS[0], 100, band=0), _net(200, SMALL_LAYERS[0], 100), _net(100, SMALL_LAYERS[1], 100), _net(100, SMALL_LAYERS[1], 100, band=2)])
  assert [g[0] for g in got] == ['halo-round', 's1b', 'halo-round', 's1b'], got


def test_trunk_layers_get_the_packed_copies_they_always_got(planner):
  """conv_packings: the stem none; every 3x3 layer the small copy; the stride-2 layers the s2 copy; the 128 -> 128 and 256 -> 256 layers
  the s1b copy; the 512 -> 512 layers (20x20 maps) no band copy"""
  layers = [(160, 8, 64, 7, 2)] + [(hw, ci, co, 3, s) for hw, ci, co, s in SMALL_LAYERS]
  got = planner([(1, hw, hw, ci, co, k, s, 0, 0, 1, NET) for hw, ci, co, k, s in layers])
  assert [g[2] for g in got] == [0, SMALL | S1B, SMALL | S1B, SMALL, SMALL | S2, SMALL | S2]
