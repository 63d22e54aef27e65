"""CPU: what a network pass runs besides its convolutions (foundationpose_amd/csrc/pass_plan.h) - hypotheses per pass, trunk parts, side
chains, shared side B, fused tail, head streams and the kernel forms of in-projections, attention and head MLP - planned by a stand-alone
program that is compiled against the header alone: no HIP, no GPU.

The expected values are written by hand from the rules the launchers and api.hip held before the header existed (three size classes: 1..2,
3..4 and 5 or more hypotheses; trunk in 2 parts from 48 on).  Every knob is shown to move what its comment says and nothing else: the whole
grid below is planned with and without it and the set of changed entries is compared with a hand-written one."""
import os
import re
import subprocess

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CSRC = os.path.join(REPO, 'foundationpose_amd', 'csrc')

PROGRAM = r'''
#include <stdio.h>
#include "pass_plan.h"
int main() {
  char what;
  int a[6], c[11];
  while (scanf(" %c %d %d %d %d %d %d", &what, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) == 7) {
    for (int i = 0; i < 11; ++i)
      if (scanf("%d", &c[i]) != 1) return 1;
    PassKnobs k;
    k.chunk = c[0], k.trunk_min = c[1], k.trunk_streams = c[2], k.one_chain = c[3], k.no_shared_b = c[4], k.tail_split = c[5];
    k.qkv_small = c[6], k.qkv64 = c[7], k.attn_small = c[8], k.headmlp64 = c[9], k.heads_serial = c[10];
    if (what == 'F') {            // kind n
      const ForwardPlan p = forward_plan(a[0], a[1], k);
      printf("%s %s %s streams=%d parts=%d", qkv_form_name(p.qkv), attn_form_name(p.attn), head_mlp_form_name(p.head_mlp), p.head_streams, p.trunk_parts);
      for (int i = 0; i < p.trunk_parts; ++i) {
        const TrunkPart t = trunk_part(p, i);
        printf(" %d+%d:hyp%d:%s", t.start, t.n, t.conv_hyp, t.splitk ? "scratch" : "-");
      }
      printf("\n");
    } else if (what == 'P') {     // kind n_total n_runs n_live flags
      const PassPlan p = pass_plan(a[0], a[1], a[2], a[3], (unsigned)a[4], k);
      printf("chunk=%d fork=%d chains=%d sharedB=%d tail=%d\n", p.chunk, (int)p.fork_sides, (int)p.side_chains, (int)p.shared_b, (int)p.fused_tail);
    } else if (what == 'Q') {     // hyp images
      printf("%s\n", qkv_form_name(qkv_form(a[0], a[1], k)));
    } else if (what == 'M') {     // M
      printf("%s\n", head_mlp_form_name(head_mlp_form(a[0], k)));
    } else if (what == 'A') {     // images
      printf("%s\n", attn_form_name(attn_form(a[0], k)));
    } else if (what == 'T') {     // n n_side_streams
      printf("%d\n", trunk_parts(a[0], k, a[1]));
    } else if (what == 'S') {     // n
      printf("%d %d\n", (int)net_offers_splitk(a[0]), hyp_chunk(a[0], k));
    } else {
      return 1;
    }
  }
  return 0;
}
'''

# PassKnobs in the order the program reads them, with the defaults of the header (= of the code before it)
KNOBS = dict(FP_CHUNK=0, FP_TRUNK_MIN=48, FP_TRUNK_STREAMS=2, FP_ONE_CHAIN=0, FP_NO_SHARED_B=0, FP_TAIL_SPLIT=0, FP_QKV_SMALL=2, FP_QKV64=0, FP_ATTN_SMALL=2,
             FP_HEADMLP64=0, FP_HEADS_SERIAL=0)
REFINE, SCORE = 0, 1
SHARED = 1                     # FP_REFINE_SHARED_TRANSLATION


@pytest.fixture(scope='module')
def planner(tmp_path_factory):
  """The compiler beside the hipcc the Makefile names (ROCm's clang++), on pass_plan.h alone."""
  hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC \?= (\S+)', open(os.path.join(CSRC, 'Makefile')).read(), flags=re.M).group(1)
  cxx = os.path.join(os.path.dirname(hipcc), 'amdclang++')
  d = tmp_path_factory.mktemp('pass_plan')
  src, exe = d / 'plan.cc', d / 'plan'
  src.write_text(PROGRAM)
  subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', CSRC, str(src), '-o', str(exe)], check=True)

  def plan(rows, **knobs):
    """rows of (letter, up to 6 ints) -> one output line each, under the default knobs except those named"""
    assert set(knobs) <= set(KNOBS)
    tail = ' '.join(str(int(v)) for v in {**KNOBS, **knobs}.values())
    text = ''.join(' '.join(str(v) for v in (tuple(r) + (0,) * 6)[:7]) + ' ' + tail + '\n' for r in rows)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split('\n')[:-1]
    assert len(out) == len(rows)
    return out
  return plan


SIZES = (1, 2, 3, 4, 5, 40, 41, 47, 48, 63, 64, 96, 252)
TWO_PARTS = {48: (24, 24), 63: (31, 32), 64: (32, 32), 96: (48, 48), 252: (126, 126)}


def _forward(kind, n):
  """the plan of a forward body of n images under the default knobs, by hand"""
  if n <= 2:
    forms = 'qkv-small attn-small mlp64'
  elif n <= 4:
    forms = 'qkv128 attn-persistent mlp64'
  else:
    forms = 'qkv128 attn-persistent mlp128'
  if kind == SCORE:
    forms = forms.rsplit(' ', 1)[0] + ' none'
  parts, start = [], 0
  for m in TWO_PARTS.get(n, (n,)):
    parts.append(f'{start}+{m}:hyp{m}:' + ('scratch' if m <= 4 else '-'))
    start += m
  return f'{forms} streams={2 if kind == REFINE else 0} parts={len(parts)} ' + ' '.join(parts)


def test_forward_plans_of_the_three_size_classes(planner):
  assert _forward(REFINE, 1) == 'qkv-small attn-small mlp64 streams=2 parts=1 0+1:hyp1:scratch'
  assert _forward(REFINE, 4) == 'qkv128 attn-persistent mlp64 streams=2 parts=1 0+4:hyp4:scratch'
  assert _forward(SCORE, 47) == 'qkv128 attn-persistent none streams=0 parts=1 0+47:hyp47:-'
  assert _forward(REFINE, 63) == 'qkv128 attn-persistent mlp128 streams=2 parts=2 0+31:hyp31:- 31+32:hyp32:-'
  for kind in (REFINE, SCORE):
    got = planner([('F', kind, n) for n in SIZES])
    assert got == [_forward(kind, n) for n in SIZES], kind


def test_trunk_parts_never_exceed_the_streams(planner):
  """min(FP_TRUNK_STREAMS, side streams, max(2, n / 32)) from FP_TRUNK_MIN on, else 1"""
  rows = [('T', n, nside) for n, nside in ((47, 8), (48, 8), (252, 8), (512, 8), (512, 4), (100, 8), (64, 8))]
  assert planner(rows) == ['1', '2', '2', '2', '2', '2', '2']
  assert planner(rows, FP_TRUNK_STREAMS=16) == ['1', '2', '7', '8', '4', '3', '2']
  assert planner(rows, FP_TRUNK_STREAMS=1) == ['1'] * 7
  assert planner([('S', n) for n in (1, 4, 5, 252)]) == ['1 1', '1 4', '0 5', '0 252']


PASS_GRID = [(REFINE, n, runs, live, flags) for n in (1, 5, 40, 47, 48, 252) for runs in (1, 2) for live in (1, 8, 9) for flags in (0, SHARED)] + \
            [(SCORE, n, runs, 1, 0) for n in (1, 40, 47, 48, 252) for runs in (1, 2)]


def _pass(kind, n, runs, live, flags):
  """by hand: side chains need one run and n < 48; shared B one run, at most 8 live objects (RefineNet, flag set); the fused tail one run (RefineNet)"""
  chains = runs == 1 and n < 48
  shared = kind == REFINE and runs == 1 and live <= 8 and flags == SHARED
  tail = kind == REFINE and runs == 1
  return f'chunk={n} fork={int(chains)} chains={int(chains)} sharedB={int(shared)} tail={int(tail)}'


def test_pass_plans_match_the_rule(planner):
  assert _pass(REFINE, 47, 1, 8, SHARED) == 'chunk=47 fork=1 chains=1 sharedB=1 tail=1'
  assert _pass(REFINE, 48, 1, 9, SHARED) == 'chunk=48 fork=0 chains=0 sharedB=0 tail=1'
  assert _pass(REFINE, 40, 2, 1, SHARED) == 'chunk=40 fork=0 chains=0 sharedB=0 tail=0'
  assert _pass(SCORE, 1, 1, 1, 0) == 'chunk=1 fork=1 chains=1 sharedB=0 tail=0'
  got = planner([('P',) + r for r in PASS_GRID])
  assert got == [_pass(*r) for r in PASS_GRID]


def test_stand_alone_calls(planner):
  """qkv_form(hyp = 0): the 128-token kernel at any size; head_mlp_form switches between M = 1600 and 1616; attn_form between 2 and 3 images"""
  assert planner([('Q', 0, n) for n in (1, 2, 3, 252)]) == ['qkv128'] * 4
  assert planner([('Q', 0, n) for n in (1, 2, 3, 252)], FP_QKV64=1) == ['qkv128'] * 4
  assert planner([('Q', 1, 1)]) == ['qkv-small']
  assert planner([('M', 16), ('M', 1600), ('M', 1616), ('M', 100800)]) == ['mlp64', 'mlp64', 'mlp128', 'mlp128']
  assert planner([('A', 1), ('A', 2), ('A', 3), ('A', 252)]) == ['attn-small', 'attn-small', 'attn-persistent', 'attn-persistent']


# the grid every knob is held to: forward plans, pass plans, stand-alone predicates
GRID = [('F', kind, n) for kind in (REFINE, SCORE) for n in SIZES + (8,)] + [('P',) + r for r in PASS_GRID] + \
       [('Q', 0, 1), ('Q', 0, 100), ('Q', 1, 1), ('M', 1600), ('M', 1616), ('A', 2), ('A', 3)]


def _moved(planner, **knobs):
  base, got = planner(GRID), planner(GRID, **knobs)
  return {row: g for row, b, g in zip(GRID, base, got) if b != g}


def _sub(line, **fields):
  """`line` with the named key=value fields replaced"""
  for k, v in fields.items():
    line, n = re.subn(rf'\b{k}=\d+', f'{k}={v}', line)
    assert n == 1
  return line


def test_trunk_knobs(planner):
  # FP_TRUNK_STREAMS=1: one part at every size, and so two side chains at every size of one run
  want = {('F', kind, n): _forward(kind, n).split(' parts=')[0] + f' parts=1 0+{n}:hyp{n}:-' for kind in (REFINE, SCORE) for n in TWO_PARTS}
  want.update({('P',) + r: _sub(_pass(*r), fork=1, chains=1) for r in PASS_GRID if r[1] >= 48 and r[2] == 1})
  assert _moved(planner, FP_TRUNK_STREAMS=1) == want
  # FP_TRUNK_MIN=8: two parts from 8 hypotheses on - parts of four are offered scratch - and no side chains there
  halves = {8: (4, 4), 40: (20, 20), 41: (20, 21), 47: (23, 24)}
  want = {}
  for kind in (REFINE, SCORE):
    for n, (a, b) in halves.items():
      sk = 'scratch' if n == 8 else '-'
      want[('F', kind, n)] = _forward(kind, n).split(' parts=')[0] + f' parts=2 0+{a}:hyp{a}:{sk} {a}+{b}:hyp{b}:{sk}'
  want.update({('P',) + r: _sub(_pass(*r), fork=0, chains=0) for r in PASS_GRID if r[1] in (40, 47) and r[2] == 1})
  assert _moved(planner, FP_TRUNK_MIN=8) == want


def test_chain_and_stream_knobs(planner):
  want = {('P',) + r: _sub(_pass(*r), fork=0, chains=0) for r in PASS_GRID if r[1] < 48 and r[2] == 1}
  assert _moved(planner, FP_ONE_CHAIN=1) == want
  want = {('F', REFINE, n): _forward(REFINE, n).replace('streams=2', 'streams=1') for n in SIZES + (8,)}
  assert _moved(planner, FP_HEADS_SERIAL=1) == want
  want = {('P',) + r: _sub(_pass(*r), sharedB=0) for r in PASS_GRID if ' sharedB=1' in _pass(*r)}
  assert len(want) == 12 and _moved(planner, FP_NO_SHARED_B=1) == want
  want = {('P',) + r: _sub(_pass(*r), tail=0) for r in PASS_GRID if ' tail=1' in _pass(*r)}
  assert len(want) == 36 and _moved(planner, FP_TAIL_SPLIT=1) == want


def test_kernel_form_knobs(planner):
  # FP_QKV64: the 64-token pair above FP_QKV_SMALL only; never for a stand-alone call
  want = {('F', kind, n): _forward(kind, n).replace('qkv128', 'qkv64-pair') for kind in (REFINE, SCORE) for n in SIZES + (8,) if n > 2}
  assert _moved(planner, FP_QKV64=1) == want
  want = {('F', kind, n): _forward(kind, n).replace('qkv-small', 'qkv128') for kind in (REFINE, SCORE) for n in (1, 2)}
  want[('Q', 1, 1)] = 'qkv128'
  assert _moved(planner, FP_QKV_SMALL=0) == want
  want = {('F', kind, n): _forward(kind, n).replace('attn-small', 'attn-persistent') for kind in (REFINE, SCORE) for n in (1, 2)}
  want[('A', 2)] = 'attn-persistent'
  assert _moved(planner, FP_ATTN_SMALL=0) == want
  want = {('F', REFINE, n): _forward(REFINE, n).replace('mlp128', 'mlp64') for n in SIZES + (8,) if n > 4}
  want[('M', 1616)] = 'mlp64'
  assert _moved(planner, FP_HEADMLP64=1) == want


def test_chunk_knob(planner):
  """FP_CHUNK=2: passes of more than two hypotheses run in chunks - one chain through encodeA (the observed side's input is still produced on
  its own stream), no shared B, no fused tail; a forward body is planned by its own images, so nothing else moves"""
  want = {('P',) + r: _sub(_pass(*r), chunk=2, chains=0, sharedB=0, tail=0) for r in PASS_GRID if r[1] > 2}
  assert _moved(planner, FP_CHUNK=2) == want
  # five hypotheses: chunks of 2, 2, 1, each a few-image body
  assert planner([('P', REFINE, 5, 1, 1, SHARED)], FP_CHUNK=2) == ['chunk=2 fork=1 chains=0 sharedB=0 tail=0']
  chunks = [min(2, 5 - s0) for s0 in range(0, 5, 2)]
  assert chunks == [2, 2, 1]
  assert planner([('F', REFINE, n) for n in chunks], FP_CHUNK=2) == ['qkv-small attn-small mlp64 streams=2 parts=1 0+2:hyp2:scratch'] * 2 + \
      ['qkv-small attn-small mlp64 streams=2 parts=1 0+1:hyp1:scratch']
  # a chunk above the pass, zero or a negative value: the whole batch
  for v in (0, -1, 6, 5):
    assert planner([('P', REFINE, 5, 1, 1, 0)], FP_CHUNK=v) == ['chunk=5 fork=1 chains=1 sharedB=0 tail=1']
