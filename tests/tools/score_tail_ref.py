"""Float64 references of the ScoreNet tail (att_cross + linear, csrc/score_tail.hip) and the inputs of its tests.  Plain torch / numpy,
no GPU: tests/test_score_tail_host.py checks the references and the inputs here, tests/test_gpu_score_tail.py the kernels against them.

  tail_reference   oracle.nets.score_tail on float64 inputs: in_proj, 4-head softmax attention, out_proj, Linear - the textbook form
  tail_emulation   the kernel's arithmetic with its ONE storage rounding: q and k rows summed in float64 and rounded once to float32;
                   the value path folded as net.hip:make_score_tail folds it (w_eff = W_o^T lin.w, b_eff = lin.w . b_o + lin.b,
                   u_h = Wv_h^T w_eff^h, c_h = bv_h . w_eff^h, all float64; derivation in the header of score_tail.hip);
                   a plain float64 softmax.  What is left between this and the kernel is the order of float64 sums and the final
                   rounding of the logit to float32.

Both return (logits (groups, L), softmax (groups, 4, L, L)) as float64 numpy arrays."""
import functools
import math

import numpy as np
import torch

from foundationpose_amd import synthetic as S
from oracle import nets

N_HEAD, D_HEAD, D_MODEL = 4, 128, 512
TAIL_KEYS = ('att_cross.in_proj_weight', 'att_cross.in_proj_bias', 'att_cross.out_proj.weight', 'att_cross.out_proj.bias',
             'linear.weight', 'linear.bias')


def _sd64(sd):
  return {k: sd[k].double() for k in TAIL_KEYS}


def _rows64(feats):
  feats = feats.detach().cpu().numpy() if torch.is_tensor(feats) else feats
  return torch.from_numpy(np.array(feats, dtype=np.float64).reshape(-1, D_MODEL))


def _softmax_of(q, k, groups, L):
  """(groups*L, 512) q, k -> (groups, 4, L, L) float64 softmax over the keys of the query's own group."""
  q = q.reshape(groups, L, N_HEAD, D_HEAD).transpose(1, 2)
  k = k.reshape(groups, L, N_HEAD, D_HEAD).transpose(1, 2)
  return torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(D_HEAD), dim=-1)


@torch.no_grad()
def tail_reference(sd, feats, L):
  sd, x = _sd64(sd), _rows64(feats)
  groups = len(x) // L
  logits = nets.score_tail(sd, x, L)
  qk = x @ sd['att_cross.in_proj_weight'][:2 * D_MODEL].T + sd['att_cross.in_proj_bias'][:2 * D_MODEL]
  p = _softmax_of(qk[:, :D_MODEL], qk[:, D_MODEL:], groups, L)
  return logits.numpy(), p.numpy()


@torch.no_grad()
def tail_emulation(sd, feats, L, round_qk=True):
  sd, x = _sd64(sd), _rows64(feats)
  groups = len(x) // L
  wi, bi = sd['att_cross.in_proj_weight'], sd['att_cross.in_proj_bias']
  lw = sd['linear.weight'].reshape(-1)
  qk = x @ wi[:2 * D_MODEL].T + bi[:2 * D_MODEL]
  if round_qk:
    qk = qk.float().double()                                                  # the kernel's qk buffer is float32
  p = _softmax_of(qk[:, :D_MODEL], qk[:, D_MODEL:], groups, L)
  w_eff = sd['att_cross.out_proj.weight'].T @ lw                              # (512)
  b_eff = lw @ sd['att_cross.out_proj.bias'] + sd['linear.bias'][0]
  wv, bv = wi[2 * D_MODEL:].reshape(N_HEAD, D_HEAD, D_MODEL), bi[2 * D_MODEL:].reshape(N_HEAD, D_HEAD)
  we = w_eff.reshape(N_HEAD, D_HEAD)
  u = torch.einsum('hd,hdk->hk', we, wv)                                      # u_h = Wv_h^T w_eff^h
  c = (we * bv).sum(-1)                                                       # c_h = bv_h . w_eff^h
  s = (x @ u.T + c).reshape(groups, L, N_HEAD).permute(0, 2, 1)               # s_j^h, (groups, 4, L)
  logits = (p @ s.unsqueeze(-1)).squeeze(-1).sum(1) + b_eff
  return logits.numpy(), p.numpy()


# ------------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_score_tail.py (and of Check B of tests/test_score_tail_host.py)

SHAPES = ((1, 1), (1, 2), (3, 3), (1, 4), (3, 5), (7, 3),      # M = 9, 15, 21: the last 4-row block of cross_qk_kernel is ragged
          (2, 63), (1, 64), (3, 65),                            # the first lane with two keys
          (1, 127), (1, 252),
          (1, 256), (3, 257),                                   # the first second pass of the key loop, 63 lanes without a key in it
          (2, 320), (1, 513),
          (4096, 2))                                            # every arrival counter in use
REGIMES = ('soft', 'onehot', 'offset')
CASES = tuple((g, L, r) for g, L in SHAPES for r in REGIMES)
TAILS = (None, 5003)                  # tail_seed of make_score_state_dict(1): the fixtures' own, and one nobody tuned
# (tail_seed, regime) -> feature scale where that tail misses a softmax window at the default scale (the windows never move)
SCALE_FOR_TAIL = {}
# (groups, L, regime) -> added to the seed of a case whose reference margins left fewer than 90 % of its groups decidable
RESEED = {}


@functools.lru_cache(maxsize=None)
def tail_sd(tail_seed=None):
  return S.make_score_state_dict(1, tail_seed=tail_seed, tail_only=True)


def regime_scale_offset(regime, L, tail_seed=None):
  scale, offset = {'soft': (0.10 if L <= 8 else 0.12, 0.0), 'onehot': (1.0, 0.0), 'offset': (0.05, 0.2)}[regime]
  return SCALE_FOR_TAIL.get((tail_seed, regime), scale), offset


def make_feats(groups, L, regime, tail_seed=None):
  """(groups*L, 512) float32 features: randn * scale + offset, seeded from (groups, L, regime)."""
  scale, offset = regime_scale_offset(regime, L, tail_seed)
  seed = (groups * 1000003 + L * 101 + REGIMES.index(regime) + RESEED.get((groups, L, regime), 0)) % (1 << 32)
  rs = np.random.RandomState(seed)
  return (rs.randn(groups * L, D_MODEL) * scale + offset).astype(np.float32)


def f32_ulp_at(x):
  """One float32 ulp at |x| (the spacing of float32 there)."""
  return float(np.spacing(np.float32(abs(float(x)))))


@functools.lru_cache(maxsize=None)
def case_refs(groups, L, regime, tail_seed=None):
  """Everything the tests need of one case, computed once: features, both references, the bounds that follow from them."""
  feats = make_feats(groups, L, regime, tail_seed)
  sd = tail_sd(tail_seed)
  ref, p = tail_reference(sd, feats, L)
  emu, _ = tail_emulation(sd, feats, L)
  ulp = f32_ulp_at(np.abs(emu).max())
  if L > 1:
    top = np.sort(ref, axis=-1)
    margin = top[:, -1] - top[:, -2]
  else:
    margin = np.full(groups, np.inf)
  for a in (feats, ref, emu, margin):
    a.setflags(write=False)
  return dict(feats=feats, ref=ref, emu=emu, pmax=p.max(-1), ulp=ulp, d=float(np.abs(emu - ref).max()), margin=margin,
              decided=margin > 4 * ulp, std=ref.std(-1))


def differential(x):
  x = np.asarray(x, dtype=np.float64)
  return x - x.mean(-1, keepdims=True)
