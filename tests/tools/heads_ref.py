"""Float64 references of the transformer heads' kernels - the attention core (csrc/attn.hip), the LayerNorm epilogues of the token Linear
(csrc/tok_gemm.hip, epilogues 2 and 3) and the fused head MLP (csrc/head_mlp.hip) - and the inputs of their tests.  Plain torch / numpy, no
GPU: tests/test_heads_ref_host.py checks the references and the inputs here, tests/test_gpu_heads_numerics.py the kernels against them.
Every reference reads the SAME fp16-rounded operands the kernel reads, so operand rounding is not an error source on either side.

ATTENTION INPUTS (per (B, T); 4 heads x 128; logits below are SCALED, i.e. q . k / sqrt(128))
  soft        q, k = randn * 1.5: what every older test draws
  early_peak  8 exactly orthogonal +-1 directions u_g (rows of a column-signed Hadamard matrix); 8 keys in block 0 are 2.0 u_g, every
              other key is randn * 0.4; query i is 1.77 u_(i mod 8) + randn * 0.3.  Its own key scores 2.0 * 1.77 * sqrt(128) = 40, every
              other key N(0, 0.7) (orthogonality: the other peaks too): margin >= 30, and for T >= 128 no running maximum moves after block 0
  last_key    the same with ONE direction and its key at T - 1: the winner sits in the last valid column, beside the masked ones
  wave_alone  (T >= 128) one direction per key block, its key somewhere in that block; query i belongs to block i mod nkb: each wave of the
              split-K form holds the winner of some queries and nothing that matters for the rest
  ascending   k_j = 0.442 (block(j) - (nkb - 1) / 2) u + randn * 0.5, q = 2 u + randn * 0.1: the logit climbs by 2 * 0.442 * sqrt(128) = 10
              per key block with N(0, 1) inside a block: every query's maximum moves in every block (alpha ~ e^-10).  The ramp is centred
              (-30 .. +30 at seven blocks, not 0 .. 60): a logit of 60 alone needs sum |q k| >= 679, beyond what the bound below allows
  offset_neg  q = 0.8 q0 - 2 u, k = 0.8 k0 + 2 u with q0, k0 = randn made orthogonal to u: the logits of a soft softmax (std 0.64) moved by
              -4 sqrt(128) = -45.25, all of them in [-80, -40].  (randn * 1.5 underneath would need sum |q k| ~ 770: the same limit.)
  uniform     every key of a (hypothesis, head) is the same vector: p = 1 / T exactly, the output is the token mean of V for every query.
              The key is zero in half of its dimensions (randn * 2.1 in the others) and the queries of a head differ ONLY there: they are 400
              different rows with the same score, bit for bit (a product with 0 is exact) - so equal output bits are a property every correct
              kernel has.  (Queries with different scores m do not give it: p~ = 2^(fma(s, c2, -fl(m c2))) carries the rounding of m c2,
              1 +- 1e-7 per query, into l and moves an output that sits on an fp16 boundary.)

THE ATTENTION BOUND, per output element, from the reference alone (attention_tol).  The kernels compute s = q . k in fp32 (MFMA), p~ = 2^((s -
m) c2) with c2 = log2(e) / sqrt(128) relative to a running (flash form) or block (split-K form) maximum m, round p~ to fp16 for the PV MFMA,
accumulate O and the row sum l in fp32, rescale, divide and round the output to fp16.
  (1) 2^-11 s_abs, s_abs = sum_j p_j |v_j|: each p~ is rounded to fp16 (relative 2^-11) while at least as large as its final value (every later
      rescale is by alpha <= 1): |sum_j (dp_j) v_j| <= 2^-11 sum_j p_j |v_j|.
  (2) 2^-11 |o|: the output is rounded to fp16 once.
  (3) ln2 c2 128 2^-24 max_j qk_abs s_abs, qk_abs = sum_d |q_d k_d|: a score summed over 128 products in fp32 is off by at most 128 * 2^-24 *
      sum_d |q_d k_d|; an error ds of a score multiplies its p by 2^(ds c2) ~ 1 + ln2 c2 ds; weighting with |v_j| and bounding every key by the
      worst one gives the term (the same shift in the denominator only helps: to first order it cancels against the numerator's).
  (4) T 2^-24 max |v|: a p~ below the smallest fp16 subnormal 2^-24 flushes to 0 and one in the subnormal range is off by at most 2^-25: at most
      2^-24 |v_j| per key.
  (5) 1e-6: exp2 and reciprocal in hardware precision, fp32 sums of l and O (each ~ T 2^-24 relative on O(1) values), fp16 subnormal outputs.
For `uniform` every p~ is 1.0, exact in fp16: (1), (3) and (4) vanish and what is left is the output rounding (2) and the fp32 sum of T values
and the division by l = T: T 2^-24 s_abs.
Term (3) must not dominate: tests/test_heads_ref_host.py checks on every input set that it is at most term (1), i.e. max qk_abs <= 2^13 /
sqrt(128) = 724 - a condition on the inputs, not a measurement.

LAYERNORM INPUTS (rows of 512; the LayerNorm input is res + x W^T + b, or tok + att W_out^T + b_out)
  centred     what every older test draws: the residual operand randn * 2 + 0.5
  shift4 / 16 / 64   x W^T and the residual's noise have std 0.7 each (row sigma ~ 1), the residual's row means are 1.05 r (2 (i + 0.5) / M - 1)
              in shuffled order: uniform over +-1.05 r, a good half of the rows beyond r / 2.  LayerNorm2 of the head MLP: its input is x1 +
              ff W2^T + b2 and only per-COLUMN constants reach it (LayerNorm1 removes whatever a row brought along), so every row gets the
              same shift: b2 = 0.75 r * 1.28 + randn * 0.1 (1.28: the row sigma of x1 + ff W2^T) - every row at |mean| / sigma ~ 0.75 r
  eps         x = randn / 50, W / 8, b / 400, residual randn * 2e-3: row std ~ 3.2e-3, variance ~ 1e-5 = eps.  Head MLP: gamma1, beta1, b1 and
              b2 scaled by 3e-3 as well, so that x1 is tiny and LayerNorm2 sees a variance of ~ 1.5e-5
"""
import functools
import math
import zlib

import numpy as np
import torch

N_HEAD, D_HEAD, D_MODEL, VT_PAD, KB = 4, 128, 512, 416, 64
ATT_REGIMES = ('soft', 'early_peak', 'ascending', 'last_key', 'wave_alone', 'offset_neg', 'uniform')
ATT_T = (400, 399, 225, 224, 65, 64, 37)
ATT_B = 3                                             # hypotheses per small case: B = 3 runs them all, B = 1 the first, B = 2 the other two
PERSISTENT_REGIMES = ('early_peak', 'ascending', 'offset_neg')
PERSISTENT_SHAPES = ((70, 400), (130, 65))
PEAK_A, PEAK_B = 2.0, 1.77                            # k* = a u, q = b u + noise: a b sqrt(128) = 40.05
LN_REGIMES = ('centred', 'shift4', 'shift16', 'shift64', 'eps')
LN_EPS = 1e-5


def att_cases():
  return tuple((r, T) for r in ATT_REGIMES for T in ATT_T if r != 'wave_alone' or T >= 128)


def _seed(*what):
  return zlib.crc32('-'.join(str(w) for w in what).encode()) & 0x7fffffff


def vt_col(t):
  """Column of token t in the transposed V image (include/foundationpose_amd.h: groups of 16 in the order 0-3, 8-11, 4-7, 12-15)."""
  t = np.asarray(t)
  return (t & ~15) | (((t >> 2) & 1) << 3) | (((t >> 3) & 1) << 2) | (t & 3)


def make_vt(v):
  """v (B, 4, T, 128) fp16 -> the V image (B, 4, 128, 416) fp16, zeros past T."""
  B, _, T, _ = v.shape
  vt = torch.zeros((B, N_HEAD, D_HEAD, VT_PAD), dtype=torch.float16)
  vt[..., torch.from_numpy(vt_col(np.arange(T)))] = v.transpose(-1, -2)
  return vt


def _directions(rs):
  """128 exactly orthogonal +-1 vectors: the rows of the Sylvester Hadamard matrix, columns signed at random."""
  h = np.ones((1, 1))
  while len(h) < D_HEAD:
    h = np.block([[h, h], [h, -h]])
  return h * rs.choice([-1.0, 1.0], D_HEAD)[None, :]


def attention_inputs(regime, B, T):
  """-> dict(qk (B T, 1024) fp16 [q | k], v (B, 4, T, 128) fp16, vt the V image); seeded from (regime, B, T)."""
  rs = np.random.RandomState(_seed('att', regime, B, T))
  nkb = -(-T // KB)
  H = _directions(rs)
  q, k, v = (rs.randn(B, N_HEAD, T, D_HEAD) for _ in range(3))
  if regime == 'soft':
    q, k = q * 1.5, k * 1.5
  elif regime == 'uniform':
    on = np.stack([rs.permutation(D_HEAD) < D_HEAD // 2 for _ in range(B * N_HEAD)]).reshape(B, N_HEAD, 1, D_HEAD)
    k = np.repeat(np.where(on, k[:, :, :1] * 2.1, 0.0), T, axis=2)
    q = np.where(on, q[:, :, :1], q) * 1.5
  elif regime == 'offset_neg':
    u = H[0]
    q = 0.8 * (q - (q @ u)[..., None] * u / D_HEAD) - 2.0 * u
    k = 0.8 * (k - (k @ u)[..., None] * u / D_HEAD) + 2.0 * u
  elif regime == 'ascending':
    u = H[0]
    ramp = np.arange(T) // KB - (nkb - 1) / 2
    q = 2.0 * u + 0.1 * q
    k = 0.442 * ramp[:, None] * u + 0.5 * k
  else:
    if regime == 'early_peak':
      ndir = min(8, T)
      pos = np.stack([rs.permutation(min(KB, T))[:ndir] for _ in range(B * N_HEAD)]).reshape(B, N_HEAD, ndir)
    elif regime == 'last_key':
      ndir, pos = 1, np.full((B, N_HEAD, 1), T - 1)
    elif regime == 'wave_alone':
      assert T >= 2 * KB
      ndir = nkb
      pos = np.stack([g * KB + rs.randint(0, min(KB, T - g * KB), size=(B, N_HEAD)) for g in range(nkb)], axis=-1)
    else:
      raise ValueError(regime)
    q = PEAK_B * H[np.arange(T) % ndir] + 0.3 * q
    k = 0.4 * k
    bi, hi = np.meshgrid(np.arange(B), np.arange(N_HEAD), indexing='ij')
    for g in range(ndir):
      k[bi, hi, pos[..., g]] = PEAK_A * H[g]
  q, k, v = (torch.from_numpy(a).half() for a in (q, k, v))
  qk = torch.cat([q.transpose(1, 2).reshape(B * T, D_MODEL), k.transpose(1, 2).reshape(B * T, D_MODEL)], dim=1).contiguous()
  return dict(qk=qk, v=v, vt=make_vt(v))


def split_qk(qk, B, T):
  """qk (B T, 1024) -> q, k (B, 4, T, 128) float64."""
  qk = qk.double().reshape(B, T, 2, N_HEAD, D_HEAD)
  return qk[:, :, 0].transpose(1, 2), qk[:, :, 1].transpose(1, 2)


def scaled_logits(qk, B, T):
  q, k = split_qk(qk, B, T)
  return (q @ k.transpose(-1, -2)) / math.sqrt(D_HEAD)


def _rows(x, B, T):
  return x.transpose(1, 2).reshape(B * T, D_MODEL)


@torch.no_grad()
def attention_ref(qk, v, B, T):
  """softmax(q k^T / sqrt(128)) v in float64 on the fp16 operands.  -> o, s_abs = sum_j p_j |v_j| (both (B T, 512), the kernel's output
  layout) and qk_abs = sum_d |q_d k_d| per (query, key): (B, 4, T, T)."""
  q, k = split_qk(qk, B, T)
  vv = v.double()
  p = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(D_HEAD), dim=-1)
  return _rows(p @ vv, B, T), _rows(p @ vv.abs(), B, T), q.abs() @ k.abs().transpose(-1, -2)


C2 = math.log2(math.e) / math.sqrt(D_HEAD)
SCORE_TERM = math.log(2) * C2 * D_HEAD * 2.0 ** -24          # x max_j qk_abs x s_abs: term (3) of the bound
QK_ABS_LIMIT = 2.0 ** -11 / SCORE_TERM                       # 724: where term (3) reaches term (1)


def attention_tol(o, s_abs, qk_abs_max, T, vmax, uniform=False):
  """The bound of the module docstring.  o, s_abs, qk_abs_max (max over the keys, spread over the query's 128 outputs): (B T, 512)."""
  if uniform:
    return 2.0 ** -11 * np.abs(o) + T * 2.0 ** -24 * s_abs
  return 2.0 ** -11 * s_abs + 2.0 ** -11 * np.abs(o) + SCORE_TERM * qk_abs_max * s_abs + T * 2.0 ** -24 * vmax + 1e-6


@functools.lru_cache(maxsize=None)
def attention_case(regime, B, T):
  """Inputs, reference and bound of one case, computed once (eight hypotheses at a time: qk_abs of (70, 400) would be 360 MB)."""
  inp = attention_inputs(regime, B, T)
  o, s_abs, qmax = [], [], []
  for b0 in range(0, B, 8):
    nb = min(8, B - b0)
    oo, ss, qa = attention_ref(inp['qk'][b0 * T:(b0 + nb) * T], inp['v'][b0:b0 + nb], nb, T)
    o.append(oo.numpy())
    s_abs.append(ss.numpy())
    qmax.append(_rows(qa.max(-1).values[..., None].expand(nb, N_HEAD, T, D_HEAD), nb, T).numpy())
  o, s_abs, qmax = (np.concatenate(a) for a in (o, s_abs, qmax))
  vmax = float(inp['v'].abs().max())
  tol = attention_tol(o, s_abs, qmax, T, vmax, uniform=regime == 'uniform')
  for a in (o, s_abs, qmax, tol):
    a.setflags(write=False)
  return dict(inp, o=o, s_abs=s_abs, qk_abs_max=qmax, tol=tol, vmax=vmax)


# ------------------------------------------------------------------------------------------------------------------------
# LayerNorm: the epilogues of fp_token_linear_f16 and the head MLP

def _ln64(y, gam, bet, eps=LN_EPS, eps_outside=False):
  mean = y.mean(-1, keepdim=True)
  var = ((y - mean) ** 2).mean(-1, keepdim=True)
  rstd = 1.0 / (var.sqrt() + eps) if eps_outside else 1.0 / (var + eps).sqrt()
  n = (y - mean) * rstd
  if gam is not None:
    n = n * gam.double() + bet.double()
  return n


def row_stats(y):
  """-> (|mean| / sigma, variance) per row, float64 numpy."""
  mean, var = y.mean(-1), y.var(-1, unbiased=False)
  return (mean.abs() / var.sqrt()).numpy(), var.numpy()


def _shift_means(rs, M, r):
  return 1.05 * r * (2 * (rs.permutation(M) + 0.5) / M - 1)


def _common(rs, M, regime):
  """x (the GEMM operand), the residual operand, W and b of a residual + Linear in front of a LayerNorm."""
  x, res = rs.randn(M, D_MODEL), rs.randn(M, D_MODEL)
  w, b = rs.randn(D_MODEL, D_MODEL) * (1.0 / D_MODEL) ** 0.5, rs.randn(D_MODEL) * 0.1
  if regime == 'centred':
    res = res * 2 + 0.5
  elif regime == 'eps':
    x, w, b, res = x / 50, w / 8, b / 400, res * 2e-3
  else:
    r = int(regime[5:])
    x, res = x * 0.7, res * 0.7 + _shift_means(rs, M, r)[:, None]
  return x, res, w, b


def _t16(a):
  return torch.from_numpy(a).half()


def _t32(a):
  return torch.from_numpy(a).float()


def _w16(a):
  return torch.from_numpy(a).half().float()          # the kernels pack the weights as fp16


@functools.lru_cache(maxsize=None)
def token_linear_inputs(regime, n_hyp):
  """-> dict(x, res (M, 512) fp16; w (512, 512) fp32 holding fp16 values; b, gam, bet fp32), M = 400 n_hyp."""
  M = 400 * n_hyp
  rs = np.random.RandomState(_seed('toklin', regime, n_hyp))
  x, res, w, b = _common(rs, M, regime)
  gam, bet = rs.rand(D_MODEL) + 0.5, rs.randn(D_MODEL) * 0.1
  return dict(x=_t16(x), res=_t16(res), w=_w16(w), b=_t32(b), gam=_t32(gam), bet=_t32(bet))


def group_sums(n):
  return n.reshape(len(n) // 16, 16, D_MODEL).sum(1)


@torch.no_grad()
def layernorm_ref(inp, eps=LN_EPS, eps_outside=False):
  """Epilogues 2 and 3 of fp_token_linear_f16 in float64: -> (LayerNorm(res + x W^T + b) gamma + beta (M, 512), the sums over groups of 16
  tokens of the normalised rows without gamma / beta (M / 16, 512), the LayerNorm input y)."""
  y = inp['res'].double() + inp['x'].double() @ inp['w'].double().T + inp['b'].double()
  return _ln64(y, inp['gam'], inp['bet'], eps, eps_outside), group_sums(_ln64(y, None, None, eps, eps_outside)), y


@functools.lru_cache(maxsize=None)
def head_mlp_inputs(regime, n_hyp):
  """-> dict(att, tok (M, 512) fp16; w_out, w1, w2 fp32 holding fp16 values; b_out, g1, be1, b1, b2 fp32), M = 400 n_hyp."""
  M = 400 * n_hyp
  rs = np.random.RandomState(_seed('headmlp', regime, n_hyp))
  att, tok, w_out, b_out = _common(rs, M, regime)
  w1, w2 = (rs.randn(D_MODEL, D_MODEL) * (1.0 / D_MODEL) ** 0.5 for _ in range(2))
  b1, b2 = rs.randn(D_MODEL) * 0.1, rs.randn(D_MODEL) * 0.1
  g1, be1 = rs.rand(D_MODEL) + 0.5, rs.randn(D_MODEL) * 0.1
  if regime == 'eps':
    g1, be1, b1, b2 = g1 * 3e-3, be1 * 3e-3, b1 * 3e-3, b2 * 3e-3
  elif regime != 'centred':
    b2 = b2 + 0.75 * int(regime[5:]) * 1.28
  return dict(att=_t16(att), tok=_t16(tok), w_out=_w16(w_out), b_out=_t32(b_out), g1=_t32(g1), be1=_t32(be1), w1=_w16(w1), b1=_t32(b1),
              w2=_w16(w2), b2=_t32(b2))


@torch.no_grad()
def head_mlp_ref(inp, eps=LN_EPS, eps_outside=False, round16=True):
  """fp_head_mlp_f16 in float64: x1 = LayerNorm1(tok + att W_out^T + b_out), ff = relu(x1 W1^T + b1), the sums over groups of 16 tokens of
  LayerNorm2(x1 + ff W2^T + b2) without gamma / beta.  round16: x1 and ff rounded to fp16 where the kernel rounds them (they are GEMM
  operands).  -> (sums (M / 16, 512), the input of LayerNorm1, the input of LayerNorm2)."""
  r16 = (lambda t: t.half().double()) if round16 else (lambda t: t)
  y1 = inp['tok'].double() + inp['att'].double() @ inp['w_out'].double().T + inp['b_out'].double()
  x1 = r16(_ln64(y1, inp['g1'], inp['be1'], eps, eps_outside))
  ff = r16(torch.relu(x1 @ inp['w1'].double().T + inp['b1'].double()))
  y2 = x1 + ff @ inp['w2'].double().T + inp['b2'].double()
  return group_sums(_ln64(y2, None, None, eps, eps_outside)), y1, y2
