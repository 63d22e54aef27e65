// What a network pass runs besides its convolutions (conv_plan.h): the schedule - hypotheses per pass, trunk parts, side chains, head streams -
// and the kernel form of every stage behind the trunk, as pure host functions of the sizes and the FP_* knobs.  Nothing here needs HIP:
// this header includes standard C headers and conv_plan.h only and compiles on its own (tests/test_pass_plan_host.py).
//
// THE THREE SIZE CLASSES of a forward body of n images (default knobs); each has its own last bits, within a class a hypothesis'
// arithmetic does not depend on its batch:
//   n = 1 .. 2    few-image forms throughout: conv_small.hip, tok_qkv_small_kernel, attention_small_kernel; 64-token head MLP; split-K scratch on offer
//   n = 3 .. 4    batch in-projections (128-token) and persistent attention; split-K 3x3 layers (scratch on offer), 64-token head MLP
//   n >= 5        batch forms, no scratch, 128-token head MLP; from 48 on the trunk as 2 parts on 2 streams (bit-identical to one batch)
//
// WHICH COUNT EACH STAGE KEYS ON, as the code does today.  "body": the images of one forward body - the whole pass, or one chunk of it
// under FP_CHUNK; "part": one trunk part of a body (the body itself below FP_TRUNK_MIN); "pass": the hypotheses of a fused pass of api.hip.
//   hypotheses per pass (hyp_chunk)            pass
//   side chains, shared side B, fused tail     pass, its runs of like objects and live objects (pass_plan)
//   trunk parts                                body
//   split-K scratch offer, ConvArgs::hyp       part   (conv_plan then keys the small form on that hyp, the split factors on the launch's own shape)
//   ConvArgs::hyp of the shared side B         pass   (fp_encode_side_b; a pass with a shared side B has no chunks: pass = body)
//   in-projections                             body   (run_qkv hands it to launch_tok_qkv as `hyp`)
//   attention                                  the launch's own images = body
//   head MLP                                   the launch's own tokens = 400 x body
//   head streams                               -
// So inside one body every stage sees the same n, chunked or not: a short last chunk of 1 .. 2 hypotheses takes the few-image forms
// THROUGHOUT, convolutions included (run_trunk plans them with the chunk, not the pass).  The stages can disagree only where knobs move them
// apart: FP_TRUNK_MIN below 6 cuts a body into parts of 1 .. 2 images whose convolutions take the few-image form while the body's
// in-projections and attention take the batch forms (FP_TRUNK_MIN below 10: parts of up to 4 get scratch, the body's head MLP is the 128-token
// form); FP_QKV_SMALL or FP_ATTN_SMALL other than 2 move one stage's threshold alone (conv_plan's is the constant 2).  With default knobs
// a trunk part has at least 24 images and the classes coincide at every size.
//
// WHERE A STAND-ALONE BUILDING-BLOCK CALL DIFFERS, on purpose:
//   * fp_token_linear_f16 epilogues 4 / 5 pass hyp = 0: the 128-token kernel at any size, one image included; 6 / 7 pass hyp = 1: the few-image form;
//   * fp_attention_f16 and fp_head_mlp_f16 have no pass: the launch's own size decides, as inside a body;
//   * fp_net_tokens runs one trunk part of n images, never cut in parts, with no side chains;
//   * fp_refine_forward / fp_score_features are whole passes with one chain (nobody forked the sides).
#pragma once
#include <limits.h>

#include "conv_plan.h"

// The knobs that steer the choice, with their defaults; pass_knobs() (net.hip) holds the process's values, read from the environment once.
// A/B timing and experiments only: except FP_CHUNK, FP_QKV_SMALL, FP_ATTN_SMALL and FP_HEADMLP64 (which move a size class) results are bit-identical.
struct PassKnobs {
  int chunk = 0;               // FP_CHUNK: hypotheses per network pass (<= 0 or above the pass: the whole batch)
  int trunk_min = 48;          // FP_TRUNK_MIN: hypotheses of a body from which its trunk is cut in parts
  int trunk_streams = 2;       // FP_TRUNK_STREAMS: most parts (below 2: never cut)
  bool one_chain = false;      // FP_ONE_CHAIN != 0: the two sides of encodeA as one chain
  bool no_shared_b = false;    // FP_NO_SHARED_B set: ignore FP_REFINE_SHARED_TRANSLATION
  bool tail_split = false;     // FP_TAIL_SPLIT set: the tail of a refinement pass as four launches instead of one
  int qkv_small = 2;           // FP_QKV_SMALL: hypotheses up to which the few-image in-projections run (0: off)
  bool qkv64 = false;          // FP_QKV64 set: the 64-token kernel, one launch for q | k, one for v, in place of the 128-token one
  int attn_small = 2;          // FP_ATTN_SMALL: images up to which attention_small_kernel (split-K) runs (0: off)
  bool headmlp64 = false;      // FP_HEADMLP64 set: the 64-token head MLP (two resident tiles) at every size
  bool heads_serial = false;   // FP_HEADS_SERIAL set: both RefineNet heads on one stream
  bool front_fused = true;     // FP_FRONT_FUSED: 0 runs the stem and the 64 -> 128 stride-2 layer of encodeA as two launches (bit-identical)
};
const PassKnobs &pass_knobs();

enum PassKind { PASS_REFINE = 0, PASS_SCORE = 1 };      // (= FP_NET_REFINE, FP_NET_SCORE)
enum AttnForm { ATTN_SMALL, ATTN_PERSISTENT };
enum HeadMlpForm { HEAD_MLP_64, HEAD_MLP_128, HEAD_MLP_NONE };
enum QkvForm { QKV_SMALL, QKV_TOK128, QKV_PAIR64 };

#define PASS_SIDE_STREAMS 8            // side streams of a context (fp_ctx::NSIDE)
#define PASS_SHARED_B_MAX_OBJECTS 8    // live objects of a pass with a shared side B (SharedB::start)
#define PASS_FLAG_SHARED_TRANSLATION 1u      // (= FP_REFINE_SHARED_TRANSLATION)

// attention_small_kernel (keys split over the workgroups of a query tile) or the persistent kernel, by the launch's images
inline AttnForm attn_form(int images, const PassKnobs &k) { return images <= k.attn_small ? ATTN_SMALL : ATTN_PERSISTENT; }

// 1 .. 4 hypotheses (tracking): the 64-token form.  Every workgroup streams all 1.5 MB of weights whatever its tile holds, so a launch
// of a handful of workgroups lasts one workgroup's life: 26.8 us for seven 64-token tiles against 38.5 for four 128-token ones at one
// hypothesis.  (Its own size class, like split-K in the 3x3 kernel: the two forms differ in the last bits, see the 128-token form's header.)
inline HeadMlpForm head_mlp_form(int M, const PassKnobs &k) { return k.headmlp64 || M <= 1600 ? HEAD_MLP_64 : HEAD_MLP_128; }

// The in-projections of a body of `images` (hyp: the body's images again; 0: a stand-alone call).  The few-image form of one and two
// hypotheses has its own bits, so FP_QKV64 compares the two batch kernels only: above FP_QKV_SMALL.
inline QkvForm qkv_form(int hyp, int images, const PassKnobs &k) {
  if (hyp > 0 && hyp <= k.qkv_small) return QKV_SMALL;
  if (hyp > 0 && k.qkv64 && images > k.qkv_small) return QKV_PAIR64;
  return QKV_TOK128;
}

// The front end of encodeA (x -> a1: the 7x7 stem, then the 64 -> 128 stride-2 layer) as ONE launch (front.hip) wherever the two launches
// would be the stem form followed by the implicit GEMM: not in the passes of one and two hypotheses, whose stride-2 layer is the few-image form.
// `images`: of the stride-2 launch as it would run; hyp: the pass's hypotheses (ConvArgs::hyp); splitk: whether scratch is on offer.
inline bool front_fused(int images, int hyp, bool splitk, int num_cu, const PassKnobs &k, const ConvKnobs &ck) {
  if (!k.front_fused || images <= 0) return false;
  ConvArgs st = conv_args(nullptr, images, 160, 160, 8, nullptr, nullptr, 64, 7, 7, 2, 3, conv_kpad(7, 7, 8), nullptr);
  ConvArgs dn = conv_args(nullptr, images, 80, 80, 64, nullptr, nullptr, 128, 3, 3, 2, 1, conv_kpad(3, 3, 64), nullptr);
  st.relu = dn.relu = 1, st.hyp = dn.hyp = hyp;
  const unsigned sk = splitk ? CONV_OFFER_SPLITK : 0u;
  return conv_plan(st, num_cu, sk, ck).form == CONV_STEM && conv_plan(dn, num_cu, CONV_OFFER_SMALL | CONV_OFFER_S2 | sk, ck).form == CONV_IGEMM2;
}

// from 48 hypotheses on (round 4, refine x5 + score of one object: 40 hypotheses 6.55 ms as one batch / 7.08 split, 48: 7.82 / 7.55, 56: 8.87 / 8.17,
// 63: 9.85 / 9.23, 64: 9.95 / 9.32, 96: 13.97 / 13.71; scripts/bench_nhyp.py): below, the halves' tiles get too small
inline int trunk_split_min(const PassKnobs &k) { return k.trunk_streams < 2 ? INT_MAX : k.trunk_min; }
inline int trunk_parts(int n, const PassKnobs &k, int n_side_streams) {
  if (n < trunk_split_min(k)) return 1;
  const int by_size = n / 32 > 2 ? n / 32 : 2;
  const int cap = k.trunk_streams < n_side_streams ? k.trunk_streams : n_side_streams;
  return cap < by_size ? cap : by_size;
}

// The networks take split-K scratch from the arena for trunk parts of up to CONV_NET_SPLITK_MAX_HYP hypotheses (conv_plan.h)
inline bool net_offers_splitk(int n) { return n <= CONV_NET_SPLITK_MAX_HYP; }

// Hypotheses per network pass: the whole batch.  FP_CHUNK=n (experiments only) splits it.
inline int hyp_chunk(int n_total, const PassKnobs &k) { return k.chunk <= 0 || k.chunk > n_total ? n_total : k.chunk; }

// Everything one forward body of n images runs behind its input
struct ForwardPlan {
  int n;
  int trunk_parts;             // 1: one batch on the caller's stream(s); more: parts on that many streams (trunk_part)
  QkvForm qkv;
  AttnForm attn;               // what launch_attention picks for the body's n images
  HeadMlpForm head_mlp;        // what launch_head_mlp picks for its 400 n tokens (ScoreNet: none)
  int head_streams;            // RefineNet: streams its two heads run on (ScoreNet: 0, no heads)
};

inline ForwardPlan forward_plan(int kind, int n, const PassKnobs &k, int n_side_streams = PASS_SIDE_STREAMS) {
  ForwardPlan p;
  p.n = n;
  p.trunk_parts = trunk_parts(n, k, n_side_streams);
  p.qkv = qkv_form(n, n, k);
  p.attn = attn_form(n, k);
  p.head_mlp = kind == PASS_REFINE ? head_mlp_form(n * 400, k) : HEAD_MLP_NONE;
  p.head_streams = kind == PASS_REFINE ? (k.heads_serial ? 1 : 2) : 0;
  return p;
}

// Part i of a body's trunk: images [start, start + n) of the body, the hyp its convolutions are planned with and whether they are offered scratch
struct TrunkPart {
  int start, n, conv_hyp;
  bool splitk;
};
inline TrunkPart trunk_part(const ForwardPlan &p, int i) {
  const int a0 = (int)((long long)p.n * i / p.trunk_parts), a1 = (int)((long long)p.n * (i + 1) / p.trunk_parts);
  return TrunkPart{a0, a1 - a0, a1 - a0, net_offers_splitk(a1 - a0)};
}

// What a fused pass of api.hip decides (n_runs: runs of like objects; n_live: objects with at least one hypothesis; flags: of the call)
struct PassPlan {
  int chunk;                   // hypotheses per forward body (hyp_chunk)
  // One run of like objects in a batch that the trunk does not cut by hypotheses: the observed side (crop window -> observed crop) is
  // produced on a side stream and does not wait for the rasteriser ...
  bool fork_sides;
  bool side_chains;            // ... and stays there through encodeA up to the channel concat (a chunked pass joins in front of its first chunk)
  bool shared_b;               // side B of iteration 1 as ONE crop per object: one run, at most 8 live objects, no chunks
  bool fused_tail;             // token means, pose update, next crop windows as one launch: one run, no chunks
};

inline PassPlan pass_plan(int kind, int n_total, int n_runs, int n_live, unsigned flags, const PassKnobs &k) {
  PassPlan p;
  p.chunk = hyp_chunk(n_total, k);
  const bool whole = p.chunk == n_total, refine_run = kind == PASS_REFINE && n_runs == 1 && whole;
  p.fork_sides = n_runs == 1 && n_total < trunk_split_min(k) && !k.one_chain;
  p.side_chains = p.fork_sides && whole;
  p.shared_b = refine_run && (flags & PASS_FLAG_SHARED_TRANSLATION) && !k.no_shared_b && n_live <= PASS_SHARED_B_MAX_OBJECTS;
  p.fused_tail = refine_run && !k.tail_split;
  return p;
}

inline const char *attn_form_name(AttnForm f) { return f == ATTN_SMALL ? "attn-small" : "attn-persistent"; }
inline const char *head_mlp_form_name(HeadMlpForm f) { return f == HEAD_MLP_64 ? "mlp64" : f == HEAD_MLP_128 ? "mlp128" : "none"; }
inline const char *qkv_form_name(QkvForm f) { return f == QKV_SMALL ? "qkv-small" : f == QKV_TOK128 ? "qkv128" : "qkv64-pair"; }
