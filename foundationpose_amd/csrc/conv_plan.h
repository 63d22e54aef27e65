// Which kernel form a convolution launch runs: ONE decision, as a pure host function of the launch's shape, the chip's CU count, what
// the caller offers (packed copies of the weights, split-K scratch) and the FP_* knobs.  Nothing here needs HIP: this header includes
// standard C headers only and compiles on its own (tests/test_conv_plan_host.py plans every case of tests/tools/conv_ref.py with it).
//
// PRIORITY (conv_plan; the first form whose conditions hold):
//   1. small         conv_small.hip   a few images of the trunks' 3x3 layers                          reads the small-packed weights
//   2. s1b           conv_s1b.hip     128 -> 128 (FP_C128_BAND=2: any) 3x3 stride 1 on 40x40 maps, more than 512 pixels per CU   s1b-packed weights
//   3. halo-splitk   conv_halo.hip    3x3 stride 1 on 40x40 / 20x20 maps, a few workgroups, >= 256 input channels                 split-K scratch
//      halo          conv_halo.hip    every other 3x3 stride-1 layer on 40x40 / 20x20 maps (tiling: halo_plan)
//   4. s2-splitk     conv.hip         3x3 stride 2 with >= 36 K-steps below S2_MIN_PIXELS output pixels                           split-K scratch
//   5. stem          stem.hip         the 7x7 stride-2 8 -> 64 layer
//   6. s2            conv_s2.hip      3x3 stride 2 to 20x20 maps from S2_MIN_PIXELS output pixels on                              s2-packed weights
//   7. igemm2        conv.hip         everything else: 1x1 (Linear), 3x3, 7x7 implicit GEMM
// A form that reads packed weights or scratch is taken only when the caller offers them (ConvOffer); CONV_FORCE_S1B puts s1b in front of
// everything for the launches its kernel supports.  The shape predicates test
// ConvArgs::res and ::post_add for null (some forms add neither); the plan reads no other pointer of the launch.
//
// WHERE THE CALLERS DIFFER, on purpose:
//   * the networks offer split-K scratch only up to four hypotheses (CONV_NET_SPLITK_MAX_HYP; run_trunk, net.hip) and none for the shared observed side
//     (fp_encode_side_b); fp_conv2d_f16 offers it at any size, so five images of the 20x20 512 -> 512 layer run halo-splitk there
//     (4 n_q = 256 <= 256 CUs) and the one-launch kernel inside a network;
//   * fp_conv2d_f16 never offers the s1b packing: the band form is reached through fp_conv3x3_band_f16, which forces it
//     (CONV_FORCE_S1B) at any image count;
//   * a stand-alone call passes hyp = 0 and takes the small form by its workgroup count (at most two per CU); a launch of a network
//     pass takes it by the pass's hypotheses (1 .. 2), whatever its own share of the images.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef FP_F16_TYPEDEF
#define FP_F16_TYPEDEF
typedef _Float16 f16;
#endif

struct ConvArgs {
  const f16 *in;
  const f16 *w;
  const float *bias;
  const f16 *res;
  const float *post_add;
  void *out;
  int Nimg, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, Kpad, M;
  int relu, out_mode;  // 0 fp16 NHWC, 1 fp32 NHWC, 2 fp16 V-transposed [b][4][128][416], token t in column vt_col(t)
  int out_ld, split_m, coff_hi, post_period, tokens;
  // split-K of the 3x3 stride-1 kernel for launches of a few workgroups (3 .. 4 hypotheses; 1 .. 2, a tracking frame, run conv_small.hip): `ksplit` workgroups share
  // the input-channel chunks of a tile and leave fp32 partial sums in `splitk` [ksplit][M][Cout]; a finishing pass adds them in a
  // fixed order and applies bias-free epilogue (the bias rides in split 0).  0 / nullptr: off.
  float *splitk = nullptr;
  int ksplit = 0;
  // 3x3 stride-2 layers: the weights in the fragment order of conv_s2.hip (s2_pack_weights); nullptr: the implicit-GEMM kernel runs
  const f16 *wpk = nullptr;
  // 3x3 stride-1 layers: the weights in the fragment order of conv_small.hip (small_pack_weights); nullptr: that form is not used
  const f16 *wsm = nullptr;
  // hypotheses of the network pass this launch belongs to (0: a stand-alone call): the few-image form is chosen by it, so that the two sides
  // of encodeA as one chain or two (twice the images per launch) take the same kernel
  int hyp = 0;
};

// K of the [Cout][Kpad] weight rows: KH KW Cin up to the next multiple of 32 (one K-step of the implicit GEMM)
inline int conv_kpad(int KH, int KW, int Cin) { return (KH * KW * Cin + 31) / 32 * 32; }

// One launch: operands, geometry and everything derived from them (Ho, Wo, M) with the defaults of the output placement - fp16 NHWC
// rows of Cout, no split into two column blocks, no residual, no ReLU, no post-add.  Callers set what differs.
inline ConvArgs conv_args(const f16 *in, int Nimg, int H, int W, int Cin, const f16 *w, const float *bias, int Cout, int KH, int KW, int stride, int pad,
                          int Kpad, void *out) {
  ConvArgs a = {};
  a.in = in, a.w = w, a.bias = bias, a.out = out;
  a.Nimg = Nimg, a.H = H, a.W = W, a.Cin = Cin, a.Cout = Cout, a.KH = KH, a.KW = KW, a.stride = stride, a.pad = pad, a.Kpad = Kpad;
  a.Ho = (H + 2 * pad - KH) / stride + 1;
  a.Wo = (W + 2 * pad - KW) / stride + 1;
  a.M = Nimg * a.Ho * a.Wo;
  a.out_ld = Cout;
  a.split_m = 0x7fffffff;
  a.post_period = 1;
  a.tokens = 400;
  return a;
}

enum ConvForm { CONV_SMALL, CONV_S1B, CONV_HALO, CONV_HALO_SPLITK, CONV_S2_SPLITK, CONV_STEM, CONV_S2, CONV_IGEMM2 };

// What the caller holds or is willing to make (bits)
enum ConvOffer : unsigned {
  CONV_OFFER_SMALL = 1,       // weights packed by small_pack_weights (ConvArgs::wsm)
  CONV_OFFER_S2 = 2,          // weights packed by s2_pack_weights in conv_s2.hip's order (ConvArgs::wpk of a stride-2 layer)
  CONV_OFFER_S1B = 4,         // ... in conv_s1b.hip's order (ConvArgs::wpk of a stride-1 layer)
  CONV_OFFER_SPLITK = 8,      // fp32 scratch for the shares of a split-K launch (ConvArgs::splitk)
  CONV_FORCE_S1B = 16,        // fp_conv3x3_band_f16: the s1b form for every launch it supports, whatever the image count, the channels and FP_C128_BAND
};

// The knobs that steer the choice, with their defaults; conv_knobs() (conv.hip) holds the process's values, read from the environment once
struct ConvKnobs {
  int small = 1;               // FP_SMALL: 0 switches conv_small.hip off (A/B timing)
  int small_max_wg = 0;        // FP_SMALL_MAX_WG: the small form by workgroup count (also inside a network pass); 0: two per CU, stand-alone calls only
  int c128_band = 1;           // FP_C128_BAND: conv_s1b.hip (bit-identical to the halo kernel); 0: off, 2: also the 256 -> 256 layers
  int ksplit_max = 8;          // FP_KSPLIT_MAX: most shares of a halo split-K launch
  int ksplit_min_chunks = 8;   // FP_KSPLIT_MIN_CHUNKS: fewest 32-channel chunks that are split (0: split the 128-channel layers too)
  int halo_tail = 1;           // FP_HALO_TAIL: 0 disables the tail split of halo_split and halo_plan (A/B timing only; results are identical)
  int halo_nt = 0;             // FP_HALO_NT: experiments: tiles of this many x 128 pixels for whatever is not a whole round
};
const ConvKnobs &conv_knobs();

// Tile constants the predicates share with the kernels
#define HL_BM 128               // conv_halo.hip: couts per tile
#define HL_CK 32                // conv_halo.hip: input channels per chunk
#define B1_W 40                 // conv_s1b.hip: map edge
#define ST_BLK 16               // stem.hip: output block edge
#define C2_BK 32                // conv.hip: K per step
// conv_s2.hip runs from this many output pixels on; below (1 .. 4 hypotheses at 20x20 outputs: the sizes whose 3x3 stride-1 layers run split-K)
// the implicit-GEMM kernel with its 64-pixel tail tiles runs
#define S2_MIN_PIXELS 2000

// ---- shape predicates: what each form's kernel can run (the packed weights it reads are the caller's offer, not part of the shape) ----
inline bool conv_halo_supported(const ConvArgs &a) {
  return a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.H == a.W && (a.W == 40 || a.W == 20) && a.Cin % HL_CK == 0 &&
         a.Cout % HL_BM == 0 && a.out_mode == 0 && a.Kpad == 9 * a.Cin && a.out_ld % 8 == 0 && a.coff_hi % 8 == 0;
}

inline bool s1b_supported(const ConvArgs &a) {
  return a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.out_mode == 0 && !a.post_add && a.H == B1_W && a.W == B1_W && a.Cin % 32 == 0 &&
         a.Cout % 128 == 0 && a.Kpad == 9 * a.Cin && a.out_ld % 8 == 0 && a.coff_hi % 8 == 0 &&
         (long long)a.Nimg * B1_W * B1_W * a.Cin * 2 < (1ll << 31);        // 32-bit byte offsets into the input (above: the general 3x3 kernel, 4 GB)
}

// co tiles of 32 per wave: 2 -> 256-cout blocks, 1 -> 128-cout blocks; 0: this Cout is not handled here.  A function of Cout alone,
// so that the weights can be packed when the network is loaded (the spatial size is not known then).
inline int s2_ct_for(int Cout) { return Cout % 256 == 0 ? 2 : Cout % 128 == 0 ? 1 : 0; }

inline bool s2_supported(const ConvArgs &a) {
  return a.KH == 3 && a.KW == 3 && a.stride == 2 && a.pad == 1 && a.out_mode == 0 && !a.res && !a.post_add && a.out_ld == a.Cout && a.split_m >= a.M &&
         a.H == a.W && a.Ho == a.Wo && a.H == 2 * a.Ho && a.Wo == 20 && a.Cin >= 16 && a.Cin % 16 == 0 && a.Kpad >= 9 * a.Cin &&
         s2_ct_for(a.Cout) != 0;
}

inline bool stem_supported(const ConvArgs &a) {
  return a.KH == 7 && a.KW == 7 && a.stride == 2 && a.pad == 3 && a.Cin == 8 && a.Cout == 64 && a.Kpad >= 400 && a.out_mode == 0 && !a.res &&
         !a.post_add && a.out_ld == 64 && a.split_m >= a.M && a.Ho % ST_BLK == 0 && a.Wo % ST_BLK == 0 && a.H == 2 * a.Ho && a.W == 2 * a.Wo;
}

// conv_small.hip has one instantiation per (input channels, stride) of the trunks' 3x3 layers, built for the map that layer runs on: the
// stride-1 layers (128 / 256 channels on 40x40 maps, 512 on 20x20) and the two stride-2 layers (64 -> 128 on 80x80 behind the stem,
// 256 -> 512 on 40x40 between the two halves of encodeAB).  -> the edge of the input map; 0: no instantiation
inline int small_map_for(int Cin, int stride) {
  if (stride == 1) return Cin == 128 || Cin == 256 ? 40 : Cin == 512 ? 20 : 0;
  if (stride == 2) return Cin == 256 ? 40 : Cin == 64 ? 80 : 0;
  return 0;
}

// The launches the small form runs: those layers in the network passes of one or two hypotheses, and stand-alone launches of at most
// FP_SMALL_MAX_WG workgroups (default 2 per CU).  FP_SMALL=0: off (A/B timing).
inline bool conv_small_shape(const ConvArgs &a, int num_cu, const ConvKnobs &k) {
  if (!k.small) return false;
  const int hw = small_map_for(a.Cin, a.stride);
  if (!(a.KH == 3 && a.KW == 3 && a.pad == 1 && hw != 0 && a.H == hw && a.W == hw && a.Ho == hw / a.stride && a.Wo == hw / a.stride && a.out_mode == 0 &&
        a.Cout % 32 == 0 && a.Kpad == 9 * a.Cin && a.out_ld % 4 == 0 && a.coff_hi % 4 == 0 && a.M > 0))
    return false;
  if (a.hyp > 0 && k.small_max_wg == 0) return a.hyp <= 2;           // inside a network pass: by its hypotheses, whatever the launch's share of them
  const long long wgs = (long long)((a.M + 31) / 32) * (a.Cout / 32);
  return wgs <= (k.small_max_wg > 0 ? k.small_max_wg : 2 * num_cu);
}

// The s1b form runs from the batch size on at which the general kernel needs more than one round of its 512-pixel tiles (82 images on 256
// CUs): below, one round of those is faster (32 hypotheses per GPU: 6.67 against 6.79 ms per step; 63: 10.24 against 10.13)
inline bool conv_s1b_use(const ConvArgs &a, int num_cu, const ConvKnobs &k) {
  return k.c128_band != 0 && (a.Cin == 128 || k.c128_band == 2) && (long long)a.M > (long long)num_cu * 512 && s1b_supported(a);
}

// Split factor of a halo launch of this shape: 0 unless the quarter tiles fill at most a quarter of the CUs (1 .. 4 hypotheses);
// then, from 8 chunks (256 channels) on, as many shares (at most 8; FP_KSPLIT_MAX) as keep >= 2 chunks per share and the grid within the chip.
// (The scratch: shares x M x Cout floats <= 4 x hypotheses x 1600 x 256 for every layer of the networks.)
inline int conv_halo_ksplit(const ConvArgs &a, int num_cu, const ConvKnobs &k) {
  if (!conv_halo_supported(a)) return 0;
  const int n_q = ((a.M + 127) / 128) * (a.Cout / HL_BM), nchunk = a.Cin / HL_CK;
  if (n_q * 4 > num_cu) return 0;
  // from 256 input channels on: with the four chunks of a 128-channel layer two shares + the finishing launch take longer than the one
  // launch (one-hypothesis step 2.17 -> 2.12 ms, four hypotheses 2.74 -> 2.56 without them; FP_KSPLIT_MIN_CHUNKS=0: split those too)
  if (nchunk < k.ksplit_min_chunks) return 0;
  int ks = k.ksplit_max;
  while (ks > 1 && (nchunk % ks != 0 || nchunk / ks < 2 || n_q * ks > num_cu)) ks >>= 1;
  return ks > 1 ? ks : 0;
}

// Split factor of a launch that is offered scratch and does not run the small form (0: none): the 3x3 stride-1 layers by conv_halo_ksplit;
// the 3x3 stride-2 layer from 36 K-steps on when its 64-pixel tiles fill at most a quarter of the workgroup slots (1 .. 4 hypotheses).
inline int conv_ksplit(const ConvArgs &a, int num_cu, const ConvKnobs &k) {
  if (const int ks = conv_halo_ksplit(a, num_cu, k)) return ks;
  const int nk = a.Kpad / C2_BK;
  if (a.KH == 3 && a.KW == 3 && a.stride == 2 && a.out_mode == 0 && a.Cin % 32 == 0 && a.Cout % 128 == 0 && a.M < S2_MIN_PIXELS && nk >= 36 && nk % 4 == 0 &&
      ((a.M + 63) / 64) * (a.Cout / 128) * 4 <= 2 * num_cu)
    return 4;
  return 0;
}

// main/tail split of the implicit GEMM's grid: whole rounds of `slots` main tiles stay; the remainder is cut in four when that shortens
// the last round (a quarter tile costs ~0.35 of a main tile: less operand reuse), i.e. when the remainder fills < ~70 % of a round.
inline void halo_split(int n_tiles, int slots, const ConvKnobs &k, int *n_main, int *n_tail4) {
  const int rem = n_tiles % slots;
  *n_main = n_tiles;
  *n_tail4 = 0;
  if (!k.halo_tail || rem == 0) return;
  if (n_tiles < slots) {
    // less than one round (tracking; a rank's shard of an 8-way job: 32 hypotheses = 100 tiles at C = 512): the launch lasts as
    // long as ONE workgroup, so quarter tiles (4 x the workgroups, ~0.35 x the time each) win as long as they fit two rounds
    if (4 * n_tiles <= 2 * slots) {
      *n_main = 0;
      *n_tail4 = 4 * n_tiles;
    }
    return;
  }
  const double cost_whole = 1.0, cost_quarter = 0.35 * ((4 * rem + slots - 1) / slots);
  if (cost_quarter < cost_whole) {
    *n_main = n_tiles - rem;
    *n_tail4 = 4 * rem;
  }
}

// Tiling of a halo launch (M pixels, n_ct cout tiles of 128, `slots` CUs, one workgroup each): whole rounds of 512-pixel tiles, and what is
// left - less than a round, or the whole of a small launch (a rank's shard of an 8-way job, a tracking frame) - as tiles of nt x 128
// pixels, nt chosen for the shortest finish.  Relative cost of a tile by its nt (measured on one-round launches at C = 512: a round
// of 128-pixel tiles lasts 0.43 of a round of 512-pixel ones - less operand reuse, the same prologue and epilogue).
inline void halo_plan(int M, int n_ct, int slots, const ConvKnobs &k, int *n_main, int *nt_tail, int *n_tail) {
  static const double kHaloTileCost[5] = {0.0, 0.43, 0.62, 0.81, 1.0};
  const int qm = (M + 127) / 128;                       // 128-pixel quarters along the pixel axis
  const int per_round = (slots / n_ct) * 4;             // quarters a round of 512-pixel tiles covers
  int full = per_round > 0 ? qm / per_round : 0;
  int rem = qm - full * per_round;
  *n_main = full * (slots / n_ct) * n_ct;
  *nt_tail = 4;
  *n_tail = 0;
  if (rem == 0) return;
  if (!k.halo_tail) {                                    // FP_HALO_TAIL=0: 512-pixel tiles only
    *n_tail = ((rem + 3) / 4) * n_ct;
    return;
  }
  if (k.halo_nt >= 1 && k.halo_nt <= 4) {
    *nt_tail = k.halo_nt;
    *n_tail = ((rem + k.halo_nt - 1) / k.halo_nt) * n_ct;
    return;
  }
  double best = 1e30;
  for (int nt = 4; nt >= 1; --nt) {
    const int wgs = ((rem + nt - 1) / nt) * n_ct;
    const double cost = ((wgs + slots - 1) / slots) * kHaloTileCost[nt];
    if (cost < best - 1e-9) {
      best = cost;
      *nt_tail = nt;
      *n_tail = wgs;
    }
  }
}

// The networks take split-K scratch from the arena for passes of up to this many hypotheses (the sizes at which a layer is a few workgroups)
#define CONV_NET_SPLITK_MAX_HYP 4

// The packed copies a layer of this shape can ever use (ConvOffer bits): what a network packs when it is loaded, before any map size is
// known.  The s1b copy is for the C -> C layers of 128 and 256 channels, the ones that run on 40x40 maps in the trunks.
inline unsigned conv_packings(int Cin, int Cout, int K, int stride, int Kpad) {
  unsigned p = 0;
  if (K != 3) return p;
  if (small_map_for(Cin, stride) != 0 && Cout % 32 == 0 && Kpad == 9 * Cin) p |= CONV_OFFER_SMALL;
  if (stride == 2 && Cin >= 16 && Cin % 16 == 0 && Kpad >= 9 * Cin && s2_ct_for(Cout) != 0) p |= CONV_OFFER_S2;
  if (stride == 1 && Cin == Cout && (Cout == 128 || Cout == 256) && Kpad == 9 * Cin) p |= CONV_OFFER_S1B;
  return p;
}

struct ConvPlan {
  ConvForm form;
  int ksplit;                      // shares of a split-K form (0: one launch)
  unsigned packing;                // the ConvOffer bit of the packed weights this form reads (0: the [Cout][Kpad] rows)
  size_t splitk_bytes;             // fp32 partial sums [ksplit][M][Cout] of a split-K form
  int n_main, nt_tail, n_tail;     // CONV_HALO: halo_plan's tiling
  const char *cls;                 // profile class (ProfScope) and FLOPs of the launch
  double flops;
};

inline ConvPlan conv_plan(const ConvArgs &a, int num_cu, unsigned offer, const ConvKnobs &k) {
  const bool halo = conv_halo_supported(a);
  ConvPlan p = {};
  p.cls = halo ? "conv3x3_halo" : (a.KW == 3) ? "conv3x3_s2" : (a.KW == 7 ? "conv7x7" : "linear");
  p.flops = 2.0 * (double)a.M * a.Cout * a.KH * a.KW * (a.Cin == 8 ? 6 : a.Cin);
  const auto with = [&p](ConvForm f, unsigned packing) {
    p.form = f, p.packing = packing;
    return p;
  };
  if ((offer & CONV_FORCE_S1B) && s1b_supported(a)) return with(CONV_S1B, CONV_OFFER_S1B);
  if ((offer & CONV_OFFER_SMALL) && conv_small_shape(a, num_cu, k)) return with(CONV_SMALL, CONV_OFFER_SMALL);      // (splits K inside its workgroups)
  if ((offer & CONV_OFFER_S1B) && conv_s1b_use(a, num_cu, k)) return with(CONV_S1B, CONV_OFFER_S1B);
  if (offer & CONV_OFFER_SPLITK) {
    p.ksplit = conv_ksplit(a, num_cu, k);
    p.splitk_bytes = (size_t)p.ksplit * a.M * a.Cout * sizeof(float);
  }
  if (halo) {
    if (p.ksplit > 1) return with(CONV_HALO_SPLITK, 0);
    halo_plan(a.M, a.Cout / HL_BM, num_cu, k, &p.n_main, &p.nt_tail, &p.n_tail);
    return with(CONV_HALO, 0);
  }
  if (p.ksplit > 1) return with(CONV_S2_SPLITK, 0);
  if (stem_supported(a)) return with(CONV_STEM, 0);
  if ((offer & CONV_OFFER_S2) && a.M >= S2_MIN_PIXELS && s2_supported(a)) return with(CONV_S2, CONV_OFFER_S2);
  return with(CONV_IGEMM2, 0);
}

// The form in the vocabulary of tests/tools/conv_ref.py
inline const char *conv_form_name(const ConvPlan &p, const ConvArgs &a) {
  switch (p.form) {
    case CONV_SMALL:
      if (a.stride == 2) return a.Cin == 64 ? "small<1,80,2,4>" : "small<2,40,2>";
      return a.Cin == 128 ? "small<1,40,1>" : a.Cin == 256 ? "small<2,40,1>" : "small<4,20,1>";
    case CONV_S1B: return "s1b";
    case CONV_HALO_SPLITK: return "halo-splitk";
    case CONV_HALO: {
      static const char *const tail[4] = {"halo-tail1", "halo-tail2", "halo-tail3", "halo-tail4"};      // (halo_plan: nt_tail = 1 .. 4)
      return p.n_main > 0 ? "halo-round" : tail[p.nt_tail - 1];
    }
    case CONV_S2_SPLITK: return "s2-splitk";
    case CONV_STEM: return "stem";
    case CONV_S2: return "s2";
    case CONV_IGEMM2: {
      const bool bm128 = a.Cout % 128 == 0;
      if (a.Cin == 8) return bm128 ? "igemm2<128,7,CIN8>" : "igemm2<64,7,CIN8>";
      if (a.KW == 3) return bm128 ? "igemm2<128,3>" : "igemm2<64,3>";
      return bm128 ? "igemm2<128,1>" : "igemm2<64,1>";
    }
  }
  return "?";
}
