// Shared host-side plumbing for libfoundationpose_amd (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <map>

#include "../../include/foundationpose_amd.h"
// The convolutions: ConvArgs, the plan that picks the kernel form of a launch and every shape predicate are in conv_plan.h; the schedule of a
// network pass and the forms of its other stages in pass_plan.h
#include "pass_plan.h"
#include "raster_tri.h"         // the rasteriser's integer rules, LDS / scratch layouts and RenderPlan

#ifndef FP_F16_TYPEDEF
#define FP_F16_TYPEDEF
typedef _Float16 f16;
#endif
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

void fp_set_error(const char *fmt, ...);

// The FP_* environment knobs: every one is read through these two, into a function-local static at its first use,
// i.e. once per process.  fp_env_int: the variable's integer value, `fallback` when it is unset; fp_env_set: whether it is set at
// all, whatever its value (FP_TAIL_SPLIT=0 switches the knob ON).
inline long long fp_env_int(const char *name, long long fallback) {
  const char *e = getenv(name);
  return e ? atoll(e) : fallback;
}
inline bool fp_env_set(const char *name) { return getenv(name) != nullptr; }

#define FP_CHECK_HIP(expr)                                                                   \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      fp_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));     \
      return FP_EHIP;                                                                        \
    }                                                                                        \
  } while (0)

#define FP_REQUIRE(cond, ...)                                                                \
  do {                                                                                       \
    if (!(cond)) {                                                                           \
      fp_set_error(__VA_ARGS__);                                                             \
      return FP_EINVAL;                                                                      \
    }                                                                                        \
  } while (0)

#define FP_TRY(expr)                 \
  do {                               \
    int _rc = (expr);                \
    if (_rc != FP_OK) return _rc;    \
  } while (0)

// The camera matrix as every kernel takes it - fx, fy, cx, cy rounded to fp32.  `fn` names the entry point in the message.
inline int fp_check_camera(const char *fn, const double *K) {
  const float fx = (float)K[0], fy = (float)K[4], cx = (float)K[2], cy = (float)K[5];
  FP_REQUIRE(fx > 0.f && fy > 0.f && isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy),
             "%s: K is not a finite camera matrix with positive focal lengths", fn);
  return FP_OK;
}

// n_views camera-to-object matrices (4 x 4, row-major): finite, with the last row 0 0 0 1
inline int fp_check_view_matrices(const char *fn, const double *cam_in_ob, int n_views) {
  for (int v = 0; v < n_views; ++v) {
    const double *m = cam_in_ob + (size_t)v * 16;
    for (int e = 0; e < 12; ++e) FP_REQUIRE(isfinite(m[e]), "%s: cam_in_ob[%d] is not finite", fn, v);
    FP_REQUIRE(m[12] == 0 && m[13] == 0 && m[14] == 0 && m[15] == 1, "%s: the last row of cam_in_ob[%d] is not 0 0 0 1", fn, v);
  }
  return FP_OK;
}

struct MeshDev {
  const float *pos, *vnormals, *vcolor, *uv, *tex;
  const int32_t *faces, *uv_idx;
  int V, F, texH, texW;
  const int4 *faces4;                   // the face indices as 16-byte records {i0, i1, i2, 0}: one load per face in the rasteriser
};

struct fp_mesh {
  MeshDev d;
  std::vector<void *> allocs;
};

struct ProfEntry {
  double total_ms = 0, flops = 0;
  int64_t launches = 0;
  std::vector<std::pair<float, float>> spans;   // (start, end) of every launch in ms since fp_ctx::ev_ref: launches of one class may overlap (two streams)
};

struct PendingEvent {
  hipEvent_t a, b;
  std::string cls;
  double flops;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// one thread per element
inline dim3 grid_for(long long n, int threads = 256) { return dim3((unsigned)((n + threads - 1) / threads)); }

// Bump arena over one hipMalloc; reset at the start of every forward.
struct Arena {
  char *base = nullptr;
  size_t cap = 0, off = 0;
  int generation = 0;      // bumped whenever the arena is (re)allocated: captured hipGraphs hold its addresses
  void *take(size_t bytes) {
    size_t o = align256(off);
    if (o + bytes > cap) return nullptr;
    off = o + bytes;
    return base + o;
  }
};

// Everything taken inside a scope goes back on every way out of it.  Declared BEFORE a StreamFanout of the same scope: the side streams
// are then joined before the offset they may still be writing behind goes back.
struct ArenaScope {
  Arena &arena;
  const size_t off;
  explicit ArenaScope(Arena &a) : arena(a), off(a.off) {}
  ~ArenaScope() { arena.off = off; }
  ArenaScope(const ArenaScope &) = delete;
  ArenaScope &operator=(const ArenaScope &) = delete;
};

// One device allocation that only grows: what a *_count call leaves in its context for the *_write call (mesh_simplify.hip,
// mesh_components.hip, segment.hip).  A call lays its arrays out with BlobLayout, ensures the total, then takes its pointers with at():
//   BlobLayout l;  const size_t o_a = l.put(a_bytes), o_b = l.put(b_bytes);
//   FP_TRY(blob.ensure(l.bytes, "fp_xxx_count", "the state"));
//   a = blob.at<A>(o_a), b = blob.at<B>(o_b);
// A blob that is large enough is reused as it is, so the arrays of a smaller call lie at other offsets over stale contents: a call
// initialises everything it reads.
struct DevBlob {
  char *base = nullptr;
  size_t cap = 0;
  // at least `bytes` bytes; `fn` and `what` name the caller and the contents in the out-of-memory message
  int ensure(size_t bytes, const char *fn, const char *what) {
    if (bytes <= cap) return FP_OK;
    if (base) FP_CHECK_HIP(hipFree(base));      // synchronises: nothing of an earlier call still runs on it
    base = nullptr, cap = 0;
    if (hipMalloc((void **)&base, bytes) != hipSuccess) {
      (void)hipGetLastError();
      base = nullptr;
      fp_set_error("%s: out of device memory for %s (%zu bytes)", fn, what, bytes);
      return FP_ENOMEM;
    }
    cap = bytes;
    return FP_OK;
  }
  void release() {
    if (base) (void)hipFree(base);
    base = nullptr, cap = 0;
  }
  template <typename T>
  T *at(size_t offset) const { return (T *)(base + offset); }
};

// offsets of consecutive arrays, each at a multiple of 256 bytes; `bytes` is the total so far
struct BlobLayout {
  size_t bytes = 0;
  size_t put(size_t n) {
    const size_t o = bytes;
    bytes = align256(bytes + n);
    return o;
  }
};

struct fp_ctx {
  int device = 0;
  Arena arena;
  int reserved_hyp = 0;
  int prof = 0;            // 0 off, 1 events around the dominant kernel class only (3x3 stride-1 convolutions), 2 around every class
  std::map<std::string, ProfEntry> prof_tab;
  std::vector<PendingEvent> pending;
  std::vector<hipEvent_t> ev_pool;   // recycled timing events: a profiled launch costs two hipEventRecord, no create / destroy
  hipEvent_t ev_ref = nullptr;       // time origin of the launch spans, recorded when profiling is switched on
  int num_cu = 256;
  void *zero_page = nullptr;   // 4 KB of zeros: DMA source for out-of-image taps
  int *tail_counter = nullptr; // FP_TAIL_MAX_GROUPS zeros: arrival counters of the score tail's last launch (left at zero by every call)
  // side streams for the per-object stages (crop window, render, observed crop) of a multi-object pass: with 8 objects
  // x 32 hypotheses a render launch fills a quarter of the chip, so the objects' stages run side by side and join the
  // launch stream before the (single) network pass
  static constexpr int NSIDE = PASS_SIDE_STREAMS;
  hipStream_t side[NSIDE] = {};
  hipEvent_t ev_fork = nullptr, ev_join[NSIDE] = {};
  bool side_ready = false;
  struct fp_simplify_state *simplify = nullptr;   // mesh_simplify.hip: what fp_mesh_simplify_count leaves for fp_mesh_simplify_write
  struct fp_components_state *components = nullptr;   // mesh_components.hip: what fp_mesh_components_count leaves for fp_mesh_components_write
  struct fp_segment_state *segment = nullptr;         // segment.hip: what fp_depth_segment_count leaves for fp_depth_segment_write
  struct fp_stereo_state *stereo = nullptr;           // stereo.hip: the working memory of fp_stereo_sgm
};
void fp_simplify_state_free(fp_ctx *ctx);         // mesh_simplify.hip; fp_ctx_destroy
void fp_components_state_free(fp_ctx *ctx);       // mesh_components.hip; fp_ctx_destroy
void fp_segment_state_free(fp_ctx *ctx);          // segment.hip; fp_ctx_destroy
void fp_stereo_state_free(fp_ctx *ctx);           // stereo.hip; fp_ctx_destroy

// stereo.hip: the host side of fp_stereo_sgm that needs no device - where the arrays of a call lie in the context's blob, and every
// check of a value (`o` receives the options as the call uses them).  scripts/stereo_host_check.cpp runs both under sanitizers.
struct StereoLayout {
  size_t o_grey_l = 0, o_grey_r = 0, o_census_l = 0, o_census_r = 0, o_sum = 0, o_dstar = 0, o_dright = 0, bytes = 0;
};
StereoLayout fp_stereo_layout(int n, int H, int W, int D, int channels);
int fp_stereo_check(const void *ctx, const void *d_left, const void *d_right, int n, int H, int W, int channels, const fp_stereo_opts *opts,
                    const float *d_depth, const fp_stereo_debug *dbg, fp_stereo_opts *o);

// rectify.hip: every check of a value of fp_remap, which needs no device.  scripts/rectify_host_check.cpp runs it under sanitizers.
int fp_remap_check(const void *ctx, const void *d_src0, const void *d_src1, int n, const fp_remap_opts *opts, const void *d_dst0, const void *d_dst1,
                   const fp_remap_debug *dbg);

// reproject.hip: every check of a value of fp_depth_reproject, which needs no device.  scripts/reproject_host_check.cpp runs it under sanitizers.
int fp_depth_reproject_check(const void *ctx, const void *d_depth, int n, int V, int Hs, int Ws, const double *Ks, const double *T_dst_src,
                             const double *K_dst, int Hd, int Wd, float zfar, const void *d_keys, const void *d_depth_out);

// detect.hip: every check of a value of fp_template_match, which needs no device
int fp_template_match_check(const void *ctx, const void *d_depth, int n_frames, int H, int W, const double *K, const void *d_table,
                            const int32_t *ranges, int n_obj, int n_in, int n_out, int anchors, int stride, int r0, int c0, float z_min, float z_max,
                            float zfar, float tol_in, float tol_out, const void *d_keys);

int fp_arena_ensure(fp_ctx *ctx, size_t bytes);
size_t fp_arena_bytes_for(int n_hyp);     // whole refine/score pass (outer buffers + network)
size_t fp_arena_inner_bytes(int n_hyp);   // network forward only

// Fork / join of independent kernel chains onto the context's side streams: the per-object stages of a multi-object pass,
// the two transformer heads of RefineNet.  With fewer than two chains everything stays on the launch stream.
struct StreamFanout {
  fp_ctx *ctx;
  hipStream_t main;
  bool fan;
  bool used[fp_ctx::NSIDE] = {};
  int rc = FP_OK;
  StreamFanout(fp_ctx *c, hipStream_t s, int n_active) : ctx(c), main(s), fan(n_active > 1) {
    if (!fan) return;
    if (!ctx->side_ready) {
      bool ok = hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) == hipSuccess;
      for (int i = 0; ok && i < fp_ctx::NSIDE; ++i)
        ok = hipStreamCreateWithFlags(&ctx->side[i], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&ctx->ev_join[i], hipEventDisableTiming) == hipSuccess;
      if (!ok) {
        fan = false;          // no side streams: run the objects one after the other
        return;
      }
      ctx->side_ready = true;
    }
    if (hipEventRecord(ctx->ev_fork, main) != hipSuccess) fan = false;
  }
  hipStream_t stream_for(int k) {
    if (!fan) return main;
    const int i = k % fp_ctx::NSIDE;
    if (!used[i]) {
      used[i] = true;
      if (hipStreamWaitEvent(ctx->side[i], ctx->ev_fork, 0) != hipSuccess) rc = FP_EHIP;
    }
    return ctx->side[i];
  }
  int join() {
    if (fan)
      for (int i = 0; i < fp_ctx::NSIDE; ++i)
        if (used[i]) {
          if (hipEventRecord(ctx->ev_join[i], ctx->side[i]) != hipSuccess || hipStreamWaitEvent(main, ctx->ev_join[i], 0) != hipSuccess) rc = FP_EHIP;
          used[i] = false;
        }
    if (rc != FP_OK) fp_set_error("stream fork/join failed");
    return rc;
  }
  // every way out of a scope that forked - an early FP_REQUIRE / FP_TRY return included - joins the side streams before the caller
  // resets the arena they may still be writing (join() is idempotent: a joined fan-out has no used stream left)
  ~StreamFanout() { (void)join(); }
  StreamFanout(const StreamFanout &) = delete;
  StreamFanout &operator=(const StreamFanout &) = delete;
};


// net.hip: the network passes with the two sides of encodeA as two chains (`ab` forked by the caller: side B's input is produced on
// ab->stream_for(0), side A's on `s`; nullptr: one chain); batches below trunk_split_min() hypotheses only (larger ones are cut in two by hypotheses)
struct fp_net;
struct RefineTailArgs;
// `tail` (optional; pose / window fields filled by the caller, head fields by the forward pass): the heads' token means, the pose update
// and the next crop windows as ONE launch behind the join of the heads (refine_tail_kernel) instead of two mean_head launches here
// `sb` (optional): side B of this pass is ONE observed crop per object - every hypothesis of an object has the same crop window (the first
// iteration of a registration: the rotation grid around one guessed centre, src/estimater.py:126-135) - already encoded by fp_encode_side_b
// (on ab->stream_for(0) when `ab` is given): encodeA runs on side A only and the objects' features are copied into the B half of the channel
// concat.  Same kernels on the same inputs as the batch: the tokens are those of the plain pass bit for bit.
struct SharedB {
  const f16 *feat;          // [n_groups][40 x 40][128] fp16: encodeA of each object's observed crop
  int n_groups;
  int start[9];             // hypothesis at which object g starts; start[n_groups] = N
};
int fp_encode_side_b(fp_ctx *ctx, const fp_net *net, const f16 *xB, int n_groups, int hyp, f16 *feat, hipStream_t s);
int fp_refine_forward_ab(fp_ctx *ctx, const fp_net *net, const void *d_net_in, int N, float *d_trans, float *d_rot, hipStream_t s, StreamFanout *ab,
                         RefineTailArgs *tail = nullptr, const SharedB *sb = nullptr);
int fp_score_features_ab(fp_ctx *ctx, const fp_net *net, const void *d_net_in, int N, float *d_feats, hipStream_t s, StreamFanout *ab, int feat_ld = 512,
                         const float *d_poses = nullptr);      // feat_ld / d_poses: [feature | pose] rows of the all-gather (score_tail.hip)

// profiling hooks (events on the launch stream)
struct ProfScope {
  fp_ctx *ctx;
  hipStream_t s;
  PendingEvent ev;
  bool on;
  ProfScope(fp_ctx *c, hipStream_t st, const char *cls, double flops)
      : ctx(c), s(st), on(c && (c->prof == 2 || (c->prof == 1 && strcmp(cls, "conv3x3_halo") == 0))) {
    if (on) {
      ev.a = take_event();
      ev.b = take_event();
      ev.cls = cls;
      ev.flops = flops;
      (void)hipEventRecord(ev.a, s);
    }
  }
  hipEvent_t take_event() {
    hipEvent_t e = nullptr;
    if (!ctx->ev_pool.empty()) {
      e = ctx->ev_pool.back();
      ctx->ev_pool.pop_back();
    } else {
      (void)hipEventCreate(&e);
    }
    return e;
  }
  ~ProfScope() {
    if (on) {
      (void)hipEventRecord(ev.b, s);
      ctx->pending.push_back(ev);
    }
  }
};

// XCD-aware tile order (MI355X: 8 XCDs with private L2s, workgroups dealt round-robin): workgroup `id` of `nwg`
// gets logical tile index L such that each XCD walks a CONTIGUOUS range of L; neighbouring tiles (which share
// halo rows / the same pixels for another cout tile) then hit the same L2.  Bijective for any nwg.  Speed only.
#ifdef __HIPCC__
__device__ __forceinline__ int xcd_remap(int id, int nwg) {
  const int xcd = id & 7, slot = id >> 3;
  const int q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}
#endif

// Kernels that need more dynamic LDS than the 64-KB default carry hipFuncAttributeMaxDynamicSharedMemorySize.  The attribute belongs to
// the function ON ONE DEVICE, so it is set for every such kernel of the library when a context is created on its device
// (fp_ctx_create -> fp_set_kernel_attributes), not lazily behind process-wide flags: a second device in one process, a graph capture
// and concurrent first launches from two threads all find the attributes in place.  Each .hip file lists its own kernels.
struct KernelLds {
  const void *fn;
  int bytes;
};
void conv_kernel_lds(std::vector<KernelLds> &v);        // conv.hip
void conv_halo_kernel_lds(std::vector<KernelLds> &v);   // conv_halo.hip
void conv_s1b_kernel_lds(std::vector<KernelLds> &v);    // conv_s1b.hip
void conv_small_kernel_lds(std::vector<KernelLds> &v);  // conv_small.hip
void conv_s2_kernel_lds(std::vector<KernelLds> &v);     // conv_s2.hip
void stem_kernel_lds(std::vector<KernelLds> &v);        // stem.hip
void front_kernel_lds(std::vector<KernelLds> &v);       // front.hip
void tok_gemm_kernel_lds(std::vector<KernelLds> &v);    // tok_gemm.hip
void tok_qkv_kernel_lds(std::vector<KernelLds> &v);     // tok_qkv.hip
void head_mlp_kernel_lds(std::vector<KernelLds> &v);    // head_mlp.hip
void attn_kernel_lds(std::vector<KernelLds> &v);        // attn.hip
void raster_kernel_lds(std::vector<KernelLds> &v);      // raster.hip
int fp_set_kernel_attributes(fp_ctx *ctx);              // api.hip: all of the above on ctx->device

// ---- kernel launchers implemented in the .hip files ----
int launch_conv(fp_ctx *ctx, const ConvArgs &a, hipStream_t s);      // conv.hip: offer from a.wsm / a.wpk / a.splitk, conv_plan, launch
// the per-form launchers, next to their kernels; each checks that the layer is one its kernel runs
int launch_conv_small(fp_ctx *ctx, const ConvArgs &a, hipStream_t s);                          // conv_small.hip
int launch_conv_s1b(fp_ctx *ctx, const ConvArgs &a, hipStream_t s);                            // conv_s1b.hip
int launch_conv_halo(const ConvArgs &a, const ConvPlan &plan, hipStream_t s);                  // conv_halo.hip: the plan's tiling, or a.ksplit shares + the finishing pass
int launch_splitk_finish(const ConvArgs &a, hipStream_t s);                                    // conv_halo.hip: adds the shares in order (also behind conv.hip's stride-2 split-K)
int launch_stem(fp_ctx *ctx, const ConvArgs &a, hipStream_t s);                                // stem.hip
int launch_conv_s2(fp_ctx *ctx, const ConvArgs &a, hipStream_t s);                             // conv_s2.hip
// front.hip: the 7x7 stem and the 64 -> 128 stride-2 layer of encodeA as one launch, x [n][160][160][8] -> a1 [n][40][40][128]; bit-identical
// to launch_stem + the implicit GEMM.  wst: the stem's weights by front_pack_stem (front_packed_stem_halfs() halfs); wpk: the stride-2 layer's
// by s2_pack_weights (order 0); a0_dbg (optional, tests): receives the stem's output [n][80][80][64] as the kernel's tiles hold it
int launch_front(fp_ctx *ctx, const f16 *x, int n, const f16 *wst, const float *b0, const f16 *wpk, const float *b1, f16 *a1, f16 *a0_dbg, hipStream_t s);
size_t front_packed_stem_halfs();
int front_pack_stem(const f16 *d_w, int Kpad, f16 *d_out, hipStream_t s);
// packed copies of a layer's [Cout][Kpad] weights
size_t s2_packed_halfs(int Cout, int Cin);
int s2_pack_weights(const f16 *d_w, int Cout, int Cin, int Kpad, f16 *d_out, hipStream_t s, int ct_force = 0, int order = 0);   // ct_force: co tiles of 32 per wave group (0: s2_ct_for); order 1: conv_s1b.hip
size_t small_packed_halfs(int Cout, int Cin);
int small_pack_weights(const f16 *d_w, int Cout, int Cin, int Kpad, f16 *d_out, hipStream_t s);
// conv.hip: the copy `packing` (one ConvOffer bit) names - its size, and the launch that writes it
size_t conv_packed_halfs(unsigned packing, int Cout, int Cin);
int conv_pack_weights(unsigned packing, const f16 *d_w, int Cout, int Cin, int Kpad, f16 *d_out, hipStream_t s);

// attn.hip (the transposed V image [b][4][128][416] and its token order vt_col(): tok_tile.h; the kernels' layouts: attn_tile.h)
int launch_attention(fp_ctx *ctx, const f16 *qk, const f16 *vt, int B, int T, f16 *out, hipStream_t s);

// Token GEMM (tok_gemm.hip): out = x (M x 512) @ W^T + b for up to TG_MAXBLK blocks of 512 output columns in one launch.
#define TG_MAXBLK 6
struct TokGemmBlock {
  const f16 *w;        // 512 x 512 weights in MFMA-fragment order (pack_tok_weights)
  const float *bias;   // 512
  void *out;           // fp16 rows (EPI_ROWS / EPI_LN) or the transposed V image (EPI_VT)
  int ld, coff;        // row stride / column offset of this block in `out` (halfs)
  int relu;
  int vt = 0;          // tok_qkv.hip: 1 = `out` is the transposed V image (tok_gemm.hip takes this from its epilogue argument)
};
struct TokGemmArgs {
  const f16 *in;       // [M][512] fp16
  int M, nblk, tokens; // tokens per hypothesis (EPI_VT, EPI_LNSUM)
  TokGemmBlock blk[TG_MAXBLK];
  const f16 *res;      // [M][512] residual (EPI_LN, EPI_LNSUM)
  const float *gamma, *beta;
  float *gsum;         // EPI_LNSUM: [M/16][512] sums of the normalised rows over groups of 16 tokens
};
enum { TG_EPI_ROWS = 0, TG_EPI_VT = 1, TG_EPI_LN = 2, TG_EPI_LNSUM = 3 };
int launch_tok_gemm(fp_ctx *ctx, const TokGemmArgs &a, int epi, hipStream_t s);
// the argument checks launch_tok_gemm and launch_tok_qkv share (tok_gemm.hip): pointers, block count, the 32-bit lane-offset limit and per
// block the conditions of its output - `out`: what the blocks write, TOK_OUT_BLK = each block's own `vt`; coff_align: of rows / V image blocks
enum { TOK_OUT_NONE, TOK_OUT_ROWS, TOK_OUT_VT, TOK_OUT_BLK };
int tok_check_args(const char *who, const TokGemmArgs &a, int out, int coff_align);
// tok_qkv.hip: the in-projections - all blocks over a resident 128-token tile (fp16 rows or the transposed V image per block)
int launch_tok_qkv(fp_ctx *ctx, const TokGemmArgs &a, hipStream_t s, int hyp = 0);      // hyp: images of the forward body (qkv_form: 1 .. 2 tok_qkv_small_kernel; 0: a stand-alone call)
// head_mlp.hip: out-projection + LayerNorm1 + linear1 + ReLU + linear2 + LayerNorm2 statistics of one transformer head in one launch
struct HeadMlpArgs {
  const f16 *att, *tok;        // [M][512]: attention output, residual tokens
  int M;
  const f16 *w_out, *w1, *w2;  // 512 x 512 in MFMA-fragment order (pack_tok_weights)
  const float *b_out, *b1, *b2, *g1, *be1;
  float *gsum;                 // [M/16][512] sums of the LayerNorm2-normalised rows over groups of 16 tokens
};
int launch_head_mlp(fp_ctx *ctx, const HeadMlpArgs &a, hipStream_t s);
// refine_tail.hip: sum of `nparts` consecutive partial rows per hypothesis (fixed order) / T, gamma, beta, Linear(512 -> out_dim)
int launch_mean_head(const float *partial, int nparts, const float *g, const float *b, int Bn, int T, const float *hw, const float *hb,
                     int out_dim, float *out, hipStream_t s);
// score_tail.hip: token mean + att.out_proj of ScoreNet in one launch; att_cross + linear + argmax in two
int launch_score_feat(const f16 *att, int Bn, int T, const float *wt, const float *bias, float *out, int ld, const float *poses, hipStream_t s);
struct ScoreTailOut {
  float *logits = nullptr;             // (groups, L), required
  int32_t *argmax = nullptr;           // (groups), optional
  float *scores = nullptr;             // (groups, L) = logits + score_offset, optional (ScorePredictor.predict: + 100, predict_score.py:209)
  float score_offset = 0.f;
  // optional, with argmax (tracking): the winning hypothesis' pose (group g: poses + g L 16) -> best_pose (groups, 16) and
  // best_pose @ get_tf_to_centered_mesh() -> best_centered (groups, 16)
  const float *poses = nullptr;
  float *best_pose = nullptr, *best_centered = nullptr;
  float cneg[3] = {0.f, 0.f, 0.f};
};
int launch_score_tail(const float *feats, int feat_ld, const float *wqk_t, const float *bqk, const double *u, const double *c, double b_eff, int groups, int L,
                      float *qk, double *sv, int *counter, const ScoreTailOut &o, hipStream_t s);
#define FP_TAIL_MAX_GROUPS 4096
int fp_score_tail_impl(fp_ctx *ctx, const fp_net *net, const float *d_feats, int feat_ld, int groups, int L, const ScoreTailOut &o, hipStream_t s);      // net.hip
// trans_tanh: 0 raw, 1 tanh * trans_normalizer, 2 trans_rep='deepim' (needs tf N x 9, K, resize = input_resize[0])
// The tail of a refinement pass as one launch (refine_tail.hip: refine_tail_kernel): both heads' token mean + output Linear, the pose update in
// place and, with `next_window`, the crop windows of the next iteration (tf / bbox overwritten; the deepim branch reads tf first)
struct CropWindowK {             // intrinsics as float, radius = diameter * crop_ratio / 2, output size (crop_window_tf_one, pose_math.h)
  float k00, k01, k02, k10, k11, k12, k20, k21, k22, radius, ow, oh;
};
CropWindowK crop_window_k(const double *K, double crop_ratio, double diameter, int ow, int oh);
// A pass of fp_track_objects: hypothesis b is object b.  What differs between the objects, per hypothesis (the rest of the tail is shared)
struct RefineTailObjs {
  int n = 0;                                      // 0: not such a pass (the scalar fields of RefineTailArgs hold for every hypothesis)
  float trans_scale[FP_TRACK_MAX_OBJECTS], radius[FP_TRACK_MAX_OBJECTS], cneg[FP_TRACK_MAX_OBJECTS][3];
  float *centered[FP_TRACK_MAX_OBJECTS];          // the object's pose @ get_tf_to_centered_mesh() (nullptr: not written)
  float *pose_out[FP_TRACK_MAX_OBJECTS];          // the object's own pose buffer, which receives the updated pose (nullptr: not written)
};
struct RefineTailArgs {
  const float *partial[2], *gam[2], *bet[2], *hw[2], *hb[2];      // per head: group sums of linear2's LayerNorm rows, ln2 gamma / beta, head Linear
  int nparts, T, rot_dim;
  float *trans, *rot;            // (N,3), (N,rot_dim): the heads' outputs (API outputs of the pass)
  float *poses;                  // (N,4,4) updated in place
  int trans_tanh;
  float tn0, tn1, tn2, rot_normalizer, trans_scale;
  float K[9], resize;            // deepim
  float *tf, *bbox;              // (N,9), (N,4)
  int next_window;
  CropWindowK win;
  // optional (the last pass of a tracking frame): pose @ get_tf_to_centered_mesh() of every hypothesis, (N,4,4) - src/estimater.py:268;
  // cneg = -model_center (the translation column of that matrix)
  float *centered = nullptr;
  float cneg[3] = {0.f, 0.f, 0.f};
  RefineTailObjs obj;            // fp_track_objects: per-object trans_scale, window radius, cneg, centered and pose copy (obj.n = N)
};
int launch_refine_tail(const RefineTailArgs &a, int N, hipStream_t s);
int launch_pose_update(const float *poseA, const float *trans, const float *rot, int N, int rot_dim, int trans_tanh,
                       float tn0, float tn1, float tn2, float rot_normalizer, float trans_scale, float *out, hipStream_t s,
                       const float *tf = nullptr, const double *K = nullptr, float resize = 160.f);

struct RenderArgs {
  MeshDev mesh;
  const float *poses, *bbox2d;
  double K[9];
  int N, H, W, Ho, Wo;
  int use_light;
  float w_ambient, w_diffuse;
  float *color, *depth, *normal, *xyz;  // mode 0
  float *rast = nullptr;                // mode 0, optional: dr.rasterize's output per pixel (u, v, z/w, triangle id + 1) - src/Utils.py:182; parity tests
  f16 *net_out;                         // mode 1
  float mesh_diameter, invalid_thres;
  int normalize_xyz;
  void *scratch = nullptr;              // render_plan(...).total bytes: the per-(hypothesis, vertex) records of the pre-pass (required)
  size_t scratch_bytes = 0;
  int dbg = 0;                          // FP_RENDER_DBG (timing experiments: phases switched off)
  // non-default lighting / projection of nvdiffrast_render (src/Utils.py:159-162,200-211)
  int light_mode = 0;                   // 0: light_dir = (0,0,1), the default; 1: direction light_vec = -light_dir; 2: point light at light_vec (light_dir=None)
  float light_vec[3] = {0.f, 0.f, -1.f};
  int has_light_color = 0;              // 0: the diffuse term takes the surface colour (light_color=None)
  float light_color[3] = {1.f, 1.f, 1.f};
  int has_proj = 0;                     // 1: proj replaces projection_matrix_from_intrinsics(K, H, W, 0.001, 100)
  double proj[16] = {0};
};
RenderPlan render_plan(int N, int V, int F, int Ho, int Wo, int num_cu);
// A render of N hypotheses goes out in sub-batches of render_chunk(...) when the worst-case scratch of all N at once (two face lists of
// every face in every strip: N * S * F * 8 B) would exceed 1 GiB (FP_RENDER_SCRATCH_MAX; tests lower it): the sub-batches run behind
// each other on the stream, over ONE scratch of render_scratch_bytes(...), with one plan (strips, face ranges) for all of them.
int render_chunk(int N, int V, int F, int Ho, int Wo, int num_cu);
size_t render_scratch_bytes(int N, int V, int F, int Ho, int Wo, int num_cu);
int launch_render(fp_ctx *ctx, const RenderArgs &a, hipStream_t s);      // a.scratch: render_scratch_bytes(a.N, ...) bytes
bool render_fits(int N, int V, int F, int Ho, int Wo, int num_cu);       // launch_render takes this output size (strips per hypothesis, pixels per strip)
int launch_crop_window_tf(const float *poses, int N, const double *K, double crop_ratio, double diameter, int ow, int oh, float *tf,
                          float *bbox, hipStream_t s);
// fp_track_objects (hypothesis b = object b, n <= FP_TRACK_MAX_OBJECTS): several objects' one-launch renders (render_kernel<1, true>) as
// ONE launch; a.mesh / a.mesh_diameter are replaced by each object's, the other fields are shared.  Every object must take the one-launch
// form (render_objects_form); each image is the one render_kernel<1, true> makes of that object alone.  `hyp`: the object's hypothesis.
bool render_objects_form(int V, int F, int Ho, int Wo, int num_cu);      // a mesh launch_render_objects takes (else: launch_render, on its own)
int launch_render_objects(fp_ctx *ctx, const RenderArgs &a, const MeshDev *const *mesh, const float *diameter, const int *hyp, int n, hipStream_t s);
// the first crop windows of such a pass: object b's pose is first copied from pose_in[b] to poses + 16 b; radius from diameter[b]
int launch_crop_window_objects(const float *const *pose_in, const double *K, double crop_ratio, const double *diameter, int n, int ow, int oh,
                               float *poses, float *tf, float *bbox, hipStream_t s);

struct CropArgs {
  const float *rgb, *geom, *tf, *poses;
  double K[9];
  int H, W, N, Ho, Wo, mode, normalize_xyz, out_fmt;
  float mesh_diameter;
  void *out;
};
int launch_crop_observed(const CropArgs &a, hipStream_t s);
// the same with hypothesis b's mesh diameter from diameter[b] (a.N <= FP_TRACK_MAX_OBJECTS; fp_track_objects) instead of a.mesh_diameter
int launch_crop_observed_objects(const CropArgs &a, const float *diameter, hipStream_t s);
int launch_warp_nearest(const float *src, int src_batch, int Hs, int Ws, int C, const float *tf, int N, int Ho, int Wo, float *out,
                        hipStream_t s);

int launch_erode(const float *d, int H, int W, int radius, float diff_thres, float ratio_thres, float zfar, float *out, hipStream_t s);
int launch_bilateral(const float *d, int H, int W, int radius, float zfar, float sigmaD, float sigmaR, float *out, hipStream_t s);
int launch_depth2xyz(const float *d, int H, int W, const double *K, float zfar, float *xyz, hipStream_t s);
int launch_depth_prefilter(const float *d, int H, int W, float diff_thres, float ratio_thres, float zfar_e, float zfar_b, float sigmaD,
                           float sigmaR, const double *K, float zfar_x, float *out, float *xyz, const unsigned char *rgb_u8, float *rgb_f, hipStream_t s);
int launch_depth2xyz_f64(const float *d, int H, int W, const double *K, float *xyz, hipStream_t s);
int launch_mask_depth_stats(const float *d, const unsigned char *mask, int H, int W, float min_depth, int *out6, float *median, hipStream_t s);
// register.hip: the kernels around the networks of fp_register_objects (n <= FP_TRACK_MAX_OBJECTS objects of one frame)
struct MaskStatsObjs {           // object o: mask[o] (H*W bytes, non-zero = object) or, with `labels` (H*W int32), the pixels equal to label[o]
  const unsigned char *mask[FP_TRACK_MAX_OBJECTS];
  int label[FP_TRACK_MAX_OBJECTS];
  const int *labels;
  int n;
};
// every object's mask_depth_stats in ONE launch: out8 + 8 o = cmin, cmax, rmin, rmax, n_mask, n_usable, median (float bits), 0
int launch_mask_depth_stats_objects(const float *d, const MaskStatsObjs &ob, int H, int W, float min_depth, int *out8, hipStream_t s);
struct RegHypObjs {              // object o: n[o] rotations at rot_grid[o], written to poses + 16 off[o] with the translation guessed from its mask
  const float *rot_grid[FP_TRACK_MAX_OBJECTS];
  int n[FP_TRACK_MAX_OBJECTS], off[FP_TRACK_MAX_OBJECTS];
  int cmin[FP_TRACK_MAX_OBJECTS], cmax[FP_TRACK_MAX_OBJECTS], rmin[FP_TRACK_MAX_OBJECTS], rmax[FP_TRACK_MAX_OBJECTS];
  float median[FP_TRACK_MAX_OBJECTS];
  double kinv[9];                // np.linalg.inv(K), row-major
  int n_obj;
};
int launch_register_hypotheses(const RegHypObjs &ob, float *poses, hipStream_t s);
struct RegRankObjs {             // object o: its n[o] refined poses / scores at off[o], ranked best first into its own buffers
  int n[FP_TRACK_MAX_OBJECTS], off[FP_TRACK_MAX_OBJECTS];
  float *poses_out[FP_TRACK_MAX_OBJECTS], *scores_out[FP_TRACK_MAX_OBJECTS], *pose_of_mesh[FP_TRACK_MAX_OBJECTS];
  long long *order_out[FP_TRACK_MAX_OBJECTS];
  float cneg[FP_TRACK_MAX_OBJECTS][3];
  int n_obj;
};
int launch_register_rank(const RegRankObjs &ob, const float *poses, const float *scores, hipStream_t s);
// metrics.hip: ADD / ADD-S / ADDsym of n_poses poses (fp_pose_errors); `slab` holds pose_errors_slab_bytes(...) bytes of partial sums
size_t pose_errors_slab_bytes(int n_pts, int n_poses, int n_sym);
int launch_pose_errors(const float *pts, int n_pts, const float *pred, const float *gt, int gt_per_pose, int n_poses, const float *sym,
                       int n_sym, int which, double *slab, float *add, float *adds, float *add_sym, hipStream_t s);
// mesh.hip: exact diameter of n_pts points and the pair that spans it (fp_mesh_diameter); `slab` holds mesh_diameter_slab_bytes(n_pts)
// bytes of per-workgroup candidates
size_t mesh_diameter_slab_bytes(int n_pts);
int launch_mesh_diameter(const float *pts, int n_pts, void *slab, float *out, int32_t *pair, hipStream_t s);
// bounds.hip: the boxes of n points in C frames and the smallest of them (fp_box_extents); `slab` holds box_extents_slab_bytes(n, C)
// bytes: the bounds per (point slice, candidate) and the per-workgroup winners
size_t box_extents_slab_bytes(int n, int C);
int launch_box_extents(const float *pts, int n, const float *frames, int C, void *slab, int32_t *out_index, float *out_lohi, float *out_vol,
                       float *all_lohi, float *all_vol, hipStream_t s);
// scan.hip: in-place exclusive scan of n 64-bit words (reduce, scan of the block sums, add: a workgroup never waits for another one);
// `sums` holds scan_sums_words(n) words for the block sums of every level
size_t scan_sums_words(long long n);
int scan_exclusive(unsigned long long *data, long long n, unsigned long long *sums, hipStream_t s);
// metrics.hip: MSSD / MSPD of n_poses poses (fp_pose_errors_bop); `slab` holds bop_errors_slab_bytes(...) bytes of tile maxima
size_t bop_errors_slab_bytes(int n_pts, int n_poses, int n_sym);
int launch_bop_errors(const float *pts, int n_pts, const float *pred, const float *gt, int gt_per_pose, int n_poses, const float *sym,
                      int n_sym, const double *K, int which, float *slab, float *mssd, float *mspd, hipStream_t s);
// metrics.hip: the VSD counts of n_poses depth renders (fp_vsd): pose b's images at dt + b * dt_stride, dg + b * dg_stride, de + b * H * W;
// adds into counts[b][2 + FP_VSD_MAX_TAUS]; launch_vsd_finish turns the counts into errors (and int32 counts, if counts_out)
int launch_vsd_count(const float *dt, size_t dt_stride, const float *dg, size_t dg_stride, const float *de, int n_poses, int H, int W,
                     const double *K, double diameter, double delta, const double *taus, int n_taus, unsigned *counts, hipStream_t s);
int launch_vsd_finish(const unsigned *counts, int n_poses, int n_taus, float *err, int *counts_out, hipStream_t s);
// scene.hip: one pass over the depth layers of a chunk of instances (fp_scene_instances): loop A (do_min) keeps the smallest positive
// depth and its instance per frame pixel in dmin / owner (read first unless `first`), loop B (do_masks) writes the chunk's masks and adds
// its counts and boxes into acc (n_inst x FP_SCENE_INFO_COLS of the whole call: launch_scene_info_init before the first chunk,
// launch_scene_info_finish after the last).  With occ_inst and do_masks but not do_min, dmin holds the finished minimum.
struct SceneLaunch {
  const float *layers, *dt;
  int n, i0, H, W, pad_x, pad_y;
  int do_min, do_masks, first, occ_depth, occ_inst;
  const double *K;
  double delta;
  float *dmin;
  int32_t *owner;
  uint8_t *mask, *mask_visib;
  int *acc;
};
int launch_scene_instances(fp_ctx *ctx, const SceneLaunch &l, hipStream_t s);
int launch_scene_info_init(int *acc, int n_inst, hipStream_t s);
int launch_scene_info_finish(const int *acc, int n_inst, int32_t *info, hipStream_t s);
