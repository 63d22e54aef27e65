// Depth from a rectified stereo pair: semi-global matching on census costs (fp_stereo_sgm).  The rule is stated in
// include/foundationpose_amd.h and restated in numpy by tests/stereo_oracle.py; everything up to the winning disparity is integer, so
// this file has to match it bit for bit, and does so on every run and in any batch.
//
//   * stereo_grey_kernel, stereo_census_kernel: one thread per pixel of both images.
//   * sgm_path_kernel<K>: one launch per selected direction.  One WAVE walks one path line (a row, a column, or a diagonal from its
//     entry pixel), one pixel per step, with the D = 64 K disparities on its lanes: lane l holds d = l K .. l K + K - 1, so d - 1 and
//     d + 1 are in the lane itself or one __shfl_up / __shfl_down away, and m_q is device_util.h's wave_min.  The cost is formed here
//     from the two census images (8 bytes a pixel); there is no cost volume.  S is laid out (pixel, d) with d fastest: a wave touches
//     128 K contiguous bytes per pixel whatever the direction.  The first selected direction WRITES S, the others add to it: the sum
//     is integer, its order does not change the bits, and within one launch a cell belongs to exactly one wave - no atomics, and
//     nothing of S is read before this call wrote it.  The loads of the next pixel (census, S) are issued before the recurrence of
//     the current one: they do not depend on it.
//   * sgm_scan_kernel<K>: one wave per image row reads S once, in order.  d* is a wave_min over (S << 8 | d).  d_R(y,x) minimises over
//     the anti-diagonal S(y, x + d, d): the running minimum of right pixel x = p - d sits in disparity slot d when the wave is at left
//     pixel p, so the K slots of every lane move up by one slot per step (one __shfl_up) and the slot that reaches d = D - 1 is final.
//   * stereo_final_kernel: one thread per pixel: the three validity tests, the parabola, fb / disparity.
//   * stereo_cost_kernel: the debug output C only.
// Working memory is one grow-only DevBlob in the context; one chain of launches on the caller's stream, no synchronisation, no host
// copy: after a first call of a size the call can sit in a captured graph.
#include "common.h"
#include "device_util.h"

typedef unsigned long long u64;

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_BIG = 1 << 24;      // above any L_r + P2 and any (S << 8 | d)

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// (n,H,W,3) uint8 -> (n,H,W) uint8, both images: i < total is the left one
__global__ __launch_bounds__(ST_THREADS) void stereo_grey_kernel(const uint8_t *__restrict__ left, const uint8_t *__restrict__ right, long long total,
                                                                 uint8_t *__restrict__ gl, uint8_t *__restrict__ gr) {
  const long long i = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (i >= 2 * total) return;
  const bool r = i >= total;
  const long long p = r ? i - total : i;
  const uint8_t *s = (r ? right : left) + (size_t)p * 3;
  (r ? gr : gl)[p] = (uint8_t)((77u * s[0] + 150u * s[1] + 29u * s[2] + 128u) >> 8);
}

__global__ __launch_bounds__(ST_THREADS) void stereo_census_kernel(const uint8_t *__restrict__ gl, const uint8_t *__restrict__ gr, long long total, int H,
                                                                   int W, u64 *__restrict__ cl, u64 *__restrict__ cr) {
  const long long i = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (i >= 2 * total) return;
  const bool r = i >= total;
  const long long p = r ? i - total : i;
  const long long hw = (long long)H * W;
  const long long v = p / hw;
  const int pix = (int)(p - v * hw), y = pix / W, x = pix - y * W;
  const uint8_t *g = (r ? gr : gl) + (size_t)v * (size_t)hw;
  const unsigned c = g[pix];
  u64 code = 0;
#pragma unroll
  for (int dy = -3; dy <= 3; ++dy) {
    const uint8_t *row = g + (size_t)clampi(y + dy, H - 1) * W;
#pragma unroll
    for (int dx = -4; dx <= 4; ++dx) {
      if (dy == 0 && dx == 0) continue;
      code = (code << 1) | (u64)(row[clampi(x + dx, W - 1)] < c ? 1 : 0);
    }
  }
  (r ? cr : cl)[p] = code;
}

// debug only: C (n,H,W,D) uint8, one thread per cell
__global__ __launch_bounds__(ST_THREADS) void stereo_cost_kernel(const u64 *__restrict__ cl, const u64 *__restrict__ cr, long long cells, int W, int D,
                                                                 uint8_t *__restrict__ C) {
  const long long i = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (i >= cells) return;
  const long long p = i / D;
  const int d = (int)(i - p * D), x = (int)(p % W);
  C[i] = x - d >= 0 ? (uint8_t)__popcll(cl[p] ^ cr[p - d]) : (uint8_t)64;
}

// K consecutive uint16 of S as one register value
template <int K>
struct SVec;
template <>
struct SVec<1> {
  typedef unsigned short T;
  static __device__ __forceinline__ void unpack(T v, int (&o)[1]) { o[0] = v; }
  static __device__ __forceinline__ T pack(const int (&o)[1]) { return (T)o[0]; }
};
template <>
struct SVec<2> {
  typedef unsigned int T;
  static __device__ __forceinline__ void unpack(T v, int (&o)[2]) { o[0] = (int)(v & 0xffffu), o[1] = (int)(v >> 16); }
  static __device__ __forceinline__ T pack(const int (&o)[2]) { return (unsigned)o[0] | ((unsigned)o[1] << 16); }
};
struct us3 {
  unsigned short a, b, c;
};
template <>
struct SVec<3> {      // D = 192: 6 bytes a lane, 2-byte aligned
  typedef us3 T;
  static __device__ __forceinline__ void unpack(T v, int (&o)[3]) { o[0] = v.a, o[1] = v.b, o[2] = v.c; }
  static __device__ __forceinline__ T pack(const int (&o)[3]) { return us3{(unsigned short)o[0], (unsigned short)o[1], (unsigned short)o[2]}; }
};
template <>
struct SVec<4> {
  typedef uint2 T;
  static __device__ __forceinline__ void unpack(T v, int (&o)[4]) {
    o[0] = (int)(v.x & 0xffffu), o[1] = (int)(v.x >> 16), o[2] = (int)(v.y & 0xffffu), o[3] = (int)(v.y >> 16);
  }
  static __device__ __forceinline__ T pack(const int (&o)[4]) {
    return make_uint2((unsigned)o[0] | ((unsigned)o[1] << 16), (unsigned)o[2] | ((unsigned)o[3] << 16));
  }
};

template <int K>
__device__ __forceinline__ void sgm_cost(const u64 *__restrict__ cl, const u64 *__restrict__ cr, size_t p, int x, int d0, int (&C)[K]) {
  const u64 c = cl[p];
#pragma unroll
  for (int k = 0; k < K; ++k) C[k] = x - (d0 + k) >= 0 ? __popcll(c ^ cr[p - (size_t)(d0 + k)]) : 64;
}

// blockIdx.x * 4 + wave = the path line, blockIdx.y = the pair.  Lines of direction (dy, dx): the H rows, the W columns, or for a
// diagonal the W pixels of the entry row followed by the other H - 1 pixels of the entry column.
template <int K>
__global__ __launch_bounds__(ST_THREADS) void sgm_path_kernel(const u64 *__restrict__ cl, const u64 *__restrict__ cr, uint16_t *__restrict__ S, int H, int W,
                                                              int dy, int dx, int lines, int P1, int P2, int first) {
  typedef typename SVec<K>::T V;
  const int lane = threadIdx.x & 63, d0 = lane * K;
  const int line = blockIdx.x * (ST_THREADS / 64) + (threadIdx.x >> 6);
  if (line >= lines) return;      // the whole wave
  const size_t img = (size_t)blockIdx.y * (size_t)H * (size_t)W;
  int y, x;
  if (dy == 0) y = line, x = dx > 0 ? 0 : W - 1;
  else if (dx == 0) x = line, y = dy > 0 ? 0 : H - 1;
  else if (line < W) x = line, y = dy > 0 ? 0 : H - 1;
  else {
    const int j = line - W + 1;      // 1 .. H - 1
    y = dy > 0 ? j : H - 1 - j, x = dx > 0 ? 0 : W - 1;
  }
  V *Sv = reinterpret_cast<V *>(S);      // cell (p, d0) is element p * 64 + lane
  size_t p = img + (size_t)y * W + x;
  int C[K], Lp[K] = {}, m = 0;
  V old = V();
  sgm_cost<K>(cl, cr, p, x, d0, C);
  if (!first) old = Sv[p * 64 + lane];
  bool head = true;
  for (;;) {
    const int yn = y + dy, xn = x + dx;
    const bool more = (unsigned)yn < (unsigned)H && (unsigned)xn < (unsigned)W;
    const size_t pn = img + (size_t)(more ? yn : y) * W + (more ? xn : x);
    int Cn[K];
    V oldn = V();
    if (more) {      // wave-uniform
      sgm_cost<K>(cl, cr, pn, xn, d0, Cn);
      if (!first) oldn = Sv[pn * 64 + lane];
    }
    int L[K];
    if (head) {
#pragma unroll
      for (int k = 0; k < K; ++k) L[k] = C[k];
    } else {
      int up = __shfl_up(Lp[K - 1], 1, 64), dn = __shfl_down(Lp[0], 1, 64);
      if (lane == 0) up = ST_BIG;       // d - 1 < 0
      if (lane == 63) dn = ST_BIG;      // d + 1 >= D
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int lo = k > 0 ? Lp[k - 1] : up, hi = k < K - 1 ? Lp[k + 1] : dn;
        const int best = min(min(Lp[k], min(lo, hi) + P1), m + P2);
        L[k] = C[k] + best - m;
      }
    }
    int mine = L[0];
#pragma unroll
    for (int k = 1; k < K; ++k) mine = min(mine, L[k]);
    m = wave_min(mine);
    int sum[K];
    SVec<K>::unpack(old, sum);
#pragma unroll
    for (int k = 0; k < K; ++k) sum[k] += L[k], Lp[k] = L[k];      // old is 0 in the first direction
    Sv[p * 64 + lane] = SVec<K>::pack(sum);
    head = false;
    if (!more) break;
    y = yn, x = xn, p = pn, old = oldn;
#pragma unroll
    for (int k = 0; k < K; ++k) C[k] = Cn[k];
  }
}

// blockIdx.x * 4 + wave = the row of the batch (pair * H + y)
template <int K>
__global__ __launch_bounds__(ST_THREADS) void sgm_scan_kernel(const uint16_t *__restrict__ S, long long rows, int W, int32_t *__restrict__ dstar,
                                                              int32_t *__restrict__ dright) {
  typedef typename SVec<K>::T V;
  const int lane = threadIdx.x & 63, d0 = lane * K;
  const long long row = (long long)blockIdx.x * (ST_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;      // the whole wave
  const size_t base = (size_t)row * (size_t)W;
  const V *Sv = reinterpret_cast<const V *>(S);
  int ring[K];      // slot d: the running minimum of (S << 8 | d') for right pixel x = p - d
#pragma unroll
  for (int k = 0; k < K; ++k) ring[k] = ST_BIG;
  V cur = Sv[base * 64 + lane];
  for (int p = 0; p < W; ++p) {
    V nxt = V();
    if (p + 1 < W) nxt = Sv[(base + p + 1) * 64 + lane];
    int key[K];
    SVec<K>::unpack(cur, key);
#pragma unroll
    for (int k = 0; k < K; ++k) key[k] = (key[k] << 8) | (d0 + k);
    int carry = __shfl_up(ring[K - 1], 1, 64);
    if (lane == 0) carry = ST_BIG;      // slot 0 starts right pixel x = p
#pragma unroll
    for (int k = K - 1; k >= 1; --k) ring[k] = min(ring[k - 1], key[k]);
    ring[0] = min(carry, key[0]);
    int mine = key[0];
#pragma unroll
    for (int k = 1; k < K; ++k) mine = min(mine, key[k]);
    const int best = wave_min(mine);
    if (lane == 0) dstar[base + p] = best & 0xff;
    if (lane == 63 && p - (64 * K - 1) >= 0) dright[base + p - (64 * K - 1)] = ring[K - 1] & 0xff;      // slot D - 1 has seen every d
    cur = nxt;
  }
  // the row's end: right pixel x = W - 1 - d has seen d' = 0 .. d, and x + d' = W is outside
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int d = d0 + k, x = W - 1 - d;
    if (x >= 0 && d != 64 * K - 1) dright[base + x] = ring[k] & 0xff;
  }
}

struct StereoRule {
  int H, W, D, lr_max, min_disparity, subpixel;
  float fb, zfar;
};

__global__ __launch_bounds__(ST_THREADS) void stereo_final_kernel(const uint16_t *__restrict__ S, const int32_t *__restrict__ dstar,
                                                                  const int32_t *__restrict__ dright, long long total, StereoRule r,
                                                                  float *__restrict__ disparity, float *__restrict__ depth) {
  const long long i = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % r.W);
  const int ds = dstar[i];
  bool valid = x - ds >= 0 && ds >= r.min_disparity;
  if (valid && r.lr_max >= 0) valid = abs(dright[i - ds] - ds) <= r.lr_max;
  float disp = (float)ds;
  if (valid && r.subpixel && ds > 0 && ds < r.D - 1) {
    const uint16_t *s = S + (size_t)i * r.D + ds;
    const int a = s[-1], b = s[0], c = s[1];
    const int den = a - 2 * b + c;
    if (den > 0) disp = (float)ds + (float)(a - c) / (float)(2 * den);
  }
  if (disparity) disparity[i] = valid ? disp : -1.f;
  if (depth) {
    float z = 0.f;
    if (valid && disp > 0.f) {
      z = r.fb / disp;
      if (z > r.zfar) z = 0.f;
    }
    depth[i] = z;
  }
}

}  // namespace

// Where the arrays of a call lie in the blob (StereoLayout: common.h).  Host arithmetic only.
StereoLayout fp_stereo_layout(int n, int H, int W, int D, int channels) {
  const size_t px = (size_t)n * (size_t)H * (size_t)W;
  BlobLayout l;
  StereoLayout o;
  if (channels == 3) o.o_grey_l = l.put(px), o.o_grey_r = l.put(px);
  o.o_census_l = l.put(px * 8), o.o_census_r = l.put(px * 8);
  o.o_sum = l.put(px * (size_t)D * 2);
  o.o_dstar = l.put(px * 4), o.o_dright = l.put(px * 4);
  o.bytes = l.bytes;
  return o;
}

// Every check of a value, before the first look into ctx (tests/test_stereo_host.py calls fp_stereo_sgm without a GPU).  Fills `o`
// with the options as the call uses them.
int fp_stereo_check(const void *ctx, const void *d_left, const void *d_right, int n, int H, int W, int channels, const fp_stereo_opts *opts,
                    const float *d_depth, const fp_stereo_debug *dbg, fp_stereo_opts *o) {
  FP_REQUIRE(ctx && d_left && d_right && opts, "fp_stereo_sgm: null argument");
  FP_REQUIRE(opts->struct_size == sizeof(fp_stereo_opts), "fp_stereo_sgm: fp_stereo_opts.struct_size = %zu (this library knows %zu)", opts->struct_size,
             sizeof(fp_stereo_opts));
  FP_REQUIRE(!dbg || dbg->struct_size == sizeof(fp_stereo_debug), "fp_stereo_sgm: fp_stereo_debug.struct_size = %zu (this library knows %zu)",
             dbg ? dbg->struct_size : (size_t)0, sizeof(fp_stereo_debug));
  *o = *opts;
  FP_REQUIRE(n >= 1 && H >= 1 && W >= 1, "fp_stereo_sgm: n %d, H %d, W %d (each >= 1)", n, H, W);
  FP_REQUIRE(channels == 1 || channels == 3, "fp_stereo_sgm: channels %d (1 or 3)", channels);
  const int D = o->max_disparity;
  FP_REQUIRE(D >= 64 && D <= FP_STEREO_MAX_DISPARITY && D % 64 == 0, "fp_stereo_sgm: max_disparity %d (a multiple of 64, 64 .. %d)", D,
             FP_STEREO_MAX_DISPARITY);
  FP_REQUIRE(n <= 65535 && (double)n * (double)H * (double)W * (double)D <= (double)FP_STEREO_MAX_CELLS,
             "fp_stereo_sgm: %d pairs of %d x %d pixels with %d disparities (at most %lld cells and 65535 pairs a call)", n, H, W, D,
             (long long)FP_STEREO_MAX_CELLS);
  FP_REQUIRE(o->p1 >= 0 && o->p1 <= o->p2, "fp_stereo_sgm: p1 %d, p2 %d (0 <= p1 <= p2)", o->p1, o->p2);
  FP_REQUIRE(8 * (64 + (long long)o->p2) <= 65535, "fp_stereo_sgm: p2 %d (8 (64 + p2) must fit 16 bits: p2 <= 8127)", o->p2);
  FP_REQUIRE(o->paths >= 1 && o->paths <= 0xFF, "fp_stereo_sgm: paths 0x%x (1 .. 0xFF, one bit per direction)", o->paths);
  FP_REQUIRE(o->min_disparity >= 0 && o->min_disparity < D, "fp_stereo_sgm: min_disparity %d (0 .. max_disparity - 1)", o->min_disparity);
  FP_REQUIRE(o->subpixel == 0 || o->subpixel == 1, "fp_stereo_sgm: subpixel %d (0 or 1)", o->subpixel);
  if (d_depth) {
    const double fb = o->fx * o->baseline;
    FP_REQUIRE(isfinite((float)fb) && (float)fb > 0.f, "fp_stereo_sgm: fx %g, baseline %g (fx baseline must be positive and finite as fp32)", o->fx,
               o->baseline);
    FP_REQUIRE(o->zfar > 0.f, "fp_stereo_sgm: zfar %g (> 0; infinity: no limit)", (double)o->zfar);      // refuses a NaN too
  }
  return FP_OK;
}

struct fp_stereo_state {
  DevBlob blob;
};

void fp_stereo_state_free(fp_ctx *ctx) {
  fp_stereo_state *st = ctx->stereo;
  if (!st) return;
  st->blob.release();
  delete st;
  ctx->stereo = nullptr;
}

template <int K>
static int stereo_aggregate(fp_ctx *ctx, const u64 *cl, const u64 *cr, uint16_t *S, int32_t *dstar, int32_t *dright, int n, int H, int W, const fp_stereo_opts &o,
                            hipStream_t s) {
  static const int DIR[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};      // (dy, dx) of bit b of paths
  {
    ProfScope ps(ctx, s, "stereo_paths", 0.0);
    int first = 1;
    for (int b = 0; b < 8; ++b) {
      if (!(o.paths >> b & 1)) continue;
      const int dy = DIR[b][0], dx = DIR[b][1];
      const int lines = dy == 0 ? H : dx == 0 ? W : W + H - 1;
      hipLaunchKernelGGL(sgm_path_kernel<K>, dim3((unsigned)((lines + 3) / 4), (unsigned)n), dim3(ST_THREADS), 0, s, cl, cr, S, H, W, dy, dx, lines,
                         o.p1, o.p2, first);
      FP_CHECK_HIP(hipGetLastError());
      first = 0;
    }
  }
  ProfScope ps(ctx, s, "stereo_winner", 0.0);
  const long long rows = (long long)n * H;
  hipLaunchKernelGGL(sgm_scan_kernel<K>, dim3((unsigned)((rows + 3) / 4)), dim3(ST_THREADS), 0, s, (const uint16_t *)S, rows, W, dstar, dright);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

extern "C" int fp_stereo_sgm(fp_ctx *ctx, const uint8_t *d_left, const uint8_t *d_right, int n, int H, int W, int channels, const fp_stereo_opts *opts,
                             float *d_disparity, float *d_depth, const fp_stereo_debug *dbg, void *stream) {
  fp_stereo_opts o;
  FP_TRY(fp_stereo_check(ctx, d_left, d_right, n, H, W, channels, opts, d_depth, dbg, &o));
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  if (!ctx->stereo) ctx->stereo = new fp_stereo_state;
  const int D = o.max_disparity;
  const StereoLayout l = fp_stereo_layout(n, H, W, D, channels);
  FP_TRY(ctx->stereo->blob.ensure(l.bytes, "fp_stereo_sgm", "the census images and the summed costs"));
  const DevBlob &b = ctx->stereo->blob;
  hipStream_t s = (hipStream_t)stream;
  const long long px = (long long)n * H * W, cells = px * D;
  const uint8_t *gl = d_left, *gr = d_right;
  if (channels == 3) {
    hipLaunchKernelGGL(stereo_grey_kernel, grid_for(2 * px), dim3(ST_THREADS), 0, s, d_left, d_right, px, b.at<uint8_t>(l.o_grey_l),
                       b.at<uint8_t>(l.o_grey_r));
    FP_CHECK_HIP(hipGetLastError());
    gl = b.at<uint8_t>(l.o_grey_l), gr = b.at<uint8_t>(l.o_grey_r);
  }
  u64 *cl = b.at<u64>(l.o_census_l), *cr = b.at<u64>(l.o_census_r);
  uint16_t *S = b.at<uint16_t>(l.o_sum);
  int32_t *dstar = b.at<int32_t>(l.o_dstar), *dright = b.at<int32_t>(l.o_dright);
  {
    ProfScope ps(ctx, s, "stereo_census", 0.0);
    hipLaunchKernelGGL(stereo_census_kernel, grid_for(2 * px), dim3(ST_THREADS), 0, s, gl, gr, px, H, W, cl, cr);
    FP_CHECK_HIP(hipGetLastError());
  }
  if (dbg && dbg->d_cost) {
    hipLaunchKernelGGL(stereo_cost_kernel, grid_for(cells), dim3(ST_THREADS), 0, s, (const u64 *)cl, (const u64 *)cr, cells, W, D, dbg->d_cost);
    FP_CHECK_HIP(hipGetLastError());
  }
  if (D == 64) FP_TRY(stereo_aggregate<1>(ctx, cl, cr, S, dstar, dright, n, H, W, o, s));
  else if (D == 128) FP_TRY(stereo_aggregate<2>(ctx, cl, cr, S, dstar, dright, n, H, W, o, s));
  else if (D == 192) FP_TRY(stereo_aggregate<3>(ctx, cl, cr, S, dstar, dright, n, H, W, o, s));
  else FP_TRY(stereo_aggregate<4>(ctx, cl, cr, S, dstar, dright, n, H, W, o, s));
  if (d_disparity || d_depth) {
    ProfScope ps(ctx, s, "stereo_winner", 0.0);
    const StereoRule r{H, W, D, o.lr_max, o.min_disparity, o.subpixel, (float)(o.fx * o.baseline), o.zfar};
    hipLaunchKernelGGL(stereo_final_kernel, grid_for(px), dim3(ST_THREADS), 0, s, (const uint16_t *)S, (const int32_t *)dstar, (const int32_t *)dright, px, r,
                       d_disparity, d_depth);
    FP_CHECK_HIP(hipGetLastError());
  }
  if (dbg) {      // copies on the same stream, behind the kernels that wrote them
    if (dbg->d_census_left) FP_CHECK_HIP(hipMemcpyAsync(dbg->d_census_left, cl, (size_t)px * 8, hipMemcpyDeviceToDevice, s));
    if (dbg->d_census_right) FP_CHECK_HIP(hipMemcpyAsync(dbg->d_census_right, cr, (size_t)px * 8, hipMemcpyDeviceToDevice, s));
    if (dbg->d_sum) FP_CHECK_HIP(hipMemcpyAsync(dbg->d_sum, S, (size_t)cells * 2, hipMemcpyDeviceToDevice, s));
    if (dbg->d_dstar) FP_CHECK_HIP(hipMemcpyAsync(dbg->d_dstar, dstar, (size_t)px * 4, hipMemcpyDeviceToDevice, s));
    if (dbg->d_dright) FP_CHECK_HIP(hipMemcpyAsync(dbg->d_dright, dright, (size_t)px * 4, hipMemcpyDeviceToDevice, s));
  }
  return FP_OK;
}
