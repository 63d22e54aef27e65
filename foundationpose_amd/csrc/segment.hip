// Objects on a supporting plane from depth: plane hypotheses scored against every pixel (fp_plane_score), the moments of a plane's inliers
// for the least-squares refit (fp_plane_moments), and the connected components of what stands above the plane as an int32 label image
// with exact integer statistics (fp_depth_segment_count / _write).  The rules are stated in include/foundationpose_amd.h and restated in
// numpy by tests/segment_oracle.py; this file follows them operation for operation (the library is built without contraction).
//
// Everything written out is a function of the input alone:
//   * the inlier counts are int32 adds: ballots and popcounts per wave, one LDS add per (wave, 64 hypotheses), one global add per
//     (workgroup, hypothesis) with a non-zero count.  A workgroup owns (view, a tile of PS_TILE pixels, a chunk of PS_CHUNK hypotheses);
//     a lane keeps its PS_PIX points in registers, the planes arrive wave-uniformly from the table plane_hyp_kernel wrote;
//   * the 10 moments take the way of gn_sums.h: a lane's pixels in order, the butterfly over the wave, the waves in order through LDS, the
//     workgroup's own slot of a slab, gn_fold_kernel over the tiles in order.  No atomics;
//   * the components come from the lock-free union-find of union_find.h over parent[n_views H W] in global memory; the invariants and
//     the termination arguments are written there.  The members are the foreground pixels (background: -1, never passed in), and the
//     root a component ends with is its lowest pixel index.  The forest does not START as singletons: seg_init_kernel points every
//     pixel at the first pixel of its horizontal run inside its wave (a ballot, no memory traffic), which keeps parent[i] <= i;
//     seg_hook_kernel then joins a pixel with the one above it, and with the one to its left only where a run was cut by a wave's
//     first lane.  One launch of hooks, one flatten pass, no host loop;
//   * components and kept components are numbered by ONE exclusive scan (scan_exclusive) of a word that carries "is a root" in its low
//     half and "is a kept root" in its high half; the numbers of a view are differences against the word at the view's first pixel,
//     so a view does not depend on its batch;
//   * the statistics are 64-bit integer adds, minima and maxima of fixed-point values: exact, so the order does not matter.  A wave
//     whose kept pixels all belong to one component reduces them with shuffles and issues each atomic once.
// The hooks are scattered 4-byte atomics, which execute at the memory side: the labelling is bound by atomic requests and launches, not
// by bytes (DESIGN.md section 5 has the measurement).
#include "common.h"
#include "device_util.h"
#include "gn_sums.h"
#include "union_find.h"

#include <math.h>

typedef unsigned long long u64;

namespace {

constexpr int SEG_THREADS = 256;
constexpr int PS_PIX = 4;
constexpr int PS_TILE = SEG_THREADS * PS_PIX;      // 1024 pixels per workgroup of plane_count_kernel and plane_moments_kernel
constexpr int PS_CHUNK = 256;                      // hypotheses per workgroup of plane_count_kernel
constexpr int PM_TERMS = FP_PLANE_MOMENT_TERMS;
static_assert(PM_TERMS == 10 && FP_SEGMENT_STATS == 16 && FP_PLANE_MAX_HYP % PS_CHUNK == 0, "the header's sizes are those of this file");

struct SegPlanes {
  float4 p[FP_TSDF_MAX_VIEWS];      // (n.x, n.y, n.z, dd) of every view
};

struct SegRule {
  float h_min, h_max, max_jump;
  int min_pixels;
};

// the point of an integer pixel at depth d (view_geom.h)
__device__ __forceinline__ float3 seg_point(const Pinhole &cam, int row, int col, float d) { return pinhole_point(cam, (float)col, (float)row, d); }

__device__ __forceinline__ float seg_height(float4 pl, float3 p) { return ((pl.x * p.x + pl.y * p.y) + pl.z * p.z) + pl.w; }

__device__ __forceinline__ long long seg_q(float x) { return (long long)rintf(fminf(fmaxf(x * 1048576.f, -0x1p34f), 0x1p34f)); }

// ---- fp_plane_score ---------------------------------------------------------------------------------------------------------------

// one thread per (view, hypothesis): the plane through the three pixels, or (0,0,0,0)
__global__ __launch_bounds__(SEG_THREADS) void plane_hyp_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask, Pinhole cam, float zfar,
                                                                const int32_t *__restrict__ trip, int n_hyp, int total,
                                                                float4 *__restrict__ planes) {
  const int t = blockIdx.x * SEG_THREADS + threadIdx.x;
  if (t >= total) return;
  const int hw = cam.H * cam.W;
  const size_t view0 = (size_t)(t / n_hyp) * (size_t)hw;
  const int idx[3] = {trip[(size_t)t * 3], trip[(size_t)t * 3 + 1], trip[(size_t)t * 3 + 2]};
  float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
  bool valid = (unsigned)idx[0] < (unsigned)hw && (unsigned)idx[1] < (unsigned)hw && (unsigned)idx[2] < (unsigned)hw && idx[0] != idx[1] &&
               idx[0] != idx[2] && idx[1] != idx[2];
  float3 p[3];
  if (valid) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float d = depth[view0 + idx[a]];
      valid = valid && depth_ok(d, zfar) && (!mask || mask[view0 + idx[a]] != 0);
      const int row = idx[a] / cam.W;
      p[a] = seg_point(cam, row, idx[a] - row * cam.W, d);
    }
  }
  if (valid) {
    const float ux = p[1].x - p[0].x, uy = p[1].y - p[0].y, uz = p[1].z - p[0].z;
    const float wx = p[2].x - p[0].x, wy = p[2].y - p[0].y, wz = p[2].z - p[0].z;
    const float mx = uy * wz - uz * wy, my = uz * wx - ux * wz, mz = ux * wy - uy * wx;
    const float l2 = (mx * mx + my * my) + mz * mz;
    if (l2 > 0.f) {
      const float l = sqrtf(l2);
      float nx = mx / l, ny = my / l, nz = mz / l;
      float dd = -((nx * p[0].x + ny * p[0].y) + nz * p[0].z);
      if (dd < 0.f) nx = -nx, ny = -ny, nz = -nz, dd = -dd;
      out = make_float4(nx, ny, nz, dd);
    }
  }
  planes[t] = out;
}

// blockIdx = (tile, chunk of hypotheses, view).  counts[view][hypothesis] has been zeroed.
__global__ __launch_bounds__(SEG_THREADS) void plane_count_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask, Pinhole cam, float zfar,
                                                                  const float4 *__restrict__ planes, int n_hyp, float tol,
                                                                  int *__restrict__ counts) {
  __shared__ int cnt[PS_CHUNK];
  const int tid = threadIdx.x, lane = tid & 63;
  const int v = blockIdx.z, h0 = blockIdx.y * PS_CHUNK;
  const int hw = cam.H * cam.W;
  const size_t view0 = (size_t)v * (size_t)hw;
  cnt[tid] = 0;      // PS_CHUNK == SEG_THREADS
  static_assert(PS_CHUNK == SEG_THREADS, "one counter per thread");
  float3 p[PS_PIX];
  bool ok[PS_PIX];
  bool any = false;
#pragma unroll
  for (int q = 0; q < PS_PIX; ++q) {
    const long long pix = (long long)blockIdx.x * PS_TILE + q * SEG_THREADS + tid;
    const bool in = pix < hw;                                      // the last tile of a view is ragged
    const float d = in ? depth[view0 + (size_t)pix] : 0.f;
    ok[q] = in && depth_ok(d, zfar);
    if (mask) ok[q] = ok[q] && mask[view0 + (size_t)(in ? pix : 0)] != 0;
    const int row = (int)(pix / cam.W);
    p[q] = seg_point(cam, row, (int)(pix - (long long)row * cam.W), d);
    any = any || ok[q];
  }
  __syncthreads();
  if (__any(any)) {      // uniform in the wave: a wave without a usable pixel adds nothing
    const float4 *pl = planes + (size_t)v * n_hyp + h0;
    const int nh = min(PS_CHUNK, n_hyp - h0);
    for (int hb = 0; hb < nh; hb += 64) {
      int mine = 0;
      const int nj = min(64, nh - hb);
      for (int j = 0; j < nj; ++j) {
        const float4 g = pl[hb + j];                                // the same address in every lane
        int c = 0;
        if (g.x != 0.f || g.y != 0.f || g.z != 0.f) {               // a hypothesis without a plane counts nothing
#pragma unroll
          for (int q = 0; q < PS_PIX; ++q) c += __popcll(__ballot(ok[q] && fabsf(seg_height(g, p[q])) < tol));
        }
        if (lane == j) mine = c;
      }
      if (mine) atomicAdd(&cnt[hb + lane], mine);
    }
  }
  __syncthreads();
  if (h0 + tid < n_hyp && cnt[tid]) atomicAdd(&counts[(size_t)v * n_hyp + h0 + tid], cnt[tid]);
}

// one workgroup per view: the largest count, ties to the lowest index; -1 when every count is 0
__global__ __launch_bounds__(SEG_THREADS) void plane_best_kernel(const int *__restrict__ counts, int n_hyp, int *__restrict__ best) {
  __shared__ u64 red[SEG_THREADS / 64];
  const int v = blockIdx.x;
  u64 key = 0;      // (count, ~index): the maximum is the largest count at the lowest index
  for (int h = threadIdx.x; h < n_hyp; h += SEG_THREADS) {
    const u64 k = ((u64)(unsigned)counts[(size_t)v * n_hyp + h] << 32) | (u64)(0xffffffffu - (unsigned)h);
    key = k > key ? k : key;
  }
  key = wave_reduce(key, [](u64 a, u64 b) { return a > b ? a : b; });
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < SEG_THREADS / 64; ++i) key = red[i] > key ? red[i] : key;
    best[v] = (key >> 32) == 0 ? -1 : (int)(0xffffffffu - (unsigned)(key & 0xffffffffu));
  }
}

// ---- fp_plane_moments -------------------------------------------------------------------------------------------------------------

// blockIdx.x = view * n_tiles + tile; the summation order is that of gn_sums.h with 10 terms
__global__ __launch_bounds__(SEG_THREADS) void plane_moments_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask, Pinhole cam, float zfar,
                                                                    SegPlanes planes, float tol, int n_tiles, double *__restrict__ slab) {
  __shared__ double red[SEG_THREADS / 64][PM_TERMS];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % n_tiles, v = blockIdx.x / n_tiles;
  const float4 g = planes.p[v];
  const int hw = cam.H * cam.W;
  const size_t view0 = (size_t)v * (size_t)hw;
  double acc[PM_TERMS];
#pragma unroll
  for (int e = 0; e < PM_TERMS; ++e) acc[e] = 0.0;
#pragma unroll
  for (int q = 0; q < PS_PIX; ++q) {
    const long long pix = (long long)tile * PS_TILE + q * SEG_THREADS + tid;
    const bool in = pix < hw;
    const float d = in ? depth[view0 + (size_t)pix] : 0.f;
    bool ok = in && depth_ok(d, zfar);
    if (mask) ok = ok && mask[view0 + (size_t)(in ? pix : 0)] != 0;
    const int row = (int)(pix / cam.W);
    const float3 p = seg_point(cam, row, (int)(pix - (long long)row * cam.W), d);
    ok = ok && fabsf(seg_height(g, p)) < tol;
    const double x = ok ? (double)p.x : 0.0, y = ok ? (double)p.y : 0.0, z = ok ? (double)p.z : 0.0;      // any other pixel is a zero row
    acc[0] += ok ? 1.0 : 0.0;
    acc[1] += x, acc[2] += y, acc[3] += z;
    acc[4] += x * x, acc[5] += x * y, acc[6] += x * z;
    acc[7] += y * y, acc[8] += y * z, acc[9] += z * z;
  }
#pragma unroll
  for (int e = 0; e < PM_TERMS; ++e) {
    const double s = wave_sum(acc[e]);
    if ((tid & 63) == 0) red[tid >> 6][e] = s;
  }
  __syncthreads();
  gn_lds_to_slab(red, slab + ((size_t)v * n_tiles + tile) * PM_TERMS);
}

// ---- fp_depth_segment_* -----------------------------------------------------------------------------------------------------------

// One thread per pixel of the batch, i = view H W + row W + col; a workgroup starts at a multiple of 64, so lane == i & 63.
// parent[i] = -1 for background; for foreground the first pixel of the run of joined pixels that ends at i, as far as it lies in this
// wave: i - 1 is in the same row when col > 0 and in the same wave when lane > 0.
__global__ __launch_bounds__(SEG_THREADS) void seg_init_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask, Pinhole cam, float zfar,
                                                               SegPlanes planes, SegRule rule, int total, int *__restrict__ parent,
                                                               int *__restrict__ cnt) {
  const int i = blockIdx.x * SEG_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  const bool in = i < total;
  const int hw = cam.H * cam.W;
  const int v = in ? i / hw : 0, pix = i - v * hw, row = pix / cam.W, col = pix - row * cam.W;
  const float d = in ? depth[i] : 0.f;
  bool fg = in && depth_ok(d, zfar);
  if (mask) fg = fg && mask[in ? i : 0] != 0;
  const float h = seg_height(planes.p[v], seg_point(cam, row, col, d));
  fg = fg && h >= rule.h_min && h <= rule.h_max;
  const float dl = __shfl_up(d, 1, 64);
  const int fgl = __shfl_up((int)fg, 1, 64);
  const bool link = fg && fgl && lane > 0 && col > 0 && fabsf(d - dl) <= rule.max_jump;
  const u64 cut = ~__ballot(link) & (lane == 63 ? ~0ull : (2ull << lane) - 1);      // lanes 0 .. lane that start a run; lane 0 always does
  const int start = 63 - __clzll((long long)cut);
  if (in) {
    parent[i] = fg ? i - (lane - start) : -1;
    cnt[i] = 0;
  }
}

// joins a foreground pixel with the one above it, and with the one to its left where seg_init_kernel could not (lane 0)
__global__ __launch_bounds__(SEG_THREADS) void seg_hook_kernel(const float *__restrict__ depth, Pinhole cam, float max_jump, int total, int *parent) {
  const int i = blockIdx.x * SEG_THREADS + threadIdx.x;
  if (i >= total || cc_load(&parent[i]) < 0) return;
  const int hw = cam.H * cam.W;
  const int pix = i % hw, row = pix / cam.W, col = pix - row * cam.W;
  const float d = depth[i];
  if (row > 0 && cc_load(&parent[i - cam.W]) >= 0 && fabsf(d - depth[i - cam.W]) <= max_jump) cc_unite(parent, i, i - cam.W);
  if ((threadIdx.x & 63) == 0 && col > 0 && cc_load(&parent[i - 1]) >= 0 && fabsf(d - depth[i - 1]) <= max_jump) cc_unite(parent, i, i - 1);
}

// parent[i] becomes the lowest pixel of i's component (the roots are final: the hooks have all run); cnt[r] counts the pixels of root r
__global__ __launch_bounds__(SEG_THREADS) void seg_flatten_kernel(int total, int *parent, int *__restrict__ cnt) {
  const int i = blockIdx.x * SEG_THREADS + threadIdx.x;
  int r = -1;
  if (i < total) {
    r = cc_load(&parent[i]);
    if (r >= 0) {
      r = cc_root(parent, r);
      __hip_atomic_store(&parent[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  wave_add_one(cnt, r, r >= 0);
}

// data[i] = (i is a root) + 2^32 (i is a root of at least min_pixels pixels); data[total] = 0 closes the scan
__global__ __launch_bounds__(SEG_THREADS) void seg_flag_kernel(int total, const int *__restrict__ label, const int *__restrict__ cnt, int min_pixels,
                                                               u64 *__restrict__ data) {
  const int i = blockIdx.x * SEG_THREADS + threadIdx.x;
  if (i > total) return;
  u64 w = 0;
  if (i < total && label[i] == i) w = 1ull | ((u64)(cnt[i] >= min_pixels ? 1 : 0) << 32);
  data[i] = w;
}

// per view {components, kept components}: the scanned words at the view's two ends; neither half borrows from the other
__global__ void seg_counts_kernel(const u64 *__restrict__ data, int n_views, int hw, int *__restrict__ out) {
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v >= n_views) return;
  const u64 dlt = data[(size_t)(v + 1) * hw] - data[(size_t)v * hw];
  out[2 * v] = (int)(dlt & 0xffffffffu), out[2 * v + 1] = (int)(dlt >> 32);
}

constexpr long long I64_MAX = 0x7fffffffffffffffll, I64_MIN = -I64_MAX - 1;

// the fields of a statistics row: 0 n, 1 rmin, 2 rmax, 3 cmin, 4 cmax, 5-7 sums of q, 8-10 minima, 11-13 maxima, 14 max q(h), 15 lowest pixel
__global__ __launch_bounds__(SEG_THREADS) void seg_stats_init_kernel(long long n, long long *__restrict__ stats) {
  const long long t = (long long)blockIdx.x * SEG_THREADS + threadIdx.x;
  if (t >= n) return;
  const int f = (int)(t & 15);
  stats[t] = (f == 3 || (f >= 8 && f <= 10)) ? I64_MAX : (f == 2 || f == 4 || (f >= 11 && f <= 14)) ? I64_MIN : 0;
}

__device__ __forceinline__ void stats_atomics(long long *row, const long long (&s)[13]) {
  atomicMax(&row[2], s[0]);
  atomicMin(&row[3], s[1]);
  atomicMax(&row[4], s[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicAdd((u64 *)&row[5 + a], (u64)s[3 + a]);      // two's complement: the signed sum
    atomicMin(&row[8 + a], s[6 + a]);
    atomicMax(&row[11 + a], s[9 + a]);
  }
  atomicMax(&row[14], s[12]);
}

// the label image and, with `stats`, the statistics of the kept components; stats rows have been initialised
__global__ __launch_bounds__(SEG_THREADS) void seg_label_kernel(const float *__restrict__ depth, Pinhole cam, SegPlanes planes, int min_pixels,
                                                                int total, const int *__restrict__ label, const int *__restrict__ cnt,
                                                                const u64 *__restrict__ data, int32_t *__restrict__ labels,
                                                                long long *__restrict__ stats) {
  const int i = blockIdx.x * SEG_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  const bool in = i < total;
  const int hw = cam.H * cam.W;
  const int v = in ? i / hw : 0, pix = i - v * hw, row = pix / cam.W, col = pix - row * cam.W;
  const int r = in ? label[i] : -1;
  const bool kept = r >= 0 && cnt[r] >= min_pixels;
  const long long k = kept ? (long long)(data[r] >> 32) : 0;      // the component's number in the batch, from 0
  if (in && labels) labels[i] = kept ? (int32_t)(k - (long long)(data[(size_t)v * hw] >> 32) + 1) : 0;
  if (!stats) return;
  const u64 act = __ballot(kept);
  if (act == 0) return;
  const float3 p = seg_point(cam, row, col, in ? depth[i] : 0.f);
  const long long qx = seg_q(p.x), qy = seg_q(p.y), qz = seg_q(p.z), qh = seg_q(seg_height(planes.p[v], p));
  if (kept && r == i) {      // the root is the component's lowest pixel: its first row
    long long *o = stats + k * FP_SEGMENT_STATS;
    o[0] = cnt[r], o[1] = row, o[15] = pix;
  }
  long long s[13] = {row, col, col, qx, qy, qz, qx, qy, qz, qx, qy, qz, qh};
  const long long lead = __shfl(k, __ffsll((long long)act) - 1, 64);
  if (__ballot(kept && k == lead) == act) {      // one component in the wave: reduce, then each atomic once
    constexpr int kind[13] = {2, 1, 2, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2};      // 0 sum, 1 min, 2 max
#pragma unroll
    for (int e = 0; e < 13; ++e) {
      long long x = kept ? s[e] : (kind[e] == 0 ? 0 : kind[e] == 1 ? I64_MAX : I64_MIN);
      if (kind[e] == 0) x = wave_reduce(x, [](long long a, long long b) { return a + b; });
      else if (kind[e] == 1) x = wave_reduce(x, [](long long a, long long b) { return a < b ? a : b; });
      else x = wave_reduce(x, [](long long a, long long b) { return a > b ? a : b; });
      s[e] = x;
    }
    if (lane == 0) stats_atomics(stats + lead * FP_SEGMENT_STATS, s);
  } else if (kept) {
    stats_atomics(stats + k * FP_SEGMENT_STATS, s);
  }
}

// the checks the four calls share, each before the first look into ctx
int seg_check_frame(const char *fn, int n_views, int H, int W, const double *K, float zfar) {
  FP_REQUIRE(n_views >= 0 && n_views <= FP_TSDF_MAX_VIEWS, "%s: n_views %d (0 .. %d)", fn, n_views, FP_TSDF_MAX_VIEWS);
  FP_REQUIRE(H >= 1 && W >= 1, "%s: H %d, W %d", fn, H, W);
  FP_REQUIRE((long long)(n_views > 0 ? n_views : 1) * H * W <= FP_SEGMENT_MAX_PIXELS, "%s: %d views of %d x %d pixels (at most %d pixels a call)",
             fn, n_views, H, W, FP_SEGMENT_MAX_PIXELS);
  FP_REQUIRE(zfar > 0.f && zfar <= 1000.f, "%s: zfar %g (0 < zfar <= 1000)", fn, (double)zfar);
  return fp_check_camera(fn, K);
}

int seg_check_planes(const char *fn, const double *planes, int n_views, SegPlanes *out) {
  memset(out, 0, sizeof(*out));
  for (int v = 0; v < n_views; ++v) {
    const float4 g = make_float4((float)planes[4 * v], (float)planes[4 * v + 1], (float)planes[4 * v + 2], (float)planes[4 * v + 3]);
    FP_REQUIRE(isfinite(g.x) && isfinite(g.y) && isfinite(g.z) && isfinite(g.w), "%s: the plane of view %d is not finite", fn, v);
    FP_REQUIRE(g.x != 0.f || g.y != 0.f || g.z != 0.f, "%s: the plane of view %d has a zero normal", fn, v);
    out->p[v] = g;
  }
  return FP_OK;
}

}  // namespace

extern "C" int fp_plane_score(fp_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int n_views, int H, int W, const double *K, float zfar,
                              const int32_t *triplets, int n_hyp, float tol, float *h_planes, int32_t *h_counts, int32_t *h_best, void *stream) {
  // Every check of a value comes before the first look INTO ctx: tests/test_segment_host.py calls this without a GPU, with a pointer for
  // ctx that must not be dereferenced.  Keep that order when adding checks.
  FP_REQUIRE(ctx && d_depth && K && h_best, "fp_plane_score: null argument");
  FP_REQUIRE(n_hyp >= 0 && n_hyp <= FP_PLANE_MAX_HYP, "fp_plane_score: n_hyp %d (0 .. %d)", n_hyp, FP_PLANE_MAX_HYP);
  FP_REQUIRE(n_hyp == 0 || (triplets && h_planes && h_counts), "fp_plane_score: null triplets, h_planes or h_counts with n_hyp > 0");
  FP_REQUIRE(tol > 0.f, "fp_plane_score: tol %g (> 0)", (double)tol);
  FP_TRY(seg_check_frame("fp_plane_score", n_views, H, W, K, zfar));
  if (n_views == 0) return FP_OK;
  const Pinhole cam = pinhole_of(K, H, W);
  hipStream_t s = (hipStream_t)stream;
  if (n_hyp == 0) {
    FP_CHECK_HIP(hipStreamSynchronize(s));
    for (int v = 0; v < n_views; ++v) h_best[v] = -1;
    return FP_OK;
  }
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  const size_t nvh = (size_t)n_views * n_hyp;
  const size_t trip_bytes = align256(nvh * 12), plane_bytes = align256(nvh * 16), count_bytes = align256(nvh * 4), best_bytes = align256((size_t)n_views * 4);
  FP_TRY(fp_arena_ensure(ctx, trip_bytes + plane_bytes + count_bytes + best_bytes + 4096));
  ArenaScope scope(ctx->arena);
  int32_t *trip = (int32_t *)ctx->arena.take(trip_bytes);
  float4 *planes = (float4 *)ctx->arena.take(plane_bytes);
  int *counts = (int *)ctx->arena.take(count_bytes);
  int *best = (int *)ctx->arena.take(best_bytes);
  FP_REQUIRE(trip && planes && counts && best, "fp_plane_score: arena exhausted");
  FP_CHECK_HIP(hipMemcpyAsync(trip, triplets, nvh * 12, hipMemcpyHostToDevice, s));
  FP_CHECK_HIP(hipMemsetAsync(counts, 0, nvh * 4, s));
  hipLaunchKernelGGL(plane_hyp_kernel, grid_for((long long)nvh), dim3(SEG_THREADS), 0, s, d_depth, d_mask, cam, zfar, (const int32_t *)trip, n_hyp, (int)nvh,
                     planes);
  FP_CHECK_HIP(hipGetLastError());
  const unsigned n_tiles = (unsigned)(((long long)H * W + PS_TILE - 1) / PS_TILE);
  hipLaunchKernelGGL(plane_count_kernel, dim3(n_tiles, (unsigned)((n_hyp + PS_CHUNK - 1) / PS_CHUNK), (unsigned)n_views), dim3(SEG_THREADS), 0, s, d_depth,
                     d_mask, cam, zfar, (const float4 *)planes, n_hyp, tol, counts);
  FP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(plane_best_kernel, dim3((unsigned)n_views), dim3(SEG_THREADS), 0, s, (const int *)counts, n_hyp, best);
  FP_CHECK_HIP(hipGetLastError());
  // the tables go back to the arena when this returns: the stream has been synchronised by then
  FP_CHECK_HIP(hipMemcpyAsync(h_planes, planes, nvh * 16, hipMemcpyDeviceToHost, s));
  FP_CHECK_HIP(hipMemcpyAsync(h_counts, counts, nvh * 4, hipMemcpyDeviceToHost, s));
  FP_CHECK_HIP(hipMemcpyAsync(h_best, best, (size_t)n_views * 4, hipMemcpyDeviceToHost, s));
  FP_CHECK_HIP(hipStreamSynchronize(s));
  return FP_OK;
}

extern "C" int fp_plane_moments(fp_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int n_views, int H, int W, const double *K, float zfar,
                                const double *planes, float tol, double *h_sums, void *stream) {
  // As above: every check of a value before the first look into ctx.
  FP_REQUIRE(ctx && d_depth && K && planes && h_sums, "fp_plane_moments: null argument");
  FP_REQUIRE(tol > 0.f, "fp_plane_moments: tol %g (> 0)", (double)tol);
  FP_TRY(seg_check_frame("fp_plane_moments", n_views, H, W, K, zfar));
  SegPlanes pl;
  FP_TRY(seg_check_planes("fp_plane_moments", planes, n_views, &pl));
  if (n_views == 0) return FP_OK;
  const Pinhole cam = pinhole_of(K, H, W);
  hipStream_t s = (hipStream_t)stream;
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  const int n_tiles = (int)(((long long)H * W + PS_TILE - 1) / PS_TILE);
  const size_t slab_bytes = (size_t)n_views * n_tiles * PM_TERMS * sizeof(double), sums_bytes = (size_t)n_views * PM_TERMS * sizeof(double);
  FP_TRY(fp_arena_ensure(ctx, slab_bytes + sums_bytes + 4096));
  ArenaScope scope(ctx->arena);
  double *slab = (double *)ctx->arena.take(slab_bytes);
  double *sums = (double *)ctx->arena.take(sums_bytes);
  FP_REQUIRE(slab && sums, "fp_plane_moments: arena exhausted");
  hipLaunchKernelGGL(plane_moments_kernel, dim3((unsigned)(n_tiles * n_views)), dim3(SEG_THREADS), 0, s, d_depth, d_mask, cam, zfar, pl, tol, n_tiles, slab);
  FP_CHECK_HIP(hipGetLastError());
  return gn_fold_to_host<PM_TERMS>(slab, n_views, n_tiles, sums, h_sums, s);
}

// What fp_depth_segment_count leaves for fp_depth_segment_write: one allocation owned by the context, grown when a larger batch arrives.
struct fp_segment_state {
  DevBlob blob;
  // views into blob
  int *head = nullptr, *parent = nullptr, *cnt = nullptr;      // {components, kept} per view; the label of every pixel; pixels at every root
  u64 *data = nullptr, *sums = nullptr;
  // the counted call
  bool valid = false;
  const float *depth = nullptr;
  int n_views = 0, H = 0, W = 0, min_pixels = 0;
  long long kept = 0;
  Pinhole cam;
  SegPlanes planes;
};

void fp_segment_state_free(fp_ctx *ctx) {
  fp_segment_state *st = ctx->segment;
  if (!st) return;
  st->blob.release();
  delete st;
  ctx->segment = nullptr;
}

static int segment_layout(fp_segment_state *st, long long total) {
  BlobLayout l;
  const size_t o_head = l.put(FP_TSDF_MAX_VIEWS * 2 * sizeof(int)), o_parent = l.put((size_t)total * 4), o_cnt = l.put((size_t)total * 4),
               o_data = l.put(((size_t)total + 1) * 8), o_sums = l.put(scan_sums_words(total + 1) * 8);
  FP_TRY(st->blob.ensure(l.bytes, "fp_depth_segment_count", "the state"));
  const DevBlob &b = st->blob;
  st->head = b.at<int>(o_head), st->parent = b.at<int>(o_parent), st->cnt = b.at<int>(o_cnt);
  st->data = b.at<u64>(o_data), st->sums = b.at<u64>(o_sums);
  return FP_OK;
}

extern "C" int fp_depth_segment_count(fp_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int n_views, int H, int W, const double *K, float zfar,
                                      const double *planes, float h_min, float h_max, float max_jump, int min_pixels, int32_t *h_counts,
                                      void *stream) {
  // As above: every check of a value before the first look into ctx.
  FP_REQUIRE(ctx && d_depth && K && planes && h_counts, "fp_depth_segment_count: null argument");
  FP_REQUIRE(max_jump > 0.f, "fp_depth_segment_count: max_jump %g (> 0)", (double)max_jump);
  FP_REQUIRE(h_max >= h_min, "fp_depth_segment_count: h_min %g, h_max %g (h_max >= h_min)", (double)h_min, (double)h_max);
  FP_REQUIRE(min_pixels >= 1, "fp_depth_segment_count: min_pixels %d (>= 1)", min_pixels);
  FP_TRY(seg_check_frame("fp_depth_segment_count", n_views, H, W, K, zfar));
  SegPlanes pl;
  FP_TRY(seg_check_planes("fp_depth_segment_count", planes, n_views, &pl));
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  if (!ctx->segment) ctx->segment = new fp_segment_state;
  fp_segment_state *st = ctx->segment;
  st->valid = false;
  hipStream_t s = (hipStream_t)stream;
  st->kept = 0;
  if (n_views > 0) {
    const long long total = (long long)n_views * H * W;
    FP_TRY(segment_layout(st, total));
    const Pinhole cam = pinhole_of(K, H, W);
    const SegRule rule{h_min, h_max, max_jump, min_pixels};
    st->cam = cam, st->planes = pl;
    hipLaunchKernelGGL(seg_init_kernel, grid_for(total), dim3(SEG_THREADS), 0, s, d_depth, d_mask, cam, zfar, pl, rule, (int)total, st->parent, st->cnt);
    FP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(seg_hook_kernel, grid_for(total), dim3(SEG_THREADS), 0, s, d_depth, cam, max_jump, (int)total, st->parent);
    FP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(seg_flatten_kernel, grid_for(total), dim3(SEG_THREADS), 0, s, (int)total, st->parent, st->cnt);
    FP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(seg_flag_kernel, grid_for(total + 1), dim3(SEG_THREADS), 0, s, (int)total, (const int *)st->parent, (const int *)st->cnt,
                       min_pixels, st->data);
    FP_CHECK_HIP(hipGetLastError());
    FP_TRY(scan_exclusive(st->data, total + 1, st->sums, s));
    hipLaunchKernelGGL(seg_counts_kernel, dim3((unsigned)((n_views + 63) / 64)), dim3(64), 0, s, (const u64 *)st->data, n_views, H * W, st->head);
    FP_CHECK_HIP(hipGetLastError());
    FP_CHECK_HIP(hipMemcpyAsync(h_counts, st->head, (size_t)n_views * 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    FP_CHECK_HIP(hipStreamSynchronize(s));
    for (int v = 0; v < n_views; ++v) st->kept += h_counts[2 * v + 1];
  } else {
    FP_CHECK_HIP(hipStreamSynchronize(s));
  }
  st->depth = d_depth, st->n_views = n_views, st->H = H, st->W = W, st->min_pixels = min_pixels;
  st->valid = true;
  return FP_OK;
}

extern "C" int fp_depth_segment_write(fp_ctx *ctx, const float *d_depth, int n_views, int H, int W, int32_t *d_labels, int64_t *d_stats, int64_t n_kept,
                                      void *stream) {
  FP_REQUIRE(ctx, "fp_depth_segment_write: null argument");
  const fp_segment_state *st = ctx->segment;
  FP_REQUIRE(st && st->valid, "fp_depth_segment_write: no fp_depth_segment_count before it");
  FP_REQUIRE(st->depth == d_depth && st->n_views == n_views && st->H == H && st->W == W,
             "fp_depth_segment_write: not the maps of the last fp_depth_segment_count (%d views of %d x %d counted)", st->n_views, st->H, st->W);
  FP_REQUIRE(n_kept == st->kept, "fp_depth_segment_write: %lld kept components given, %lld counted", (long long)n_kept, st->kept);
  FP_REQUIRE(d_labels, "fp_depth_segment_write: d_labels is null");
  if (n_views == 0) return FP_OK;
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const long long total = (long long)n_views * H * W;
  long long *stats = n_kept > 0 ? (long long *)d_stats : nullptr;
  if (stats) {
    hipLaunchKernelGGL(seg_stats_init_kernel, grid_for(n_kept * FP_SEGMENT_STATS), dim3(SEG_THREADS), 0, s, (long long)n_kept * FP_SEGMENT_STATS, stats);
    FP_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(seg_label_kernel, grid_for(total), dim3(SEG_THREADS), 0, s, d_depth, st->cam, st->planes, st->min_pixels, (int)total,
                     (const int *)st->parent, (const int *)st->cnt, (const u64 *)st->data, d_labels, stats);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
