// Depth maps of one or several calibrated pinhole cameras reprojected into ONE target pinhole camera of another size
// (fp_depth_reproject): registering the depth of an RGB-D sensor into its colour camera, or merging a rig of depth cameras into one view.
// A forward warp with a z-buffer - a scatter, which no gather (fp_remap) can do.  The rule is stated in include/foundationpose_amd.h
// and restated in numpy by tests/depth_reproject_oracle.py; everything is fp32 with every operation rounded once in the written order
// (the library is built without contraction), so this file has to match the oracle bit for bit, on every run and in any batch.
//
//   * hipMemsetAsync fills the key buffer (8 bytes a target pixel) with all ones.
//   * reproject_scatter_kernel: one thread per source pixel; blockIdx.y is the view and blockIdx.z the frame, so a view's camera and
//     transform - kernel arguments - arrive as scalar loads.  A thread computes the footprint of its pixel in the target (at most
//     FP_REPROJECT_MAX_SPLAT x FP_REPROJECT_MAX_SPLAT pixels) and folds (depth bits << 32 | source index) into each of them with one
//     integer atomicMin without a return value: the nearest surface wins, among equal depths the lowest source index, whatever the order
//     of the threads.  A positive fp32's bit order is its value order (the device of surface_distance.hip and raster.hip).
//   * reproject_finalise_kernel: one thread per target pixel turns its key into the depth and the winner's source index.
// No allocation and no synchronisation: the caller brings the key buffer, and the three nodes can be captured into a graph at once.
#include "common.h"
#include "view_geom.h"

namespace {

typedef unsigned long long u64;

constexpr int RP_THREADS = 256;
constexpr u64 RP_EMPTY = ~(u64)0;

struct ReprojectViews {
  Pinhole cam[FP_REPROJECT_MAX_VIEWS];
  Rigid to_dst[FP_REPROJECT_MAX_VIEWS];
};

__device__ __forceinline__ float3 rigid_point(const Rigid &m, const float3 p) {
  return make_float3(rigid_apply(m, 0, p.x, p.y, p.z), rigid_apply(m, 1, p.x, p.y, p.z), rigid_apply(m, 2, p.x, p.y, p.z));
}

// the range rule along one axis: lo / hi of the footprint (e0, e1 = the two corners, c = the centre) and the centre's own pixel pc
__device__ __forceinline__ void splat_range(float e0, float e1, float c, float &lo, float &hi, float &pc) {
  const float a = ceilf(fminf(e0, e1)), b = ceilf(fmaxf(e0, e1)) - 1.f;
  pc = floorf(c + 0.5f);
  lo = fminf(a, pc), hi = fmaxf(b, pc);
}

__global__ __launch_bounds__(RP_THREADS) void reproject_scatter_kernel(ReprojectViews views, Pinhole dst, const float *__restrict__ depth,
                                                                       u64 *__restrict__ keys, float zfar) {
  const int s = blockIdx.y, frame = blockIdx.z, V = gridDim.y;
  const Pinhole &cam = views.cam[s];
  const Rigid &T = views.to_dst[s];
  const int hw = cam.H * cam.W;      // V hw <= 2^31 - 1
  const int pix = blockIdx.x * RP_THREADS + threadIdx.x;
  if (pix >= hw) return;
  const float d = depth[((size_t)frame * V + s) * (size_t)hw + pix];
  if (!depth_ok(d, zfar)) return;
  const int r = pix / cam.W, c = pix - r * cam.W;
  const float cf = (float)c, rf = (float)r;
  const float3 q = rigid_point(T, pinhole_point(cam, cf, rf, d));
  if (!depth_ok(q.z, zfar)) return;
  const float3 q0 = rigid_point(T, pinhole_point(cam, cf - 0.5f, rf - 0.5f, d));
  const float3 q1 = rigid_point(T, pinhole_point(cam, cf + 0.5f, rf + 0.5f, d));
  if (!(q0.z > 0.f && q1.z > 0.f)) return;
  const float2 pc = project_ratio(dst, q.x, q.y, q.z), p0 = project_ratio(dst, q0.x, q0.y, q0.z), p1 = project_ratio(dst, q1.x, q1.y, q1.z);
  // everything is decided in float: nothing huge and no NaN reaches a cast
  if (!(isfinite(pc.x) && isfinite(pc.y) && isfinite(p0.x) && isfinite(p0.y) && isfinite(p1.x) && isfinite(p1.y))) return;
  float x_lo, x_hi, xc, y_lo, y_hi, yc;
  splat_range(p0.x, p1.x, pc.x, x_lo, x_hi, xc);
  splat_range(p0.y, p1.y, pc.y, y_lo, y_hi, yc);
  if (!(isfinite(x_lo) && isfinite(x_hi) && isfinite(y_lo) && isfinite(y_hi))) return;
  if ((x_hi - x_lo) + 1.f > (float)FP_REPROJECT_MAX_SPLAT || (y_hi - y_lo) + 1.f > (float)FP_REPROJECT_MAX_SPLAT)
    x_lo = x_hi = xc, y_lo = y_hi = yc;      // a grazing surface or an absurd magnification: the centre's pixel alone
  x_lo = fmaxf(x_lo, 0.f), x_hi = fminf(x_hi, (float)(dst.W - 1));
  y_lo = fmaxf(y_lo, 0.f), y_hi = fminf(y_hi, (float)(dst.H - 1));
  if (x_lo > x_hi || y_lo > y_hi) return;      // from here on 0 <= lo <= hi <= size - 1 and hi - lo < FP_REPROJECT_MAX_SPLAT
  const int x0 = (int)x_lo, x1 = (int)x_hi, y0 = (int)y_lo, y1 = (int)y_hi;
  const u64 key = ((u64)__float_as_uint(q.z) << 32) | (u64)(unsigned)(s * hw + pix);
  u64 *out = keys + (size_t)frame * (size_t)dst.H * (size_t)dst.W;
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x) atomicMin(out + (size_t)y * dst.W + x, key);
}

// total = the target pixels of one frame; blockIdx.y is the frame
__global__ __launch_bounds__(RP_THREADS) void reproject_finalise_kernel(const u64 *__restrict__ keys, int total, float *__restrict__ depth_out,
                                                                        int32_t *__restrict__ source) {
  const int p = blockIdx.x * RP_THREADS + threadIdx.x;
  if (p >= total) return;
  const size_t i = (size_t)blockIdx.y * (size_t)total + p;
  const u64 k = keys[i];
  const bool hit = k != RP_EMPTY;
  depth_out[i] = hit ? __uint_as_float((unsigned)(k >> 32)) : 0.f;
  if (source) source[i] = hit ? (int32_t)(unsigned)k : -1;
}

}  // namespace

// Every check of a value, before the first look into ctx (tests/test_depth_reproject_host.py calls fp_depth_reproject without a GPU).
int fp_depth_reproject_check(const void *ctx, const void *d_depth, int n, int V, int Hs, int Ws, const double *Ks, const double *T_dst_src,
                             const double *K_dst, int Hd, int Wd, float zfar, const void *d_keys, const void *d_depth_out) {
  FP_REQUIRE(ctx && d_depth && Ks && T_dst_src && K_dst && d_keys && d_depth_out, "fp_depth_reproject: null argument");
  FP_REQUIRE(n >= 1 && n <= FP_REPROJECT_MAX_FRAMES, "fp_depth_reproject: n %d (1 .. %d)", n, FP_REPROJECT_MAX_FRAMES);
  FP_REQUIRE(V >= 1 && V <= FP_REPROJECT_MAX_VIEWS, "fp_depth_reproject: V %d (1 .. %d)", V, FP_REPROJECT_MAX_VIEWS);
  FP_REQUIRE(Hs >= 1 && Ws >= 1 && Hd >= 1 && Wd >= 1 && Hs <= FP_REMAP_MAX_SIDE && Ws <= FP_REMAP_MAX_SIDE && Hd <= FP_REMAP_MAX_SIDE &&
                 Wd <= FP_REMAP_MAX_SIDE,
             "fp_depth_reproject: %d x %d to %d x %d (each side 1 .. %d)", Hs, Ws, Hd, Wd, FP_REMAP_MAX_SIDE);
  FP_REQUIRE((long long)V * Hs * Ws <= 0x7fffffffLL, "fp_depth_reproject: %d views of %d x %d pixels (at most 2^31 - 1 source pixels a frame)", V, Hs,
             Ws);
  for (int s = 0; s < V; ++s) {
    for (int e = 0; e < 9; ++e) FP_REQUIRE(isfinite(Ks[s * 9 + e]), "fp_depth_reproject: Ks[%d] holds a value that is not finite", s);
    for (int e = 0; e < 16; ++e) FP_REQUIRE(isfinite(T_dst_src[s * 16 + e]), "fp_depth_reproject: T_dst_src[%d] holds a value that is not finite", s);
    const Pinhole c = pinhole_of(Ks + s * 9, Hs, Ws);
    const Rigid t = rigid_of(T_dst_src + s * 16);
    bool fits = isfinite(c.fx) && isfinite(c.fy) && isfinite(c.cx) && isfinite(c.cy);      // a finite double can round to an fp32 infinity
    for (float v : t.r) fits = fits && isfinite(v);
    for (float v : t.t) fits = fits && isfinite(v);
    FP_REQUIRE(fits, "fp_depth_reproject: Ks[%d] or T_dst_src[%d] holds a value that is not finite in fp32", s, s);
    FP_REQUIRE(c.fx > 0.f && c.fy > 0.f, "fp_depth_reproject: Ks[%d]: fx, fy must be > 0", s);
  }
  for (int e = 0; e < 9; ++e) FP_REQUIRE(isfinite(K_dst[e]), "fp_depth_reproject: K_dst holds a value that is not finite");
  const Pinhole c = pinhole_of(K_dst, Hd, Wd);
  FP_REQUIRE(isfinite(c.fx) && isfinite(c.fy) && isfinite(c.cx) && isfinite(c.cy), "fp_depth_reproject: K_dst holds a value that is not finite in fp32");
  FP_REQUIRE(c.fx > 0.f && c.fy > 0.f, "fp_depth_reproject: K_dst: fx, fy must be > 0");
  FP_REQUIRE(zfar > 0.f, "fp_depth_reproject: zfar %g (> 0; infinity: no limit)", (double)zfar);      // refuses a NaN too
  FP_REQUIRE((uintptr_t)d_keys % 8 == 0, "fp_depth_reproject: d_keys is not 8-byte aligned");
  return FP_OK;
}

extern "C" int fp_depth_reproject(fp_ctx *ctx, const float *d_depth, int n, int V, int Hs, int Ws, const double *Ks, const double *T_dst_src,
                                  const double *K_dst, int Hd, int Wd, float zfar, uint64_t *d_keys, float *d_depth_out, int32_t *d_source,
                                  void *stream) {
  FP_TRY(fp_depth_reproject_check(ctx, d_depth, n, V, Hs, Ws, Ks, T_dst_src, K_dst, Hd, Wd, zfar, d_keys, d_depth_out));
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  ReprojectViews views{};
  for (int s = 0; s < V; ++s) views.cam[s] = pinhole_of(Ks + s * 9, Hs, Ws), views.to_dst[s] = rigid_of(T_dst_src + s * 16);
  const Pinhole dst = pinhole_of(K_dst, Hd, Wd);
  hipStream_t st = (hipStream_t)stream;
  const size_t target = (size_t)n * Hd * Wd;
  {      // with profiling on, each node has a class of its own (scripts/bench_depth_reproject.py)
    ProfScope node(ctx, st, "reproject_fill", 0.0);
    FP_CHECK_HIP(hipMemsetAsync(d_keys, 0xff, target * sizeof(u64), st));
  }
  {
    ProfScope node(ctx, st, "reproject_scatter", 0.0);
    hipLaunchKernelGGL(reproject_scatter_kernel, dim3(grid_for((long long)Hs * Ws, RP_THREADS).x, (unsigned)V, (unsigned)n), dim3(RP_THREADS), 0, st, views,
                       dst, d_depth, reinterpret_cast<u64 *>(d_keys), zfar);
  }
  {
    ProfScope node(ctx, st, "reproject_finalise", 0.0);
    hipLaunchKernelGGL(reproject_finalise_kernel, dim3(grid_for((long long)Hd * Wd, RP_THREADS).x, (unsigned)n), dim3(RP_THREADS), 0, st,
                       reinterpret_cast<const u64 *>(d_keys), Hd * Wd, d_depth_out, d_source);
  }
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
