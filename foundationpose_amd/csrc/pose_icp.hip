// Polishing object poses against the depth of the frame they are seen in: one Gauss-Newton linearisation of point-to-plane ICP between
// the rendered model and the observed depth for N poses at once (fp_pose_depth_align), the step of every pose on the device
// (fp_pose_gn_step) and the loop of both behind the existing crop-window and render launchers (fp_pose_polish).  The arithmetic is
// stated in include/foundationpose_amd.h and restated in numpy by tests/pose_icp_oracle.py; this file follows it operation for operation
// (the library is built without contraction).
//
// pose_align_kernel is one of the three aligners of gn_sums.h, which holds what they share: the tile, the three passes, the association,
// the point-to-plane row, the 29 sums in double and their way to gn_fold_kernel; the camera is that of view_geom.h.  A workgroup owns
// (pose, a tile of GN_TILE map pixels); the pose is uniform in the workgroup, so its origin arrives as three scalar loads.  Pass one
// reads the model's point and normal (12-byte records, the reads coalesce); pass two projects into the frame and gathers each pixel's
// 16-byte normal and 4-byte depth, all GN_PIX x 2 gathers in flight together; pass three is the arithmetic.  No atomics on the sums.
// A wave whose 256 map pixels are all background (most of a crop's border) writes zero rows and +0.0 sums and skips passes two and
// three.  The two pixel counts are integers: ballots per wave, one pair per workgroup in a slab of their own, added per pose by
// pose_counts_fold_kernel.  No atomics there either, and no memset: every launch writes all it later reads.
//
// pose_gn_step_kernel is one thread per pose in double: the gates of the loop, LDL^T of the damped 6 x 6 system without square roots,
// the pose update.  It exists so that the loop needs no host: nothing synchronises, and the whole of fp_pose_polish can sit in a hipGraph.
#include "common.h"
#include "device_util.h"
#include "gn_sums.h"

#include <math.h>

static_assert(FP_POSE_ALIGN_TERMS == GN_TERMS, "the header's term count is that of gn_accumulate");
static_assert(sizeof(fp_pose_state) == 136, "fp_pose_state is laid out as the header and foundationpose_amd/_lib.py state it");

namespace {

__global__ __launch_bounds__(GN_THREADS) void pose_align_kernel(const float *__restrict__ xyz, const float *__restrict__ normal,
                                                                const float *__restrict__ depth, const float4 *__restrict__ normals, Pinhole cam,
                                                                const float *__restrict__ poses, int hw, int n_tiles, float dist2_max, float cos_min,
                                                                float *__restrict__ rows, double *__restrict__ slab, int *__restrict__ cslab) {
  __shared__ double red[GN_THREADS / 64][GN_TERMS];
  __shared__ int cnt[GN_THREADS / 64][2];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % n_tiles, pr = blockIdx.x / n_tiles;
  const float c0 = poses[(size_t)pr * 16 + 3], c1 = poses[(size_t)pr * 16 + 7], c2 = poses[(size_t)pr * 16 + 11];      // uniform: scalar loads
  const size_t map0 = (size_t)pr * (size_t)hw;

  // pass 1: the model's point and normal in the camera frame
  float y[GN_PIX][3], nm[GN_PIX][3];
  bool ok[GN_PIX];
  int pix[GN_PIX];
#pragma unroll
  for (int q = 0; q < GN_PIX; ++q) {
    pix[q] = tile * GN_TILE + q * GN_THREADS + tid;
    const bool in = pix[q] < hw;                                   // the last tile of a map is ragged
    const float *py = xyz + (map0 + (size_t)(in ? pix[q] : 0)) * 3, *pn = normal + (map0 + (size_t)(in ? pix[q] : 0)) * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      y[q][a] = in ? py[a] : 0.f;
      nm[q][a] = in ? pn[a] : 0.f;
    }
    ok[q] = y[q][2] >= 0.001f;                                     // background is 0; a NaN skips
  }
  int n_rendered = 0, n_observed = 0;                              // of the wave; uniform in it

  // A wave without a single rendered pixel skips the passes below (gn_sums.h).
  if (!gn_empty_wave<8>(ok, rows, map0, pix, hw, red[tid >> 6])) {
    // pass 2: the point's pixel in the frame, the two gathers
    PixelHit h[GN_PIX];
    float dt[GN_PIX];
    float4 nt[GN_PIX];
#pragma unroll
    for (int q = 0; q < GN_PIX; ++q) {
      n_rendered += __popcll(__ballot(ok[q]));
      gn_associate(cam, y[q], ok[q], normals, depth, 0, h[q], nt[q], dt[q]);
    }

    // pass 3: the gates, the row, the sums
    double acc[GN_TERMS];
#pragma unroll
    for (int e = 0; e < GN_TERMS; ++e) acc[e] = 0.0;
#pragma unroll
    for (int q = 0; q < GN_PIX; ++q) {
      bool valid = ok[q] && nt[q].w != 0.f;
      n_observed += __popcll(__ballot(valid));
      float r = gn_plane_residual(cam, valid, y[q], h[q].cf, h[q].rf, dt[q], nt[q], nm[q], dist2_max, cos_min), J[6];
      gn_twist_row(J, nt[q].x, nt[q].y, nt[q].z, y[q][0] - c0, y[q][1] - c1, y[q][2] - c2);
      gn_mask(J, r, valid);
      if (rows && pix[q] < hw) gn_store_row((float4 *)(rows + (map0 + (size_t)pix[q]) * 8), J, r, valid);
      gn_accumulate(acc, J, r, valid);
    }
    gn_wave_to_lds(acc, red[tid >> 6], 0);
  }
  if ((tid & 63) == 0) cnt[tid >> 6][0] = n_rendered, cnt[tid >> 6][1] = n_observed;
  __syncthreads();
  gn_lds_to_slab(red, slab + ((size_t)pr * n_tiles + tile) * GN_TERMS);
  if (cslab && tid < 2) {
    int s = 0;
#pragma unroll
    for (int wv = 0; wv < GN_THREADS / 64; ++wv) s += cnt[wv][tid];
    cslab[((size_t)pr * n_tiles + tile) * 2 + tid] = s;
  }
}

// one thread per (pose, count): the pose's tiles
__global__ __launch_bounds__(64) void pose_counts_fold_kernel(const int *__restrict__ cslab, int N, int n_tiles, int *__restrict__ counts) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= N * 2) return;
  const int *c = cslab + (size_t)(t >> 1) * n_tiles * 2 + (t & 1);
  int s = 0;
  for (int k = 0; k < n_tiles; ++k) s += c[(size_t)k * 2];
  counts[t] = s;
}

// One thread per pose.  Everything in double, in the header's order.
__global__ __launch_bounds__(64) void pose_gn_step_kernel(const double *__restrict__ sums, float *__restrict__ poses, fp_pose_state *__restrict__ state,
                                                          int N, double damping, double min_pixels, int closing, int first) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= N) return;
  fp_pose_state &st = state[i];
  if (first) st = fp_pose_state{};                                 // the first round of fp_pose_polish: whatever the record held, it is fresh
  if (st.stopped != 0) return;                                     // a stopped pose is never touched again
  const double *s = sums + (size_t)i * GN_TERMS;
  float *P = poses + (size_t)i * 16;
  const double count = s[28];
  if (!(count >= min_pixels)) {
    if (st.steps > 0) {
      #pragma unroll
      for (int e = 0; e < 16; ++e) P[e] = st.prev_pose[e];
    } else {                                                       // never moved: the fit on record is this evaluation's
      #pragma unroll
      for (int e = 0; e < 16; ++e) st.prev_pose[e] = P[e];
      st.fit_count = count;
      st.fit_ms = count > 0.0 ? s[27] / count : 0.0;
    }
    st.stopped = FP_POSE_STOP_FEW_PIXELS;
    return;
  }
  const double ms = s[27] / count;
  if (st.steps > 0 && ms > st.fit_ms) {
    #pragma unroll
    for (int e = 0; e < 16; ++e) P[e] = st.prev_pose[e];
    st.stopped = FP_POSE_STOP_RESIDUAL_ROSE;
    return;
  }
  #pragma unroll
  for (int e = 0; e < 16; ++e) st.prev_pose[e] = P[e];
  st.fit_ms = ms;
  st.fit_count = count;
  if (closing) return;

  // M = A + damping trace(A) I, g = -b
  double M[6][6], g[6];
  {
    int e = 0;
    #pragma unroll
    for (int a = 0; a < 6; ++a)
      #pragma unroll
      for (int b = a; b < 6; ++b) M[a][b] = M[b][a] = s[e++];
  }
  const double lam = damping * (((((M[0][0] + M[1][1]) + M[2][2]) + M[3][3]) + M[4][4]) + M[5][5]);
  #pragma unroll
  for (int a = 0; a < 6; ++a) {
    M[a][a] = M[a][a] + lam;
    g[a] = -s[21 + a];
  }
  // M = L D L^T, L unit lower triangular, column by column
  double L[6][6], D[6];
  #pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = M[j][j];
    #pragma unroll
    for (int k = 0; k < j; ++k) d = d - (L[j][k] * D[k]) * L[j][k];
    if (!(d > 0.0)) {
      st.stopped = FP_POSE_STOP_SINGULAR;
      return;
    }
    D[j] = d;
    #pragma unroll
    for (int a = j + 1; a < 6; ++a) {
      double v = M[a][j];
      #pragma unroll
      for (int k = 0; k < j; ++k) v = v - (L[a][k] * D[k]) * L[j][k];
      L[a][j] = v / d;
    }
  }
  double z[6], xi[6];
  #pragma unroll
  for (int a = 0; a < 6; ++a) {
    double v = g[a];
    #pragma unroll
    for (int k = 0; k < a; ++k) v = v - L[a][k] * z[k];
    z[a] = v;
  }
  #pragma unroll
  for (int a = 5; a >= 0; --a) {
    double v = z[a] / D[a];
    #pragma unroll
    for (int k = a + 1; k < 6; ++k) v = v - L[k][a] * xi[k];
    xi[a] = v;
  }
  #pragma unroll
  for (int a = 0; a < 6; ++a) st.xi[a] = xi[a];

  // R <- (I + a [w] + b [w]^2) R, t <- t + tau
  const double w0 = xi[3], w1 = xi[4], w2 = xi[5];
  const double th = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
  double ca, cb;
  if (th < 1e-4) {
    ca = 1.0 - th * th / 6.0;
    cb = 0.5 - th * th / 24.0;
  } else {
    ca = sin(th) / th;
    cb = (1.0 - cos(th)) / (th * th);
  }
  const double Kx[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
  double E[3][3];
  #pragma unroll
  for (int a = 0; a < 3; ++a)
    #pragma unroll
    for (int b = 0; b < 3; ++b) {
      const double k2 = (Kx[a][0] * Kx[0][b] + Kx[a][1] * Kx[1][b]) + Kx[a][2] * Kx[2][b];
      E[a][b] = ((a == b ? 1.0 : 0.0) + ca * Kx[a][b]) + cb * k2;
    }
  float out[12];
  #pragma unroll
  for (int a = 0; a < 3; ++a) {
    #pragma unroll
    for (int b = 0; b < 3; ++b)
      out[a * 4 + b] = (float)((E[a][0] * (double)P[b] + E[a][1] * (double)P[4 + b]) + E[a][2] * (double)P[8 + b]);
    out[a * 4 + 3] = (float)((double)P[a * 4 + 3] + xi[a]);
  }
  #pragma unroll
  for (int e = 0; e < 12; ++e) P[e] = out[e];
  st.steps = st.steps + 1;
}

struct AlignShape {
  Pinhole cam;
  int hw, n_tiles;
};

// the value checks of fp_pose_depth_align that fp_pose_polish shares; nothing here looks into ctx
int align_shape(const char *fn, int N, int h, int w, int H, int W, const double *K, float dist_max, float cos_min, AlignShape &o) {
  FP_REQUIRE(N >= 0 && N <= FP_POSE_ALIGN_MAX_POSES, "%s: N %d (0 .. %d)", fn, N, FP_POSE_ALIGN_MAX_POSES);
  FP_REQUIRE(h >= 1 && w >= 1 && H >= 1 && W >= 1, "%s: map %d x %d, frame %d x %d", fn, h, w, H, W);
  FP_REQUIRE((long long)h * w <= (1 << 24) && (long long)H * W <= (1 << 28), "%s: map %d x %d or frame %d x %d too large", fn, h, w, H, W);
  FP_REQUIRE(dist_max > 0.f, "%s: dist_max %g (> 0)", fn, (double)dist_max);
  FP_REQUIRE(cos_min >= -1.f && cos_min <= 1.f, "%s: cos_min %g (-1 .. 1)", fn, (double)cos_min);
  FP_TRY(fp_check_camera(fn, K));
  o.cam = pinhole_of(K, H, W);
  o.hw = h * w;
  o.n_tiles = (o.hw + GN_TILE - 1) / GN_TILE;      // <= 2^14, times 1024 poses: inside a grid
  return FP_OK;
}

size_t align_slab_bytes(const AlignShape &sh, int N) { return (size_t)N * (size_t)sh.n_tiles * GN_TERMS * sizeof(double); }
size_t align_cslab_bytes(const AlignShape &sh, int N) { return (size_t)N * (size_t)sh.n_tiles * 2 * sizeof(int); }

// the launches of one linearisation; `slab` holds align_slab_bytes and, with `counts`, `cslab` align_cslab_bytes.  With h_sums the sums
// are copied there and the stream is synchronised; without, nothing synchronises
int launch_pose_align(const AlignShape &sh, const float *xyz, const float *normal, const float *depth, const float *normals, const float *poses, int N,
                      float dist_max, float cos_min, float *rows, double *slab, int *cslab, double *sums, int *counts, double *h_sums, hipStream_t s) {
  hipLaunchKernelGGL(pose_align_kernel, dim3((unsigned)(sh.n_tiles * N)), dim3(GN_THREADS), 0, s, xyz, normal, depth, (const float4 *)normals, sh.cam,
                     poses, sh.hw, sh.n_tiles, dist_max * dist_max, cos_min, rows, slab, counts ? cslab : nullptr);
  FP_CHECK_HIP(hipGetLastError());
  if (counts) {
    hipLaunchKernelGGL(pose_counts_fold_kernel, dim3((unsigned)((N * 2 + 63) / 64)), dim3(64), 0, s, (const int *)cslab, N, sh.n_tiles, counts);
    FP_CHECK_HIP(hipGetLastError());
  }
  return gn_fold_to_host<GN_TERMS>(slab, N, sh.n_tiles, sums, h_sums, s);
}

int step_checks(const char *fn, int N, double damping, int min_pixels) {
  FP_REQUIRE(N >= 0 && N <= FP_POSE_ALIGN_MAX_POSES, "%s: N %d (0 .. %d)", fn, N, FP_POSE_ALIGN_MAX_POSES);
  FP_REQUIRE(damping >= 0.0 && isfinite(damping), "%s: damping %g (>= 0, finite)", fn, damping);
  FP_REQUIRE(min_pixels >= 1, "%s: min_pixels %d (>= 1)", fn, min_pixels);
  return FP_OK;
}

int launch_pose_gn_step(const double *sums, float *poses, fp_pose_state *state, int N, double damping, int min_pixels, int closing, int first,
                        hipStream_t s) {
  hipLaunchKernelGGL(pose_gn_step_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, s, sums, poses, state, N, damping, (double)min_pixels,
                     closing ? 1 : 0, first ? 1 : 0);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

}  // namespace

extern "C" int fp_pose_depth_align(fp_ctx *ctx, const float *d_xyz, const float *d_normal, int N, int h, int w, const float *d_depth,
                                   const float *d_normals, int H, int W, const double *K, const float *d_poses, float dist_max, float cos_min,
                                   float *d_rows, double *d_sums, int32_t *d_counts, double *h_sums, void *stream) {
  // Every check of a value comes before the first look INTO ctx: tests/test_pose_icp_host.py calls this without a GPU, with a pointer
  // for ctx that must not be dereferenced.  Keep that order when adding checks.
  FP_REQUIRE(ctx && d_xyz && d_normal && d_depth && d_normals && K && d_poses && d_sums, "fp_pose_depth_align: null argument");
  FP_REQUIRE(((uintptr_t)d_normals & 15) == 0, "fp_pose_depth_align: d_normals is not 16-byte aligned (it is read as float4)");
  FP_REQUIRE(((uintptr_t)d_rows & 15) == 0, "fp_pose_depth_align: d_rows is not 16-byte aligned (it is written as float4)");
  AlignShape sh;
  FP_TRY(align_shape("fp_pose_depth_align", N, h, w, H, W, K, dist_max, cos_min, sh));
  if (N == 0) return FP_OK;
  hipStream_t s = (hipStream_t)stream;
  const size_t slab_bytes = align_slab_bytes(sh, N);
  const size_t cslab_bytes = d_counts ? align_cslab_bytes(sh, N) : 0;
  FP_TRY(fp_arena_ensure(ctx, slab_bytes + cslab_bytes + 4096));
  // the slab goes back to the arena when the launches are queued (with h_sums: synchronised) - the next taker runs behind them on the same stream
  ArenaScope scope(ctx->arena);
  double *slab = (double *)ctx->arena.take(slab_bytes);
  int *cslab = (int *)ctx->arena.take(cslab_bytes);
  FP_REQUIRE(slab && cslab, "fp_pose_depth_align: arena exhausted");
  return launch_pose_align(sh, d_xyz, d_normal, d_depth, d_normals, d_poses, N, dist_max, cos_min, d_rows, slab, cslab, d_sums, d_counts, h_sums, s);
}

extern "C" int fp_pose_gn_step(fp_ctx *ctx, const double *d_sums, float *d_poses, fp_pose_state *d_state, int N, double damping, int min_pixels,
                               int closing, void *stream) {
  // As above: every check of a value before the first look into ctx (which this call never needs).
  FP_REQUIRE(ctx && d_sums && d_poses && d_state, "fp_pose_gn_step: null argument");
  FP_REQUIRE(((uintptr_t)d_state & 7) == 0, "fp_pose_gn_step: d_state is not 8-byte aligned");
  FP_TRY(step_checks("fp_pose_gn_step", N, damping, min_pixels));
  if (N == 0) return FP_OK;
  return launch_pose_gn_step(d_sums, d_poses, d_state, N, damping, min_pixels, closing, 0, (hipStream_t)stream);
}

extern "C" int fp_pose_polish(fp_ctx *ctx, const fp_mesh *mesh, float *d_poses, int N, const double *K, int H, int W, const float *d_depth,
                              const float *d_normals, int crop, double crop_ratio, double mesh_diameter, int iterations, float dist_max,
                              float cos_min, double damping, int min_pixels, fp_pose_state *d_state, double *d_sums, int32_t *d_counts,
                              void *stream) {
  // As above: every check of a value before the first look into ctx or mesh.
  FP_REQUIRE(ctx && mesh && d_poses && K && d_depth && d_normals && d_state && d_sums, "fp_pose_polish: null argument");
  FP_REQUIRE(((uintptr_t)d_normals & 15) == 0, "fp_pose_polish: d_normals is not 16-byte aligned (it is read as float4)");
  FP_REQUIRE(((uintptr_t)d_state & 7) == 0, "fp_pose_polish: d_state is not 8-byte aligned");
  FP_REQUIRE(crop >= 0, "fp_pose_polish: crop %d (0: the full frame)", crop);
  FP_REQUIRE(iterations >= 0 && iterations <= FP_POSE_POLISH_MAX_ITERATIONS, "fp_pose_polish: iterations %d (0 .. %d)", iterations,
             FP_POSE_POLISH_MAX_ITERATIONS);
  FP_REQUIRE(crop == 0 || (crop_ratio > 0 && mesh_diameter > 0 && isfinite(crop_ratio) && isfinite(mesh_diameter)),
             "fp_pose_polish: crop_ratio %g, mesh_diameter %g (> 0, finite)", crop_ratio, mesh_diameter);
  const int h = crop ? crop : H, w = crop ? crop : W;
  AlignShape sh;
  FP_TRY(align_shape("fp_pose_polish", N, h, w, H, W, K, dist_max, cos_min, sh));
  FP_TRY(step_checks("fp_pose_polish", N, damping, min_pixels));
  if (N == 0) return FP_OK;
  hipStream_t s = (hipStream_t)stream;
  const MeshDev &md = mesh->d;
  FP_REQUIRE(render_fits(N, md.V, md.F, h, w, ctx->num_cu), "fp_pose_polish: the rasteriser does not take maps of %d x %d", h, w);
  const size_t map_bytes = (size_t)N * sh.hw * 3 * sizeof(float), slab_bytes = align_slab_bytes(sh, N), cslab_bytes = align_cslab_bytes(sh, N);
  const size_t rs_bytes = render_scratch_bytes(N, md.V, md.F, h, w, ctx->num_cu);
  FP_TRY(fp_arena_ensure(ctx, 2 * map_bytes + slab_bytes + cslab_bytes + rs_bytes + (size_t)N * 13 * sizeof(float) + 8 * 256 + 4096));
  // everything taken goes back when the launches are queued - the next taker runs behind them on the same stream
  ArenaScope scope(ctx->arena);
  float *xyz = (float *)ctx->arena.take(map_bytes), *nrm = (float *)ctx->arena.take(map_bytes);
  double *slab = (double *)ctx->arena.take(slab_bytes);
  int *cslab = (int *)ctx->arena.take(cslab_bytes);
  float *tf = (float *)ctx->arena.take((size_t)N * 9 * sizeof(float)), *bbox = (float *)ctx->arena.take((size_t)N * 4 * sizeof(float));
  void *rs = ctx->arena.take(rs_bytes);
  FP_REQUIRE(xyz && nrm && slab && cslab && tf && bbox && rs, "fp_pose_polish: arena exhausted");
  RenderArgs a;
  memset(&a, 0, sizeof(a));
  a.mesh = md;
  a.poses = d_poses;
  a.bbox2d = crop ? bbox : nullptr;
  for (int i = 0; i < 9; ++i) a.K[i] = K[i];
  a.N = N, a.H = H, a.W = W, a.Ho = h, a.Wo = w;
  a.w_ambient = 0.8f, a.w_diffuse = 0.5f;
  a.normal = nrm, a.xyz = xyz;
  a.scratch = rs, a.scratch_bytes = rs_bytes;
  for (int it = 0; it <= iterations; ++it) {
    if (crop) FP_TRY(launch_crop_window_tf(d_poses, N, K, crop_ratio, mesh_diameter, w, h, tf, bbox, s));
    FP_TRY(launch_render(ctx, a, s));
    FP_TRY(launch_pose_align(sh, xyz, nrm, d_depth, d_normals, d_poses, N, dist_max, cos_min, nullptr, slab, cslab, d_sums, d_counts, nullptr, s));
    FP_TRY(launch_pose_gn_step(d_sums, d_poses, d_state, N, damping, min_pixels, it == iterations, it == 0, s));      // round 0 starts fresh records
  }
  return FP_OK;
}
