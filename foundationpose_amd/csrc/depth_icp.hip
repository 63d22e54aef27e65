// Posing reference views from depth alone: normals of depth maps (fp_depth_normals) and one Gauss-Newton linearisation of point-to-plane
// ICP between pairs of depth maps with projective association (fp_depth_pairs_align).  The arithmetic is stated in
// include/foundationpose_amd.h and restated in numpy by tests/depth_icp_oracle.py; this file follows it operation for operation (the
// library is built without contraction).  The joint solve over all views is the caller's (foundationpose_amd/reconstruct.py).
//
// Both kernels move memory.  The normals kernel is one thread per pixel: five depth reads (the pixel and its four neighbours, the rows
// above and below come from L2) and one 16-byte write.  The pairs kernel is one of the three aligners of gn_sums.h, which holds what they
// share: the tile, the three passes, the association, the point-to-plane row, the 29 sums in double and their way to gn_fold_kernel;
// the camera and the transforms are those of view_geom.h.  A workgroup owns (pair, a tile of GN_TILE source pixels); the pair is uniform
// in the workgroup, so its matrices arrive as scalar loads from the pair table.  Pass one reads the source normal and depth (the reads
// coalesce); pass two projects into the target and gathers each pixel's 16-byte normal and 4-byte depth, all GN_PIX x 2 gathers in
// flight together; pass three is the arithmetic.  No atomics.  A wave whose 256 source pixels have no normal (the background of a
// masked view) skips passes two and three.
//
// The photometric term (fp_view_intensity, fp_depth_pairs_align_photo) rides on the same association.  view_intensity_kernel is one thread
// per pixel again: the pixel's normal, the rgb of the pixel and of its four neighbours where the normal is there, one 16-byte write.
// depth_pairs_kernel<true> is the same body with one more 16-byte source read in pass one and one more 16-byte gather in pass two; it keeps
// what the photometric row needs of a pixel (x, y, the sub-pixel offset, the two intensity records, the geometric verdict) and sweeps the
// pixels a second time after the 29 geometric sums have gone through the wave into LDS, so that only 29 double accumulators are alive at
// a time; the workgroup's slot then holds 58 numbers.  depth_pairs_kernel<false> is the geometric kernel, statement for statement.
#include "common.h"
#include "device_util.h"
#include "gn_sums.h"

#include <math.h>

namespace {

constexpr int PX_THREADS = 256;      // the two kernels of one thread per pixel

// what a pair (s, t) needs of its two views, as fp32
struct PairRec {
  Rigid cs;                  // C_s: camera s -> object
  Rigid it;                  // D_t: object -> camera t
  float rct[9];              // the rotation of C_t
  int s, t, pad;
};
static_assert(sizeof(PairRec) == 144, "the pair table is read as scalar loads of this layout");

__global__ __launch_bounds__(PX_THREADS) void depth_normals_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask, Pinhole cam,
                                                                   float zfar, float max_jump, long long total, float4 *__restrict__ out) {
  const long long idx = (long long)blockIdx.x * PX_THREADS + threadIdx.x;
  if (idx >= total) return;
  const long long hw = (long long)cam.H * cam.W;
  const long long pix = idx % hw;
  const int r = (int)(pix / cam.W), c = (int)(pix - (long long)r * cam.W);
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (r >= 1 && r <= cam.H - 2 && c >= 1 && c <= cam.W - 2) {      // the four neighbours are pixels of the same view
    const float d = depth[idx], dl = depth[idx - 1], dr = depth[idx + 1], du = depth[idx - cam.W], dd = depth[idx + cam.W];
    bool ok = depth_ok(d, zfar) && depth_ok(dl, zfar) && depth_ok(dr, zfar) && depth_ok(du, zfar) && depth_ok(dd, zfar);
    if (mask) ok = ok && mask[idx] != 0 && mask[idx - 1] != 0 && mask[idx + 1] != 0 && mask[idx - cam.W] != 0 && mask[idx + cam.W] != 0;
    ok = ok && fabsf(dl - d) <= max_jump && fabsf(dr - d) <= max_jump && fabsf(du - d) <= max_jump && fabsf(dd - d) <= max_jump;
    if (ok) {
      const float kl = pinhole_ray_x(cam, (float)(c - 1)), kr = pinhole_ray_x(cam, (float)(c + 1)), kc = pinhole_ray_x(cam, (float)c);
      const float ku = pinhole_ray_y(cam, (float)(r - 1)), kd = pinhole_ray_y(cam, (float)(r + 1)), km = pinhole_ray_y(cam, (float)r);
      const float ax = kr * dr - kl * dl, ay = km * dr - km * dl, az = dr - dl;      // p(r,c+1) - p(r,c-1)
      const float bx = kc * dd - kc * du, by = kd * dd - ku * du, bz = dd - du;      // p(r+1,c) - p(r-1,c)
      const float mx = by * az - bz * ay, my = bz * ax - bx * az, mz = bx * ay - by * ax;
      const float l2 = (mx * mx + my * my) + mz * mz;
      if (l2 > 0.f) {
        const float l = sqrtf(l2);
        o = make_float4(mx / l, my / l, mz / l, 1.f);
      }
    }
  }
  out[idx] = o;
}

// I = ((0.299 R + 0.587 G) + 0.114 B) / 255 of one pixel
__device__ __forceinline__ float grey(const uint8_t *__restrict__ rgb, long long idx) {
  const uint8_t *p = rgb + (size_t)idx * 3;
  return ((0.299f * (float)p[0] + 0.587f * (float)p[1]) + 0.114f * (float)p[2]) / 255.f;
}

__global__ __launch_bounds__(PX_THREADS) void view_intensity_kernel(const uint8_t *__restrict__ rgb, const float4 *__restrict__ normals, int H, int W,
                                                                    long long total, float4 *__restrict__ out) {
  const long long idx = (long long)blockIdx.x * PX_THREADS + threadIdx.x;
  if (idx >= total) return;
  const long long hw = (long long)H * W;
  const long long pix = idx % hw;
  const int r = (int)(pix / W), c = (int)(pix - (long long)r * W);
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  // a normal of fp_depth_normals is never on the border; the test keeps the four neighbours inside the view for any other map
  if (r >= 1 && r <= H - 2 && c >= 1 && c <= W - 2 && normals[idx].w != 0.f)
    o = make_float4(grey(rgb, idx), (grey(rgb, idx + 1) - grey(rgb, idx - 1)) * 0.5f, (grey(rgb, idx + W) - grey(rgb, idx - W)) * 0.5f, 1.f);
  out[idx] = o;
}

// PHOTO: the photometric rows and their 29 sums behind the geometric ones (the header's second rule); `intensity` and i_max are not
// looked at without it.
template <bool PHOTO>
__global__ __launch_bounds__(GN_THREADS) void depth_pairs_kernel(const float *__restrict__ depth, const float4 *__restrict__ normals,
                                                                 const float4 *__restrict__ intensity, Pinhole cam,
                                                                 const PairRec *__restrict__ recs, int n_tiles, float dist2_max, float cos_min,
                                                                 float i_max, float *__restrict__ rows, double *__restrict__ slab) {
  constexpr int TERMS = PHOTO ? FP_PHOTO_ALIGN_TERMS : FP_DEPTH_ALIGN_TERMS;
  constexpr int ROW = PHOTO ? 16 : 8;                               // floats per pixel of `rows`
  __shared__ double red[GN_THREADS / 64][TERMS];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % n_tiles, pr = blockIdx.x / n_tiles;
  const PairRec &m = recs[pr];
  const long long hw = (long long)cam.H * cam.W;
  const size_t src0 = (size_t)m.s * (size_t)hw, tgt0 = (size_t)m.t * (size_t)hw;      // 0 <= s, t < n_views: checked on the host

  // pass 1: the source pixel's normal and depth
  float d[GN_PIX];
  float4 ns[GN_PIX];
  bool ok[GN_PIX];
  long long pix[GN_PIX];
  float4 ia[GN_PIX];                                               // PHOTO: the source pixel's intensity record
#pragma unroll
  for (int q = 0; q < GN_PIX; ++q) {
    pix[q] = (long long)tile * GN_TILE + q * GN_THREADS + tid;
    const bool in = pix[q] < hw;                                   // the last tile of a view is ragged
    ns[q] = in ? normals[src0 + (size_t)pix[q]] : make_float4(0.f, 0.f, 0.f, 0.f);
    d[q] = in ? depth[src0 + (size_t)pix[q]] : 0.f;
    if constexpr (PHOTO) ia[q] = in ? intensity[src0 + (size_t)pix[q]] : make_float4(0.f, 0.f, 0.f, 0.f);
    ok[q] = ns[q].w != 0.f;
  }

  // A wave without a single source normal - most waves of a masked object's view - skips the passes below (gn_sums.h).
  if (!gn_empty_wave<ROW>(ok, rows, (size_t)pr * (size_t)hw, pix, hw, red[tid >> 6])) {
  // pass 2: the point in the object frame and in camera t, its pixel there, the two gathers
  float x[GN_PIX][3], y[GN_PIX][3], cf[GN_PIX], rf[GN_PIX], dt[GN_PIX];
  float4 nt[GN_PIX];
  float4 ib[GN_PIX];                                               // PHOTO: the target pixel's intensity record,
  float du[GN_PIX], dv[GN_PIX];                                    // the projection's offset from that pixel's centre,
  bool geo[GN_PIX];                                                // and whether the pixel passed every geometric gate
#pragma unroll
  for (int q = 0; q < GN_PIX; ++q) {
    const int row = (int)(pix[q] / cam.W), col = (int)(pix[q] - (long long)row * cam.W);
    const float3 p = pinhole_point(cam, (float)col, (float)row, d[q]);
#pragma unroll
    for (int a = 0; a < 3; ++a) x[q][a] = rigid_apply(m.cs, a, p.x, p.y, p.z);
#pragma unroll
    for (int a = 0; a < 3; ++a) y[q][a] = rigid_apply(m.it, a, x[q][0], x[q][1], x[q][2]);
    ok[q] = ok[q] && y[q][2] >= 0.001f;
    PixelHit h;
    const size_t tp = gn_associate(cam, y[q], ok[q], normals, depth, tgt0, h, nt[q], dt[q]);
    cf[q] = h.cf, rf[q] = h.rf;
    if constexpr (PHOTO) {
      ib[q] = ok[q] ? intensity[tp] : make_float4(0.f, 0.f, 0.f, 0.f);
      du[q] = h.u - cf[q], dv[q] = h.v - rf[q];
    }
  }

  // pass 3: the gates, the row, the sums
  double acc[GN_TERMS];
#pragma unroll
  for (int e = 0; e < GN_TERMS; ++e) acc[e] = 0.0;
#pragma unroll
  for (int q = 0; q < GN_PIX; ++q) {
    bool valid = ok[q] && nt[q].w != 0.f;
    float w[3], g[3], no[3], J[6];                                 // the source normal in the object frame and in camera t
#pragma unroll
    for (int a = 0; a < 3; ++a) w[a] = rigid_rotate(m.cs, a, ns[q].x, ns[q].y, ns[q].z);
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = rigid_rotate(m.it, a, w[0], w[1], w[2]);
    float r = gn_plane_residual(cam, valid, y[q], cf[q], rf[q], dt[q], nt[q], g, dist2_max, cos_min);
#pragma unroll
    for (int a = 0; a < 3; ++a) no[a] = mat3_row(m.rct, a, nt[q].x, nt[q].y, nt[q].z);
    gn_twist_row(J, no[0], no[1], no[2], x[q][0], x[q][1], x[q][2]);
    gn_mask(J, r, valid);
    if (rows && pix[q] < hw) gn_store_row((float4 *)(rows + ((size_t)pr * (size_t)hw + (size_t)pix[q]) * ROW), J, r, valid);
    if constexpr (PHOTO) geo[q] = valid;
    gn_accumulate(acc, J, r, valid);
  }
  gn_wave_to_lds(acc, red[tid >> 6], 0);

  // pass 4 (PHOTO): the photometric row and its sums, the 29 accumulators used again
  if constexpr (PHOTO) {
#pragma unroll
    for (int e = 0; e < GN_TERMS; ++e) acc[e] = 0.0;
#pragma unroll
    for (int q = 0; q < GN_PIX; ++q) {
      bool valid = geo[q] && ia[q].w != 0.f && ib[q].w != 0.f;
      float r = ((ib[q].x + ib[q].y * du[q]) + ib[q].z * dv[q]) - ia[q].x;
      valid = valid && fabsf(r) < i_max;
      const float jx = (ib[q].y * cam.fx) / y[q][2], jy = (ib[q].z * cam.fy) / y[q][2];
      const float jz = -((jx * y[q][0] + jy * y[q][1]) / y[q][2]);
      float a[3], J[6];
#pragma unroll
      for (int k = 0; k < 3; ++k) a[k] = mat3_row(m.rct, k, jx, jy, jz);
      gn_twist_row(J, a[0], a[1], a[2], x[q][0], x[q][1], x[q][2]);
      gn_mask(J, r, valid);
      if (rows && pix[q] < hw) gn_store_row((float4 *)(rows + ((size_t)pr * (size_t)hw + (size_t)pix[q]) * ROW) + 2, J, r, valid);
      gn_accumulate(acc, J, r, valid);
    }
    gn_wave_to_lds(acc, red[tid >> 6], GN_TERMS);
  }
  }
  __syncthreads();
  gn_lds_to_slab(red, slab + ((size_t)pr * n_tiles + tile) * TERMS);
}

}  // namespace

extern "C" int fp_depth_normals(fp_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int n_views, int H, int W, const double *K, float zfar,
                                float max_jump, float *d_normals, void *stream) {
  // Every check of a value comes before the first look INTO ctx: tests/test_depth_icp_host.py calls this without a GPU, with a pointer
  // for ctx that must not be dereferenced.  Keep that order when adding checks.
  FP_REQUIRE(ctx && d_depth && K && d_normals, "fp_depth_normals: null argument");
  FP_REQUIRE(((uintptr_t)d_normals & 15) == 0, "fp_depth_normals: d_normals is not 16-byte aligned (it is written as float4)");
  FP_REQUIRE(n_views >= 0 && n_views <= FP_TSDF_MAX_VIEWS, "fp_depth_normals: n_views %d (0 .. %d)", n_views, FP_TSDF_MAX_VIEWS);
  FP_REQUIRE(H >= 1 && W >= 1, "fp_depth_normals: H %d, W %d", H, W);
  FP_REQUIRE(zfar > 0.f, "fp_depth_normals: zfar %g (> 0)", (double)zfar);
  FP_REQUIRE(max_jump > 0.f, "fp_depth_normals: max_jump %g (> 0)", (double)max_jump);
  FP_TRY(fp_check_camera("fp_depth_normals", K));
  const Pinhole cam = pinhole_of(K, H, W);
  const long long total = (long long)n_views * H * W;
  const long long blocks = (total + PX_THREADS - 1) / PX_THREADS;
  FP_REQUIRE(blocks <= 0x7fffffff, "fp_depth_normals: %d views of %d x %d pixels are too many for one launch", n_views, H, W);
  if (n_views == 0) return FP_OK;
  hipLaunchKernelGGL(depth_normals_kernel, dim3((unsigned)blocks), dim3(PX_THREADS), 0, (hipStream_t)stream, d_depth, d_mask, cam, zfar, max_jump,
                     total, (float4 *)d_normals);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

namespace {

// fp_depth_pairs_align (d_intensity null) and fp_depth_pairs_align_photo (d_intensity given): the same checks, pair table, slab and fold,
// with 29 or 58 numbers per pair and rows of 8 or 16 floats.  `fn` names the entry point in the messages.
int pairs_align(const char *fn, fp_ctx *ctx, const float *d_depth, const float *d_normals, const float *d_intensity, bool photo, int n_views, int H,
                int W, const double *K, const double *cam_in_ob, const int32_t *pairs, int n_pairs, float dist_max, float cos_min, float i_max,
                float *d_rows, double *h_sums, void *stream) {
  // As above: every check of a value before the first look into ctx.
  FP_REQUIRE(ctx && d_depth && d_normals && K && cam_in_ob && h_sums && (d_intensity || !photo), "%s: null argument", fn);
  FP_REQUIRE(((uintptr_t)d_normals & 15) == 0, "%s: d_normals is not 16-byte aligned (it is read as float4)", fn);
  FP_REQUIRE(((uintptr_t)d_intensity & 15) == 0, "%s: d_intensity is not 16-byte aligned (it is read as float4)", fn);
  FP_REQUIRE(((uintptr_t)d_rows & 15) == 0, "%s: d_rows is not 16-byte aligned (it is written as float4)", fn);
  FP_REQUIRE(n_views >= 0 && n_views <= FP_TSDF_MAX_VIEWS, "%s: n_views %d (0 .. %d)", fn, n_views, FP_TSDF_MAX_VIEWS);
  FP_REQUIRE(n_pairs >= 0 && n_pairs <= FP_DEPTH_ALIGN_MAX_PAIRS, "%s: n_pairs %d (0 .. %d)", fn, n_pairs, FP_DEPTH_ALIGN_MAX_PAIRS);
  FP_REQUIRE(pairs || n_pairs == 0, "%s: null pairs", fn);
  FP_REQUIRE(H >= 1 && W >= 1, "%s: H %d, W %d", fn, H, W);
  FP_REQUIRE(dist_max > 0.f, "%s: dist_max %g (> 0)", fn, (double)dist_max);
  FP_REQUIRE(cos_min >= -1.f && cos_min <= 1.f, "%s: cos_min %g (-1 .. 1)", fn, (double)cos_min);
  FP_REQUIRE(!photo || i_max > 0.f, "%s: i_max %g (> 0)", fn, (double)i_max);
  FP_TRY(fp_check_camera(fn, K));
  FP_TRY(fp_check_view_matrices(fn, cam_in_ob, n_views));
  const Pinhole cam = pinhole_of(K, H, W);
  std::vector<PairRec> recs((size_t)n_pairs);
  for (int p = 0; p < n_pairs; ++p) {
    const int s = pairs[2 * p], t = pairs[2 * p + 1];
    FP_REQUIRE(s >= 0 && s < n_views && t >= 0 && t < n_views, "%s: pair %d = (%d, %d) of %d views", fn, p, s, t, n_views);
    FP_REQUIRE(s != t, "%s: pair %d joins view %d to itself", fn, p, s);
    const double *ms = cam_in_ob + (size_t)s * 16, *mt = cam_in_ob + (size_t)t * 16;
    PairRec &r = recs[p];
    r.cs = rigid_of(ms), r.it = rigid_inverse_of(mt);
    memcpy(r.rct, rigid_of(mt).r, sizeof(r.rct));
    r.s = s, r.t = t, r.pad = 0;
  }
  const long long n_tiles = ((long long)H * W + GN_TILE - 1) / GN_TILE;
  FP_REQUIRE(n_tiles * FP_DEPTH_ALIGN_MAX_PAIRS <= 0x7fffffff, "%s: %d x %d pixels are too many for one launch", fn, H, W);
  if (n_pairs == 0) return FP_OK;
  hipStream_t s = (hipStream_t)stream;
  const size_t terms = photo ? FP_PHOTO_ALIGN_TERMS : FP_DEPTH_ALIGN_TERMS;
  const size_t slab_bytes = (size_t)n_pairs * (size_t)n_tiles * terms * sizeof(double);
  const size_t sums_bytes = (size_t)n_pairs * terms * sizeof(double);
  const size_t recs_bytes = (size_t)n_pairs * sizeof(PairRec);
  FP_TRY(fp_arena_ensure(ctx, slab_bytes + sums_bytes + recs_bytes + 4096));
  ArenaScope scope(ctx->arena);
  double *slab = (double *)ctx->arena.take(slab_bytes);
  double *sums = (double *)ctx->arena.take(sums_bytes);
  PairRec *d_recs = (PairRec *)ctx->arena.take(recs_bytes);
  FP_REQUIRE(slab && sums && d_recs, "%s: arena exhausted", fn);
  // `recs` outlives the copy: the stream is synchronised before this returns
  FP_CHECK_HIP(hipMemcpyAsync(d_recs, recs.data(), recs_bytes, hipMemcpyHostToDevice, s));
  const dim3 grid((unsigned)(n_tiles * n_pairs));
  // the slab, the sums and the pair table go back to the arena, and `recs` goes, when this returns: gn_fold_to_host has synchronised by then
  if (photo) {
    hipLaunchKernelGGL(depth_pairs_kernel<true>, grid, dim3(GN_THREADS), 0, s, d_depth, (const float4 *)d_normals, (const float4 *)d_intensity, cam,
                       (const PairRec *)d_recs, (int)n_tiles, dist_max * dist_max, cos_min, i_max, d_rows, slab);
    FP_CHECK_HIP(hipGetLastError());
    return gn_fold_to_host<FP_PHOTO_ALIGN_TERMS>(slab, n_pairs, (int)n_tiles, sums, h_sums, s);
  }
  hipLaunchKernelGGL(depth_pairs_kernel<false>, grid, dim3(GN_THREADS), 0, s, d_depth, (const float4 *)d_normals, (const float4 *)nullptr, cam,
                     (const PairRec *)d_recs, (int)n_tiles, dist_max * dist_max, cos_min, 0.f, d_rows, slab);
  FP_CHECK_HIP(hipGetLastError());
  return gn_fold_to_host<FP_DEPTH_ALIGN_TERMS>(slab, n_pairs, (int)n_tiles, sums, h_sums, s);
}

}  // namespace

extern "C" int fp_depth_pairs_align(fp_ctx *ctx, const float *d_depth, const float *d_normals, int n_views, int H, int W, const double *K,
                                    const double *cam_in_ob, const int32_t *pairs, int n_pairs, float dist_max, float cos_min, float *d_rows,
                                    double *h_sums, void *stream) {
  return pairs_align("fp_depth_pairs_align", ctx, d_depth, d_normals, nullptr, false, n_views, H, W, K, cam_in_ob, pairs, n_pairs, dist_max, cos_min,
                     0.f, d_rows, h_sums, stream);
}

extern "C" int fp_depth_pairs_align_photo(fp_ctx *ctx, const float *d_depth, const float *d_normals, const float *d_intensity, int n_views, int H, int W,
                                          const double *K, const double *cam_in_ob, const int32_t *pairs, int n_pairs, float dist_max, float cos_min,
                                          float i_max, float *d_rows, double *h_sums, void *stream) {
  return pairs_align("fp_depth_pairs_align_photo", ctx, d_depth, d_normals, d_intensity, true, n_views, H, W, K, cam_in_ob, pairs, n_pairs, dist_max,
                     cos_min, i_max, d_rows, h_sums, stream);
}

extern "C" int fp_view_intensity(fp_ctx *ctx, const uint8_t *d_rgb, const float *d_normals, int n_views, int H, int W, float *d_intensity, void *stream) {
  // As above: every check of a value before the first look into ctx.
  FP_REQUIRE(ctx && d_rgb && d_normals && d_intensity, "fp_view_intensity: null argument");
  FP_REQUIRE(((uintptr_t)d_normals & 15) == 0, "fp_view_intensity: d_normals is not 16-byte aligned (it is read as float4)");
  FP_REQUIRE(((uintptr_t)d_intensity & 15) == 0, "fp_view_intensity: d_intensity is not 16-byte aligned (it is written as float4)");
  FP_REQUIRE(n_views >= 0 && n_views <= FP_TSDF_MAX_VIEWS, "fp_view_intensity: n_views %d (0 .. %d)", n_views, FP_TSDF_MAX_VIEWS);
  FP_REQUIRE(H >= 1 && W >= 1, "fp_view_intensity: H %d, W %d", H, W);
  const long long total = (long long)n_views * H * W;
  const long long blocks = (total + PX_THREADS - 1) / PX_THREADS;
  FP_REQUIRE(blocks <= 0x7fffffff, "fp_view_intensity: %d views of %d x %d pixels are too many for one launch", n_views, H, W);
  if (n_views == 0) return FP_OK;
  hipLaunchKernelGGL(view_intensity_kernel, dim3((unsigned)blocks), dim3(PX_THREADS), 0, (hipStream_t)stream, d_rgb, (const float4 *)d_normals, H, W,
                     total, (float4 *)d_intensity);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
