// The two ends of a Gauss-Newton linearisation kernel (tsdf_align_kernel in tsdf.hip, both passes of depth_pairs_kernel in depth_icp.hip,
// pose_align_kernel in pose_icp.hip).  The back end: the row of a pixel and the 29 sums of an item - a view, a pair or a pose: the 21
// entries of the upper triangle of J^T J row by row, the 6 of J^T r, r^2 and the number of valid pixels - and the host's tail behind
// the kernel (gn_fold_to_host).  The front end: the tile (GN_THREADS, GN_PIX, GN_TILE), the empty-wave shortcut, and for the two
// kernels with projective association the association step, the point-to-plane gates and residual, and the twist row; the camera and
// the transforms are those of view_geom.h.  The device functions are __forceinline__.
//
// The summation order is part of the documented results ("a pair does not depend on its batch", "terms 0..28 are bit-identical to the
// geometric call"); tests/gn_sums_oracle.py restates it and the GPU tests hold the kernels to it bit for bit.  A workgroup of GN_THREADS
// threads (WAVES waves) owns a tile of GN_TILE = GN_PIX x GN_THREADS pixels of one item; the pixels past the item's last one are zero rows.
//   1. Pixel tile * GN_TILE + q * GN_THREADS + tid belongs to lane tid.
//   2. A lane starts every sum at +0.0 and adds its pixels q = 0 .. GN_PIX - 1 in that order (gn_accumulate): J and r widened to double, a
//      product, an add - the library is built without contraction.  The count adds 1.0 for a valid pixel; an invalid pixel is a zero row
//      (gn_mask) and adds +0.0 to everything.
//   3. Over the 64 lanes of a wave: wave_sum's butterfly, partner distance 32, 16, .. 1, s = s + s[lane ^ o]; every lane ends with the
//      same value and lane 0 writes it to LDS (gn_wave_to_lds).
//   4. After the kernel's barrier thread `term` adds the waves from wave 0 up, red[0] + red[1] + .., and writes the workgroup's own slot of
//      the slab (gn_lds_to_slab).  No atomics.
//   5. gn_fold_kernel: one thread per (item, term) adds the item's slots from 0.0 in tile order.
//
// The kernels take their pixels in three passes: what a pixel reads of its own item; then the address and the gathers of every pixel -
// nothing in this pass depends on a gathered value, so all of a lane's gathers are in flight together (gn_associate is that pass's body
// and uses nothing it loads); then the arithmetic.
#pragma once
#include "device_util.h"
#include "view_geom.h"

constexpr int GN_TERMS = 29;
constexpr int GN_THREADS = 256;
constexpr int GN_PIX = 4;
constexpr int GN_TILE = GN_THREADS * GN_PIX;      // 1024 pixels per workgroup
static_assert(FP_TSDF_ALIGN_TERMS == GN_TERMS && FP_DEPTH_ALIGN_TERMS == GN_TERMS && FP_PHOTO_ALIGN_TERMS == 2 * GN_TERMS,
              "the header's term counts are those of gn_accumulate");

// a pixel that is not valid has a zero row
__device__ __forceinline__ void gn_mask(float (&J)[6], float &r, bool valid) {
  if (!valid) {
#pragma unroll
    for (int i = 0; i < 6; ++i) J[i] = 0.f;
    r = 0.f;
  }
}

// the row as the header lays it out: J0 .. J5, r, valid, as two 16-byte stores
__device__ __forceinline__ void gn_store_row(float4 *o, const float (&J)[6], float r, bool valid) {
  o[0] = make_float4(J[0], J[1], J[2], J[3]);
  o[1] = make_float4(J[4], J[5], r, valid ? 1.f : 0.f);
}

__device__ __forceinline__ void gn_accumulate(double (&acc)[GN_TERMS], const float (&J)[6], float r, bool valid) {
  double Jd[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) Jd[i] = (double)J[i];
  const double rd = (double)r;
  int e = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) acc[e++] += Jd[i] * Jd[j];
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[21 + i] += Jd[i] * rd;
  acc[27] += rd * rd;
  acc[28] += valid ? 1.0 : 0.0;
}

// the row of a twist (translation, rotation about the origin X is measured from): J = {n, X x n}
__device__ __forceinline__ void gn_twist_row(float (&J)[6], float nx, float ny, float nz, float X, float Y, float Z) {
  J[0] = nx, J[1] = ny, J[2] = nz;
  J[3] = Y * nz - Z * ny, J[4] = Z * nx - X * nz, J[5] = X * ny - Y * nx;
}

// A wave none of whose pixels is `ok` after pass one has nothing to project: its rows (ROW floats a pixel, from pixel item0 of `rows`) are
// zeros and its TERMS partial sums are +0.0, the value the passes would arrive at (0.f x 0.f widened and added to +0.0).  True when the
// wave was such a wave and is done; uniform in the wave.
template <int ROW, int TERMS, typename I>
__device__ __forceinline__ bool gn_empty_wave(const bool (&ok)[GN_PIX], float *__restrict__ rows, size_t item0, const I (&pix)[GN_PIX], I hw,
                                              double (&red_row)[TERMS]) {
  static_assert(GN_PIX == 4 && ROW % 4 == 0 && TERMS <= 64, "four pixels a lane, rows of float4, one lane per term");
  if (__any(ok[0] || ok[1] || ok[2] || ok[3])) return false;
  if (rows) {
#pragma unroll
    for (int q = 0; q < GN_PIX; ++q)
      if (pix[q] < hw) {
        float4 *o = (float4 *)(rows + (item0 + (size_t)pix[q]) * ROW);
#pragma unroll
        for (int k = 0; k < ROW / 4; ++k) o[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
  }
  if ((threadIdx.x & 63) < TERMS) red_row[threadIdx.x & 63] = 0.0;
  return true;
}

// Projective association of the point y (camera frame of the target) with the target view that starts at pixel view0 of `normals` and
// `depth`: the ICP rule of view_geom.h, ok = ok and in frame, the gathers of the pixel's normal and depth (zeros where not ok).  Returns
// the pixel's index for whatever else the caller gathers there; inside the view whenever ok.
__device__ __forceinline__ size_t gn_associate(const Pinhole &cam, const float (&y)[3], bool &ok, const float4 *__restrict__ normals,
                                               const float *__restrict__ depth, size_t view0, PixelHit &h, float4 &nt, float &dt) {
  h = project_icp(cam, y[0], y[1], y[2]);
  ok = ok && h.in;
  const size_t tp = view0 + (ok ? (size_t)(int)h.rf * cam.W + (size_t)(int)h.cf : 0);
  nt = ok ? normals[tp] : make_float4(0.f, 0.f, 0.f, 0.f);
  dt = ok ? depth[tp] : 0.f;
  return tp;
}

// The point-to-plane gates and residual of an associated pixel: e = y - (the pixel (cf, rf) at the gathered depth), valid = valid and
// |e|^2 < dist2_max and g . n >= cos_min, r = n . e.  n is the gathered normal, g the source normal in the target's camera frame; `valid`
// comes in as ok and nt.w != 0.
__device__ __forceinline__ float gn_plane_residual(const Pinhole &cam, bool &valid, const float (&y)[3], float cf, float rf, float dt, float4 nt,
                                                   const float (&g)[3], float dist2_max, float cos_min) {
  const float3 p = pinhole_point(cam, cf, rf, dt);
  const float ex = y[0] - p.x, ey = y[1] - p.y, ez = y[2] - p.z;
  valid = valid && (ex * ex + ey * ey) + ez * ez < dist2_max;
  valid = valid && (g[0] * nt.x + g[1] * nt.y) + g[2] * nt.z >= cos_min;
  return (nt.x * ex + nt.y * ey) + nt.z * ez;
}

// the wave's 29 sums to red_row[offset .. offset + 28], the wave's row of the workgroup's LDS array
template <int TERMS_PER_SLOT>
__device__ __forceinline__ void gn_wave_to_lds(const double (&acc)[GN_TERMS], double (&red_row)[TERMS_PER_SLOT], int offset) {
  static_assert(TERMS_PER_SLOT % GN_TERMS == 0, "a slot holds whole sets of sums");
#pragma unroll
  for (int e = 0; e < GN_TERMS; ++e) {
    const double s = wave_sum(acc[e]);
    if ((threadIdx.x & 63) == 0) red_row[offset + e] = s;
  }
}

// after the barrier behind the last gn_wave_to_lds: the waves in wave order, to the workgroup's slot of the slab
template <int WAVES, int TERMS>
__device__ __forceinline__ void gn_lds_to_slab(const double (&red)[WAVES][TERMS], double *__restrict__ slab_slot) {
  const int term = threadIdx.x;
  if (term < TERMS) {
    double s = red[0][term];
    for (int wv = 1; wv < WAVES; ++wv) s += red[wv][term];
    slab_slot[term] = s;
  }
}

namespace {

// one thread per (item, term): the item's slots in tile order, TERMS numbers per slot; eight loads in flight, added in tile order
template <int TERMS>
__global__ __launch_bounds__(64) void gn_fold_kernel(const double *__restrict__ slab, int n_items, int n_tiles, double *__restrict__ sums) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n_items * TERMS) return;
  const int p = t / TERMS, e = t % TERMS;
  const double *sb = slab + (size_t)p * n_tiles * TERMS + e;
  double s = 0.0;
  int k = 0;
  for (; k + 8 <= n_tiles; k += 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = sb[(size_t)(k + i) * TERMS];
#pragma unroll
    for (int i = 0; i < 8; ++i) s += v[i];
  }
  for (; k < n_tiles; ++k) s += sb[(size_t)k * TERMS];
  sums[t] = s;
}

// The host's tail of an aligner, behind its kernel on stream s: the fold of the slab into `sums` and, with h_sums, their copy to the host
// and a synchronisation.  The stream is synchronised on every path once the copy is asked for - also after a failed launch or copy - so
// that nothing the caller hands back to the arena, and no host buffer an earlier copy reads, is in use when this returns.  Without
// h_sums nothing synchronises (fp_pose_polish runs in a hipGraph): what went back to the arena is next taken behind these launches on
// the same stream.
template <int TERMS>
inline int gn_fold_to_host(const double *slab, int n_items, int n_tiles, double *sums, double *h_sums, hipStream_t s) {
  hipLaunchKernelGGL(gn_fold_kernel<TERMS>, dim3((unsigned)(((size_t)n_items * TERMS + 63) / 64)), dim3(64), 0, s, slab, n_items, n_tiles, sums);
  const hipError_t e0 = hipGetLastError();
  hipError_t e1 = hipSuccess, e2 = hipSuccess;
  if (h_sums) {
    if (e0 == hipSuccess) e1 = hipMemcpyAsync(h_sums, sums, (size_t)n_items * TERMS * sizeof(double), hipMemcpyDeviceToHost, s);
    e2 = hipStreamSynchronize(s);
  }
  FP_CHECK_HIP(e0);
  FP_CHECK_HIP(e1);
  FP_CHECK_HIP(e2);
  return FP_OK;
}

}  // namespace
