// The back end of a Gauss-Newton linearisation kernel (tsdf_align_kernel in tsdf.hip, both passes of depth_pairs_kernel in depth_icp.hip):
// the row of a pixel and the 29 sums of an item - a view or a pair: the 21 entries of the upper triangle of J^T J row by row, the 6 of
// J^T r, r^2 and the number of valid pixels.  Device only; include after device_util.h.  Everything is __forceinline__.
//
// The summation order is part of the documented results ("a pair does not depend on its batch", "terms 0..28 are bit-identical to the
// geometric call"); tests/gn_sums_oracle.py restates it and the GPU tests hold the kernels to it bit for bit.  A workgroup of 64 WAVES
// threads owns a tile of PIX x 64 WAVES pixels of one item; the pixels past the item's last one are zero rows.
//   1. Pixel tile * (PIX * 64 WAVES) + q * 64 WAVES + tid belongs to lane tid.
//   2. A lane starts every sum at +0.0 and adds its pixels q = 0 .. PIX - 1 in that order (gn_accumulate): J and r widened to double, a
//      product, an add - the library is built without contraction.  The count adds 1.0 for a valid pixel; an invalid pixel is a zero row
//      (gn_mask) and adds +0.0 to everything.
//   3. Over the 64 lanes of a wave: wave_sum's butterfly, partner distance 32, 16, .. 1, s = s + s[lane ^ o]; every lane ends with the
//      same value and lane 0 writes it to LDS (gn_wave_to_lds).
//   4. After the kernel's barrier thread `term` adds the waves from wave 0 up, red[0] + red[1] + .., and writes the workgroup's own slot of
//      the slab (gn_lds_to_slab).  No atomics.
//   5. gn_fold_kernel: one thread per (item, term) adds the item's slots from 0.0 in tile order.
#pragma once
#include "device_util.h"

constexpr int GN_TERMS = 29;
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

}  // namespace
