// Boxes of a point set in C candidate frames, and the smallest of them (fp_box_extents): the search of Utils.oriented_bounds.
//
// The rule per candidate c with frame rows r_0, r_1, r_2 - this project's own, restated in fp32 numpy by tests/oriented_bounds_oracle.py:
//   q_k   = ((r_k0 * x) + (r_k1 * y)) + (r_k2 * z)            fp32, in that order, nothing contracted (-ffp-contract=off)
//   lo_k  = min, hi_k = max of q_k over all points            fminf / fmaxf from +inf / -inf: a NaN projection is passed over
//   vol   = ((hi_0 - lo_0) * (hi_1 - lo_1)) * (hi_2 - lo_2)   fp32
// The winner is taken by a total order on (vol, c): a candidate is eligible when vol >= 0 - a NaN volume never wins, nor does the negative
// one of a candidate that saw no finite projection - the smaller volume first, then the lower index.  min and max do not depend on the
// order of their operands, so every number is the same bits whatever the tiling, the launch shape or the run.  No sqrtf and no division
// on the device: the frames come normalised from the host.
//
// A workgroup owns BX_CAND candidates and one slice of the points: each lane keeps BX_Q frames (9 floats) and their six running bounds
// in registers, a tile of BX_TILE points is staged in LDS as float4 and read back as broadcasts, so one 16-byte LDS read feeds BX_Q x 3
// projections per lane.  grid = (candidate blocks, point slices): few candidates against many points still fill the chip.  Every
// workgroup writes its bounds to its own rows of a slab; box_fold_kernel folds the slices of a candidate (into slice 0 of the slab),
// forms the volumes and leaves one (vol, c) per workgroup; box_winner_kernel folds those.  No atomics, no arrival counters.
#include "common.h"

#include <algorithm>
#include <limits>

namespace {

constexpr int BX_THREADS = 256;
constexpr int BX_Q = 4;                          // candidate frames per lane
constexpr int BX_CAND = BX_THREADS * BX_Q;       // candidates per workgroup
constexpr int BX_TILE = 1024;                    // points per LDS tile: 16 KiB of float4
constexpr int BX_TARGET_BLOCKS = 1024;           // slices are added until the first launch has about this many workgroups (256 CUs x 4)
constexpr int BX_WIN_THREADS = 1024;

static_assert(BX_CAND == FP_BOX_EXTENTS_CAND && BX_TILE == FP_BOX_EXTENTS_TILE, "the header states the tile sizes");

struct BoxCand {
  float vol;
  int c;
};

__device__ __forceinline__ bool better(const BoxCand &a, const BoxCand &b) { return a.vol < b.vol || (a.vol == b.vol && a.c < b.c); }

// fold the candidates of a workgroup of NT threads; the result is valid in thread 0.  `red` holds NT / 64 candidates.
template <int NT>
__device__ __forceinline__ BoxCand block_best(BoxCand c, BoxCand *red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    BoxCand t{__shfl_xor(c.vol, o, 64), __shfl_xor(c.c, o, 64)};
    if (better(t, c)) c = t;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < NT / 64; ++w)
      if (better(red[w], c)) c = red[w];
  return c;
}

constexpr float BX_INF = std::numeric_limits<float>::infinity();
// no candidate yet: loses to every eligible one, +inf volumes included
#define BX_NONE BoxCand{BX_INF, 0x7fffffff}

// slab: (S, C, 6) floats, row (s, c) = lo[3], hi[3] of candidate c over the points of slice s
__global__ __launch_bounds__(BX_THREADS) void box_extents_kernel(const float *__restrict__ pts, int n, const float *__restrict__ frames, int C,
                                                                 int slice_pts, float *__restrict__ slab) {
  __shared__ float4 lds[BX_TILE];
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * BX_CAND;

  // this lane's frames (a candidate past C repeats the last one and is not written)
  float r[BX_Q][9], lo[BX_Q][3], hi[BX_Q][3];
#pragma unroll
  for (int q = 0; q < BX_Q; ++q) {
    const size_t k = (size_t)min(c0 + q * BX_THREADS + tid, C - 1) * 9;
#pragma unroll
    for (int e = 0; e < 9; ++e) r[q][e] = frames[k + e];
#pragma unroll
    for (int e = 0; e < 3; ++e) lo[q][e] = BX_INF, hi[q][e] = -BX_INF;
  }

  const int p0 = blockIdx.y * slice_pts, p1 = min(n, p0 + slice_pts);      // slice_pts is a multiple of BX_TILE; p0 < n
  for (int t0 = p0; t0 < p1; t0 += BX_TILE) {
    const int cnt = min(BX_TILE, p1 - t0);
    __syncthreads();                                                       // the previous tile has been read
    for (int jj = tid; jj < cnt; jj += BX_THREADS) {
      const size_t k = (size_t)(t0 + jj) * 3;
      lds[jj] = make_float4(pts[k], pts[k + 1], pts[k + 2], 0.f);
    }
    __syncthreads();
#pragma unroll 4
    for (int jj = 0; jj < cnt; ++jj) {
      const float4 p = lds[jj];
#pragma unroll
      for (int q = 0; q < BX_Q; ++q)
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          const float v = ((r[q][3 * e] * p.x) + (r[q][3 * e + 1] * p.y)) + (r[q][3 * e + 2] * p.z);
          lo[q][e] = fminf(lo[q][e], v);
          hi[q][e] = fmaxf(hi[q][e], v);
        }
    }
  }

#pragma unroll
  for (int q = 0; q < BX_Q; ++q) {
    const int c = c0 + q * BX_THREADS + tid;
    if (c >= C) continue;
    float *row = slab + ((size_t)blockIdx.y * C + c) * 6;
#pragma unroll
    for (int e = 0; e < 3; ++e) row[e] = lo[q][e], row[3 + e] = hi[q][e];
  }
}

// One thread per candidate, BX_Q candidates per lane as above: fold its S slices into slice 0, form the volume, write the optional
// outputs; part[blockIdx.x] = the best (vol, c) of the workgroup.
__global__ __launch_bounds__(BX_THREADS) void box_fold_kernel(float *__restrict__ slab, int C, int S, float *__restrict__ all_lohi,
                                                              float *__restrict__ all_vol, BoxCand *__restrict__ part) {
  __shared__ BoxCand red[BX_THREADS / 64];
  BoxCand best = BX_NONE;
#pragma unroll
  for (int q = 0; q < BX_Q; ++q) {
    const int c = blockIdx.x * BX_CAND + q * BX_THREADS + threadIdx.x;
    if (c >= C) continue;
    float b[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) b[e] = slab[(size_t)c * 6 + e];
#pragma unroll 8
    for (int s = 1; s < S; ++s) {                // (independent loads: several slices in flight)
      const float *row = slab + ((size_t)s * C + c) * 6;
#pragma unroll
      for (int e = 0; e < 3; ++e) b[e] = fminf(b[e], row[e]), b[3 + e] = fmaxf(b[3 + e], row[3 + e]);
    }
    const float vol = ((b[3] - b[0]) * (b[4] - b[1])) * (b[5] - b[2]);
    if (S > 1)
#pragma unroll
      for (int e = 0; e < 6; ++e) slab[(size_t)c * 6 + e] = b[e];
    if (all_lohi)
#pragma unroll
      for (int e = 0; e < 6; ++e) all_lohi[(size_t)c * 6 + e] = b[e];
    if (all_vol) all_vol[c] = vol;
    const BoxCand t{vol, c};
    if (vol >= 0.f && better(t, best)) best = t;
  }
  best = block_best<BX_THREADS>(best, red);
  if (threadIdx.x == 0) part[blockIdx.x] = best;
}

// one workgroup: fold the per-workgroup winners and write the winner's record from slice 0 of the slab.  No eligible candidate (every
// volume NaN or negative): index -1 and NaN everywhere.
__global__ __launch_bounds__(BX_WIN_THREADS) void box_winner_kernel(const float *__restrict__ slab, const BoxCand *__restrict__ part, int n_part,
                                                                    int32_t *__restrict__ out_index, float *__restrict__ out_lohi,
                                                                    float *__restrict__ out_vol) {
  __shared__ BoxCand red[BX_WIN_THREADS / 64];
  BoxCand best = BX_NONE;
  for (int k = threadIdx.x; k < n_part; k += BX_WIN_THREADS) {
    const BoxCand t = part[k];
    if (better(t, best)) best = t;
  }
  best = block_best<BX_WIN_THREADS>(best, red);
  if (threadIdx.x == 0) {
    const bool found = best.c != 0x7fffffff;
    const float nan = __int_as_float(0x7fc00000);
    out_index[0] = found ? best.c : -1;
    out_vol[0] = found ? best.vol : nan;
    for (int e = 0; e < 6; ++e) out_lohi[e] = found ? slab[(size_t)best.c * 6 + e] : nan;
  }
}

struct BoxPlan {
  int cand_blocks, slice_pts, S;
};

BoxPlan box_plan(int n, int C) {
  BoxPlan p;
  p.cand_blocks = (C + BX_CAND - 1) / BX_CAND;
  const int tiles = (n + BX_TILE - 1) / BX_TILE;
  const int want = std::min(tiles, std::max(1, (BX_TARGET_BLOCKS + p.cand_blocks - 1) / p.cand_blocks));
  const int tiles_per_slice = (tiles + want - 1) / want;
  p.slice_pts = tiles_per_slice * BX_TILE;
  p.S = (tiles + tiles_per_slice - 1) / tiles_per_slice;         // every slice holds at least one point
  return p;
}

size_t part_offset(int n, int C) { return align256((size_t)box_plan(n, C).S * C * 6 * sizeof(float)); }

}  // namespace

size_t box_extents_slab_bytes(int n, int C) { return part_offset(n, C) + (size_t)box_plan(n, C).cand_blocks * sizeof(BoxCand); }

int launch_box_extents(const float *pts, int n, const float *frames, int C, void *slab, int32_t *out_index, float *out_lohi, float *out_vol,
                       float *all_lohi, float *all_vol, hipStream_t s) {
  const BoxPlan p = box_plan(n, C);
  float *bounds = (float *)slab;
  BoxCand *part = (BoxCand *)((char *)slab + part_offset(n, C));
  hipLaunchKernelGGL(box_extents_kernel, dim3(p.cand_blocks, p.S), dim3(BX_THREADS), 0, s, pts, n, frames, C, p.slice_pts, bounds);
  FP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(box_fold_kernel, dim3(p.cand_blocks), dim3(BX_THREADS), 0, s, bounds, C, p.S, all_lohi, all_vol, part);
  FP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(box_winner_kernel, dim3(1), dim3(BX_WIN_THREADS), 0, s, (const float *)bounds, (const BoxCand *)part, p.cand_blocks,
                     out_index, out_lohi, out_vol);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
