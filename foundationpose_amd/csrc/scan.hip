// In-place exclusive scan of 64-bit words (scan_exclusive, declared in common.h): reduce / scan of the block sums / add, recursive on the
// host, so a workgroup never waits for another one.  tsdf.hip, mesh_simplify.hip, mesh_components.hip and surface_distance.hip number their
// outputs with it.
#include "common.h"

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 4;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;     // 1024 words per workgroup
typedef unsigned long long u64;

// sum of a workgroup's tile -> sums[block]
__global__ __launch_bounds__(SCAN_THREADS) void scan_reduce_kernel(const u64 *__restrict__ in, long long n, u64 *__restrict__ sums) {
  __shared__ u64 red[SCAN_THREADS];
  const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
  u64 s = 0;
#pragma unroll
  for (int q = 0; q < SCAN_ITEMS; ++q)
    if (base + q < n) s += in[base + q];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = SCAN_THREADS / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = red[0];
}

// in-place exclusive scan of every workgroup's tile, started at offsets[block] (0 when null: the single-tile level)
__global__ __launch_bounds__(SCAN_THREADS) void scan_tile_kernel(u64 *__restrict__ data, long long n, const u64 *__restrict__ offsets) {
  __shared__ u64 part[SCAN_THREADS];
  const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
  u64 x[SCAN_ITEMS];
  u64 s = 0;
#pragma unroll
  for (int q = 0; q < SCAN_ITEMS; ++q) {
    x[q] = base + q < n ? data[base + q] : 0;
    s += x[q];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < SCAN_THREADS; o <<= 1) {         // Hillis-Steele over the 256 thread sums: inclusive
    const u64 add = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  u64 run = (offsets ? offsets[blockIdx.x] : 0) + part[threadIdx.x] - s;
#pragma unroll
  for (int q = 0; q < SCAN_ITEMS; ++q) {
    if (base + q < n) data[base + q] = run;
    run += x[q];
  }
}

}  // namespace

size_t scan_sums_words(long long n) {
  size_t w = 0;
  while (n > SCAN_TILE) {
    n = (n + SCAN_TILE - 1) / SCAN_TILE;
    w += (size_t)n;
  }
  return w + 1;
}

int scan_exclusive(unsigned long long *data, long long n, unsigned long long *sums, hipStream_t s) {
  const long long nb = (n + SCAN_TILE - 1) / SCAN_TILE;
  if (nb <= 1) {
    hipLaunchKernelGGL(scan_tile_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, data, n, (const u64 *)nullptr);
    FP_CHECK_HIP(hipGetLastError());
    return FP_OK;
  }
  hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, (const u64 *)data, n, sums);
  FP_CHECK_HIP(hipGetLastError());
  FP_TRY(scan_exclusive(sums, nb, sums + nb, s));
  hipLaunchKernelGGL(scan_tile_kernel, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, data, n, (const u64 *)sums);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
