// Exact diameter of a point set (src/Utils.py:559-574 without the random sub-sample): max over i < j of |p_i - p_j|, and the pair.
//
// The points are cut into tiles of MD_TILE.  A workgroup owns one pair of tiles (ta <= tb, the upper triangle only): each lane keeps
// MD_Q points of tile ta in registers, tile tb is staged once in LDS as float4 and read back as broadcasts (every lane reads the same
// address), so one 16-byte LDS read feeds MD_Q distance evaluations per lane.  The squared distance is dx*dx + dy*dy + dz*dz in fp32 in
// exactly that order (the library is built without contraction): d(i, j) and d(j, i) are the same bits, and so is a pair's value
// whatever tile, lane or launch evaluates it.  sqrtf is taken once, of the final maximum.
//
// The result does not depend on the order anything runs in: a candidate is (d2, i, j) with i < j, and `better` is a total order on
// candidates - larger d2 first, then the smaller i, then the smaller j.  A lane scans j upwards and replaces only on a strictly larger
// d2, so it keeps the smallest j of its point; lanes, waves and workgroups are then folded with `better`.  Every workgroup writes its
// candidate to its own slot of a slab; mesh_diameter_finish folds the slab.  No atomics, no arrival counters.
#include "common.h"

namespace {

constexpr int MD_THREADS = 256;
constexpr int MD_Q = 4;                          // points of tile ta per lane
constexpr int MD_TILE = MD_THREADS * MD_Q;       // points per tile: 16 KiB of float4 in LDS
constexpr int MD_FIN_THREADS = 1024;

struct Cand {
  float d2;
  int i, j;
};

__device__ __forceinline__ bool better(const Cand &a, const Cand &b) {
  return a.d2 > b.d2 || (a.d2 == b.d2 && (a.i < b.i || (a.i == b.i && a.j < b.j)));
}

// fold the candidates of a workgroup of NT threads; the result is valid in thread 0.  `red` holds NT / 64 candidates.
template <int NT>
__device__ __forceinline__ Cand block_best(Cand c, Cand *red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    Cand t{__shfl_xor(c.d2, o, 64), __shfl_xor(c.i, o, 64), __shfl_xor(c.j, o, 64)};
    if (better(t, c)) c = t;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < NT / 64; ++w)
      if (better(red[w], c)) c = red[w];
  return c;
}

// tile pair number k of the upper triangle, rows in order: row ta holds (ta, ta), (ta, ta + 1), .. (ta, T - 1)
__device__ __forceinline__ void tile_pair(long long k, int T, int &ta, int &tb) {
  auto row_start = [T](long long r) { return r * T - r * (r - 1) / 2; };
  const double b = 2.0 * T + 1.0;
  long long r = (long long)((b - sqrt(b * b - 8.0 * (double)k)) * 0.5);
  r = r < 0 ? 0 : (r > T - 1 ? T - 1 : r);
  while (r > 0 && row_start(r) > k) --r;           // the double-precision guess is off by one at most; these settle it exactly
  while (r < T - 1 && row_start(r + 1) <= k) ++r;
  ta = (int)r;
  tb = (int)(r + (k - row_start(r)));
}

template <bool DIAG>
__device__ __forceinline__ void scan_tile(const float4 *lds, int cnt, int j0, const float *px, const float *py, const float *pz,
                                          const int *pi, float *best, int *bj) {
#pragma unroll 4
  for (int jj = 0; jj < cnt; ++jj) {
    const float4 r = lds[jj];
    const int j = j0 + jj;
#pragma unroll
    for (int q = 0; q < MD_Q; ++q) {
      const float dx = px[q] - r.x, dy = py[q] - r.y, dz = pz[q] - r.z;
      const float d = dx * dx + dy * dy + dz * dz;
      if (d > best[q] && (!DIAG || j != pi[q])) best[q] = d, bj[q] = j;
    }
  }
}

__global__ __launch_bounds__(MD_THREADS) void mesh_diameter_kernel(const float *__restrict__ pts, int n, int T, Cand *__restrict__ slab) {
  __shared__ float4 lds[MD_TILE];
  __shared__ Cand red[MD_THREADS / 64];
  const int tid = threadIdx.x;
  int ta, tb;
  tile_pair((long long)blockIdx.x, T, ta, tb);

  // this lane's points of tile ta (a point past n repeats the last one and is left out of the fold)
  float px[MD_Q], py[MD_Q], pz[MD_Q], best[MD_Q];
  int pi[MD_Q], bj[MD_Q];
#pragma unroll
  for (int q = 0; q < MD_Q; ++q) {
    pi[q] = ta * MD_TILE + q * MD_THREADS + tid;
    const size_t k = (size_t)min(pi[q], n - 1) * 3;
    px[q] = pts[k], py[q] = pts[k + 1], pz[q] = pts[k + 2];
    best[q] = -1.f, bj[q] = -1;
  }

  const int j0 = tb * MD_TILE, cnt = min(MD_TILE, n - j0);
  for (int jj = tid; jj < cnt; jj += MD_THREADS) {
    const size_t k = (size_t)(j0 + jj) * 3;
    lds[jj] = make_float4(pts[k], pts[k + 1], pts[k + 2], 0.f);
  }
  __syncthreads();
  if (ta == tb)
    scan_tile<true>(lds, cnt, j0, px, py, pz, pi, best, bj);
  else
    scan_tile<false>(lds, cnt, j0, px, py, pz, pi, best, bj);

  // in the diagonal tile a lane may have met its partner below itself: the pair is stored as (smaller, larger) index
  Cand c{-1.f, 0x7fffffff, 0x7fffffff};
#pragma unroll
  for (int q = 0; q < MD_Q; ++q) {
    if (pi[q] >= n || bj[q] < 0) continue;
    const Cand t{best[q], min(pi[q], bj[q]), max(pi[q], bj[q])};
    if (better(t, c)) c = t;
  }
  c = block_best<MD_THREADS>(c, red);
  if (tid == 0) slab[blockIdx.x] = c;
}

// one workgroup: fold the slab, take the root.  n_cand = 0 (fewer than two points): diameter 0, pair (0, 0).
__global__ __launch_bounds__(MD_FIN_THREADS) void mesh_diameter_finish_kernel(const Cand *__restrict__ slab, long long n_cand, float *out,
                                                                              int32_t *pair) {
  __shared__ Cand red[MD_FIN_THREADS / 64];
  Cand c{-1.f, 0x7fffffff, 0x7fffffff};
  for (long long k = threadIdx.x; k < n_cand; k += MD_FIN_THREADS) {
    const Cand t = slab[k];
    if (better(t, c)) c = t;
  }
  c = block_best<MD_FIN_THREADS>(c, red);
  if (threadIdx.x == 0) {
    const bool found = c.d2 >= 0.f;              // false without a pair, or when every distance is NaN
    out[0] = found ? sqrtf(c.d2) : 0.f;
    if (pair) pair[0] = found ? c.i : 0, pair[1] = found ? c.j : 0;
  }
}

long long diameter_tile_pairs(int n_pts) {
  if (n_pts < 2) return 0;
  const long long T = (n_pts + MD_TILE - 1) / MD_TILE;
  return T * (T + 1) / 2;
}

}  // namespace

size_t mesh_diameter_slab_bytes(int n_pts) { return (size_t)diameter_tile_pairs(n_pts) * sizeof(Cand); }

int launch_mesh_diameter(const float *pts, int n_pts, void *slab, float *out, int32_t *pair, hipStream_t s) {
  const long long blocks = diameter_tile_pairs(n_pts);
  FP_REQUIRE(blocks <= 0x7fffffff, "fp_mesh_diameter: %d points are too many for one launch", n_pts);
  if (blocks > 0) {
    hipLaunchKernelGGL(mesh_diameter_kernel, dim3((unsigned)blocks), dim3(MD_THREADS), 0, s, pts, n_pts, (n_pts + MD_TILE - 1) / MD_TILE,
                       (Cand *)slab);
    FP_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(mesh_diameter_finish_kernel, dim3(1), dim3(MD_FIN_THREADS), 0, s, (const Cand *)slab, blocks, out, pair);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
