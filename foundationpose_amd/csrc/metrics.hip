// Pose-error metrics against ground truth (src/Utils.py:232-253): ADD, ADD-S and ADD with symmetry transforms, for B poses in one launch.
//
// Everything is evaluated in the camera frame, exactly as the definitions read, so no pose has to be rigid for the result to hold:
//   ADD_b     = mean_i |D_b p_i|,               D_b   = pred_b - gt_b           (3x4 rows, formed in double, rounded once)
//   ADDsym_b  = min_k mean_i |D_bk p_i|,        D_bk  = pred_b - gt_b S_k
//   ADD-S_b   = mean_i min_j |gt_b p_i - pred_b p_j|   (ground-truth points query the predicted points: cKDTree(pred).query(gt))
// A workgroup owns (pose b, a tile of PM_TILE query points); each lane keeps PM_Q transformed queries in registers as packed fp32 pairs.
// The predicted points of ADD-S are transformed while they are staged through LDS in chunks of PM_CHUNK float4 and read back as
// broadcasts (every lane reads the same address).  Distances use the difference form dx, dy, dz -> fma(dx, dx, fma(dy, dy, dz * dz)):
// pred_b = gt_b gives exactly 0.  No float atomics: each (b, tile) writes its double partial sums to a slab, which pose_errors_finish
// adds in tile order and divides by N, so a pose's result is bit-identical whatever batch it is in and at whatever index.
#include "common.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int PM_THREADS = 256;
constexpr int PM_Q = 8;                         // queries per lane: PM_Q / 2 packed pairs
constexpr int PM_TILE = PM_THREADS * PM_Q;      // query points per workgroup
constexpr int PM_CHUNK = 2048;                  // predicted points per LDS chunk (32 KiB of float4: five workgroups fit one CU's LDS)
constexpr int PM_TERMS0 = 2;                    // slab terms per (pose, tile): [0] ADD-S, [1] ADD, [2 + k] symmetry k

struct PoseErrArgs {
  const float *pts;        // (N, 3)
  const float *pred;       // (B, 4, 4)
  const float *gt;         // (4, 4) or (B, 4, 4)
  const float *sym;        // (K, 4, 4) or null
  int n, n_sym, gt_per_pose, which, n_tiles, n_terms;
  double *slab;            // [B][n_terms][n_tiles]
};

// rows 0..2 of  A - G * S  (S null: the identity), in double, rounded once to float
__device__ __forceinline__ void pose_diff(const float *A, const float *G, const float *S, float *D) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double gs;
      if (S) {
        gs = (double)G[r * 4 + 0] * (double)S[0 * 4 + c];
        gs = fma((double)G[r * 4 + 1], (double)S[1 * 4 + c], gs);
        gs = fma((double)G[r * 4 + 2], (double)S[2 * 4 + c], gs);
        gs = fma((double)G[r * 4 + 3], (double)S[3 * 4 + c], gs);
      } else {
        gs = (double)G[r * 4 + c];
      }
      D[r * 4 + c] = (float)((double)A[r * 4 + c] - gs);
    }
}

__device__ __forceinline__ void xform(const float *M, float x, float y, float z, float &ox, float &oy, float &oz) {
  ox = fmaf(M[0], x, fmaf(M[1], y, fmaf(M[2], z, M[3])));
  oy = fmaf(M[4], x, fmaf(M[5], y, fmaf(M[6], z, M[7])));
  oz = fmaf(M[8], x, fmaf(M[9], y, fmaf(M[10], z, M[11])));
}

__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf(fmaf(x, x, fmaf(y, y, z * z))); }

// sum over the workgroup in a fixed order (butterfly within each wave, then the waves in order); the total is valid in thread 0.
// `red` holds PM_THREADS / 64 doubles; the caller synchronises before `red` is reused.
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < PM_THREADS / 64; ++i) s += red[i];
  return s;
}

__global__ __launch_bounds__(PM_THREADS) void pose_errors_kernel(PoseErrArgs a) {
  __shared__ float4 lds[PM_CHUNK];
  double *red = (double *)lds;            // the block sums reuse the chunk buffer once the ADD-S loop is done
  const int tile = blockIdx.x % a.n_tiles, b = blockIdx.x / a.n_tiles;
  const int tid = threadIdx.x;
  const float *P = a.pred + (size_t)b * 16;
  const float *G = a.gt + (a.gt_per_pose ? (size_t)b * 16 : 0);
  double *slab = a.slab + (size_t)b * a.n_terms * a.n_tiles + tile;

  // this lane's model points (a query past N repeats the last point and is left out of every sum)
  float px[PM_Q], py[PM_Q], pz[PM_Q];
  bool valid[PM_Q];
#pragma unroll
  for (int q = 0; q < PM_Q; ++q) {
    const int i = tile * PM_TILE + q * PM_THREADS + tid;
    valid[q] = i < a.n;
    const size_t k = (size_t)(valid[q] ? i : a.n - 1) * 3;
    px[q] = a.pts[k], py[q] = a.pts[k + 1], pz[q] = a.pts[k + 2];
  }

  if (a.which & FP_ERR_ADDS) {
    float Gm[12], Pm[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) Gm[i] = G[i], Pm[i] = P[i];
    f32x2 qx[PM_Q / 2], qy[PM_Q / 2], qz[PM_Q / 2], m[PM_Q / 2];
#pragma unroll
    for (int k = 0; k < PM_Q / 2; ++k) {
      float x0, y0, z0, x1, y1, z1;
      xform(Gm, px[2 * k], py[2 * k], pz[2 * k], x0, y0, z0);
      xform(Gm, px[2 * k + 1], py[2 * k + 1], pz[2 * k + 1], x1, y1, z1);
      qx[k] = f32x2{x0, x1}, qy[k] = f32x2{y0, y1}, qz[k] = f32x2{z0, z1};
      m[k] = f32x2{__builtin_inff(), __builtin_inff()};
    }
    for (int c0 = 0; c0 < a.n; c0 += PM_CHUNK) {
      const int cnt = min(PM_CHUNK, a.n - c0);
      const int cnt8 = (cnt + 7) & ~7;    // padded with copies of the chunk's last point: a duplicate leaves every minimum unchanged
      __syncthreads();                    // the previous chunk has been read by every wave
      for (int j = tid; j < cnt8; j += PM_THREADS) {
        const size_t k = (size_t)(c0 + min(j, cnt - 1)) * 3;
        float x, y, z;
        xform(Pm, a.pts[k], a.pts[k + 1], a.pts[k + 2], x, y, z);
        lds[j] = make_float4(x, y, z, 0.f);
      }
      __syncthreads();
#pragma unroll 4
      for (int j = 0; j < cnt8; j += 2) {
        const float4 r0 = lds[j], r1 = lds[j + 1];
#pragma unroll
        for (int k = 0; k < PM_Q / 2; ++k) {
          const f32x2 dx0 = qx[k] - r0.x, dy0 = qy[k] - r0.y, dz0 = qz[k] - r0.z;
          const f32x2 dx1 = qx[k] - r1.x, dy1 = qy[k] - r1.y, dz1 = qz[k] - r1.z;
          const f32x2 d0 = __builtin_elementwise_fma(dx0, dx0, __builtin_elementwise_fma(dy0, dy0, dz0 * dz0));
          const f32x2 d1 = __builtin_elementwise_fma(dx1, dx1, __builtin_elementwise_fma(dy1, dy1, dz1 * dz1));
          m[k] = __builtin_elementwise_min(m[k], __builtin_elementwise_min(d0, d1));
        }
      }
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < PM_Q / 2; ++k) {
      if (valid[2 * k]) s += (double)sqrtf(m[k].x);
      if (valid[2 * k + 1]) s += (double)sqrtf(m[k].y);
    }
    __syncthreads();                      // the chunk buffer becomes `red`
    s = block_sum(s, red);
    if (tid == 0) slab[0] = s;
  }

  // ADD (S = identity) and ADD under each symmetry transform: one 3x4 difference matrix each
  const int k_first = (a.which & FP_ERR_ADD) ? -1 : 0, k_end = (a.which & FP_ERR_ADD_SYM) ? a.n_sym : 0;
  for (int k = k_first; k < k_end; ++k) {
    float D[12];
    pose_diff(P, G, k < 0 ? nullptr : a.sym + (size_t)k * 16, D);
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < PM_Q; ++q) {
      float x, y, z;
      xform(D, px[q], py[q], pz[q], x, y, z);
      if (valid[q]) s += (double)norm3(x, y, z);
    }
    __syncthreads();                      // `red` of the previous sum has been read
    s = block_sum(s, red);
    if (tid == 0) slab[(size_t)(PM_TERMS0 + k) * a.n_tiles] = s;
  }
}

// one thread per pose: the slabs in tile order, / N; ADDsym = the least mean over the symmetry transforms
__global__ __launch_bounds__(64) void pose_errors_finish_kernel(const double *__restrict__ slab, int B, int n, int n_tiles, int n_terms,
                                                                int n_sym, int which, float *add, float *adds, float *add_sym) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const double *sb = slab + (size_t)b * n_terms * n_tiles;
  auto mean = [&](int term) {
    double s = 0.0;
    for (int t = 0; t < n_tiles; ++t) s += sb[(size_t)term * n_tiles + t];
    return s / (double)n;
  };
  if (which & FP_ERR_ADDS) adds[b] = (float)mean(0);
  if (which & FP_ERR_ADD) add[b] = (float)mean(1);
  if (which & FP_ERR_ADD_SYM) {
    double best = mean(PM_TERMS0);
    for (int k = 1; k < n_sym; ++k) best = fmin(best, mean(PM_TERMS0 + k));
    add_sym[b] = (float)best;
  }
}

}  // namespace

size_t pose_errors_slab_bytes(int n_pts, int n_poses, int n_sym) {
  const size_t n_tiles = ((size_t)n_pts + PM_TILE - 1) / PM_TILE;
  return (size_t)n_poses * n_tiles * (PM_TERMS0 + (size_t)n_sym) * sizeof(double);
}

int launch_pose_errors(const float *pts, int n_pts, const float *pred, const float *gt, int gt_per_pose, int n_poses, const float *sym,
                       int n_sym, int which, double *slab, float *add, float *adds, float *add_sym, hipStream_t s) {
  const int n_tiles = (n_pts + PM_TILE - 1) / PM_TILE;
  const size_t blocks = (size_t)n_tiles * n_poses;
  FP_REQUIRE(blocks <= 0x7fffffff, "fp_pose_errors: %d poses x %d points is too large for one launch", n_poses, n_pts);
  const int n_s = (which & FP_ERR_ADD_SYM) ? n_sym : 0;
  PoseErrArgs a{pts, pred, gt, sym, n_pts, n_s, gt_per_pose, which, n_tiles, PM_TERMS0 + n_s, slab};
  hipLaunchKernelGGL(pose_errors_kernel, dim3((unsigned)blocks), dim3(PM_THREADS), 0, s, a);
  FP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(pose_errors_finish_kernel, dim3((n_poses + 63) / 64), dim3(64), 0, s, slab, n_poses, n_pts, n_tiles, a.n_terms, n_s,
                     which, add, adds, add_sym);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
