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
#include "device_util.h"
#include "view_geom.h"

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

// entry (r, c) of  G * S  in double (S null: the identity)
__device__ __forceinline__ double gs_entry(const float *G, const float *S, int r, int c) {
  if (!S) return (double)G[r * 4 + c];
  double gs = (double)G[r * 4 + 0] * (double)S[0 * 4 + c];
  gs = fma((double)G[r * 4 + 1], (double)S[1 * 4 + c], gs);
  gs = fma((double)G[r * 4 + 2], (double)S[2 * 4 + c], gs);
  return fma((double)G[r * 4 + 3], (double)S[3 * 4 + c], gs);
}

// rows 0..2 of  A - G * S  (S null: the identity), in double, rounded once to float
__device__ __forceinline__ void pose_diff(const float *A, const float *G, const float *S, float *D) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) D[r * 4 + c] = (float)((double)A[r * 4 + c] - gs_entry(G, S, r, c));
}

// rows 0..2 of  G * S, in double, rounded once to float
__device__ __forceinline__ void pose_mul(const float *G, const float *S, float *M) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) M[r * 4 + c] = (float)gs_entry(G, S, r, c);
}

__device__ __forceinline__ void xform(const float *M, float x, float y, float z, float &ox, float &oy, float &oz) {
  ox = fmaf(M[0], x, fmaf(M[1], y, fmaf(M[2], z, M[3])));
  oy = fmaf(M[4], x, fmaf(M[5], y, fmaf(M[6], z, M[7])));
  oz = fmaf(M[8], x, fmaf(M[9], y, fmaf(M[10], z, M[11])));
}

__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf(fmaf(x, x, fmaf(y, y, z * z))); }

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
    s = block_sum<PM_THREADS>(s, red);        // its first barrier: the chunk buffer becomes `red`
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
    s = block_sum<PM_THREADS>(s, red);
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

// ---- BOP errors (bop_toolkit pose_error.py: mssd, mspd, vsd) -----------------------------------------------------------------------------
//   MSSD_b = min_k max_i |D_bk p_i|,                       D_bk = pred_b - gt_b S_k     (pose_diff, as ADDsym)
//   MSPD_b = min_k max_i |pi(pred_b p_i) - pi(M_bk p_i)|,  M_bk = gt_b S_k              (formed in double, rounded once)
// with pi(x) = (fx x/z + cx, fy y/z + cy) in double from the fp32 camera-frame points; a point at z <= 0 under either transform makes that
// k's maximum +inf.  A workgroup owns (pose b, a tile of PM_TILE points) and writes the tile's maximum for every k to a float slab;
// bop_errors_finish takes the maximum over the tiles and the minimum over k.  Maxima and minima do not depend on the order they are
// taken in, so a pose's result is bit-identical whatever batch it is in.
//
// VSD (visib_mode 'bop19') of B poses: the depth renders come from the rasteriser (fp_vsd in api.hip); vsd_count_kernel reads each pixel
// of (depth_test, render(gt), render(pred)) once, forms the three distance maps in float64 without contraction, and counts |union|,
// |inter| and the per-tau costs with wave ballots.  The counts go to global integer atomics: integer sums are exact in any order.
namespace {

struct BopErrArgs {
  const float *pts;        // (N, 3)
  const float *pred;       // (B, 4, 4)
  const float *gt;         // (4, 4) or (B, 4, 4)
  const float *sym;        // (K, 4, 4) or null (the identity only)
  int n, n_k, gt_per_pose, which, n_tiles;
  double fx, fy, cx, cy;
  float *slab;             // [B][2][n_k][n_tiles]: MSSD, MSPD tile maxima
};

// maximum over the workgroup, valid in every thread; `red` holds PM_THREADS / 64 floats
__device__ __forceinline__ float block_max(float v, float *red) {
  v = wave_max(v);
  __syncthreads();                        // the previous maximum has been read
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = red[0];
  for (int i = 1; i < PM_THREADS / 64; ++i) m = fmaxf(m, red[i]);
  return m;
}

__device__ __forceinline__ void project(const BopErrArgs &a, float x, float y, float z, double &u, double &v) {
  const double iz = 1.0 / (double)z;
  u = a.fx * ((double)x * iz) + a.cx;
  v = a.fy * ((double)y * iz) + a.cy;
}

__global__ __launch_bounds__(PM_THREADS) void bop_errors_kernel(BopErrArgs a) {
  __shared__ float red[PM_THREADS / 64];
  const int tile = blockIdx.x % a.n_tiles, b = blockIdx.x / a.n_tiles;
  const int tid = threadIdx.x;
  const float *P = a.pred + (size_t)b * 16;
  const float *G = a.gt + (a.gt_per_pose ? (size_t)b * 16 : 0);
  float *slab = a.slab + (size_t)b * 2 * a.n_k * a.n_tiles + tile;
  const float inf = __builtin_inff();

  float px[PM_Q], py[PM_Q], pz[PM_Q];
  bool valid[PM_Q];
#pragma unroll
  for (int q = 0; q < PM_Q; ++q) {
    const int i = tile * PM_TILE + q * PM_THREADS + tid;
    valid[q] = i < a.n;
    const size_t k = (size_t)(valid[q] ? i : a.n - 1) * 3;
    px[q] = a.pts[k], py[q] = a.pts[k + 1], pz[q] = a.pts[k + 2];
  }

  // MSPD: the pixels of the predicted points, once for every k
  double pu[PM_Q], pv[PM_Q];
  bool behind = false;
  if (a.which & FP_BOP_MSPD) {
    float Pm[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) Pm[i] = P[i];
#pragma unroll
    for (int q = 0; q < PM_Q; ++q) {
      float x, y, z;
      xform(Pm, px[q], py[q], pz[q], x, y, z);
      if (valid[q] && !(z > 0.f)) behind = true;
      project(a, x, y, z, pu[q], pv[q]);
    }
  }

  for (int k = 0; k < a.n_k; ++k) {
    const float *S = a.sym ? a.sym + (size_t)k * 16 : nullptr;
    if (a.which & FP_BOP_MSSD) {
      float D[12];
      pose_diff(P, G, S, D);
      float m = 0.f;
#pragma unroll
      for (int q = 0; q < PM_Q; ++q) {
        float x, y, z;
        xform(D, px[q], py[q], pz[q], x, y, z);
        if (valid[q]) m = fmaxf(m, norm3(x, y, z));
      }
      m = block_max(m, red);
      if (tid == 0) slab[(size_t)k * a.n_tiles] = m;
    }
    if (a.which & FP_BOP_MSPD) {
      float M[12];
      pose_mul(G, S, M);
      float m = behind ? inf : 0.f;
#pragma unroll
      for (int q = 0; q < PM_Q; ++q) {
        float x, y, z;
        xform(M, px[q], py[q], pz[q], x, y, z);
        if (!valid[q]) continue;
        if (!(z > 0.f)) {
          m = inf;
        } else {
          double u, v;
          project(a, x, y, z, u, v);
          const double du = pu[q] - u, dv = pv[q] - v;
          m = fmaxf(m, (float)sqrt(du * du + dv * dv));
        }
      }
      m = block_max(m, red);
      if (tid == 0) slab[(size_t)(a.n_k + k) * a.n_tiles] = m;
    }
  }
}

// one thread per pose: the maximum over the tiles, the minimum over the symmetry transforms
__global__ __launch_bounds__(64) void bop_errors_finish_kernel(const float *__restrict__ slab, int B, int n_tiles, int n_k, int which,
                                                               float *mssd, float *mspd) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const float *sb = slab + (size_t)b * 2 * n_k * n_tiles;
  auto min_max = [&](int term) {
    float best = __builtin_inff();
    for (int k = 0; k < n_k; ++k) {
      const float *t = sb + ((size_t)term * n_k + k) * n_tiles;
      float m = t[0];
      for (int i = 1; i < n_tiles; ++i) m = fmaxf(m, t[i]);
      best = fminf(best, m);
    }
    return best;
  };
  if (which & FP_BOP_MSSD) mssd[b] = min_max(0);
  if (which & FP_BOP_MSPD) mspd[b] = min_max(1);
}

constexpr int VSD_THREADS = 256;
constexpr int VSD_UNROLL = 4;                     // pixels per lane whose loads are in flight together
constexpr int VSD_BAND_PIXELS = 8192;             // pixels of one workgroup: whole rows, about this many

struct VsdArgs {
  const float *dt, *dg, *de;                      // depth_test, render(gt), render(pred): pose b's images at + b * stride
  size_t dt_stride, dg_stride, de_stride;
  int H, W, rows, n_taus;
  double cx, cy, inv_fx, inv_fy, diameter, delta;
  double taus[FP_VSD_MAX_TAUS];
  unsigned *counts;                               // [pose][2 + FP_VSD_MAX_TAUS]: |union|, |inter|, cost_tau (zeroed by the caller)
};

// grid (bands of `rows` rows, poses); the pose's counts start at counts + blockIdx.y * (2 + FP_VSD_MAX_TAUS)
__global__ __launch_bounds__(VSD_THREADS) void vsd_count_kernel(VsdArgs a) {
  __shared__ unsigned red[VSD_THREADS / 64][2 + FP_VSD_MAX_TAUS];
  const int b = blockIdx.y;
  const float *dt = a.dt + b * a.dt_stride, *dg = a.dg + b * a.dg_stride, *de = a.de + b * a.de_stride;
  const int p0 = blockIdx.x * a.rows * a.W;
  const int p1 = min(a.H, (blockIdx.x + 1) * a.rows) * a.W;
  unsigned n_union = 0, n_inter = 0, cost[FP_VSD_MAX_TAUS];
#pragma unroll
  for (int t = 0; t < FP_VSD_MAX_TAUS; ++t) cost[t] = 0;

  for (int pb = p0 + threadIdx.x; pb < p1; pb += VSD_THREADS * VSD_UNROLL) {
    float e4[VSD_UNROLL], g4[VSD_UNROLL];
#pragma unroll
    for (int j = 0; j < VSD_UNROLL; ++j) {
      const int p = pb + j * VSD_THREADS;
      e4[j] = p < p1 ? de[p] : 0.f;
      g4[j] = p < p1 ? dg[p] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < VSD_UNROLL; ++j) {
      // a pixel that is background in both renders is in neither mask: nothing more is read for it
      const bool any = e4[j] != 0.f || g4[j] != 0.f;
      if (!__builtin_amdgcn_ballot_w64(any)) continue;
      bool vg = false, ve = false;
      double c = 0.0;
      if (any) {
        const int p = pb + j * VSD_THREADS;
        const int v = p / a.W, u = p - v * a.W;
        const double u_cx = (double)u - a.cx, v_cy = (double)v - a.cy;
        const double Dt = ray_distance((double)dt[p], u_cx, v_cy, a.inv_fx, a.inv_fy);
        const double Dg = ray_distance((double)g4[j], u_cx, v_cy, a.inv_fx, a.inv_fy);
        const double De = ray_distance((double)e4[j], u_cx, v_cy, a.inv_fx, a.inv_fy);
        const float ft = (float)Dt;
        vg = Dg > 0.0 && ((double)((float)Dg - ft) <= a.delta || Dt == 0.0);
        ve = (De > 0.0 && ((double)((float)De - ft) <= a.delta || Dt == 0.0)) || (vg && De > 0.0);
        if (vg && ve) c = fabs(Dg - De) / a.diameter;
      }
      const bool inter = vg && ve;
      n_union += __popcll(__builtin_amdgcn_ballot_w64(vg || ve));
      const unsigned long long mi = __builtin_amdgcn_ballot_w64(inter);
      n_inter += __popcll(mi);
      if (mi) {
#pragma unroll
        for (int t = 0; t < FP_VSD_MAX_TAUS; ++t)
          if (t < a.n_taus) cost[t] += __popcll(__builtin_amdgcn_ballot_w64(inter && c >= a.taus[t]));
      }
    }
  }
  // the counts are the same in every lane of a wave: one row per wave, summed over the waves, one atomic per count and workgroup
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[w][0] = n_union, red[w][1] = n_inter;
#pragma unroll
    for (int t = 0; t < FP_VSD_MAX_TAUS; ++t) red[w][2 + t] = cost[t];
  }
  __syncthreads();
  if (threadIdx.x < 2 + a.n_taus) {
    unsigned s = 0;
    for (int i = 0; i < VSD_THREADS / 64; ++i) s += red[i][threadIdx.x];
    if (s) atomicAdd(a.counts + (size_t)b * (2 + FP_VSD_MAX_TAUS) + threadIdx.x, s);
  }
}

// e_tau = (cost_tau + |union| - |inter|) / |union|, 1 for an empty union (bop_toolkit pose_error.vsd)
__global__ __launch_bounds__(64) void vsd_finish_kernel(const unsigned *__restrict__ counts, int B, int n_taus, float *err, int *counts_out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B * n_taus) return;
  const int b = i / n_taus, t = i - b * n_taus;
  const unsigned *c = counts + (size_t)b * (2 + FP_VSD_MAX_TAUS);
  const unsigned n_union = c[0], n_inter = c[1];
  err[i] = n_union == 0 ? 1.f : (float)((double)(c[2 + t] + n_union - n_inter) / (double)n_union);
  if (counts_out) {
    int *o = counts_out + (size_t)b * (2 + n_taus);
    if (t == 0) o[0] = (int)n_union, o[1] = (int)n_inter;
    o[2 + t] = (int)c[2 + t];
  }
}

}  // namespace

size_t bop_errors_slab_bytes(int n_pts, int n_poses, int n_sym) {
  const size_t n_tiles = ((size_t)n_pts + PM_TILE - 1) / PM_TILE;
  return (size_t)n_poses * n_tiles * 2 * (size_t)(n_sym > 0 ? n_sym : 1) * sizeof(float);
}

int launch_bop_errors(const float *pts, int n_pts, const float *pred, const float *gt, int gt_per_pose, int n_poses, const float *sym,
                      int n_sym, const double *K, int which, float *slab, float *mssd, float *mspd, hipStream_t s) {
  const int n_tiles = (n_pts + PM_TILE - 1) / PM_TILE;
  const size_t blocks = (size_t)n_tiles * n_poses;
  FP_REQUIRE(blocks <= 0x7fffffff, "fp_pose_errors_bop: %d poses x %d points is too large for one launch", n_poses, n_pts);
  BopErrArgs a{pts, pred, gt, n_sym > 0 ? sym : nullptr, n_pts, n_sym > 0 ? n_sym : 1, gt_per_pose, which, n_tiles,
               K ? K[0] : 0.0, K ? K[4] : 0.0, K ? K[2] : 0.0, K ? K[5] : 0.0, slab};
  hipLaunchKernelGGL(bop_errors_kernel, dim3((unsigned)blocks), dim3(PM_THREADS), 0, s, a);
  FP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(bop_errors_finish_kernel, dim3((n_poses + 63) / 64), dim3(64), 0, s, slab, n_poses, n_tiles, a.n_k, which, mssd, mspd);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

int launch_vsd_count(const float *dt, size_t dt_stride, const float *dg, size_t dg_stride, const float *de, int n_poses, int H, int W,
                     const double *K, double diameter, double delta, const double *taus, int n_taus, unsigned *counts, hipStream_t s) {
  if (n_poses == 0) return FP_OK;
  VsdArgs a;
  a.dt = dt, a.dg = dg, a.de = de;
  a.dt_stride = dt_stride, a.dg_stride = dg_stride, a.de_stride = (size_t)H * W;
  a.H = H, a.W = W, a.n_taus = n_taus;
  a.rows = std::max(1, VSD_BAND_PIXELS / W);
  a.cx = K[2], a.cy = K[5], a.inv_fx = 1.0 / K[0], a.inv_fy = 1.0 / K[4];
  a.diameter = diameter, a.delta = delta;
  for (int t = 0; t < FP_VSD_MAX_TAUS; ++t) a.taus[t] = t < n_taus ? taus[t] : 0.0;
  a.counts = counts;
  const int bands = (H + a.rows - 1) / a.rows;
  hipLaunchKernelGGL(vsd_count_kernel, dim3(bands, n_poses), dim3(VSD_THREADS), 0, s, a);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

int launch_vsd_finish(const unsigned *counts, int n_poses, int n_taus, float *err, int *counts_out, hipStream_t s) {
  const int n = n_poses * n_taus;
  hipLaunchKernelGGL(vsd_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, s, counts, n_poses, n_taus, err, counts_out);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
