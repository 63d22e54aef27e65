// Kernels around the networks of a multi-object registration (fp_register_objects; FoundationPose.register, src/estimater.py:159-240, for
// several objects of one frame): the mask reductions of every object in one launch, the hypothesis sets built on the device, and the
// per-object ranking that ends the call.
#include <hip/hip_runtime.h>

#include "common.h"

// ---- mask reductions of all objects (src/estimater.py:137-156,173-177 per object): workgroup o reduces object o.  mask_depth_stats_kernel
// (crop.hip) scans the whole image five times for one object; here one launch covers every object, the first scan (bounding box and counts)
// is the only one over the whole image, and the four radix-select passes scan the object's bounding box alone - every usable pixel lies
// inside it, so the histograms, and with them the two order statistics, are those of the full scan.  Same arithmetic for the even count.
// out + 8 o: [0] cmin [1] cmax [2] rmin [3] rmax [4] n_mask [5] n_usable [6] median (float bits) [7] 0
__global__ __launch_bounds__(1024) void mask_depth_stats_objects_kernel(const float *__restrict__ depth, MaskStatsObjs ob, int H, int W, float min_depth,
                                                                        int *__restrict__ out) {
  __shared__ int s_red[6];
  __shared__ unsigned s_hist[2][256];
  __shared__ unsigned s_prefix[2], s_rank[2];
  const int o = blockIdx.x, n = H * W, tid = threadIdx.x;
  const unsigned char *__restrict__ mask = ob.mask[o];
  const int *__restrict__ labels = ob.labels;
  const int label = ob.label[o];
  int *res = out + (size_t)o * 8;
  if (tid == 0) {
    s_red[0] = 0x7fffffff; s_red[1] = -1; s_red[2] = 0x7fffffff; s_red[3] = -1; s_red[4] = 0; s_red[5] = 0;
  }
  __syncthreads();
  int cmin = 0x7fffffff, cmax = -1, rmin = 0x7fffffff, rmax = -1, nm = 0, nu = 0;
  for (int i = tid; i < n; i += blockDim.x) {
    const bool in = labels ? labels[i] == label : mask[i] != 0;
    if (in) {
      const int r = i / W, c = i - r * W;
      cmin = min(cmin, c); cmax = max(cmax, c); rmin = min(rmin, r); rmax = max(rmax, r);
      ++nm;
      if (depth[i] >= min_depth) ++nu;
    }
  }
  if (nm) {
    atomicMin(&s_red[0], cmin); atomicMax(&s_red[1], cmax); atomicMin(&s_red[2], rmin); atomicMax(&s_red[3], rmax);
    atomicAdd(&s_red[4], nm); atomicAdd(&s_red[5], nu);
  }
  __syncthreads();
  const int n_us = s_red[5];
  const int c0 = s_red[0], r0 = s_red[2], bw = s_red[1] - s_red[0] + 1, bh = s_red[3] - s_red[2] + 1;
  if (tid < 6) res[tid] = s_red[tid];
  if (tid == 7) res[7] = 0;
  if (n_us == 0) {
    if (tid == 0) res[6] = 0;          // (0.f)
    return;
  }
  // usable depths are >= min_depth > 0: their bit patterns order like the values.  8-bit radix select, both order statistics at once.
  if (tid < 2) {
    s_prefix[tid] = 0;
    s_rank[tid] = tid == 0 ? (unsigned)((n_us - 1) / 2) : (unsigned)(n_us / 2);
  }
  const int nb = bw * bh;               // (1 .. H * W)
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = tid; i < 512; i += blockDim.x) s_hist[i >> 8][i & 255] = 0;
    __syncthreads();
    const unsigned p0 = s_prefix[0], p1 = s_prefix[1];
    const unsigned hi_mask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    for (int j = tid; j < nb; j += blockDim.x) {
      const int br = j / bw;
      const int i = (r0 + br) * W + c0 + (j - br * bw);
      const bool in = labels ? labels[i] == label : mask[i] != 0;
      if (in) {
        const float z = depth[i];
        if (z >= min_depth) {
          const unsigned u = __float_as_uint(z);
          const unsigned d = (u >> shift) & 255u;
          if ((u & hi_mask) == (p0 & hi_mask)) atomicAdd(&s_hist[0][d], 1u);
          if ((u & hi_mask) == (p1 & hi_mask)) atomicAdd(&s_hist[1][d], 1u);
        }
      }
    }
    __syncthreads();
    if (tid < 2) {
      unsigned r = s_rank[tid], cum = 0;
      int d = 0;
      for (; d < 255; ++d) {
        const unsigned c = s_hist[tid][d];
        if (r < cum + c) break;
        cum += c;
      }
      s_rank[tid] = r - cum;
      s_prefix[tid] |= (unsigned)d << shift;
    }
    __syncthreads();
  }
  if (tid == 0) res[6] = (int)__float_as_uint(__fmul_rn(__fadd_rn(__uint_as_float(s_prefix[0]), __uint_as_float(s_prefix[1])), 0.5f));
}

int launch_mask_depth_stats_objects(const float *d, const MaskStatsObjs &ob, int H, int W, float min_depth, int *out8, hipStream_t s) {
  FP_REQUIRE(ob.n >= 1 && ob.n <= FP_TRACK_MAX_OBJECTS, "mask stats: %d objects", ob.n);
  hipLaunchKernelGGL(mask_depth_stats_objects_kernel, dim3(ob.n), dim3(1024), 0, s, d, ob, H, W, min_depth, out8);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

// ---- hypothesis sets (src/estimater.py:126-156,196-199: generate_random_pose_hypo over guess_translation): hypothesis i of object o is
// rot_grid[o][i] with the translation (inv(K) @ [uc, vc, 1]) * median, uc / vc the centre of the mask's bounding box.  float64 as numpy
// computes it - the 3-term dot product in the order numpy's matmul takes, fma(k0, uc, k1 * vc) + k2 -, rounded once to float32.
__global__ __launch_bounds__(64) void register_hypotheses_kernel(RegHypObjs ob, float *__restrict__ poses) {
  const int o = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ob.n[o]) return;
  const double uc = (double)(ob.cmin[o] + ob.cmax[o]) / 2.0, vc = (double)(ob.rmin[o] + ob.rmax[o]) / 2.0;
  const double med = (double)ob.median[o];
  const float *g = ob.rot_grid[o] + (size_t)i * 16;
  float *p = poses + ((size_t)ob.off[o] + i) * 16;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double ray = __dadd_rn(__fma_rn(ob.kinv[r * 3], uc, __dmul_rn(ob.kinv[r * 3 + 1], vc)), ob.kinv[r * 3 + 2]);
    p[r * 4 + 0] = g[r * 4 + 0];
    p[r * 4 + 1] = g[r * 4 + 1];
    p[r * 4 + 2] = g[r * 4 + 2];
    p[r * 4 + 3] = (float)__dmul_rn(ray, med);
  }
  p[12] = g[12], p[13] = g[13], p[14] = g[14], p[15] = g[15];
}

int launch_register_hypotheses(const RegHypObjs &ob, float *poses, hipStream_t s) {
  FP_REQUIRE(ob.n_obj >= 1 && ob.n_obj <= FP_TRACK_MAX_OBJECTS, "hypothesis sets: %d objects", ob.n_obj);
  int n_max = 0;
  for (int o = 0; o < ob.n_obj; ++o) n_max = ob.n[o] > n_max ? ob.n[o] : n_max;
  if (n_max == 0) return FP_OK;
  hipLaunchKernelGGL(register_hypotheses_kernel, dim3((n_max + 63) / 64, ob.n_obj), dim3(64), 0, s, ob, poses);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

// ---- ranking (src/estimater.py:230-237: scores.argsort(descending=True), poses[order], scores[order], best_id, pose_last and
// pose_last @ get_tf_to_centered_mesh()): workgroup o ranks object o.  The rank of hypothesis i is the number of hypotheses that come before
// it in the stable descending order (a greater score, or an equal one at a lower index), so every rank is taken exactly once; NaN ranks
// above every number and -0.0 equals +0.0, as torch sorts them.  pose_of_mesh: the rotation block is copied, column 3 is the dot product
// row . (cneg, 1) in the order of torch's float32 matrix product on this device (a chain of fused multiply-adds from the left).
__device__ __forceinline__ unsigned rank_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);        // monotone in v; +NaN patterns lie above +inf
}
// the key of a score: every NaN is one key above +inf, and -0.0 takes the key of +0.0 (the two compare equal, so their order is the index order)
__device__ __forceinline__ unsigned score_key(float v) {
  return rank_key(v != v ? __uint_as_float(0x7fc00000u) : (v == 0.f ? 0.f : v));
}

__global__ __launch_bounds__(256) void register_rank_kernel(RegRankObjs ob, const float *__restrict__ poses, const float *__restrict__ scores) {
  const int o = blockIdx.x, n = ob.n[o];
  const float *sc = scores + ob.off[o];
  const float *ps = poses + (size_t)ob.off[o] * 16;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float v = sc[i];
    const unsigned k = score_key(v);
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const unsigned kj = score_key(sc[j]);
      rank += (kj > k || (kj == k && j < i)) ? 1 : 0;
    }
    ob.scores_out[o][rank] = v;
    ob.order_out[o][rank] = (long long)i;
    const float *p = ps + (size_t)i * 16;
    float *q = ob.poses_out[o] + (size_t)rank * 16;
#pragma unroll
    for (int e = 0; e < 16; ++e) q[e] = p[e];
    if (rank == 0) {
      float *c = ob.pose_of_mesh[o];
      const float *cn = ob.cneg[o];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        c[r * 4 + 0] = p[r * 4 + 0];
        c[r * 4 + 1] = p[r * 4 + 1];
        c[r * 4 + 2] = p[r * 4 + 2];
        c[r * 4 + 3] = __fadd_rn(__fmaf_rn(p[r * 4 + 2], cn[2], __fmaf_rn(p[r * 4 + 1], cn[1], __fmul_rn(p[r * 4 + 0], cn[0]))), p[r * 4 + 3]);
      }
    }
  }
}

int launch_register_rank(const RegRankObjs &ob, const float *poses, const float *scores, hipStream_t s) {
  FP_REQUIRE(ob.n_obj >= 1 && ob.n_obj <= FP_TRACK_MAX_OBJECTS, "ranking: %d objects", ob.n_obj);
  hipLaunchKernelGGL(register_rank_kernel, dim3(ob.n_obj), dim3(256), 0, s, ob, poses, scores);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
