// The tail of a RefineNet pass behind the transformer heads: token mean + output Linear of a head (mean_head_kernel), both heads' means and
// Linears, the pose update and the next iteration's crop windows as one launch (refine_tail_kernel), and the pose update alone
// (pose_update_kernel).
//
// Reference: learning/models/refine_network.py:88-91; pose update: learning/training/predict_pose_refine.py:195-231 + pytorch3d
// so3_exp_map + src/Utils.py:848-855.
#include "common.h"
#include "device_util.h"
#include "pose_math.h"

// Token mean + output Linear behind the final LayerNorm of a RefineNet head:
// mean_t(Linear(LN(x_t))) == Linear(mean_t LN(x_t))  (refine_network.py:90-91).  The LayerNorm itself runs in the epilogue of
// linear2 (tok_gemm.hip, EPI_LNSUM), which leaves the sums of the normalised rows over groups of 16 tokens; one small workgroup
// per hypothesis adds these partial rows in a fixed order (deterministic), applies gamma / beta and the output Linear.
// (a) the 512 features of hypothesis b: partial rows added in a fixed order, gamma / beta applied -> meanv.  NH heads at once: every
// load of every head is in flight before the first add (one memory round trip; a loop that waits per load was 25 of them)
#define MH_MAXPARTS 32
template <int NH>
__device__ __forceinline__ void mean_head_rows(float (*meanv)[512], int b, const float *const *partial, int nparts, const float *const *gam,
                                               const float *const *bet, int T) {
  const int f = threadIdx.x;
  float v[NH][MH_MAXPARTS];
#pragma unroll
  for (int h = 0; h < NH; ++h)
#pragma unroll
    for (int u = 0; u < MH_MAXPARTS; ++u) v[h][u] = partial[h][((size_t)b * nparts + min(u, nparts - 1)) * 512 + f];
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    float m = 0.f;
#pragma unroll
    for (int u = 0; u < MH_MAXPARTS; ++u)
      if (u < nparts) m += v[h][u];
    meanv[h][f] = m * (1.f / (float)T) * gam[h][f] + bet[h][f];
  }
}
// (b) output `o` of the head Linear by one wave
__device__ __forceinline__ float mean_head_out(const float *meanv, const float *__restrict__ hw, const float *__restrict__ hb, int o, int lane) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += meanv[lane * 8 + i] * hw[(size_t)o * 512 + lane * 8 + i];
  s = wave_sum(s);
  return s + hb[o];
}

__global__ __launch_bounds__(512) void mean_head_kernel(const float *__restrict__ partial, int nparts, const float *__restrict__ gam,
                                                        const float *__restrict__ bet, int T, const float *__restrict__ hw,
                                                        const float *__restrict__ hb, int out_dim, float *__restrict__ out) {
  __shared__ float meanv[1][512];
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float *p1[1] = {partial}, *g1[1] = {gam}, *b1[1] = {bet};
  mean_head_rows<1>(meanv, b, p1, nparts, g1, b1, T);
  __syncthreads();
  for (int o = wave; o < out_dim; o += 8) {
    const float r = mean_head_out(meanv[0], hw, hb, o, lane);
    if (lane == 0) out[(size_t)b * out_dim + o] = r;
  }
}

// The tail of a refinement pass in ONE launch behind the join of the two heads: token mean + output Linear of the translation head
// and of the rotation head (two mean_head_kernel launches), the pose update (pose_update_kernel) and - when another iteration
// follows - its crop windows (crop_window_tf_kernel): four dependent launches of a few microseconds each, a workgroup per hypothesis.
// Every piece is the building block's own device function: the results are those of the four launches bit for bit.
// OBJS (a pass of fp_track_objects, hypothesis b = object b): trans_scale, the window radius, cneg and the centred output are object b's,
// and the updated pose is also copied to the object's own buffer
template <bool OBJS>
__global__ __launch_bounds__(512) void refine_tail_kernel(RefineTailArgs a) {
  __shared__ float meanv[2][512], delta[2][8];      // delta: this hypothesis' head outputs (also written to a.trans / a.rot)
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  mean_head_rows<2>(meanv, b, a.partial, a.nparts, a.gam, a.bet, a.T);
  __syncthreads();
  for (int o = wave; o < 3 + a.rot_dim; o += 8) {
    const int h = o >= 3, oh = h ? o - 3 : o;
    const float r = mean_head_out(meanv[h], a.hw[h], a.hb[h], oh, lane);
    if (lane == 0) {
      (h ? a.rot + (size_t)b * a.rot_dim : a.trans + (size_t)b * 3)[oh] = r;
      delta[h][oh] = r;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  DeepimArgs dp;
  dp.tf = a.tf;
  dp.resize = a.resize;
  for (int i = 0; i < 9; ++i) dp.K[i] = a.K[i];
  if constexpr (OBJS) {
    pose_update_one(b, a.poses, delta[0], delta[1], a.rot_dim, a.trans_tanh, a.tn0, a.tn1, a.tn2, a.rot_normalizer, a.obj.trans_scale[b], dp, a.poses);
    if (a.next_window) {
      CropWindowK w = a.win;
      w.radius = a.obj.radius[b];
      crop_window_tf_one(b, a.poses, w, a.tf, a.bbox);
    }
    const float *p = a.poses + (size_t)b * 16;
    if (float *c = a.obj.centered[b]) pose_of_mesh_one(p, a.obj.cneg[b], c);
    if (float *o = a.obj.pose_out[b])
#pragma unroll
      for (int i = 0; i < 16; ++i) o[i] = p[i];
  } else {
    pose_update_one(b, a.poses, delta[0], delta[1], a.rot_dim, a.trans_tanh, a.tn0, a.tn1, a.tn2, a.rot_normalizer, a.trans_scale, dp, a.poses);
    if (a.next_window) crop_window_tf_one(b, a.poses, a.win, a.tf, a.bbox);
    if (a.centered) pose_of_mesh_one(a.poses + (size_t)b * 16, a.cneg, a.centered + (size_t)b * 16);
  }
}

int launch_refine_tail(const RefineTailArgs &a, int N, hipStream_t s) {
  FP_REQUIRE(a.rot_dim == 3 || a.rot_dim == 6, "refine tail: rot_dim must be 3 or 6");
  FP_REQUIRE(a.nparts >= 1 && a.nparts <= MH_MAXPARTS, "refine tail: %d partial rows per hypothesis (at most %d)", a.nparts, MH_MAXPARTS);
  FP_REQUIRE(a.obj.n == 0 || (a.obj.n == N && N <= FP_TRACK_MAX_OBJECTS), "refine tail: %d hypotheses for %d objects", N, a.obj.n);
  if (N == 0) return FP_OK;
  if (a.obj.n) hipLaunchKernelGGL(refine_tail_kernel<true>, dim3(N), dim3(512), 0, s, a);
  else hipLaunchKernelGGL(refine_tail_kernel<false>, dim3(N), dim3(512), 0, s, a);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

int launch_mean_head(const float *partial, int nparts, const float *g, const float *b, int Bn, int T, const float *hw, const float *hb,
                     int out_dim, float *out, hipStream_t s) {
  FP_REQUIRE(nparts >= 1 && nparts <= MH_MAXPARTS, "mean_head: %d partial rows per hypothesis (at most %d)", nparts, MH_MAXPARTS);
  if (Bn == 0) return FP_OK;
  hipLaunchKernelGGL(mean_head_kernel, dim3(Bn), dim3(512), 0, s, partial, nparts, g, b, T, hw, hb, out_dim, out);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

// pose update (predict_pose_refine.py:195-231): float32, mirrors oracle/predict.py:pose_update (pose_math.h)
__global__ void pose_update_kernel(const float *__restrict__ poseA, const float *__restrict__ trans, const float *__restrict__ rot,
                                   int N, int rot_dim, int trans_tanh, float tn0, float tn1, float tn2, float rot_normalizer,
                                   float trans_scale, DeepimArgs dp, float *__restrict__ outp) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= N) return;
  pose_update_one(b, poseA, trans + (size_t)b * 3, rot + (size_t)b * rot_dim, rot_dim, trans_tanh, tn0, tn1, tn2, rot_normalizer, trans_scale, dp, outp);
}

int launch_pose_update(const float *poseA, const float *trans, const float *rot, int N, int rot_dim, int trans_tanh, float tn0,
                       float tn1, float tn2, float rot_normalizer, float trans_scale, float *out, hipStream_t s, const float *tf,
                       const double *K, float resize) {
  FP_REQUIRE(rot_dim == 3 || rot_dim == 6, "pose_update: rot_dim must be 3 or 6");
  FP_REQUIRE(trans_tanh >= 0 && trans_tanh <= 2, "pose_update: trans mode %d unknown (0 raw, 1 tanh, 2 deepim)", trans_tanh);
  FP_REQUIRE(trans_tanh != 2 || (tf && K), "pose_update: trans_rep='deepim' needs the crop transforms and K");
  if (N == 0) return FP_OK;
  DeepimArgs dp;
  dp.tf = tf;
  dp.resize = resize;
  for (int i = 0; i < 9; ++i) dp.K[i] = K ? (float)K[i] : 0.f;
  hipLaunchKernelGGL(pose_update_kernel, dim3((N + 63) / 64), dim3(64), 0, s, poseA, trans, rot, N, rot_dim, trans_tanh, tn0, tn1, tn2,
                     rot_normalizer, trans_scale, dp, out);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
