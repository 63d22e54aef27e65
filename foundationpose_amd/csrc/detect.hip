// Finding an object in a depth frame without a mask (fp_template_match): depth templates of the model - in-samples on the silhouette,
// out-samples on a ring outside it, both as 3-D offsets from the object's centre - matched at every pixel of an anchor lattice.  The depth at
// the anchor pixel fixes the scale, so a candidate is (template, anchor sample, anchor pixel) and its centre follows in closed form.  The
// rule is stated in include/foundationpose_amd.h and restated in numpy by tests/detect_oracle.py; everything is fp32 with every operation
// rounded once in the written order (the library is built without contraction), so this file has to match the oracle bit for bit, on
// every run and in any batch.
//
//   * template_match_kernel: a workgroup is ONE wave and takes an 8 x 8 tile of the anchor lattice, a lane per anchor pixel; blockIdx.y is
//     the object and blockIdx.z the frame.  The object's templates stream through LDS in chunks of TM_LDS_SAMPLES float4 samples
//     (fp_template_match_info tells how many templates that is); every lane reads the same sample at the same time, which LDS broadcasts.
//     The depth gathers of one template fall into a window of about the tile plus one object footprint and are left to the vector cache:
//     a 640 x 480 frame is 1.2 MB, far inside L2, and staging the window would cost a barrier per template.
//   * A lane carries the maximum key of its pixel in a register and writes it once: no atomics, and the key's low half orders equal
//     scores by the lowest (template, anchor), so the result does not depend on the order of anything.
//   * The prune is exact: a candidate is left as soon as the passes still possible cannot lift its key above the running maximum.  The
//     winner is never pruned, so its counts are exact too.
// No allocation and no host synchronisation: one launch, which can be captured into a graph.
#include "common.h"
#include "view_geom.h"

namespace {

constexpr int TM_TILE_W = 8, TM_TILE_H = 8, TM_THREADS = TM_TILE_W * TM_TILE_H;      // one wave
constexpr int TM_LDS_SAMPLES = 1024;      // float4 samples of a staged chunk: 16 KB
constexpr int TM_PRUNE_EVERY = 8;         // samples between two looks at the bound

struct MatchRanges {
  int v[FP_TEMPLATE_MAX_OBJECTS + 1];
};

struct MatchArgs {
  Pinhole cam;
  int n_in, n_out, anchors, stride, r0, c0, Hs, Ws, n_obj, chunk;
  float z_min, z_max, zfar, tol_in, tol_out;
};

// One sample of a candidate centred at (Cx, Cy, zc): where its depth is to be read and whether there is anything to read.  Branch-free -
// a sample that fails reads pixel 0 and is not counted - so that the gathers of a group of samples are in flight together: with one wave
// on a SIMD the kernel is bound by the latency of these gathers.  Nothing huge and no NaN reaches a cast.
struct Probe {
  float Z;
  int at;
  bool ok;
};

__device__ __forceinline__ Probe probe_sample(const Pinhole &cam, float Cx, float Cy, float zc, const float4 S) {
  Probe p;
  const float X = Cx + S.x, Y = Cy + S.y;
  p.Z = zc + S.z;
  const PixelHit h = project_icp(cam, X, Y, p.Z);
  p.ok = p.Z >= 0.001f && h.in;
  p.at = (int)(p.ok ? h.rf : 0.f) * cam.W + (int)(p.ok ? h.cf : 0.f);
  return p;
}

// the passes among samples [s0, s0 + N) of S: in-samples (o >= 0.001 and |o - Z| <= tol) or out-samples (no reading, or |o - Z| > tol)
template <int N, bool IN>
__device__ __forceinline__ int count_passes(const Pinhole &cam, const float *__restrict__ D, float Cx, float Cy, float zc, const float4 *S, int s0,
                                            float tol) {
  Probe p[N];
  float o[N];
#pragma unroll
  for (int k = 0; k < N; ++k) p[k] = probe_sample(cam, Cx, Cy, zc, S[s0 + k]);
#pragma unroll
  for (int k = 0; k < N; ++k) o[k] = D[p[k].at];
  int n = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const bool pass = IN ? (o[k] >= 0.001f && fabsf(o[k] - p[k].Z) <= tol) : (!(o[k] >= 0.001f) || fabsf(o[k] - p[k].Z) > tol);
    n += (p[k].ok && pass) ? 1 : 0;
  }
  return n;
}

__global__ __launch_bounds__(TM_THREADS) void template_match_kernel(MatchArgs a, MatchRanges ranges, const float *__restrict__ depth,
                                                                    const float4 *__restrict__ table, uint32_t *__restrict__ keys,
                                                                    uint32_t *__restrict__ counts) {
  __shared__ float4 lds[TM_LDS_SAMPLES];
  const int tiles_w = (a.Ws + TM_TILE_W - 1) / TM_TILE_W;
  const int tile_r = blockIdx.x / tiles_w, tile_c = blockIdx.x - tile_r * tiles_w;
  const int lane = threadIdx.x;
  const int i = tile_r * TM_TILE_H + lane / TM_TILE_W, j = tile_c * TM_TILE_W + lane % TM_TILE_W;      // the lattice point of this lane
  const int obj = blockIdx.y, frame = blockIdx.z;
  const int t_begin = ranges.v[obj], t_end = ranges.v[obj + 1];
  const int ns = a.n_in + a.n_out;
  const Pinhole &cam = a.cam;
  const float *D = depth + (size_t)frame * cam.H * cam.W;

  const bool inside = i < a.Hs && j < a.Ws;
  const int r = a.r0 + i * a.stride, c = a.c0 + j * a.stride;      // inside: r < H and c < W by the definition of Hs, Ws
  const float d = inside ? D[r * cam.W + c] : 0.f;
  const bool live = depth_ok(d, a.zfar);
  const float bx = pinhole_ray_x(cam, (float)c) * d, by = pinhole_ray_y(cam, (float)r) * d;

  uint32_t best = 0, best_counts = 0;
  for (int t0 = t_begin; t0 < t_end; t0 += a.chunk) {
    const int nt = min(a.chunk, t_end - t0);
    __syncthreads();      // the previous chunk has been read by every lane
    for (int e = lane; e < nt * ns; e += TM_THREADS) lds[e] = table[(size_t)t0 * ns + e];
    __syncthreads();
    if (!live) continue;
    for (int tt = 0; tt < nt; ++tt) {
      const float4 *S = lds + tt * ns;
      const uint32_t t_local = (uint32_t)(t0 + tt - t_begin);
      for (int an = 0; an < a.anchors; ++an) {
        const uint32_t low = 0xFFFFu - (4u * t_local + (uint32_t)an);
        const float4 A = S[an];
        const float zc = d - A.z;
        if (!(zc >= a.z_min && zc <= a.z_max)) continue;
        if ((((uint32_t)(a.n_in * a.n_out)) << 16 | low) <= best) continue;
        const float Cx = bx - A.x, Cy = by - A.y;
        int n_in_pass = 0, n_out_pass = 0;
        bool pruned = false;
        // groups of TM_PRUNE_EVERY samples with their gathers in flight together, a look at the bound after each, then the rest one by one
        int s = 0;
        for (; s + TM_PRUNE_EVERY <= a.n_in && !pruned; s += TM_PRUNE_EVERY) {
          n_in_pass += count_passes<TM_PRUNE_EVERY, true>(cam, D, Cx, Cy, zc, S, s, a.tol_in);
          pruned = (((uint32_t)((n_in_pass + (a.n_in - (s + TM_PRUNE_EVERY))) * a.n_out)) << 16 | low) <= best;
        }
        if (!pruned) {
          for (; s < a.n_in; ++s) n_in_pass += count_passes<1, true>(cam, D, Cx, Cy, zc, S, s, a.tol_in);
          pruned = (((uint32_t)(n_in_pass * a.n_out)) << 16 | low) <= best;
        }
        const float4 *So = S + a.n_in;
        s = 0;
        for (; s + TM_PRUNE_EVERY <= a.n_out && !pruned; s += TM_PRUNE_EVERY) {
          n_out_pass += count_passes<TM_PRUNE_EVERY, false>(cam, D, Cx, Cy, zc, So, s, a.tol_out);
          pruned = (((uint32_t)(n_in_pass * (n_out_pass + (a.n_out - (s + TM_PRUNE_EVERY))))) << 16 | low) <= best;
        }
        if (!pruned)
          for (; s < a.n_out; ++s) n_out_pass += count_passes<1, false>(cam, D, Cx, Cy, zc, So, s, a.tol_out);
        if (pruned) continue;      // its key could not exceed the maximum, and an equal key is the same candidate
        const uint32_t key = ((uint32_t)(n_in_pass * n_out_pass)) << 16 | low;
        if (key > best) best = key, best_counts = (uint32_t)n_in_pass << 16 | (uint32_t)n_out_pass;
      }
    }
  }
  if (!inside) return;
  const size_t at = (((size_t)frame * a.n_obj + obj) * a.Hs + i) * a.Ws + j;
  keys[at] = best;
  if (counts) counts[at] = best_counts;
}

}  // namespace

extern "C" int fp_template_match_info(int n_samples, int *chunk_templates) {
  FP_REQUIRE(chunk_templates, "fp_template_match_info: null argument");
  FP_REQUIRE(n_samples >= 2 && n_samples <= FP_TEMPLATE_MAX_SAMPLES, "fp_template_match_info: %d samples a template (2 .. %d)", n_samples,
             FP_TEMPLATE_MAX_SAMPLES);
  *chunk_templates = TM_LDS_SAMPLES / n_samples;
  return FP_OK;
}

// Every check of a value, before the first look into ctx (tests/test_detect_host.py calls fp_template_match without a GPU).
int fp_template_match_check(const void *ctx, const void *d_depth, int n_frames, int H, int W, const double *K, const void *d_table,
                            const int32_t *ranges, int n_obj, int n_in, int n_out, int anchors, int stride, int r0, int c0, float z_min, float z_max,
                            float zfar, float tol_in, float tol_out, const void *d_keys) {
  FP_REQUIRE(ctx && d_depth && K && d_table && ranges && d_keys, "fp_template_match: null argument");
  FP_REQUIRE(n_frames >= 0 && n_frames <= FP_TEMPLATE_MAX_FRAMES, "fp_template_match: n_frames %d (0 .. %d)", n_frames, FP_TEMPLATE_MAX_FRAMES);
  FP_REQUIRE(H >= 1 && W >= 1 && H <= FP_REMAP_MAX_SIDE && W <= FP_REMAP_MAX_SIDE, "fp_template_match: a frame of %d x %d (each side 1 .. %d)", H, W,
             FP_REMAP_MAX_SIDE);
  FP_REQUIRE(stride >= 1, "fp_template_match: stride %d (>= 1)", stride);
  FP_REQUIRE(r0 >= 0 && r0 < H && c0 >= 0 && c0 < W, "fp_template_match: the offset (%d, %d) lies outside the %d x %d frame", r0, c0, H, W);
  FP_REQUIRE(tol_in > 0.f && tol_out > 0.f, "fp_template_match: tol_in %g, tol_out %g (both > 0)", (double)tol_in, (double)tol_out);      // a NaN too
  FP_REQUIRE(z_min <= z_max, "fp_template_match: z_min %g > z_max %g", (double)z_min, (double)z_max);      // refuses a NaN too
  FP_REQUIRE(zfar > 0.f, "fp_template_match: zfar %g (> 0; infinity: no limit)", (double)zfar);
  for (int e = 0; e < 9; ++e) FP_REQUIRE(isfinite(K[e]), "fp_template_match: K holds a value that is not finite");
  FP_TRY(fp_check_camera("fp_template_match", K));
  FP_REQUIRE(n_in >= 1 && n_out >= 1 && (long long)n_in * n_out <= 65535, "fp_template_match: n_in %d, n_out %d (each >= 1, n_in n_out <= 65535)", n_in,
             n_out);
  FP_REQUIRE(n_in + n_out <= FP_TEMPLATE_MAX_SAMPLES, "fp_template_match: %d samples a template (at most %d)", n_in + n_out, FP_TEMPLATE_MAX_SAMPLES);
  FP_REQUIRE(anchors >= 1 && anchors <= FP_TEMPLATE_MAX_ANCHORS && anchors <= n_in, "fp_template_match: anchors %d (1 .. %d, at most n_in)", anchors,
             FP_TEMPLATE_MAX_ANCHORS);
  FP_REQUIRE(n_obj >= 1 && n_obj <= FP_TEMPLATE_MAX_OBJECTS, "fp_template_match: n_obj %d (1 .. %d)", n_obj, FP_TEMPLATE_MAX_OBJECTS);
  FP_REQUIRE(ranges[0] == 0, "fp_template_match: ranges[0] is %d, not 0", ranges[0]);
  for (int o = 0; o < n_obj; ++o) {
    FP_REQUIRE(ranges[o + 1] >= ranges[o], "fp_template_match: ranges decrease at object %d", o);
    FP_REQUIRE(4LL * (ranges[o + 1] - ranges[o]) <= 65536, "fp_template_match: object %d has %d templates (at most 16384)", o, ranges[o + 1] - ranges[o]);
  }
  FP_REQUIRE((uintptr_t)d_table % 16 == 0, "fp_template_match: d_table is not 16-byte aligned");
  return FP_OK;
}

extern "C" int fp_template_match(fp_ctx *ctx, const float *d_depth, int n_frames, int H, int W, const double *K, const float *d_table,
                                 const int32_t *ranges, int n_obj, int n_in, int n_out, int anchors, int stride, int r0, int c0, float z_min,
                                 float z_max, float zfar, float tol_in, float tol_out, uint32_t *d_keys, uint32_t *d_counts, void *stream) {
  FP_TRY(fp_template_match_check(ctx, d_depth, n_frames, H, W, K, d_table, ranges, n_obj, n_in, n_out, anchors, stride, r0, c0, z_min, z_max, zfar, tol_in,
                                 tol_out, d_keys));
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  MatchArgs a{};
  a.cam = pinhole_of(K, H, W);
  a.n_in = n_in, a.n_out = n_out, a.anchors = anchors, a.stride = stride, a.r0 = r0, a.c0 = c0, a.n_obj = n_obj;
  a.Hs = (H - r0 + stride - 1) / stride, a.Ws = (W - c0 + stride - 1) / stride;
  a.chunk = TM_LDS_SAMPLES / (n_in + n_out);
  a.z_min = z_min, a.z_max = z_max, a.zfar = zfar, a.tol_in = tol_in, a.tol_out = tol_out;
  MatchRanges rg{};
  for (int o = 0; o <= n_obj; ++o) rg.v[o] = ranges[o];
  if (n_frames == 0) return FP_OK;
  const size_t cells = (size_t)n_frames * n_obj * a.Hs * a.Ws;
  if (ranges[n_obj] == 0) {      // no template: no candidate anywhere
    FP_CHECK_HIP(hipMemsetAsync(d_keys, 0, cells * sizeof(uint32_t), st));
    if (d_counts) FP_CHECK_HIP(hipMemsetAsync(d_counts, 0, cells * sizeof(uint32_t), st));
    return FP_OK;
  }
  const unsigned tiles = (unsigned)(((a.Hs + TM_TILE_H - 1) / TM_TILE_H) * ((a.Ws + TM_TILE_W - 1) / TM_TILE_W));
  ProfScope node(ctx, st, "template_match", 0.0);
  hipLaunchKernelGGL(template_match_kernel, dim3(tiles, (unsigned)n_obj, (unsigned)n_frames), dim3(TM_THREADS), 0, st, a, rg, d_depth,
                     reinterpret_cast<const float4 *>(d_table), d_keys, d_counts);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
