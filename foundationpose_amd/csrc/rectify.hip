// Warping images and depth maps through a camera model: undistortion and stereo rectification (fp_remap).  The rule is stated in
// include/foundationpose_amd.h and restated in numpy by tests/rectify_oracle.py; the map is fp32 with every operation rounded once in the
// written order (the library is built without contraction), the colour blend is integer, the depth rule one correctly rounded division:
// this file has to match the oracle bit for bit, and does so on every run and in any batch.
//
//   * remap_kernel<MODE, CH>: one launch for all images of a call.  blockIdx.y is the side (the plan): the plans are kernel arguments
//     and the side is uniform in the block, so a plan's numbers arrive as scalar loads.  A thread owns RM_PX = 4 consecutive
//     destination pixels of its side's flat (image, row, col) order, computes the map once per pixel and samples all channels, and
//     writes whole dwords: 4 grey pixels are one dword, 4 RGB pixels three, 4 depths one float4, 4 validity bytes one dword, 4 map
//     entries two float4.  The last pixels of a side, and outputs that are not 16-byte aligned, take element stores.
//   * The source is gathered: four taps a pixel and channel from two source rows (bytes), one in depth mode.  Neighbouring destination
//     pixels read neighbouring source pixels, so the taps of a wave fall into a few cache lines.
// No working memory, no atomics, no synchronisation: one launch on the caller's stream.
#include "common.h"
#include "view_geom.h"

namespace {

constexpr int RM_THREADS = 256;
constexpr int RM_PX = 4;      // destination pixels of one thread

struct RemapPlans {
  fp_remap_plan p[2];
};

struct RemapSide {
  const void *src;
  void *dst;
  uint8_t *valid;
  float *map;
};

struct RemapSides {
  RemapSide s[2];
};

struct MapHit {
  float u, v, Z;
  bool ray;      // steps 3 and 5 of the rule passed
};

// step 1 of the rule, with exactly its parentheses
__device__ __forceinline__ MapHit remap_map(const fp_remap_plan &P, float col, float row) {
  const Pinhole kn{P.k_new[0], P.k_new[1], P.k_new[2], P.k_new[3], P.dst_h, P.dst_w};
  const float x = pinhole_ray_x(kn, col), y = pinhole_ray_y(kn, row);
  const float X = mat3_row(P.rot, 0, x, y, 1.f), Y = mat3_row(P.rot, 1, x, y, 1.f), Z = mat3_row(P.rot, 2, x, y, 1.f);
  MapHit h;
  h.Z = Z;
  h.u = h.v = __int_as_float(0x7fc00000);
  h.ray = Z > 0.f;
  if (h.ray) {
    const float xr = X / Z, yr = Y / Z;
    const float r2 = xr * xr + yr * yr;
    h.ray = r2 < P.r2_max;
    if (h.ray) {
      const float *k = P.dist;
      const float radial = (1.f + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))) / (1.f + r2 * (k[5] + r2 * (k[6] + r2 * k[7])));
      const float xy2 = 2.f * (xr * yr);
      const float xd = (xr * radial + k[2] * xy2) + k[3] * (r2 + 2.f * (xr * xr));
      const float yd = (yr * radial + k[2] * (r2 + 2.f * (yr * yr))) + k[3] * xy2;
      h.u = P.k_raw[0] * xd + P.k_raw[2];
      h.v = P.k_raw[1] * yd + P.k_raw[3];
    }
  }
  return h;
}

// MODE 0: uint8 with CH channels; MODE 1: float32 depth (CH = 1).  total = the destination pixels of one side (images x H_dst x W_dst).
template <int MODE, int CH>
__global__ __launch_bounds__(RM_THREADS) void remap_kernel(RemapPlans plans, RemapSides sides, long long total, float zfar, int vec) {
  const int side = blockIdx.y;
  const fp_remap_plan &P = plans.p[side];
  const RemapSide &S = sides.s[side];
  const long long p0 = ((long long)blockIdx.x * RM_THREADS + threadIdx.x) * RM_PX;
  if (p0 >= total) return;
  const int cnt = total - p0 < RM_PX ? (int)(total - p0) : RM_PX;
  const int Hs = P.src_h, Ws = P.src_w, Hd = P.dst_h, Wd = P.dst_w;
  const long long hw = (long long)Hd * Wd;
  long long img = p0 / hw;
  const int rem = (int)(p0 - img * hw);
  int row = rem / Wd, col = rem - row * Wd;
  const size_t src_image = (size_t)Hs * (size_t)Ws * CH;      // elements
  const float fu_max = (float)((Ws - 1) * 256), fv_max = (float)((Hs - 1) * 256);      // exact: a side is at most 16384

  uint32_t pix[MODE == 0 ? CH : 1] = {};      // colour: the 4 CH bytes of the thread in memory order
  float dep[RM_PX] = {};
  float mu[RM_PX], mv[RM_PX];
  uint32_t ok = 0;      // byte k = validity of pixel k
#pragma unroll
  for (int k = 0; k < RM_PX; ++k) {
    mu[k] = mv[k] = 0.f;
    if (k < cnt) {
      const MapHit h = remap_map(P, (float)col, (float)row);
      mu[k] = h.u, mv[k] = h.v;
      if (MODE == 0) {
        const float fu = floorf(h.u * 256.f + 0.5f), fv = floorf(h.v * 256.f + 0.5f);
        const bool in = h.ray && fu >= 0.f && fu <= fu_max && fv >= 0.f && fv <= fv_max;
        if (in) {
          const int qu = (int)fu, qv = (int)fv;
          const int u0 = qu >> 8, a = qu & 255, v0 = qv >> 8, b = qv & 255;
          const int u1 = min(u0 + 1, Ws - 1), v1 = min(v0 + 1, Hs - 1);      // reached only with weight 0
          const uint8_t *s = static_cast<const uint8_t *>(S.src) + (size_t)img * src_image;
          const uint8_t *r0 = s + (size_t)v0 * Ws * CH, *r1 = s + (size_t)v1 * Ws * CH;
          const int w00 = (256 - a) * (256 - b), w01 = a * (256 - b), w10 = (256 - a) * b, w11 = a * b;
#pragma unroll
          for (int c = 0; c < CH; ++c) {
            const int v = (w00 * r0[u0 * CH + c] + w01 * r0[u1 * CH + c] + w10 * r1[u0 * CH + c] + w11 * r1[u1 * CH + c] + 32768) >> 16;
            const int byte = k * CH + c;
            pix[byte >> 2] |= (uint32_t)v << ((byte & 3) * 8);
          }
          ok |= 1u << (k * 8);
        }
      } else {
        const float cf = floorf(h.u + 0.5f), rf = floorf(h.v + 0.5f);
        const bool in = h.ray && cf >= 0.f && cf <= (float)(Ws - 1) && rf >= 0.f && rf <= (float)(Hs - 1);
        if (in) {
          const float d = (static_cast<const float *>(S.src) + (size_t)img * src_image)[(size_t)(int)rf * Ws + (int)cf];
          if (depth_ok(d, zfar)) dep[k] = d / h.Z;
          ok |= 1u << (k * 8);
        }
      }
      if (++col == Wd) {
        col = 0;
        if (++row == Hd) row = 0, ++img;
      }
    }
  }

  if (cnt == RM_PX && vec) {
    if (MODE == 0) {
      uint32_t *o = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(S.dst) + (size_t)p0 * CH);
#pragma unroll
      for (int w = 0; w < CH; ++w) o[w] = pix[w];
    } else {
      *reinterpret_cast<float4 *>(static_cast<float *>(S.dst) + p0) = make_float4(dep[0], dep[1], dep[2], dep[3]);
    }
    if (S.valid) *reinterpret_cast<uint32_t *>(S.valid + p0) = ok;
    if (S.map) {
      float4 *m = reinterpret_cast<float4 *>(S.map + (size_t)p0 * 2);
      m[0] = make_float4(mu[0], mv[0], mu[1], mv[1]);
      m[1] = make_float4(mu[2], mv[2], mu[3], mv[3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < RM_PX; ++k) {
      if (k >= cnt) break;
      if (MODE == 0) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int byte = k * CH + c;
          static_cast<uint8_t *>(S.dst)[(size_t)(p0 + k) * CH + c] = (uint8_t)(pix[byte >> 2] >> ((byte & 3) * 8));
        }
      } else {
        static_cast<float *>(S.dst)[p0 + k] = dep[k];
      }
      if (S.valid) S.valid[p0 + k] = (uint8_t)(ok >> (k * 8));
      if (S.map) S.map[(size_t)(p0 + k) * 2] = mu[k], S.map[(size_t)(p0 + k) * 2 + 1] = mv[k];
    }
  }
}

bool plan_values_finite(const fp_remap_plan &p) {
  bool ok = true;
  for (float v : p.k_new) ok = ok && isfinite(v);
  for (float v : p.rot) ok = ok && isfinite(v);
  for (float v : p.k_raw) ok = ok && isfinite(v);
  for (float v : p.dist) ok = ok && isfinite(v);
  return ok;
}

}  // namespace

// Every check of a value, before the first look into ctx (tests/test_rectify_host.py calls fp_remap without a GPU).
int fp_remap_check(const void *ctx, const void *d_src0, const void *d_src1, int n, const fp_remap_opts *opts, const void *d_dst0, const void *d_dst1,
                   const fp_remap_debug *dbg) {
  FP_REQUIRE(ctx && opts && d_src0 && d_dst0, "fp_remap: null argument");
  FP_REQUIRE(opts->struct_size == sizeof(fp_remap_opts), "fp_remap: fp_remap_opts.struct_size = %zu (this library knows %zu)", opts->struct_size,
             sizeof(fp_remap_opts));
  FP_REQUIRE(!dbg || dbg->struct_size == sizeof(fp_remap_debug), "fp_remap: fp_remap_debug.struct_size = %zu (this library knows %zu)",
             dbg ? dbg->struct_size : (size_t)0, sizeof(fp_remap_debug));
  FP_REQUIRE(opts->mode == FP_REMAP_COLOUR || opts->mode == FP_REMAP_DEPTH, "fp_remap: mode %d (FP_REMAP_COLOUR or FP_REMAP_DEPTH)", opts->mode);
  FP_REQUIRE(opts->channels == 1 || (opts->channels == 3 && opts->mode == FP_REMAP_COLOUR), "fp_remap: channels %d (1 or 3; a depth map has 1)",
             opts->channels);
  FP_REQUIRE(opts->n_plans == 1 || opts->n_plans == 2, "fp_remap: n_plans %d (1 or 2)", opts->n_plans);
  FP_REQUIRE(n >= 1 && n % opts->n_plans == 0, "fp_remap: n %d (>= 1 and a multiple of n_plans %d)", n, opts->n_plans);
  FP_REQUIRE(opts->n_plans == 1 || (d_src1 && d_dst1), "fp_remap: n_plans 2 needs d_src1 and d_dst1");
  for (int i = 0; i < opts->n_plans; ++i) {
    const fp_remap_plan &p = opts->plan[i];
    FP_REQUIRE(p.src_h >= 1 && p.src_w >= 1 && p.dst_h >= 1 && p.dst_w >= 1 && p.src_h <= FP_REMAP_MAX_SIDE && p.src_w <= FP_REMAP_MAX_SIDE &&
                   p.dst_h <= FP_REMAP_MAX_SIDE && p.dst_w <= FP_REMAP_MAX_SIDE,
               "fp_remap: plan %d maps %d x %d to %d x %d (each side 1 .. %d)", i, p.src_h, p.src_w, p.dst_h, p.dst_w, FP_REMAP_MAX_SIDE);
    FP_REQUIRE(p.src_h == opts->plan[0].src_h && p.src_w == opts->plan[0].src_w && p.dst_h == opts->plan[0].dst_h && p.dst_w == opts->plan[0].dst_w,
               "fp_remap: the two plans differ in size (%d x %d -> %d x %d and %d x %d -> %d x %d)", opts->plan[0].src_h, opts->plan[0].src_w,
               opts->plan[0].dst_h, opts->plan[0].dst_w, p.src_h, p.src_w, p.dst_h, p.dst_w);
    FP_REQUIRE(plan_values_finite(p), "fp_remap: plan %d holds a value that is not finite", i);
    FP_REQUIRE(p.k_new[0] > 0.f && p.k_new[1] > 0.f && p.k_raw[0] > 0.f && p.k_raw[1] > 0.f, "fp_remap: plan %d: fx, fy of both cameras must be > 0", i);
    FP_REQUIRE(p.r2_max > 0.f, "fp_remap: plan %d: r2_max %g (> 0; infinity: no limit)", i, (double)p.r2_max);      // refuses a NaN too
  }
  FP_REQUIRE((double)(n / opts->n_plans) * (double)opts->plan[0].dst_h * (double)opts->plan[0].dst_w <= (double)(1LL << 40),
             "fp_remap: %d images of %d x %d pixels (at most 2^40 destination pixels a plan)", n, opts->plan[0].dst_h, opts->plan[0].dst_w);
  if (opts->mode == FP_REMAP_DEPTH) FP_REQUIRE(opts->zfar > 0.f, "fp_remap: zfar %g (> 0; infinity: no limit)", (double)opts->zfar);
  return FP_OK;
}

extern "C" int fp_remap(fp_ctx *ctx, const void *d_src0, const void *d_src1, int n, const fp_remap_opts *opts, void *d_dst0, void *d_dst1, uint8_t *d_valid0,
                        uint8_t *d_valid1, const fp_remap_debug *dbg, void *stream) {
  FP_TRY(fp_remap_check(ctx, d_src0, d_src1, n, opts, d_dst0, d_dst1, dbg));
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  const int sides = opts->n_plans;
  RemapPlans plans;
  plans.p[0] = opts->plan[0], plans.p[1] = opts->plan[sides - 1];
  RemapSides io{};
  io.s[0] = RemapSide{d_src0, d_dst0, d_valid0, dbg ? dbg->d_map0 : nullptr};
  if (sides == 2) io.s[1] = RemapSide{d_src1, d_dst1, d_valid1, dbg ? dbg->d_map1 : nullptr};
  int vec = 1;      // dword and float4 stores need their alignment at pixel 0 of a side
  for (int i = 0; i < sides; ++i)
    vec = vec && (uintptr_t)io.s[i].dst % 16 == 0 && (uintptr_t)io.s[i].valid % 4 == 0 && (uintptr_t)io.s[i].map % 16 == 0;
  const fp_remap_plan &p = opts->plan[0];
  const long long total = (long long)(n / sides) * p.dst_h * p.dst_w;
  const dim3 grid((unsigned)((total + RM_THREADS * RM_PX - 1) / (RM_THREADS * RM_PX)), (unsigned)sides);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(ctx, s, "remap", 0.0);
  if (opts->mode == FP_REMAP_DEPTH) hipLaunchKernelGGL((remap_kernel<1, 1>), grid, dim3(RM_THREADS), 0, s, plans, io, total, opts->zfar, vec);
  else if (opts->channels == 1) hipLaunchKernelGGL((remap_kernel<0, 1>), grid, dim3(RM_THREADS), 0, s, plans, io, total, 0.f, vec);
  else hipLaunchKernelGGL((remap_kernel<0, 3>), grid, dim3(RM_THREADS), 0, s, plans, io, total, 0.f, vec);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
