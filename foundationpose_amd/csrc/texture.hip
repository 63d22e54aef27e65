// Texture baking: the colours of posed RGB-D reference views gathered into a per-face texture atlas of a mesh (fp_texture_bake).  The
// atlas layout and the arithmetic are stated in include/foundationpose_amd.h and restated in numpy by tests/texture_bake_oracle.py; this
// file follows the statement operation for operation (the library is built without contraction).
//
// The kernel is a gather.  One thread per texel, the workgroup is 64 x 4 texels, so a wave is 64 consecutive texels of one atlas row:
// a run of c of them lies in one cell row and hence in at most two faces (A left of the anti-diagonal, B right of it).  The lanes of a
// run read the same three face indices and the same nine coordinates - same-address loads of one wave are one request to the cache, so
// a face's vertices are fetched once per run and not once per texel.  The view matrices are kernel arguments (a view index is uniform in
// the wave: scalar loads), the views loop inside the thread in index order, and a texel belongs to one thread: no atomics, no
// synchronisation, the same bits on every run.  Neighbouring texels of a face project to neighbouring pixels, so the depth and colour
// reads of a wave fall into a few cache lines per view.  Plain vector loads and stores; there is no LDS stage: nothing is shared beyond
// what the cache already merges.  The camera, the object -> camera transforms and the projection (the ratio rule) are those of view_geom.h.
#include "common.h"
#include "view_geom.h"

#include <math.h>

namespace {

constexpr int TB_X = 64, TB_Y = 4;

struct TexCfg {
  int T, c, g, F, V, top_n, n_views;
  float zfar, depth_tol, cos_min;
};

__device__ __forceinline__ uint8_t to_u8(float x) { return (uint8_t)fminf(fmaxf(floorf(x + 0.5f), 0.f), 255.f); }

__global__ __launch_bounds__(TB_X *TB_Y) void texture_bake_kernel(const float *__restrict__ pos, const int32_t *__restrict__ faces,
                                                                   const uint8_t *__restrict__ vcol, const uint8_t *__restrict__ rgb,
                                                                   const float *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                                   uint8_t *__restrict__ tex, int8_t *__restrict__ used, TexCfg k, Pinhole cam, Rigids views) {
  const int X = blockIdx.x * TB_X + threadIdx.x, Y = blockIdx.y * TB_Y + threadIdx.y;
  if (X >= k.T || Y >= k.T) return;
  const size_t o = (size_t)Y * k.T + X;
  const int col = X / k.c, row = Y / k.c;
  int i = X - col * k.c, j = Y - row * k.c;
  int f = -1;
  if (col < k.g && row < k.g) {
    const int cell = row * k.g + col, s = i + j;
    if (s <= k.c - 2) f = 2 * cell;
    else if (s >= k.c) f = 2 * cell + 1, i = k.c - 1 - i, j = k.c - 1 - j;
    if (f >= k.F) f = -1;
  }
  if (f < 0) {
    tex[o * 3] = 0, tex[o * 3 + 1] = 0, tex[o * 3 + 2] = 0;
    if (used) used[o] = -1;
    return;
  }
  const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  if (i0 < 0 || i0 >= k.V || i1 < 0 || i1 >= k.V || i2 < 0 || i2 >= k.V) {      // never followed
    tex[o * 3] = 128, tex[o * 3 + 1] = 128, tex[o * 3 + 2] = 128;
    if (used) used[o] = 0;
    return;
  }
  // clamped barycentrics of the texel centre
  const float mf = (float)(k.c - 3);
  float b1 = (float)i / mf, b2 = (float)j / mf;
  float b0 = (1.f - b1) - b2;
  if (b0 < 0.f) {
    const float s = b1 + b2;
    b0 = 0.f, b1 = b1 / s, b2 = b2 / s;
  }
  const float p0x = pos[(size_t)i0 * 3], p0y = pos[(size_t)i0 * 3 + 1], p0z = pos[(size_t)i0 * 3 + 2];
  const float p1x = pos[(size_t)i1 * 3], p1y = pos[(size_t)i1 * 3 + 1], p1z = pos[(size_t)i1 * 3 + 2];
  const float p2x = pos[(size_t)i2 * 3], p2y = pos[(size_t)i2 * 3 + 1], p2z = pos[(size_t)i2 * 3 + 2];
  const float px = (b0 * p0x + b1 * p1x) + b2 * p2x, py = (b0 * p0y + b1 * p1y) + b2 * p2y, pz = (b0 * p0z + b1 * p1z) + b2 * p2z;
  // geometric unit normal (a degenerate face: 0 / 0, every view skips)
  const float ax = p1x - p0x, ay = p1y - p0y, az = p1z - p0z, bx = p2x - p0x, by = p2y - p0y, bz = p2z - p0z;
  float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const float nl = sqrtf((nx * nx + ny * ny) + nz * nz);
  nx = nx / nl, ny = ny / nl, nz = nz / nl;

  float tw[4] = {-1.f, -1.f, -1.f, -1.f}, tr[4] = {0.f, 0.f, 0.f, 0.f}, tg[4] = {0.f, 0.f, 0.f, 0.f}, tb[4] = {0.f, 0.f, 0.f, 0.f};
  int cnt = 0;
  const float Wl = (float)(cam.W - 1), Hl = (float)(cam.H - 1);
  const size_t hw = (size_t)cam.H * cam.W;
  for (int v = 0; v < k.n_views; ++v) {
    const Rigid &m = views.v[v];
    // rigid_apply of view_geom.h, written out: through the helper this loop's arithmetic is packed differently and the bake is 1.5 % slower
    const float qz = ((m.r[6] * px + m.r[7] * py) + m.r[8] * pz) + m.t[2];
    if (!(qz >= 0.001f)) continue;
    const float qx = ((m.r[0] * px + m.r[1] * py) + m.r[2] * pz) + m.t[0];
    const float qy = ((m.r[3] * px + m.r[4] * py) + m.r[5] * pz) + m.t[1];
    const float2 uv = project_ratio(cam, qx, qy, qz);
    const float xf = uv.x, yf = uv.y;
    const float x0 = floorf(xf), y0 = floorf(yf);
    if (!(x0 >= 0.f && x0 < Wl && y0 >= 0.f && y0 < Hl)) continue;      // the 2 x 2 footprint (x0 .. x0 + 1, y0 .. y0 + 1) lies inside
    const float cn = floorf(xf + 0.5f), rn = floorf(yf + 0.5f);          // x0 <= cn <= x0 + 1: inside too
    const size_t base = (size_t)v * hw;
    const size_t pn = base + (size_t)(int)rn * cam.W + (size_t)(int)cn;
    const float d = depth[pn];
    if (!depth_ok(d, k.zfar)) continue;
    if (mask && mask[pn] == 0) continue;
    if (!(fabsf(d - qz) <= k.depth_tol)) continue;
    // the camera centre in the object frame, from the same fp32 matrix
    const float ccx = -((m.r[0] * m.t[0] + m.r[3] * m.t[1]) + m.r[6] * m.t[2]);
    const float ccy = -((m.r[1] * m.t[0] + m.r[4] * m.t[1]) + m.r[7] * m.t[2]);
    const float ccz = -((m.r[2] * m.t[0] + m.r[5] * m.t[1]) + m.r[8] * m.t[2]);
    const float dx = ccx - px, dy = ccy - py, dz = ccz - pz;
    const float dl = sqrtf((dx * dx + dy * dy) + dz * dz);
    const float cosang = ((nx * dx + ny * dy) + nz * dz) / dl;
    if (!(cosang >= k.cos_min)) continue;
    if (cnt < k.top_n) ++cnt;
    const float last = k.top_n == 1 ? tw[0] : k.top_n == 2 ? tw[1] : k.top_n == 3 ? tw[2] : tw[3];      // (no indexed register array)
    if (!(cosang > last)) continue;                 // not among the best top_n: its sample would be dropped
    const float wx = xf - x0, wy = yf - y0;
    const size_t a00 = (base + (size_t)(int)y0 * cam.W + (size_t)(int)x0) * 3, a01 = a00 + (size_t)cam.W * 3;
    float smp[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float t00 = (float)rgb[a00 + ch], t10 = (float)rgb[a00 + 3 + ch], t01 = (float)rgb[a01 + ch], t11 = (float)rgb[a01 + 3 + ch];
      const float ta = t00 + wx * (t10 - t00), tb2 = t01 + wx * (t11 - t01);
      smp[ch] = ta + wy * (tb2 - ta);
    }
    // sorted insertion, cosang descending; `>` keeps the lower view index in front of an equal one
#pragma unroll
    for (int s = 3; s >= 0; --s) {
      if (s < k.top_n) {
        if (s > 0 && cosang > tw[s - 1]) tw[s] = tw[s - 1], tr[s] = tr[s - 1], tg[s] = tg[s - 1], tb[s] = tb[s - 1];
        else if (cosang > tw[s]) tw[s] = cosang, tr[s] = smp[0], tg[s] = smp[1], tb[s] = smp[2];
      }
    }
  }
  float cr, cg, cb;
  if (cnt > 0) {
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s < cnt) sw = sw + tw[s], sr = sr + tw[s] * tr[s], sg = sg + tw[s] * tg[s], sb = sb + tw[s] * tb[s];
    }
    cr = sr / sw, cg = sg / sw, cb = sb / sw;
  } else if (vcol) {
    cr = (b0 * (float)vcol[(size_t)i0 * 3] + b1 * (float)vcol[(size_t)i1 * 3]) + b2 * (float)vcol[(size_t)i2 * 3];
    cg = (b0 * (float)vcol[(size_t)i0 * 3 + 1] + b1 * (float)vcol[(size_t)i1 * 3 + 1]) + b2 * (float)vcol[(size_t)i2 * 3 + 1];
    cb = (b0 * (float)vcol[(size_t)i0 * 3 + 2] + b1 * (float)vcol[(size_t)i1 * 3 + 2]) + b2 * (float)vcol[(size_t)i2 * 3 + 2];
  } else {
    cr = cg = cb = 128.f;
  }
  tex[o * 3] = to_u8(cr), tex[o * 3 + 1] = to_u8(cg), tex[o * 3 + 2] = to_u8(cb);
  if (used) used[o] = (int8_t)cnt;
}

// the three uv entries of every face: texel centres, exact in fp32 for a power-of-two T
__global__ __launch_bounds__(256) void texture_uv_kernel(float *__restrict__ uv, int F, int T, int c, int g) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const int cell = f >> 1, col = cell % g, row = cell / g, m = c - 3;
  const bool B = f & 1;
  const int ci[3] = {B ? c - 1 : 0, B ? c - 1 - m : m, B ? c - 1 : 0};
  const int cj[3] = {B ? c - 1 : 0, B ? c - 1 : 0, B ? c - 1 - m : m};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    uv[((size_t)f * 3 + q) * 2] = ((float)(col * c + ci[q]) + 0.5f) / (float)T;
    uv[((size_t)f * 3 + q) * 2 + 1] = ((float)(row * c + cj[q]) + 0.5f) / (float)T;
  }
}

// the atlas is g x g cells: the smallest g with g * g >= ceil(F / 2)
int texture_grid(int F) {
  const long long cells = ((long long)F + 1) / 2;
  int g = 1;
  while ((long long)g * g < cells) ++g;
  return g;
}

}  // namespace

extern "C" int fp_texture_bake(fp_ctx *ctx, const float *d_pos, int V, const int32_t *d_faces, int F, const uint8_t *d_vertex_colors,
                               const uint8_t *d_rgb, const float *d_depth, const uint8_t *d_mask, int n_views, int H, int W, const double *K,
                               const double *cam_in_ob, const fp_texture_cfg *cfg, uint8_t *d_texture, float *d_uv, int8_t *d_used,
                               void *stream) {
  FP_REQUIRE(ctx && d_pos && d_faces && K && cfg && d_texture && d_uv, "fp_texture_bake: null argument");
  FP_REQUIRE(cfg->struct_size == sizeof(fp_texture_cfg), "fp_texture_bake: fp_texture_cfg.struct_size = %zu (this library knows %zu)",
             cfg->struct_size, sizeof(fp_texture_cfg));
  FP_REQUIRE(V >= 1 && F >= 1 && F <= FP_TEXTURE_MAX_FACES, "fp_texture_bake: V %d, F %d (at least 1; at most %d faces)", V, F, FP_TEXTURE_MAX_FACES);
  FP_REQUIRE(n_views >= 0 && n_views <= FP_TSDF_MAX_VIEWS, "fp_texture_bake: n_views %d (0 .. %d)", n_views, FP_TSDF_MAX_VIEWS);
  FP_REQUIRE(n_views == 0 || (d_rgb && d_depth && cam_in_ob), "fp_texture_bake: null d_rgb, d_depth or cam_in_ob with %d views", n_views);
  FP_REQUIRE(n_views == 0 || (H >= 2 && W >= 2 && (size_t)H * (size_t)W <= ((size_t)1 << 30)), "fp_texture_bake: H %d, W %d (at least 2 each)", H, W);
  const int T = cfg->tex_size;
  FP_REQUIRE(T >= FP_TEXTURE_MIN_SIZE && T <= FP_TEXTURE_MAX_SIZE && (T & (T - 1)) == 0, "fp_texture_bake: tex_size %d (a power of two, %d .. %d)", T,
             FP_TEXTURE_MIN_SIZE, FP_TEXTURE_MAX_SIZE);
  const int g = texture_grid(F), c = T / g;
  if (c < 4) {
    int fit = T;
    while (fit <= FP_TEXTURE_MAX_SIZE && fit / g < 4) fit *= 2;
    if (fit <= FP_TEXTURE_MAX_SIZE)
      fp_set_error("fp_texture_bake: %d faces give cells of %d texels at tex_size %d (at least 4); tex_size %d fits", F, c, T, fit);
    else
      fp_set_error("fp_texture_bake: %d faces give cells of %d texels at tex_size %d (at least 4); no tex_size up to %d fits", F, c, T,
                   FP_TEXTURE_MAX_SIZE);
    return FP_EINVAL;
  }
  FP_REQUIRE(cfg->top_n >= 1 && cfg->top_n <= FP_TEXTURE_MAX_TOP_N, "fp_texture_bake: top_n %d (1 .. %d)", cfg->top_n, FP_TEXTURE_MAX_TOP_N);
  FP_REQUIRE(cfg->depth_tol >= 0.f && cfg->cos_min > 0.f && cfg->cos_min <= 1.f && cfg->zfar > 0.f,
             "fp_texture_bake: depth_tol %g (>= 0), cos_min %g (in (0, 1]), zfar %g (> 0)", (double)cfg->depth_tol, (double)cfg->cos_min, (double)cfg->zfar);
  TexCfg k{T, c, g, F, V, cfg->top_n, n_views, cfg->zfar, cfg->depth_tol, cfg->cos_min};
  FP_TRY(fp_check_camera("fp_texture_bake", K));
  FP_TRY(fp_check_view_matrices("fp_texture_bake", cam_in_ob, n_views));
  hipLaunchKernelGGL(texture_uv_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_uv, F, T, c, g);
  FP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(texture_bake_kernel, dim3((unsigned)(T / TB_X), (unsigned)(T / TB_Y)), dim3(TB_X, TB_Y), 0, (hipStream_t)stream, d_pos, d_faces,
                     d_vertex_colors, d_rgb, d_depth, d_mask, d_texture, d_used, k, pinhole_of(K, H, W), rigids_of(cam_in_ob, n_views, true));
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
