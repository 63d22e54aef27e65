// fp_draw_poses: posed 3-D boxes, xyz axes and the silhouettes of an owner map drawn on a uint8 frame (the picture the reference's demo
// ends with: draw_posed_3d_box / draw_xyz_axis, src/Utils.py:667-749, main.py:67-71), as two launches on the caller's stream.
//
// Launch 1 (draw_setup_kernel, one workgroup per 32 objects): a thread per segment - 12 box edges and 3 axes an object - multiplies
// pose @ offset, clips to FP_DRAW_ZNEAR, projects with K and rounds the endpoints, all in float64.  The tiled pass works in fp32, and a
// segment that crosses the near plane has endpoints of 1e4 .. 1e6 pixels, where fp32 holds a distance to no better than a hundredth of
// a pixel.  So the thread also cuts the (rounded) segment, still in float64, to the frame grown by DRAW_GROW pixels - a pixel of the
// frame within thickness / 2 + 1 of the segment has its nearest point inside that box, every other pixel gets coverage 0 either way -
// and leaves a 32-byte record: start point, unit direction, length, half width, colour.  A dropped segment is a record of half width 0.
// Launch 2 (draw_tile_kernel): a workgroup owns a tile of 64 x 16 pixels, a thread 4 neighbouring pixels of a row (three dword loads
// and stores where the rows allow, bytes otherwise).  256 records at a time, each thread tests one record against the tile (the bounding
// box of the capsule grown by thickness / 2 + 1, and the distance of the tile's centre); a ballot per wave and the waves' counts in LDS
// compact the hits into an LDS list IN RECORD ORDER, and the pixels blend the list in that order.  No atomics: a pixel is one thread's.
#include "common.h"
#include <math.h>
#include <algorithm>

namespace {

constexpr int DR_THREADS = 256;
constexpr int DR_TILE_W = 64, DR_TILE_H = 16, DR_PX = 4;      // a thread: DR_PX pixels of a row; 16 threads across, 16 rows
constexpr int DR_SEGS = 15;                                   // segments per object: 12 edges, 3 axes
constexpr int DR_SETUP_OBJS = 32;                             // objects per set-up launch (their parameters travel as kernel arguments)
constexpr double DR_GROW = 64.0;                              // > the largest thickness / 2 + 1 (thickness <= 64)
constexpr double DR_MAX_COORD = 1048576.0;                    // 2^20

struct DrawRec {                 // 32 bytes
  float ax, ay, ux, uy;          // start point, unit direction
  float len, hw;                 // length; thickness / 2 + 0.5, 0 = dropped
  uint32_t rgb, pad;             // colour, channel c in byte c
};

struct DrawObjK {                // what the set-up launch needs of an fp_draw_object
  float bmin[3], bmax[3];
  float off[12];                 // rows 0 .. 2 of the offset (row 3 of a rigid matrix is 0 0 0 1)
  float axis_scale;
  uint32_t box_rgb, axis_rgb[3], fill_rgb;
};

struct SetupArgs {
  const float *poses;            // (n, 4, 4) of this launch's objects
  DrawRec *recs;                 // n * DR_SEGS
  uint2 *objcol;                 // n x (fill, box) colours
  double K[6];
  int n, H, W, flags;
  float box_hw, axis_hw;
  DrawObjK obj[DR_SETUP_OBJS];
};

__device__ __forceinline__ bool clip_edge(double p, double q, double &t0, double &t1) {
  if (p == 0.0) return q >= 0.0;
  const double r = q / p;
  if (p < 0.0) {
    if (r > t1) return false;
    if (r > t0) t0 = r;
  } else {
    if (r < t0) return false;
    if (r < t1) t1 = r;
  }
  return true;
}

__global__ __launch_bounds__(DR_THREADS) void draw_setup_kernel(SetupArgs a) {
  for (int o = threadIdx.x; o < a.n; o += DR_THREADS) a.objcol[o] = make_uint2(a.obj[o].fill_rgb, a.obj[o].box_rgb);
  for (int s = threadIdx.x; s < a.n * DR_SEGS; s += DR_THREADS) {
    const int o = s / DR_SEGS, k = s % DR_SEGS;
    const DrawObjK &ob = a.obj[o];
    DrawRec rec;
    rec.ax = rec.ay = rec.uy = rec.len = rec.hw = 0.f, rec.ux = 1.f, rec.rgb = rec.pad = 0u;
    const bool is_axis = k >= 12;
    bool keep = is_axis ? (a.flags & FP_DRAW_AXES) != 0 : (a.flags & FP_DRAW_BOX) != 0;
    double p0[3], p1[3];
    if (is_axis) {
#pragma unroll
      for (int c = 0; c < 3; ++c) p0[c] = 0.0, p1[c] = c == k - 12 ? (double)ob.axis_scale : 0.0;
      rec.rgb = k == 12 ? ob.axis_rgb[0] : (k == 13 ? ob.axis_rgb[1] : ob.axis_rgb[2]);
    } else {
      const int ax = k >> 2, i = (k >> 1) & 1, j = k & 1;      // the edge runs along ax; i, j pick min / max of the two other axes in order
      const int b1 = ax == 0 ? 1 : 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double lo = (double)fminf(ob.bmin[c], ob.bmax[c]), hi = (double)fmaxf(ob.bmin[c], ob.bmax[c]);
        const bool top = c == b1 ? i != 0 : j != 0;
        p0[c] = c == ax ? lo : (top ? hi : lo), p1[c] = c == ax ? hi : (top ? hi : lo);
      }
      rec.rgb = ob.box_rgb;
    }
    // M = pose @ offset, rows 0 .. 2; camera points
    double c0[3], c1[3];
    const float *P = a.poses + (size_t)o * 16;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      double m[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < 3; ++t) acc += (double)P[r * 4 + t] * (double)ob.off[t * 4 + c];
        m[c] = acc + (c == 3 ? (double)P[r * 4 + 3] : 0.0);
      }
      c0[r] = m[0] * p0[0] + m[1] * p0[1] + m[2] * p0[2] + m[3];
      c1[r] = m[0] * p1[0] + m[1] * p1[1] + m[2] * p1[2] + m[3];
    }
    const double zn = FP_DRAW_ZNEAR;
    if (!(c0[2] >= zn) && !(c1[2] >= zn)) keep = false;        // wholly behind (NaN counts as behind)
    if (keep && (c0[2] < zn || c1[2] < zn)) {
      const bool first = c0[2] < zn;                              // the end that is cut
      const double zi = first ? c1[2] : c0[2], zo = first ? c0[2] : c1[2];
      const double t = (zn - zi) / (zo - zi);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double vi = first ? c1[r] : c0[r], vo = first ? c0[r] : c1[r];
        const double cut = r == 2 ? zn : vi + t * (vo - vi);
        if (first) c0[r] = cut;
        else c1[r] = cut;
      }
    }
    double e[4] = {0, 0, 0, 0};                                   // x0, y0, x1, y1, rounded
    if (keep) {
      e[0] = rint((a.K[0] * c0[0] + a.K[1] * c0[1] + a.K[2] * c0[2]) / c0[2]);
      e[1] = rint((a.K[3] * c0[0] + a.K[4] * c0[1] + a.K[5] * c0[2]) / c0[2]);
      e[2] = rint((a.K[0] * c1[0] + a.K[1] * c1[1] + a.K[2] * c1[2]) / c1[2]);
      e[3] = rint((a.K[3] * c1[0] + a.K[4] * c1[1] + a.K[5] * c1[2]) / c1[2]);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (!(fabs(e[c]) <= DR_MAX_COORD)) keep = false;
    }
    if (keep) {
      // Liang-Barsky against the grown frame
      const double dx = e[2] - e[0], dy = e[3] - e[1];
      const double x_lo = -DR_GROW, x_hi = (double)(a.W - 1) + DR_GROW, y_lo = -DR_GROW, y_hi = (double)(a.H - 1) + DR_GROW;
      double t0 = 0.0, t1 = 1.0;
      keep = clip_edge(-dx, e[0] - x_lo, t0, t1) && clip_edge(dx, x_hi - e[0], t0, t1) && clip_edge(-dy, e[1] - y_lo, t0, t1) &&
             clip_edge(dy, y_hi - e[1], t0, t1);
      if (keep) {
        const double len = sqrt(dx * dx + dy * dy);
        rec.ax = (float)(e[0] + t0 * dx), rec.ay = (float)(e[1] + t0 * dy);
        if (len > 0.0) rec.ux = (float)(dx / len), rec.uy = (float)(dy / len);
        rec.len = (float)((t1 - t0) * len);
        rec.hw = is_axis ? a.axis_hw : a.box_hw;
      }
    }
    a.recs[s] = rec;
  }
}

struct TileArgs {
  const uint8_t *in;
  uint8_t *out;
  const int32_t *owner;
  const DrawRec *recs;
  const uint2 *objcol;
  int H, W, n_rec, n_obj, flags, tiles_x;
  float opacity, fill_alpha;
};

// distance in fp32 of (px, py) to the record's segment
__device__ __forceinline__ float seg_dist(float4 r0, float len, float px, float py) {
  const float rx = px - r0.x, ry = py - r0.y;
  const float along = rx * r0.z + ry * r0.w, perp = rx * r0.w - ry * r0.z;
  const float ex = fmaxf(fmaxf(-along, along - len), 0.f);
  return sqrtf(perp * perp + ex * ex);
}

__device__ __forceinline__ void blend(float (&c)[3], float a, uint32_t rgb) {
  c[0] = c[0] + a * ((float)(rgb & 255u) - c[0]);
  c[1] = c[1] + a * ((float)((rgb >> 8) & 255u) - c[1]);
  c[2] = c[2] + a * ((float)((rgb >> 16) & 255u) - c[2]);
}

__device__ __forceinline__ uint32_t to_byte(float v) { return (uint32_t)(int)rintf(fminf(fmaxf(v, 0.f), 255.f)); }

// VEC: W is a multiple of 4 and the images are 4-byte aligned (the owner map 16-byte): a thread's 12 bytes are three dwords
template <bool VEC>
__global__ __launch_bounds__(DR_THREADS) void draw_tile_kernel(TileArgs a) {
  __shared__ float4 s_r0[DR_THREADS];
  __shared__ float4 s_r1[DR_THREADS];
  __shared__ int s_cnt[DR_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile_x = blockIdx.x % a.tiles_x, tile_y = blockIdx.x / a.tiles_x;
  const int x0 = tile_x * DR_TILE_W + (tid & 15) * DR_PX, y = tile_y * DR_TILE_H + (tid >> 4);
  const bool row_ok = y < a.H;
  const size_t base = ((size_t)y * a.W + x0) * 3;
  bool ok[DR_PX];
#pragma unroll
  for (int j = 0; j < DR_PX; ++j) ok[j] = row_ok && x0 + j < a.W;      // (VEC: all four or none)

  float c[DR_PX][3];
#pragma unroll
  for (int j = 0; j < DR_PX; ++j) c[j][0] = c[j][1] = c[j][2] = 0.f;
  if constexpr (VEC) {
    if (ok[0]) {
      const uint32_t *p = reinterpret_cast<const uint32_t *>(a.in + base);
      const uint32_t w[3] = {p[0], p[1], p[2]};
#pragma unroll
      for (int b = 0; b < 12; ++b) c[b / 3][b % 3] = (float)((w[b >> 2] >> ((b & 3) * 8)) & 255u);
    }
  } else {
#pragma unroll
    for (int j = 0; j < DR_PX; ++j)
      if (ok[j]) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[j][ch] = (float)a.in[base + j * 3 + ch];
      }
  }

  // the silhouettes come first
  if (a.owner && (a.flags & (FP_DRAW_FILL | FP_DRAW_CONTOUR)) && ok[0]) {
    const size_t po = (size_t)y * a.W + x0;
    const unsigned n_obj = (unsigned)a.n_obj;
    int own[DR_PX];
    if constexpr (VEC) {
      const int4 v = *reinterpret_cast<const int4 *>(a.owner + po);
      own[0] = v.x, own[1] = v.y, own[2] = v.z, own[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < DR_PX; ++j) own[j] = ok[j] ? a.owner[po + j] : -1;
    }
    bool any = false;
#pragma unroll
    for (int j = 0; j < DR_PX; ++j) {
      if ((unsigned)own[j] >= n_obj) own[j] = -1;
      any |= own[j] >= 0;
    }
    if (any) {
      int up[DR_PX], dn[DR_PX], lf = 0, rt = 0;
      const bool contour = (a.flags & FP_DRAW_CONTOUR) != 0;
      const bool has_up = y > 0, has_dn = y + 1 < a.H, has_lf = x0 > 0, has_rt = x0 + DR_PX < a.W;
      if (contour) {
#pragma unroll
        for (int j = 0; j < DR_PX; ++j) up[j] = dn[j] = -1;
        if constexpr (VEC) {
          if (has_up) {
            const int4 v = *reinterpret_cast<const int4 *>(a.owner + po - a.W);
            up[0] = v.x, up[1] = v.y, up[2] = v.z, up[3] = v.w;
          }
          if (has_dn) {
            const int4 v = *reinterpret_cast<const int4 *>(a.owner + po + a.W);
            dn[0] = v.x, dn[1] = v.y, dn[2] = v.z, dn[3] = v.w;
          }
        } else {
#pragma unroll
          for (int j = 0; j < DR_PX; ++j) {
            if (has_up && ok[j]) up[j] = a.owner[po - a.W + j];
            if (has_dn && ok[j]) dn[j] = a.owner[po + a.W + j];
          }
        }
        if (has_lf) lf = a.owner[po - 1];
        if (has_rt) rt = a.owner[po + DR_PX];
#pragma unroll
        for (int j = 0; j < DR_PX; ++j) {
          if ((unsigned)up[j] >= n_obj) up[j] = -1;
          if ((unsigned)dn[j] >= n_obj) dn[j] = -1;
        }
        if ((unsigned)lf >= n_obj) lf = -1;
        if ((unsigned)rt >= n_obj) rt = -1;
      }
#pragma unroll
      for (int j = 0; j < DR_PX; ++j) {
        if (own[j] < 0 || !ok[j]) continue;
        const uint2 col = a.objcol[own[j]];
        if (a.flags & FP_DRAW_FILL) blend(c[j], a.fill_alpha, col.x);
        if (contour) {
          const bool e_lf = j > 0 ? own[j - 1] != own[j] : (has_lf && lf != own[j]);
          const bool e_rt = j + 1 < DR_PX ? (x0 + j + 1 < a.W && own[j + 1] != own[j]) : (has_rt && rt != own[j]);
          if (e_lf || e_rt || (has_up && up[j] != own[j]) || (has_dn && dn[j] != own[j])) {
            c[j][0] = (float)(col.y & 255u), c[j][1] = (float)((col.y >> 8) & 255u), c[j][2] = (float)((col.y >> 16) & 255u);
          }
        }
      }
    }
  }

  // the segments, 256 records a round
  const float tcx = (float)(tile_x * DR_TILE_W) + 0.5f * (DR_TILE_W - 1), tcy = (float)(tile_y * DR_TILE_H) + 0.5f * (DR_TILE_H - 1);
  const float t_lo_x = (float)(tile_x * DR_TILE_W), t_hi_x = t_lo_x + (float)(DR_TILE_W - 1);
  const float t_lo_y = (float)(tile_y * DR_TILE_H), t_hi_y = t_lo_y + (float)(DR_TILE_H - 1);
  constexpr float HALF_DIAG = 33.f;      // > sqrt(31.5^2 + 7.5^2)
  const float py = (float)y;
  for (int r_base = 0; r_base < a.n_rec; r_base += DR_THREADS) {
    const int i = r_base + tid;
    float4 r0 = make_float4(0.f, 0.f, 1.f, 0.f), r1 = make_float4(0.f, 0.f, 0.f, 0.f);
    bool hit = false;
    if (i < a.n_rec) {
      const float4 *p = reinterpret_cast<const float4 *>(a.recs + i);
      r0 = p[0], r1 = p[1];
      if (r1.y > 0.f) {
        const float m = r1.y + 0.5f;                                   // thickness / 2 + 1
        const float ex = r0.x + r1.x * r0.z, ey = r0.y + r1.x * r0.w;
        hit = fminf(r0.x, ex) - m <= t_hi_x && fmaxf(r0.x, ex) + m >= t_lo_x && fminf(r0.y, ey) - m <= t_hi_y && fmaxf(r0.y, ey) + m >= t_lo_y &&
              seg_dist(r0, r1.x, tcx, tcy) <= m + HALF_DIAG;
      }
    }
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(hit);
    if (r_base) __syncthreads();                                      // the previous round's list has been read
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < DR_THREADS / 64; ++w) {
      const int n = s_cnt[w];
      off += w < wave ? n : 0, total += n;
    }
    if (hit) {
      off += __popcll(bal & ((1ull << lane) - 1ull));
      s_r0[off] = r0, s_r1[off] = r1;
    }
    __syncthreads();
    if (!ok[0]) continue;
    for (int k = 0; k < total; ++k) {
      const float4 q0 = s_r0[k], q1 = s_r1[k];
      const uint32_t rgb = __float_as_uint(q1.z);
#pragma unroll
      for (int j = 0; j < DR_PX; ++j) {
        const float d = seg_dist(q0, q1.x, (float)(x0 + j), py);
        const float cov = fminf(fmaxf(q1.y - d, 0.f), 1.f) * a.opacity;
        if (cov > 0.f) blend(c[j], cov, rgb);
      }
    }
  }

  if constexpr (VEC) {
    if (ok[0]) {
      uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
      for (int b = 0; b < 12; ++b) w[b >> 2] |= to_byte(c[b / 3][b % 3]) << ((b & 3) * 8);
      uint32_t *p = reinterpret_cast<uint32_t *>(a.out + base);
      p[0] = w[0], p[1] = w[1], p[2] = w[2];
    }
  } else {
#pragma unroll
    for (int j = 0; j < DR_PX; ++j)
      if (ok[j]) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) a.out[base + j * 3 + ch] = (uint8_t)to_byte(c[j][ch]);
      }
  }
}

uint32_t pack_rgb(const uint8_t *c) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }

}  // namespace

extern "C" int fp_draw_poses(fp_ctx *ctx, const fp_draw_args *a, void *stream) {
  FP_REQUIRE(ctx && a, "fp_draw_poses: null ctx or args");
  FP_REQUIRE(a->struct_size == sizeof(fp_draw_args), "fp_draw_poses: fp_draw_args.struct_size = %zu (this library knows %zu)", a->struct_size,
             sizeof(fp_draw_args));
  FP_REQUIRE(a->d_img_in && a->d_img_out && a->K, "fp_draw_poses: null d_img_in, d_img_out or K");
  FP_REQUIRE(a->H >= 1 && a->W >= 1 && (size_t)a->H * (size_t)a->W <= ((size_t)1 << 30), "fp_draw_poses: image %dx%d", a->W, a->H);
  FP_REQUIRE(a->n_obj >= 0 && a->n_obj <= FP_DRAW_MAX_OBJECTS, "fp_draw_poses: n_obj %d outside 0..%d", a->n_obj, FP_DRAW_MAX_OBJECTS);
  FP_REQUIRE(a->n_obj == 0 || (a->objs && a->d_poses), "fp_draw_poses: null objs or d_poses with n_obj %d", a->n_obj);
  const int all_flags = FP_DRAW_BOX | FP_DRAW_AXES | FP_DRAW_FILL | FP_DRAW_CONTOUR;
  FP_REQUIRE((a->flags & ~all_flags) == 0, "fp_draw_poses: unknown bits in flags = %d", a->flags);
  FP_REQUIRE(!(a->flags & (FP_DRAW_FILL | FP_DRAW_CONTOUR)) || a->d_owner, "fp_draw_poses: FP_DRAW_FILL / FP_DRAW_CONTOUR with d_owner null");
  FP_REQUIRE(a->box_thickness > 0.f && a->box_thickness <= 64.f && a->axis_thickness > 0.f && a->axis_thickness <= 64.f,
             "fp_draw_poses: thickness (%g, %g) outside (0, 64]", a->box_thickness, a->axis_thickness);
  FP_REQUIRE(a->opacity >= 0.f && a->opacity <= 1.f && a->fill_alpha >= 0.f && a->fill_alpha <= 1.f,
             "fp_draw_poses: opacity %g / fill_alpha %g outside [0, 1]", a->opacity, a->fill_alpha);
  const size_t px = (size_t)a->H * a->W, img_bytes = px * 3;
  const uintptr_t pin = (uintptr_t)a->d_img_in, pout = (uintptr_t)a->d_img_out;
  FP_REQUIRE(pin == pout || pin + img_bytes <= pout || pout + img_bytes <= pin, "fp_draw_poses: d_img_in and d_img_out overlap in part");
  hipStream_t s = (hipStream_t)stream;
  if (a->n_obj == 0 || a->flags == 0) {
    if (pin != pout) FP_CHECK_HIP(hipMemcpyAsync(a->d_img_out, a->d_img_in, img_bytes, hipMemcpyDeviceToDevice, s));
    return FP_OK;
  }

  const int n_rec = a->n_obj * DR_SEGS;
  const size_t rec_bytes = (size_t)n_rec * sizeof(DrawRec), col_bytes = (size_t)a->n_obj * sizeof(uint2);
  FP_TRY(fp_arena_ensure(ctx, rec_bytes + col_bytes + 4096));
  const size_t mark = ctx->arena.off;
  int rc = FP_OK;
  DrawRec *recs = (DrawRec *)ctx->arena.take(rec_bytes);
  uint2 *objcol = (uint2 *)ctx->arena.take(col_bytes);
  if (!recs || !objcol) {
    fp_set_error("fp_draw_poses: arena exhausted");
    rc = FP_ENOMEM;
  }
  for (int o0 = 0; rc == FP_OK && o0 < a->n_obj; o0 += DR_SETUP_OBJS) {
    SetupArgs sa;
    sa.n = std::min(DR_SETUP_OBJS, a->n_obj - o0);
    sa.poses = a->d_poses + (size_t)o0 * 16, sa.recs = recs + (size_t)o0 * DR_SEGS, sa.objcol = objcol + o0;
    for (int k = 0; k < 6; ++k) sa.K[k] = a->K[k];
    sa.H = a->H, sa.W = a->W, sa.flags = a->flags;
    sa.box_hw = a->box_thickness * 0.5f + 0.5f, sa.axis_hw = a->axis_thickness * 0.5f + 0.5f;
    for (int o = 0; o < sa.n; ++o) {
      const fp_draw_object &ob = a->objs[o0 + o];
      DrawObjK &k = sa.obj[o];
      for (int c = 0; c < 3; ++c) k.bmin[c] = ob.bbox_min[c], k.bmax[c] = ob.bbox_max[c];
      for (int c = 0; c < 12; ++c) k.off[c] = ob.offset[c];
      k.axis_scale = ob.axis_scale;
      k.box_rgb = pack_rgb(ob.box_color), k.fill_rgb = pack_rgb(ob.fill_color);
      for (int c = 0; c < 3; ++c) k.axis_rgb[c] = pack_rgb(ob.axis_color + 3 * c);
    }
    for (int o = sa.n; o < DR_SETUP_OBJS; ++o) memset(&sa.obj[o], 0, sizeof(DrawObjK));
    ProfScope ps(ctx, s, "draw_setup", (double)sa.n * DR_SEGS);
    hipLaunchKernelGGL(draw_setup_kernel, dim3(1), dim3(DR_THREADS), 0, s, sa);
    if (hipGetLastError() != hipSuccess) {
      fp_set_error("fp_draw_poses: the set-up launch failed");
      rc = FP_EHIP;
    }
  }
  if (rc == FP_OK) {
    TileArgs t;
    t.in = a->d_img_in, t.out = a->d_img_out, t.owner = (a->flags & (FP_DRAW_FILL | FP_DRAW_CONTOUR)) ? a->d_owner : nullptr;
    t.recs = recs, t.objcol = objcol;
    t.H = a->H, t.W = a->W, t.n_rec = (a->flags & (FP_DRAW_BOX | FP_DRAW_AXES)) ? n_rec : 0, t.n_obj = a->n_obj, t.flags = a->flags;
    t.tiles_x = (a->W + DR_TILE_W - 1) / DR_TILE_W;
    t.opacity = a->opacity, t.fill_alpha = a->fill_alpha;
    const int tiles_y = (a->H + DR_TILE_H - 1) / DR_TILE_H;
    const bool vec = a->W % 4 == 0 && pin % 4 == 0 && pout % 4 == 0 && (uintptr_t)t.owner % 16 == 0;
    // (profiling: the class' work figure is the BYTES the pass must move: the frame in and out, and the owner map once)
    ProfScope ps(ctx, s, "draw", (double)px * (6.0 + (t.owner ? 4.0 : 0.0)));
    const dim3 grid((unsigned)t.tiles_x * (unsigned)tiles_y);
    if (vec) hipLaunchKernelGGL(draw_tile_kernel<true>, grid, dim3(DR_THREADS), 0, s, t);
    else hipLaunchKernelGGL(draw_tile_kernel<false>, grid, dim3(DR_THREADS), 0, s, t);
    if (hipGetLastError() != hipSuccess) {
      fp_set_error("fp_draw_poses: the tiled launch failed");
      rc = FP_EHIP;
    }
  }
  ctx->arena.off = mark;
  return rc;
}
