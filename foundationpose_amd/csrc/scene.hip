// fp_scene_instances (api.hip): from the depth layers of n instances, one render each on the padded canvas, to BOP's annotations in one
// pass: mask, mask_visib (visibility rule 'bop19', the expression of vsd_count_kernel in metrics.hip), the z-buffer composite (owner,
// depth) and per-instance pixel counts and boxes (bop_toolkit calc_gt_masks.py / calc_gt_info.py / visibility.estimate_visib_mask_gt).
//
// A thread owns PX neighbouring canvas pixels of one row (PX = 4 when the frame width and pad_x are multiples of 4: 16-byte layer loads,
// 4-byte mask stores; else 1), lanes along x.  Loop A runs over the chunk's layers with the smallest positive depth and its instance in
// registers; loop B runs over the same layers again - a workgroup's part of a layer is 4 KB, so the second read comes out of the caches -
// and forms the masks against the occluder distance, which is complete by then.  The distance dist(d) at a pixel does not decrease with d
// (every product, sum and the square root round monotonically), so the smallest positive distance is dist(smallest positive depth): the
// running minimum across chunks is the float32 composite depth itself.
// Counts and boxes: a wave that holds no pixel of the instance (nearly all of them) leaves after one ballot; the others reduce with
// shuffles, add into the workgroup's LDS row with LDS atomics, and the workgroup issues one global integer atomic (add / min / max) per
// field that it changed.  Integer sums, minima and maxima do not depend on their order: the results are deterministic.
#include "common.h"
#include "device_util.h"
#include "view_geom.h"
#include <algorithm>
#include <climits>

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_TILE = 32;                       // instances whose LDS rows a workgroup holds at a time
constexpr int SC_COLS = FP_SCENE_INFO_COLS;
constexpr int SC_MIN = 1, SC_MASKS = 2;          // the loops a launch runs

struct SceneArgs {
  const float *layers;                            // (n, Hc, Wc) depth renders of the chunk's instances
  const float *dt;                                // (H, W) depth_test or null
  int n, i0;                                      // instances of the chunk; index of its first one in the call
  int H, W, Hc, Wc, pad_x, pad_y;
  int loops, first, occ_depth, occ_inst;
  double cx, cy, inv_fx, inv_fy, delta;           // of the canvas: cx' = cx + pad_x, cy' = cy + pad_y
  float *dmin;                                    // (H, W) running smallest positive depth (loop A: read unless `first`, written), or null
  int32_t *owner;                                 // (H, W) its instance, or null
  uint8_t *mask, *mask_visib;                     // (n_inst, H, W) of the whole call (indexed by i0 + i), or null
  int *acc;                                       // (n_inst, SC_COLS) accumulators of the whole call, or null
};

__device__ __forceinline__ bool is_min_col(int c) { return c == FP_SCENE_INFO_BBOX_OBJ || c == FP_SCENE_INFO_BBOX_OBJ + 1 ||
                                                           c == FP_SCENE_INFO_BBOX_VISIB || c == FP_SCENE_INFO_BBOX_VISIB + 1; }
__device__ __forceinline__ int col_identity(int c) { return c < FP_SCENE_INFO_BBOX_OBJ ? 0 : (is_min_col(c) ? INT_MAX : INT_MIN); }

template <int PX>
__device__ __forceinline__ void load_px(const float *p, bool ok, float (&d)[PX]) {
  if constexpr (PX == 4) {
    const float4 v = ok ? *reinterpret_cast<const float4 *>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
    d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
  } else {
    d[0] = ok ? p[0] : 0.f;
  }
}

template <int PX>
__device__ __forceinline__ void store_mask(uint8_t *p, const bool (&b)[PX]) {
  if constexpr (PX == 4) {
    *reinterpret_cast<uint32_t *>(p) = (b[0] ? 0xffu : 0u) | (b[1] ? 0xff00u : 0u) | (b[2] ? 0xff0000u : 0u) | (b[3] ? 0xff000000u : 0u);
  } else {
    p[0] = b[0] ? 255 : 0;
  }
}

// grid (groups of SC_THREADS * PX pixels along x, canvas rows)
template <int PX>
__global__ __launch_bounds__(SC_THREADS) void scene_instances_kernel(SceneArgs a) {
  __shared__ int red[SC_TILE][SC_COLS];
  const int xc = (blockIdx.x * SC_THREADS + threadIdx.x) * PX, yc = blockIdx.y;      // canvas pixel of the thread's first pixel
  const bool on_canvas = xc < a.Wc;                                                  // (Wc is a multiple of PX)
  const int u0 = xc - a.pad_x, v = yc - a.pad_y;                                     // image coordinates
  // the PX pixels lie inside the frame together or not at all (PX = 4: W and pad_x are multiples of 4)
  const bool in_frame = on_canvas && v >= 0 && v < a.H && u0 >= 0 && u0 < a.W;
  const size_t pc = (size_t)yc * a.Wc + xc, pxc = (size_t)a.Hc * a.Wc;
  const size_t pf = in_frame ? (size_t)v * a.W + u0 : 0, pxf = (size_t)a.H * a.W;

  float dmin[PX];
  int own[PX];
#pragma unroll
  for (int j = 0; j < PX; ++j) dmin[j] = 0.f, own[j] = -1;

  if (a.loops & SC_MIN) {
    if (!a.first && a.dmin && in_frame) {
      load_px<PX>(a.dmin + pf, true, dmin);
      if (a.owner) {
#pragma unroll
        for (int j = 0; j < PX; ++j) own[j] = a.owner[pf + j];
      }
    }
    if (in_frame) {
      constexpr int UN = 4;                        // layers whose loads are in flight together
      for (int i = 0; i < a.n; i += UN) {
        float d[UN][PX];
#pragma unroll
        for (int k = 0; k < UN; ++k) load_px<PX>(a.layers + (size_t)(i + k < a.n ? i + k : i) * pxc + pc, i + k < a.n, d[k]);
#pragma unroll
        for (int k = 0; k < UN; ++k)
#pragma unroll
          for (int j = 0; j < PX; ++j)
            if (d[k][j] > 0.f && (dmin[j] == 0.f || d[k][j] < dmin[j])) dmin[j] = d[k][j], own[j] = a.i0 + i + k;
      }
      if (a.dmin) {
        if constexpr (PX == 4) *reinterpret_cast<float4 *>(a.dmin + pf) = make_float4(dmin[0], dmin[1], dmin[2], dmin[3]);
        else a.dmin[pf] = dmin[0];
      }
      if (a.owner) {
        if constexpr (PX == 4) *reinterpret_cast<int4 *>(a.owner + pf) = make_int4(own[0], own[1], own[2], own[3]);
        else a.owner[pf] = own[0];
      }
    }
  } else if (a.occ_inst && a.dmin && in_frame) {   // (no dmin: a call that asks for `mask` alone - nothing looks at the occluder)
    load_px<PX>(a.dmin + pf, true, dmin);          // complete: the first pass over the chunks has run
  }
  if (!(a.loops & SC_MASKS)) return;

  // the occluder of the thread's pixels: float32 of its distance, and whether there is none
  float focc[PX];
  bool no_occ[PX], valid[PX];
  double u_cx[PX];
  const double v_cy = (double)yc - a.cy;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    u_cx[j] = (double)(xc + j) - a.cx;
    focc[j] = 0.f, no_occ[j] = true, valid[j] = false;
  }
  if (in_frame) {
    float t[PX];
    load_px<PX>(a.dt ? a.dt + pf : nullptr, a.dt != nullptr, t);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      valid[j] = t[j] > 0.f;
      double Docc = a.occ_depth ? ray_distance((double)t[j], u_cx[j], v_cy, a.inv_fx, a.inv_fy) : 0.0;
      if (a.occ_inst && dmin[j] > 0.f) {
        const double Dmin = ray_distance((double)dmin[j], u_cx[j], v_cy, a.inv_fx, a.inv_fy);
        if (Dmin > 0.0 && (!(Docc > 0.0) || Dmin < Docc)) Docc = Dmin;
      }
      focc[j] = (float)Docc, no_occ[j] = Docc == 0.0;
    }
  }

  const int lane = threadIdx.x & 63;
  for (int t0 = 0; t0 < a.n; t0 += SC_TILE) {
    const int nt = min(SC_TILE, a.n - t0);
    if (a.acc) {
      __syncthreads();                             // the previous tile's rows have been flushed
      for (int k = threadIdx.x; k < nt * SC_COLS; k += SC_THREADS) red[k / SC_COLS][k % SC_COLS] = col_identity(k % SC_COLS);
      __syncthreads();
    }
    for (int ti = 0; ti < nt; ++ti) {
      const int i = t0 + ti;
      float d[PX];
      load_px<PX>(a.layers + (size_t)i * pxc + pc, on_canvas, d);
      bool m[PX], vis[PX];
      bool any = false;
#pragma unroll
      for (int j = 0; j < PX; ++j) m[j] = d[j] > 0.f, vis[j] = false, any |= m[j];
      const bool wave_any = __builtin_amdgcn_ballot_w64(any) != 0;
      if (wave_any && in_frame) {
#pragma unroll
        for (int j = 0; j < PX; ++j)
          if (m[j]) {
            const double Dm = ray_distance((double)d[j], u_cx[j], v_cy, a.inv_fx, a.inv_fy);
            vis[j] = Dm > 0.0 && ((double)((float)Dm - focc[j]) <= a.delta || no_occ[j]);
          }
      }
      if (in_frame) {
        const size_t o = (size_t)(a.i0 + i) * pxf + pf;
        if (a.mask) store_mask<PX>(a.mask + o, m);
        if (a.mask_visib) store_mask<PX>(a.mask_visib + o, vis);
      }
      if (!a.acc || !wave_any) continue;           // (uniform over the wave)
      int c_all = 0, c_valid = 0, c_vis = 0, c_in = 0, x0 = INT_MAX, x1 = INT_MIN, vx0 = INT_MAX, vx1 = INT_MIN;
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        c_all += m[j], c_in += m[j] && in_frame, c_valid += m[j] && valid[j], c_vis += vis[j];
        if (m[j]) x0 = min(x0, u0 + j), x1 = max(x1, u0 + j);
        if (vis[j]) vx0 = min(vx0, u0 + j), vx1 = max(vx1, u0 + j);
      }
      const bool any_vis = __builtin_amdgcn_ballot_w64(c_vis != 0) != 0;
      // (every lane of a wave is in one canvas row)
      c_all = wave_sum(c_all), c_in = wave_sum(c_in), c_valid = wave_sum(c_valid);
      x0 = wave_min(x0), x1 = wave_max(x1);
      if (any_vis) c_vis = wave_sum(c_vis), vx0 = wave_min(vx0), vx1 = wave_max(vx1);
      if (lane == 0) {
        int *r = red[ti];
        atomicAdd(&r[FP_SCENE_INFO_PX_COUNT_ALL], c_all);
        if (c_valid) atomicAdd(&r[FP_SCENE_INFO_PX_COUNT_VALID], c_valid);
        if (c_in) atomicAdd(&r[FP_SCENE_INFO_PX_COUNT_IN_FRAME], c_in);
        atomicMin(&r[FP_SCENE_INFO_BBOX_OBJ + 0], x0), atomicMin(&r[FP_SCENE_INFO_BBOX_OBJ + 1], v);
        atomicMax(&r[FP_SCENE_INFO_BBOX_OBJ + 2], x1), atomicMax(&r[FP_SCENE_INFO_BBOX_OBJ + 3], v);
        if (any_vis) {
          atomicAdd(&r[FP_SCENE_INFO_PX_COUNT_VISIB], c_vis);
          atomicMin(&r[FP_SCENE_INFO_BBOX_VISIB + 0], vx0), atomicMin(&r[FP_SCENE_INFO_BBOX_VISIB + 1], v);
          atomicMax(&r[FP_SCENE_INFO_BBOX_VISIB + 2], vx1), atomicMax(&r[FP_SCENE_INFO_BBOX_VISIB + 3], v);
        }
      }
    }
    if (a.acc) {
      __syncthreads();
      for (int k = threadIdx.x; k < nt * SC_COLS; k += SC_THREADS) {
        const int c = k % SC_COLS, val = red[k / SC_COLS][c];
        if (val == col_identity(c)) continue;
        int *g = a.acc + (size_t)(a.i0 + t0 + k / SC_COLS) * SC_COLS + c;
        if (c < FP_SCENE_INFO_BBOX_OBJ) atomicAdd(g, val);
        else if (is_min_col(c)) atomicMin(g, val);
        else atomicMax(g, val);
      }
    }
  }
}

__global__ __launch_bounds__(256) void scene_info_init_kernel(int *acc, int n) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < n * SC_COLS) acc[k] = col_identity(k % SC_COLS);
}

// an empty set: count 0 and a box of four -1
__global__ __launch_bounds__(256) void scene_info_finish_kernel(const int *__restrict__ acc, int n, int32_t *info) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n * SC_COLS) return;
  const int i = k / SC_COLS, c = k % SC_COLS;
  int val = acc[k];
  if (c >= FP_SCENE_INFO_BBOX_VISIB) {
    if (acc[i * SC_COLS + FP_SCENE_INFO_PX_COUNT_VISIB] == 0) val = -1;
  } else if (c >= FP_SCENE_INFO_BBOX_OBJ) {
    if (acc[i * SC_COLS + FP_SCENE_INFO_PX_COUNT_ALL] == 0) val = -1;
  }
  info[k] = val;
}

}  // namespace

int launch_scene_info_init(int *acc, int n_inst, hipStream_t s) {
  if (n_inst == 0) return FP_OK;
  hipLaunchKernelGGL(scene_info_init_kernel, dim3((n_inst * SC_COLS + 255) / 256), dim3(256), 0, s, acc, n_inst);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

int launch_scene_info_finish(const int *acc, int n_inst, int32_t *info, hipStream_t s) {
  if (n_inst == 0) return FP_OK;
  hipLaunchKernelGGL(scene_info_finish_kernel, dim3((n_inst * SC_COLS + 255) / 256), dim3(256), 0, s, acc, n_inst, info);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

int launch_scene_instances(fp_ctx *ctx, const SceneLaunch &l, hipStream_t s) {
  if (l.n == 0) return FP_OK;
  SceneArgs a;
  a.layers = l.layers, a.dt = l.dt, a.n = l.n, a.i0 = l.i0;
  a.H = l.H, a.W = l.W, a.pad_x = l.pad_x, a.pad_y = l.pad_y, a.Hc = l.H + 2 * l.pad_y, a.Wc = l.W + 2 * l.pad_x;
  a.loops = (l.do_min ? SC_MIN : 0) | (l.do_masks ? SC_MASKS : 0), a.first = l.first;
  a.occ_depth = l.occ_depth, a.occ_inst = l.occ_inst;
  a.cx = l.K[2] + (double)l.pad_x, a.cy = l.K[5] + (double)l.pad_y, a.inv_fx = 1.0 / l.K[0], a.inv_fy = 1.0 / l.K[4], a.delta = l.delta;
  a.dmin = l.dmin, a.owner = l.owner, a.mask = l.mask, a.mask_visib = l.mask_visib, a.acc = l.acc;
  // 16-byte loads and stores need 16-byte addresses (a null pointer counts as aligned)
  const uintptr_t addr = (uintptr_t)l.layers | (uintptr_t)l.dt | (uintptr_t)l.dmin | (uintptr_t)l.owner | (uintptr_t)l.mask | (uintptr_t)l.mask_visib;
  const bool vec = l.W % 4 == 0 && l.pad_x % 4 == 0 && addr % 16 == 0;
  const int px = vec ? 4 : 1;
  const dim3 grid((a.Wc / px + SC_THREADS - 1) / SC_THREADS, a.Hc);
  FP_REQUIRE(grid.y <= 65535u, "fp_scene_instances: canvas of %d rows", a.Hc);
  // (profiling: the class' work figure is the BYTES the pass must move: every layer once, the depth image, and what it writes)
  const double pxc = (double)a.Hc * a.Wc, pxf = (double)a.H * a.W;
  double bytes = pxc * 4.0 * l.n;
  if (l.do_masks) bytes += (l.dt ? pxf * 4.0 : 0.0) + pxf * l.n * ((l.mask ? 1.0 : 0.0) + (l.mask_visib ? 1.0 : 0.0));
  if (l.do_min) bytes += pxf * ((l.dmin ? 4.0 : 0.0) + (l.owner ? 4.0 : 0.0)) * (l.first ? 1.0 : 2.0);
  ProfScope ps(ctx, s, "scene_pass", bytes);
  if (vec) hipLaunchKernelGGL(scene_instances_kernel<4>, grid, dim3(SC_THREADS), 0, s, a);
  else hipLaunchKernelGGL(scene_instances_kernel<1>, grid, dim3(SC_THREADS), 0, s, a);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
