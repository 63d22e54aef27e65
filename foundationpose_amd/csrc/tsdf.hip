// Model-free set-up: posed depth maps fused into a truncated signed distance volume (fp_tsdf_integrate) and a welded, coloured triangle
// mesh extracted from it by marching tetrahedra (fp_tsdf_extract_count / _write).  The arithmetic is stated in
// include/foundationpose_amd.h and restated in numpy by tests/tsdf_oracle.py; this file follows it operation for operation (the library is
// built without contraction).
//
// Both big kernels move memory, they do not compute: one thread per sample point, the linear point index is the thread index, so the six
// volume planes stream coalesced (i is fastest in memory and in the wave); the depth images are gathered through L2 - neighbouring points
// project to neighbouring pixels.  The view matrices are kernel arguments: a view index is uniform in the wave, so they arrive as scalar
// loads.  The views loop inside the thread: a call reads and writes the volume once however many views it gets.  The camera, the
// transforms and the projection (the ratio rule) are those of view_geom.h.
//
// Extraction: flag + count per point (7-bit edge mask, faces of the point's cube) -> exclusive scan of (vertices | faces << 32) as one
// 64-bit word -> vertex write -> face write.  A vertex id is the scanned base of the owning point plus the rank of the edge slot in the
// mask, so neighbouring cubes find the same id without a hash or an atomic.  The scan is scan_exclusive of scan.hip.
#include "common.h"
#include "device_util.h"
#include "gn_sums.h"

#include <math.h>

namespace {

constexpr int TS_THREADS = 256;
constexpr int TAB_BYTES = 6 * 16 * 8;                  // per tetrahedron and sign case: the triangle count, then 6 vertex codes
typedef unsigned long long u64;

struct TsdfGrid {
  int nx, ny, nz, n;
  float ox, oy, oz, vs, trunc;
};

// corner code = dx | dy << 1 | dz << 2.  The far end of edge slot s, and the slot of a corner-code difference.
__device__ __constant__ const int SLOT_CORNER[7] = {1, 2, 4, 3, 5, 6, 7};
constexpr int HOST_SLOT_OF_CODE[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
// tetrahedron p: corners 0, TET_C1[p], TET_C2[p], 7 - the permutations of (x, y, z) in lexicographic order
__device__ __constant__ const int TET_C1[6] = {1, 1, 2, 2, 4, 4};
__device__ __constant__ const int TET_C2[6] = {3, 5, 3, 6, 5, 6};
constexpr int HOST_TET_C1[6] = {1, 1, 2, 2, 4, 4};
constexpr int HOST_TET_C2[6] = {3, 5, 3, 6, 5, 6};

__global__ __launch_bounds__(TS_THREADS) void tsdf_integrate_kernel(TsdfGrid g, float *__restrict__ pT, float *__restrict__ pW,
                                                                    float *__restrict__ pR, float *__restrict__ pG, float *__restrict__ pB,
                                                                    float *__restrict__ pC, const float *__restrict__ depth,
                                                                    const uint8_t *__restrict__ rgb, const uint8_t *__restrict__ mask, Pinhole cam,
                                                                    float zfar, int n_views, Rigids views) {      // object -> camera
  const int idx = blockIdx.x * TS_THREADS + threadIdx.x;
  if (idx >= g.n) return;
  const int i = idx % g.nx, j = (idx / g.nx) % g.ny, k = idx / (g.nx * g.ny);
  const float sx = g.ox + g.vs * (float)i, sy = g.oy + g.vs * (float)j, sz = g.oz + g.vs * (float)k;
  float T = pT[idx], Wt = pW[idx];
  float cr = 0.f, cg = 0.f, cb = 0.f, cw = 0.f;
  if (rgb) cr = pR[idx], cg = pG[idx], cb = pB[idx], cw = pC[idx];
  bool touched = false, touched_c = false;
  const float Wf = (float)cam.W, Hf = (float)cam.H;
  const size_t hw = (size_t)cam.H * cam.W;
  for (int v = 0; v < n_views; ++v) {
    const Rigid &m = views.v[v];
    const float qz = rigid_apply(m, 2, sx, sy, sz);
    if (!(qz >= 0.001f)) continue;
    const float2 uv = project_ratio(cam, rigid_apply(m, 0, sx, sy, sz), rigid_apply(m, 1, sx, sy, sz), qz);
    const float cf = floorf(uv.x + 0.5f), rf = floorf(uv.y + 0.5f);
    if (!(cf >= 0.f && cf < Wf && rf >= 0.f && rf < Hf)) continue;
    const size_t px = (size_t)v * hw + (size_t)(int)rf * cam.W + (size_t)(int)cf;       // 0 <= row < H, 0 <= col < W: inside view v
    const float d = depth[px];
    if (!depth_ok(d, zfar)) continue;
    if (mask && mask[px] == 0) continue;
    const float sdf = d - qz;
    if (sdf < -g.trunc) continue;
    const float tau = fminf(1.f, sdf / g.trunc);
    T = (T * Wt + tau) / (Wt + 1.f);
    Wt = Wt + 1.f;
    touched = true;
    if (rgb && sdf <= g.trunc) {
      const float w1 = cw + 1.f;
      cr = (cr * cw + (float)rgb[px * 3]) / w1;
      cg = (cg * cw + (float)rgb[px * 3 + 1]) / w1;
      cb = (cb * cw + (float)rgb[px * 3 + 2]) / w1;
      cw = w1;
      touched_c = true;
    }
  }
  if (touched) pT[idx] = T, pW[idx] = Wt;
  if (touched_c) pR[idx] = cr, pG[idx] = cg, pB[idx] = cb, pC[idx] = cw;
}

// bits over the 8 corners of the cube at point idx: inside the volume, observed, negative
__device__ __forceinline__ void cube_state(const TsdfGrid &g, const float *__restrict__ pT, const float *__restrict__ pW, float min_w, int idx,
                                           int i, int j, int k, unsigned &inb, unsigned &ob, unsigned &ng) {
  inb = ob = ng = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
    if (i + dx < g.nx && j + dy < g.ny && k + dz < g.nz) {
      const int q = idx + dx + g.nx * (dy + g.ny * dz);
      inb |= 1u << c;
      if (pW[q] >= min_w) ob |= 1u << c;
      if (pT[q] < 0.f) ng |= 1u << c;
    }
  }
}

// the sign case of tetrahedron p (bit q: corner q is negative), or -1 when one of its corners is not observed
__device__ __forceinline__ int tet_case(int p, unsigned ob, unsigned ng) {
  const int c1 = TET_C1[p], c2 = TET_C2[p];
  const unsigned need = 1u | (1u << c1) | (1u << c2) | (1u << 7);
  if ((ob & need) != need) return -1;
  return (int)((ng & 1u) | (((ng >> c1) & 1u) << 1) | (((ng >> c2) & 1u) << 2) | (((ng >> 7) & 1u) << 3));
}

// pass 1: the edge mask of every point and cnt[idx] = vertices | faces << 32; cnt[n] = 0 closes the scan (its scanned value is the total)
__global__ __launch_bounds__(TS_THREADS) void tsdf_count_kernel(TsdfGrid g, const float *__restrict__ pT, const float *__restrict__ pW, float min_w,
                                                                const uint8_t *__restrict__ tab, uint8_t *__restrict__ emask,
                                                                u64 *__restrict__ cnt) {
  __shared__ uint8_t ltab[TAB_BYTES];
  for (int t = threadIdx.x; t < TAB_BYTES; t += TS_THREADS) ltab[t] = tab[t];
  __syncthreads();
  const int idx = blockIdx.x * TS_THREADS + threadIdx.x;
  if (idx > g.n) return;
  if (idx == g.n) {
    cnt[idx] = 0;
    return;
  }
  const int i = idx % g.nx, j = (idx / g.nx) % g.ny, k = idx / (g.nx * g.ny);
  unsigned inb, ob, ng;
  cube_state(g, pT, pW, min_w, idx, i, j, k, inb, ob, ng);
  unsigned em = 0;
  if (ob & 1u) {
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      const int c = SLOT_CORNER[s];
      if (((ob >> c) & 1u) && (((ng >> c) ^ ng) & 1u)) em |= 1u << s;
    }
  }
  unsigned nf = 0;
  if (inb == 0xffu) {
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const int m = tet_case(p, ob, ng);
      if (m > 0) nf += ltab[(p * 16 + m) * 8];
    }
  }
  emask[idx] = (uint8_t)em;
  cnt[idx] = (u64)__popc(em) | ((u64)nf << 32);
}

// ---- pass 3: vertices ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float grad_axis(const float *__restrict__ pT, const float *__restrict__ pW, float min_w, int q, int pos, int n_axis,
                                           int stride, float Tc) {
  const bool hp = pos + 1 < n_axis && pW[q + stride] >= min_w;
  const bool hm = pos > 0 && pW[q - stride] >= min_w;
  if (hp && hm) return (pT[q + stride] - pT[q - stride]) * 0.5f;
  if (hp) return pT[q + stride] - Tc;
  if (hm) return Tc - pT[q - stride];
  return 0.f;
}

__global__ __launch_bounds__(TS_THREADS) void tsdf_vertex_kernel(TsdfGrid g, const float *__restrict__ pT, const float *__restrict__ pW,
                                                                 const float *__restrict__ pR, const float *__restrict__ pG,
                                                                 const float *__restrict__ pB, float min_w, const uint8_t *__restrict__ emask,
                                                                 const u64 *__restrict__ base, float *__restrict__ verts,
                                                                 float *__restrict__ normals, uint8_t *__restrict__ colors) {
  const int idx = blockIdx.x * TS_THREADS + threadIdx.x;
  if (idx >= g.n) return;
  const unsigned em = emask[idx];
  if (em == 0) return;
  const int i = idx % g.nx, j = (idx / g.nx) % g.ny, k = idx / (g.nx * g.ny);
  const int sxy = g.nx * g.ny;
  size_t vid = (size_t)(unsigned)base[idx];
  const float Ta = pT[idx];
  const float ax = g.ox + g.vs * (float)i, ay = g.oy + g.vs * (float)j, az = g.oz + g.vs * (float)k;
  float ga[3] = {0.f, 0.f, 0.f};
  if (normals) {
    ga[0] = grad_axis(pT, pW, min_w, idx, i, g.nx, 1, Ta);
    ga[1] = grad_axis(pT, pW, min_w, idx, j, g.ny, g.nx, Ta);
    ga[2] = grad_axis(pT, pW, min_w, idx, k, g.nz, sxy, Ta);
  }
  for (int s = 0; s < 7; ++s) {
    if (!((em >> s) & 1u)) continue;
    const int c = SLOT_CORNER[s];
    const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
    const int q = idx + dx + g.nx * (dy + g.ny * dz);
    const float Tb = pT[q];
    const float u = Ta / (Ta - Tb);
    const float bx = g.ox + g.vs * (float)(i + dx), by = g.oy + g.vs * (float)(j + dy), bz = g.oz + g.vs * (float)(k + dz);
    verts[vid * 3] = ax + (bx - ax) * u;
    verts[vid * 3 + 1] = ay + (by - ay) * u;
    verts[vid * 3 + 2] = az + (bz - az) * u;
    if (colors) {
      const float *pl[3] = {pR, pG, pB};
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float ca = pl[ch][idx], cb = pl[ch][q];
        const float x = floorf((ca + (cb - ca) * u) + 0.5f);
        colors[vid * 3 + ch] = (uint8_t)fminf(fmaxf(x, 0.f), 255.f);
      }
    }
    if (normals) {
      const float gb[3] = {grad_axis(pT, pW, min_w, q, i + dx, g.nx, 1, Tb), grad_axis(pT, pW, min_w, q, j + dy, g.ny, g.nx, Tb),
                           grad_axis(pT, pW, min_w, q, k + dz, g.nz, sxy, Tb)};
      float nv[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) nv[a] = ga[a] + (gb[a] - ga[a]) * u;
      const float len = sqrtf((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
      if (len > 0.f) nv[0] = nv[0] / len, nv[1] = nv[1] / len, nv[2] = nv[2] / len;
#pragma unroll
      for (int a = 0; a < 3; ++a) normals[vid * 3 + a] = nv[a];
    }
    ++vid;
  }
}

// ---- pass 4: faces -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TS_THREADS) void tsdf_face_kernel(TsdfGrid g, const float *__restrict__ pT, const float *__restrict__ pW, float min_w,
                                                               const uint8_t *__restrict__ tab, const uint8_t *__restrict__ emask,
                                                               const u64 *__restrict__ base, int32_t *__restrict__ faces) {
  __shared__ uint8_t ltab[TAB_BYTES];
  for (int t = threadIdx.x; t < TAB_BYTES; t += TS_THREADS) ltab[t] = tab[t];
  __syncthreads();
  const int idx = blockIdx.x * TS_THREADS + threadIdx.x;
  if (idx >= g.n) return;
  size_t fid = (size_t)(base[idx] >> 32);
  if ((size_t)(base[idx + 1] >> 32) == fid) return;          // base holds n + 1 words
  const int i = idx % g.nx, j = (idx / g.nx) % g.ny, k = idx / (g.nx * g.ny);
  unsigned inb, ob, ng;
  cube_state(g, pT, pW, min_w, idx, i, j, k, inb, ob, ng);      // a cube with faces lies wholly inside: inb = 0xff
  for (int p = 0; p < 6; ++p) {
    const int m = tet_case(p, ob, ng);
    if (m <= 0) continue;
    const uint8_t *e = ltab + (p * 16 + m) * 8;
    const int nt = e[0];
    for (int t = 0; t < nt * 3; ++t) {
      const int code = e[1 + t];
      const int oc = code >> 3, slot = code & 7;                // the owning corner of the edge, and its slot there
      const int q = idx + (oc & 1) + g.nx * (((oc >> 1) & 1) + g.ny * (oc >> 2));
      faces[fid * 3 + t] = (int32_t)((unsigned)base[q] + (unsigned)__popc((unsigned)emask[q] & ((1u << slot) - 1u)));
    }
    fid += nt;
  }
}

// The 16-case table of the 6 tetrahedra, derived from the rule in the header.  Entry (p, m): byte 0 = triangles, bytes 1 .. 6 = their
// vertices as (owning corner code << 3 | slot).  Orientation by geometry: vertices at the edge midpoints, the normal must point from
// the centroid of the negative corners to that of the others.
void build_table(uint8_t *tab) {
  memset(tab, 0, TAB_BYTES);
  for (int p = 0; p < 6; ++p) {
    const int corner[4] = {0, HOST_TET_C1[p], HOST_TET_C2[p], 7};
    double P[4][3];
    for (int q = 0; q < 4; ++q)
      for (int a = 0; a < 3; ++a) P[q][a] = (corner[q] >> a) & 1;
    for (int m = 1; m < 15; ++m) {
      int neg[4], pos[4], nn = 0, np = 0;
      for (int q = 0; q < 4; ++q) {
        if ((m >> q) & 1)
          neg[nn++] = q;
        else
          pos[np++] = q;
      }
      int edges[4][2], ne, tris[2][3], nt;
      if (nn == 2) {
        const int quad[4][2] = {{neg[0], pos[0]}, {neg[0], pos[1]}, {neg[1], pos[1]}, {neg[1], pos[0]}};
        memcpy(edges, quad, sizeof(quad));
        ne = 4, nt = 2;
        const int tt[2][3] = {{0, 1, 2}, {0, 2, 3}};
        memcpy(tris, tt, sizeof(tt));
      } else {
        const int L = nn == 1 ? neg[0] : pos[0];
        const int *others = nn == 1 ? pos : neg;
        for (int e = 0; e < 3; ++e) edges[e][0] = L, edges[e][1] = others[e];
        ne = 3, nt = 1;
        tris[0][0] = 0, tris[0][1] = 1, tris[0][2] = 2;
      }
      double mid[4][3], dir[3];
      for (int e = 0; e < ne; ++e)
        for (int a = 0; a < 3; ++a) mid[e][a] = 0.5 * (P[edges[e][0]][a] + P[edges[e][1]][a]);
      for (int a = 0; a < 3; ++a) {
        double cn = 0, cp = 0;
        for (int q = 0; q < nn; ++q) cn += P[neg[q]][a];
        for (int q = 0; q < np; ++q) cp += P[pos[q]][a];
        dir[a] = cp / np - cn / nn;
      }
      uint8_t *e8 = tab + (p * 16 + m) * 8;
      e8[0] = (uint8_t)nt;
      for (int t = 0; t < nt; ++t) {
        const double *v0 = mid[tris[t][0]], *v1 = mid[tris[t][1]], *v2 = mid[tris[t][2]];
        const double a[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, b[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
        const double nrm[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        if (nrm[0] * dir[0] + nrm[1] * dir[1] + nrm[2] * dir[2] < 0) {
          const int sw = tris[t][1];
          tris[t][1] = tris[t][2], tris[t][2] = sw;
        }
        for (int c = 0; c < 3; ++c) {
          const int *ed = edges[tris[t][c]];
          const int lo = ed[0] < ed[1] ? ed[0] : ed[1], hi = ed[0] < ed[1] ? ed[1] : ed[0];      // corner `lo` is the componentwise smaller one
          e8[1 + t * 3 + c] = (uint8_t)((corner[lo] << 3) | HOST_SLOT_OF_CODE[corner[hi] - corner[lo]]);
        }
      }
    }
  }
}

}  // namespace

struct fp_tsdf {
  int device = 0;
  TsdfGrid g{};
  float *plane[6] = {};
  u64 *base = nullptr;          // n + 1 words: counts, then (after the scan) vertex base | face base << 32
  uint8_t *emask = nullptr;     // n
  u64 *sums = nullptr;          // the block sums of every scan level
  uint8_t *tab = nullptr;
  unsigned long long generation = 1, counted_generation = 0;      // integrate / reset bump `generation`
  float min_weight = 0.f;
  long long n_vertices = 0, n_faces = 0;
  std::vector<void *> allocs;
};

extern "C" int fp_tsdf_create(fp_ctx *ctx, const double *origin, float voxel_size, const int *dims, float trunc, fp_tsdf **out) {
  FP_REQUIRE(ctx && origin && dims && out, "fp_tsdf_create: null argument");
  FP_REQUIRE(dims[0] >= 2 && dims[1] >= 2 && dims[2] >= 2, "fp_tsdf_create: dims %d %d %d (each >= 2)", dims[0], dims[1], dims[2]);
  const long long n = (long long)dims[0] * dims[1] * dims[2];
  FP_REQUIRE((long long)dims[0] * dims[1] <= FP_TSDF_MAX_POINTS && n <= FP_TSDF_MAX_POINTS, "fp_tsdf_create: %d x %d x %d points, at most %d",
             dims[0], dims[1], dims[2], FP_TSDF_MAX_POINTS);
  FP_REQUIRE(voxel_size > 0.f && isfinite(voxel_size) && trunc > 0.f && isfinite(trunc), "fp_tsdf_create: voxel_size %g, trunc %g (both > 0)",
             (double)voxel_size, (double)trunc);
  FP_REQUIRE(isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2]), "fp_tsdf_create: origin is not finite");
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  fp_tsdf *v = new fp_tsdf;
  v->device = ctx->device;
  v->g = TsdfGrid{dims[0], dims[1], dims[2], (int)n, (float)origin[0], (float)origin[1], (float)origin[2], voxel_size, trunc};
  auto take = [&](size_t bytes, void **p) -> bool {
    if (hipMalloc(p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    v->allocs.push_back(*p);
    return true;
  };
  bool ok = true;
  for (int p = 0; ok && p < 6; ++p) ok = take((size_t)n * sizeof(float), (void **)&v->plane[p]);
  ok = ok && take((size_t)(n + 1) * sizeof(u64), (void **)&v->base) && take((size_t)n, (void **)&v->emask) &&
       take(scan_sums_words(n + 1) * sizeof(u64), (void **)&v->sums) && take(TAB_BYTES, (void **)&v->tab);
  if (!ok) {
    fp_set_error("fp_tsdf_create: out of device memory for %d x %d x %d points (33 bytes a point)", dims[0], dims[1], dims[2]);
    fp_tsdf_destroy(v);
    return FP_ENOMEM;
  }
  uint8_t tab[TAB_BYTES];
  build_table(tab);
  hipError_t e = hipMemcpy(v->tab, tab, TAB_BYTES, hipMemcpyHostToDevice);
  for (int p = 0; e == hipSuccess && p < 6; ++p) e = hipMemset(v->plane[p], 0, (size_t)n * sizeof(float));
  if (e != hipSuccess) {
    fp_set_error("fp_tsdf_create: %s", hipGetErrorString(e));
    fp_tsdf_destroy(v);
    return FP_EHIP;
  }
  *out = v;
  return FP_OK;
}

extern "C" int fp_tsdf_destroy(fp_tsdf *vol) {
  if (!vol) return FP_OK;
  for (void *p : vol->allocs) (void)hipFree(p);
  delete vol;
  return FP_OK;
}

extern "C" int fp_tsdf_reset(fp_ctx *ctx, fp_tsdf *vol, void *stream) {
  FP_REQUIRE(ctx && vol, "fp_tsdf_reset: null argument");
  FP_REQUIRE(ctx->device == vol->device, "fp_tsdf_reset: the volume lives on device %d, the context on %d", vol->device, ctx->device);
  ++vol->generation;
  for (int p = 0; p < 6; ++p) FP_CHECK_HIP(hipMemsetAsync(vol->plane[p], 0, (size_t)vol->g.n * sizeof(float), (hipStream_t)stream));
  return FP_OK;
}

extern "C" int fp_tsdf_integrate(fp_ctx *ctx, fp_tsdf *vol, const float *d_depth, const uint8_t *d_rgb, const uint8_t *d_mask, int n_views, int H,
                                 int W, const double *K, const double *cam_in_ob, float zfar, void *stream) {
  FP_REQUIRE(ctx && vol && d_depth && K && cam_in_ob, "fp_tsdf_integrate: null argument");
  FP_REQUIRE(ctx->device == vol->device, "fp_tsdf_integrate: the volume lives on device %d, the context on %d", vol->device, ctx->device);
  FP_REQUIRE(n_views >= 0 && n_views <= FP_TSDF_MAX_VIEWS, "fp_tsdf_integrate: n_views %d (0 .. %d)", n_views, FP_TSDF_MAX_VIEWS);
  FP_REQUIRE(H >= 1 && W >= 1, "fp_tsdf_integrate: H %d, W %d", H, W);
  FP_REQUIRE(zfar > 0.f, "fp_tsdf_integrate: zfar %g (> 0)", (double)zfar);
  FP_TRY(fp_check_camera("fp_tsdf_integrate", K));
  if (n_views == 0) return FP_OK;
  FP_TRY(fp_check_view_matrices("fp_tsdf_integrate", cam_in_ob, n_views));
  ++vol->generation;
  const TsdfGrid &g = vol->g;
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((g.n + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0, (hipStream_t)stream, g,
                     vol->plane[0], vol->plane[1], vol->plane[2], vol->plane[3], vol->plane[4], vol->plane[5], d_depth, d_rgb, d_mask, pinhole_of(K, H, W),
                     zfar, n_views, rigids_of(cam_in_ob, n_views, true));
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

extern "C" int fp_tsdf_extract_count(fp_ctx *ctx, fp_tsdf *vol, float min_weight, int64_t *h_counts, void *stream) {
  FP_REQUIRE(ctx && vol && h_counts, "fp_tsdf_extract_count: null argument");
  FP_REQUIRE(ctx->device == vol->device, "fp_tsdf_extract_count: the volume lives on device %d, the context on %d", vol->device, ctx->device);
  FP_REQUIRE(min_weight > 0.f, "fp_tsdf_extract_count: min_weight %g (> 0)", (double)min_weight);
  const TsdfGrid &g = vol->g;
  hipStream_t s = (hipStream_t)stream;
  vol->counted_generation = 0;
  hipLaunchKernelGGL(tsdf_count_kernel, dim3((unsigned)((g.n + 1 + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0, s, g,
                     (const float *)vol->plane[0], (const float *)vol->plane[1], min_weight, (const uint8_t *)vol->tab, vol->emask, vol->base);
  FP_CHECK_HIP(hipGetLastError());
  FP_TRY(scan_exclusive(vol->base, (long long)g.n + 1, vol->sums, s));
  u64 total = 0;
  FP_CHECK_HIP(hipMemcpyAsync(&total, vol->base + g.n, sizeof(u64), hipMemcpyDeviceToHost, s));
  FP_CHECK_HIP(hipStreamSynchronize(s));
  vol->n_vertices = (long long)(total & 0xffffffffull);
  vol->n_faces = (long long)(total >> 32);
  vol->min_weight = min_weight;
  vol->counted_generation = vol->generation;
  h_counts[0] = vol->n_vertices;
  h_counts[1] = vol->n_faces;
  return FP_OK;
}

extern "C" int fp_tsdf_extract_write(fp_ctx *ctx, fp_tsdf *vol, float *d_vertices, float *d_normals, uint8_t *d_colors, int32_t *d_faces,
                                     int64_t n_vertices, int64_t n_faces, void *stream) {
  FP_REQUIRE(ctx && vol, "fp_tsdf_extract_write: null argument");
  FP_REQUIRE(ctx->device == vol->device, "fp_tsdf_extract_write: the volume lives on device %d, the context on %d", vol->device, ctx->device);
  FP_REQUIRE(vol->counted_generation == vol->generation,
             "fp_tsdf_extract_write: no fp_tsdf_extract_count since the volume was last integrated into or reset");
  FP_REQUIRE(n_vertices == vol->n_vertices && n_faces == vol->n_faces, "fp_tsdf_extract_write: %lld vertices, %lld faces given, %lld and %lld counted",
             (long long)n_vertices, (long long)n_faces, vol->n_vertices, vol->n_faces);
  FP_REQUIRE((d_vertices || n_vertices == 0) && (d_faces || n_faces == 0), "fp_tsdf_extract_write: d_vertices or d_faces is null");
  const TsdfGrid &g = vol->g;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((g.n + TS_THREADS - 1) / TS_THREADS));
  if (n_vertices > 0) {
    hipLaunchKernelGGL(tsdf_vertex_kernel, grid, dim3(TS_THREADS), 0, s, g, (const float *)vol->plane[0], (const float *)vol->plane[1],
                       (const float *)vol->plane[2], (const float *)vol->plane[3], (const float *)vol->plane[4], vol->min_weight,
                       (const uint8_t *)vol->emask, (const u64 *)vol->base, d_vertices, d_normals, d_colors);
    FP_CHECK_HIP(hipGetLastError());
  }
  if (n_faces > 0) {
    hipLaunchKernelGGL(tsdf_face_kernel, grid, dim3(TS_THREADS), 0, s, g, (const float *)vol->plane[0], (const float *)vol->plane[1], vol->min_weight,
                       (const uint8_t *)vol->tab, (const uint8_t *)vol->emask, (const u64 *)vol->base, d_faces);
    FP_CHECK_HIP(hipGetLastError());
  }
  return FP_OK;
}

extern "C" int fp_tsdf_read_plane(fp_ctx *ctx, const fp_tsdf *vol, int plane, float *d_out, void *stream) {
  FP_REQUIRE(ctx && vol && d_out, "fp_tsdf_read_plane: null argument");
  FP_REQUIRE(plane >= 0 && plane < 6, "fp_tsdf_read_plane: plane %d (0 .. 5)", plane);
  FP_CHECK_HIP(hipMemcpyAsync(d_out, vol->plane[plane], (size_t)vol->g.n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return FP_OK;
}

// ---- frame-to-model alignment: one Gauss-Newton linearisation of every view against the volume (fp_tsdf_align) -----------------------
// One of the three aligners of gn_sums.h, which holds what they share: the tile, the three passes, the twist row, the 29 sums in double
// and their way to gn_fold_kernel; the camera and the transforms are those of view_geom.h.  A workgroup owns (view, a tile of GN_TILE
// pixels); the view is uniform in the workgroup, so its matrix arrives as scalar loads.  Pass one reads depth and mask (the reads
// coalesce); pass two finds the cell and gathers tsdf and weight of its 8 corners, all GN_PIX x 16 loads in flight together; pass three
// is the arithmetic.  No atomics: a view's sums depend on nothing but its own pixels.
namespace {

__global__ __launch_bounds__(GN_THREADS) void tsdf_align_kernel(TsdfGrid g, const float *__restrict__ pT, const float *__restrict__ pW,
                                                                const float *__restrict__ depth, const uint8_t *__restrict__ mask, Pinhole cam,
                                                                float zfar, float min_w, int n_tiles, Rigids views,      // camera -> object
                                                                float *__restrict__ rows, double *__restrict__ slab) {
  __shared__ double red[GN_THREADS / 64][GN_TERMS];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % n_tiles, v = blockIdx.x / n_tiles;
  const Rigid &m = views.v[v];
  const long long hw = (long long)cam.H * cam.W;
  const size_t view0 = (size_t)v * (size_t)hw;
  const int sxy = g.nx * g.ny;

  // pass 1: depth and mask
  float d[GN_PIX];
  bool ok[GN_PIX];
  long long pix[GN_PIX];
#pragma unroll
  for (int q = 0; q < GN_PIX; ++q) {
    pix[q] = (long long)tile * GN_TILE + q * GN_THREADS + tid;
    const bool in = pix[q] < hw;                                   // the last tile of a view is ragged
    d[q] = in ? depth[view0 + (size_t)pix[q]] : 0.f;
    ok[q] = depth_ok(d[q], zfar);
    if (mask) ok[q] = ok[q] && (in ? mask[view0 + (size_t)pix[q]] : (uint8_t)0) != 0;
  }

  // pass 2: the point in the object frame, its cell, the 16 gathers
  float x[GN_PIX][3], f[GN_PIX][3], Tc[GN_PIX][8], Wc[GN_PIX][8];
#pragma unroll
  for (int q = 0; q < GN_PIX; ++q) {
    const int row = (int)(pix[q] / cam.W), col = (int)(pix[q] - (long long)row * cam.W);
    const float3 p = pinhole_point(cam, (float)col, (float)row, d[q]);
#pragma unroll
    for (int a = 0; a < 3; ++a) x[q][a] = rigid_apply(m, a, p.x, p.y, p.z);
    const float gx = (x[q][0] - g.ox) / g.vs, gy = (x[q][1] - g.oy) / g.vs, gz = (x[q][2] - g.oz) / g.vs;
    const float fi = floorf(gx), fj = floorf(gy), fk = floorf(gz);
    f[q][0] = gx - fi, f[q][1] = gy - fj, f[q][2] = gz - fk;
    // all eight corners inside: 0 <= i and i + 1 <= n - 1, decided in float so that a NaN or a huge value never reaches the cast
    ok[q] = ok[q] && fi >= 0.f && fi <= (float)(g.nx - 2) && fj >= 0.f && fj <= (float)(g.ny - 2) && fk >= 0.f && fk <= (float)(g.nz - 2);
    const int idx = ok[q] ? (int)fi + g.nx * ((int)fj + g.ny * (int)fk) : 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int p = idx + (c & 1) + g.nx * ((c >> 1) & 1) + sxy * (c >> 2);      // inside the volume whenever ok
      Tc[q][c] = ok[q] ? pT[p] : 0.f;
      Wc[q][c] = ok[q] ? pW[p] : 0.f;
    }
  }

  // pass 3: interpolant, gradient, the row, the sums
  double acc[GN_TERMS];
#pragma unroll
  for (int e = 0; e < GN_TERMS; ++e) acc[e] = 0.0;
  const float gscale = g.trunc / g.vs;
#pragma unroll
  for (int q = 0; q < GN_PIX; ++q) {
    const float *T = Tc[q];
    const float u = f[q][0], w = f[q][1], z = f[q][2];
    bool valid = ok[q];
#pragma unroll
    for (int c = 0; c < 8; ++c) valid = valid && Wc[q][c] >= min_w;
    const float d00 = T[1] - T[0], d10 = T[3] - T[2], d01 = T[5] - T[4], d11 = T[7] - T[6];      // x-differences at (y, z)
    const float a00 = T[0] + d00 * u, a10 = T[2] + d10 * u, a01 = T[4] + d01 * u, a11 = T[6] + d11 * u;
    const float e0 = a10 - a00, e1 = a11 - a01;                                                    // y-differences of the x-lerps at z
    const float b0 = a00 + e0 * w, b1 = a01 + e1 * w;
    const float dz = b1 - b0;
    const float Ti = b0 + dz * z;
    valid = valid && fabsf(Ti) < 1.f;
    const float h0 = d00 + (d10 - d00) * w, h1 = d01 + (d11 - d01) * w;
    const float Gx = (h0 + (h1 - h0) * z) * gscale, Gy = (e0 + (e1 - e0) * z) * gscale, Gz = dz * gscale;
    float J[6], r = Ti * g.trunc;
    gn_twist_row(J, Gx, Gy, Gz, x[q][0], x[q][1], x[q][2]);
    gn_mask(J, r, valid);
    if (rows && pix[q] < hw) gn_store_row((float4 *)(rows + (view0 + (size_t)pix[q]) * 8), J, r, valid);
    gn_accumulate(acc, J, r, valid);
  }
  gn_wave_to_lds(acc, red[tid >> 6], 0);
  __syncthreads();
  gn_lds_to_slab(red, slab + ((size_t)v * n_tiles + tile) * GN_TERMS);
}

}  // namespace

extern "C" int fp_tsdf_align(fp_ctx *ctx, const fp_tsdf *vol, const float *d_depth, const uint8_t *d_mask, int n_views, int H, int W, const double *K,
                             const double *cam_in_ob, float zfar, float min_weight, float *d_rows, double *h_sums, void *stream) {
  // Every check of a value comes before the first look INTO ctx or vol (the device check below): tests/test_tsdf_align_host.py calls this
  // without a GPU, with pointers for ctx and vol that must not be dereferenced.  Keep that order when adding checks.
  FP_REQUIRE(ctx && vol && d_depth && K && cam_in_ob && h_sums, "fp_tsdf_align: null argument");
  FP_REQUIRE(((uintptr_t)d_rows & 15) == 0, "fp_tsdf_align: d_rows is not 16-byte aligned (it is written as float4)");
  FP_REQUIRE(n_views >= 0 && n_views <= FP_TSDF_MAX_VIEWS, "fp_tsdf_align: n_views %d (0 .. %d)", n_views, FP_TSDF_MAX_VIEWS);
  FP_REQUIRE(H >= 1 && W >= 1, "fp_tsdf_align: H %d, W %d", H, W);
  FP_REQUIRE(zfar > 0.f, "fp_tsdf_align: zfar %g (> 0)", (double)zfar);
  FP_REQUIRE(min_weight > 0.f, "fp_tsdf_align: min_weight %g (> 0)", (double)min_weight);
  FP_TRY(fp_check_camera("fp_tsdf_align", K));
  FP_TRY(fp_check_view_matrices("fp_tsdf_align", cam_in_ob, n_views));
  const long long n_tiles = ((long long)H * W + GN_TILE - 1) / GN_TILE;
  FP_REQUIRE(n_tiles * FP_TSDF_MAX_VIEWS <= 0x7fffffff, "fp_tsdf_align: %d x %d pixels are too many for one launch", H, W);
  FP_REQUIRE(ctx->device == vol->device, "fp_tsdf_align: the volume lives on device %d, the context on %d", vol->device, ctx->device);
  if (n_views == 0) return FP_OK;
  hipStream_t s = (hipStream_t)stream;
  const size_t slab_bytes = (size_t)n_views * (size_t)n_tiles * FP_TSDF_ALIGN_TERMS * sizeof(double);
  const size_t sums_bytes = (size_t)n_views * FP_TSDF_ALIGN_TERMS * sizeof(double);
  FP_TRY(fp_arena_ensure(ctx, slab_bytes + sums_bytes + 4096));
  ArenaScope scope(ctx->arena);
  double *slab = (double *)ctx->arena.take(slab_bytes);
  double *sums = (double *)ctx->arena.take(sums_bytes);
  FP_REQUIRE(slab && sums, "fp_tsdf_align: arena exhausted");
  const TsdfGrid &g = vol->g;
  hipLaunchKernelGGL(tsdf_align_kernel, dim3((unsigned)(n_tiles * n_views)), dim3(GN_THREADS), 0, s, g, (const float *)vol->plane[0],
                     (const float *)vol->plane[1], d_depth, d_mask, pinhole_of(K, H, W), zfar, min_weight, (int)n_tiles,
                     rigids_of(cam_in_ob, n_views, false), d_rows, slab);
  FP_CHECK_HIP(hipGetLastError());
  // the slab and the sums go back to the arena when this returns: gn_fold_to_host has synchronised by then
  return gn_fold_to_host<FP_TSDF_ALIGN_TERMS>(slab, n_views, (int)n_tiles, sums, h_sums, s);
}
