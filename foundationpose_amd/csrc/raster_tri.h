// The rasteriser's shared rules (raster.hip), each once: the A record of a vertex, the sign-normalised edge functions of a triangle with the
// barycentrics and z/w they give, the depth key, the perspective-correct weights, the LDS layout of a strip workgroup, the layout of the
// scratch, and the plan (strips, face ranges, launch form).  The host part is plain C++17 and compiles without HIP
// (tests/test_raster_tri_host.py); every function is __host__ __device__, and everything here is called by shipped code:
//   vertex_records            rt_a_describable, rt_a_pack;
//   render_kernel, set-up     rt_strip_lds: the carve of the LDS the plan sized;
//   render_kernel, pass 1     rt_tri_a (A unpack), rt_key;
//   render_kernel, resolve    rt_a_all, RtEdges<int / long long>, rt_persp, rt_persp_hom;
//   host                      rt_render_plan, rt_render_chunk, rt_render_fits, rt_strip_limits, RtScratch.
// The candidate range, the top-left flags and the filing by size class are NOT here: passes 1a / 1b and the two classification forms write
// them out, because through shared functions the render was measurably slower at unchanged register counts (figures at render_kernel).
// oracle/raster_c.c and tests/tools/raster_ref.py restate these rules independently and do not include this file.
//
// Units: a snapped vertex (X, Y) is in 1/16 pixel; pixel (i, j) has its centre at (16 i + 8, 16 j + 8).  Rows are GL rows (bottom-up).
#pragma once
#include <math.h>
#include <stddef.h>

#ifdef __HIPCC__
#define RT_FN __host__ __device__ __forceinline__
#else
#define RT_FN inline
#endif

#define RB_A_NONE 0x7fff7fffu           // A record of a vertex A cannot describe (its second word then carries w, not z/w)
#define RB_SMALL 4                      // candidate pixels of a "small" triangle
#define RB_MEDIUM 32                    // ... of a "medium" one; larger triangles are rasterised by a whole wave
#define RB_SLOW 0x80000000u             // list B entry flag: needs the C records (64-bit edge functions or the homogeneous form)
#define RB_MAXS 255                     // strips per hypothesis

RT_FN unsigned rt_ordered_key(float z) {          // unsigned order = float order
  const unsigned b = __builtin_bit_cast(unsigned, z);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// framebuffer key: nearest wins under an unsigned minimum, ties go to the lower face id
RT_FN unsigned long long rt_key(float zp, int face) { return ((unsigned long long)rt_ordered_key(zp) << 32) | (unsigned)face; }

// ---- A record: word x = X | Y << 16 as two int16 where |X|, |Y| < 16384 (the range of the 32-bit edge functions), else RB_A_NONE ----
RT_FN bool rt_a_describable(int X, int Y) { return X > -16384 && X < 16384 && Y > -16384 && Y < 16384; }
RT_FN unsigned rt_a_pack(int X, int Y) { return ((unsigned)X & 0xffffu) | ((unsigned)Y << 16); }
RT_FN int rt_a_X(unsigned x) { return (short)(x & 0xffffu); }
RT_FN int rt_a_Y(unsigned x) { return (int)x >> 16; }
template <class A> RT_FN bool rt_a_all(const A &a0, const A &a1, const A &a2) { return a0.x != RB_A_NONE && a1.x != RB_A_NONE && a2.x != RB_A_NONE; }

template <class I> struct RtTri {               // int where the A records describe the triangle, long long otherwise (C records)
  I X0, Y0, X1, Y1, X2, Y2;
  RT_FN I area2() const { return (X1 - X0) * (Y2 - Y0) - (X2 - X0) * (Y1 - Y0); }        // signed; 0: covers nothing
};
template <class A> RT_FN RtTri<int> rt_tri_a(const A &a0, const A &a1, const A &a2) {
  return {rt_a_X(a0.x), rt_a_Y(a0.x), rt_a_X(a1.x), rt_a_Y(a1.x), rt_a_X(a2.x), rt_a_Y(a2.x)};
}

// ---- edge functions, sign-normalised so that the inside is positive.  |X|, |Y| < 2^14 -> differences < 2^15, products < 2^30, sums
// < 2^31: the int form holds the same integers as the long long form, so barycentrics and depths are bit-identical. ----
template <class I> struct RtEdges {
  RtTri<I> v;
  I area, dx0, dy0, dx1, dy1, dx2, dy2;
  float fa;
  RT_FN explicit RtEdges(const RtTri<I> &t) : v(t) {
    area = t.area2();
    const I sg = area > 0 ? 1 : -1;
    area *= sg;
    dx0 = sg * (t.X2 - t.X1), dy0 = sg * (t.Y2 - t.Y1);
    dx1 = sg * (t.X0 - t.X2), dy1 = sg * (t.Y0 - t.Y2);
    dx2 = sg * (t.X1 - t.X0), dy2 = sg * (t.Y1 - t.Y0);
    fa = (float)area;
  }
  static RT_FN I centre(int i) { return 16 * (I)i + 8; }                  // of pixel column / row i, in the vertices' units
  RT_FN void at(I Px, I Py, I &e0, I &e1, I &e2) const {                  // the three edge functions at a pixel centre
    e0 = dx0 * (Py - v.Y1) - dy0 * (Px - v.X1);
    e1 = dx1 * (Py - v.Y2) - dy1 * (Px - v.X2);
    e2 = dx2 * (Py - v.Y0) - dy2 * (Px - v.X0);
  }
  // z/w at the pixel (barycentrics b_k = e_k / area, screen-affine interpolation, fixed operation order); false outside the near / far planes
  RT_FN bool depth(I e0, I e1, I e2, float z0, float z1, float z2, float &b0, float &b1, float &b2, float &zp) const {
    b0 = (float)e0 / fa, b1 = (float)e1 / fa, b2 = (float)e2 / fa;
    zp = fmaf(b2, z2, fmaf(b1, z1, b0 * z0));
    return zp >= -1.f && zp <= 1.f;
  }
};

// perspective-correct weights from the screen-space barycentrics and the vertices' w
RT_FN void rt_persp(float b0, float b1, float b2, float w0, float w1, float w2, float &u, float &v, float &wo) {
  const float q0 = b0 / w0, q1 = b1 / w1, q2 = b2 / w2;
  const float qs = (q0 + q1) + q2;
  u = q0 / qs, v = q1 / qs, wo = (1.f - u) - v;
}

// ---- LDS of a strip workgroup: byte offsets of the framebuffer (8 B per pixel), the queue of covered pixels (2 B per pixel), the hypothesis'
// A records (8 B per vertex, lds_verts) and (solo: the one-launch form) the strip's two face lists of 16-bit entries ----
constexpr size_t rt_up16(size_t x) { return (x + 15) & ~(size_t)15; }
struct RtStripLds {
  size_t zbuf, covq, recA, listA, listB, total;
};
constexpr RtStripLds rt_strip_lds(int strip_rows, int Wo, int V, int F, int lds_verts, int solo) {
  const size_t px = (size_t)strip_rows * Wo;
  const size_t covq = px * 8, recA = covq + rt_up16(px * 2), a_end = recA + ((lds_verts || solo) ? rt_up16((size_t)V * 8) : 0);
  const size_t listA = rt_up16(a_end), listB = listA + (size_t)((F + 7) & ~7) * 2;
  return {0, covq, recA, listA, listB, solo ? listB + (size_t)((F + 7) & ~7) * 2 : a_end};
}
constexpr size_t RT_LDS_BUDGET = 148 * 1024;    // dynamic LDS of a workgroup

// ---- scratch of a launch: the vertex records C (16 B), B (32 B) and A (8 B) of every (hypothesis, vertex), the list counters and the two
// face lists of every (hypothesis, strip) (worst case: every face in every strip); byte offsets, each region a multiple of 256 B ----
constexpr size_t rt_up256(size_t x) { return (x + 255) & ~(size_t)255; }
struct RtScratch {
  size_t recC, recB, recA, count, listA, listB, total;
};
constexpr RtScratch rt_scratch(int N, int V, int S, int G, int Fg) {
  const size_t recB = rt_up256((size_t)N * V * 16), recA = recB + rt_up256((size_t)N * V * 32), count = recA + rt_up256((size_t)N * V * 8);
  const size_t listA = count + rt_up256((size_t)N * S * G * 16), list = rt_up256((size_t)N * S * G * Fg * 4);
  return {0, recB, recA, count, listA, listA + list, listA + 2 * list};
}

// ---- the plan ----
struct RenderKnobs {
  int force_s = 0;                      // FP_RENDER_S: strips per hypothesis (experiments)
  int solo_max = 2;                     // FP_RENDER_SOLO: largest batch that takes the one-launch form (0: off)
  size_t scratch_max = (size_t)1 << 30; // FP_RENDER_SCRATCH_MAX: a render whose scratch would exceed it goes out in sub-batches
};
struct RenderPlan {
  int S, strip_rows, lds_verts;         // strips per hypothesis, rows per strip, whether the triangle pass keeps the vertex records in LDS
  int G, Fg;                            // face ranges per hypothesis in the classification, faces per range
  int solo;                             // one or two hypotheses: the whole render in the strip kernel's launch (raster.hip: render_kernel<.., true>)
  size_t a_lds, lds_bytes, solo_lds;    // dynamic LDS of the classification, of the strip kernel, of the strip kernel's one-launch form
  RtScratch sc;
  size_t total;                         // = sc.total
};
// the strip limits: the strip count fits the classification's counters, a strip pixel's index fits the 16-bit queue
constexpr bool rt_strip_limits(const RenderPlan &p, int Wo) { return p.S <= RB_MAXS && p.strip_rows * Wo <= 65535; }
constexpr bool rt_shape_ok(int F, int Ho, int Wo) { return Ho >= 1 && Wo >= 1 && (size_t)Wo * 10 <= 64 * 1024 && F < (1 << 30); }

inline RenderPlan rt_render_plan(int N, int V, int F, int Ho, int Wo, int num_cu, const RenderKnobs &k) {
  RenderPlan p;
  p.lds_verts = (size_t)V * 8 <= 64 * 1024 ? 1 : 0;                          // the hypothesis' A records beside the strip
  p.a_lds = p.lds_verts ? rt_up16((size_t)V * 8) : 0;
  int rows_max = (int)((RT_LDS_BUDGET - p.a_lds - 16) / ((size_t)Wo * 10));  // 8 B framebuffer + 2 B covered-pixel queue per pixel
  if (p.lds_verts && (rows_max < 1 || (Ho + rows_max - 1) / rows_max > RB_MAXS)) {
    // a large full frame (1920x1200 beside 8k vertices) would need more than RB_MAXS strips: the A records stay in global memory
    p.lds_verts = 0;
    p.a_lds = 0;
    rows_max = (int)((RT_LDS_BUDGET - 16) / ((size_t)Wo * 10));
  }
  if (rows_max > Ho) rows_max = Ho;
  if (rows_max < 1) rows_max = 1;
  int S = (Ho + rows_max - 1) / rows_max;
  // 27-row strips of a 160-row crop; thinner ones while the launch is under ~0.8 workgroups per CU (a workgroup's resolve pass shrinks
  // with its strip; twice the strips are then still under two rounds)
  while (S < 4 && Ho / (S * 2) >= 8) S *= 2;
  // (measured, 160x160 crops of the 16k-face mesh, strips 6 -> 12: 24 hypotheses 58 -> 49 us, 32: 72 -> 62, 40: 72 -> 78, 63: 92 -> 100)
  while ((size_t)N * S * 5 <= (size_t)num_cu * 4 && S < 16 && Ho / (S * 2) >= 8) S *= 2;
  if (k.force_s > 0 && (Ho + k.force_s - 1) / k.force_s <= rows_max) S = k.force_s;
  p.strip_rows = (Ho + S - 1) / S;
  p.S = (Ho + p.strip_rows - 1) / p.strip_rows;
  p.lds_bytes = rt_strip_lds(p.strip_rows, Wo, V, F, p.lds_verts, 0).total;
  p.G = 1;                                        // face ranges per hypothesis in the classification: more while it would fill < 1/4 of the chip
  while ((size_t)N * p.G * 4 <= (size_t)num_cu && p.G < 8 && F / (p.G * 2) >= 1024) p.G *= 2;
  p.Fg = (F + p.G - 1) / p.G;
  p.sc = rt_scratch(N, V, p.S, p.G, p.Fg);
  p.total = p.sc.total;
  // one or two hypotheses (a tracking frame): vertex pass, classification and triangle pass as ONE launch (render_kernel<.., true>) when a
  // strip, the A records and the strip's two 16-bit face lists fit a workgroup's LDS
  p.solo_lds = rt_strip_lds(p.strip_rows, Wo, V, F, 1, 1).total;
  p.solo = (N <= k.solo_max && p.lds_verts && F <= 65535 && p.solo_lds <= RT_LDS_BUDGET) ? 1 : 0;
  return p;
}
// A render of N hypotheses goes out in sub-batches of this many when the scratch of all N at once would exceed the cap
inline int rt_render_chunk(int N, int V, int F, int Ho, int Wo, int num_cu, const RenderKnobs &k) {
  int chunk = N < 1 ? 1 : N;
  while (chunk > 1 && rt_render_plan(chunk, V, F, Ho, Wo, num_cu, k).total > k.scratch_max) chunk = (chunk + 1) / 2;
  return chunk;
}
inline bool rt_render_fits(int N, int V, int F, int Ho, int Wo, int num_cu, const RenderKnobs &k) {
  return rt_shape_ok(F, Ho, Wo) && rt_strip_limits(rt_render_plan(rt_render_chunk(N, V, F, Ho, Wo, num_cu, k), V, F, Ho, Wo, num_cu, k), Wo);
}

#ifdef __HIPCC__
// the homogeneous form's weights l_k / sum (triangles that straddle the camera plane)
__device__ __forceinline__ void rt_persp_hom(const float *l, float &u, float &v, float &wo) {
  const float ls = __fadd_rn(__fadd_rn(l[0], l[1]), l[2]);
  u = __fdiv_rn(l[0], ls), v = __fdiv_rn(l[1], ls), wo = (1.f - u) - v;
}
#endif
