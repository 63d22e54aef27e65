// The pinhole camera and the rigid transform of the depth toolkits and the Gauss-Newton aligners (tsdf.hip, texture.hip, depth_icp.hip,
// pose_icp.hip, segment.hip; the ray distance also metrics.hip and scene.hip), each rule once.  The host part is plain C++ and compiles
// without HIP (tests/test_view_geom_host.py); the device part is __forceinline__ and keeps the order and the parentheses written here,
// which the documented bit-for-bit results rest on - the library is built without contraction.  Not for the network pass: crop.hip,
// raster.hip, register.hip and pose_math.h serve another contract.
//
// Camera.  Pinhole holds fx, fy, cx, cy of K rounded to fp32 (pinhole_of) and the size of the image; zfar and a view count travel beside it.
//   * The ray of a pixel: (col - cx) / fx and (row - cy) / fy (pinhole_ray_x / _y); its point at depth d: (ray_x d, ray_y d, d)
//     (pinhole_point).  Column and row are floats, so that an integer pixel and an already rounded projection take the same way.
//   * A depth counts when d >= 0.001 and d < zfar (depth_ok); a NaN does not.
//   * Two projection rules, which round differently; each is part of its callers' documented results:
//       the ICP rule    u = (fx x) / z + cx, v = (fy y) / z + cy (project_icp), with the pixel cf = floor(u + 0.5), rf = floor(v + 0.5)
//                       and the verdict 0 <= cf <= W - 1, 0 <= rf <= H - 1 decided in float, so that a NaN or a huge value never reaches
//                       a cast.  Callers: depth_pairs_kernel (depth_icp.hip) and pose_align_kernel (pose_icp.hip), through gn_associate.
//       the ratio rule  u = fx (x / z) + cx, v = fy (y / z) + cy (project_ratio).  Callers: tsdf_integrate_kernel (tsdf.hip), which
//                       rounds to the nearest pixel and tests cf < W, and texture_bake_kernel (texture.hip), which tests the 2 x 2
//                       footprint of floor(u), floor(v); the two tests stay with their callers.
//   * The distance along a pixel's ray in double, sqrt(((u - cx) d / fx)^2 + ((v - cy) d / fy)^2 + d^2) with the reciprocals of fx and fy
//     passed in (ray_distance): bop_toolkit's misc.depth_im_to_dist_im_fast at one pixel, in float64, the products and sums in the
//     order written and never contracted.  Callers: the VSD and scene-instance metrics (metrics.hip, scene.hip).
//
// Rigid transform.  Rigid is a rotation, row-major, and a translation in fp32.  rigid_of(m) takes both from a row-major 4 x 4 double
// matrix; rigid_inverse_of(m) is the inverse of a rigid m: the transposed rotation and t[i] = -((m[0][i] m[0][3] + m[1][i] m[1][3]) +
// m[2][i] m[2][3]), computed in double and rounded once.  Row a of R p is (r[3a] x + r[3a+1] y) + r[3a+2] z (mat3_row, rigid_rotate);
// rigid_apply adds t[a] last.
#pragma once
#include "../../include/foundationpose_amd.h"

struct Pinhole {
  float fx, fy, cx, cy;
  int H, W;
};

struct Rigid {
  float r[9], t[3];
};

// one transform per view, as a kernel argument: a view index is uniform in the wave, so a view's twelve numbers arrive as scalar loads
struct Rigids {
  Rigid v[FP_TSDF_MAX_VIEWS];
};

inline Pinhole pinhole_of(const double *K, int H, int W) { return Pinhole{(float)K[0], (float)K[4], (float)K[2], (float)K[5], H, W}; }

inline Rigid rigid_of(const double *m) {
  Rigid o;
  for (int a = 0; a < 3; ++a) {
    for (int i = 0; i < 3; ++i) o.r[a * 3 + i] = (float)m[a * 4 + i];
    o.t[a] = (float)m[a * 4 + 3];
  }
  return o;
}

inline Rigid rigid_inverse_of(const double *m) {
  Rigid o;
  for (int i = 0; i < 3; ++i) {
    for (int a = 0; a < 3; ++a) o.r[i * 3 + a] = (float)m[a * 4 + i];
    o.t[i] = (float)-((m[0 * 4 + i] * m[3] + m[1 * 4 + i] * m[7]) + m[2 * 4 + i] * m[11]);
  }
  return o;
}

// the first n_views of `cam_in_ob` (4 x 4 each) as they are or inverted; the rest zeros
inline Rigids rigids_of(const double *cam_in_ob, int n_views, bool inverse) {
  Rigids o{};
  for (int v = 0; v < n_views; ++v) o.v[v] = inverse ? rigid_inverse_of(cam_in_ob + (size_t)v * 16) : rigid_of(cam_in_ob + (size_t)v * 16);
  return o;
}

#ifdef __HIPCC__
__device__ __forceinline__ float pinhole_ray_x(const Pinhole &c, float col) { return (col - c.cx) / c.fx; }
__device__ __forceinline__ float pinhole_ray_y(const Pinhole &c, float row) { return (row - c.cy) / c.fy; }

__device__ __forceinline__ float3 pinhole_point(const Pinhole &c, float col, float row, float d) {
  return make_float3(pinhole_ray_x(c, col) * d, pinhole_ray_y(c, row) * d, d);
}

__device__ __forceinline__ bool depth_ok(float d, float zfar) { return d >= 0.001f && d < zfar; }

struct PixelHit {
  float u, v, cf, rf;
  bool in;
};

__device__ __forceinline__ PixelHit project_icp(const Pinhole &c, float x, float y, float z) {
  PixelHit h;
  h.u = (c.fx * x) / z + c.cx, h.v = (c.fy * y) / z + c.cy;
  h.cf = floorf(h.u + 0.5f), h.rf = floorf(h.v + 0.5f);
  h.in = h.cf >= 0.f && h.cf <= (float)(c.W - 1) && h.rf >= 0.f && h.rf <= (float)(c.H - 1);
  return h;
}

__device__ __forceinline__ float2 project_ratio(const Pinhole &c, float x, float y, float z) {
  return make_float2(c.fx * (x / z) + c.cx, c.fy * (y / z) + c.cy);
}

__device__ __forceinline__ double ray_distance(double d, double u_cx, double v_cy, double inv_fx, double inv_fy) {
#pragma clang fp contract(off)
  const double X = (u_cx * d) * inv_fx, Y = (v_cy * d) * inv_fy;
  return sqrt((X * X + Y * Y) + d * d);
}

__device__ __forceinline__ float mat3_row(const float (&r)[9], int a, float x, float y, float z) {
  return (r[a * 3] * x + r[a * 3 + 1] * y) + r[a * 3 + 2] * z;
}
__device__ __forceinline__ float rigid_rotate(const Rigid &m, int a, float x, float y, float z) { return mat3_row(m.r, a, x, y, z); }
__device__ __forceinline__ float rigid_apply(const Rigid &m, int a, float x, float y, float z) { return mat3_row(m.r, a, x, y, z) + m.t[a]; }
#endif
