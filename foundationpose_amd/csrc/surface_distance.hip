// Distance between surfaces: the exact distance from points to a triangle mesh (fp_point_mesh_distance), its statistics
// (fp_distance_stats), a deterministic area-weighted surface sampler (fp_mesh_sample_surface) and the distances of a sample set under many
// rigid transforms with their statistics per transform (fp_symmetry_residuals: the same kernel, the queries formed in registers).  The rules are stated in
// include/foundationpose_amd.h and restated in float64 numpy in tests/surface_distance_oracle.py.  The nearest thing in the reference is
// the cKDTree query of adds_err (src/Utils.py:242-253): point to VERTEX, so it depends on the tessellation; this is point to triangle.
//
// Brute force.  A workgroup owns (a tile of SD_TILE queries, a slice of the faces); each lane keeps SD_Q queries in registers.  The faces
// are staged through LDS in chunks of SD_CHUNK precomputed records of five float4 (a, ab, ac, the dot products, their guarded inverses,
// the unit normal, a flag; formed in double, rounded once): the per-face work is done once per chunk and the records are read back as broadcasts (every lane reads the same address).  A
// lane keeps the smallest fp32 squared distance and its face per query (strictly smaller replaces, faces ascend: ties go to the lowest
// index) and folds the pair into the query's 64-bit key (d2 bits << 32 | face) with one integer atomicMin: non-negative fp32 bit
// patterns order as unsigned integers, so the key keeps the tie rule whatever the face slices are.  surfdist_finish_kernel unpacks the
// keys and, for `closest`, evaluates the winning pair again with the same function.  No float atomics; 20 KiB of static LDS.
//
// fp_points_mesh_align / fp_points_mesh_polish (rigid alignment of a point set to the mesh) sit on the same search: the queries are
// formed from (pose, point) with a transform stride of 16 floats, and mesh_align_kernel - one of the aligners of gn_sums.h - unpacks the
// keys as surfdist_finish_kernel does, evaluates the winning pair again with pair_d2 and turns (closest point, face normal) into the
// rows and the 29 sums of a Gauss-Newton step; fp_pose_gn_step (pose_icp.hip) takes the step.
#include "common.h"
#include "device_util.h"
#include "gn_sums.h"

#include <math.h>

static_assert(FP_POSE_ALIGN_TERMS == GN_TERMS, "the sums of fp_points_mesh_align are those fp_pose_gn_step reads");
static_assert(sizeof(fp_pose_state) % 8 == 0, "the records of d_state are reset as 64-bit words");

namespace {

typedef unsigned long long u64;

constexpr int SD_THREADS = 256;
constexpr int SD_Q = FP_SURFDIST_TILE / SD_THREADS;      // queries per lane
constexpr int SD_TILE = FP_SURFDIST_TILE;                // queries per workgroup
constexpr int SD_CHUNK = FP_SURFDIST_CHUNK;              // face records per LDS chunk (5 float4 each: 20 KiB)
constexpr int SD_REC = 5;
constexpr int SD_MIN_GROUPS = 1024;                      // the face slices bring the grid to about this many workgroups (256 CUs x 4)
constexpr float SD_FLAG_TRIANGLE = 0.f, SD_FLAG_DEGENERATE = 1.f;
static_assert(SD_TILE % SD_THREADS == 0 && SD_CHUNK % SD_THREADS == 0, "tile and chunk are multiples of the workgroup");

struct FaceRec {
  float ax, ay, az, flag;
  float abx, aby, abz, e00;
  float acx, acy, acz, e11;
  float e01, inv_e00, inv_e11, inv_ebc;
  float nx, ny, nz, det;
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return fmaf(ax, bx, fmaf(ay, by, az * bz)); }
__device__ __forceinline__ double dot3d(double ax, double ay, double az, double bx, double by, double bz) { return fma(ax, bx, fma(ay, by, az * bz)); }
// (float)(1 / e), or 0 where e is 0 or that is not finite (a segment of zero length is its end point)
__device__ __forceinline__ float guarded_inv(double e) {
  const float r = (float)(1.0 / e);
  return (e > 0.0 && r < __builtin_inff()) ? r : 0.f;
}

// The record of face f.  What belongs to the face alone is formed in DOUBLE from the fp32 positions and rounded once: the work is done
// once per chunk, and the unit normal of a sliver - its cross product cancels - keeps full fp32 precision.  A face that is never
// selected (an index outside [0, V), a non-finite vertex) has a = NaN: every d2 of it is NaN.
__device__ __forceinline__ FaceRec face_record(const float *__restrict__ pos, int V, const int32_t *__restrict__ faces, int f) {
  FaceRec r;
  const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
  const bool in_range = (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
  const size_t k0 = in_range ? (size_t)i0 * 3 : 0, k1 = in_range ? (size_t)i1 * 3 : 0, k2 = in_range ? (size_t)i2 * 3 : 0;
  const float ax = pos[k0], ay = pos[k0 + 1], az = pos[k0 + 2];
  const double abx = (double)pos[k1] - ax, aby = (double)pos[k1 + 1] - ay, abz = (double)pos[k1 + 2] - az;
  const double acx = (double)pos[k2] - ax, acy = (double)pos[k2 + 1] - ay, acz = (double)pos[k2 + 2] - az;
  const double bcx = acx - abx, bcy = acy - aby, bcz = acz - abz;
  const double e00 = dot3d(abx, aby, abz, abx, aby, abz), e01 = dot3d(abx, aby, abz, acx, acy, acz), e11 = dot3d(acx, acy, acz, acx, acy, acz);
  const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
  const double det = dot3d(nx, ny, nz, nx, ny, nz), inv_len = 1.0 / sqrt(det);
  r.abx = (float)abx, r.aby = (float)aby, r.abz = (float)abz;
  r.acx = (float)acx, r.acy = (float)acy, r.acz = (float)acz;
  r.e00 = (float)e00, r.e01 = (float)e01, r.e11 = (float)e11, r.det = (float)det;
  r.inv_e00 = guarded_inv(e00), r.inv_e11 = guarded_inv(e11), r.inv_ebc = guarded_inv(dot3d(bcx, bcy, bcz, bcx, bcy, bcz));
  const bool triangle = det > 0.0 && inv_len < __builtin_inf() && r.det > 0.f;
  r.nx = triangle ? (float)(nx * inv_len) : 0.f, r.ny = triangle ? (float)(ny * inv_len) : 0.f, r.nz = triangle ? (float)(nz * inv_len) : 0.f;
  r.flag = triangle ? SD_FLAG_TRIANGLE : SD_FLAG_DEGENERATE;
  const bool finite = abx - abx == 0.0 && aby - aby == 0.0 && abz - abz == 0.0 && acx - acx == 0.0 && acy - acy == 0.0 && acz - acz == 0.0 &&
                      fabsf(ax) < __builtin_inff() && fabsf(ay) < __builtin_inff() && fabsf(az) < __builtin_inff();
  const float bad = __builtin_nanf("");
  const bool keep = in_range && finite;
  r.ax = keep ? ax : bad, r.ay = keep ? ay : bad, r.az = keep ? az : bad;
  return r;
}

// squared distance from the point at `ap` (relative to the segment's origin) to the segment o + t e, t in [0, 1]; (qx, qy, qz) = t e
__device__ __forceinline__ float segment_d2(float apx, float apy, float apz, float ex, float ey, float ez, float inv_ee, float &qx, float &qy,
                                            float &qz) {
  const float t = fminf(fmaxf(dot3(apx, apy, apz, ex, ey, ez) * inv_ee, 0.f), 1.f);
  qx = t * ex, qy = t * ey, qz = t * ez;
  const float dx = apx - qx, dy = apy - qy, dz = apz - qz;
  return fmaf(dx, dx, fmaf(dy, dy, dz * dz));
}

// The pair rule of the header.  (px, py, pz) the query; `degenerate`: the record's flag as the caller tests it; returns d2 and the
// closest point RELATIVE TO a in (qx, qy, qz).
__device__ __forceinline__ float pair_d2(const FaceRec &r, bool degenerate, float px, float py, float pz, float &qx, float &qy, float &qz) {
  const float apx = px - r.ax, apy = py - r.ay, apz = pz - r.az;
  if (degenerate) {
    float best = segment_d2(apx, apy, apz, r.abx, r.aby, r.abz, r.inv_e00, qx, qy, qz);
    float tx, ty, tz;
    float d = segment_d2(apx, apy, apz, r.acx, r.acy, r.acz, r.inv_e11, tx, ty, tz);
    if (d < best) best = d, qx = tx, qy = ty, qz = tz;
    d = segment_d2(apx - r.abx, apy - r.aby, apz - r.abz, r.acx - r.abx, r.acy - r.aby, r.acz - r.abz, r.inv_ebc, tx, ty, tz);
    if (d < best) best = d, qx = r.abx + tx, qy = r.aby + ty, qz = r.abz + tz;
    return best;
  }
  // the six dot products, each from its own difference vector: nothing cancels against the distance from a to b or c
  const float bpx = apx - r.abx, bpy = apy - r.aby, bpz = apz - r.abz, cpx = apx - r.acx, cpy = apy - r.acy, cpz = apz - r.acz;
  const float d1 = dot3(r.abx, r.aby, r.abz, apx, apy, apz), d2 = dot3(r.acx, r.acy, r.acz, apx, apy, apz);
  const float d3 = dot3(r.abx, r.aby, r.abz, bpx, bpy, bpz), d4 = dot3(r.acx, r.acy, r.acz, bpx, bpy, bpz);
  const float d5 = dot3(r.abx, r.aby, r.abz, cpx, cpy, cpz), d6 = dot3(r.acx, r.acy, r.acz, cpx, cpy, cpz);
  const float vc = fmaf(r.e00, d2, -(r.e01 * d1)), vb = fmaf(r.e11, d1, -(r.e01 * d2));
  // the interior: the foot of the perpendicular, q = ap - h n with the unit normal n - (s, t) of a sliver would be ill-conditioned
  const float h = dot3(r.nx, r.ny, r.nz, apx, apy, apz);
  float dx = h * r.nx, dy = h * r.ny, dz = h * r.nz;
  // edge bc: q = ab + w bc, from b along the edge itself.  va = d3 d6 - d5 d4 = det - vb - vc is tested by its sign alone:
  // va <= 0  <=>  vb + vc >= det
  const float bcx = r.acx - r.abx, bcy = r.acy - r.aby, bcz = r.acz - r.abz;
  const float w = fminf(fmaxf(dot3(bcx, bcy, bcz, bpx, bpy, bpz) * r.inv_ebc, 0.f), 1.f);
  bool inside = true, on_bc = false;
  if (vb + vc >= r.det && d4 - d3 >= 0.f && d5 - d6 >= 0.f) on_bc = true, inside = false;
  // the other five regions: q = s ab + t ac
  float s = 0.f, t = 0.f;
  if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) s = 0.f, t = d2 * r.inv_e11, inside = false, on_bc = false;  // edge ac
  if (d6 >= 0.f && d5 <= d6) s = 0.f, t = 1.f, inside = false, on_bc = false;                          // vertex c
  if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) s = d1 * r.inv_e00, t = 0.f, inside = false, on_bc = false;  // edge ab
  if (d3 >= 0.f && d4 <= d3) s = 1.f, t = 0.f, inside = false, on_bc = false;                          // vertex b
  if (d1 <= 0.f && d2 <= 0.f) s = 0.f, t = 0.f, inside = false, on_bc = false;                         // vertex a
  const float ex = on_bc ? fmaf(w, bcx, r.abx) : fmaf(t, r.acx, s * r.abx);
  const float ey = on_bc ? fmaf(w, bcy, r.aby) : fmaf(t, r.acy, s * r.aby);
  const float ez = on_bc ? fmaf(w, bcz, r.abz) : fmaf(t, r.acz, s * r.abz);
  qx = inside ? apx - dx : ex, qy = inside ? apy - dy : ey, qz = inside ? apz - dz : ez;
  dx = inside ? dx : apx - ex, dy = inside ? dy : apy - ey, dz = inside ? dz : apz - ez;
  return fmaf(dx, dx, fmaf(dy, dy, dz * dz));
}

__device__ __forceinline__ FaceRec load_record(const float4 *lds, int j) {
  const float4 r0 = lds[j * SD_REC], r1 = lds[j * SD_REC + 1], r2 = lds[j * SD_REC + 2], r3 = lds[j * SD_REC + 3], r4 = lds[j * SD_REC + 4];
  return FaceRec{r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w, r4.x, r4.y, r4.z, r4.w};
}

struct SurfDistArgs {
  const float *pts;        // (n, 3)
  const float *pos;        // (V, 3)
  const int32_t *faces;    // (F, 3)
  int n, V, F, chunks_per_slice;
  u64 *keys;               // [n]: d2 bits << 32 | face, all ones before the launch
  // fp_symmetry_residuals, fp_points_mesh_align (TRANSFORMED): the n queries are g = k n_per + i, query g the point pts[i] under tfs[k]
  const float *tfs;        // (n / n_per, 3, 4) row-major [R|t], tf_stride floats apart: 12, or 16 for the first three rows of (4,4) poses
  int n_per, tf_stride;
  float *q_out;            // (n, 3) or null: the transformed points
};

// the query of the header: q = R p + t per row, the translation innermost
__device__ __forceinline__ void transform_point(const float *__restrict__ m, float x, float y, float z, float &qx, float &qy, float &qz) {
  qx = fmaf(m[0], x, fmaf(m[1], y, fmaf(m[2], z, m[3])));
  qy = fmaf(m[4], x, fmaf(m[5], y, fmaf(m[6], z, m[7])));
  qz = fmaf(m[8], x, fmaf(m[9], y, fmaf(m[10], z, m[11])));
}

// grid (tiles of SD_TILE queries, face slices of chunks_per_slice chunks).  TRANSFORMED: the queries are formed here from (transform,
// point) and never read back; everything after the load is the same code, so the result of a query is the same function of (q, mesh)
template <bool TRANSFORMED>
__global__ __launch_bounds__(SD_THREADS) void surfdist_kernel(SurfDistArgs a) {
  __shared__ float4 lds[SD_CHUNK * SD_REC];
  const int tid = threadIdx.x;
  const int q0 = blockIdx.x * SD_TILE;
  float px[SD_Q], py[SD_Q], pz[SD_Q], best[SD_Q];
  int bface[SD_Q];
#pragma unroll
  for (int q = 0; q < SD_Q; ++q) {
    const int i = min(q0 + q * SD_THREADS + tid, a.n - 1);      // a query past n repeats the last one and is not written
    if (TRANSFORMED) {
      const int k = i / a.n_per, j = i - k * a.n_per;
      transform_point(a.tfs + (size_t)k * a.tf_stride, a.pts[(size_t)j * 3], a.pts[(size_t)j * 3 + 1], a.pts[(size_t)j * 3 + 2], px[q], py[q], pz[q]);
      if (a.q_out && blockIdx.y == 0 && i == q0 + q * SD_THREADS + tid)
        a.q_out[(size_t)i * 3] = px[q], a.q_out[(size_t)i * 3 + 1] = py[q], a.q_out[(size_t)i * 3 + 2] = pz[q];
    } else {
      px[q] = a.pts[(size_t)i * 3], py[q] = a.pts[(size_t)i * 3 + 1], pz[q] = a.pts[(size_t)i * 3 + 2];
    }
    best[q] = __builtin_inff(), bface[q] = -1;
  }
  const long long f_begin = (long long)blockIdx.y * a.chunks_per_slice * SD_CHUNK;
  const int f_end = (int)min((long long)a.F, f_begin + (long long)a.chunks_per_slice * SD_CHUNK);
  for (int c0 = (int)f_begin; c0 < f_end; c0 += SD_CHUNK) {
    const int cnt = min(SD_CHUNK, f_end - c0);
    __syncthreads();                      // the previous chunk has been read by every wave
    for (int j = tid; j < cnt; j += SD_THREADS) {
      const FaceRec r = face_record(a.pos, a.V, a.faces, c0 + j);
      lds[j * SD_REC] = make_float4(r.ax, r.ay, r.az, r.flag);
      lds[j * SD_REC + 1] = make_float4(r.abx, r.aby, r.abz, r.e00);
      lds[j * SD_REC + 2] = make_float4(r.acx, r.acy, r.acz, r.e11);
      lds[j * SD_REC + 3] = make_float4(r.e01, r.inv_e00, r.inv_e11, r.inv_ebc);
      lds[j * SD_REC + 4] = make_float4(r.nx, r.ny, r.nz, r.det);
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const FaceRec r = load_record(lds, j);
      const bool degenerate = __builtin_amdgcn_readfirstlane(__float_as_int(r.flag)) != 0;      // the same in every lane: a scalar branch
#pragma unroll
      for (int q = 0; q < SD_Q; ++q) {
        float qx, qy, qz;
        const float d = pair_d2(r, degenerate, px[q], py[q], pz[q], qx, qy, qz);
        if (d < best[q]) best[q] = d, bface[q] = c0 + j;      // NaN and +inf never pass: such a pair is never selected
      }
    }
  }
#pragma unroll
  for (int q = 0; q < SD_Q; ++q) {
    const int i = q0 + q * SD_THREADS + tid;
    if (i < a.n && bface[q] >= 0) atomicMin(a.keys + i, ((u64)__float_as_uint(best[q]) << 32) | (u64)(unsigned)bface[q]);
  }
}

// one thread per query: the key unpacked; `closest` from the winning pair, evaluated by the same function
__global__ __launch_bounds__(SD_THREADS) void surfdist_finish_kernel(SurfDistArgs a, float *dist, int32_t *face, float *closest) {
  const int i = blockIdx.x * SD_THREADS + threadIdx.x;
  if (i >= a.n) return;
  const u64 key = a.keys[i];
  const int f = (int)(unsigned)(key & 0xffffffffu);
  const bool found = key != ~(u64)0;
  const float nan = __builtin_nanf("");
  dist[i] = found ? sqrtf(__uint_as_float((unsigned)(key >> 32))) : nan;
  if (face) face[i] = found ? f : -1;
  if (!closest) return;
  float cx = nan, cy = nan, cz = nan;
  if (found) {
    const FaceRec r = face_record(a.pos, a.V, a.faces, f);
    float qx, qy, qz;
    (void)pair_d2(r, r.flag != SD_FLAG_TRIANGLE, a.pts[(size_t)i * 3], a.pts[(size_t)i * 3 + 1], a.pts[(size_t)i * 3 + 2], qx, qy, qz);
    cx = r.ax + qx, cy = r.ay + qy, cz = r.az + qz;
  }
  closest[(size_t)i * 3] = cx, closest[(size_t)i * 3 + 1] = cy, closest[(size_t)i * 3 + 2] = cz;
}

// ---- rigid alignment: the rows and the 29 sums of one linearisation (fp_points_mesh_align) ---------------------------------------------
// One of the aligners of gn_sums.h: a workgroup owns (pose, a tile of GN_TILE source points); the pose is uniform in the workgroup.  A
// point's query is formed again by transform_point - the bits the search saw -, its key is unpacked and the winning pair evaluated again
// as in surfdist_finish_kernel; from e = y - closest on, plain products, sums and differences (the header's rule).  ROWS rows a point:
// one (point to plane) or three (point to point, in axis order, the count on the first).  A wave past the pose's last point has +0.0
// sums and nothing to write.
struct MeshAlignArgs {
  const float *pts;        // (n, 3)
  const float *poses;      // (N, 16)
  const float *pos;        // (V, 3)
  const int32_t *faces;    // (F, 3)
  const u64 *keys;         // [N n], as the search left them
  int n, V, n_tiles;
  float dist_max;
  float *dist;             // (N n) or null
  int32_t *face;           // (N n) or null
  float *closest, *normal; // (N n, 3) or null
  float *rows;             // (N n, ROWS, 8) or null
  double *slab;            // [N][n_tiles][GN_TERMS]
};

template <int ROWS>
__global__ __launch_bounds__(GN_THREADS) void mesh_align_kernel(MeshAlignArgs a) {
  static_assert(ROWS == 1 || ROWS == 3, "point to plane or point to point");
  __shared__ double red[GN_THREADS / 64][GN_TERMS];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % a.n_tiles, pr = blockIdx.x / a.n_tiles;
  const float *P = a.poses + (size_t)pr * 16;                      // uniform: scalar loads
  const float t0 = P[3], t1 = P[7], t2 = P[11];
  const size_t item0 = (size_t)pr * (size_t)a.n;
  int pix[GN_PIX];
  bool ok[GN_PIX];
#pragma unroll
  for (int q = 0; q < GN_PIX; ++q) {
    pix[q] = tile * GN_TILE + q * GN_THREADS + tid;
    ok[q] = pix[q] < a.n;                                          // the last tile of a pose is ragged
  }
  if (!gn_empty_wave<ROWS * 8>(ok, a.rows, item0, pix, a.n, red[tid >> 6])) {
    double acc[GN_TERMS];
#pragma unroll
    for (int e = 0; e < GN_TERMS; ++e) acc[e] = 0.0;
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int q = 0; q < GN_PIX; ++q) {
      const size_t i = ok[q] ? (size_t)pix[q] : 0, g = item0 + i;
      float y0, y1, y2;
      transform_point(P, a.pts[i * 3], a.pts[i * 3 + 1], a.pts[i * 3 + 2], y0, y1, y2);
      const u64 key = ok[q] ? a.keys[g] : ~(u64)0;
      const int f = (int)(unsigned)(key & 0xffffffffu);
      const bool found = key != ~(u64)0;
      const float dist = found ? sqrtf(__uint_as_float((unsigned)(key >> 32))) : nan;      // as surfdist_finish_kernel
      float cx = nan, cy = nan, cz = nan, nx = 0.f, ny = 0.f, nz = 0.f;
      bool triangle = false;
      if (found) {
        const FaceRec r = face_record(a.pos, a.V, a.faces, f);
        float qx, qy, qz;
        (void)pair_d2(r, r.flag != SD_FLAG_TRIANGLE, y0, y1, y2, qx, qy, qz);
        cx = r.ax + qx, cy = r.ay + qy, cz = r.az + qz;
        nx = r.nx, ny = r.ny, nz = r.nz;
        triangle = r.flag == SD_FLAG_TRIANGLE;
      }
      if (ok[q]) {
        if (a.dist) a.dist[g] = dist;
        if (a.face) a.face[g] = found ? f : -1;
        if (a.closest) a.closest[g * 3] = cx, a.closest[g * 3 + 1] = cy, a.closest[g * 3 + 2] = cz;
        if (a.normal) a.normal[g * 3] = nx, a.normal[g * 3 + 1] = ny, a.normal[g * 3 + 2] = nz;
      }
      const float e[3] = {y0 - cx, y1 - cy, y2 - cz};
      const float X0 = y0 - t0, X1 = y1 - t1, X2 = y2 - t2;
      const bool within = found && dist <= a.dist_max;               // NaN fails
      if (ROWS == 1) {
        const bool valid = within && triangle;
        float r = (nx * e[0] + ny * e[1]) + nz * e[2], J[6];
        gn_twist_row(J, nx, ny, nz, X0, X1, X2);
        gn_mask(J, r, valid);
        if (a.rows && ok[q]) gn_store_row((float4 *)(a.rows + g * 8), J, r, valid);
        gn_accumulate(acc, J, r, valid);
      } else {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          float r = e[ax], J[6];
          gn_twist_row(J, ax == 0 ? 1.f : 0.f, ax == 1 ? 1.f : 0.f, ax == 2 ? 1.f : 0.f, X0, X1, X2);
          gn_mask(J, r, within);
          if (a.rows && ok[q]) gn_store_row((float4 *)(a.rows + (g * 3 + ax) * 8), J, r, within && ax == 0);      // the count rides on the first row
          gn_accumulate(acc, J, r, within && ax == 0);
        }
      }
    }
    gn_wave_to_lds(acc, red[tid >> 6], 0);
  }
  __syncthreads();
  gn_lds_to_slab(red, a.slab + ((size_t)pr * a.n_tiles + tile) * GN_TERMS);
}

// ---- statistics of a distance array ---------------------------------------------------------------------------------------------------
constexpr int DS_THREADS = 256;
constexpr int DS_ITEMS = 16;
constexpr int DS_TILE = DS_THREADS * DS_ITEMS;           // entries per workgroup
constexpr int DS_TERMS = FP_SURFDIST_STATS_TAU0 + FP_SURFDIST_MAX_TAUS;

struct DistStatsArgs {
  const float *dist;
  int n, n_taus, n_tiles;
  double taus[FP_SURFDIST_MAX_TAUS];
  double *slab;            // [DS_TERMS][n_tiles]
};

__global__ __launch_bounds__(DS_THREADS) void dist_stats_kernel(DistStatsArgs a) {
  __shared__ double red[DS_THREADS / 64];
  double cnt = 0.0, bad = 0.0, s1 = 0.0, s2 = 0.0, mx = 0.0, le[FP_SURFDIST_MAX_TAUS];
#pragma unroll
  for (int t = 0; t < FP_SURFDIST_MAX_TAUS; ++t) le[t] = 0.0;
#pragma unroll 4
  for (int k = 0; k < DS_ITEMS; ++k) {
    const long long i = (long long)blockIdx.x * DS_TILE + k * DS_THREADS + threadIdx.x;
    if (i >= a.n) break;
    const float f = a.dist[i];
    if (!(fabsf(f) < __builtin_inff())) {
      bad += 1.0;
      continue;
    }
    const double d = (double)f;
    cnt += 1.0, s1 += d, s2 = fma(d, d, s2), mx = fmax(mx, d);
#pragma unroll
    for (int t = 0; t < FP_SURFDIST_MAX_TAUS; ++t)
      if (t < a.n_taus && d <= a.taus[t]) le[t] += 1.0;
  }
  double *slab = a.slab + blockIdx.x;
  double v;
  v = block_sum<DS_THREADS>(cnt, red);
  if (threadIdx.x == 0) slab[(size_t)FP_SURFDIST_STATS_COUNT * a.n_tiles] = v;
  v = block_sum<DS_THREADS>(s1, red);
  if (threadIdx.x == 0) slab[(size_t)FP_SURFDIST_STATS_SUM * a.n_tiles] = v;
  v = block_sum<DS_THREADS>(s2, red);
  if (threadIdx.x == 0) slab[(size_t)FP_SURFDIST_STATS_SUM_SQ * a.n_tiles] = v;
  v = block_sum<DS_THREADS>(bad, red);
  if (threadIdx.x == 0) slab[(size_t)FP_SURFDIST_STATS_NOT_FINITE * a.n_tiles] = v;
  mx = wave_max(mx);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < DS_THREADS / 64; ++i) mx = fmax(mx, red[i]);
    slab[(size_t)FP_SURFDIST_STATS_MAX * a.n_tiles] = fmax(mx, red[0]);
  }
#pragma unroll
  for (int t = 0; t < FP_SURFDIST_MAX_TAUS; ++t) {
    if (t >= a.n_taus) break;
    v = block_sum<DS_THREADS>(le[t], red);
    if (threadIdx.x == 0) slab[(size_t)(FP_SURFDIST_STATS_TAU0 + t) * a.n_tiles] = v;
  }
}

// one thread per term: the tile partials in tile order (the maximum: in any order)
__global__ __launch_bounds__(64) void dist_stats_finish_kernel(const double *__restrict__ slab, int n_tiles, int n_terms, double *stats) {
  const int term = threadIdx.x;
  if (term >= n_terms) return;
  const double *p = slab + (size_t)term * n_tiles;
  double s = 0.0;
  if (term == FP_SURFDIST_STATS_MAX)
    for (int t = 0; t < n_tiles; ++t) s = fmax(s, p[t]);
  else
    for (int t = 0; t < n_tiles; ++t) s += p[t];
  stats[term] = s;
}

// ---- statistics per transform (fp_symmetry_residuals) ---------------------------------------------------------------------------------
// The T n keys are tiled by SD_TILE like the queries; a tile may hold the end of one transform, whole ones, and the start of another.  A
// workgroup writes one partial per (tile j, transform k) it holds into column j + k of the slab: along g = k n + i the pair (j, k) only
// ever steps forward, so j + k names each pair once and the columns of transform k are k + its first tile .. k + its last tile.
constexpr int SR_ITEMS = SD_TILE / DS_THREADS;

struct SymStatsArgs {
  const u64 *keys;         // [total]
  int total, n_per, n_taus, n_cols;      // n_cols = tiles + T
  double taus[FP_SURFDIST_MAX_TAUS];
  double *slab;            // [DS_TERMS][n_cols]
  float *dist;             // (total) or null
};

__global__ __launch_bounds__(DS_THREADS) void sym_stats_kernel(SymStatsArgs a) {
  __shared__ double red[DS_TERMS][DS_THREADS / 64];
  const int g0 = blockIdx.x * SD_TILE, g1 = min(g0 + SD_TILE, a.total);
  float d[SR_ITEMS];
  int kq[SR_ITEMS];
#pragma unroll
  for (int q = 0; q < SR_ITEMS; ++q) {
    const int g = g0 + q * DS_THREADS + threadIdx.x;
    d[q] = 0.f, kq[q] = -1;
    if (g < g1) {
      const u64 key = a.keys[g];
      d[q] = key != ~(u64)0 ? sqrtf(__uint_as_float((unsigned)(key >> 32))) : __builtin_nanf("");      // as surfdist_finish_kernel
      kq[q] = g / a.n_per;
      if (a.dist) a.dist[g] = d[q];
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = g0 / a.n_per; k <= (g1 - 1) / a.n_per; ++k) {
    double v[DS_TERMS];
#pragma unroll
    for (int t = 0; t < DS_TERMS; ++t) v[t] = 0.0;
#pragma unroll
    for (int q = 0; q < SR_ITEMS; ++q) {
      if (kq[q] != k) continue;
      if (!(fabsf(d[q]) < __builtin_inff())) {
        v[FP_SURFDIST_STATS_NOT_FINITE] += 1.0;
        continue;
      }
      const double x = (double)d[q];
      v[FP_SURFDIST_STATS_COUNT] += 1.0, v[FP_SURFDIST_STATS_SUM] += x, v[FP_SURFDIST_STATS_SUM_SQ] = fma(x, x, v[FP_SURFDIST_STATS_SUM_SQ]);
      v[FP_SURFDIST_STATS_MAX] = fmax(v[FP_SURFDIST_STATS_MAX], x);
#pragma unroll
      for (int t = 0; t < FP_SURFDIST_MAX_TAUS; ++t)
        if (t < a.n_taus && x <= a.taus[t]) v[FP_SURFDIST_STATS_TAU0 + t] += 1.0;
    }
    // a fixed order: butterfly within each wave, then the waves in order; a lane outside transform k adds 0
#pragma unroll
    for (int t = 0; t < DS_TERMS; ++t) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const double w = __shfl_xor(v[t], o, 64);
        v[t] = t == FP_SURFDIST_STATS_MAX ? fmax(v[t], w) : v[t] + w;
      }
    }
    __syncthreads();                      // `red` of the previous transform has been read
    if (lane == 0) {
#pragma unroll
      for (int t = 0; t < DS_TERMS; ++t) red[t][wave] = v[t];
    }
    __syncthreads();
    if (threadIdx.x < FP_SURFDIST_STATS_TAU0 + a.n_taus) {
      const int t = threadIdx.x;
      double s = 0.0;
      for (int i = 0; i < DS_THREADS / 64; ++i) s = t == FP_SURFDIST_STATS_MAX ? fmax(s, red[t][i]) : s + red[t][i];
      a.slab[(size_t)t * a.n_cols + blockIdx.x + k] = s;
    }
  }
}

// one thread per (transform, term): the partials of the transform's tiles in tile order
__global__ __launch_bounds__(DS_THREADS) void sym_stats_finish_kernel(const double *__restrict__ slab, int n_cols, int n_per, int T, int n_terms,
                                                                      double *stats) {
  const int idx = blockIdx.x * DS_THREADS + threadIdx.x;
  const int k = idx / n_terms, term = idx - k * n_terms;
  if (k >= T) return;
  const int j0 = (int)(((long long)k * n_per) / SD_TILE), j1 = (int)((((long long)k + 1) * n_per - 1) / SD_TILE);
  const double *p = slab + (size_t)term * n_cols + k;
  double s = 0.0;
  if (term == FP_SURFDIST_STATS_MAX)
    for (int j = j0; j <= j1; ++j) s = fmax(s, p[j]);
  else
    for (int j = j0; j <= j1; ++j) s += p[j];
  stats[(size_t)k * n_terms + term] = s;
}

// ---- surface sampler -------------------------------------------------------------------------------------------------------------------
constexpr int SS_THREADS = 256;
constexpr int SS_TOTAL_THREADS = 1024;

// area of face f in double from the fp32 positions: 0.5 |ab x ac|; 0 for a face that is not followed (index out of range) or not finite
__global__ __launch_bounds__(SS_THREADS) void sample_area_kernel(const float *__restrict__ pos, int V, const int32_t *__restrict__ faces, int F,
                                                                 double *area) {
  const int f = blockIdx.x * SS_THREADS + threadIdx.x;
  if (f >= F) return;
  const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
  double A = 0.0;
  if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
    const double ax = pos[(size_t)i0 * 3], ay = pos[(size_t)i0 * 3 + 1], az = pos[(size_t)i0 * 3 + 2];
    const double ux = (double)pos[(size_t)i1 * 3] - ax, uy = (double)pos[(size_t)i1 * 3 + 1] - ay, uz = (double)pos[(size_t)i1 * 3 + 2] - az;
    const double vx = (double)pos[(size_t)i2 * 3] - ax, vy = (double)pos[(size_t)i2 * 3 + 1] - ay, vz = (double)pos[(size_t)i2 * 3 + 2] - az;
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    A = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
    if (!(A < __builtin_inf())) A = 0.0;
  }
  area[f] = A;
}

// one workgroup: total[0] = the sum of the areas (thread t adds faces t, t + 1024, ..; then a tree over the threads)
__global__ __launch_bounds__(SS_TOTAL_THREADS) void sample_total_kernel(const double *__restrict__ area, int F, double *total) {
  __shared__ double red[SS_TOTAL_THREADS];
  double s = 0.0;
  for (int f = threadIdx.x; f < F; f += SS_TOTAL_THREADS) s += area[f];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = SS_TOTAL_THREADS / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) total[0] = red[0];
}

// area_q[f] = rint(area[f] / total 2^40) as int64 (0 when the total is not a positive finite number); prefix[F] = 0 closes the scan
__global__ __launch_bounds__(SS_THREADS) void sample_quantise_kernel(const double *__restrict__ area, const double *__restrict__ total, int F,
                                                                     u64 *prefix, long long *area_q) {
  const int f = blockIdx.x * SS_THREADS + threadIdx.x;
  if (f > F) return;
  const double A = total[0];
  long long q = 0;
  if (f < F && A > 0.0 && A < __builtin_inf()) q = __double2ll_rn(area[f] / A * 1099511627776.0);
  prefix[f] = (u64)q;
  if (f < F && area_q) area_q[f] = q;
}

// Chris Wellons' lowbias32
__device__ __forceinline__ unsigned lowbias32(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// prefix: the exclusive sums of area_q, prefix[F] the total
__global__ __launch_bounds__(SS_THREADS) void sample_points_kernel(const float *__restrict__ pos, const int32_t *__restrict__ faces, int F,
                                                                   const u64 *__restrict__ prefix, int n, unsigned seed, float *points,
                                                                   int32_t *face, float *bary) {
  const int i = blockIdx.x * SS_THREADS + threadIdx.x;
  if (i >= n) return;
  const u64 total = prefix[F];
  const u64 t = ((2ull * (u64)i + 1ull) * total) / (2ull * (u64)n);
  // the first face whose inclusive sum prefix[f + 1] exceeds t (total > t: it exists whenever total > 0)
  int lo = 0, hi = F - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid + 1] > t) hi = mid; else lo = mid + 1;
  }
  const int f = lo;
  const unsigned base = lowbias32(seed);
  unsigned ku = lowbias32(base + 2u * (unsigned)i) >> 8, kv = lowbias32(base + 2u * (unsigned)i + 1u) >> 8;
  if (ku + kv >= (1u << 24)) ku = (1u << 24) - 1u - ku, kv = (1u << 24) - 1u - kv;      // u + v > 1: reflected, exactly
  const float u = (float)(((double)ku + 0.5) * (1.0 / 16777216.0)), v = (float)(((double)kv + 0.5) * (1.0 / 16777216.0));
  const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];      // in range: its area is > 0
  const bool ok = total > 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float p = __builtin_nanf("");
    if (ok) {
      const float a = pos[(size_t)i0 * 3 + k];
      p = fmaf(v, pos[(size_t)i2 * 3 + k] - a, fmaf(u, pos[(size_t)i1 * 3 + k] - a, a));
    }
    points[(size_t)i * 3 + k] = p;
  }
  if (face) face[i] = ok ? f : -1;
  if (bary) bary[(size_t)i * 2] = u, bary[(size_t)i * 2 + 1] = v;
}

}  // namespace

extern "C" int fp_point_mesh_distance(fp_ctx *ctx, const float *d_points, int n, const float *d_pos, int V, const int32_t *d_faces, int F,
                                      float *d_dist, int32_t *d_face, float *d_closest, void *stream) {
  FP_REQUIRE(ctx && d_pos && d_faces, "fp_point_mesh_distance: null argument");
  FP_REQUIRE(V >= 1 && F >= 1 && F <= FP_SURFDIST_MAX_FACES, "fp_point_mesh_distance: V %d, F %d (at least 1; at most %d faces)", V, F,
             FP_SURFDIST_MAX_FACES);
  FP_REQUIRE(n >= 0 && n <= FP_SURFDIST_MAX_POINTS, "fp_point_mesh_distance: n %d (0 .. %d)", n, FP_SURFDIST_MAX_POINTS);
  if (n == 0) return FP_OK;
  FP_REQUIRE(d_points && d_dist, "fp_point_mesh_distance: null d_points or d_dist with n %d", n);
  hipStream_t s = (hipStream_t)stream;
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  const size_t bytes = (size_t)n * sizeof(u64);
  FP_TRY(fp_arena_ensure(ctx, bytes + 4096));
  ArenaScope scope(ctx->arena);
  u64 *keys = (u64 *)ctx->arena.take(bytes);
  FP_REQUIRE(keys, "fp_point_mesh_distance: arena exhausted");
  FP_CHECK_HIP(hipMemsetAsync(keys, 0xff, bytes, s));
  const int tiles = (n + SD_TILE - 1) / SD_TILE, chunks = (F + SD_CHUNK - 1) / SD_CHUNK;
  const int slices = std::min(chunks, std::max(1, (SD_MIN_GROUPS + tiles - 1) / tiles));
  SurfDistArgs a{d_points, d_pos, d_faces, n, V, F, (chunks + slices - 1) / slices, keys, nullptr, 0, 0, nullptr};
  const int slices_used = (chunks + a.chunks_per_slice - 1) / a.chunks_per_slice;
  hipLaunchKernelGGL(surfdist_kernel<false>, dim3((unsigned)tiles, (unsigned)slices_used), dim3(SD_THREADS), 0, s, a);
  FP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(surfdist_finish_kernel, dim3((unsigned)((n + SD_THREADS - 1) / SD_THREADS)), dim3(SD_THREADS), 0, s, a, d_dist, d_face,
                     d_closest);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

extern "C" int fp_symmetry_residuals(fp_ctx *ctx, const float *d_points, int n, const float *d_tfs, int T, const float *d_pos, int V,
                                     const int32_t *d_faces, int F, const double *h_taus, int n_taus, double *d_stats, float *d_q, float *d_dist,
                                     void *stream) {
  FP_REQUIRE(ctx && d_pos && d_faces && d_tfs && d_stats, "fp_symmetry_residuals: null argument");
  FP_REQUIRE(V >= 1 && F >= 1 && F <= FP_SURFDIST_MAX_FACES, "fp_symmetry_residuals: V %d, F %d (at least 1; at most %d faces)", V, F,
             FP_SURFDIST_MAX_FACES);
  FP_REQUIRE(T >= 1 && n >= 0 && (long long)T * n <= FP_SURFDIST_MAX_POINTS, "fp_symmetry_residuals: T %d, n %d (T at least 1, T n 0 .. %d)", T, n,
             FP_SURFDIST_MAX_POINTS);
  FP_REQUIRE(n_taus >= 0 && n_taus <= FP_SURFDIST_MAX_TAUS && (h_taus || n_taus == 0), "fp_symmetry_residuals: n_taus %d (0 .. %d)", n_taus,
             FP_SURFDIST_MAX_TAUS);
  FP_REQUIRE(d_points || n == 0, "fp_symmetry_residuals: d_points null with n %d", n);
  hipStream_t s = (hipStream_t)stream;
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  const int n_terms = FP_SURFDIST_STATS_TAU0 + n_taus;
  if (n == 0) {
    FP_CHECK_HIP(hipMemsetAsync(d_stats, 0, (size_t)T * n_terms * sizeof(double), s));
    return FP_OK;
  }
  const int total = T * n;
  const int tiles = (total + SD_TILE - 1) / SD_TILE, chunks = (F + SD_CHUNK - 1) / SD_CHUNK;
  SymStatsArgs st;
  st.total = total, st.n_per = n, st.n_taus = n_taus, st.n_cols = tiles + T, st.dist = d_dist;
  for (int t = 0; t < FP_SURFDIST_MAX_TAUS; ++t) st.taus[t] = t < n_taus ? h_taus[t] : 0.0;
  const size_t key_bytes = (size_t)total * sizeof(u64), slab_bytes = (size_t)DS_TERMS * st.n_cols * sizeof(double);
  FP_TRY(fp_arena_ensure(ctx, key_bytes + slab_bytes + 256 + 4096));
  ArenaScope scope(ctx->arena);
  u64 *keys = (u64 *)ctx->arena.take(key_bytes);
  st.slab = (double *)ctx->arena.take(slab_bytes);
  FP_REQUIRE(keys && st.slab, "fp_symmetry_residuals: arena exhausted");
  st.keys = keys;
  FP_CHECK_HIP(hipMemsetAsync(keys, 0xff, key_bytes, s));
  const int slices = std::min(chunks, std::max(1, (SD_MIN_GROUPS + tiles - 1) / tiles));
  SurfDistArgs a{d_points, d_pos, d_faces, total, V, F, (chunks + slices - 1) / slices, keys, d_tfs, n, 12, d_q};
  const int slices_used = (chunks + a.chunks_per_slice - 1) / a.chunks_per_slice;
  hipLaunchKernelGGL(surfdist_kernel<true>, dim3((unsigned)tiles, (unsigned)slices_used), dim3(SD_THREADS), 0, s, a);
  FP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(sym_stats_kernel, dim3((unsigned)tiles), dim3(DS_THREADS), 0, s, st);
  FP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(sym_stats_finish_kernel, dim3((unsigned)(((long long)T * n_terms + DS_THREADS - 1) / DS_THREADS)), dim3(DS_THREADS), 0, s,
                     (const double *)st.slab, st.n_cols, n, T, n_terms, d_stats);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

namespace {

struct MeshAlignOut {
  float *q, *dist;
  int32_t *face;
  float *closest, *normal, *rows;
};

// the value checks the two calls share; nothing here looks into ctx
int mesh_align_checks(const char *fn, const float *d_points, int n, int N, int V, int F, const void *d_keys) {
  FP_REQUIRE(N >= 0 && N <= FP_POSE_ALIGN_MAX_POSES, "%s: N %d (0 .. %d)", fn, N, FP_POSE_ALIGN_MAX_POSES);
  FP_REQUIRE(n >= 0 && (long long)N * n <= FP_SURFDIST_MAX_POINTS, "%s: N %d, n %d (n at least 0, N n at most %d)", fn, N, n, FP_SURFDIST_MAX_POINTS);
  FP_REQUIRE(V >= 1 && F >= 1 && F <= FP_SURFDIST_MAX_FACES, "%s: V %d, F %d (at least 1; at most %d faces)", fn, V, F, FP_SURFDIST_MAX_FACES);
  FP_REQUIRE(d_points || n == 0, "%s: d_points null with n %d", fn, n);
  FP_REQUIRE(((uintptr_t)d_keys & 7) == 0, "%s: d_keys is not 8-byte aligned", fn);
  return FP_OK;
}

int mesh_align_stage_checks(const char *fn, int mode, float dist_max) {
  FP_REQUIRE(mode == FP_MESH_ALIGN_PLANE || mode == FP_MESH_ALIGN_POINT, "%s: mode %d (FP_MESH_ALIGN_PLANE or FP_MESH_ALIGN_POINT)", fn, mode);
  FP_REQUIRE(dist_max > 0.f, "%s: dist_max %g (> 0)", fn, (double)dist_max);
  return FP_OK;
}

int mesh_align_tiles(int n) { return (n + GN_TILE - 1) / GN_TILE; }      // <= 2^14, times 1024 poses: inside a grid
size_t mesh_align_slab_bytes(int N, int n) { return (size_t)N * (size_t)mesh_align_tiles(n) * GN_TERMS * sizeof(double); }

// Sets n 64-bit words: the keys to all ones, the records of d_state and empty sums to zero bytes.  A launch, not hipMemsetAsync: these
// calls are made to sit in a captured graph, and no captured path of the library holds a memset node.
__global__ __launch_bounds__(256) void fill_words_kernel(u64 *__restrict__ p, size_t n, u64 value) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = value;
}

int launch_fill_words(u64 *p, size_t n, u64 value, hipStream_t s) {
  if (n == 0) return FP_OK;
  hipLaunchKernelGGL(fill_words_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, n, value);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

// the launches of one linearisation, N >= 1: the keys set to all ones, the search, the rows, the fold.  `slab` holds
// mesh_align_slab_bytes.  With h_sums the sums are copied there and the stream is synchronised; without, nothing synchronises
int launch_mesh_align(const float *pts, int n, const float *poses, int N, const float *pos, int V, const int32_t *faces, int F, int mode,
                      float dist_max, u64 *keys, const MeshAlignOut &o, double *slab, double *sums, double *h_sums, hipStream_t s) {
  if (n == 0) {                           // no rows: zero sums
    FP_TRY(launch_fill_words((u64 *)sums, (size_t)N * GN_TERMS, 0, s));
    if (h_sums) {
      memset(h_sums, 0, (size_t)N * GN_TERMS * sizeof(double));
      FP_CHECK_HIP(hipStreamSynchronize(s));
    }
    return FP_OK;
  }
  const int total = N * n;
  FP_TRY(launch_fill_words(keys, (size_t)total, ~(u64)0, s));
  const int tiles = (total + SD_TILE - 1) / SD_TILE, chunks = (F + SD_CHUNK - 1) / SD_CHUNK;
  const int slices = std::min(chunks, std::max(1, (SD_MIN_GROUPS + tiles - 1) / tiles));
  SurfDistArgs a{pts, pos, faces, total, V, F, (chunks + slices - 1) / slices, keys, poses, n, 16, o.q};
  const int slices_used = (chunks + a.chunks_per_slice - 1) / a.chunks_per_slice;
  hipLaunchKernelGGL(surfdist_kernel<true>, dim3((unsigned)tiles, (unsigned)slices_used), dim3(SD_THREADS), 0, s, a);
  FP_CHECK_HIP(hipGetLastError());
  const int n_tiles = mesh_align_tiles(n);
  MeshAlignArgs m{pts, poses, pos, faces, keys, n, V, n_tiles, dist_max, o.dist, o.face, o.closest, o.normal, o.rows, slab};
  if (mode == FP_MESH_ALIGN_PLANE)
    hipLaunchKernelGGL(mesh_align_kernel<1>, dim3((unsigned)(n_tiles * N)), dim3(GN_THREADS), 0, s, m);
  else
    hipLaunchKernelGGL(mesh_align_kernel<3>, dim3((unsigned)(n_tiles * N)), dim3(GN_THREADS), 0, s, m);
  FP_CHECK_HIP(hipGetLastError());
  return gn_fold_to_host<GN_TERMS>(slab, N, n_tiles, sums, h_sums, s);
}

}  // namespace

extern "C" int fp_points_mesh_align(fp_ctx *ctx, const float *d_points, int n, const float *d_poses, int N, const float *d_pos, int V,
                                    const int32_t *d_faces, int F, int mode, float dist_max, uint64_t *d_keys, float *d_q, float *d_dist,
                                    int32_t *d_face, float *d_closest, float *d_normal, float *d_rows, double *d_sums, double *h_sums,
                                    void *stream) {
  // Every check of a value comes before the first look INTO ctx, as in pose_icp.hip: tests/test_mesh_align_host.py calls this without a
  // GPU, with a pointer for ctx that must not be dereferenced.
  FP_REQUIRE(ctx && d_poses && d_pos && d_faces && d_keys && d_sums, "fp_points_mesh_align: null argument");
  FP_TRY(mesh_align_checks("fp_points_mesh_align", d_points, n, N, V, F, d_keys));
  FP_TRY(mesh_align_stage_checks("fp_points_mesh_align", mode, dist_max));
  FP_REQUIRE(((uintptr_t)d_rows & 15) == 0, "fp_points_mesh_align: d_rows is not 16-byte aligned (it is written as float4)");
  if (N == 0) return FP_OK;
  hipStream_t s = (hipStream_t)stream;
  const size_t slab_bytes = mesh_align_slab_bytes(N, n);
  FP_TRY(fp_arena_ensure(ctx, slab_bytes + 4096));
  // the slab goes back to the arena when the launches are queued (with h_sums: synchronised) - the next taker runs behind them on the same stream
  ArenaScope scope(ctx->arena);
  double *slab = (double *)ctx->arena.take(slab_bytes);
  FP_REQUIRE(slab, "fp_points_mesh_align: arena exhausted");
  const MeshAlignOut o{d_q, d_dist, d_face, d_closest, d_normal, d_rows};
  return launch_mesh_align(d_points, n, d_poses, N, d_pos, V, d_faces, F, mode, dist_max, (u64 *)d_keys, o, slab, d_sums, h_sums, s);
}

extern "C" int fp_points_mesh_polish(fp_ctx *ctx, const float *d_points, int n, float *d_poses, int N, const float *d_pos, int V,
                                     const int32_t *d_faces, int F, const fp_mesh_align_stage *h_stages, int n_stages, double damping,
                                     int min_points, fp_pose_state *d_state, double *d_sums, uint64_t *d_keys, void *stream) {
  // As above: every check of a value before the first look into ctx.
  FP_REQUIRE(ctx && d_poses && d_pos && d_faces && d_keys && d_sums && d_state && h_stages, "fp_points_mesh_polish: null argument");
  FP_TRY(mesh_align_checks("fp_points_mesh_polish", d_points, n, N, V, F, d_keys));
  FP_REQUIRE(((uintptr_t)d_state & 7) == 0, "fp_points_mesh_polish: d_state is not 8-byte aligned");
  FP_REQUIRE(n_stages >= 1 && n_stages <= FP_MESH_ALIGN_MAX_STAGES, "fp_points_mesh_polish: n_stages %d (1 .. %d)", n_stages, FP_MESH_ALIGN_MAX_STAGES);
  for (int k = 0; k < n_stages; ++k) {
    FP_TRY(mesh_align_stage_checks("fp_points_mesh_polish", h_stages[k].mode, h_stages[k].dist_max));
    FP_REQUIRE(h_stages[k].iterations >= 0 && h_stages[k].iterations <= FP_POSE_POLISH_MAX_ITERATIONS,
               "fp_points_mesh_polish: stage %d has %d iterations (0 .. %d)", k, h_stages[k].iterations, FP_POSE_POLISH_MAX_ITERATIONS);
  }
  FP_REQUIRE(damping >= 0.0 && isfinite(damping), "fp_points_mesh_polish: damping %g (>= 0, finite)", damping);
  FP_REQUIRE(min_points >= 1, "fp_points_mesh_polish: min_points %d (>= 1)", min_points);
  if (N == 0) return FP_OK;
  hipStream_t s = (hipStream_t)stream;
  const size_t slab_bytes = mesh_align_slab_bytes(N, n);
  FP_TRY(fp_arena_ensure(ctx, slab_bytes + 4096));
  // the slab goes back when the launches are queued - the next taker runs behind them on the same stream
  ArenaScope scope(ctx->arena);
  double *slab = (double *)ctx->arena.take(slab_bytes);
  FP_REQUIRE(slab, "fp_points_mesh_polish: arena exhausted");
  const MeshAlignOut none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < n_stages; ++k) {
    const fp_mesh_align_stage &st = h_stages[k];
    const bool last = k == n_stages - 1;
    FP_TRY(launch_fill_words((u64 *)d_state, (size_t)N * (sizeof(fp_pose_state) / sizeof(u64)), 0, s));      // every stage starts fresh records
    for (int it = 0; it < st.iterations + (last ? 1 : 0); ++it) {                         // the last stage ends with the closing round
      FP_TRY(launch_mesh_align(d_points, n, d_poses, N, d_pos, V, d_faces, F, st.mode, st.dist_max, (u64 *)d_keys, none, slab, d_sums, nullptr, s));
      FP_TRY(fp_pose_gn_step(ctx, d_sums, d_poses, d_state, N, damping, min_points, last && it == st.iterations, stream));
    }
  }
  return FP_OK;
}

extern "C" int fp_distance_stats(fp_ctx *ctx, const float *d_dist, int n, const double *h_taus, int n_taus, double *d_stats, void *stream) {
  FP_REQUIRE(ctx && d_stats, "fp_distance_stats: null argument");
  FP_REQUIRE(n >= 0 && n <= FP_SURFDIST_MAX_POINTS, "fp_distance_stats: n %d (0 .. %d)", n, FP_SURFDIST_MAX_POINTS);
  FP_REQUIRE(d_dist || n == 0, "fp_distance_stats: d_dist null with n %d", n);
  FP_REQUIRE(n_taus >= 0 && n_taus <= FP_SURFDIST_MAX_TAUS && (h_taus || n_taus == 0), "fp_distance_stats: n_taus %d (0 .. %d)", n_taus,
             FP_SURFDIST_MAX_TAUS);
  hipStream_t s = (hipStream_t)stream;
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  const int n_terms = FP_SURFDIST_STATS_TAU0 + n_taus;
  if (n == 0) {
    FP_CHECK_HIP(hipMemsetAsync(d_stats, 0, (size_t)n_terms * sizeof(double), s));
    return FP_OK;
  }
  DistStatsArgs a;
  a.dist = d_dist, a.n = n, a.n_taus = n_taus, a.n_tiles = (n + DS_TILE - 1) / DS_TILE;
  for (int t = 0; t < FP_SURFDIST_MAX_TAUS; ++t) a.taus[t] = t < n_taus ? h_taus[t] : 0.0;
  const size_t bytes = (size_t)DS_TERMS * a.n_tiles * sizeof(double);
  FP_TRY(fp_arena_ensure(ctx, bytes + 4096));
  ArenaScope scope(ctx->arena);
  a.slab = (double *)ctx->arena.take(bytes);
  FP_REQUIRE(a.slab, "fp_distance_stats: arena exhausted");
  hipLaunchKernelGGL(dist_stats_kernel, dim3((unsigned)a.n_tiles), dim3(DS_THREADS), 0, s, a);
  FP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(dist_stats_finish_kernel, dim3(1), dim3(64), 0, s, (const double *)a.slab, a.n_tiles, n_terms, d_stats);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

extern "C" int fp_mesh_sample_surface(fp_ctx *ctx, const float *d_pos, int V, const int32_t *d_faces, int F, int n, uint32_t seed,
                                      float *d_points, int32_t *d_face, float *d_bary, int64_t *d_area_q, void *stream) {
  FP_REQUIRE(ctx && d_pos && d_faces, "fp_mesh_sample_surface: null argument");
  FP_REQUIRE(V >= 1 && F >= 1 && F <= FP_SURFDIST_MAX_FACES, "fp_mesh_sample_surface: V %d, F %d (at least 1; at most %d faces)", V, F,
             FP_SURFDIST_MAX_FACES);
  FP_REQUIRE(n >= 0 && n <= FP_SURFDIST_MAX_SAMPLES, "fp_mesh_sample_surface: n %d (0 .. %d)", n, FP_SURFDIST_MAX_SAMPLES);
  FP_REQUIRE(d_points || n == 0, "fp_mesh_sample_surface: d_points null with n %d", n);
  hipStream_t s = (hipStream_t)stream;
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  const size_t area_bytes = (size_t)F * sizeof(double), prefix_bytes = ((size_t)F + 1) * sizeof(u64);
  const size_t sums_bytes = scan_sums_words((long long)F + 1) * sizeof(u64);
  FP_TRY(fp_arena_ensure(ctx, area_bytes + prefix_bytes + sums_bytes + 256 + 5 * 256 + 4096));
  ArenaScope scope(ctx->arena);
  double *area = (double *)ctx->arena.take(area_bytes);
  double *total = (double *)ctx->arena.take(256);
  u64 *prefix = (u64 *)ctx->arena.take(prefix_bytes);
  u64 *sums = (u64 *)ctx->arena.take(sums_bytes);
  FP_REQUIRE(area && total && prefix && sums, "fp_mesh_sample_surface: arena exhausted");
  const unsigned fb = (unsigned)((F + SS_THREADS - 1) / SS_THREADS);
  hipLaunchKernelGGL(sample_area_kernel, dim3(fb), dim3(SS_THREADS), 0, s, d_pos, V, d_faces, F, area);
  FP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(sample_total_kernel, dim3(1), dim3(SS_TOTAL_THREADS), 0, s, (const double *)area, F, total);
  FP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(sample_quantise_kernel, dim3((unsigned)((F + 1 + SS_THREADS - 1) / SS_THREADS)), dim3(SS_THREADS), 0, s,
                     (const double *)area, (const double *)total, F, prefix, (long long *)d_area_q);
  FP_CHECK_HIP(hipGetLastError());
  // the one synchronisation: a mesh without area cannot be sampled, and the caller is told so
  double h_total = 0.0;
  FP_CHECK_HIP(hipMemcpyAsync(&h_total, total, sizeof(double), hipMemcpyDeviceToHost, s));
  FP_CHECK_HIP(hipStreamSynchronize(s));
  FP_REQUIRE(h_total > 0.0 && h_total < __builtin_inf(), "fp_mesh_sample_surface: the mesh's total area is %g (it must be positive and finite)",
             h_total);
  if (n == 0) return FP_OK;
  FP_TRY(scan_exclusive(prefix, (long long)F + 1, sums, s));
  hipLaunchKernelGGL(sample_points_kernel, dim3((unsigned)((n + SS_THREADS - 1) / SS_THREADS)), dim3(SS_THREADS), 0, s, d_pos, d_faces, F,
                     (const u64 *)prefix, n, (unsigned)seed, d_points, d_face, d_bary);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
