// Vertex-clustering mesh simplification (fp_mesh_simplify_count / _write).  The rule is stated in include/foundationpose_amd.h and restated
// in numpy by tests/mesh_simplify_oracle.py; this file follows it operation for operation (the library is built without contraction).
//
// Everything written out is a function of the input alone, whatever order the lanes run in:
//   * the bounding box is a min / max, taken with integer atomics on the order-preserving image of the float bits;
//   * a cluster is found through an open-addressing table on the packed cell (cz << 42 | cy << 21 | cx - the same partition as the
//     header's key, without a wait for the dims): a 64-bit compare-and-swap claims a slot, atomicMin records the lowest member.  WHICH
//     slot a cluster gets depends on the race; nothing below reads a slot number except to find that lowest member again;
//   * clusters are numbered by an exclusive scan over "this vertex is the lowest member of its cluster" (scan_exclusive, scan.hip);
//   * faces go through a second table keyed on the sorted id triple, atomicMin of the face index; the survivors and the clusters they
//     reference are numbered by two more scans;
//   * the attribute sums are 64-bit INTEGER adds of fixed-point values: exact, so the order of the adds does not matter.
// There is no floating-point atomic and no wave-level pre-aggregation (DESIGN.md section 5 has the measurement behind that).
//
// All kernels are one thread per vertex or face and move memory: coalesced reads of the inputs, scattered atomics into the tables.  The
// atomics execute at the memory side, so the table passes are bound by atomic requests, not by bytes.
#include "common.h"

#include <math.h>
#include <algorithm>

typedef unsigned long long u64;

namespace {

constexpr int MS_THREADS = 256;
constexpr u64 MS_EMPTY = ~0ull;                 // hipMemset 0xff; a packed key has bit 63 clear
constexpr int MS_MAX_DIM = 1 << 21;
constexpr double MS_FIX = 1073741824.0;         // 2^30

struct MsHead {
  unsigned lo[3], hi[3];      // order-preserving images of the bounding box' float bits
  int err;                    // MS_ERR_*
  int pad;
  u64 total[3];               // clusters, surviving faces, vertices kept
};
enum { MS_ERR_DIM = 1, MS_ERR_FACE = 2 };

// unsigned order of the images = numeric order of the floats
__host__ __device__ __forceinline__ unsigned ord_of(unsigned u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ __forceinline__ unsigned bits_of(unsigned o) { return (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o; }

__device__ __forceinline__ u64 mix64(u64 x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// the slot of `key` in an open-addressing table of mask + 1 slots (never full: at most half of them are ever claimed).  A slot goes
// from MS_EMPTY to one key once and stays, so a plain read that sees the key, or another one, is final; only an empty-looking slot
// needs the compare-and-swap.
__device__ __forceinline__ int table_slot(u64 *__restrict__ keys, unsigned mask, u64 key) {
  unsigned slot = (unsigned)mix64(key) & mask;
  for (unsigned probe = 0; probe <= mask; ++probe) {
    u64 seen = keys[slot];
    if (seen == MS_EMPTY) seen = atomicCAS(&keys[slot], MS_EMPTY, key);
    if (seen == MS_EMPTY || seen == key) return (int)slot;
    slot = (slot + 1) & mask;
  }
  return -1;      // not reached
}

__global__ __launch_bounds__(MS_THREADS) void ms_bbox_kernel(const float *__restrict__ pos, int V, MsHead *__restrict__ head) {
  unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  for (int v = blockIdx.x * MS_THREADS + threadIdx.x; v < V; v += gridDim.x * MS_THREADS)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const unsigned o = ord_of(__float_as_uint(pos[(size_t)v * 3 + a]));
      lo[a] = min(lo[a], o), hi[a] = max(hi[a], o);
    }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      lo[a] = min(lo[a], (unsigned)__shfl_xor((int)lo[a], o, 64));
      hi[a] = max(hi[a], (unsigned)__shfl_xor((int)hi[a], o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&head->lo[a], lo[a]);
      atomicMax(&head->hi[a], hi[a]);
    }
  }
}

// the cell of every vertex, its cluster's slot, the lowest member of every cluster
__global__ __launch_bounds__(MS_THREADS) void ms_vertex_insert_kernel(const float *__restrict__ pos, int V, float cell, MsHead *__restrict__ head,
                                                                      u64 *__restrict__ keys, int *__restrict__ low, unsigned mask,
                                                                      int *__restrict__ vslot) {
  const int v = blockIdx.x * MS_THREADS + threadIdx.x;
  if (v >= V) return;
  u64 key = 0;
  bool bad = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float o = __uint_as_float(bits_of(head->lo[a]));
    const float f = floorf((pos[(size_t)v * 3 + a] - o) / cell);
    const bool ok = f >= 0.f && f < (float)MS_MAX_DIM;      // decided in float: a NaN or a huge value never reaches the cast
    bad = bad || !ok;
    key |= (u64)(ok ? (long long)f : 0ll) << (21 * a);
  }
  if (bad) atomicOr(&head->err, MS_ERR_DIM);
  const int slot = table_slot(keys, mask, key);
  if (slot >= 0) atomicMin(&low[slot], v);
  vslot[v] = max(slot, 0);
}

// data[v] = 1 where v is the lowest member of its cluster; data[V] = 0 closes the scan
__global__ __launch_bounds__(MS_THREADS) void ms_vertex_flag_kernel(int V, const int *__restrict__ low, const int *__restrict__ vslot,
                                                                    u64 *__restrict__ data) {
  const int v = blockIdx.x * MS_THREADS + threadIdx.x;
  if (v > V) return;
  data[v] = v < V && low[vslot[v]] == v ? 1 : 0;
}

// in place: the slot of a vertex becomes the id of its cluster
__global__ __launch_bounds__(MS_THREADS) void ms_cluster_id_kernel(int V, const int *__restrict__ low, const u64 *__restrict__ scan_v, int *vslot) {
  const int v = blockIdx.x * MS_THREADS + threadIdx.x;
  if (v >= V) return;
  vslot[v] = (int)scan_v[low[vslot[v]]];
}

__global__ __launch_bounds__(MS_THREADS) void ms_face_insert_kernel(const int32_t *__restrict__ faces, int F, int V, const int *__restrict__ cid,
                                                                    MsHead *__restrict__ head, u64 *__restrict__ keys, int *__restrict__ low,
                                                                    unsigned mask, int *__restrict__ fslot) {
  const int f = blockIdx.x * MS_THREADS + threadIdx.x;
  if (f >= F) return;
  const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) {
    atomicOr(&head->err, MS_ERR_FACE);
    fslot[f] = -1;
    return;
  }
  const int a = cid[i0], b = cid[i1], c = cid[i2];
  if (a == b || b == c || a == c) {
    fslot[f] = -1;
    return;
  }
  const int lo = min(a, min(b, c)), hi = max(a, max(b, c)), mid = a + b + c - lo - hi;
  const int slot = table_slot(keys, mask, ((u64)lo << 42) | ((u64)mid << 21) | (u64)hi);
  if (slot >= 0) atomicMin(&low[slot], f);
  fslot[f] = slot;
}

// fdata[f] = 1 for a surviving face; rdata[c] = 1 for a cluster one of them references (every writer stores the same word)
__global__ __launch_bounds__(MS_THREADS) void ms_face_flag_kernel(const int32_t *__restrict__ faces, int F, const int *__restrict__ cid,
                                                                  const int *__restrict__ low, const int *__restrict__ fslot,
                                                                  u64 *__restrict__ fdata, u64 *__restrict__ rdata) {
  const int f = blockIdx.x * MS_THREADS + threadIdx.x;
  if (f > F) return;
  const bool keep = f < F && fslot[f] >= 0 && low[fslot[f]] == f;
  fdata[f] = keep ? 1 : 0;
  if (keep)
#pragma unroll
    for (int k = 0; k < 3; ++k) rdata[cid[faces[(size_t)f * 3 + k]]] = 1;
}

__global__ void ms_totals_kernel(const u64 *scan_v, int V, const u64 *fdata, int F, const u64 *rdata, MsHead *head) {
  head->total[0] = scan_v[V];
  head->total[1] = F > 0 ? fdata[F] : 0;
  head->total[2] = F > 0 ? rdata[V] : scan_v[V];
}

// the output vertex of cluster c, or -1.  rdata is the scan over V + 1 words of the referenced flags; null when F == 0 (every cluster kept)
__device__ __forceinline__ int out_vertex(const u64 *__restrict__ rdata, int c) {
  if (!rdata) return c;
  const u64 r = rdata[c];
  return rdata[c + 1] != r ? (int)r : -1;
}

// acc row of an output vertex: 0..2 sum q, 3 members, 4..6 sum of the fixed-point normals, 7 unused (one 64-byte line); cacc: 3 colour sums
__global__ __launch_bounds__(MS_THREADS) void ms_accumulate_kernel(const float *__restrict__ pos, const float *__restrict__ nrm,
                                                                   const uint8_t *__restrict__ col, int V, const MsHead *__restrict__ head,
                                                                   const int *__restrict__ cid, const u64 *__restrict__ rdata,
                                                                   u64 *__restrict__ acc, unsigned *__restrict__ cacc, int32_t *__restrict__ vmap) {
  const int v = blockIdx.x * MS_THREADS + threadIdx.x;
  if (v >= V) return;
  const int out = out_vertex(rdata, cid[v]);
  if (vmap) vmap[v] = out;
  if (out < 0) return;
  u64 *row = acc + (size_t)out * 8;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double o = (double)__uint_as_float(bits_of(head->lo[a]));
    atomicAdd(&row[a], (u64)llrint(((double)pos[(size_t)v * 3 + a] - o) * MS_FIX));
  }
  atomicAdd(&row[3], 1ull);
  if (nrm)
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicAdd(&row[4 + a], (u64)llrint((double)nrm[(size_t)v * 3 + a] * MS_FIX));
  if (col)
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicAdd(&cacc[(size_t)out * 4 + a], (unsigned)col[(size_t)v * 3 + a]);
}

// the lowest member of every kept cluster writes its output vertex
__global__ __launch_bounds__(MS_THREADS) void ms_vertex_write_kernel(const float *__restrict__ pos, const float *__restrict__ nrm,
                                                                     const uint8_t *__restrict__ col, int V, const MsHead *__restrict__ head,
                                                                     const u64 *__restrict__ scan_v, const u64 *__restrict__ rdata,
                                                                     const u64 *__restrict__ acc, const unsigned *__restrict__ cacc,
                                                                     float *__restrict__ out_pos, float *__restrict__ out_nrm,
                                                                     uint8_t *__restrict__ out_col) {
  const int v = blockIdx.x * MS_THREADS + threadIdx.x;
  if (v >= V) return;
  const u64 c = scan_v[v];
  if (scan_v[v + 1] == c) return;
  const int out = out_vertex(rdata, (int)c);
  if (out < 0) return;
  const u64 *row = acc + (size_t)out * 8;
  const long long n = (long long)row[3];
  if (n == 1) {         // a cluster of one keeps its member's bits
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      out_pos[(size_t)out * 3 + a] = pos[(size_t)v * 3 + a];
      if (out_nrm) out_nrm[(size_t)out * 3 + a] = nrm[(size_t)v * 3 + a];
      if (out_col) out_col[(size_t)out * 3 + a] = col[(size_t)v * 3 + a];
    }
    return;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double o = (double)__uint_as_float(bits_of(head->lo[a]));
    out_pos[(size_t)out * 3 + a] = (float)(o + ((double)(long long)row[a] / (double)n) / MS_FIX);
  }
  if (out_nrm) {
    const double sx = (double)(long long)row[4], sy = (double)(long long)row[5], sz = (double)(long long)row[6];
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    out_nrm[(size_t)out * 3] = len > 0.0 ? (float)(sx / len) : 0.f;
    out_nrm[(size_t)out * 3 + 1] = len > 0.0 ? (float)(sy / len) : 0.f;
    out_nrm[(size_t)out * 3 + 2] = len > 0.0 ? (float)(sz / len) : 0.f;
  }
  if (out_col)
#pragma unroll
    for (int a = 0; a < 3; ++a) out_col[(size_t)out * 3 + a] = (uint8_t)((2ll * (long long)cacc[(size_t)out * 4 + a] + n) / (2ll * n));
}

__global__ __launch_bounds__(MS_THREADS) void ms_face_write_kernel(const int32_t *__restrict__ faces, int F, const int *__restrict__ cid,
                                                                   const u64 *__restrict__ fdata, const u64 *__restrict__ rdata,
                                                                   int32_t *__restrict__ out_faces) {
  const int f = blockIdx.x * MS_THREADS + threadIdx.x;
  if (f >= F) return;
  const u64 o = fdata[f];
  if (fdata[f + 1] == o) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) out_faces[(size_t)o * 3 + k] = (int32_t)rdata[cid[faces[(size_t)f * 3 + k]]];      // a surviving face's clusters are all referenced
}

unsigned table_slots(long long n) {
  unsigned cap = 1024;
  while ((long long)cap < 2 * n) cap <<= 1;
  return cap;
}

}  // namespace

// What fp_mesh_simplify_count leaves for fp_mesh_simplify_write: one allocation owned by the context, grown when a larger mesh arrives.
struct fp_simplify_state {
  DevBlob blob;
  DevBlob acc;                // the attribute sums of fp_mesh_simplify_write: 80 bytes per output vertex
  // views into blob
  MsHead *head = nullptr;
  u64 *vkeys = nullptr, *fkeys = nullptr, *scan_v = nullptr, *rdata = nullptr, *fdata = nullptr, *sums = nullptr;
  int *vlow = nullptr, *flow = nullptr, *cid = nullptr, *fslot = nullptr;
  // the counted call
  bool valid = false;
  const float *pos = nullptr;
  const int32_t *faces = nullptr;
  int V = 0, F = 0;
  float cell = 0.f;
  long long nv = 0, nf = 0;
};

void fp_simplify_state_free(fp_ctx *ctx) {
  fp_simplify_state *st = ctx->simplify;
  if (!st) return;
  st->blob.release();
  st->acc.release();
  delete st;
  ctx->simplify = nullptr;
}

static int simplify_layout(fp_simplify_state *st, int V, int F) {
  const unsigned vcap = table_slots(V), fcap = F > 0 ? table_slots(F) : 0;
  const long long nscan = (long long)(V > F ? V : F) + 1;
  BlobLayout l;
  const size_t o_head = l.put(sizeof(MsHead)), o_vkeys = l.put((size_t)vcap * 8), o_fkeys = l.put((size_t)fcap * 8), o_scan = l.put(((size_t)V + 1) * 8),
               o_rdata = l.put(((size_t)V + 1) * 8), o_fdata = l.put(((size_t)F + 1) * 8), o_sums = l.put(scan_sums_words(nscan) * 8),
               o_vlow = l.put((size_t)vcap * 4), o_flow = l.put((size_t)fcap * 4), o_cid = l.put((size_t)V * 4), o_fslot = l.put((size_t)F * 4);
  FP_TRY(st->blob.ensure(l.bytes, "fp_mesh_simplify_count", "the tables"));
  const DevBlob &b = st->blob;
  st->head = b.at<MsHead>(o_head);
  st->vkeys = b.at<u64>(o_vkeys), st->fkeys = b.at<u64>(o_fkeys), st->scan_v = b.at<u64>(o_scan), st->rdata = b.at<u64>(o_rdata);
  st->fdata = b.at<u64>(o_fdata), st->sums = b.at<u64>(o_sums);
  st->vlow = b.at<int>(o_vlow), st->flow = b.at<int>(o_flow), st->cid = b.at<int>(o_cid), st->fslot = b.at<int>(o_fslot);
  return FP_OK;
}

extern "C" int fp_mesh_simplify_count(fp_ctx *ctx, const float *d_pos, int V, const int32_t *d_faces, int F, float cell, int64_t *h_counts,
                                      void *stream) {
  FP_REQUIRE(ctx && h_counts, "fp_mesh_simplify_count: null argument");
  FP_REQUIRE(V >= 0 && V <= FP_MESH_SIMPLIFY_MAX_VERTICES, "fp_mesh_simplify_count: V %d (0 .. %d)", V, FP_MESH_SIMPLIFY_MAX_VERTICES);
  FP_REQUIRE(F >= 0 && F <= FP_MESH_SIMPLIFY_MAX_FACES, "fp_mesh_simplify_count: F %d (0 .. %d)", F, FP_MESH_SIMPLIFY_MAX_FACES);
  FP_REQUIRE((d_pos || V == 0) && (d_faces || F == 0), "fp_mesh_simplify_count: d_pos or d_faces is null");
  FP_REQUIRE(V > 0 || F == 0, "fp_mesh_simplify_count: %d faces without a vertex", F);
  FP_REQUIRE(cell > 0.f && isfinite(cell), "fp_mesh_simplify_count: cell %g (> 0)", (double)cell);
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  if (!ctx->simplify) ctx->simplify = new fp_simplify_state;
  fp_simplify_state *st = ctx->simplify;
  st->valid = false;
  hipStream_t s = (hipStream_t)stream;
  if (V > 0) {
    FP_TRY(simplify_layout(st, V, F));
    const unsigned vcap = table_slots(V), fcap = F > 0 ? table_slots(F) : 0;
    FP_CHECK_HIP(hipMemsetAsync(st->head, 0, sizeof(MsHead), s));
    FP_CHECK_HIP(hipMemsetAsync(st->head->lo, 0xff, sizeof(st->head->lo), s));
    FP_CHECK_HIP(hipMemsetAsync(st->vkeys, 0xff, (size_t)vcap * 8, s));
    FP_CHECK_HIP(hipMemsetAsync(st->vlow, 0x7f, (size_t)vcap * 4, s));
    const unsigned bb = (unsigned)std::min<long long>(((long long)V + MS_THREADS - 1) / MS_THREADS, 4LL * ctx->num_cu);
    hipLaunchKernelGGL(ms_bbox_kernel, dim3(bb), dim3(MS_THREADS), 0, s, d_pos, V, st->head);
    FP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(ms_vertex_insert_kernel, grid_for(V), dim3(MS_THREADS), 0, s, d_pos, V, cell, st->head, st->vkeys, st->vlow, vcap - 1, st->cid);
    FP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(ms_vertex_flag_kernel, grid_for((long long)V + 1), dim3(MS_THREADS), 0, s, V, (const int *)st->vlow, (const int *)st->cid,
                       st->scan_v);
    FP_CHECK_HIP(hipGetLastError());
    FP_TRY(scan_exclusive(st->scan_v, (long long)V + 1, st->sums, s));
    hipLaunchKernelGGL(ms_cluster_id_kernel, grid_for(V), dim3(MS_THREADS), 0, s, V, (const int *)st->vlow, (const u64 *)st->scan_v, st->cid);
    FP_CHECK_HIP(hipGetLastError());
    if (F > 0) {
      FP_CHECK_HIP(hipMemsetAsync(st->fkeys, 0xff, (size_t)fcap * 8, s));
      FP_CHECK_HIP(hipMemsetAsync(st->flow, 0x7f, (size_t)fcap * 4, s));
      FP_CHECK_HIP(hipMemsetAsync(st->rdata, 0, ((size_t)V + 1) * 8, s));
      hipLaunchKernelGGL(ms_face_insert_kernel, grid_for(F), dim3(MS_THREADS), 0, s, d_faces, F, V, (const int *)st->cid, st->head, st->fkeys, st->flow,
                         fcap - 1, st->fslot);
      FP_CHECK_HIP(hipGetLastError());
      hipLaunchKernelGGL(ms_face_flag_kernel, grid_for((long long)F + 1), dim3(MS_THREADS), 0, s, d_faces, F, (const int *)st->cid,
                         (const int *)st->flow, (const int *)st->fslot, st->fdata, st->rdata);
      FP_CHECK_HIP(hipGetLastError());
      FP_TRY(scan_exclusive(st->fdata, (long long)F + 1, st->sums, s));
      FP_TRY(scan_exclusive(st->rdata, (long long)V + 1, st->sums, s));
    }
    hipLaunchKernelGGL(ms_totals_kernel, dim3(1), dim3(1), 0, s, (const u64 *)st->scan_v, V, (const u64 *)st->fdata, F, (const u64 *)st->rdata,
                       st->head);
    FP_CHECK_HIP(hipGetLastError());
    MsHead h;
    FP_CHECK_HIP(hipMemcpyAsync(&h, st->head, sizeof(h), hipMemcpyDeviceToHost, s));
    FP_CHECK_HIP(hipStreamSynchronize(s));
    float lo[3], hi[3];
    double extent = 0.0;
    for (int a = 0; a < 3; ++a) {
      const unsigned bl = bits_of(h.lo[a]), bh = bits_of(h.hi[a]);
      memcpy(&lo[a], &bl, 4), memcpy(&hi[a], &bh, 4);
      FP_REQUIRE(isfinite(lo[a]) && isfinite(hi[a]), "fp_mesh_simplify_count: the positions are not finite");
      extent = std::max(extent, (double)hi[a] - (double)lo[a]);
    }
    FP_REQUIRE(!(h.err & MS_ERR_DIM),
               "fp_mesh_simplify_count: cell %g cuts the bounding box (largest extent %g) into more than %d cells along an axis; a cell of %.9g fits",
               (double)cell, extent, MS_MAX_DIM, extent / MS_MAX_DIM * 1.001);
    FP_REQUIRE(!(h.err & MS_ERR_FACE), "fp_mesh_simplify_count: a face names a vertex outside 0 .. %d", V - 1);
    // the fixed-point sums of a cluster stay inside int64: extent * 2^30 * V < 2^62
    FP_REQUIRE(extent * MS_FIX * (double)V < 4611686018427387904.0, "fp_mesh_simplify_count: a bounding box of extent %g with %d vertices overflows the 2^-30 fixed point",
               extent, V);
    st->nv = (long long)h.total[2];
    st->nf = (long long)h.total[1];
  } else {
    FP_CHECK_HIP(hipStreamSynchronize(s));
    st->nv = st->nf = 0;
  }
  st->pos = d_pos, st->faces = d_faces, st->V = V, st->F = F, st->cell = cell;
  st->valid = true;
  h_counts[0] = st->nv;
  h_counts[1] = st->nf;
  return FP_OK;
}

extern "C" int fp_mesh_simplify_write(fp_ctx *ctx, const float *d_pos, const float *d_normals, const uint8_t *d_colors, int V, const int32_t *d_faces,
                                      int F, float cell, float *d_out_pos, float *d_out_normals, uint8_t *d_out_colors, int32_t *d_out_faces,
                                      int32_t *d_out_vertex_map, int64_t n_vertices, int64_t n_faces, void *stream) {
  FP_REQUIRE(ctx, "fp_mesh_simplify_write: null argument");
  const fp_simplify_state *cs = ctx->simplify;
  FP_REQUIRE(cs && cs->valid, "fp_mesh_simplify_write: no fp_mesh_simplify_count before it");
  FP_REQUIRE(cs->pos == d_pos && cs->faces == d_faces && cs->V == V && cs->F == F,
             "fp_mesh_simplify_write: not the mesh of the last fp_mesh_simplify_count (%d vertices, %d faces counted)", cs->V, cs->F);
  FP_REQUIRE(memcmp(&cs->cell, &cell, sizeof(float)) == 0, "fp_mesh_simplify_write: cell %g, the last fp_mesh_simplify_count had %g", (double)cell,
             (double)cs->cell);
  FP_REQUIRE(n_vertices == cs->nv && n_faces == cs->nf, "fp_mesh_simplify_write: %lld vertices, %lld faces given, %lld and %lld counted",
             (long long)n_vertices, (long long)n_faces, cs->nv, cs->nf);
  FP_REQUIRE((d_out_pos || n_vertices == 0) && (d_out_faces || n_faces == 0), "fp_mesh_simplify_write: d_out_pos or d_out_faces is null");
  FP_REQUIRE((d_normals || !d_out_normals) && (d_colors || !d_out_colors), "fp_mesh_simplify_write: an output attribute without its input");
  if (V == 0) return FP_OK;
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  fp_simplify_state *st = ctx->simplify;
  hipStream_t s = (hipStream_t)stream;
  const float *nrm = d_out_normals ? d_normals : nullptr;
  const uint8_t *col = d_out_colors ? d_colors : nullptr;
  const u64 *rdata = F > 0 ? st->rdata : nullptr;
  const size_t acc_bytes = (size_t)n_vertices * 64, need = acc_bytes + (size_t)n_vertices * 16;
  FP_TRY(st->acc.ensure(need, "fp_mesh_simplify_write", "the sums"));
  u64 *acc = st->acc.at<u64>(0);
  unsigned *cacc = st->acc.at<unsigned>(acc_bytes);
  if (n_vertices > 0 || d_out_vertex_map) {
    if (need) FP_CHECK_HIP(hipMemsetAsync(acc, 0, need, s));
    hipLaunchKernelGGL(ms_accumulate_kernel, grid_for(V), dim3(MS_THREADS), 0, s, d_pos, nrm, col, V, (const MsHead *)st->head, (const int *)st->cid,
                       rdata, acc, cacc, d_out_vertex_map);
    FP_CHECK_HIP(hipGetLastError());
  }
  if (n_vertices > 0) {
    hipLaunchKernelGGL(ms_vertex_write_kernel, grid_for(V), dim3(MS_THREADS), 0, s, d_pos, nrm, col, V, (const MsHead *)st->head,
                       (const u64 *)st->scan_v, rdata, (const u64 *)acc, (const unsigned *)cacc, d_out_pos, d_out_normals, d_out_colors);
    FP_CHECK_HIP(hipGetLastError());
  }
  if (n_faces > 0) {
    hipLaunchKernelGGL(ms_face_write_kernel, grid_for(F), dim3(MS_THREADS), 0, s, d_faces, F, (const int *)st->cid, (const u64 *)st->fdata,
                       (const u64 *)st->rdata, d_out_faces);
    FP_CHECK_HIP(hipGetLastError());
  }
  return FP_OK;
}
