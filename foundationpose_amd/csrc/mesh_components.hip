// Connected components of a triangle list, selection and order-preserving compaction (fp_mesh_components_count / _write).  The rule is
// stated in include/foundationpose_amd.h and restated in numpy by tests/mesh_components_oracle.py.
//
// Everything written out is a function of the input alone, whatever order the lanes run in:
//   * the components come from the lock-free union-find of union_find.h over parent[V] in global memory, started from singletons; the
//     invariants and the termination arguments are written there.  The root a component ends with is its lowest vertex index;
//   * one flatten pass then makes parent[v] that lowest index for every vertex: the label;
//   * components are numbered by an exclusive scan over "v is its own label" (scan_exclusive, scan.hip), as fp_mesh_simplify numbers
//     its clusters; kept vertices and kept faces are numbered by two more scans, so both keep their input order;
//   * the per-component counts are int32 atomic adds and the largest count an atomicMax: exact, so the order does not matter.  The
//     lowest-numbered component among those of the largest count is an atomicMin over their labels.
// One launch of hooks, one of compression; no host loop.
//
// All kernels are one thread per vertex or face.  The hooks are scattered 4-byte atomics, which execute at the memory side: the pass is
// bound by atomic requests, not by bytes.  The counts of a mesh that is ONE component would be F adds to one address; a wave whose
// active lanes all name the same label adds their number once instead (wave_add_one).
#include "common.h"
#include "device_util.h"
#include "union_find.h"

#include <math.h>
#include <algorithm>

typedef unsigned long long u64;

namespace {

constexpr int CC_THREADS = 256;

struct CcHead {
  int err;          // a face named a vertex outside 0 .. V-1
  int max_faces;    // M: the largest n_faces of a component
  int best;         // the lowest label among the components with M faces (largest_only)
  int kept;         // kept components
  u64 total[3];     // components, kept vertices, kept faces
};

struct CcRule {
  int min_faces, largest_only;
  float min_fraction;
};

__device__ __forceinline__ bool cc_kept(int n_faces, int label, const CcHead *head, CcRule rule) {
  const bool cand = n_faces >= 1 && n_faces >= rule.min_faces && (double)n_faces >= (double)rule.min_fraction * (double)head->max_faces;
  return cand && (!rule.largest_only || label == head->best);
}

__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(int V, int *__restrict__ parent, int *__restrict__ cnt) {
  const int v = blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= V) return;
  parent[v] = v;
  cnt[2 * (size_t)v] = 0, cnt[2 * (size_t)v + 1] = 0;
}

// one thread per face: a-b and b-c.  A face with an index outside 0 .. V-1 raises the error and is not followed
__global__ __launch_bounds__(CC_THREADS) void cc_hook_kernel(const int32_t *__restrict__ faces, int F, int V, int *parent, CcHead *__restrict__ head) {
  const int f = blockIdx.x * CC_THREADS + threadIdx.x;
  if (f >= F) return;
  const int a = faces[(size_t)f * 3], b = faces[(size_t)f * 3 + 1], c = faces[(size_t)f * 3 + 2];
  if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) {
    atomicOr(&head->err, 1);
    return;
  }
  if (a != b) cc_unite(parent, a, b);
  if (b != c) cc_unite(parent, b, c);
}

// parent[v] becomes the lowest index of v's component (the roots are final: the hooks have all run); data[v] = 1 where v is that
// lowest index, data[V] = 0 closes the scan; cnt[2 r] counts the vertices of the component of label r.
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int V, int *parent, int *__restrict__ cnt, u64 *__restrict__ data) {
  const int v = blockIdx.x * CC_THREADS + threadIdx.x;
  int r = -1;
  if (v < V) {
    r = cc_root(parent, v);
    __hip_atomic_store(&parent[v], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (v <= V) data[v] = v < V && r == v ? 1 : 0;
  wave_add_one(cnt, 2 * r, v < V);
}

// a face belongs to the component of its first vertex
__global__ __launch_bounds__(CC_THREADS) void cc_face_count_kernel(const int32_t *__restrict__ faces, int F, int V, const int *__restrict__ label,
                                                                   int *__restrict__ cnt) {
  const int f = blockIdx.x * CC_THREADS + threadIdx.x;
  int r = 0;
  bool on = false;
  if (f < F) {
    const int a = faces[(size_t)f * 3];
    on = (unsigned)a < (unsigned)V;       // a bad face is an error of the call (cc_hook_kernel); never followed
    if (on) r = label[a];
  }
  wave_add_one(cnt, 2 * r + 1, on);
}

__global__ __launch_bounds__(CC_THREADS) void cc_max_kernel(int V, const int *__restrict__ label, const int *__restrict__ cnt, CcHead *head) {
  const int v = blockIdx.x * CC_THREADS + threadIdx.x;
  const int m = wave_max(v < V && label[v] == v ? cnt[2 * (size_t)v + 1] : 0);
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&head->max_faces, m);
}

__global__ __launch_bounds__(CC_THREADS) void cc_best_kernel(int V, const int *__restrict__ label, const int *__restrict__ cnt, CcHead *head) {
  const int v = blockIdx.x * CC_THREADS + threadIdx.x;
  const int b = wave_min(v < V && label[v] == v && cnt[2 * (size_t)v + 1] == head->max_faces ? v : 0x7fffffff);
  if ((threadIdx.x & 63) == 0 && b != 0x7fffffff) atomicMin(&head->best, b);
}

// vdata[v] = 1 for a vertex of a kept component; vdata[V] = 0
__global__ __launch_bounds__(CC_THREADS) void cc_vertex_flag_kernel(int V, const int *__restrict__ label, const int *__restrict__ cnt, CcHead *head,
                                                                    CcRule rule, u64 *__restrict__ vdata) {
  const int v = blockIdx.x * CC_THREADS + threadIdx.x;
  bool keep = false;
  int root = 0;
  if (v < V) {
    const int r = label[v];
    keep = cc_kept(cnt[2 * (size_t)r + 1], r, head, rule);
    root = keep && r == v ? 1 : 0;
  }
  if (v <= V) vdata[v] = keep ? 1 : 0;
  root = wave_sum(root);
  if ((threadIdx.x & 63) == 0 && root > 0) atomicAdd(&head->kept, root);
}

// fdata[f] = 1 for a face of a kept component; vdata still holds the flags here: its scan comes after
__global__ __launch_bounds__(CC_THREADS) void cc_face_flag_kernel(const int32_t *__restrict__ faces, int F, int V, const u64 *__restrict__ vdata,
                                                                  u64 *__restrict__ fdata) {
  const int f = blockIdx.x * CC_THREADS + threadIdx.x;
  if (f > F) return;
  const int a = f < F ? faces[(size_t)f * 3] : -1;
  fdata[f] = (unsigned)a < (unsigned)V ? vdata[a] : 0;
}

__global__ void cc_totals_kernel(const u64 *scan_v, const u64 *vdata, int V, const u64 *fdata, int F, CcHead *head) {
  head->total[0] = scan_v[V];
  head->total[1] = vdata[V];
  head->total[2] = F > 0 ? fdata[F] : 0;
}

__global__ __launch_bounds__(CC_THREADS) void cc_vertex_write_kernel(const float *__restrict__ pos, const float *__restrict__ nrm,
                                                                     const uint8_t *__restrict__ col, int V, const int *__restrict__ label,
                                                                     const int *__restrict__ cnt, const u64 *__restrict__ scan_v,
                                                                     const u64 *__restrict__ vdata, float *__restrict__ out_pos,
                                                                     float *__restrict__ out_nrm, uint8_t *__restrict__ out_col,
                                                                     int32_t *__restrict__ vmap, int32_t *__restrict__ out_label,
                                                                     int32_t *__restrict__ out_stats) {
  const int v = blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= V) return;
  const int r = label[v];
  if (out_label) out_label[v] = r;
  if (out_stats && r == v) {
    const size_t c = (size_t)scan_v[v];
    out_stats[2 * c] = cnt[2 * (size_t)v], out_stats[2 * c + 1] = cnt[2 * (size_t)v + 1];
  }
  const u64 o = vdata[v];
  const bool kept = vdata[v + 1] != o;
  if (vmap) vmap[v] = kept ? (int32_t)o : -1;
  if (!kept) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (out_pos) out_pos[(size_t)o * 3 + a] = pos[(size_t)v * 3 + a];
    if (out_nrm) out_nrm[(size_t)o * 3 + a] = nrm[(size_t)v * 3 + a];
    if (out_col) out_col[(size_t)o * 3 + a] = col[(size_t)v * 3 + a];
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_face_write_kernel(const int32_t *__restrict__ faces, int F, const u64 *__restrict__ vdata,
                                                                   const u64 *__restrict__ fdata, int32_t *__restrict__ out_faces) {
  const int f = blockIdx.x * CC_THREADS + threadIdx.x;
  if (f >= F) return;
  const u64 o = fdata[f];
  if (fdata[f + 1] == o) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) out_faces[(size_t)o * 3 + k] = (int32_t)vdata[faces[(size_t)f * 3 + k]];      // a kept face's vertices are all kept
}

}  // namespace

// What fp_mesh_components_count leaves for fp_mesh_components_write: one allocation owned by the context, grown when a larger mesh arrives.
struct fp_components_state {
  DevBlob blob;
  // views into blob
  CcHead *head = nullptr;
  int *parent = nullptr, *cnt = nullptr;      // the label of every vertex; {n_vertices, n_faces} at the label of every component
  u64 *scan_v = nullptr, *vdata = nullptr, *fdata = nullptr, *sums = nullptr;
  // the counted call
  bool valid = false;
  const int32_t *faces = nullptr;
  int V = 0, F = 0;
  long long nc = 0, nv = 0, nf = 0;
};

void fp_components_state_free(fp_ctx *ctx) {
  fp_components_state *st = ctx->components;
  if (!st) return;
  st->blob.release();
  delete st;
  ctx->components = nullptr;
}

static int components_layout(fp_components_state *st, int V, int F) {
  const long long nscan = (long long)(V > F ? V : F) + 1;
  BlobLayout l;
  const size_t o_head = l.put(sizeof(CcHead)), o_parent = l.put((size_t)V * 4), o_cnt = l.put((size_t)V * 8), o_scan = l.put(((size_t)V + 1) * 8),
               o_vdata = l.put(((size_t)V + 1) * 8), o_fdata = l.put(((size_t)F + 1) * 8), o_sums = l.put(scan_sums_words(nscan) * 8);
  FP_TRY(st->blob.ensure(l.bytes, "fp_mesh_components_count", "the state"));
  const DevBlob &b = st->blob;
  st->head = b.at<CcHead>(o_head);
  st->parent = b.at<int>(o_parent), st->cnt = b.at<int>(o_cnt);
  st->scan_v = b.at<u64>(o_scan), st->vdata = b.at<u64>(o_vdata), st->fdata = b.at<u64>(o_fdata), st->sums = b.at<u64>(o_sums);
  return FP_OK;
}

extern "C" int fp_mesh_components_count(fp_ctx *ctx, const int32_t *d_faces, int F, int V, int min_faces, float min_fraction, int largest_only,
                                        int64_t *h_counts, void *stream) {
  FP_REQUIRE(ctx && h_counts, "fp_mesh_components_count: null argument");
  FP_REQUIRE(V >= 0 && V <= FP_MESH_COMPONENTS_MAX_VERTICES, "fp_mesh_components_count: V %d (0 .. %d)", V, FP_MESH_COMPONENTS_MAX_VERTICES);
  FP_REQUIRE(F >= 0 && F <= FP_MESH_COMPONENTS_MAX_FACES, "fp_mesh_components_count: F %d (0 .. %d)", F, FP_MESH_COMPONENTS_MAX_FACES);
  FP_REQUIRE(d_faces || F == 0, "fp_mesh_components_count: d_faces is null");
  FP_REQUIRE(V > 0 || F == 0, "fp_mesh_components_count: %d faces without a vertex", F);
  FP_REQUIRE(min_faces >= 1, "fp_mesh_components_count: min_faces %d (>= 1)", min_faces);
  FP_REQUIRE(min_fraction >= 0.f && min_fraction <= 1.f, "fp_mesh_components_count: min_fraction %g (0 .. 1)", (double)min_fraction);
  FP_REQUIRE(largest_only == 0 || largest_only == 1, "fp_mesh_components_count: largest_only %d (0 or 1)", largest_only);
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  if (!ctx->components) ctx->components = new fp_components_state;
  fp_components_state *st = ctx->components;
  st->valid = false;
  hipStream_t s = (hipStream_t)stream;
  if (V > 0) {
    FP_TRY(components_layout(st, V, F));
    const CcRule rule{min_faces, largest_only, min_fraction};
    FP_CHECK_HIP(hipMemsetAsync(st->head, 0, sizeof(CcHead), s));
    FP_CHECK_HIP(hipMemsetAsync(&st->head->best, 0x7f, sizeof(int), s));      // above every vertex index
    hipLaunchKernelGGL(cc_init_kernel, grid_for(V), dim3(CC_THREADS), 0, s, V, st->parent, st->cnt);
    FP_CHECK_HIP(hipGetLastError());
    if (F > 0) {
      hipLaunchKernelGGL(cc_hook_kernel, grid_for(F), dim3(CC_THREADS), 0, s, d_faces, F, V, st->parent, st->head);
      FP_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(cc_flatten_kernel, grid_for((long long)V + 1), dim3(CC_THREADS), 0, s, V, st->parent, st->cnt, st->scan_v);
    FP_CHECK_HIP(hipGetLastError());
    FP_TRY(scan_exclusive(st->scan_v, (long long)V + 1, st->sums, s));
    if (F > 0) {
      hipLaunchKernelGGL(cc_face_count_kernel, grid_for(F), dim3(CC_THREADS), 0, s, d_faces, F, V, (const int *)st->parent, st->cnt);
      FP_CHECK_HIP(hipGetLastError());
      hipLaunchKernelGGL(cc_max_kernel, grid_for(V), dim3(CC_THREADS), 0, s, V, (const int *)st->parent, (const int *)st->cnt, st->head);
      FP_CHECK_HIP(hipGetLastError());
      if (largest_only) {
        hipLaunchKernelGGL(cc_best_kernel, grid_for(V), dim3(CC_THREADS), 0, s, V, (const int *)st->parent, (const int *)st->cnt, st->head);
        FP_CHECK_HIP(hipGetLastError());
      }
    }
    // without a face no component has one: nothing is kept, and the flags say so without M
    hipLaunchKernelGGL(cc_vertex_flag_kernel, grid_for((long long)V + 1), dim3(CC_THREADS), 0, s, V, (const int *)st->parent, (const int *)st->cnt,
                       st->head, rule, st->vdata);
    FP_CHECK_HIP(hipGetLastError());
    if (F > 0) {
      hipLaunchKernelGGL(cc_face_flag_kernel, grid_for((long long)F + 1), dim3(CC_THREADS), 0, s, d_faces, F, V, (const u64 *)st->vdata, st->fdata);
      FP_CHECK_HIP(hipGetLastError());
      FP_TRY(scan_exclusive(st->fdata, (long long)F + 1, st->sums, s));
    }
    FP_TRY(scan_exclusive(st->vdata, (long long)V + 1, st->sums, s));
    hipLaunchKernelGGL(cc_totals_kernel, dim3(1), dim3(1), 0, s, (const u64 *)st->scan_v, (const u64 *)st->vdata, V, (const u64 *)st->fdata, F,
                       st->head);
    FP_CHECK_HIP(hipGetLastError());
    CcHead h;
    FP_CHECK_HIP(hipMemcpyAsync(&h, st->head, sizeof(h), hipMemcpyDeviceToHost, s));
    FP_CHECK_HIP(hipStreamSynchronize(s));
    FP_REQUIRE(!h.err, "fp_mesh_components_count: a face names a vertex outside 0 .. %d", V - 1);
    st->nc = (long long)h.total[0], st->nv = (long long)h.total[1], st->nf = (long long)h.total[2];
    h_counts[1] = h.kept;
  } else {
    FP_CHECK_HIP(hipStreamSynchronize(s));
    st->nc = st->nv = st->nf = 0;
    h_counts[1] = 0;
  }
  st->faces = d_faces, st->V = V, st->F = F;
  st->valid = true;
  h_counts[0] = st->nc;
  h_counts[2] = st->nv;
  h_counts[3] = st->nf;
  return FP_OK;
}

extern "C" int fp_mesh_components_write(fp_ctx *ctx, const float *d_pos, const float *d_normals, const uint8_t *d_colors, int V, const int32_t *d_faces,
                                        int F, float *d_out_pos, float *d_out_normals, uint8_t *d_out_colors, int32_t *d_out_faces,
                                        int32_t *d_out_vertex_map, int32_t *d_out_label, int32_t *d_out_stats, int64_t n_vertices, int64_t n_faces,
                                        void *stream) {
  FP_REQUIRE(ctx, "fp_mesh_components_write: null argument");
  const fp_components_state *st = ctx->components;
  FP_REQUIRE(st && st->valid, "fp_mesh_components_write: no fp_mesh_components_count before it");
  FP_REQUIRE(st->faces == d_faces && st->V == V && st->F == F,
             "fp_mesh_components_write: not the mesh of the last fp_mesh_components_count (%d vertices, %d faces counted)", st->V, st->F);
  FP_REQUIRE(n_vertices == st->nv && n_faces == st->nf, "fp_mesh_components_write: %lld vertices, %lld faces given, %lld and %lld counted",
             (long long)n_vertices, (long long)n_faces, st->nv, st->nf);
  FP_REQUIRE((d_out_pos || n_vertices == 0) && (d_out_faces || n_faces == 0), "fp_mesh_components_write: d_out_pos or d_out_faces is null");
  FP_REQUIRE(d_pos || n_vertices == 0, "fp_mesh_components_write: d_pos is null");
  FP_REQUIRE((d_normals || !d_out_normals) && (d_colors || !d_out_colors), "fp_mesh_components_write: an output attribute without its input");
  if (V == 0) return FP_OK;
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const bool copy = n_vertices > 0;
  if (copy || d_out_vertex_map || d_out_label || d_out_stats) {
    hipLaunchKernelGGL(cc_vertex_write_kernel, grid_for(V), dim3(CC_THREADS), 0, s, d_pos, d_out_normals ? d_normals : nullptr,
                       d_out_colors ? d_colors : nullptr, V, (const int *)st->parent, (const int *)st->cnt, (const u64 *)st->scan_v,
                       (const u64 *)st->vdata, copy ? d_out_pos : nullptr, copy ? d_out_normals : nullptr, copy ? d_out_colors : nullptr,
                       d_out_vertex_map, d_out_label, d_out_stats);
    FP_CHECK_HIP(hipGetLastError());
  }
  if (n_faces > 0) {
    hipLaunchKernelGGL(cc_face_write_kernel, grid_for(F), dim3(CC_THREADS), 0, s, d_faces, F, (const u64 *)st->vdata, (const u64 *)st->fdata, d_out_faces);
    FP_CHECK_HIP(hipGetLastError());
  }
  return FP_OK;
}
