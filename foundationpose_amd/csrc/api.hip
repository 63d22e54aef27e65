// extern "C" entry points of libfoundationpose_amd (see include/foundationpose_amd.h).
#include "common.h"
#include <memory>
#include <cstring>

#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <algorithm>

static thread_local char g_err[1024] = "";

void fp_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char *fp_last_error(void) { return g_err; }
extern "C" int fp_version(void) { return 102; }

// ---- context / arena ---------------------------------------------------------------------------
size_t fp_arena_bytes_for(int n_hyp) {
  // per hypothesis: net input 0.82 MB (x2 sides) + the forward's buffers (fp_arena_inner_bytes)
  return (size_t)n_hyp * (size_t)(17u << 20) + ((size_t)64 << 20);
}

size_t fp_arena_inner_bytes(int n_hyp) {
  // exact sum of the forward's buffers is 11,485,184 B per hypothesis (DESIGN.md "HBM layout")
  // + 2.9 MB per hypothesis for the second transformer head's buffers (the two heads of RefineNet run side by side)
  return (size_t)n_hyp * (size_t)(15u << 20) + ((size_t)8 << 20) + (n_hyp <= 4 ? ((size_t)40 << 20) : 0);   // + split-K scratch (1 .. 4 hypotheses)
}

int fp_arena_ensure(fp_ctx *ctx, size_t bytes) {
  Arena &a = ctx->arena;
  if (a.cap - a.off >= bytes && a.base) return FP_OK;
  if (a.off != 0) {
    fp_set_error("arena too small for a nested request of %zu bytes (cap %zu, used %zu); call fp_ctx_reserve first", bytes, a.cap, a.off);
    return FP_ENOMEM;
  }
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  if (a.base) {
    FP_CHECK_HIP(hipDeviceSynchronize());
    FP_CHECK_HIP(hipFree(a.base));
    a.base = nullptr;
    a.cap = 0;
  }
  void *p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    fp_set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return FP_ENOMEM;
  }
  a.base = (char *)p;
  a.cap = bytes;
  a.off = 0;
  ++a.generation;
  return FP_OK;
}

int fp_set_kernel_attributes(fp_ctx *ctx) {
  std::vector<KernelLds> v;
  conv_kernel_lds(v), conv_halo_kernel_lds(v), conv_s1b_kernel_lds(v), conv_small_kernel_lds(v), conv_s2_kernel_lds(v), stem_kernel_lds(v), front_kernel_lds(v);
  tok_gemm_kernel_lds(v), tok_qkv_kernel_lds(v), head_mlp_kernel_lds(v), attn_kernel_lds(v), raster_kernel_lds(v);
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  for (const KernelLds &k : v)
    if (k.bytes > 48 * 1024) FP_CHECK_HIP(hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes));
  return FP_OK;
}

extern "C" int fp_ctx_create(int device, fp_ctx **out) {
  FP_REQUIRE(out, "fp_ctx_create: null out");
  int n = 0;
  FP_CHECK_HIP(hipGetDeviceCount(&n));
  FP_REQUIRE(device >= 0 && device < n, "fp_ctx_create: device %d out of range (%d visible)", device, n);
  FP_CHECK_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  FP_CHECK_HIP(hipGetDeviceProperties(&prop, device));
  fp_ctx *c = new fp_ctx;
  c->device = device;
  c->num_cu = prop.multiProcessorCount;
  // one allocation: the 4-KB zero page, then the score tail's arrival counters (zeros as well)
  if (hipMalloc(&c->zero_page, 4096 + FP_TAIL_MAX_GROUPS * sizeof(int)) != hipSuccess ||
      hipMemset(c->zero_page, 0, 4096 + FP_TAIL_MAX_GROUPS * sizeof(int)) != hipSuccess) {
    delete c;
    fp_set_error("fp_ctx_create: zero page allocation failed");
    return FP_ENOMEM;
  }
  c->tail_counter = (int *)((char *)c->zero_page + 4096);
  const int rc = fp_set_kernel_attributes(c);      // per device: every kernel of the library that needs more than 64 KB of LDS
  if (rc != FP_OK) {
    (void)hipFree(c->zero_page);
    delete c;
    return rc;
  }
  *out = c;
  return FP_OK;
}

extern "C" int fp_ctx_destroy(fp_ctx *ctx) {
  if (!ctx) return FP_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  for (auto &e : ctx->pending) {
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
  for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
  if (ctx->ev_ref) (void)hipEventDestroy(ctx->ev_ref);
  if (ctx->side_ready) {
    for (int i = 0; i < fp_ctx::NSIDE; ++i) {
      (void)hipStreamDestroy(ctx->side[i]);
      (void)hipEventDestroy(ctx->ev_join[i]);
    }
    (void)hipEventDestroy(ctx->ev_fork);
  }
  fp_simplify_state_free(ctx);
  fp_components_state_free(ctx);
  fp_segment_state_free(ctx);
  fp_stereo_state_free(ctx);
  if (ctx->arena.base) (void)hipFree(ctx->arena.base);
  if (ctx->zero_page) (void)hipFree(ctx->zero_page);
  delete ctx;
  return FP_OK;
}

extern "C" int fp_ctx_arena_generation(const fp_ctx *ctx) { return ctx ? ctx->arena.generation : -1; }

extern "C" int fp_ctx_reserve(fp_ctx *ctx, int max_hyp) {
  FP_REQUIRE(ctx && max_hyp >= 1, "fp_ctx_reserve: bad argument");
  FP_REQUIRE(ctx->arena.off == 0, "fp_ctx_reserve: arena in use");
  size_t need = fp_arena_bytes_for(max_hyp);
  if (ctx->arena.cap >= need) return FP_OK;
  FP_TRY(fp_arena_ensure(ctx, need));          // (off == 0 and cap < need: it frees the old block and allocates)
  ctx->reserved_hyp = max_hyp;
  return FP_OK;
}

// ---- profiling ---------------------------------------------------------------------------------
static int prof_drain(fp_ctx *ctx);

extern "C" int fp_prof_enable(fp_ctx *ctx, int on) {
  FP_REQUIRE(ctx, "fp_prof_enable: null ctx");
  ctx->prof = on < 0 ? 0 : (on > 2 ? 2 : on);
  if (ctx->prof) {                            // the time origin of the launch spans (fp_prof_read_busy), renewed whenever profiling is
    FP_TRY(prof_drain(ctx));                  // switched on: the spans are float32 milliseconds since then
    if (!ctx->ev_ref) FP_CHECK_HIP(hipEventCreate(&ctx->ev_ref));
    FP_CHECK_HIP(hipEventRecord(ctx->ev_ref, nullptr));
    FP_CHECK_HIP(hipEventSynchronize(ctx->ev_ref));
  }
  return FP_OK;
}

static int prof_drain(fp_ctx *ctx) {
  for (auto &e : ctx->pending) {
    FP_CHECK_HIP(hipEventSynchronize(e.b));
    float ms = 0.f, t0 = 0.f;
    FP_CHECK_HIP(hipEventElapsedTime(&ms, e.a, e.b));
    ProfEntry &p = ctx->prof_tab[e.cls];
    if (ctx->ev_ref && hipEventElapsedTime(&t0, ctx->ev_ref, e.a) == hipSuccess) p.spans.emplace_back(t0, t0 + ms);
    p.total_ms += ms;
    p.flops += e.flops;
    p.launches += 1;
    ctx->ev_pool.push_back(e.a);
    ctx->ev_pool.push_back(e.b);
  }
  ctx->pending.clear();
  return FP_OK;
}

extern "C" int fp_prof_read(fp_ctx *ctx, const char *cls, double *total_ms, int64_t *launches, double *flops) {
  FP_REQUIRE(ctx && cls, "fp_prof_read: null argument");
  FP_TRY(prof_drain(ctx));
  auto it = ctx->prof_tab.find(cls);
  ProfEntry e = (it == ctx->prof_tab.end()) ? ProfEntry() : it->second;
  if (total_ms) *total_ms = e.total_ms;
  if (launches) *launches = e.launches;
  if (flops) *flops = e.flops;
  return FP_OK;
}

// Time during which AT LEAST ONE launch of the class was executing (the union of the launch spans): equal to total_ms when the
// launches follow one another, smaller when launches of the class overlap - the two half-batch trunks on two streams, the two
// RefineNet heads.  FLOPs / busy time is the rate the chip sustains on the class.
extern "C" int fp_prof_read_busy(fp_ctx *ctx, const char *cls, double *busy_ms) {
  FP_REQUIRE(ctx && cls && busy_ms, "fp_prof_read_busy: null argument");
  FP_TRY(prof_drain(ctx));
  *busy_ms = 0.0;
  auto it = ctx->prof_tab.find(cls);
  if (it == ctx->prof_tab.end()) return FP_OK;
  std::vector<std::pair<float, float>> v = it->second.spans;
  std::sort(v.begin(), v.end());
  double busy = 0.0;
  float cur_a = 0.f, cur_b = -1.f;
  for (const auto &sp : v) {
    if (cur_b < cur_a || sp.first > cur_b) {
      if (cur_b >= cur_a) busy += cur_b - cur_a;
      cur_a = sp.first;
      cur_b = sp.second;
    } else if (sp.second > cur_b) {
      cur_b = sp.second;
    }
  }
  if (cur_b >= cur_a) busy += cur_b - cur_a;
  *busy_ms = busy;
  return FP_OK;
}

extern "C" int fp_prof_reset(fp_ctx *ctx) {
  FP_REQUIRE(ctx, "fp_prof_reset: null ctx");
  FP_TRY(prof_drain(ctx));
  ctx->prof_tab.clear();
  return FP_OK;
}

// ---- mesh --------------------------------------------------------------------------------------
template <typename T>
static int up(fp_mesh *m, const T *h, size_t n, const T **d) {
  void *p = nullptr;
  FP_CHECK_HIP(hipMalloc(&p, n * sizeof(T)));
  m->allocs.push_back(p);
  FP_CHECK_HIP(hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice));
  *d = (const T *)p;
  return FP_OK;
}

extern "C" int fp_mesh_create(fp_ctx *ctx, const float *h_pos, int V, const int32_t *h_faces, int F, const float *h_vnormals,
                              const float *h_vertex_color, const float *h_uv, int n_uv, const int32_t *h_uv_idx, const float *h_tex,
                              int texH, int texW, fp_mesh **out) {
  FP_REQUIRE(ctx && h_pos && h_faces && h_vnormals && out, "fp_mesh_create: null argument");
  FP_REQUIRE(V > 0 && F > 0, "fp_mesh_create: empty mesh (V=%d F=%d)", V, F);
  FP_REQUIRE(h_vertex_color || (h_uv && h_uv_idx && h_tex && texH > 0 && texW > 0 && n_uv > 0),
             "fp_mesh_create: need vertex colours or (uv, uv_idx, tex)");
  for (int i = 0; i < F * 3; ++i) FP_REQUIRE(h_faces[i] >= 0 && h_faces[i] < V, "fp_mesh_create: face index %d out of range", h_faces[i]);
  const bool textured = (h_tex != nullptr && h_vertex_color == nullptr);
  if (textured)
    for (int i = 0; i < F * 3; ++i) FP_REQUIRE(h_uv_idx[i] >= 0 && h_uv_idx[i] < n_uv, "fp_mesh_create: uv index out of range");
  FP_CHECK_HIP(hipSetDevice(ctx->device));
  fp_mesh *m = new fp_mesh;
  memset(&m->d, 0, sizeof(MeshDev));
  m->d.V = V;
  m->d.F = F;
  int rc = FP_OK;
  auto run = [&]() -> int {
    FP_TRY(up(m, h_pos, (size_t)V * 3, &m->d.pos));
    FP_TRY(up(m, h_faces, (size_t)F * 3, &m->d.faces));
    {
      std::vector<int4> f4(F);
      for (int t = 0; t < F; ++t) f4[t] = make_int4(h_faces[t * 3], h_faces[t * 3 + 1], h_faces[t * 3 + 2], 0);
      FP_TRY(up(m, f4.data(), (size_t)F, &m->d.faces4));
    }
    FP_TRY(up(m, h_vnormals, (size_t)V * 3, &m->d.vnormals));
    if (textured) {
      FP_TRY(up(m, h_uv, (size_t)n_uv * 2, &m->d.uv));
      FP_TRY(up(m, h_uv_idx, (size_t)F * 3, &m->d.uv_idx));
      FP_TRY(up(m, h_tex, (size_t)texH * texW * 3, &m->d.tex));
      m->d.texH = texH;
      m->d.texW = texW;
    } else {
      FP_TRY(up(m, h_vertex_color, (size_t)V * 3, &m->d.vcolor));
    }
    return FP_OK;
  };
  rc = run();
  if (rc != FP_OK) {
    for (void *p : m->allocs) (void)hipFree(p);
    delete m;
    return rc;
  }
  *out = m;
  return FP_OK;
}

extern "C" int fp_mesh_destroy(fp_mesh *m) {
  if (!m) return FP_OK;
  for (void *p : m->allocs) (void)hipFree(p);
  delete m;
  return FP_OK;
}

// ---- render / crops ------------------------------------------------------------------------------
extern "C" int fp_crop_window_tf(fp_ctx *ctx, const float *d_poses, int N, const double *K, double crop_ratio, double mesh_diameter,
                                 int out_w, int out_h, float *d_tf, float *d_bbox2d, void *stream) {
  FP_REQUIRE(ctx && d_poses && K && d_tf, "fp_crop_window_tf: null argument");
  FP_REQUIRE(N >= 0 && out_w > 0 && out_h > 0 && mesh_diameter > 0 && crop_ratio > 0, "fp_crop_window_tf: bad argument");
  return launch_crop_window_tf(d_poses, N, K, crop_ratio, mesh_diameter, out_w, out_h, d_tf, d_bbox2d, (hipStream_t)stream);
}

// A render called on its own (the nvdiffrast_render API, fp_render_net): its scratch (transformed vertices + strip face lists) comes
// from the context's arena and is released when the launches are queued - the next taker runs behind them on the same stream.
static int render_with_arena_scratch(fp_ctx *ctx, RenderArgs &a, hipStream_t s) {
  if (a.N == 0) return FP_OK;
  const size_t bytes = render_scratch_bytes(a.N, a.mesh.V, a.mesh.F, a.Ho, a.Wo, ctx->num_cu);     // (sub-batches above 1 GiB: launch_render)
  FP_TRY(fp_arena_ensure(ctx, bytes + 4096));
  ArenaScope scope(ctx->arena);
  a.scratch = ctx->arena.take(bytes);
  a.scratch_bytes = bytes;
  return a.scratch ? launch_render(ctx, a, s) : FP_ENOMEM;
}

static int fill_render(RenderArgs &a, const fp_mesh *mesh, const float *d_poses, int N, const double *K, int H, int W,
                       const float *d_bbox2d, int out_h, int out_w) {
  FP_REQUIRE(mesh && K && (d_poses || N == 0), "render: null argument");
  FP_REQUIRE(N >= 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0, "render: bad shape");
  memset(&a, 0, sizeof(a));
  a.mesh = mesh->d;
  a.poses = d_poses;
  a.bbox2d = d_bbox2d;
  for (int i = 0; i < 9; ++i) a.K[i] = K[i];
  a.N = N;
  a.H = H;
  a.W = W;
  a.Ho = out_h;
  a.Wo = out_w;
  return FP_OK;
}

extern "C" int fp_render(fp_ctx *ctx, const fp_mesh *mesh, const float *d_poses, int N, const double *K, int H, int W,
                         const float *d_bbox2d, int out_h, int out_w, int use_light, float w_ambient, float w_diffuse, float *d_color,
                         float *d_depth, float *d_normal, float *d_xyz, void *stream) {
  FP_REQUIRE(ctx, "fp_render: null ctx");
  RenderArgs a;
  FP_TRY(fill_render(a, mesh, d_poses, N, K, H, W, d_bbox2d, out_h, out_w));
  a.use_light = use_light;
  a.w_ambient = w_ambient;
  a.w_diffuse = w_diffuse;
  a.color = d_color;
  a.depth = d_depth;
  a.normal = d_normal;
  a.xyz = d_xyz;
  return render_with_arena_scratch(ctx, a, (hipStream_t)stream);
}

extern "C" int fp_render_ex(fp_ctx *ctx, const fp_mesh *mesh, const float *d_poses, int N, const double *K, int H, int W,
                            const float *d_bbox2d, int out_h, int out_w, const fp_render_opts *opts_in, float *d_color, float *d_depth,
                            float *d_normal, float *d_xyz, void *stream) {
  FP_REQUIRE(ctx, "fp_render_ex: null ctx");
  if (!opts_in) return fp_render(ctx, mesh, d_poses, N, K, H, W, d_bbox2d, out_h, out_w, 0, 0.8f, 0.5f, d_color, d_depth, d_normal, d_xyz, stream);
  // versioned by size: a caller built against the header before `d_rast` passes a shorter struct - never read past what it holds
  fp_render_opts o;
  memset(&o, 0, sizeof(o));
  {
    const size_t sz = opts_in->struct_size, sz_r4 = offsetof(fp_render_opts, d_rast);
    FP_REQUIRE(sz == sizeof(fp_render_opts) || sz == sz_r4, "fp_render_ex: fp_render_opts.struct_size = %zu (this library knows %zu and %zu)", sz, sz_r4, sizeof(fp_render_opts));
    memcpy(&o, opts_in, sz);
  }
  const fp_render_opts *opts = &o;
  FP_REQUIRE(opts->light_mode >= 0 && opts->light_mode <= 2, "fp_render_ex: light_mode %d unknown", opts->light_mode);
  static const double unit_k[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  FP_REQUIRE(K || opts->has_projection, "fp_render_ex: neither K nor a projection matrix");
  RenderArgs a;
  FP_TRY(fill_render(a, mesh, d_poses, N, K ? K : unit_k, H, W, d_bbox2d, out_h, out_w));
  a.use_light = opts->use_light;
  a.w_ambient = opts->w_ambient;
  a.w_diffuse = opts->w_diffuse;
  a.light_mode = opts->light_mode;
  a.has_light_color = opts->has_light_color;
  for (int c = 0; c < 3; ++c) a.light_vec[c] = opts->light_vec[c], a.light_color[c] = opts->light_color[c];
  a.has_proj = opts->has_projection;
  for (int i = 0; i < 16; ++i) a.proj[i] = opts->projection[i];
  a.color = d_color;
  a.depth = d_depth;
  a.normal = d_normal;
  a.xyz = d_xyz;
  a.rast = opts->d_rast;
  return render_with_arena_scratch(ctx, a, (hipStream_t)stream);
}

// scratch: render_scratch_bytes(N, ...) bytes for the vertex pre-pass and the strip face lists (nullptr: taken from the arena here)
static int render_net_impl(fp_ctx *ctx, const fp_mesh *mesh, const float *d_poses, int N, const double *K, int H, int W,
                           const float *d_bbox2d, int out_h, int out_w, double mesh_diameter, int normalize_xyz, float invalid_thres,
                           void *d_net_out, void *scratch, size_t scratch_bytes, void *stream) {
  FP_REQUIRE(ctx && d_net_out, "fp_render_net: null argument");
  RenderArgs a;
  FP_TRY(fill_render(a, mesh, d_poses, N, K, H, W, d_bbox2d, out_h, out_w));
  a.use_light = 1;  // make_crop_data_batch renders with use_light=True (predict_pose_refine.py:49)
  a.w_ambient = 0.8f;
  a.w_diffuse = 0.5f;
  a.net_out = (f16 *)d_net_out;
  a.mesh_diameter = (float)mesh_diameter;
  a.invalid_thres = invalid_thres;
  a.normalize_xyz = normalize_xyz;
  if (!scratch) return render_with_arena_scratch(ctx, a, (hipStream_t)stream);
  a.scratch = scratch;
  a.scratch_bytes = scratch_bytes;
  return launch_render(ctx, a, (hipStream_t)stream);
}

extern "C" int fp_render_net(fp_ctx *ctx, const fp_mesh *mesh, const float *d_poses, int N, const double *K, int H, int W,
                             const float *d_bbox2d, int out_h, int out_w, double mesh_diameter, int normalize_xyz, float invalid_thres,
                             void *d_net_out, void *stream) {
  return render_net_impl(ctx, mesh, d_poses, N, K, H, W, d_bbox2d, out_h, out_w, mesh_diameter, normalize_xyz, invalid_thres, d_net_out,
                         nullptr, 0, stream);
}

extern "C" int fp_crop_observed(fp_ctx *ctx, const float *d_rgb, const float *d_geom, int H, int W, const double *K, const float *d_tf,
                                const float *d_poses, int N, int out_h, int out_w, int mode, double mesh_diameter, int normalize_xyz,
                                int out_fmt, void *d_out, void *stream) {
  FP_REQUIRE(ctx && d_rgb && d_geom && K && d_tf && d_poses && d_out, "fp_crop_observed: null argument");
  FP_REQUIRE(out_fmt == 0 || out_fmt == 1, "fp_crop_observed: out_fmt must be 0 or 1");
  CropArgs a;
  a.rgb = d_rgb;
  a.geom = d_geom;
  a.tf = d_tf;
  a.poses = d_poses;
  for (int i = 0; i < 9; ++i) a.K[i] = K[i];
  a.H = H;
  a.W = W;
  a.N = N;
  a.Ho = out_h;
  a.Wo = out_w;
  a.mode = mode;
  a.normalize_xyz = normalize_xyz;
  a.out_fmt = out_fmt;
  a.mesh_diameter = (float)mesh_diameter;
  a.out = d_out;
  ProfScope ps(ctx, (hipStream_t)stream, "crop", (double)N * out_h * out_w * (out_fmt == 1 ? 16.0 : 24.0));      // bytes written
  return launch_crop_observed(a, (hipStream_t)stream);
}

extern "C" int fp_warp_nearest(fp_ctx *ctx, const float *d_src, int src_batch, int src_h, int src_w, int channels, const float *d_tf, int N,
                               int out_h, int out_w, float *d_out, void *stream) {
  FP_REQUIRE(ctx && d_src && d_tf && d_out, "fp_warp_nearest: null argument");
  return launch_warp_nearest(d_src, src_batch, src_h, src_w, channels, d_tf, N, out_h, out_w, d_out, (hipStream_t)stream);
}

extern "C" int fp_erode_depth(fp_ctx *ctx, const float *d_depth, int H, int W, int radius, float depth_diff_thres, float ratio_thres,
                              float zfar, float *d_out, void *stream) {
  FP_REQUIRE(ctx && d_depth && d_out && H > 0 && W > 0 && radius >= 0, "fp_erode_depth: bad argument");
  return launch_erode(d_depth, H, W, radius, depth_diff_thres, ratio_thres, zfar, d_out, (hipStream_t)stream);
}
extern "C" int fp_bilateral_filter_depth(fp_ctx *ctx, const float *d_depth, int H, int W, int radius, float zfar, float sigmaD,
                                         float sigmaR, float *d_out, void *stream) {
  FP_REQUIRE(ctx && d_depth && d_out && H > 0 && W > 0 && radius >= 0, "fp_bilateral_filter_depth: bad argument");
  return launch_bilateral(d_depth, H, W, radius, zfar, sigmaD, sigmaR, d_out, (hipStream_t)stream);
}
extern "C" int fp_depth2xyzmap(fp_ctx *ctx, const float *d_depth, int H, int W, const double *K, float zfar, float *d_xyz, void *stream) {
  FP_REQUIRE(ctx && d_depth && d_xyz && K && H > 0 && W > 0, "fp_depth2xyzmap: bad argument");
  return launch_depth2xyz(d_depth, H, W, K, zfar, d_xyz, (hipStream_t)stream);
}

extern "C" int fp_depth_prefilter(fp_ctx *ctx, const float *d_depth, int H, int W, int radius, float depth_diff_thres, float ratio_thres,
                                  float zfar_erode, float zfar_bilateral, float sigmaD, float sigmaR, const double *K, float zfar_xyz,
                                  float *d_depth_out, float *d_xyz, const uint8_t *d_rgb_u8, float *d_rgb_f32, void *stream) {
  FP_REQUIRE(ctx && d_depth && d_depth_out && d_xyz && K && H > 0 && W > 0, "fp_depth_prefilter: bad argument");
  FP_REQUIRE((d_rgb_u8 == nullptr) == (d_rgb_f32 == nullptr), "fp_depth_prefilter: d_rgb_u8 and d_rgb_f32 go together");
  FP_REQUIRE(radius == 2, "fp_depth_prefilter: radius %d (the fused prelude is built for the radius 2 of src/estimater.py:256-257; "
                          "other radii: fp_erode_depth, fp_bilateral_filter_depth, fp_depth2xyzmap)", radius);
  FP_REQUIRE(d_depth != d_depth_out, "fp_depth_prefilter: in-place filtering is not possible (neighbouring workgroups read the input)");
  return launch_depth_prefilter(d_depth, H, W, depth_diff_thres, ratio_thres, zfar_erode, zfar_bilateral, sigmaD, sigmaR, K, zfar_xyz, d_depth_out,
                                d_xyz, d_rgb_u8, d_rgb_f32, (hipStream_t)stream);
}

extern "C" int fp_depth2xyzmap_f64(fp_ctx *ctx, const float *d_depth, int H, int W, const double *K, float *d_xyz, void *stream) {
  FP_REQUIRE(ctx && d_depth && d_xyz && K && H > 0 && W > 0, "fp_depth2xyzmap_f64: bad argument");
  return launch_depth2xyz_f64(d_depth, H, W, K, d_xyz, (hipStream_t)stream);
}

extern "C" int fp_mask_depth_stats(fp_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int H, int W, float min_depth, int32_t *h_stats6,
                                   float *h_median, void *stream) {
  FP_REQUIRE(ctx && d_depth && d_mask && h_stats6 && h_median && H > 0 && W > 0, "fp_mask_depth_stats: bad argument");
  hipStream_t s = (hipStream_t)stream;
  FP_TRY(fp_arena_ensure(ctx, 4096));
  ArenaScope scope(ctx->arena);      // (released behind the copy and the wait below: host bookkeeping, nothing else takes in between)
  int *d_out = (int *)ctx->arena.take(8 * sizeof(int));
  FP_REQUIRE(d_out, "fp_mask_depth_stats: arena exhausted");
  FP_TRY(launch_mask_depth_stats(d_depth, d_mask, H, W, min_depth, d_out, (float *)(d_out + 6), s));
  int host[8];
  FP_CHECK_HIP(hipMemcpyAsync(host, d_out, sizeof(host), hipMemcpyDeviceToHost, s));
  FP_CHECK_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < 6; ++i) h_stats6[i] = host[i];
  memcpy(h_median, &host[6], sizeof(float));
  return FP_OK;
}

extern "C" int fp_pose_errors(fp_ctx *ctx, const float *d_pts, int n_pts, const float *d_pred, const float *d_gt, int gt_per_pose, int n_poses,
                              const float *d_sym, int n_sym, int which, float *d_add, float *d_adds, float *d_add_sym, void *stream) {
  FP_REQUIRE(ctx && d_pts && d_pred && d_gt, "fp_pose_errors: null argument");
  FP_REQUIRE(n_pts >= 1 && n_poses >= 1, "fp_pose_errors: n_pts %d, n_poses %d (both must be >= 1)", n_pts, n_poses);
  FP_REQUIRE((which & ~(FP_ERR_ADD | FP_ERR_ADDS | FP_ERR_ADD_SYM)) == 0, "fp_pose_errors: unknown bits in which = %d", which);
  FP_REQUIRE(gt_per_pose == 0 || gt_per_pose == 1, "fp_pose_errors: gt_per_pose must be 0 or 1");
  FP_REQUIRE(!(which & FP_ERR_ADD) || d_add, "fp_pose_errors: FP_ERR_ADD requested with d_add null");
  FP_REQUIRE(!(which & FP_ERR_ADDS) || d_adds, "fp_pose_errors: FP_ERR_ADDS requested with d_adds null");
  FP_REQUIRE(!(which & FP_ERR_ADD_SYM) || (d_add_sym && d_sym && n_sym >= 1),
             "fp_pose_errors: FP_ERR_ADD_SYM needs d_add_sym, d_sym and n_sym >= 1 (n_sym %d)", n_sym);
  if (which == 0) return FP_OK;
  const size_t bytes = pose_errors_slab_bytes(n_pts, n_poses, (which & FP_ERR_ADD_SYM) ? n_sym : 0);
  FP_TRY(fp_arena_ensure(ctx, bytes + 4096));
  ArenaScope scope(ctx->arena);
  double *slab = (double *)ctx->arena.take(bytes);
  FP_REQUIRE(slab, "fp_pose_errors: arena exhausted");
  // the slab is consumed by the finishing launch on the same stream before anything else takes it
  return launch_pose_errors(d_pts, n_pts, d_pred, d_gt, gt_per_pose, n_poses, d_sym, n_sym, which, slab, d_add, d_adds, d_add_sym,
                            (hipStream_t)stream);
}

extern "C" int fp_pose_errors_bop(fp_ctx *ctx, const float *d_pts, int n_pts, const float *d_pred, const float *d_gt, int gt_per_pose,
                                  int n_poses, const float *d_sym, int n_sym, const double *K, int which, float *d_mssd, float *d_mspd,
                                  void *stream) {
  FP_REQUIRE(ctx && d_pts && d_pred && d_gt, "fp_pose_errors_bop: null argument");
  FP_REQUIRE(n_pts >= 1 && n_poses >= 0 && n_sym >= 0, "fp_pose_errors_bop: n_pts %d (>= 1), n_poses %d, n_sym %d (>= 0)", n_pts, n_poses, n_sym);
  FP_REQUIRE(n_sym == 0 || d_sym, "fp_pose_errors_bop: n_sym %d with d_sym null", n_sym);
  FP_REQUIRE(gt_per_pose == 0 || gt_per_pose == 1, "fp_pose_errors_bop: gt_per_pose must be 0 or 1");
  FP_REQUIRE((which & ~(FP_BOP_MSSD | FP_BOP_MSPD)) == 0, "fp_pose_errors_bop: unknown bits in which = %d", which);
  FP_REQUIRE(!(which & FP_BOP_MSSD) || d_mssd, "fp_pose_errors_bop: FP_BOP_MSSD requested with d_mssd null");
  FP_REQUIRE(!(which & FP_BOP_MSPD) || (d_mspd && K), "fp_pose_errors_bop: FP_BOP_MSPD needs d_mspd and K");
  if (which == 0 || n_poses == 0) return FP_OK;
  const size_t bytes = bop_errors_slab_bytes(n_pts, n_poses, n_sym);
  FP_TRY(fp_arena_ensure(ctx, bytes + 4096));
  ArenaScope scope(ctx->arena);
  float *slab = (float *)ctx->arena.take(bytes);
  FP_REQUIRE(slab, "fp_pose_errors_bop: arena exhausted");
  // the slab is consumed by the finishing launch on the same stream before anything else takes it
  return launch_bop_errors(d_pts, n_pts, d_pred, d_gt, gt_per_pose, n_poses, d_sym, n_sym, K, which, slab, d_mssd, d_mspd, (hipStream_t)stream);
}

extern "C" int fp_mesh_diameter(fp_ctx *ctx, const float *d_pts, int n_pts, float *d_out_diameter, int32_t *d_out_pair, void *stream) {
  FP_REQUIRE(ctx && d_out_diameter, "fp_mesh_diameter: null argument");
  FP_REQUIRE(n_pts >= 0 && n_pts <= FP_MESH_DIAMETER_MAX_POINTS, "fp_mesh_diameter: n_pts %d (0 .. %d)", n_pts, FP_MESH_DIAMETER_MAX_POINTS);
  FP_REQUIRE(d_pts || n_pts == 0, "fp_mesh_diameter: d_pts null with n_pts %d", n_pts);
  const size_t bytes = mesh_diameter_slab_bytes(n_pts);
  FP_TRY(fp_arena_ensure(ctx, bytes + 4096));
  ArenaScope scope(ctx->arena);
  void *slab = ctx->arena.take(bytes);
  FP_REQUIRE(slab, "fp_mesh_diameter: arena exhausted");
  // the slab is consumed by the finishing launch on the same stream before anything else takes it
  return launch_mesh_diameter(d_pts, n_pts, slab, d_out_diameter, d_out_pair, (hipStream_t)stream);
}

extern "C" int fp_box_extents(fp_ctx *ctx, const float *d_points, int n, const float *d_frames, int C, int32_t *d_best_index, float *d_best_lohi,
                              float *d_best_volume, float *d_all_lohi, float *d_all_volume, void *stream) {
  FP_REQUIRE(ctx && d_points && d_frames && d_best_index && d_best_lohi && d_best_volume, "fp_box_extents: null argument");
  FP_REQUIRE(n >= 1 && n <= FP_BOX_EXTENTS_MAX_POINTS, "fp_box_extents: n %d (1 .. %d)", n, FP_BOX_EXTENTS_MAX_POINTS);
  FP_REQUIRE(C >= 1 && C <= FP_BOX_EXTENTS_MAX_FRAMES, "fp_box_extents: C %d (1 .. %d)", C, FP_BOX_EXTENTS_MAX_FRAMES);
  FP_REQUIRE((long long)n * C <= FP_BOX_EXTENTS_MAX_EVALS, "fp_box_extents: n C = %lld above %lld: cut the candidates into several calls",
             (long long)n * C, (long long)FP_BOX_EXTENTS_MAX_EVALS);
  const size_t bytes = box_extents_slab_bytes(n, C);
  FP_TRY(fp_arena_ensure(ctx, bytes + 4096));
  ArenaScope scope(ctx->arena);
  void *slab = ctx->arena.take(bytes);
  FP_REQUIRE(slab, "fp_box_extents: arena exhausted");
  // the slab is consumed by the finishing launches on the same stream before anything else takes it
  return launch_box_extents(d_points, n, d_frames, C, slab, d_best_index, d_best_lohi, d_best_volume, d_all_lohi, d_all_volume,
                            (hipStream_t)stream);
}

// poses per render chunk of fp_vsd: their depth images (and those of their ground truth, one per pose) within this many bytes
static const size_t kVsdDepthBudget = (size_t)512 << 20;

extern "C" int fp_vsd(fp_ctx *ctx, const fp_mesh *mesh, const float *d_depth_test, int depth_per_pose, int H, int W, const double *K,
                      const float *d_pred, const float *d_gt, int gt_per_pose, int n_poses, double diameter, double delta,
                      const double *h_taus, int n_taus, float *d_err, int32_t *d_counts, void *stream) {
  FP_REQUIRE(ctx && mesh && d_depth_test && K && d_pred && d_gt && h_taus && d_err, "fp_vsd: null argument");
  FP_REQUIRE(n_taus >= 1 && n_taus <= FP_VSD_MAX_TAUS, "fp_vsd: n_taus %d outside 1..%d", n_taus, FP_VSD_MAX_TAUS);
  FP_REQUIRE(H >= 1 && W >= 1 && (size_t)H * W <= ((size_t)1 << 30), "fp_vsd: image %dx%d", H, W);
  FP_REQUIRE(diameter > 0, "fp_vsd: diameter %g must be > 0", diameter);
  FP_REQUIRE((depth_per_pose == 0 || depth_per_pose == 1) && (gt_per_pose == 0 || gt_per_pose == 1),
             "fp_vsd: depth_per_pose and gt_per_pose must be 0 or 1");
  FP_REQUIRE(n_poses >= 0, "fp_vsd: n_poses %d", n_poses);
  if (n_poses == 0) return FP_OK;
  hipStream_t s = (hipStream_t)stream;
  const size_t px = (size_t)H * W;
  const size_t per_pose = px * sizeof(float) * (gt_per_pose ? 2 : 1);
  const int chunk = (int)std::min<size_t>({(size_t)n_poses, std::max<size_t>(1, kVsdDepthBudget / per_pose), 65535});
  const int last = n_poses - (n_poses - 1) / chunk * chunk;
  // one scratch for every render of the call: the largest of the full chunk, the last one and the shared ground truth
  size_t rs = std::max(render_scratch_bytes(chunk, mesh->d.V, mesh->d.F, H, W, ctx->num_cu),
                       render_scratch_bytes(last, mesh->d.V, mesh->d.F, H, W, ctx->num_cu));
  if (!gt_per_pose) rs = std::max(rs, render_scratch_bytes(1, mesh->d.V, mesh->d.F, H, W, ctx->num_cu));
  const size_t counts_bytes = (size_t)n_poses * (2 + FP_VSD_MAX_TAUS) * sizeof(unsigned);
  const size_t dg_bytes = px * sizeof(float) * (gt_per_pose ? chunk : 1), de_bytes = px * sizeof(float) * chunk;
  FP_TRY(fp_arena_ensure(ctx, counts_bytes + dg_bytes + de_bytes + rs + 4 * 256 + 4096));
  ArenaScope scope(ctx->arena);
  unsigned *counts = (unsigned *)ctx->arena.take(counts_bytes);
  float *dg = (float *)ctx->arena.take(dg_bytes);
  float *de = (float *)ctx->arena.take(de_bytes);
  FP_REQUIRE(counts && dg && de, "fp_vsd: arena exhausted");
  FP_CHECK_HIP(hipMemsetAsync(counts, 0, counts_bytes, s));
  // render_with_arena_scratch takes the render scratch behind these buffers and releases it when the launches are queued
  auto render_depth = [&](const float *poses, int n, float *out) -> int {
    RenderArgs a;
    FP_TRY(fill_render(a, mesh, poses, n, K, H, W, nullptr, H, W));
    a.depth = out;
    return render_with_arena_scratch(ctx, a, s);
  };
  if (!gt_per_pose) FP_TRY(render_depth(d_gt, 1, dg));
  for (int b0 = 0; b0 < n_poses; b0 += chunk) {
    const int n = std::min(chunk, n_poses - b0);
    FP_TRY(render_depth(d_pred + (size_t)b0 * 16, n, de));
    if (gt_per_pose) FP_TRY(render_depth(d_gt + (size_t)b0 * 16, n, dg));
    FP_TRY(launch_vsd_count(d_depth_test + (depth_per_pose ? (size_t)b0 * px : 0), depth_per_pose ? px : 0, dg, gt_per_pose ? px : 0, de,
                            n, H, W, K, diameter, delta, h_taus, n_taus, counts + (size_t)b0 * (2 + FP_VSD_MAX_TAUS), s));
  }
  return launch_vsd_finish(counts, n_poses, n_taus, d_err, d_counts, s);
}

// instances per render chunk of fp_scene_instances: their depth layers on the padded canvas within this many bytes
static const size_t kSceneDepthBudget = (size_t)512 << 20;

extern "C" int fp_scene_instances(fp_ctx *ctx, const fp_mesh *const *meshes, const float *d_poses, int n_inst, const double *K, int H, int W,
                                  int pad_x, int pad_y, const float *d_depth_test, int occluders, double delta, uint8_t *d_mask,
                                  uint8_t *d_mask_visib, int32_t *d_owner, float *d_depth, int32_t *d_info, void *stream) {
  FP_REQUIRE(ctx && K, "fp_scene_instances: null ctx or K");
  FP_REQUIRE(n_inst >= 0 && n_inst <= FP_SCENE_MAX_INSTANCES, "fp_scene_instances: n_inst %d outside 0..%d", n_inst, FP_SCENE_MAX_INSTANCES);
  FP_REQUIRE(n_inst == 0 || (meshes && d_poses), "fp_scene_instances: null meshes or d_poses with n_inst %d", n_inst);
  for (int i = 0; i < n_inst; ++i) FP_REQUIRE(meshes[i], "fp_scene_instances: meshes[%d] is null", i);
  FP_REQUIRE(H >= 1 && W >= 1, "fp_scene_instances: image %dx%d", H, W);
  FP_REQUIRE(pad_x >= 0 && pad_y >= 0, "fp_scene_instances: negative pad (%d, %d)", pad_x, pad_y);
  FP_REQUIRE(occluders != 0 && (occluders & ~(FP_SCENE_OCC_DEPTH | FP_SCENE_OCC_INSTANCES)) == 0,
             "fp_scene_instances: occluders = %d (FP_SCENE_OCC_DEPTH | FP_SCENE_OCC_INSTANCES, at least one)", occluders);
  FP_REQUIRE(!(occluders & FP_SCENE_OCC_DEPTH) || d_depth_test, "fp_scene_instances: FP_SCENE_OCC_DEPTH with d_depth_test null");
  FP_REQUIRE(delta >= 0, "fp_scene_instances: delta %g must be >= 0", delta);
  const long long Wc_ll = (long long)W + 2LL * pad_x, Hc_ll = (long long)H + 2LL * pad_y;
  FP_REQUIRE(Wc_ll * 10 <= 64 * 1024, "fp_scene_instances: canvas width %lld (W %d + 2 pad_x %d) is above the rasteriser's 6553: reduce pad_x",
             Wc_ll, W, pad_x);
  FP_REQUIRE(Hc_ll <= 65535 && Hc_ll * Wc_ll <= ((long long)1 << 30), "fp_scene_instances: canvas %lldx%lld: reduce pad_y", Hc_ll, Wc_ll);
  hipStream_t s = (hipStream_t)stream;
  const int Hc = (int)Hc_ll, Wc = (int)Wc_ll;
  const size_t pxf = (size_t)H * W, pxc = (size_t)Hc * Wc;
  if (n_inst == 0) {
    if (d_owner) FP_CHECK_HIP(hipMemsetAsync(d_owner, 0xff, pxf * sizeof(int32_t), s));
    if (d_depth) FP_CHECK_HIP(hipMemsetAsync(d_depth, 0, pxf * sizeof(float), s));
    return FP_OK;
  }
  double Kc[9];
  for (int i = 0; i < 9; ++i) Kc[i] = K[i];
  Kc[2] = K[2] + (double)pad_x, Kc[5] = K[5] + (double)pad_y;
  const bool occ_inst = (occluders & FP_SCENE_OCC_INSTANCES) != 0, occ_depth = (occluders & FP_SCENE_OCC_DEPTH) != 0;
  const bool want_masks = d_mask || d_mask_visib || d_info;
  const bool need_min = d_owner || d_depth || (occ_inst && (d_mask_visib || d_info));
  if (!want_masks && !need_min) return FP_OK;
  const int chunk = (int)std::min<size_t>((size_t)n_inst, std::max<size_t>(1, kSceneDepthBudget / (pxc * sizeof(float))));
  // the minimum over every chunk first, then the masks (two renders), only where a visibility test reads that minimum
  const bool two_pass = occ_inst && (d_mask_visib || d_info) && chunk < n_inst;
  // one scratch for every render of the call: the largest run of instances of one mesh inside a chunk
  size_t rs = 0;
  for (int b0 = 0; b0 < n_inst; b0 += chunk)
    for (int r0 = b0, e = std::min(n_inst, b0 + chunk); r0 < e;) {
      int r1 = r0 + 1;
      while (r1 < e && meshes[r1] == meshes[r0]) ++r1;
      if (!render_fits(r1 - r0, meshes[r0]->d.V, meshes[r0]->d.F, Hc, Wc, ctx->num_cu)) {
        if (pad_x || pad_y)
          fp_set_error("fp_scene_instances: the canvas of %dx%d pixels (frame %dx%d, pad_x %d, pad_y %d) needs more strips than the rasteriser "
                       "has: reduce pad_x / pad_y", Wc, Hc, W, H, pad_x, pad_y);
        else
          fp_set_error("fp_scene_instances: a frame of %dx%d pixels needs more strips than the rasteriser has", W, H);
        return FP_EINVAL;
      }
      rs = std::max(rs, render_scratch_bytes(r1 - r0, meshes[r0]->d.V, meshes[r0]->d.F, Hc, Wc, ctx->num_cu));
      r0 = r1;
    }
  const size_t layer_bytes = pxc * sizeof(float) * chunk, acc_bytes = (size_t)n_inst * FP_SCENE_INFO_COLS * sizeof(int);
  FP_TRY(fp_arena_ensure(ctx, layer_bytes + acc_bytes + pxf * 8 + rs + 8 * 256 + 4096));
  ArenaScope scope(ctx->arena);
  float *layers = (float *)ctx->arena.take(layer_bytes);
  int *acc = d_info ? (int *)ctx->arena.take(acc_bytes) : nullptr;
  // the running minimum lives in the caller's d_depth / d_owner; a call that needs it over several chunks without asking for it borrows the arena
  float *dmin = d_depth ? d_depth : (need_min && chunk < n_inst ? (float *)ctx->arena.take(pxf * sizeof(float)) : nullptr);
  if (!layers || (d_info && !acc) || (need_min && chunk < n_inst && !dmin)) {
    fp_set_error("fp_scene_instances: arena exhausted");
    return FP_ENOMEM;
  }
  if (acc) FP_TRY(launch_scene_info_init(acc, n_inst, s));
  // render_with_arena_scratch takes the render scratch behind these buffers and releases it when the launches are queued
  auto render_chunk_layers = [&](int b0, int n) -> int {
    for (int r0 = b0; r0 < b0 + n;) {
      int r1 = r0 + 1;
      while (r1 < b0 + n && meshes[r1] == meshes[r0]) ++r1;
      RenderArgs a;
      FP_TRY(fill_render(a, meshes[r0], d_poses + (size_t)r0 * 16, r1 - r0, Kc, Hc, Wc, nullptr, Hc, Wc));
      a.depth = layers + (size_t)(r0 - b0) * pxc;
      FP_TRY(render_with_arena_scratch(ctx, a, s));
      r0 = r1;
    }
    return FP_OK;
  };
  auto pass = [&](bool do_min, bool do_masks) -> int {
    for (int b0 = 0; b0 < n_inst; b0 += chunk) {
      const int n = std::min(chunk, n_inst - b0);
      FP_TRY(render_chunk_layers(b0, n));
      SceneLaunch l;
      l.layers = layers, l.dt = d_depth_test, l.n = n, l.i0 = b0, l.H = H, l.W = W, l.pad_x = pad_x, l.pad_y = pad_y;
      l.do_min = do_min, l.do_masks = do_masks, l.first = b0 == 0, l.occ_depth = occ_depth, l.occ_inst = occ_inst;
      l.K = K, l.delta = delta, l.dmin = dmin, l.owner = d_owner, l.mask = d_mask, l.mask_visib = d_mask_visib, l.acc = acc;
      FP_TRY(launch_scene_instances(ctx, l, s));
    }
    return FP_OK;
  };
  if (two_pass) {
    FP_TRY(pass(true, false));
    FP_TRY(pass(false, true));
  } else {
    FP_TRY(pass(need_min, want_masks));
  }
  return acc ? launch_scene_info_finish(acc, n_inst, d_info, s) : FP_OK;
}

extern "C" int fp_pose_update(fp_ctx *ctx,const float *d_poseA, const float *d_trans, const float *d_rot, int N, int rot_dim,
                              int trans_rep_tanh, const float *tn, float rot_normalizer, float trans_scale, float *d_pose_out,
                              void *stream) {
  FP_REQUIRE(ctx && d_poseA && d_trans && d_rot && d_pose_out, "fp_pose_update: null argument");
  float t0 = tn ? tn[0] : 1.f, t1 = tn ? tn[1] : 1.f, t2 = tn ? tn[2] : 1.f;
  FP_REQUIRE(trans_rep_tanh == 0 || trans_rep_tanh == 1, "fp_pose_update: trans_rep_tanh must be 0 or 1 (trans_rep='deepim': fp_pose_update_deepim)");
  return launch_pose_update(d_poseA, d_trans, d_rot, N, rot_dim, trans_rep_tanh, t0, t1, t2, rot_normalizer, trans_scale, d_pose_out,
                            (hipStream_t)stream);
}

extern "C" int fp_pose_update_deepim(fp_ctx *ctx, const float *d_poseA, const float *d_trans, const float *d_rot, int N, int rot_dim,
                                     const float *d_tf_to_crops, const double *K, float input_resize, float rot_normalizer, float trans_scale,
                                     float *d_pose_out, void *stream) {
  FP_REQUIRE(ctx && d_poseA && d_trans && d_rot && d_pose_out && d_tf_to_crops && K, "fp_pose_update_deepim: null argument");
  return launch_pose_update(d_poseA, d_trans, d_rot, N, rot_dim, 2, 1.f, 1.f, 1.f, rot_normalizer, trans_scale, d_pose_out, (hipStream_t)stream,
                            d_tf_to_crops, K, input_resize);
}

// ---- composed loops --------------------------------------------------------------------------------
#define TAKE(ptr, type, count)                                                             \
  type *ptr = (type *)ctx->arena.take((size_t)(count) * sizeof(type));                     \
  if (!ptr) {                                                                              \
    fp_set_error("arena exhausted (%s); call fp_ctx_reserve with a larger max_hyp", #ptr); \
    return FP_ENOMEM;                                                                      \
  }

static int check_objs(const fp_object_batch *objs, int n_obj, int *total) {
  FP_REQUIRE(objs && n_obj >= 1, "multi: need at least one object");
  int N = 0;
  for (int o = 0; o < n_obj; ++o) {
    FP_REQUIRE(objs[o].mesh && objs[o].d_rgb && objs[o].d_geom && objs[o].K, "multi: object %d has a null field", o);
    FP_REQUIRE(objs[o].n >= 0 && objs[o].H > 1 && objs[o].W > 1 && objs[o].mesh_diameter > 0, "multi: object %d has a bad shape", o);
    N += objs[o].n;
  }
  *total = N;
  return FP_OK;
}

// Objects whose crop windows and renders can share one launch: same mesh, camera and frame size (their hypotheses are
// contiguous in d_poses).  A rank of the sharded multi-GPU job holds a slice of several objects of ONE mesh: one 252-hypothesis
// render instead of eight 32-hypothesis ones that each fill a quarter of the chip.
static bool same_render_key(const fp_object_batch &a, const fp_object_batch &b) {
  return a.mesh == b.mesh && a.H == b.H && a.W == b.W && a.mesh_diameter == b.mesh_diameter && memcmp(a.K, b.K, 9 * sizeof(double)) == 0;
}

// scratch block of one 160 x 160 render of n hypotheses, rounded to the arena's 256 bytes: the passes lay such blocks end to end
static size_t render_block_bytes(fp_ctx *ctx, const fp_mesh *mesh, int n) {
  return (render_scratch_bytes(n, mesh->d.V, mesh->d.F, 160, 160, ctx->num_cu) + 255) & ~(size_t)255;
}

// The non-empty runs of like objects of a pass, in order: objects [o0, o1), their `cnt` hypotheses from hypothesis `off` on, and the run's
// own block of the pass' render scratch (the renders of the runs may overlap on side streams; a run whose worst case exceeds 1 GiB is
// rendered in sub-batches: launch_render).  An object without hypotheses adds nothing to its run; a run of such objects only is left out.
struct RenderRun {
  int o0, o1, off, cnt;
  size_t soff, sbytes;
};

// -> the scratch of all runs; `runs` (optional) receives them
static size_t render_runs(fp_ctx *ctx, const fp_object_batch *objs, int n_obj, std::vector<RenderRun> *runs) {
  size_t bytes = 0;
  for (int o = 0, off = 0; o < n_obj;) {
    int e = o + 1, cnt = objs[o].n;
    while (e < n_obj && same_render_key(objs[o], objs[e])) cnt += objs[e++].n;
    if (cnt > 0) {
      const size_t sb = render_block_bytes(ctx, objs[o].mesh, cnt);
      if (runs) runs->push_back(RenderRun{o, e, off, cnt, bytes, sb});
      bytes += sb;
    }
    off += cnt;
    o = e;
  }
  return bytes;
}

// arena bytes of a fused pass over N hypotheses: crop transforms, the two net-input sides (0.82 MB per hypothesis), the render
// scratch, the network forward
static size_t pass_arena_bytes(int N, size_t render_scratch) {
  return (size_t)N * ((size_t)1 << 20) + ((size_t)1 << 20) + render_scratch + fp_arena_inner_bytes(N);
}

static_assert(FP_REFINE_SHARED_TRANSLATION == PASS_FLAG_SHARED_TRANSLATION && FP_NET_REFINE == PASS_REFINE && FP_NET_SCORE == PASS_SCORE, "pass_plan.h restates them");

struct NetInputOpts {
  int mode;                  // of the observed crop (fp_crop_observed)
  float invalid_thres;       // of the rendered side
  double crop_ratio;
  int normalize_xyz;
  bool windows_written;      // tf / bbox hold this pass' crop windows already
  // shared side B (`sb` optional; one run): ONE observed crop per live object (window and translation of its first hypothesis = of all of
  // them) into xB1, encoded into featB (= sb->feat) by `net`; sb->start / n_groups are filled here
  const fp_net *net;
  SharedB *sb;
  f16 *xB1, *featB;
};

// The input of ONE network pass over every object: per run of like objects the crop windows (tf, bbox) and the render (side A: net_in[0, N))
// on the run's stream, per object the observed crop (side B: net_in[N, 2N)).  `ab` (set for two side chains - PassPlan::fork_sides: the
// rendered side (crop window -> rasteriser -> encodeA) and the observed side (crop window -> observed crop -> encodeA) on two streams up to
// the channel concat of run_trunk, bit-identical to one chain - or a shared side B; forked behind the crop windows) is left for the forward
// pass to join; the runs' streams are joined here.
static int build_net_input(fp_ctx *ctx, const fp_object_batch *objs, const std::vector<RenderRun> &runs, int N, const PassPlan &plan, const float *d_poses,
                           const NetInputOpts &op, float *tf, float *bbox, f16 *net_in, char *rscratch, hipStream_t s,
                           std::unique_ptr<StreamFanout> &ab) {
  const size_t img = (size_t)160 * 160 * 8;
  const bool two_sides = plan.fork_sides;
  StreamFanout fo(ctx, s, two_sides ? 1 : (int)runs.size());
  if (op.sb) op.sb->n_groups = 0;
  int k = 0;
  for (const RenderRun &r : runs) {
    const fp_object_batch &ob = objs[r.o0];
    hipStream_t so = fo.stream_for(k++);
    int off = r.off;
    const float *p = d_poses + (size_t)off * 16;
    if (!op.windows_written)
      FP_TRY(launch_crop_window_tf(p, r.cnt, ob.K, op.crop_ratio, ob.mesh_diameter, 160, 160, tf + (size_t)off * 9, bbox + (size_t)off * 4, so));
    if (two_sides || op.sb) ab.reset(new StreamFanout(ctx, s, 2));
    int rc = render_net_impl(ctx, ob.mesh, p, r.cnt, ob.K, ob.H, ob.W, bbox + (size_t)off * 4, 160, 160, ob.mesh_diameter, op.normalize_xyz,
                             op.invalid_thres, net_in + (size_t)off * img, rscratch + r.soff, r.sbytes, so);
    hipStream_t sb_stream = ab ? ab->stream_for(0) : so;
    for (int q = r.o0; q < r.o1 && rc == FP_OK; ++q) {
      const fp_object_batch &oq = objs[q];
      if (oq.n == 0) continue;
      f16 *out = net_in + ((size_t)N + off) * img;
      if (op.sb) {
        op.sb->start[op.sb->n_groups] = off;
        out = op.xB1 + (size_t)op.sb->n_groups++ * img;
      }
      rc = fp_crop_observed(ctx, oq.d_rgb, oq.d_geom, oq.H, oq.W, oq.K, tf + (size_t)off * 9, d_poses + (size_t)off * 16, op.sb ? 1 : oq.n, 160, 160,
                            op.mode, oq.mesh_diameter, op.normalize_xyz, 1, out, sb_stream);
      off += oq.n;
    }
    if (op.sb && rc == FP_OK) {
      op.sb->start[op.sb->n_groups] = off;
      rc = fp_encode_side_b(ctx, op.net, op.xB1, op.sb->n_groups, N, op.featB, sb_stream);
    }
    if (rc != FP_OK) {
      if (ab) (void)ab->join();
      (void)fo.join();
      return rc;
    }
  }
  return fo.join();
}

// The fields of a refinement pass' tail launch that every pass fills alike (iteration `it` of `iteration`; `diameter`: of the crop windows)
static RefineTailArgs fill_refine_tail(const fp_refine_cfg *cfg, const double *K, double diameter, float *tf, float *bbox, float *poses, int it,
                                       int iteration) {
  RefineTailArgs t;
  memset(&t, 0, sizeof(t));
  t.poses = poses;
  t.trans_tanh = cfg->trans_rep_tanh;
  t.tn0 = cfg->trans_normalizer[0], t.tn1 = cfg->trans_normalizer[1], t.tn2 = cfg->trans_normalizer[2];
  t.rot_normalizer = cfg->rot_normalizer;
  for (int i = 0; i < 9; ++i) t.K[i] = (float)K[i];
  t.resize = 160.f;
  t.tf = tf, t.bbox = bbox;
  t.next_window = it + 1 < iteration;
  t.win = crop_window_k(K, cfg->crop_ratio, diameter, 160, 160);
  return t;
}

// `centered` (optional, one run of like objects): poses @ get_tf_to_centered_mesh() of the LAST iteration, written by that pass' tail launch
struct RefineFinal {
  float *centered;
  float cneg[3];
};

static int refine_predict_impl(fp_ctx *ctx, const fp_net *net, const fp_object_batch *objs, int n_obj, const fp_refine_cfg *cfg,
                               float *d_poses, int iteration, float *d_trans, float *d_rot, void *stream, const RefineFinal *fin, unsigned flags = 0) {
  FP_REQUIRE(ctx && net && cfg && d_poses, "fp_refine_predict_multi: null argument");
  FP_REQUIRE(iteration >= 0, "fp_refine_predict_multi: bad iteration");
  int N = 0;
  FP_TRY(check_objs(objs, n_obj, &N));
  if (N == 0 || iteration == 0) return FP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int rot_dim = fp_net_rot_dim(net);
  std::vector<RenderRun> runs;          // once per call: every iteration walks the same runs over the same scratch blocks
  const size_t rs_total = render_runs(ctx, objs, n_obj, &runs);
  FP_TRY(fp_arena_ensure(ctx, pass_arena_bytes(N, rs_total) + (size_t)n_obj * ((size_t)4 << 20)));
  ArenaScope scope(ctx->arena);
  const size_t img = (size_t)160 * 160 * 8;
  TAKE(tf, float, (size_t)N * 9);
  TAKE(bbox, float, (size_t)N * 4);
  TAKE(trans, float, (size_t)N * 3);
  TAKE(rot, float, (size_t)N * 6);
  TAKE(net_in, f16, (size_t)2 * N * img);
  float *tr = d_trans ? d_trans : trans, *ro = d_rot ? d_rot : rot;
  TAKE(rscratch, char, rs_total);                              // reused by every iteration
  // plan.fused_tail - one run of like objects (one camera, one mesh, one diameter): the heads' token means, the pose update and the crop windows of
  // the next iteration are ONE launch behind the heads (refine_tail_kernel) instead of four.  Bit-identical.
  // plan.shared_b - FP_REFINE_SHARED_TRANSLATION: in the FIRST iteration every hypothesis of an object has the crop window of the object's first one, so
  // side B - the observed crop and its way through encodeA - is ONE image per object: cropped and encoded once on the side stream
  // (fp_encode_side_b), copied into the B half of the channel concat by run_trunk.  One run of like objects, at most 8 of them, no
  // hypothesis chunks; otherwise the plain pass runs.
  int n_live = 0;
  for (int o = 0; o < n_obj; ++o) n_live += objs[o].n > 0;
  const PassPlan plan = pass_plan(PASS_REFINE, N, (int)runs.size(), n_live, flags, pass_knobs());
  NetInputOpts op = {0, 0.001f, cfg->crop_ratio, cfg->normalize_xyz, false, net, nullptr, nullptr, nullptr};
  SharedB sb;
  sb.feat = nullptr;
  if (plan.shared_b) {
    TAKE(xB1, f16, (size_t)n_live * img);
    TAKE(featB, f16, (size_t)n_live * 1600 * 128);
    op.xB1 = xB1, op.featB = featB, sb.feat = featB;
  }
  for (int it = 0; it < iteration; ++it) {
    std::unique_ptr<StreamFanout> ab;
    op.windows_written = plan.fused_tail && it > 0;       // (from the second iteration on the previous pass' tail has written the windows)
    op.sb = plan.shared_b && it == 0 ? &sb : nullptr;
    FP_TRY(build_net_input(ctx, objs, runs, N, plan, d_poses, op, tf, bbox, net_in, rscratch, s, ab));
    if (plan.fused_tail) {
      const fp_object_batch &ob = objs[runs[0].o0];
      RefineTailArgs t = fill_refine_tail(cfg, ob.K, ob.mesh_diameter, tf, bbox, d_poses, it, iteration);
      t.trans_scale = cfg->normalize_xyz ? (float)(ob.mesh_diameter / 2) : 1.f;
      if (fin && it + 1 == iteration) {
        t.centered = fin->centered;
        for (int c = 0; c < 3; ++c) t.cneg[c] = fin->cneg[c];
      }
      FP_TRY(fp_refine_forward_ab(ctx, net, net_in, N, tr, ro, s, ab.get(), &t, op.sb));
      continue;
    }
    FP_REQUIRE(!fin, "refine pass: the centred poses come from the fused tail launch (one run of like objects, no chunks, the tail not split by its knob)");
    FP_TRY(fp_refine_forward_ab(ctx, net, net_in, N, tr, ro, s, ab.get(), nullptr, op.sb));     // ONE network pass for every object (joins `ab`)
    // pose update: one launch per run of objects with the same translation scale (one launch when they share a mesh).  Not the render
    // runs: the key here is the scale alone, and trans_rep='deepim' also needs the object's intrinsics (one launch per object)
    for (int o = 0, off = 0; o < n_obj;) {
      const float trans_scale = cfg->normalize_xyz ? (float)(objs[o].mesh_diameter / 2) : 1.f;
      int cnt = 0, e = o;
      while (e < n_obj && (cfg->normalize_xyz ? (float)(objs[e].mesh_diameter / 2) : 1.f) == trans_scale && (cfg->trans_rep_tanh != 2 || e == o))
        cnt += objs[e++].n;
      if (cnt > 0)
        FP_TRY(launch_pose_update(d_poses + (size_t)off * 16, tr + (size_t)off * 3, ro + (size_t)off * rot_dim, cnt, rot_dim,
                                  cfg->trans_rep_tanh, cfg->trans_normalizer[0], cfg->trans_normalizer[1], cfg->trans_normalizer[2],
                                  cfg->rot_normalizer, trans_scale, d_poses + (size_t)off * 16, s, tf + (size_t)off * 9, objs[o].K, 160.f));      // in place
      off += cnt;
      o = e;
    }
  }
  return FP_OK;
}

extern "C" int fp_refine_predict_multi(fp_ctx *ctx, const fp_net *net, const fp_object_batch *objs, int n_obj, const fp_refine_cfg *cfg,
                                       float *d_poses, int iteration, float *d_trans, float *d_rot, void *stream) {
  return refine_predict_impl(ctx, net, objs, n_obj, cfg, d_poses, iteration, d_trans, d_rot, stream, nullptr);
}

extern "C" int fp_refine_predict_multi_flags(fp_ctx *ctx, const fp_net *net, const fp_object_batch *objs, int n_obj, const fp_refine_cfg *cfg,
                                             float *d_poses, int iteration, float *d_trans, float *d_rot, unsigned flags, void *stream) {
  FP_REQUIRE((flags & ~(unsigned)FP_REFINE_SHARED_TRANSLATION) == 0, "fp_refine_predict_multi_flags: unknown flag bits 0x%x", flags);
  return refine_predict_impl(ctx, net, objs, n_obj, cfg, d_poses, iteration, d_trans, d_rot, stream, nullptr, flags);
}

extern "C" int fp_refine_predict(fp_ctx *ctx, const fp_net *net, const fp_mesh *mesh, const float *d_rgb, const float *d_xyz_map,
                                 int H, int W, const double *K, double mesh_diameter, const fp_refine_cfg *cfg, float *d_poses, int N,
                                 int iteration, float *d_trans, float *d_rot, void *stream) {
  FP_REQUIRE(N >= 0, "fp_refine_predict: bad N");
  fp_object_batch ob = {mesh, d_rgb, d_xyz_map, H, W, K, mesh_diameter, N};
  return fp_refine_predict_multi(ctx, net, &ob, 1, cfg, d_poses, iteration, d_trans, d_rot, stream);
}

static int score_features_impl(fp_ctx *ctx, const fp_net *net, const fp_object_batch *objs, int n_obj, double crop_ratio,
                               int normalize_xyz, const float *d_poses, float *d_feats, int feat_ld, bool with_pose, void *stream) {
  FP_REQUIRE(ctx && net && d_poses && d_feats, "fp_score_predict_features_multi: null argument");
  int N = 0;
  FP_TRY(check_objs(objs, n_obj, &N));
  if (N == 0) return FP_OK;
  hipStream_t s = (hipStream_t)stream;
  std::vector<RenderRun> runs;
  const size_t rs_total = render_runs(ctx, objs, n_obj, &runs);
  FP_TRY(fp_arena_ensure(ctx, pass_arena_bytes(N, rs_total)));
  ArenaScope scope(ctx->arena);
  TAKE(tf, float, (size_t)N * 9);
  TAKE(bbox, float, (size_t)N * 4);
  TAKE(net_in, f16, (size_t)2 * N * (size_t)160 * 160 * 8);
  TAKE(rscratch, char, rs_total);
  std::unique_ptr<StreamFanout> ab;
  const NetInputOpts op = {1, 0.1f, crop_ratio, normalize_xyz, false, nullptr, nullptr, nullptr, nullptr};
  const PassPlan plan = pass_plan(PASS_SCORE, N, (int)runs.size(), n_obj, 0, pass_knobs());
  FP_TRY(build_net_input(ctx, objs, runs, N, plan, d_poses, op, tf, bbox, net_in, rscratch, s, ab));
  return fp_score_features_ab(ctx, net, net_in, N, d_feats, s, ab.get(), feat_ld, with_pose ? d_poses : nullptr);
}

extern "C" int fp_score_predict_features_multi(fp_ctx *ctx, const fp_net *net, const fp_object_batch *objs, int n_obj, double crop_ratio,
                                               int normalize_xyz, const float *d_poses, float *d_feats, void *stream) {
  return score_features_impl(ctx, net, objs, n_obj, crop_ratio, normalize_xyz, d_poses, d_feats, 512, false, stream);
}

extern "C" int fp_score_predict_rows_multi(fp_ctx *ctx, const fp_net *net, const fp_object_batch *objs, int n_obj, double crop_ratio,
                                           int normalize_xyz, const float *d_poses, float *d_rows, void *stream) {
  return score_features_impl(ctx, net, objs, n_obj, crop_ratio, normalize_xyz, d_poses, d_rows, 528, true, stream);
}

extern "C" int fp_score_predict_features(fp_ctx *ctx, const fp_net *net, const fp_mesh *mesh, const float *d_rgb, const float *d_depth,
                                         int H, int W, const double *K, double mesh_diameter, double crop_ratio, int normalize_xyz,
                                         const float *d_poses, int N, float *d_feats, void *stream) {
  FP_REQUIRE(N >= 0, "fp_score_predict_features: N<0");
  fp_object_batch ob = {mesh, d_rgb, d_depth, H, W, K, mesh_diameter, N};
  return fp_score_predict_features_multi(ctx, net, &ob, 1, crop_ratio, normalize_xyz, d_poses, d_feats, stream);
}

// ---- one tracking frame, every launch of it (src/estimater.py:250-268; n_hyp > 1: the multi-hypothesis mode of BASELINE configs[4]) ----
// hypotheses of the multi-hypothesis mode: R_i = dR_i R, t_i = t + dt_i (tracking.py), hypothesis 0 = the pose itself
__global__ void track_hypotheses_kernel(const float *__restrict__ P, const float *__restrict__ pose, int n, float *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *p = P + (size_t)i * 16;
  float *o = out + (size_t)i * 16;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      float acc = __fmul_rn(p[r * 4 + 0], pose[0 * 4 + c]);
      acc = __fadd_rn(acc, __fmul_rn(p[r * 4 + 1], pose[1 * 4 + c]));
      acc = __fadd_rn(acc, __fmul_rn(p[r * 4 + 2], pose[2 * 4 + c]));
      o[r * 4 + c] = acc;
    }
    o[r * 4 + 3] = __fadd_rn(pose[r * 4 + 3], p[r * 4 + 3]);
  }
  o[12] = 0.f, o[13] = 0.f, o[14] = 0.f, o[15] = 1.f;
}

// depth prelude of a frame: erode -> bilateral -> back-projection with `K` (src/estimater.py:256-260), + uint8 -> float colours; one launch
static int depth_prelude(const float *d_depth, int H, int W, const double *K, float *d_depth_f, float *d_xyz, int rgb_is_u8, const void *d_rgb,
                         float *d_rgb_f, hipStream_t s) {
  return launch_depth_prefilter(d_depth, H, W, 0.001f, 0.8f, 100.f, 100.f, 2.f, 100000.f, K, 3.0e38f, d_depth_f, d_xyz,
                                rgb_is_u8 ? (const uint8_t *)d_rgb : nullptr, rgb_is_u8 ? d_rgb_f : nullptr, s);
}

extern "C" int fp_track_frame(fp_ctx *ctx, const fp_track_args *a, void *stream) {
  FP_REQUIRE(ctx && a, "fp_track_frame: null argument");
  FP_REQUIRE(a->struct_size == sizeof(fp_track_args), "fp_track_frame: fp_track_args.struct_size = %zu (this library knows %zu)", a->struct_size, sizeof(fp_track_args));
  FP_REQUIRE(a->refine_net && a->mesh && a->d_rgb && a->d_depth && a->K && a->refine_cfg && a->d_pose && a->d_pose_of_mesh && a->d_depth_f && a->d_xyz,
             "fp_track_frame: null field");
  FP_REQUIRE(a->H > 0 && a->W > 0 && a->iteration >= 1 && a->n_hyp >= 1, "fp_track_frame: bad H / W / iteration / n_hyp");
  FP_REQUIRE(!a->rgb_is_u8 || a->d_rgb_f, "fp_track_frame: a uint8 frame needs the float workspace d_rgb_f");
  const bool multi = a->n_hyp > 1;
  FP_REQUIRE(!multi || (a->score_net && a->d_perturb && a->d_poses && a->d_scores && a->d_best), "fp_track_frame: n_hyp > 1 needs score_net, d_perturb, d_poses, d_scores, d_best");
  hipStream_t s = (hipStream_t)stream;
  double K32[9];          // the prelude back-projects with the float32 camera matrix
  for (int i = 0; i < 9; ++i) K32[i] = (double)(float)a->K[i];
  FP_TRY(depth_prelude(a->d_depth, a->H, a->W, K32, a->d_depth_f, a->d_xyz, a->rgb_is_u8, a->d_rgb, a->d_rgb_f, s));
  const float *rgb_f = a->rgb_is_u8 ? a->d_rgb_f : (const float *)a->d_rgb;
  RefineFinal fin;
  for (int c = 0; c < 3; ++c) fin.cneg[c] = -a->model_center[c];
  if (!multi) {
    // track_one: the pose is refined IN PLACE; its last tail launch also writes pose @ get_tf_to_centered_mesh()
    fin.centered = a->d_pose_of_mesh;
    fp_object_batch ob = {a->mesh, rgb_f, a->d_xyz, a->H, a->W, a->K, a->mesh_diameter, 1};
    return refine_predict_impl(ctx, a->refine_net, &ob, 1, a->refine_cfg, a->d_pose, a->iteration, nullptr, nullptr, stream, &fin);
  }
  hipLaunchKernelGGL(track_hypotheses_kernel, dim3((a->n_hyp + 63) / 64), dim3(64), 0, s, a->d_perturb, a->d_pose, a->n_hyp, a->d_poses);
  FP_CHECK_HIP(hipGetLastError());
  fp_object_batch ob = {a->mesh, rgb_f, a->d_xyz, a->H, a->W, a->K, a->mesh_diameter, a->n_hyp};
  FP_TRY(refine_predict_impl(ctx, a->refine_net, &ob, 1, a->refine_cfg, a->d_poses, a->iteration, nullptr, nullptr, stream, nullptr));
  FP_TRY(fp_arena_ensure(ctx, (size_t)a->n_hyp * (512 + 1) * 4 + 4096));
  ArenaScope scope(ctx->arena);
  float *feats = (float *)ctx->arena.take((size_t)a->n_hyp * 512 * sizeof(float));
  float *logits = (float *)ctx->arena.take((size_t)a->n_hyp * sizeof(float));
  if (!feats || !logits) {
    fp_set_error("fp_track_frame: arena exhausted");
    return FP_ENOMEM;
  }
  fp_object_batch od = {a->mesh, rgb_f, a->d_depth_f, a->H, a->W, a->K, a->mesh_diameter, a->n_hyp};
  FP_TRY(fp_score_predict_features_multi(ctx, a->score_net, &od, 1, a->score_crop_ratio, a->score_normalize_xyz, a->d_poses, feats, stream));
  ScoreTailOut o;
  o.logits = logits, o.scores = a->d_scores, o.score_offset = 100.f, o.argmax = a->d_best;
  o.poses = a->d_poses, o.best_pose = a->d_pose, o.best_centered = a->d_pose_of_mesh;
  for (int c = 0; c < 3; ++c) o.cneg[c] = fin.cneg[c];
  return fp_score_tail_impl(ctx, a->score_net, feats, 512, 1, a->n_hyp, o, s);
}

// ---- track_one of several objects of one frame (fp_track_objects): hypothesis o of the pass is object o.  Per iteration ONE render launch
// for the objects the one-launch form takes (render_objects_kernel; the others one launch each), ONE observed-crop launch, one network pass
// over the n_obj images and one tail launch; the first iteration's crop windows are one launch that also gathers the objects' poses.  Each
// stage is the one-object pass' arithmetic on the object's own mesh and diameter.
static int track_objects_pass(fp_ctx *ctx, const fp_track_objects_args *a, const float *rgb_f, hipStream_t s) {
  const int N = a->n_obj;
  const fp_refine_cfg *cfg = a->refine_cfg;
  const fp_track_object *objs = a->objs;
  const size_t img = (size_t)160 * 160 * 8;
  bool solo[FP_TRACK_MAX_OBJECTS];
  size_t rs = 0;                // scratch of the objects rendered on their own
  for (int o = 0; o < N; ++o) {
    const MeshDev &m = objs[o].mesh->d;
    solo[o] = render_objects_form(m.V, m.F, 160, 160, ctx->num_cu);
    if (!solo[o]) rs += render_block_bytes(ctx, objs[o].mesh, 1);
  }
  FP_TRY(fp_arena_ensure(ctx, pass_arena_bytes(N, rs) + (size_t)N * 16 * sizeof(float) + 4096));
  ArenaScope scope(ctx->arena);
  TAKE(poses, float, (size_t)N * 16);
  TAKE(tf, float, (size_t)N * 9);
  TAKE(bbox, float, (size_t)N * 4);
  TAKE(trans, float, (size_t)N * 3);
  TAKE(rot, float, (size_t)N * 6);
  TAKE(net_in, f16, (size_t)2 * N * img);
  TAKE(rscratch, char, rs);
  const float *pose_in[FP_TRACK_MAX_OBJECTS];
  const MeshDev *mesh[FP_TRACK_MAX_OBJECTS];
  float diam[FP_TRACK_MAX_OBJECTS], rdiam[FP_TRACK_MAX_OBJECTS];
  double diam_d[FP_TRACK_MAX_OBJECTS];
  int hyp[FP_TRACK_MAX_OBJECTS], n_solo = 0;
  for (int o = 0; o < N; ++o) {
    pose_in[o] = objs[o].d_pose;
    diam[o] = (float)objs[o].mesh_diameter;
    diam_d[o] = objs[o].mesh_diameter;
    if (solo[o]) mesh[n_solo] = &objs[o].mesh->d, rdiam[n_solo] = diam[o], hyp[n_solo++] = o;
  }
  RenderArgs ra;          // render_net_impl's fields; mesh and diameter come per object
  FP_TRY(fill_render(ra, objs[0].mesh, poses, N, a->K, a->H, a->W, bbox, 160, 160));
  ra.use_light = 1;
  ra.w_ambient = 0.8f;
  ra.w_diffuse = 0.5f;
  ra.net_out = net_in;
  ra.invalid_thres = 0.001f;
  ra.normalize_xyz = cfg->normalize_xyz;
  CropArgs ca;            // fp_crop_observed's fields; the diameter comes per object
  memset(&ca, 0, sizeof(ca));
  ca.rgb = rgb_f, ca.geom = a->d_xyz, ca.tf = tf, ca.poses = poses;
  for (int i = 0; i < 9; ++i) ca.K[i] = a->K[i];
  ca.H = a->H, ca.W = a->W, ca.N = N, ca.Ho = 160, ca.Wo = 160, ca.mode = 0, ca.normalize_xyz = cfg->normalize_xyz, ca.out_fmt = 1;
  ca.out = net_in + (size_t)N * img;
  const bool two_sides = pass_plan(PASS_REFINE, N, 1, N, 0, pass_knobs()).fork_sides;       // the objects share the camera: one run, as in the one-object pass
  for (int it = 0; it < a->iteration; ++it) {
    if (it == 0)         // (from the second iteration on the previous pass' tail has written the windows)
      FP_TRY(launch_crop_window_objects(pose_in, a->K, cfg->crop_ratio, diam_d, N, 160, 160, poses, tf, bbox, s));
    std::unique_ptr<StreamFanout> ab;
    if (two_sides) ab.reset(new StreamFanout(ctx, s, 2));          // forks behind the crop windows
    if (n_solo) FP_TRY(launch_render_objects(ctx, ra, mesh, rdiam, hyp, n_solo, s));
    size_t voff = 0;
    for (int o = 0; o < N; ++o) {
      if (solo[o]) continue;
      const size_t rsb = render_block_bytes(ctx, objs[o].mesh, 1);
      FP_TRY(render_net_impl(ctx, objs[o].mesh, poses + (size_t)o * 16, 1, a->K, a->H, a->W, bbox + (size_t)o * 4, 160, 160, objs[o].mesh_diameter,
                             cfg->normalize_xyz, 0.001f, net_in + (size_t)o * img, rscratch + voff, rsb, s));
      voff += rsb;
    }
    {
      hipStream_t sb = ab ? ab->stream_for(0) : s;
      ProfScope ps(ctx, sb, "crop", (double)N * 160 * 160 * 16.0);      // bytes written
      FP_TRY(launch_crop_observed_objects(ca, diam, sb));
    }
    RefineTailArgs t = fill_refine_tail(cfg, a->K, objs[0].mesh_diameter, tf, bbox, poses, it, a->iteration);
    t.obj.n = N;
    const bool last = it + 1 == a->iteration;
    for (int o = 0; o < N; ++o) {
      t.obj.trans_scale[o] = cfg->normalize_xyz ? (float)(objs[o].mesh_diameter / 2) : 1.f;
      t.obj.radius[o] = crop_window_k(a->K, cfg->crop_ratio, objs[o].mesh_diameter, 160, 160).radius;
      for (int c = 0; c < 3; ++c) t.obj.cneg[o][c] = -objs[o].model_center[c];
      t.obj.centered[o] = last ? objs[o].d_pose_of_mesh : nullptr;
      t.obj.pose_out[o] = last ? objs[o].d_pose : nullptr;
    }
    FP_TRY(fp_refine_forward_ab(ctx, a->refine_net, net_in, N, trans, rot, s, ab.get(), &t, nullptr));
  }
  return FP_OK;
}

extern "C" int fp_track_objects(fp_ctx *ctx, const fp_track_objects_args *a, void *stream) {
  FP_REQUIRE(ctx && a, "fp_track_objects: null argument");
  FP_REQUIRE(a->struct_size == sizeof(fp_track_objects_args), "fp_track_objects: fp_track_objects_args.struct_size = %zu (this library knows %zu)",
             a->struct_size, sizeof(fp_track_objects_args));
  FP_REQUIRE(a->refine_net && a->d_rgb && a->d_depth && a->K && a->refine_cfg && a->objs && a->d_depth_f && a->d_xyz, "fp_track_objects: null field");
  FP_REQUIRE(a->H > 1 && a->W > 1 && a->iteration >= 1, "fp_track_objects: bad H / W / iteration");
  FP_REQUIRE(a->n_obj >= 1 && a->n_obj <= FP_TRACK_MAX_OBJECTS, "fp_track_objects: n_obj = %d (1 .. %d objects)", a->n_obj, FP_TRACK_MAX_OBJECTS);
  FP_REQUIRE(!a->rgb_is_u8 || a->d_rgb_f, "fp_track_objects: a uint8 frame needs the float workspace d_rgb_f");
  for (int o = 0; o < a->n_obj; ++o) {
    const fp_track_object &ob = a->objs[o];
    FP_REQUIRE(ob.mesh && ob.d_pose && ob.d_pose_of_mesh, "fp_track_objects: object %d has a null field", o);
    FP_REQUIRE(ob.mesh_diameter > 0, "fp_track_objects: object %d has a bad mesh_diameter", o);
  }
  FP_REQUIRE(hyp_chunk(a->n_obj, pass_knobs()) == a->n_obj, "fp_track_objects: the chunk knob cuts the pass of %d images (the fused tail needs it whole)", a->n_obj);
  hipStream_t s = (hipStream_t)stream;
  // the depth prelude of fp_track_frame, once for all objects
  double K32[9];
  for (int i = 0; i < 9; ++i) K32[i] = (double)(float)a->K[i];
  FP_TRY(depth_prelude(a->d_depth, a->H, a->W, K32, a->d_depth_f, a->d_xyz, a->rgb_is_u8, a->d_rgb, a->d_rgb_f, s));
  return track_objects_pass(ctx, a, a->rgb_is_u8 ? a->d_rgb_f : (const float *)a->d_rgb, s);
}

// ---- FoundationPose.register for several objects of one frame (fp_register_objects) and its pieces -----------------------------------
static int mask_stats_objects(fp_ctx *ctx, const float *d_depth, const MaskStatsObjs &mo, int H, int W, float min_depth, int32_t *h_stats,
                              float *h_median, hipStream_t s) {
  FP_TRY(fp_arena_ensure(ctx, 4096));
  ArenaScope scope(ctx->arena);      // (released behind the copy and the wait below: host bookkeeping, nothing else takes in between)
  int *d_out = (int *)ctx->arena.take((size_t)mo.n * 8 * sizeof(int));
  FP_REQUIRE(d_out, "mask stats: arena exhausted");
  {
    ProfScope ps(ctx, s, "mask_stats", (double)H * W * mo.n);
    FP_TRY(launch_mask_depth_stats_objects(d_depth, mo, H, W, min_depth, d_out, s));
  }
  int host[FP_TRACK_MAX_OBJECTS * 8];
  FP_CHECK_HIP(hipMemcpyAsync(host, d_out, (size_t)mo.n * 8 * sizeof(int), hipMemcpyDeviceToHost, s));      // ONE copy for all objects
  FP_CHECK_HIP(hipStreamSynchronize(s));
  for (int o = 0; o < mo.n; ++o) {
    for (int i = 0; i < 6; ++i) h_stats[o * 6 + i] = host[o * 8 + i];
    memcpy(h_median + o, &host[o * 8 + 6], sizeof(float));
  }
  return FP_OK;
}

extern "C" int fp_mask_depth_stats_objects(fp_ctx *ctx, const float *d_depth, const uint8_t *const *d_masks, const int32_t *d_labels,
                                           const int32_t *labels, int n_obj, int H, int W, float min_depth, int32_t *h_stats, float *h_median,
                                           void *stream) {
  FP_REQUIRE(ctx && d_depth && h_stats && h_median && H > 0 && W > 0 && (size_t)H * W <= ((size_t)1 << 30), "fp_mask_depth_stats_objects: bad argument");
  FP_REQUIRE(n_obj >= 1 && n_obj <= FP_TRACK_MAX_OBJECTS, "fp_mask_depth_stats_objects: n_obj = %d (1 .. %d objects)", n_obj, FP_TRACK_MAX_OBJECTS);
  FP_REQUIRE(d_labels ? labels != nullptr : d_masks != nullptr, "fp_mask_depth_stats_objects: a label image needs `labels`, otherwise `d_masks`");
  MaskStatsObjs mo;
  memset(&mo, 0, sizeof(mo));
  mo.n = n_obj, mo.labels = d_labels;
  for (int o = 0; o < n_obj; ++o) {
    if (d_labels) {
      mo.label[o] = labels[o];
    } else {
      FP_REQUIRE(d_masks[o], "fp_mask_depth_stats_objects: mask %d is null", o);
      mo.mask[o] = d_masks[o];
    }
  }
  return mask_stats_objects(ctx, d_depth, mo, H, W, min_depth, h_stats, h_median, (hipStream_t)stream);
}

static void fill_hyp_object(RegHypObjs &ho, int k, const float *rot_grid, int n, int off, const int32_t *st6, float median) {
  ho.rot_grid[k] = rot_grid, ho.n[k] = n, ho.off[k] = off;
  ho.cmin[k] = st6[0], ho.cmax[k] = st6[1], ho.rmin[k] = st6[2], ho.rmax[k] = st6[3];
  ho.median[k] = median;
}

extern "C" int fp_register_hypotheses(fp_ctx *ctx, const float *const *d_rot_grids, const int *n_hyp, int n_obj, const int32_t *h_stats,
                                      const float *h_median, const double *K_inv, float *d_poses, void *stream) {
  FP_REQUIRE(ctx && d_rot_grids && n_hyp && h_stats && h_median && K_inv && d_poses, "fp_register_hypotheses: null argument");
  FP_REQUIRE(n_obj >= 1 && n_obj <= FP_TRACK_MAX_OBJECTS, "fp_register_hypotheses: n_obj = %d (1 .. %d objects)", n_obj, FP_TRACK_MAX_OBJECTS);
  RegHypObjs ho;
  memset(&ho, 0, sizeof(ho));
  ho.n_obj = n_obj;
  for (int i = 0; i < 9; ++i) ho.kinv[i] = K_inv[i];
  int off = 0;
  for (int o = 0; o < n_obj; ++o) {
    FP_REQUIRE(n_hyp[o] >= 0 && (n_hyp[o] == 0 || d_rot_grids[o]), "fp_register_hypotheses: object %d has a bad rotation grid", o);
    fill_hyp_object(ho, o, d_rot_grids[o], n_hyp[o], off, h_stats + o * 6, h_median[o]);
    off += n_hyp[o];
  }
  return launch_register_hypotheses(ho, d_poses, (hipStream_t)stream);
}

extern "C" int fp_register_rank(fp_ctx *ctx, const float *d_poses, const float *d_scores, const int *n_hyp, int n_obj, const float *model_centers,
                                float *const *d_poses_out, float *const *d_scores_out, int64_t *const *d_order_out, float *const *d_pose_of_mesh,
                                void *stream) {
  FP_REQUIRE(ctx && d_poses && d_scores && n_hyp && model_centers && d_poses_out && d_scores_out && d_order_out && d_pose_of_mesh,
             "fp_register_rank: null argument");
  FP_REQUIRE(n_obj >= 1 && n_obj <= FP_TRACK_MAX_OBJECTS, "fp_register_rank: n_obj = %d (1 .. %d objects)", n_obj, FP_TRACK_MAX_OBJECTS);
  RegRankObjs ro;
  memset(&ro, 0, sizeof(ro));
  ro.n_obj = n_obj;
  int off = 0;
  for (int o = 0; o < n_obj; ++o) {
    FP_REQUIRE(n_hyp[o] >= 1 && d_poses_out[o] && d_scores_out[o] && d_order_out[o] && d_pose_of_mesh[o], "fp_register_rank: object %d has a null output or no hypothesis", o);
    ro.n[o] = n_hyp[o], ro.off[o] = off;
    ro.poses_out[o] = d_poses_out[o], ro.scores_out[o] = d_scores_out[o], ro.order_out[o] = (long long *)d_order_out[o], ro.pose_of_mesh[o] = d_pose_of_mesh[o];
    for (int c = 0; c < 3; ++c) ro.cneg[o][c] = -model_centers[o * 3 + c];
    off += n_hyp[o];
  }
  return launch_register_rank(ro, d_poses, d_scores, (hipStream_t)stream);
}

extern "C" int fp_register_objects(fp_ctx *ctx, fp_register_objects_args *a, void *stream) {
  FP_REQUIRE(ctx && a, "fp_register_objects: null argument");
  FP_REQUIRE(a->struct_size == sizeof(fp_register_objects_args), "fp_register_objects: fp_register_objects_args.struct_size = %zu (this library knows %zu)",
             a->struct_size, sizeof(fp_register_objects_args));
  FP_REQUIRE(a->refine_net && a->score_net && a->d_rgb && a->d_depth && a->K && a->K_inv && a->refine_cfg && a->objs && a->d_depth_f && a->d_xyz,
             "fp_register_objects: null field");
  FP_REQUIRE(a->H > 1 && a->W > 1 && (size_t)a->H * a->W <= ((size_t)1 << 30) && a->iteration >= 0, "fp_register_objects: bad H / W / iteration");
  FP_REQUIRE(a->n_obj >= 1 && a->n_obj <= FP_TRACK_MAX_OBJECTS, "fp_register_objects: n_obj = %d (1 .. %d objects)", a->n_obj, FP_TRACK_MAX_OBJECTS);
  FP_REQUIRE(!a->rgb_is_u8 || a->d_rgb_f, "fp_register_objects: a uint8 frame needs the float workspace d_rgb_f");
  FP_REQUIRE(a->max_pass_hyp >= 0, "fp_register_objects: bad max_pass_hyp");
  const int n_obj = a->n_obj, cap = a->max_pass_hyp ? a->max_pass_hyp : FP_REGISTER_PASS_HYP;
  MaskStatsObjs mo;
  memset(&mo, 0, sizeof(mo));
  mo.n = n_obj, mo.labels = a->d_labels;
  for (int o = 0; o < n_obj; ++o) {
    const fp_register_object &ob = a->objs[o];
    FP_REQUIRE(ob.mesh && ob.d_rot_grid && ob.d_poses && ob.d_scores && ob.d_order && ob.d_pose_of_mesh, "fp_register_objects: object %d has a null field", o);
    FP_REQUIRE(ob.mesh_diameter > 0 && ob.n_hyp >= 1, "fp_register_objects: object %d has a bad mesh_diameter / n_hyp", o);
    FP_REQUIRE(a->d_labels || ob.d_mask, "fp_register_objects: object %d has no mask and there is no label image", o);
    mo.mask[o] = a->d_labels ? nullptr : ob.d_mask, mo.label[o] = ob.label;
  }
  hipStream_t s = (hipStream_t)stream;
  // the depth prelude of register(), once for all objects: erode -> bilateral (and uint8 -> float colours) in one launch, then the float64
  // back-projection register() uses (Utils.depth2xyzmap), which overwrites the prelude's float32 one
  {
    ProfScope ps(ctx, s, "prelude", (double)a->H * a->W);
    FP_TRY(depth_prelude(a->d_depth, a->H, a->W, a->K, a->d_depth_f, a->d_xyz, a->rgb_is_u8, a->d_rgb, a->d_rgb_f, s));
  }
  FP_TRY(launch_depth2xyz_f64(a->d_depth_f, a->H, a->W, a->K, a->d_xyz, s));
  const float *rgb_f = a->rgb_is_u8 ? a->d_rgb_f : (const float *)a->d_rgb;
  // every object's mask reductions: one launch, one copy, the call's one wait for the stream
  int32_t st[FP_TRACK_MAX_OBJECTS * 6];
  float med[FP_TRACK_MAX_OBJECTS];
  FP_TRY(mask_stats_objects(ctx, a->d_depth_f, mo, a->H, a->W, 0.001f, st, med, s));
  int live[FP_TRACK_MAX_OBJECTS], off[FP_TRACK_MAX_OBJECTS], n_live = 0, N = 0;
  for (int o = 0; o < n_obj; ++o) {
    fp_register_object &ob = a->objs[o];
    for (int i = 0; i < 6; ++i) ob.stats[i] = st[o * 6 + i];
    ob.median = med[o];
    ob.registered = ob.stats[5] >= FP_REGISTER_MIN_VALID;
    for (int r = 0; r < 3; ++r) ob.guess_translation[r] = 0.0;
    if (ob.stats[4] > 0 && ob.stats[5] > 0) {
      const double uc = (ob.stats[0] + ob.stats[1]) / 2.0, vc = (ob.stats[2] + ob.stats[3]) / 2.0;
      for (int r = 0; r < 3; ++r)
        ob.guess_translation[r] = (__builtin_fma(a->K_inv[r * 3], uc, a->K_inv[r * 3 + 1] * vc) + a->K_inv[r * 3 + 2]) * (double)med[o];
    }
    if (ob.registered) live[n_live] = o, off[n_live++] = N, N += ob.n_hyp;
  }
  if (n_live == 0) return FP_OK;
  // network passes: consecutive live objects while the pass stays within `cap` hypotheses; an object of 1 or 2 hypotheses is a pass of its own
  int pass_of[FP_TRACK_MAX_OBJECTS], n_pass = 0;
  size_t pass_bytes = 0;
  for (int k = 0, in_pass = 0; k < n_live; ++k) {
    const int n = a->objs[live[k]].n_hyp;
    const bool alone = n <= 2 || (k > 0 && a->objs[live[k - 1]].n_hyp <= 2);
    if (k == 0 || alone || in_pass + n > cap) ++n_pass, in_pass = 0;
    pass_of[k] = n_pass - 1;
    in_pass += n;
  }
  fp_object_batch batch[FP_TRACK_MAX_OBJECTS];
  for (int k = 0; k < n_live; ++k) {
    const fp_register_object &ob = a->objs[live[k]];
    batch[k] = fp_object_batch{ob.mesh, rgb_f, a->d_xyz, a->H, a->W, a->K, ob.mesh_diameter, ob.n_hyp};
  }
  for (int p = 0, k0 = 0; p < n_pass; ++p) {
    int k1 = k0, np = 0;
    while (k1 < n_live && pass_of[k1] == p) np += batch[k1++].n;
    const size_t need = pass_arena_bytes(np, render_runs(ctx, batch + k0, k1 - k0, nullptr)) + (size_t)(k1 - k0) * ((size_t)4 << 20);
    pass_bytes = need > pass_bytes ? need : pass_bytes;
    k0 = k1;
  }
  // the call's own buffers (hypotheses, features, logits, scores) lie in front of the passes' workspace: sized before anything is taken
  const size_t own = (size_t)N * (16 + 512 + 2) * sizeof(float) + ((size_t)1 << 20);
  const size_t tail_bytes = (size_t)N * (1024 * 4 + 4 * 8) + ((size_t)2 << 20);
  FP_TRY(fp_arena_ensure(ctx, own + (pass_bytes > tail_bytes ? pass_bytes : tail_bytes) + ((size_t)1 << 20)));
  ArenaScope scope(ctx->arena);
  TAKE(hyp, float, (size_t)N * 16);
  TAKE(feats, float, (size_t)N * 512);
  TAKE(logits, float, (size_t)N);
  TAKE(scores, float, (size_t)N);
  RegHypObjs ho;
  memset(&ho, 0, sizeof(ho));
  ho.n_obj = n_live;
  for (int i = 0; i < 9; ++i) ho.kinv[i] = a->K_inv[i];
  for (int k = 0; k < n_live; ++k) fill_hyp_object(ho, k, a->objs[live[k]].d_rot_grid, a->objs[live[k]].n_hyp, off[k], st + live[k] * 6, med[live[k]]);
  FP_TRY(launch_register_hypotheses(ho, hyp, s));
  for (int p = 0, k0 = 0; p < n_pass; ++p) {
    int k1 = k0;
    while (k1 < n_live && pass_of[k1] == p) ++k1;
    float *ph = hyp + (size_t)off[k0] * 16;
    // (every hypothesis of an object has the object's guessed translation: FP_REFINE_SHARED_TRANSLATION holds by construction)
    FP_TRY(refine_predict_impl(ctx, a->refine_net, batch + k0, k1 - k0, a->refine_cfg, ph, a->iteration, nullptr, nullptr, stream, nullptr,
                               FP_REFINE_SHARED_TRANSLATION));
    for (int k = k0; k < k1; ++k) batch[k].d_geom = a->d_depth_f;         // the scorer reads the filtered depth
    FP_TRY(score_features_impl(ctx, a->score_net, batch + k0, k1 - k0, a->score_crop_ratio, a->score_normalize_xyz, ph, feats + (size_t)off[k0] * 512,
                               512, false, stream));
    for (int k = k0; k < k1; ++k) {      // att_cross couples the hypotheses of ONE object: a group of its own length per object
      ScoreTailOut to;
      to.logits = logits + off[k], to.scores = scores + off[k], to.score_offset = 100.f;
      FP_TRY(fp_score_tail_impl(ctx, a->score_net, feats + (size_t)off[k] * 512, 512, 1, batch[k].n, to, s));
    }
    k0 = k1;
  }
  RegRankObjs ro;
  memset(&ro, 0, sizeof(ro));
  ro.n_obj = n_live;
  for (int k = 0; k < n_live; ++k) {
    const fp_register_object &ob = a->objs[live[k]];
    ro.n[k] = ob.n_hyp, ro.off[k] = off[k];
    ro.poses_out[k] = ob.d_poses, ro.scores_out[k] = ob.d_scores, ro.order_out[k] = (long long *)ob.d_order, ro.pose_of_mesh[k] = ob.d_pose_of_mesh;
    for (int c = 0; c < 3; ++c) ro.cneg[k][c] = -ob.model_center[c];
  }
  return launch_register_rank(ro, hyp, scores, s);          // the call's last launch: the results land in the objects' buffers (pinned host: no copy)
}

// ---- building blocks ---------------------------------------------------------------------------------
// What the plan of a stand-alone launch asks for, from the arena (under the caller's ArenaScope; consumed on the stream before anything
// else takes it): the packed copy of the weights its form reads, packed here as a network packs it at load, and the split-K scratch
static int conv_materialise(fp_ctx *ctx, ConvArgs &a, const ConvPlan &plan, hipStream_t s) {
  const size_t bytes = plan.packing ? conv_packed_halfs(plan.packing, a.Cout, a.Cin) * sizeof(f16) : plan.splitk_bytes;
  if (bytes == 0) return FP_OK;
  FP_TRY(fp_arena_ensure(ctx, bytes + 4096));
  void *p = ctx->arena.take(bytes);
  if (!p) return FP_ENOMEM;
  if (!plan.packing) {
    a.splitk = (float *)p;
    return FP_OK;
  }
  (plan.packing == CONV_OFFER_SMALL ? a.wsm : a.wpk) = (const f16 *)p;
  return conv_pack_weights(plan.packing, a.w, a.Cout, a.Cin, a.Kpad, (f16 *)p, s);
}

// one convolution launch on its own: fp16 or fp32 NHWC output, no split, no post-add.  Planned with everything on offer that a network
// holds for a layer but the s1b packing (conv_plan.h: where the callers differ), so that the parity tests reach each form
extern "C" int fp_conv2d_f16(fp_ctx *ctx, const void *d_in, int Nimg, int H, int W, int Cin, const void *d_w_packed, const float *d_bias,
                             int Cout, int KH, int KW, int stride, int pad, const void *d_res, int relu, void *d_out, int out_f32,
                             void *stream) {
  FP_REQUIRE(ctx && d_in && d_w_packed && d_bias && d_out, "fp_conv2d_f16: null argument");
  FP_REQUIRE(stride >= 1 && pad >= 0 && Nimg >= 0, "fp_conv2d_f16: bad stride/pad/N");
  ConvArgs a = conv_args((const f16 *)d_in, Nimg, H, W, Cin, (const f16 *)d_w_packed, d_bias, Cout, KH, KW, stride, pad, conv_kpad(KH, KW, Cin), d_out);
  a.res = (const f16 *)d_res, a.relu = relu, a.out_mode = out_f32 ? 1 : 0;
  ArenaScope scope(ctx->arena);
  const unsigned offer = out_f32 ? 0 : CONV_OFFER_SMALL | CONV_OFFER_S2 | CONV_OFFER_SPLITK;
  FP_TRY(conv_materialise(ctx, a, conv_plan(a, ctx->num_cu, offer, conv_knobs()), (hipStream_t)stream));
  return launch_conv(ctx, a, (hipStream_t)stream);      // (plans again from what `a` now holds: the same form)
}

// Building block for the parity tests: the band-in-LDS form of the C -> C 3x3 stride-1 layers on 40x40 maps (conv_s1b.hip; C = 128 or 256),
// which the networks use for batches of more than 40 hypotheses (more than one round of the general kernel's tiles); same operands as fp_conv2d_f16 (w_packed [C][9 C] fp16).
extern "C" int fp_conv3x3_band_f16(fp_ctx *ctx, const void *d_in, int Nimg, int C, const void *d_w_packed, const float *d_bias, const void *d_res,
                                   int relu, void *d_out, void *stream) {
  FP_REQUIRE(ctx && d_in && d_w_packed && d_bias && d_out && Nimg >= 0, "fp_conv3x3_band_f16: bad argument");
  FP_REQUIRE(C == 128 || C == 256, "fp_conv3x3_band_f16: C=%d (128 or 256)", C);
  ConvArgs a = conv_args((const f16 *)d_in, Nimg, 40, 40, C, (const f16 *)d_w_packed, d_bias, C, 3, 3, 1, 1, conv_kpad(3, 3, C), d_out);
  a.res = (const f16 *)d_res, a.relu = relu;
  if (a.M == 0) return FP_OK;
  const ConvPlan plan = conv_plan(a, ctx->num_cu, CONV_FORCE_S1B, conv_knobs());
  FP_REQUIRE(plan.form == CONV_S1B, "fp_conv3x3_band_f16: %d images are more than the band kernel addresses", Nimg);
  ArenaScope scope(ctx->arena);
  FP_TRY(conv_materialise(ctx, a, plan, (hipStream_t)stream));
  return launch_conv_s1b(ctx, a, (hipStream_t)stream);
}

// Building block for the parity tests: the front end of encodeA as the networks run it from three hypotheses on (front.hip) - the 7x7 stem and the
// 64 -> 128 stride-2 layer in one launch, the stem's output in LDS only.  Operands as fp_conv2d_f16 takes them ([64][416] and [128][576] fp16
// rows, folded biases); the fragment-order copies a network makes at load are made here, in the arena.
extern "C" int fp_front_end_f16(fp_ctx *ctx, const void *d_x, int Nimg, const void *d_w0_packed, const float *d_b0, const void *d_w1_packed,
                                const float *d_b1, void *d_a1, void *d_a0, void *stream) {
  FP_REQUIRE(ctx && d_x && d_w0_packed && d_b0 && d_w1_packed && d_b1 && d_a1 && Nimg >= 0, "fp_front_end_f16: bad argument");
  if (Nimg == 0) return FP_OK;
  hipStream_t s = (hipStream_t)stream;
  ArenaScope scope(ctx->arena);
  const size_t h0 = front_packed_stem_halfs(), h1 = conv_packed_halfs(CONV_OFFER_S2, 128, 64);
  FP_TRY(fp_arena_ensure(ctx, (h0 + h1) * sizeof(f16) + 4096));
  f16 *wst = (f16 *)ctx->arena.take(h0 * sizeof(f16)), *wpk = (f16 *)ctx->arena.take(h1 * sizeof(f16));
  if (!wst || !wpk) return FP_ENOMEM;
  FP_TRY(front_pack_stem((const f16 *)d_w0_packed, conv_kpad(7, 7, 8), wst, s));
  FP_TRY(conv_pack_weights(CONV_OFFER_S2, (const f16 *)d_w1_packed, 128, 64, conv_kpad(3, 3, 64), wpk, s));
  return launch_front(ctx, (const f16 *)d_x, Nimg, wst, d_b0, wpk, d_b1, (f16 *)d_a1, (f16 *)d_a0, s);
}

extern "C" int fp_attention_f16(fp_ctx *ctx, const void *d_qk, const void *d_vt, int B, int T, void *d_out, void *stream) {
  FP_REQUIRE(ctx && d_qk && d_vt && d_out, "fp_attention_f16: null argument");
  return launch_attention(ctx, (const f16 *)d_qk, (const f16 *)d_vt, B, T, (f16 *)d_out, (hipStream_t)stream);
}

// ---- host: mycpp.cluster_poses ------------------------------------------------------------------------
extern "C" int fp_cluster_poses(float angle_diff_deg, float dist_diff_m, const float *in, int n_in, const float *sym, int n_sym,
                                float *out) {
  FP_REQUIRE(in && sym && out && n_in >= 1 && n_sym >= 1, "fp_cluster_poses: bad argument");
  const float radian_thres = angle_diff_deg / 180.0f * (float)M_PI;
  int n_out = 0;
  auto keep = [&](const float *p) {
    memcpy(out + (size_t)n_out * 16, p, 16 * sizeof(float));
    ++n_out;
  };
  keep(in);
  for (int i = 1; i < n_in; ++i) {
    const float *cur = in + (size_t)i * 16;
    bool isnew = true;
    for (int c = 0; c < n_out && isnew; ++c) {
      const float *cl = out + (size_t)c * 16;
      float dx = cl[3] - cur[3], dy = cl[7] - cur[7], dz = cl[11] - cur[11];
      if (std::sqrt(dx * dx + dy * dy + dz * dz) >= dist_diff_m) continue;
      for (int k = 0; k < n_sym; ++k) {
        const float *tf = sym + (size_t)k * 16;
        float R[9];  // rotation block of cur @ tf
        for (int r = 0; r < 3; ++r)
          for (int cc = 0; cc < 3; ++cc) R[r * 3 + cc] = cur[r * 4] * tf[cc] + cur[r * 4 + 1] * tf[4 + cc] + cur[r * 4 + 2] * tf[8 + cc] + cur[r * 4 + 3] * tf[12 + cc];
        float tr = 0.f;  // trace(R * cl_R^T)
        for (int r = 0; r < 3; ++r)
          for (int cc = 0; cc < 3; ++cc) tr += R[r * 3 + cc] * cl[r * 4 + cc];
        float cs = (tr - 1.f) / 2.0f;
        cs = std::fmax(std::fmin(cs, 1.0f), -1.0f);
        if (std::acos(cs) < radian_thres) {
          isnew = false;
          break;
        }
      }
    }
    if (isnew) keep(cur);
  }
  return n_out;
}
