// The front end of encodeA / encoderA as ONE launch: a1 = ConvBNReLU_3x3s2(ConvBNReLU_7x7s2(x)), x = n x 160x160x8 fp16 ->
// a1 = n x 40x40x128 fp16 NHWC (network_modules.py:37-50 via refine_network.py:37-38 / score_network.py:36-37).  The stem's output
// a0 (n x 80x80x64) stays in LDS: as two launches (stem.hip, then the implicit GEMM of conv.hip) it is written once and read back
// 1.7 times over, 1.1 GB of the 1.58 GB those two launches move per network pass of 504 images.
//
// BIT-IDENTICAL to the two launches: the same instruction (v_mfma_f32_32x32x16_f16), accumulators that start at the folded BN bias, the
// K order of each layer (stem: 25 k-steps of two taps, 8 channels per tap, tap 49 zero weights; stride-2 layer: K index =
// tap * 64 + ci in steps of 16, lane half lh holds 8 consecutive k), out-of-image taps read exact zeros, a0 is rounded where
// stem7x7_kernel rounds it ((f16)fmaxf(acc, 0)) and a1 where conv_igemm2_kernel does (max((f16)acc, 0)).
//
// Shape.  512 threads = 8 waves, one workgroup per CU, persistent over tiles (in XCD order: an XCD's workgroups walk neighbouring tiles, whose
// regions share halo rows in its L2).  A tile is 8 rows x 20 columns of a1 (160 pixels = 5 MFMA pixel tiles; 10 tiles per image); it needs
// 17 x 41 pixels of a0 (rows 2 oy0 - 1 .. + 16, columns 2 ox0 - 1 .. + 40; row / column -1 is the stride-2 layer's padding: zeros) and
// 39 x 87 pixels of x.  The stem is recomputed for the halo: 17 x 41 / (16 x 40) = 1.09.  Per tile:
//   1. the input region (39 rows x 89 columns, 16-byte pixels) is in LDS, brought by LDS-DMA; outside the image the source is the zero
//      page.  A region row is two column-parity planes (45 even + 44 odd slots, pitch 93): the region layout of conv_band.h.
//   2. stem phase: the a0 tile as 23 pixel tiles of 32 (17 rows of 42 flattened; column 41 and the tail are computed and dropped) x 64
//      couts; wave w owns cout tile w & 1 and pixel tiles (w >> 1) + 4 j, j < 6: 6 accumulator tiles, 150 MFMAs, one B read per MFMA and
//      one weight fragment per k-step.  2 x pitch = 42 (mod 16): the 32 lanes of a B read cover 32 consecutive 16-byte slots (mod 16) also
//      across a row break - conflict free.  The wave's 25 weight fragments stream L2 -> registers through a buffer descriptor
//      (front_pack_stem's order), four k-steps ahead.  a0 -> LDS in the stride-2 band layout of conv_band.h: four 16-channel planes of 17
//      rows x 42 pixel slots x 32 bytes; written 16 bytes per lane after a v_permlane32_swap of the two lane halves' channel quads.
//   3. the input region is dead: the NEXT tile's region streams into it (issued by waves 4 .. 7) while
//   4. the stride-2 phase runs: wave w owns cout tile w & 3 and pixel tiles {0, 1, 2} (w < 4) or {3, 4}: a SIMD's two waves share one
//      stream of 36 weight fragments (conv_s2.hip's packing with one cout tile per wave, read tap-major, eight k-steps ahead) and issue
//      180 MFMAs together.
//   5. epilogue: per-wave staging through the (dead) a0 planes, 16-byte NHWC stores; the next tile's first stem fragments are requested in
//      front of the stores, and the top of the loop waits by count (wait_vm_lgkm<8>), so nothing waits for the stores.
// LDS: 65536 (input region, 64 DMA instructions of 1 KB) + 91392 (a0 planes) = 156928 bytes.  243 VGPRs, no AGPRs, scratch 0
// (-Rpass-analysis=kernel-resource-usage; 16 SGPRs live in VGPR lanes).
#include "common.h"
#include "conv_band.h"

#define FR_THREADS 512
#define FR_TILES_PER_IMG 10
#define FR_IN_ROWS 39
#define FR_IN_PITCH 93                     // 16-byte slots per region row: 45 even columns, 44 odd ones, 4 unused; 2 x 93 = 42 (mod 16)
#define FR_IN_ODD 45                       // first slot of the odd-column plane
#define FR_IN_COLS 89
#define FR_IN_INSTR 64                     // DMA instructions of 1 KB per region: 8 per wave (39 x 93 = 3627 slots of 4096)
#define FR_IN_BYTES (FR_IN_INSTR * 1024)
#define FR_A0_ROWS 17
#define FR_A0_W 42                         // a0 columns per row as the stem phase walks them (41 used)
#define FR_A0_PIX (FR_A0_ROWS * FR_A0_W)   // 714
#define FR_A0_P 42                         // 32-byte pixel slots per a0 row: 20 even columns + 21 odd ones, 2 P = 20 (mod 16)
#define FR_A0_PLANE (FR_A0_ROWS * FR_A0_P * 32)
#define FR_A0_BYTES (4 * FR_A0_PLANE)
#define FR_LDS_BYTES (FR_IN_BYTES + FR_A0_BYTES)
#define FR_STAGE_LD 40                     // halfs per staged output pixel (32 + 8 pad)
static_assert(FR_IN_ROWS * FR_IN_PITCH <= FR_IN_INSTR * 64 && (2 * FR_IN_PITCH - FR_A0_W) % 16 == 0 && (2 * FR_A0_P - 20) % 16 == 0, "pitches");
static_assert(FR_LDS_BYTES <= 160 * 1024 && 8 * 32 * FR_STAGE_LD * 2 <= FR_A0_BYTES, "LDS budget");

struct FrontArgs {
  const f16 *x;          // [n][160][160][8]
  const f16 *wst;        // stem weights, front_pack_stem's order
  const float *b0;       // [64]
  const f16 *wpk;        // 64 -> 128 weights, s2_pack_weights' order 0 with one cout tile per wave
  const float *b1;       // [128]
  f16 *a1;               // [n][40][40][128]
  f16 *a0_dbg;           // optional [n][80][80][64]: the a0 tiles as the stem phase leaves them (tests)
  const f16 *zero_page;
  int n_tiles;
};

// Stem weights [64][Kpad] -> fragment order [k-step 25][cout tile 2][lane 64][8 halfs]; lane (lr, lh) = W[i*32 + lr][(2s + lh)*8 .. +8]
// (tap 49 = the zero padding of the [Cout][Kpad] rows), as stem7x7_kernel stages them
__global__ void front_pack_stem_kernel(const f16 *__restrict__ w, int Kpad, f16 *__restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 50 * 512) return;
  const int e = idx & 7, lane = (idx >> 3) & 63, f = idx >> 9, s = f >> 1, i = f & 1;
  out[idx] = w[stem_frag_src(Kpad, i, s, lane) + e];
}

// One 1-KB weight fragment through a buffer descriptor: wave-uniform descriptor and fragment offset (scalar registers) + 16 bytes per
// lane, so that the unrolled loops keep no address per fragment in vector registers; a read past `bytes` returns zeros
__device__ __forceinline__ half8 front_frag(__amdgpu_buffer_rsrc_t rsrc, int frag, int lane16) {
  return __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane16, frag * 1024, 0));
}

// The stride-2 phase of one wave: NJ pixel tiles from J0 on x cout tile cg.  `aq`: the first 8 weight fragments, already requested.
template <int NJ, int J0>
__device__ __forceinline__ void front_s2_mma(const FrontArgs &p, const unsigned char *a0s, __amdgpu_buffer_rsrc_t wp, half8 (&aq)[8], const float4 (&bias1)[1][4], floatx16 (&acc)[1][NJ],
                                             int cg, int lane) {
  const int lr = lane & 31, lh = lane >> 5;
  int qb[NJ];                                                           // byte address of (base slot, half lh) before the swizzle
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int pl = 32 * (J0 + j) + lr, jr = pl / 20, ox = pl - jr * 20;
    qb[j] = band_addr(s2_tile_row(jr, 8) * FR_A0_P + ox, lh);           // (8: a tile lies in one image)
  }
  acc_from_bias(acc, bias1);
  // k-step k = tap * 4 + chunk: plane `chunk` of the a0 tile
  auto b_read = [&](int k, int j) __attribute__((always_inline)) -> half8 { return band_read_s2<FR_A0_P, 20>(a0s + (k & 3) * FR_A0_PLANE, qb[j], k >> 2); };
  half8 b[2][NJ];
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int j = 0; j < NJ; ++j) b[d][j] = b_read(d, j);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < 36; ++k) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aq[k & 7], b[k & 1][j], acc[0][j], 0, 0, 0);
      if (k + 2 < 36) b[k & 1][j] = b_read(k + 2, j);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (k + 8 < 36) aq[k & 7] = front_frag(wp, ((k + 8) & 3) * 9 + ((k + 8) >> 2), lane * 16);
    __builtin_amdgcn_sched_barrier(0);
  }
  wait_lgkm();
  __builtin_amdgcn_s_barrier();                                         // every wave is done with the a0 planes: staging may overwrite them
  __builtin_amdgcn_sched_barrier(0);
}

// ---- epilogue: fp16, ReLU (as conv_igemm2_kernel: on the rounded value), one 32-pixel tile at a time through this wave's staging rows ----
template <int NJ, int J0>
__device__ __forceinline__ void front_s2_store(const FrontArgs &p, f16 *stage, const floatx16 (&acc)[1][NJ], int cg, int lane, int img, int oy0, int ox0) {
  const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    band_store_tile<FR_STAGE_LD>(stage, acc, j, lane, lr, lh, RoundThenRelu{}, [&](int px, int c16) {
      const int pl = 32 * (J0 + j) + px, jr = pl / 20, ox = pl - jr * 20;
      const size_t m = ((size_t)img * 40 + oy0 + jr) * 40 + ox0 + ox;
      return BandDst{p.a1 + m * 128 + cg * 32 + c16 * 8};
    });
}

__global__ __launch_bounds__(FR_THREADS, 1) void front_kernel(FrontArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fr_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) void *)fr_smem;
  unsigned char *a0s = fr_smem + FR_IN_BYTES;

  // region of tile t -> LDS: slot q of region row r = input pixel (4 oy0 - 5 + r, 4 ox0 - 5 + j), j = 2 q (q < 45) or 2 (q - 45) + 1.
  // Issued by waves 4 .. 7 only, 16 DMA instructions each: they have two pixel tiles in the stride-2 phase where waves 0 .. 3 have three, and
  // a SIMD's waves 4 + k and k share its issue slots, so the address arithmetic of the one runs under the MFMAs of the other.
  auto load_region = [&](int t) __attribute__((always_inline)) {
    if (wave < 4) return;
    const int img = t / FR_TILES_PER_IMG, r10 = t - img * FR_TILES_PER_IMG;
    const int iyb = 4 * ((r10 >> 1) * 8) - 5, ixb = 4 * ((r10 & 1) * 20) - 5;
    const f16 *src_img = p.x + (size_t)img * 160 * 160 * 8;
    int lv = lane;                                           // opaque per call: the slots' rows and columns are not kept in registers across the tile loop
    asm volatile("" : "+v"(lv));
#pragma unroll
    for (int v = 0; v < FR_IN_INSTR / 4; ++v) {
      const int u = (wave - 4) + 4 * v;
      const int slot = u * 64 + lv, r = slot / FR_IN_PITCH, q = slot - r * FR_IN_PITCH;
      const int iy = iyb + r, ix = ixb + stem_slot_col(FR_IN_ODD, q);
      const bool ok = r < FR_IN_ROWS && q < FR_IN_COLS && iy >= 0 && iy < 160 && ix >= 0 && ix < 160;
      glds16(ok ? src_img + ((size_t)iy * 160 + ix) * 8 : p.zero_page, lds0 + u * 1024);
    }
  };

  // ---- stem phase: wave w owns cout tile w & 1 and the a0 pixel tiles (w >> 1) + 4 j, j < 6, of the flattened 17 x 42 tile (24 slots for 23
  // tiles: the last one and the tail of tile 22 are computed from clamped addresses and not stored) ----
  const int ci = wave & 1, pg = wave >> 1;
  const int cg = wave & 3;
  // this wave's 36 fragments of the stride-2 layer, (chunk, tap) at (chunk * 9 + tap) KB, and the stem's 50
  const __amdgpu_buffer_rsrc_t wp2 = __builtin_amdgcn_make_buffer_rsrc((void *)(p.wpk + (size_t)(cg * 4 * 9) * 512), 0, 36 * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t wst = __builtin_amdgcn_make_buffer_rsrc((void *)p.wst, 0, 50 * 1024, 0x00020000);
  f16 *stage = reinterpret_cast<f16 *>(a0s) + (size_t)wave * (32 * FR_STAGE_LD);
  float4 bias0[1][4];
  bias_quads(bias0, p.b0, ci * 32, lh);
  half8 aw[4];                                               // stem weight ring: k-steps s .. s + 3 of this wave's cout tile
  auto aw_prologue = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int d = 0; d < 4; ++d) aw[d] = front_frag(wst, d * 2 + ci, lane * 16);
  };
  // a0 pixel of (pixel tile slot j, lane): row, column of the 17 x 42 tile and whether it is stored
  auto a0_pixel = [&](int j, int lrv, int *row, int *col) __attribute__((always_inline)) -> bool {
    const int pa_raw = 32 * (pg + 4 * j) + lrv, pa = min(pa_raw, FR_A0_PIX - 1);
    *row = pa / FR_A0_W, *col = pa - *row * FR_A0_W;
    return pa_raw < FR_A0_PIX && *col < 41;
  };

  // tiles in XCD order: the workgroups of one XCD walk neighbouring tiles, whose input regions share halo rows and columns in its L2
  const int tile0 = xcd_remap(blockIdx.x, gridDim.x);
  aw_prologue();
  if (tile0 < p.n_tiles) load_region(tile0);
  bool first = true;
  for (int tile = tile0; tile < p.n_tiles; tile += gridDim.x) {
    const int img = tile / FR_TILES_PER_IMG, r10 = tile - img * FR_TILES_PER_IMG;
    const int oy0 = (r10 >> 1) * 8, ox0 = (r10 & 1) * 20;

    floatx16 acc0[1][6];
    acc_from_bias(acc0, bias0);
    floatx16(&acc)[6] = acc0[0];
    int lrv = lr, lhv = lh;                                  // opaque per tile: what is derived from them does not live in registers across the tile loop
    asm volatile("" : "+v"(lrv), "+v"(lhv));
    unsigned pix_off[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      int row, col;
      (void)a0_pixel(j, lrv, &row, &col);
      pix_off[j] = (unsigned)(stem_pixel_slot(FR_IN_PITCH, row, col) * 16);
    }
    // This tile's region has landed.  First tile: everything this wave has in flight.  Later tiles: the region's DMAs were issued in front
    // of the stride-2 phase's weight loads, which have been consumed (vector-memory operations retire in issue order); behind them are
    // only the 4 stem fragments of aw_prologue and the 4 or 6 output stores of the previous tile, which need not be waited for.  After
    // the barrier every wave's part has landed, and every wave has read its staging rows of the previous tile back.
    if (first) wait_vm_lgkm<0>();
    else wait_vm_lgkm<8>();
    first = false;
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);

    // this lane half's tap of k-step s: tap 2 s, + the step to tap 2 s + 1 in the upper half (tap 49 = zero weights: any slot)
    const int lmask = -lhv;
    auto tap_a = [](int s, int h) { return stem_tap_slots(FR_IN_PITCH, FR_IN_ODD, stem_step_tap(s, h)) * 16; };
    auto b_read = [&](int s, int j) __attribute__((always_inline)) -> half8 {
      const int o0 = tap_a(s, 0), o1 = tap_a(s, 1);
      return *reinterpret_cast<const half8 *>(fr_smem + (pix_off[j] + (unsigned)((o1 - o0) & lmask)) + o0);
    };
    half8 bf[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) bf[j] = b_read(0, j);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 25; ++s) {
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aw[s & 3], bf[j], acc[j], 0, 0, 0);
        if (s + 1 < 25) bf[j] = b_read(s + 1, j);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (s + 4 < 25) aw[s & 3] = front_frag(wst, (s + 4) * 2 + ci, lane * 16);
      __builtin_amdgcn_sched_barrier(0);
    }
    // the stride-2 phase's first weight fragments: requested here, they land behind the a0 writes and the barrier
    half8 aq[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) aq[k] = front_frag(wp2, (k & 3) * 9 + (k >> 2), lane * 16);
    float4 bias1[1][4];                                      // ... and the bias its accumulators start at
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) bias1[0][rg] = *reinterpret_cast<const float4 *>(p.b1 + cg * 32 + rg * 8 + lh * 4); // (bias_quads written out: hipcc moves waits)

    // ---- a0 -> LDS planes: bias + ReLU + fp16 as stem7x7_kernel; zeros where the pixel is the stride-2 layer's padding ----
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      int row, c;
      const bool keep = a0_pixel(j, lrv, &row, &c);
      const int gy = 2 * oy0 - 1 + row, gx = 2 * ox0 - 1 + c;
      const bool inside = gy >= 0 && gx >= 0;
      const int ps = row * FR_A0_P + s2_col_slot(20, c - 1);                       // the slot conv_band.h's stride-2 read expects a0 column 2 ox0 - 1 + c in
      // a lane holds channels rg*8 + lh*4 .. +4 of its pixel: the half exchange of v_permlane32_swap leaves channels (2m)*8 .. +8 in lane
      // (lr, 0) and (2m+1)*8 .. +8 in lane (lr, 1) - the two 16-byte halves of the pixel's slot in plane ci*2 + m, one 16-byte write each
      unsigned char *dst = a0s + band_swizzle(band_addr(ps, lh));
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        half4 h0, h1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          h0[e] = inside ? (f16)fmaxf(acc[j][(2 * m) * 4 + e], 0.f) : (f16)0.f;
          h1[e] = inside ? (f16)fmaxf(acc[j][(2 * m + 1) * 4 + e], 0.f) : (f16)0.f;
        }
        uint2 va = __builtin_bit_cast(uint2, h0), vb = __builtin_bit_cast(uint2, h1);
        auto rx = __builtin_amdgcn_permlane32_swap(va.x, vb.x, false, false);
        auto ry = __builtin_amdgcn_permlane32_swap(va.y, vb.y, false, false);
        const uint4 v = make_uint4(rx[0], ry[0], rx[1], ry[1]);
        if (keep) {
          *reinterpret_cast<uint4 *>(dst + (ci * 2 + m) * FR_A0_PLANE) = v;
          if (p.a0_dbg && inside) *reinterpret_cast<uint4 *>(p.a0_dbg + (((size_t)img * 80 + gy) * 80 + gx) * 64 + ci * 32 + m * 16 + lh * 8) = v;
        }
      }
    }
    wait_lgkm();
    __builtin_amdgcn_s_barrier();                            // the a0 tile is complete; every wave is done with the input region
    __builtin_amdgcn_sched_barrier(0);
    if (tile + (int)gridDim.x < p.n_tiles) load_region(tile + gridDim.x);

    // the next tile's first stem fragments are requested in front of the output stores: waiting for them later does not wait for the stores
    if (wave < 4) {
      floatx16 acc2[1][3];
      front_s2_mma<3, 0>(p, a0s, wp2, aq, bias1, acc2, cg, lane);
      aw_prologue();
      front_s2_store<3, 0>(p, stage, acc2, cg, lane, img, oy0, ox0);
    } else {
      floatx16 acc2[1][2];
      front_s2_mma<2, 3>(p, a0s, wp2, aq, bias1, acc2, cg, lane);
      aw_prologue();
      front_s2_store<2, 3>(p, stage, acc2, cg, lane, img, oy0, ox0);
    }
  }
}

void front_kernel_lds(std::vector<KernelLds> &v) { v.push_back({(const void *)front_kernel, FR_LDS_BYTES}); }

size_t front_packed_stem_halfs() { return (size_t)50 * 512; }

int front_pack_stem(const f16 *d_w, int Kpad, f16 *d_out, hipStream_t s) {
  FP_REQUIRE(Kpad >= 400, "front_pack_stem: Kpad=%d", Kpad);
  hipLaunchKernelGGL(front_pack_stem_kernel, dim3(100), dim3(256), 0, s, d_w, Kpad, d_out);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

int launch_front(fp_ctx *ctx, const f16 *x, int n, const f16 *wst, const float *b0, const f16 *wpk, const float *b1, f16 *a1, f16 *a0_dbg, hipStream_t s) {
  FP_REQUIRE(x && wst && b0 && wpk && b1 && a1 && n >= 0, "launch_front: bad argument");
  FP_REQUIRE((long long)n * FR_TILES_PER_IMG < (1ll << 30), "launch_front: %d images", n);
  if (n == 0) return FP_OK;
  FrontArgs p{x, wst, b0, wpk, b1, a1, a0_dbg, (const f16 *)ctx->zero_page, n * FR_TILES_PER_IMG};
  const int grid = p.n_tiles < ctx->num_cu ? p.n_tiles : ctx->num_cu;
  ProfScope ps(ctx, s, "conv7x7", 2.0 * n * (6400.0 * 64 * 49 * 6 + 1600.0 * 128 * 9 * 64));      // both layers' FLOPs in the stem's class
  hipLaunchKernelGGL(front_kernel, dim3(grid), dim3(FR_THREADS), FR_LDS_BYTES, s, p);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
