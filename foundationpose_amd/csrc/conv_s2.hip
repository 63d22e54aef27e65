// 3x3 / stride-2 / pad-1 convolution onto 20x20 maps (encodeAB.2: 256 -> 512 at 40x40 -> 20x20; ConvBNReLU,
// network_modules.py:37-50 via refine_network.py:46 / score_network.py:45) for gfx950 with the input BAND of an output tile resident
// in LDS.
//
// The implicit-GEMM kernel of conv.hip gathers every tap of every output pixel separately (each input pixel is staged 2.25 times
// per 128-cout block through LDS-DMA, 85 FLOP per staged byte) and is bound by that fill.  Here
//   * a workgroup (4 waves) owns 160 consecutive output pixels (8 rows of 20, flattened over images: a tile may straddle two
//     images) x 256 (or 128) output channels; wave w owns 64 (32) couts x ALL 160 pixels = CT x 5 accumulator tiles of
//     v_mfma_f32_32x32x16_f16;
//   * per 16-channel input chunk the band of input rows the tile needs (<= 18 rows x 41 columns of 32-byte pixels = 24 KB) goes to
//     LDS ONCE by LDS-DMA, double buffered, and feeds all 9 taps, in the stride-2 layout of conv_band.h (two column-parity planes per band
//     row, swizzled halves, 2P = W_out (mod 16): conflict-free ds_read_b128, but for a 16-lane group that spans two images of a tile);
//   * the waves split the output channels and nothing else, so no weight is shared between waves: weights never touch LDS.  They are
//     packed at load time in MFMA-fragment order (s2_pack_weights) and each wave streams its own fragments L2 -> registers with
//     coalesced 1-KB loads, three taps ahead;
//   * the B fragment of (tap t + 1, pixel tile j) is read right behind the MFMAs of (tap t, tile j): five MFMA pairs hide its latency;
//   * two workgroups share a CU (48 KB LDS, <= 256 VGPRs each): one's chunk loop runs beside the other's prologue / epilogue.
// Epilogue: accumulators start at the folded BN bias, ReLU, fp16, staged per wave through the (free) band buffers, 16-byte NHWC stores.
// The accumulation order of an output element (chunks in order, taps in order, 16 channels per step) does not depend on the tile.
// The 64 -> 128 layer onto 40x40 maps stays on the implicit-GEMM kernel: the same form (4 rows of 40, P = 84) was measured 226 against
// 208 us in a bench step - a 16-channel chunk pass touches every 128-byte line of the band and uses 32 bytes of it, and with Cin = 64 the
// bands in flight on an XCD (64 workgroups x 104 KB of lines) overflow its 4-MB L2 before the other three chunks come by.
#include "common.h"
#include "conv_band.h"

#define S2_THREADS 256
#define S2_STAGE_PAD 8

template <int WO, int ROWS, int CT>
struct S2Cfg {
  static constexpr int P = 42;                                         // band row pitch in 32-byte pixel slots: WO even + (WO + 1) odd columns, 2P = WO (mod 16)
  static_assert(WO == 20, "pitch chosen for 20-wide outputs");
  static constexpr int BROWS = 2 * ROWS + 2;                           // + 1 for the zero row between two images inside a tile
  static constexpr int NPT = ROWS * WO / 32;                           // pixel tiles of 32
  static constexpr int BAND_INSTR = ((BROWS * P + 31) / 32 + 3) / 4 * 4;   // 1-KB DMA instructions per chunk (a multiple of the 4 waves)
  static constexpr int BAND_BYTES = BAND_INSTR * 1024;
  static constexpr int DPW = BAND_INSTR / 4;
  static constexpr int STAGE_LD = CT * 32 + S2_STAGE_PAD;              // halfs per staged output pixel
  static constexpr int LDS_BYTES = 2 * BAND_BYTES;
  static_assert(ROWS * WO == NPT * 32 && (2 * P - WO) % 16 == 0 && P >= 2 * WO + 1, "tile / pitch");
  static_assert(4 * 32 * STAGE_LD * 2 <= BAND_BYTES, "epilogue staging fits one band buffer");
};

// Fragment order: [cout block][wave 4][chunk Cin/16][tap 9][co tile CT][lane 64][8 halfs]; lane (lr, lh) of a fragment holds
// W[co = ((cb*4 + wave)*CT + ct)*32 + lr][k = tap*Cin + chunk*16 + lh*8 .. +8] of the [Cout][Kpad] image (K index = tap*Cin + ci).
// order 1 (conv_s1b.hip): [wave group][32-channel group][tap 9][16-channel half 2][co tile CT][lane][8 halfs]
__global__ void s2_pack_kernel(const f16 *__restrict__ w, int Cin, int Kpad, int CT, size_t total, f16 *__restrict__ out, int order) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int e = idx & 7, lane = (idx >> 3) & 63;
  size_t rest = idx >> 9;
  const int nch = Cin / 16;
  const int ct = rest % CT;
  rest /= CT;
  int tap, chunk;
  if (order == 1) {
    const int ks = rest % 2;
    rest /= 2;
    tap = rest % 9;
    rest /= 9;
    chunk = (int)(rest % (nch / 2)) * 2 + ks;
    rest /= nch / 2;
  } else {
    tap = rest % 9;
    rest /= 9;
    chunk = rest % nch;
    rest /= nch;                                                        // = cb*4 + wave
  }
  const int co = ((int)rest * CT + ct) * 32 + (lane & 31);
  const int k = tap * Cin + chunk * 16 + (lane >> 5) * 8 + e;
  out[idx] = w[(size_t)co * Kpad + k];
}

template <int WO, int ROWS, int CT>
__global__ __launch_bounds__(S2_THREADS, 2) void conv3x3_s2_kernel(ConvArgs p, const f16 *__restrict__ wpk, const f16 *__restrict__ zero_page,
                                                                    int n_tiles, int n_cob) {
  using C = S2Cfg<WO, ROWS, CT>;
  constexpr int HO = WO, HI = 2 * WO, WI = 2 * WO, P = C::P, NPT = C::NPT, DPW = C::DPW;
  extern __shared__ __attribute__((aligned(16))) unsigned char s2_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) void *)s2_smem;

  const int tile = xcd_remap(blockIdx.x, n_tiles);
  const int cb = tile % n_cob, pt = tile / n_cob;                       // the cout blocks of a pixel tile are neighbours: they share the band in L2
  const int g0 = pt * ROWS;                                             // first flattened output row (image * HO + oy)
  const int img0 = g0 / HO, oy0 = g0 - img0 * HO;
  const int jb = HO - oy0;                                              // first local row that belongs to the next image (>= ROWS: none)
  const int nch = p.Cin >> 4;

  // ---- band DMA (conv_band.h): band row b <= 2 jb holds input row 2 oy0 + b - 1 of image img0; b > 2 jb row b - 2 jb - 2 of image img0 + 1 ----
  unsigned src_off[DPW];                                                // byte offset of (pixel, logical half) in the input, chunk 0
  band_dma_offsets(src_off, wave, lane, [&](int q, int hl) {
    const BandSrc s = s2_band_src(P, WO, C::BROWS, oy0, jb, p.Nimg - img0, q);
    return s.ok ? (unsigned)(((((img0 + s.img) * HI + s.iy) * WI + s.ix) * p.Cin + hl * 8) * 2) : BAND_ZERO;
  });
  // (written out here and in conv_s1b.hip: through a shared helper hipcc allocates this kernel's scalar registers differently)
  auto dma = [&](int ch, int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int v = 0; v < DPW; ++v) {
      const char *src = src_off[v] != BAND_ZERO ? (const char *)p.in + src_off[v] + ch * 32 : (const char *)zero_page;
      glds16(src, lds0 + buf * C::BAND_BYTES + (wave + 4 * v) * 1024);
    }
  };

  // ---- B fragments: lane = output pixel 32 j + lr of the tile (local row jr, column ox), k half lh ----
  int qb[NPT];                                                          // byte address of (base slot, half lh) before the swizzle
#pragma unroll
  for (int j = 0; j < NPT; ++j) {
    const int pl = 32 * j + lr, jr = pl / WO, ox = pl - jr * WO;
    qb[j] = band_addr(s2_tile_row(jr, jb) * P + ox, lh);
  }

  // ---- A fragments: this wave's stream of 1-KB fragments, (chunk, tap, co tile) in order ----
  WeightRing<CT> ring{reinterpret_cast<const half8 *>(wpk) + ((size_t)(cb * 4 + wave) * nch * 9 * CT) * 64 + lane};

  dma(0, 0);
#pragma unroll
  for (int d = 0; d < 3; ++d) ring.fetch(d);

  const int co0 = (cb * 4 + wave) * CT * 32;
  floatx16 acc[CT][NPT];
  acc_from_bias(acc, p.bias, co0, lh);
  // conv_band.h's band_k_loop<9> written out: through the helper hipcc lays this kernel's chunk loop out differently and allocates other registers
  for (int ch = 0; ch < nch; ++ch) {
    wait_vm_lgkm<0>();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (ch + 1 < nch) dma(ch + 1, (ch + 1) & 1);
    const unsigned char *band = s2_smem + (ch & 1) * C::BAND_BYTES;
    half8 b[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) b[j] = band_read_s2<P, WO>(band, qb[j], 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
      for (int j = 0; j < NPT; ++j) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[ct][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ring.aq[t % 3][ct], b[j], acc[ct][j], 0, 0, 0);
        if (t < 8) b[j] = band_read_s2<P, WO>(band, qb[j], t + 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      ring.fetch(t % 3);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  wait_vm_lgkm<0>();
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  // ---- epilogue: ReLU, fp16, one 32-pixel tile at a time through this wave's staging rows, 16-byte NHWC stores ----
  f16 *stage = reinterpret_cast<f16 *>(s2_smem) + (size_t)wave * (32 * C::STAGE_LD);
  const size_t m0 = (size_t)g0 * WO;
#pragma unroll
  for (int j = 0; j < NPT; ++j)
    band_store_tile<C::STAGE_LD>(stage, acc, j, lane, lr, lh, ReluThenRound<>{p.relu ? 0.f : -__builtin_inff()}, [&](int px, int c16) {
      const size_t m = m0 + 32 * j + px;
      return BandDst{(f16 *)p.out + m * p.Cout + co0 + c16 * 8, m < (size_t)p.M};
    });
}

size_t s2_packed_halfs(int Cout, int Cin) { return (size_t)Cout * 9 * Cin + 3 * 2 * 512; }    // + three taps of prefetch past the end

int s2_pack_weights(const f16 *d_w, int Cout, int Cin, int Kpad, f16 *d_out, hipStream_t s, int ct_force, int order) {
  const int ct = ct_force ? ct_force : s2_ct_for(Cout);
  FP_REQUIRE(ct != 0 && Cin % 16 == 0 && Kpad >= 9 * Cin && (order == 0 || Cin % 32 == 0), "s2_pack_weights: unsupported layer");
  const size_t total = (size_t)Cout * 9 * Cin;
  FP_CHECK_HIP(hipMemsetAsync(d_out + total, 0, (s2_packed_halfs(Cout, Cin) - total) * sizeof(f16), s));
  hipLaunchKernelGGL(s2_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_w, Cin, Kpad, ct, total, d_out, order);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

template <int WO, int ROWS, int CT>
static int s2_launch(fp_ctx *ctx, const ConvArgs &a, const f16 *wpk, hipStream_t s) {
  using C = S2Cfg<WO, ROWS, CT>;
  const int rows = a.Nimg * WO, n_pt = (rows + ROWS - 1) / ROWS, n_cob = a.Cout / (128 * CT), n_tiles = n_pt * n_cob;
  hipLaunchKernelGGL((conv3x3_s2_kernel<WO, ROWS, CT>), dim3(n_tiles), dim3(S2_THREADS), C::LDS_BYTES, s, a, wpk, (const f16 *)ctx->zero_page, n_tiles,
                     n_cob);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

void conv_s2_kernel_lds(std::vector<KernelLds> &v) {
  v.push_back({(const void *)conv3x3_s2_kernel<20, 8, 2>, S2Cfg<20, 8, 2>::LDS_BYTES});
  v.push_back({(const void *)conv3x3_s2_kernel<20, 8, 1>, S2Cfg<20, 8, 1>::LDS_BYTES});
}

int launch_conv_s2(fp_ctx *ctx, const ConvArgs &a, hipStream_t s) {
  FP_REQUIRE(a.wpk && s2_supported(a), "launch_conv_s2: unsupported layer or no packed weights");
  return s2_ct_for(a.Cout) == 2 ? s2_launch<20, 8, 2>(ctx, a, a.wpk, s) : s2_launch<20, 8, 1>(ctx, a, a.wpk, s);
}
