// 3x3 / stride-1 / pad-1 convolutions on 40x40 maps - 128 -> 128 (the four ResnetBasicBlock convolutions of encodeA / encoderA) and
// 256 -> 256 (those of encodeAB's first stage; network_modules.py:73-111 via refine_network.py:39-47) - on the structure of conv_s2.hip
// (the band pieces of conv_band.h) instead of conv_halo.hip.
// Bit-identical to conv3x3_halo_dma_kernel<40>: an output element accumulates in the same order - 32-channel groups, inside a group
// kernel row by kernel row, inside a row tap by tap, inside a tap the two 16-channel MFMA steps - from the same bias, and the epilogue
// rounds once after the same fp32 residual add (tests/test_gpu_kernels.py::test_band_kernel_equals_halo_kernel).  Full-batch launches
// (504 images, kernel trace, first form with 16-channel chunks): 215 / 242 us without / with residual against 223 / 247 us.
//
// With four K chunks of 32 channels the 8-wave halo kernel spends 39 % of a workgroup's life in prologue and epilogue, one workgroup
// per CU.  Here
//   * a workgroup (4 waves) owns 8 output rows x 40 = 320 pixels of ONE image (5 tiles per image: no tile straddles two) x a block of
//     128 output channels (the blocks of a pixel tile are neighbours in the grid: they share the band in L2): wave (c, p) owns 64 couts (2 accumulator tiles) x the 160 pixels of rows 4p .. 4p+3 (5 pixel tiles of 32);
//   * per 32-channel group the band goes to LDS once by LDS-DMA as two 16-channel planes (10 input rows x 42 columns of 32-byte
//     pixels each in the stride-1 layout of conv_band.h, row pitch 56 = 40 (mod 16)), double buffered (72 KB), and feeds all 9 taps of both;
//   * weights never touch LDS: packed at load time in MFMA-fragment order (s2_pack_weights, order 1: group, tap, 16-channel half,
//     co tile), each wave streams the fragments of its 64 couts L2 -> registers three steps ahead: 2 KB per 10 MFMAs;
//   * two workgroups per CU (<= 256 VGPRs each).
// Epilogue: accumulators start at the folded BN bias; residual rows staged through LDS and added in fp32, ReLU, one rounding to fp16,
// 16-byte NHWC stores (with the channel-concat addressing of the last encodeA layer: out_ld / split_m / coff_hi).
// Default for the 128 -> 128 layers (FP_C128_BAND=0 sends them back to the halo kernel).  The 256 -> 256 layers take it with FP_C128_BAND=2
// only: bit-identical too, but in an alternating A/B of the bench step 35.54 / 35.66 / 35.60 ms against 35.50 / 35.54 / 35.57 - with
// eight K groups the halo kernel's prologue / epilogue share is small and its weights are shared through LDS (here each cout block
// re-reads the band and each wave streams its own weights).
#include "common.h"
#include "conv_band.h"
#include "conv_tile.h"

#define B1_THREADS 256
// (B1_W = 40, the map edge: conv_plan.h)
#define B1_ROWS 8
#define B1_P 56
#define B1_BROWS (B1_ROWS + 2)
#define B1_PLANE_BYTES (B1_BROWS * B1_P * 32)             // one 16-channel plane of the band: 560 slots of 32 B = 17 920 B (a multiple of 256)
#define B1_BAND_INSTR 36                                  // 1-KB DMA instructions per 32-channel group (two planes = 35 KB), 9 per wave
#define B1_BAND_BYTES (B1_BAND_INSTR * 1024)
#define B1_DPW (B1_BAND_INSTR / 4)
#define B1_NPT 5
#define B1_STAGE_LD 72                                    // halfs per staged pixel: 64 couts + 8 pad
#define B1_LDS_BYTES (2 * B1_BAND_BYTES)

template <bool RES>
__global__ __launch_bounds__(B1_THREADS, 2) void conv3x3_s1_band_kernel(ConvArgs p, const f16 *__restrict__ wpk, const f16 *__restrict__ zero_page, int n_tiles,
                                                                        int n_cob) {
  constexpr int W = B1_W, H = B1_W, P = B1_P, NPT = B1_NPT, DPW = B1_DPW, CT = 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char b1_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  const int ch = wave & 1, ph = wave >> 1;                 // cout half, pixel half
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) void *)b1_smem;
  const int tile = xcd_remap(blockIdx.x, n_tiles);
  const int cob = tile % n_cob, pt = tile / n_cob;          // 128-cout block, pixel tile
  const int img = pt / (H / B1_ROWS), oy0 = (pt - img * (H / B1_ROWS)) * B1_ROWS;
  const int ngrp = p.Cin >> 5;                             // 32-channel groups

  // ---- band DMA (conv_band.h): slot qq of the group's 1120 = plane ks = qq / 560, slot q of the plane; band row b holds input row oy0 - 1 + b ----
  static_assert((B1_BROWS * B1_P) % 16 == 0, "bit 3 of a plane's slot is bit 3 of the group's slot");
  unsigned src_off[DPW];                                   // byte offset of (pixel, plane, logical half) in the input, group 0
  band_dma_offsets(src_off, wave, lane, [&](int qq, int hl) {
    const int ks = qq >= B1_BROWS * P ? 1 : 0;
    const BandSrc s = s1_band_src(P, W, B1_BROWS, oy0, qq - ks * (B1_BROWS * P));
    return s.ok ? (unsigned)((((img * H + s.iy) * W + s.ix) * p.Cin + ks * 16 + hl * 8) * 2) : BAND_ZERO;
  });
  // (written out here and in conv_s2.hip: through a shared helper hipcc allocates the kernels' scalar registers differently)
  auto dma = [&](int grp, int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int v = 0; v < DPW; ++v) {
      const char *src = src_off[v] != BAND_ZERO ? (const char *)p.in + src_off[v] + grp * 64 : (const char *)zero_page;
      glds16(src, lds0 + buf * B1_BAND_BYTES + (wave + 4 * v) * 1024);
    }
  };
  // ---- B fragments: lane = output pixel 32 j + lr of the wave's 160 (local row jr of its 4, column ox), k half lh; band row 4 ph + jr + ky
  // holds input row oy0 + 4 ph + jr + ky - 1 ----
  int qb[NPT];
#pragma unroll
  for (int j = 0; j < NPT; ++j) {
    const int pl = 32 * j + lr, jr = pl / W, ox = pl - jr * W;
    qb[j] = band_addr((4 * ph + jr) * P + ox, lh);
  }
  // ---- A fragments: this wave's stream of 1-KB fragments, (group, tap, 16-channel half, co tile) in order (s2_pack_weights order 1) ----
  WeightRing<CT> ring{reinterpret_cast<const half8 *>(wpk) + ((size_t)(cob * 2 + ch) * ngrp * 18 * CT) * 64 + lane};
  dma(0, 0);
#pragma unroll
  for (int d = 0; d < 3; ++d) ring.fetch(d);

  const int co0 = cob * 128 + ch * 64;
  floatx16 acc[CT][NPT];
  acc_from_bias(acc, p.bias, co0, lh);
  // step st = tap * 2 + ks (tap = ky * 3 + kx): the halo kernel's order inside a 32-channel group
  band_k_loop<18>(acc, ring, ngrp, dma, [&](int buf, int st, int j) __attribute__((always_inline)) {
    return band_read_s1<P>(b1_smem + buf * B1_BAND_BYTES + (st & 1) * B1_PLANE_BYTES, qb[j], st >> 1);
  });

  // ---- epilogue: one 32-pixel tile at a time through this wave's staging rows (32 px x 64 couts) ----
  f16 *stage = reinterpret_cast<f16 *>(b1_smem) + (size_t)wave * (32 * B1_STAGE_LD);
  const float lo = p.relu ? 0.f : -__builtin_inff();
  const int m_wave = (img * H + oy0 + 4 * ph) * W;        // first output pixel of this wave (flattened over images)
#pragma unroll
  for (int j = 0; j < NPT; ++j) {
    if constexpr (RES) {
      // residual rows of the tile: 16-byte pieces, 8 lanes per pixel row of 64 couts -> staging, then added in fp32 in the accumulator layout
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int px = u * 8 + (lane >> 3), c8 = lane & 7;
        const int m = m_wave + 32 * j + px;
        const uint4 rv = *reinterpret_cast<const uint4 *>(p.res + (size_t)m * p.Cout + co0 + c8 * 8);
        *reinterpret_cast<uint4 *>(&stage[px * B1_STAGE_LD + c8 * 8]) = rv;
      }
      wait_vm_lgkm<0>();
    }
    band_store_tile<B1_STAGE_LD>(stage, acc, j, lane, lr, lh, ReluThenRound<RES>{lo}, [&](int px, int c16) {
      const int m = m_wave + 32 * j + px;                 // (the channel-concat addressing of the last encodeA layer)
      return BandDst{ct_out_ptr(p, m) + co0 + c16 * 8};
    });
  }
}

void conv_s1b_kernel_lds(std::vector<KernelLds> &v) {
  v.push_back({(const void *)conv3x3_s1_band_kernel<true>, B1_LDS_BYTES});
  v.push_back({(const void *)conv3x3_s1_band_kernel<false>, B1_LDS_BYTES});
}

int launch_conv_s1b(fp_ctx *ctx, const ConvArgs &a, hipStream_t s) {
  FP_REQUIRE(a.wpk && s1b_supported(a), "launch_conv_s1b: unsupported layer or no packed weights");
  const int n_cob = a.Cout / 128, n_tiles = a.Nimg * (B1_W / B1_ROWS) * n_cob;
  if (a.res) {
    hipLaunchKernelGGL(conv3x3_s1_band_kernel<true>, dim3(n_tiles), dim3(B1_THREADS), B1_LDS_BYTES, s, a, a.wpk, (const f16 *)ctx->zero_page, n_tiles, n_cob);
  } else {
    hipLaunchKernelGGL(conv3x3_s1_band_kernel<false>, dim3(n_tiles), dim3(B1_THREADS), B1_LDS_BYTES, s, a, a.wpk, (const f16 *)ctx->zero_page, n_tiles, n_cob);
  }
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
