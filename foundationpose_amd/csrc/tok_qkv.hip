// In-projections of the transformer heads (gfx950): q, k and v of nn.MultiheadAttention / nn.TransformerEncoderLayer
// (learning/models/refine_network.py:56-70, score_network.py:53-54; packed in_proj_weight (1536, 512) = [Wq; Wk; Wv])
// for up to TG_MAXBLK blocks of 512 output columns that read the SAME tokens - RefineNet: q, k, v of both heads, six blocks.
//
// What bounds a token GEMM on this chip is the weight stream L2 -> registers: tok_gemm.hip's 64-token tile re-streams the 512 KB of a
// 512-column block per 64 tokens, 64 B/clk/CU at the MFMA rate where the path delivers ~30-35 (MI355X_MICROARCH.md: 66-73 GB/s per CU
// from the XCD's L2), and it loads the token tile once per block.  Here
//   * a workgroup (8 waves, one per CU) keeps a tile of 128 tokens x 512 (128 KB) resident in LDS (layouts of the tile, the weight
//     fragments, the accumulators, the stagings and the V image: tok_tile.h) and walks the column blocks over it: the tile is loaded
//     once for all blocks, and a weight fragment (one coalesced 1-KB load per wave) now feeds FOUR MFMAs: 32 B/clk/CU at the MFMA rate;
//   * a wave owns 64 output columns x 128 tokens (2 x 4 accumulator tiles, v_mfma_f32_32x32x16_f16); the K loop has no barrier and no
//     LDS write: per k-step of 16 two weight fragments (prefetched 3 steps ahead), four token fragments, eight MFMAs;
//   * work = (tile, block) units in tile-major order, cut into equal contiguous ranges over the workgroups (at most one per CU): a
//     launch is balanced to one unit whatever M is - 252 hypotheses are 788 tiles x 6 blocks = 18.5 units per CU, 32 hypotheses 100
//     x 6 = 2.3 - and a workgroup reloads the tile only when its range crosses into the next one;
//   * epilogues, per wave and 32-token slice through a private 4-KB staging area (the two waves of a SIMD drift apart: one's epilogue
//     runs beside the other's K loop): fp16 rows as whole 128-byte segments (q | k), or the transposed V image (MFMA operands
//     swapped so that a lane owns a channel and 4 consecutive tokens).
// Arithmetic per output element is that of tok_gemm.hip (bias first, k ascending in steps of 16, one rounding to fp16): bit-identical
// (tests/test_gpu_kernels.py::test_token_qkv_equals_the_64_token_kernel).
#include "common.h"
#include "device_util.h"
#include "tok_tile.h"

#define TQ_ROWS 128
#define TQ_THREADS 512
#define TQ_SEG_BYTES (TQ_ROWS * 256)              // one k segment of 128 of the resident tile: 32 KB
#define TQ_TILE_BYTES (4 * TQ_SEG_BYTES)          // 128 KB
#define TQ_STAGE_BYTES 4096                       // per wave: 32 tokens x 64 columns (rows) / 64 channels x 32 tokens (V image)
#define TQ_LDS_BYTES (TQ_TILE_BYTES + 8 * TQ_STAGE_BYTES)      // 160 KB

// acc[i][j] = bias + tile (tokens j*32 .. +31) x W^T (columns wave*64 + i*32 .. +31).  VT: operands swapped (a lane owns a channel).
template <bool VT>
__device__ __forceinline__ void tq_kloop(const TokGemmBlock &blk, const unsigned char *tile, int wave, int lane, floatx16 (&acc)[2][4]) {
  const int lr = lane & 31, lh = lane >> 5;
  if constexpr (VT) acc_from_bias_vt(acc, blk.bias, wave * 64, lr);
  else acc_from_bias(acc, blk.bias, wave * 64, lh);
  const u32x4 *wp = reinterpret_cast<const u32x4 *>(blk.w) + wfrag_own8(wave, 0, 0) * 64 + lane;
  u32x4 wr[3][2];                         // weight prefetch distance 3 k-steps (4 spills)
  tok_w_prefetch(wr, wp);
  tok_kloop_rot<VT, false>(wr, wp, tile, lr, lh, acc, nullptr);
}

__global__ __launch_bounds__(TQ_THREADS, 1) void tok_qkv_kernel(TokGemmArgs p, int n_units, int units_per_wg) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tq_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) void *)tq_smem;
  unsigned char *stage = tq_smem + TQ_TILE_BYTES + wave * TQ_STAGE_BYTES;
  const int u0 = blockIdx.x * units_per_wg, u1 = min(u0 + units_per_wg, n_units);
  int cur_tile = -1;
  for (int u = u0; u < u1; ++u) {
    const int tile = u / p.nblk, b = u - tile * p.nblk;
    const TokGemmBlock &blk = p.blk[b];
    const int m0 = tile * TQ_ROWS;
    if (tile != cur_tile) {
      __syncthreads();                                     // every wave is done with the previous tile
      tok_tile_dma<TQ_ROWS, 8, true>(p.in, m0, p.M, wave, lane, lds0);
      wait_vm<0>();
      __syncthreads();
      cur_tile = tile;
    }
    floatx16 acc[2][4];
    if (blk.vt) {
      tq_kloop<true>(blk, tq_smem, wave, lane, acc);
      // swapped accumulator layout.  Per 32-token slice: stage [channel][token in vt order] (tq_vt_off), then 16-byte stores along the
      // token axis of the image
      f16 *img = (f16 *)blk.out;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q)       // 4 consecutive tokens inside the slice
            *reinterpret_cast<half4 *>(stage + tq_vt_off(acc_vt_chan(i, lr), vt_col(acc_vt_token(0, q * 4, lh)))) = acc_quad_f16(acc[i][j], q);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int c = v * 16 + (lane >> 2), unit = lane & 3;
          const uint4 val = *reinterpret_cast<const uint4 *>(stage + tq_vt_off(c, unit * 8));
          const int m = m0 + j * 32 + unit * 8;                     // the 8 tokens of a unit lie in one group of 16: one hypothesis
          if (m < p.M) vt_store_unit(img, blk.coff + wave * 64 + c, m, p.tokens, unit & 1, val);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      }
    } else {
      tq_kloop<false>(blk, tq_smem, wave, lane, acc);
      // fp16 rows: per 32-token slice the wave's 64 columns through its staging (tq_stage_off), then whole 128-byte row segments
      const bool relu = blk.relu != 0;
      f16 *obase = (f16 *)blk.out + blk.coff + wave * 64;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            half4 hv = acc_quad_f16(acc[i][j], rg);
            if (relu) hv = relu4(hv);
            *reinterpret_cast<half4 *>(stage + tq_stage_off(lr, acc_row_chan(i, rg, lh))) = hv;
          }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int row = v * 8 + (lane >> 3), unit = lane & 7;
          const uint4 val = *reinterpret_cast<const uint4 *>(stage + tq_stage_off(row, unit * 8));
          const int m = m0 + j * 32 + row;
          if (m < p.M) *reinterpret_cast<uint4 *>(obase + (size_t)m * blk.ld + unit * 8) = val;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      }
    }
  }
}

// The same in-projections for ONE or TWO hypotheses (a tracking frame, src/estimater.py:250-268).  There the kernel above is 24 units on
// 24 CUs, each with 67 MFLOP of its own: 14.6 us, bound by the matrix pipes of a tenth of the chip.  Here a workgroup is (32 tokens,
// block, 128 of its 512 columns) - 13 x 6 x 4 = 312 per hypothesis, two per CU - and its 8 waves are 4 quarters of K x 2 halves of the
// columns: 16 weight fragments per wave (coalesced 1-KB loads of pack_tok_weights' image, all requested up front), the token tile -
// 32 KB, contiguous - copied to LDS once (row pitch 512 + 8 halfs), 16 MFMAs, the four K quarters added through LDS in order, bias,
// and the rows or the transposed V image written as the kernel above writes them.  K in four quarters: a summation order of its own (the
// few-image size class, like conv_small.hip), not the bit pattern of tok_gemm.hip.
#define TS_PITCH 520                               // halfs per token row in LDS
#define TS_PLD 132                                 // floats per token row of a partial tile (128 columns + 4)
#define TS_LDS_BYTES (4 * 32 * TS_PLD * 4)         // 4 K quarters x 32 tokens x 128 columns fp32 (67.6 KB); the token tile (33 KB) lies in the same bytes first
__global__ __launch_bounds__(512, 2) void tok_qkv_small_kernel(TokGemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ts_smem[];
  f16 *tile = reinterpret_cast<f16 *>(ts_smem);
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 31, lh = lane >> 5;
  const int kq = w & 3, chh = w >> 2;                        // K quarter, column half (64 columns: fragments i = 2 chh, 2 chh + 1)
  const int g = blockIdx.x & 3, b = (blockIdx.x >> 2) % p.nblk, tl = (blockIdx.x >> 2) / p.nblk;
  const TokGemmBlock &blk = p.blk[b];
  const int m0 = tl * 32;
  // weights: this wave's 16 fragments (column quarter g, K quarter kq, column half chh)
  u32x4 wf[8][2];
  {
    // (wfrag is linear in its arguments: the wave-uniform and the per-wave part as two terms; as one term: one more lgkmcnt wait)
    const u32x4 *wp = reinterpret_cast<const u32x4 *>(blk.w) + wfrag_own_small(g, kq, 0, 0, 0) * 64 + wfrag_own_small(0, 0, chh, 0, 0) * 64 + lane;
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int i = 0; i < 2; ++i) wf[k][i] = wp[wfrag(0, k, i) * 64];
  }
  // the token tile: rows m0 .. m0 + 31 (rows past M repeat the last one), 2048 pieces of 16 bytes
  {
    u32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + u * 512, row = i >> 6, c8 = i & 63;
      v[u] = *reinterpret_cast<const u32x4 *>(p.in + (size_t)min(m0 + row, p.M - 1) * 512 + c8 * 8);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + u * 512, row = i >> 6, c8 = i & 63;
      *reinterpret_cast<u32x4 *>(tile + row * TS_PITCH + c8 * 8) = v[u];
    }
  }
  wait_lgkm();           // (not a __syncthreads(): the weight loads stay in flight)
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  floatx16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const half8 tf = *reinterpret_cast<const half8 *>(tile + lr * TS_PITCH + (kq * 8 + k) * 16 + lh * 8);
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<half8 *>(&wf[k][i]), tf, acc[i], 0, 0, 0);
  }
  __syncthreads();                                              // the tile is read: its bytes take the partial sums [K quarter][token][column]
  float *part = reinterpret_cast<float *>(ts_smem);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg)
      *reinterpret_cast<float4 *>(part + ((size_t)kq * 32 + lr) * TS_PLD + chh * 64 + i * 32 + rg * 8 + lh * 4) =
          make_float4(acc[i][rg * 4 + 0], acc[i][rg * 4 + 1], acc[i][rg * 4 + 2], acc[i][rg * 4 + 3]);
  __syncthreads();
  const int cbase = blk.coff + g * 128;
  if (!blk.vt) {
    // rows: thread = (token tid / 16, 8 columns): the four quarters in order, bias, ReLU, one 16-byte store
    const int tk = tid >> 4, c8 = (tid & 15) * 8, m = m0 + tk;
    if (m >= p.M) return;
    float v8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v8[e] = part[(size_t)tk * TS_PLD + c8 + e];
#pragma unroll
    for (int q = 1; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 8; ++e) v8[e] += part[((size_t)q * 32 + tk) * TS_PLD + c8 + e];
    half8 hv;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float x = v8[e] + blk.bias[g * 128 + c8 + e];
      if (blk.relu) x = fmaxf(x, 0.f);
      hv[e] = (f16)x;
    }
    *reinterpret_cast<half8 *>((f16 *)blk.out + (size_t)m * blk.ld + cbase + c8) = hv;
    return;
  }
  // transposed V image: thread = (channel tid & 127, group of 16 tokens (tid >> 7) & 1), threads 0 .. 255; a group lies in one hypothesis
  if (tid >= 256) return;
  const int ch = tid & 127, grp = tid >> 7, mg = m0 + grp * 16;
  if (mg >= p.M) return;
  const int bb = mg / p.tokens, t0 = mg - bb * p.tokens;          // t0 is a multiple of 16
  const int col = cbase + ch, hh = col >> 7, d = col & 127;
  const float bias = blk.bias[g * 128 + ch];
  half8 lo, hi;                                                   // image order of a group of 16: tokens 0-3, 8-11 | 4-7, 12-15
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int row = grp * 16 + t;
    float x = part[(size_t)row * TS_PLD + ch];
#pragma unroll
    for (int q = 1; q < 4; ++q) x += part[((size_t)q * 32 + row) * TS_PLD + ch];
    const f16 hx = (f16)(x + bias);
    const int pos = vt_col(t);
    if (pos < 8) lo[pos] = hx;
    else hi[pos - 8] = hx;
  }
  // (tok_tile.h's vt_row and vt_store_unit written out: either one moves this kernel's lgkmcnt waits; two calls of the latter are 9 more stores)
  f16 *rowp = (f16 *)blk.out + (((size_t)bb * 4 + hh) * 128 + d) * 416;
  *reinterpret_cast<half8 *>(rowp + t0) = lo;
  *reinterpret_cast<half8 *>(rowp + t0 + 8) = hi;
  if (t0 + 16 == p.tokens)                                        // the image is 416 tokens wide: zeros behind a hypothesis' last tokens
    for (int z = p.tokens; z < 416; z += 8) *reinterpret_cast<uint4 *>(rowp + z) = uint4{0u, 0u, 0u, 0u};
}

void tok_qkv_kernel_lds(std::vector<KernelLds> &v) {
  v.push_back({(const void *)tok_qkv_kernel, TQ_LDS_BYTES});
  v.push_back({(const void *)tok_qkv_small_kernel, TS_LDS_BYTES});
}

int launch_tok_qkv(fp_ctx *ctx, const TokGemmArgs &a, hipStream_t s, int hyp) {
  FP_TRY(tok_check_args("tok_qkv", a, TOK_OUT_BLK, 64));
  if (a.M == 0) return FP_OK;
  ProfScope ps(ctx, s, "linear", 2.0 * (double)a.M * 512.0 * 512.0 * a.nblk);
  if (qkv_form(hyp, hyp, pass_knobs()) == QKV_SMALL) {          // (the 64-token pair is two launch_tok_gemm launches: run_qkv, net.hip)
    hipLaunchKernelGGL(tok_qkv_small_kernel, dim3(((a.M + 31) / 32) * a.nblk * 4), dim3(512), TS_LDS_BYTES, s, a);
    FP_CHECK_HIP(hipGetLastError());
    return FP_OK;
  }
  const int n_tiles = (a.M + TQ_ROWS - 1) / TQ_ROWS, n_units = n_tiles * a.nblk;
  int n_wg = n_units < ctx->num_cu ? n_units : ctx->num_cu;
  const int upw = (n_units + n_wg - 1) / n_wg;
  n_wg = (n_units + upw - 1) / upw;
  hipLaunchKernelGGL(tok_qkv_kernel, dim3(n_wg), dim3(TQ_THREADS), TQ_LDS_BYTES, s, a, n_units, upw);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
