// Token GEMM for the transformer heads (gfx950): every nn.Linear that acts on the (N*400, 512) token tensor -
// the q/k/v in-projections, the attention out-projection, linear1 and linear2 of nn.TransformerEncoderLayer
// (learning/models/refine_network.py:56-70, score_network.py:53-54) - with the residual add, the LayerNorm
// and the token mean that follow them fused into the epilogue.
//
//   out[m][c] = sum_k x[m][k] * W[c][k] + b[c]            K = 512, 512 output columns per workgroup
//
// A 1x1 layer has no spatial reuse: in the implicit-GEMM kernel of conv.hip both operands stream through LDS-DMA and the
// L2 -> LDS fill (25 B/clk/CU measured) bounds the K loop at half the MFMA rate, with a workgroup barrier per K-step.
// Here
//   * the ACTIVATION tile (64 tokens x 512 = 64 KB) is brought into LDS ONCE (LDS-DMA; the swizzled layout, the weight-fragment
//     image, the accumulator and V image layouts and the pieces shared with tok_qkv.hip / head_mlp.hip: tok_tile.h) and stays
//     resident for the whole K loop;
//   * the WEIGHTS never touch LDS: each of the 4 waves owns 128 output columns and loads its MFMA fragments straight
//     from global memory / L2 into registers (one coalesced 1-KB global_load_dwordx4 per fragment), prefetched TG_D k-steps ahead;
//   * so the K loop has NO barrier and no LDS write: per k-step of 16 a wave issues 4 global loads, 2 ds_read_b128 and
//     8 v_mfma_f32_32x32x16_f16 (128 columns x 64 tokens = 4 x 2 accumulator tiles, 128 VGPRs);
//   * TWO workgroups share a CU (76 KB of LDS, <= 256 VGPRs each): the three phases of a workgroup's life - tile load
//     (HBM read), K loop (MFMA) and epilogue (LDS transpose + HBM write) - take about the same time (stamps of the first form,
//     one 8-wave workgroup per CU with a 128-token tile: 15k / 15k / 10-48k cycles) and use different units, so one
//     workgroup's K loop runs beside the other's load or epilogue instead of after it.
// Epilogues (compile-time):
//   EPI_ROWS   bias (+ReLU) -> fp16 rows (q|k projection, linear1)
//   EPI_VT     bias -> transposed V image; the MFMA operands are swapped for this one so that a lane owns one channel and 4
//              consecutive tokens per register quad
//   EPI_LN     bias + residual (fp32) -> LayerNorm over the 512 columns (two-pass statistics in fp32 on the accumulators,
//              cross-wave through LDS) -> fp16 rows (out-projection + norm1)
//   EPI_LNSUM  the same LayerNorm, but instead of the rows only their sums over groups of 16 tokens are written (fp32):
//              norm2 feeds nothing but the token mean (refine_network.py:90-91); 16 divides 400, so a group never spans two
//              hypotheses and the reduction order of a hypothesis does not depend on where it sits in the batch.
// The residual stream and the LayerNorm inputs stay fp32 (the reference's autocast keeps them fp32 as well: `x + pe`
// promotes, layer_norm runs in fp32); only GEMM operands are fp16.
#include "common.h"
#include "device_util.h"
#include "tok_tile.h"

#define TG_ROWS 64
#define TG_THREADS 256
#define TG_LDS_BYTES 77824                      // 76 KB: two workgroups per CU.  Tile 64 KB; the epilogue staging (68 - 72 KB) re-uses it
#define TG_RED_OFF 73728                        // reduction scratch [2][4 waves][64] floats behind the staging

enum { EPI_ROWS = TG_EPI_ROWS, EPI_VT = TG_EPI_VT, EPI_LN = TG_EPI_LN, EPI_LNSUM = TG_EPI_LNSUM };

#ifdef HALO_STAMP
// diagnostic build only (make -B EXTRA=-DHALO_STAMP): s_memtime per wave at entry / tile resident / K loop done / exit
__device__ unsigned long long g_tok_stamps[2048 * 4 * 4];
extern "C" __attribute__((visibility("default"))) int fp_dbg_tok_stamps(unsigned long long *host) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_tok_stamps), sizeof(g_tok_stamps)) == hipSuccess ? 0 : -1;
}
#define TSTAMP(i) do { if (blockIdx.x < 2048 && lane == 0) g_tok_stamps[((size_t)blockIdx.x * 4 + wave) * 4 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define TSTAMP(i) do { } while (0)
#endif

template <int EPI>
__global__ __launch_bounds__(TG_THREADS, 2) void tok_gemm_kernel(TokGemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tg_smem[];
  const int L = xcd_remap(blockIdx.x, gridDim.x);          // workgroups that share an XCD's L2 walk the column blocks of one row tile
  const int rt = L / p.nblk, cb = L - rt * p.nblk;
  const TokGemmBlock &blk = p.blk[cb];
  const int m0 = rt * TG_ROWS;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) void *)tg_smem;
  TSTAMP(0);
  tok_tile_dma<TG_ROWS, 4>(p.in, m0, p.M, wave, lane, lds0);

  // ---- this wave's weight fragments; accumulators start at the bias (device_util.h's acc_from_bias / acc_from_bias_vt written out:
  // through the calls hipcc allocates this kernel's registers differently) ----
  const u32x4 *wp = reinterpret_cast<const u32x4 *>(blk.w) + wfrag_own4(wave, 0, 0) * 64 + lane;
  floatx16 acc[4][2];
  if constexpr (EPI == EPI_VT) {          // swapped operands: a lane owns ONE channel (i*32 + lr) of the wave's 128
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float b = blk.bias[wave * 128 + i * 32 + lr];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = b;
    }
  } else {                                // a lane owns one token and channels i*32 + rg*8 + lh*4 + (0..3)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const float4 bv = *reinterpret_cast<const float4 *>(blk.bias + wave * 128 + i * 32 + rg * 8 + lh * 4);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j][rg * 4 + 0] = bv.x;
          acc[i][j][rg * 4 + 1] = bv.y;
          acc[i][j][rg * 4 + 2] = bv.z;
          acc[i][j][rg * 4 + 3] = bv.w;
        }
      }
  }
  constexpr int TG_D = (EPI == EPI_LN || EPI == EPI_LNSUM) ? 3 : 4;   // weight prefetch distance in k-steps of 16 (3 where the
                                                                        // LayerNorm epilogue needs the registers: no spills)
  u32x4 wr[TG_D][4];
  tok_w_prefetch(wr, wp);

  unsigned xo[8];                          // token fragments: the table form of tok_tile.h
#pragma unroll
  for (int s = 0; s < 8; ++s) xo[s] = (unsigned)tile_frag_xo(s, lr, lh);

  wait_vm<0>();      // tile (and the first weight fragments) landed
  __syncthreads();
  TSTAMP(1);

  tok_kloop_db<4, TG_D, EPI == EPI_VT>(wr, wp, tg_smem + lr * 256, xo, acc);

  TSTAMP(2);
  __syncthreads();                                       // every wave is done with the tile: the epilogues re-use its LDS
  float *red = reinterpret_cast<float *>(tg_smem + TG_RED_OFF);

  if constexpr (EPI == EPI_VT) {
    // swapped accumulator layout: stage as [channel][token in vt order] (row = 64 tokens = 128 B + pad), then 16-byte stores along
    // the token axis of the image
    f16 *vs = reinterpret_cast<f16 *>(tg_smem) + (size_t)wave * (128 * TG_VT_LD);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)       // 4 consecutive tokens (tile-relative; the tile starts at a multiple of 16)
          *reinterpret_cast<half4 *>(&vs[tg_vt_off(acc_vt_chan(i, lr), vt_col(acc_vt_token(j, q * 4, lh)))]) = acc_quad_f16(acc[i][j], q);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    // read back: instruction u covers 8 channel rows x 8 chunks of 8 tokens
    f16 *img = (f16 *)blk.out;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int c = u * 8 + (lane >> 3), ch8 = lane & 7;
      const uint4 v = *reinterpret_cast<const uint4 *>(&vs[tg_vt_off(c, ch8 * 8)]);
      const int m = m0 + ch8 * 8;                       // the 8 tokens of a chunk lie in one group of 16: one hypothesis
      if (m < p.M) vt_store_unit(img, blk.coff + wave * 128 + c, m, p.tokens, ch8 & 1, v);
    }
    TSTAMP(3);
    return;
  }

  if constexpr (EPI == EPI_LN || EPI == EPI_LNSUM) {
    // residual tile -> the (now free) tile region by LDS-DMA, then added in fp32 in the accumulator layout (a register quad is an
    // 8-byte half chunk of the tile).  The add and the statistics below stay written out - the independent second implementation
    // beside head_mlp.hip's: as functions shared with it they cost this kernel 2 VGPRs (EPI_LN) and change the SGPRs of EPI_LNSUM
    tok_tile_dma<TG_ROWS, 4>(p.res, m0, p.M, wave, lane, lds0);
    wait_vm<0>();
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = acc_row_token(j, lr);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const half4 rq = *reinterpret_cast<const half4 *>(tg_smem + tile_quad_off<TG_ROWS, 4>(wave, i, rg, row, lh));
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][j][rg * 4 + e] += (float)rq[e];
        }
    }
    // LayerNorm statistics per token over the 512 columns: lane -> 64 of the wave's 128 columns, partner lane (xor 32) the
    // other 64, then the 4 waves through LDS in a fixed order.  Two passes (mean, then centred second moment).
    float mean[2], rstd[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) s += acc[i][j][e];
      s += __shfl_xor(s, 32);
      if (lh == 0) red[wave * 64 + j * 32 + lr] = s;
    }
    __syncthreads();                                     // (also: every wave has consumed its residual chunks)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) s += red[w * 64 + j * 32 + lr];
      mean[j] = s * (1.f / 512.f);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          acc[i][j][e] -= mean[j];
          s += acc[i][j][e] * acc[i][j][e];
        }
      s += __shfl_xor(s, 32);
      if (lh == 0) red[256 + wave * 64 + j * 32 + lr] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) s += red[256 + w * 64 + j * 32 + lr];
      rstd[j] = rsqrtf(s * (1.f / 512.f) + 1e-5f);
    }
    if constexpr (EPI == EPI_LNSUM) {
      tok_gsum_store<4>(TokLane{lane, wave, lr, lh}, acc, rstd, m0, p.M, p.gsum);   // gamma / beta are applied after the token mean (mean_head_kernel)
      TSTAMP(3);
      return;
    }
    // gamma / beta, then the fp16 row epilogue below
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int c = wave * 128 + i * 32 + rg * 8 + lh * 4;
        const float4 gv = *reinterpret_cast<const float4 *>(p.gamma + c), bv = *reinterpret_cast<const float4 *>(p.beta + c);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j][rg * 4 + 0] = acc[i][j][rg * 4 + 0] * rstd[j] * gv.x + bv.x;
          acc[i][j][rg * 4 + 1] = acc[i][j][rg * 4 + 1] * rstd[j] * gv.y + bv.y;
          acc[i][j][rg * 4 + 2] = acc[i][j][rg * 4 + 2] * rstd[j] * gv.z + bv.z;
          acc[i][j][rg * 4 + 3] = acc[i][j][rg * 4 + 3] * rstd[j] * gv.w + bv.w;
        }
      }
  }

  if constexpr (EPI != EPI_VT && EPI != EPI_LNSUM) {
    // fp16 rows: the wave's 64 tokens x 128 columns through its private staging (no workgroup barrier), 16-byte stores of
    // whole 256-byte row segments.  (EPI_LN: the barrier after the first statistics pass ordered the last residual reads of
    // every wave before these writes.)
    f16 *stage = reinterpret_cast<f16 *>(tg_smem) + (size_t)wave * (TG_ROWS * TG_STAGE_LD);   // 17 KB per wave
    const bool relu = blk.relu != 0;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          half4 hv = acc_quad_f16(acc[i][j], rg);
          if (relu) hv = relu4(hv);
          *reinterpret_cast<half4 *>(&stage[tg_stage_off(acc_row_token(j, lr), acc_row_chan(i, rg, lh))]) = hv;
        }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    f16 *obase = (f16 *)blk.out + blk.coff + wave * 128;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int px = u * 4 + (lane >> 4), c16 = lane & 15;
      const uint4 v = *reinterpret_cast<const uint4 *>(&stage[tg_stage_off(px, c16 * 8)]);
      if (m0 + px < p.M) *reinterpret_cast<uint4 *>(obase + (size_t)(m0 + px) * blk.ld + c16 * 8) = v;
    }
    TSTAMP(3);
  }
}

template <int EPI>
static int tg_launch(const TokGemmArgs &a, hipStream_t s) {
  const int n_rt = (a.M + TG_ROWS - 1) / TG_ROWS;
  hipLaunchKernelGGL((tok_gemm_kernel<EPI>), dim3(n_rt * a.nblk), dim3(TG_THREADS), TG_LDS_BYTES, s, a);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

void tok_gemm_kernel_lds(std::vector<KernelLds> &v) {
  v.push_back({(const void *)tok_gemm_kernel<EPI_ROWS>, TG_LDS_BYTES});
  v.push_back({(const void *)tok_gemm_kernel<EPI_VT>, TG_LDS_BYTES});
  v.push_back({(const void *)tok_gemm_kernel<EPI_LN>, TG_LDS_BYTES});
  v.push_back({(const void *)tok_gemm_kernel<EPI_LNSUM>, TG_LDS_BYTES});
}

int tok_check_args(const char *who, const TokGemmArgs &a, int out, int coff_align) {
  FP_REQUIRE(a.in && a.M >= 0 && a.nblk >= 1 && a.nblk <= TG_MAXBLK, "%s: bad arguments", who);
  if (a.M == 0) return FP_OK;
  FP_REQUIRE((double)a.M * TOK_K * 2.0 < 4294967296.0, "%s: M=%d too large for 32-bit lane offsets", who, a.M);
  for (int b = 0; b < a.nblk; ++b) {
    const TokGemmBlock &k = a.blk[b];
    FP_REQUIRE(k.w && k.bias, "%s: block %d has null weights", who, b);
    const int o = out == TOK_OUT_BLK ? (k.vt ? TOK_OUT_VT : TOK_OUT_ROWS) : out;
    if (o == TOK_OUT_NONE) continue;
    FP_REQUIRE(k.out && k.coff % coff_align == 0, "%s: bad output of block %d", who, b);
    if (o == TOK_OUT_VT) FP_REQUIRE(a.tokens > 0 && a.tokens % 16 == 0 && a.tokens <= VT_LD, "%s: tokens=%d must be a multiple of 16, <= 416", who, a.tokens);
    else FP_REQUIRE(k.ld % 8 == 0, "%s: row stride of block %d is not a multiple of 8", who, b);
  }
  return FP_OK;
}

int launch_tok_gemm(fp_ctx *ctx, const TokGemmArgs &a, int epi, hipStream_t s) {
  FP_TRY(tok_check_args("tok_gemm", a, epi == EPI_VT ? TOK_OUT_VT : epi == EPI_LNSUM ? TOK_OUT_NONE : TOK_OUT_ROWS, epi == EPI_ROWS ? 128 : 1));
  if (a.M == 0) return FP_OK;
  ProfScope ps(ctx, s, "linear", 2.0 * (double)a.M * 512.0 * 512.0 * a.nblk);
  switch (epi) {
    case EPI_ROWS:
      return tg_launch<EPI_ROWS>(a, s);
    case EPI_VT:
      return tg_launch<EPI_VT>(a, s);
    case EPI_LN:
      FP_REQUIRE(a.nblk == 1 && a.res && a.gamma && a.beta, "tok_gemm: LN epilogue needs one block, residual, gamma, beta");
      return tg_launch<EPI_LN>(a, s);
    case EPI_LNSUM:
      FP_REQUIRE(a.nblk == 1 && a.res && a.gsum && a.M % 16 == 0, "tok_gemm: LN-sum epilogue needs one block, residual, gsum, M %% 16 == 0");
      return tg_launch<EPI_LNSUM>(a, s);
  }
  FP_REQUIRE(false, "tok_gemm: unknown epilogue %d", epi);
}
