// fp16 NHWC implicit-GEMM convolution / linear layer on MFMA (gfx950).
//
// Replaces the cuDNN convolutions + BN + ReLU + residual adds of learning/models/network_modules.py:37-111
// (BN folded into weights/bias at load) and, with KH=KW=1, every nn.Linear of the transformer heads.
//
//   out[m][co] = act( sum_{tap,ci} in[pix(m)+off(tap)][ci] * w[co][tap*Cin+ci] + bias[co] (+ res[m][co]) ) (+ post_add)
//
// GEMM view: M_gemm = Cout (weights are the MFMA A operand), N_gemm = pixels (activations are the B
// operand, gathered per row straight from the NHWC tensor - no im2col buffer), K = KH*KW*Cin.
// With this orientation a lane of the 32x32 accumulator owns ONE pixel and 4 consecutive output
// channels per register quad => 8-byte channel-contiguous NHWC stores, and the "V transposed"
// store used by the attention kernel ([b][head][d][token]) is lane-contiguous.
//
// Tile: 256 pixels x BM couts (BM = 128 | 64) per 256-thread workgroup, 2x2 waves, each wave (BM/2) x 128 via
// v_mfma_f32_32x32x16_f16; both operands staged by LDS-DMA through a 3-deep ring (below).  The 3x3 stride-1 layers
// have their own kernel (conv_halo.hip).
#include "common.h"
#include "conv_tile.h"
#include <cstdlib>
#include <type_traits>

#define CV_BK 32

// ------------------------------------------------------------------------------------------------
// 256 pixels x BM couts per workgroup, both operands staged by LDS-DMA (global_load_lds_dwordx4,
// per-lane gather address, out-of-image taps read a zero page), the swizzled 64-byte row tile of
// conv_tile.h (conflict-free ds_read_b128), 3-deep ring: two K-steps of DMA are in flight under the current
// step's 16 MFMAs per wave.  Used for the 1x1 (Linear) layers, the stride-2 3x3 and the 7x7 stem.
// ------------------------------------------------------------------------------------------------
// (C2_BK = 32, K per step: conv_plan.h; C2_BN = 256 pixels and every index rule: conv_tile.h)

#ifdef HALO_STAMP
// diagnostic build only (make -B EXTRA=-DHALO_STAMP): per-wave cycle counts of prologue / K loop / epilogue
__device__ unsigned long long g_igemm_stamps[4096 * 4 * 4];
extern "C" __attribute__((visibility("default"))) int fp_dbg_igemm_stamps(unsigned long long *host) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_igemm_stamps), sizeof(g_igemm_stamps)) == hipSuccess ? 0 : -1;
}
#define ISTAMP(x) x
#else
#define ISTAMP(x)
#endif

// LDS-DMA (glds16: scalar base + lane offset for the linear operands, one address per lane for the gather) and the counted waits: device_util.h

// One workgroup tile: 64 NT pixels x BM couts, 4 waves as 2 (cout halves) x 2 (pixel halves), each wave (BM/2) x 32 NT.
// NT = 4 -> the 256-pixel main tiles, NT = 1 -> 64-pixel tail tiles (conv_igemm2_kernel).  The accumulation order of an
// output element does not depend on NT.
template <int BM, int KW, bool CIN8, int NT, bool RES, bool SPLIT = false>
__device__ __forceinline__ void igemm2_tile(const ConvArgs &p, const f16 *__restrict__ zero_page, const int m0, const int c0, f16 *smem, const int ks = 0) {
  constexpr int TN = 64 * NT;                              // pixels per workgroup
  constexpr int XH = TN * C2_BK, WH = BM * C2_BK;          // halfs per stage
  ISTAMP(const unsigned long long t_entry = __builtin_amdgcn_s_memtime();)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  constexpr int WM = BM / 2, MT = WM / 32;
  constexpr int WQ = c2_wq(BM);                            // weight DMA instructions per wave per stage
  const int lr = lane & 31, lh = lane >> 5;
  const int HoWo = p.Ho * p.Wo;
  const int ntaps = p.KH * p.KW;

  // ---- DMA source bookkeeping: instruction q of this wave is slot q*4 + wave of the pixel image (gather form, conv_tile.h) ----
  const int chp = lane & 3;
  long long xbase[NT];
  int iy0[NT], ix0[NT], xch[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int px = ct_dma_row(ct_dma_slot(q, 4, wave), lane);
    const int m = m0 + px;
    const bool mv = m < p.M;
    const int mm = mv ? m : 0;
    const int n = mm / HoWo, rem = mm - n * HoWo;
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    iy0[q] = mv ? oy * p.stride - p.pad : -100000;          // invalid pixel -> every tap out of range
    ix0[q] = ox * p.stride - p.pad;
    xbase[q] = (long long)n * p.H * p.W * p.Cin;
    xch[q] = ct_dma_chunk(px, lane);                         // source chunk (swizzle on the SOURCE side)
  }
  // weights (the rule is ct_w_off; written out: profiles/conv_tile_isa.md): instruction q of wave w covers couts (q*4 + w)*16 + lane/4; the swizzle term ((co>>2)&3) = (lane>>4)&3 does not
  // depend on q, so ONE 32-bit lane offset serves every q and K-step, the rest of the address is scalar
  const unsigned woff = (unsigned)(((wave * 16 + (lane >> 2)) * p.Kpad + ((chp ^ ((lane >> 4) & 3)) * 8)) * 2);
  const f16 *wbase = p.w + (size_t)c0 * p.Kpad;
  // DMA instruction d of a stage: d = 0..NT-1 the activation gather (pixel group d), d = NT.. the weights
  // 1x1 (Linear) layers: a pixel's K-row is contiguous, the gather address of step kt is a fixed 32-bit lane offset from the
  // scalar base p.in + kt*64 B - no per-step tap / bounds / 64-bit address arithmetic in front of the DMA
  // (pixels past M are clamped to the last pixel: their products only reach output rows that are never stored)
  unsigned xlin[NT];
  const bool lin = KW == 1 && !CIN8 && p.stride == 1 && p.pad == 0 && (double)p.M * p.Cin * 2.0 < 4294967296.0;   // output pixel m reads input pixel m
  if (lin) {
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int m = min(m0 + ct_dma_row(ct_dma_slot(q, 4, wave), lane), p.M - 1);
      xlin[q] = (unsigned)(m * p.Cin + xch[q] * 8) * 2u;
    }
  }
  auto stage_one = [&](int kt, int buf, int d) __attribute__((always_inline)) {
    f16 *xs = smem + buf * (XH + WH), *ws = xs + XH;
    if (d < NT) {
      const int q = d;
      if (lin) {
        glds16(p.in + kt * C2_BK, xlin[q], xs + ct_dma_lds(ct_dma_slot(q, 4, wave)));
        return;
      }
      const int k = kt * C2_BK + xch[q] * 8;
      int tap, ci;
      if (CIN8) {
        tap = k >> 3;
        ci = 0;
      } else {
        tap = (kt * C2_BK) / p.Cin;
        ci = k - tap * p.Cin;
      }
      const int ky = tap / KW, kx = tap - ky * KW;
      const int iy = iy0[q] + ky, ix = ix0[q] + kx;
      const bool ok = tap < ntaps && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      const f16 *src = ok ? p.in + xbase[q] + ((long long)iy * p.W + ix) * p.Cin + ci : zero_page;
      glds16(src, xs + ct_dma_lds(ct_dma_slot(q, 4, wave)));
    } else {
      const int q = d - NT;
      glds16(wbase + (size_t)(q * 64) * p.Kpad + (size_t)kt * C2_BK, woff, ws + ct_dma_lds(ct_dma_slot(q, 4, wave)));
    }
  };
  auto stage = [&](int kt, int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int d = 0; d < NT + WQ; ++d) stage_one(kt, buf, d);
  };

  // ---- fragment bases (conv_tile.h; rows +32 keep the same swizzle) ----
  int wa[2], xa[NT][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    wa[ks] = ct_frag(wm * WM + lr, ks, lh);
#pragma unroll
    for (int j = 0; j < NT; ++j) xa[j][ks] = ct_frag(wn * (32 * NT) + acc_row_token(j, lr), ks, lh);
  }

  // accumulators start at the bias (fp32): a lane owns channels wm*WM + acc_row_chan(i, rg, lh) + (0..3) of its pixels (written out: profiles/conv_tile_isa.md)
  floatx16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      float4 bv = *reinterpret_cast<const float4 *>(p.bias + c0 + wm * WM + i * 32 + rg * 8 + lh * 4);
      if (SPLIT && ks != 0) bv = make_float4(0.f, 0.f, 0.f, 0.f);          // (split-K: the bias rides in share 0)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        acc[i][j][rg * 4 + 0] = bv.x;
        acc[i][j][rg * 4 + 1] = bv.y;
        acc[i][j][rg * 4 + 2] = bv.z;
        acc[i][j][rg * 4 + 3] = bv.w;
      }
    }

  // split-K (SPLIT): share ks of p.ksplit walks K-steps [kb, kb + nk) and leaves fp32 sums for splitk_finish_kernel (conv_halo.hip)
  const int nk = SPLIT ? p.Kpad / C2_BK / p.ksplit : p.Kpad / C2_BK, kb = SPLIT ? ks * nk : 0;
  // 3-deep LDS-DMA ring: K-steps kt+1 and kt+2 stay in flight across the barrier (counted vmcnt + raw s_barrier;
  // a __syncthreads() would drain them).  Every wave issues exactly DMAW instructions per stage.
  constexpr int DMAW = c2_dmaw(NT, BM);
  ISTAMP(const unsigned long long t_loop = __builtin_amdgcn_s_memtime();)
  stage(kb, 0);
  if (nk > 1) stage(kb + 1, 1);
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = c2_slot(kt);
    if (c2_wait_allowed(kt, nk, DMAW) != 0) wait_vm_lgkm<DMAW>();
    else wait_vm_lgkm<0>();
    __builtin_amdgcn_s_barrier();          // stage kt landed for every wave; slot (kt+2)%3 was last read in step kt-1: free
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 2 < nk) stage(kb + kt + 2, c2_slot(kt + 2));
    const f16 *xs = smem + cur * (XH + WH), *ws = xs + XH;
    // two k-steps per stage, software-pipelined like the halo kernel: pixel-tile-major MFMA order, the pixel fragment of
    // step 1 is requested as soon as step 0's MFMAs on that register have been issued (counted lgkmcnt waits).  (Issuing
    // the DMAs of stage kt+2 from between the MFMAs, as the halo kernel does, was measured 2-4 % slower here: these layers
    // are bound by the L2 -> LDS fill, and the fill wants its requests as early as possible.)
    half8 af[2][MT], bf[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) af[0][i] = *reinterpret_cast<const half8 *>(&ws[wa[0] + i * CT_TILE32]);
#pragma unroll
    for (int j = 0; j < NT; ++j) bf[j] = *reinterpret_cast<const half8 *>(&xs[xa[j][0]]);
#pragma unroll
    for (int i = 0; i < MT; ++i) af[1][i] = *reinterpret_cast<const half8 *>(&ws[wa[1] + i * CT_TILE32]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[ks][i], bf[j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (ks == 0) bf[j] = *reinterpret_cast<const half8 *>(&xs[xa[j][1]]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // ---- epilogue, fp16 NHWC: residual staged through LDS and added in fp32, LDS transpose, 16-byte row stores.  The K loop
  // of a Linear layer is only 16 steps long, so the epilogue weighs a quarter of the tile; it is written to issue few vector
  // instructions: ReLU on the packed fp16 pair after conversion (rounding is monotonic and keeps 0: same result as before
  // it), no per-row output select when the whole tile lies on one side of split_m.  (Reading the residual as 8-byte
  // gathers in the accumulator layout behind the first DMA stages was measured: epilogue -6.8k cycles, K loop +16k.) ----
  ISTAMP(const unsigned long long t_epi = __builtin_amdgcn_s_memtime();)
  if constexpr (SPLIT) {      // fp32 sums of this share for splitk_finish_kernel
    ct_splitk_store(p, acc, ks, m0 + wn * (32 * NT), c0, wm * WM, lr, lh);
    return;
  }
  if (p.out_mode == 0) {
    f16 *stage = smem;
    constexpr int CPR = BM / 8;           // 16-byte chunks per staged row
    constexpr int NCH = TN * CPR / 256;
    constexpr int RB = NCH < 8 ? NCH : 8;
    u32x4 rv[NCH];
    if constexpr (RES) {                  // residual tile: ONE batch of coalesced 16-byte loads before the barrier, staged through LDS (row pieces: ct_piece_px / ct_piece_c16)
#pragma unroll
      for (int u = 0; u < NCH; ++u) {
        const int idx = tid + 256 * u, px = idx / CPR, c16 = idx % CPR;
        const int m = min(m0 + px, p.M - 1);    // unconditional (clamped) load: a guarded one makes hipcc wait per element
        rv[u] = *reinterpret_cast<const u32x4 *>(p.res + (size_t)m * p.Cout + c0 + c16 * 8);
      }
    }
    __syncthreads();
    if constexpr (RES) {
#pragma unroll
      for (int u = 0; u < NCH; ++u) {
        const int idx = tid + 256 * u, px = idx / CPR, c16 = idx % CPR;
        *reinterpret_cast<u32x4 *>(&stage[ct_stage_off(BM, px, c16 * 8)]) = rv[u];
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < NT; ++j) {      // each lane reads back exactly the 8-byte slots it overwrites below: no barrier in between
        const int pxl = wn * (32 * NT) + acc_row_token(j, lr);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const half4 rq = *reinterpret_cast<const half4 *>(&stage[ct_stage_off(BM, pxl, wm * WM + acc_row_chan(i, rg, lh))]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][rg * 4 + e] += (float)rq[e];
          }
      }
    }
    if (p.post_add) {                     // fp32 add after the ReLU (positional embedding): one layer per forward
      const float lo = p.relu ? 0.f : -__builtin_inff();
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int pxl = wn * (32 * NT) + acc_row_token(j, lr);
        const int prow = min(m0 + pxl, p.M - 1) % p.post_period;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const int col = wm * WM + acc_row_chan(i, rg, lh);
            const float4 pv = *reinterpret_cast<const float4 *>(p.post_add + (size_t)prow * p.Cout + c0 + col);
            half4 hv;
            hv[0] = (f16)(fmaxf(acc[i][j][rg * 4 + 0], lo) + pv.x);
            hv[1] = (f16)(fmaxf(acc[i][j][rg * 4 + 1], lo) + pv.y);
            hv[2] = (f16)(fmaxf(acc[i][j][rg * 4 + 2], lo) + pv.z);
            hv[3] = (f16)(fmaxf(acc[i][j][rg * 4 + 3], lo) + pv.w);
            *reinterpret_cast<half4 *>(&stage[ct_stage_off(BM, pxl, col)]) = hv;
          }
      }
    } else {
      auto convert = [&](auto relu_c) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int pxl = wn * (32 * NT) + acc_row_token(j, lr);
#pragma unroll
          for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
              half4 hv;
#pragma unroll
              for (int e = 0; e < 4; ++e) hv[e] = (f16)acc[i][j][rg * 4 + e];
              if constexpr (decltype(relu_c)::value) hv = __builtin_elementwise_max(hv, half4{(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f});
              *reinterpret_cast<half4 *>(&stage[ct_stage_off(BM, pxl, wm * WM + acc_row_chan(i, rg, lh))]) = hv;
            }
        }
      };
      if (p.relu) convert(std::true_type{});
      else convert(std::false_type{});
    }
    __syncthreads();
    const bool side_hi = m0 >= p.split_m;
    if (side_hi || m0 + TN <= p.split_m) {          // whole tile on one side: one scalar base, rows at a fixed stride
      f16 *obase = ct_out_ptr(p, m0) + c0;
#pragma unroll
      for (int i0 = 0; i0 < NCH; i0 += RB) {
        uint4 ov[RB];
#pragma unroll
        for (int u = 0; u < RB; ++u) {
          const int idx = tid + 256 * (i0 + u), px = idx / CPR, c16 = idx % CPR;
          ov[u] = *reinterpret_cast<const uint4 *>(&stage[ct_stage_off(BM, px, c16 * 8)]);
        }
#pragma unroll
        for (int u = 0; u < RB; ++u) {
          const int idx = tid + 256 * (i0 + u), px = idx / CPR, c16 = idx % CPR;
          if (m0 + px < p.M) *reinterpret_cast<uint4 *>(obase + (long long)px * p.out_ld + c16 * 8) = ov[u];
        }
      }
    } else {
#pragma unroll
      for (int i0 = 0; i0 < NCH; i0 += RB) {
        uint4 ov[RB];
#pragma unroll
        for (int u = 0; u < RB; ++u) {
          const int idx = tid + 256 * (i0 + u), px = idx / CPR, c16 = idx % CPR;
          ov[u] = *reinterpret_cast<const uint4 *>(&stage[ct_stage_off(BM, px, c16 * 8)]);
        }
#pragma unroll
        for (int u = 0; u < RB; ++u) {
          const int idx = tid + 256 * (i0 + u), px = idx / CPR, c16 = idx % CPR;
          const int m = m0 + px;
          if (m < p.M) {
            const long long orow = ct_out_row(m, p.split_m);
            const int coff = ct_out_col(m, p.split_m, p.coff_hi);
            *reinterpret_cast<uint4 *>((f16 *)p.out + orow * p.out_ld + coff + c0 + c16 * 8) = ov[u];
          }
        }
      }
    }
    ISTAMP(if (lane == 0 && blockIdx.x < 4096) {
      unsigned long long *o = g_igemm_stamps + ((size_t)blockIdx.x * 4 + wave) * 4;
      const unsigned long long t_exit = __builtin_amdgcn_s_memtime();
      if (wave == 1) {          // wave 1: absolute entry / exit times and the hardware slot (HW_ID | XCC_ID << 32): per-CU timelines
        o[0] = t_entry; o[1] = t_exit;
        o[2] = (unsigned long long)__builtin_amdgcn_s_getreg(63492) | ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32);
      } else {
        o[0] = t_loop - t_entry; o[1] = t_epi - t_loop; o[2] = t_exit - t_epi;
      }
      o[3] = 1;
    })
    return;
  }

  // ---- epilogue, other output modes (fp32 NHWC, transposed V): direct stores ----
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int m = m0 + wn * (32 * NT) + j * 32 + lr;
    if (m >= p.M) continue;
    const long long orow = ct_out_row(m, p.split_m);
    const int coff = ct_out_col(m, p.split_m, p.coff_hi);
    int prow = 0;
    if (p.post_add) prow = m % p.post_period;
    int tb = 0, tt = 0;
    if (p.out_mode == 2) {
      tb = m / p.tokens;
      tt = vt_col(m - tb * p.tokens);
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int co = c0 + wm * WM + i * 32 + rg * 8 + lh * 4;
        float v[4];
        v[0] = acc[i][j][rg * 4 + 0];      // the bias is already in the accumulator
        v[1] = acc[i][j][rg * 4 + 1];
        v[2] = acc[i][j][rg * 4 + 2];
        v[3] = acc[i][j][rg * 4 + 3];
        if (p.res) {
          half4 rv = *reinterpret_cast<const half4 *>(p.res + (size_t)m * p.Cout + co);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += (float)rv[e];
        }
        if (p.relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        if (p.post_add) {
          const float4 pv = *reinterpret_cast<const float4 *>(p.post_add + (size_t)prow * p.Cout + co);
          v[0] += pv.x;
          v[1] += pv.y;
          v[2] += pv.z;
          v[3] += pv.w;
        }
        if (p.out_mode == 0) {
          half4 hv;
#pragma unroll
          for (int e = 0; e < 4; ++e) hv[e] = (f16)v[e];
          *reinterpret_cast<half4 *>((f16 *)p.out + orow * p.out_ld + coff + co) = hv;
        } else if (p.out_mode == 1) {
          *reinterpret_cast<float4 *>((float *)p.out + orow * p.out_ld + coff + co) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            ((f16 *)p.out)[vt_row(tb, co + e) + tt] = (f16)v[e];
          }
        }
      }
    }
  }
}

// Grid = n_main workgroups of 256 px x BM co, then n_tail4 workgroups of 64 px covering the LAST main-size tiles cut in four
// (see conv3x3_halo kernels: at N=252 these layers have 1576 or 3150 tiles for 512 slots - a last round that is 8-15 % full).
template <int BM, int KW, bool CIN8, bool RES>
__global__ __launch_bounds__(256, 2) void conv_igemm2_kernel(ConvArgs p, const f16 *__restrict__ zero_page, int n_main) {
  extern __shared__ __attribute__((aligned(16))) f16 smem[];
  const int n_ct = p.Cout / BM;
  if ((int)blockIdx.x < n_main) {
    const CtTile T = ct_grid_main(xcd_remap(blockIdx.x, n_main), n_ct, C2_BN, BM);
    igemm2_tile<BM, KW, CIN8, 4, RES>(p, zero_page, T.m0, T.c0, smem);
  } else {
    const CtTile T = c2_grid_tail(xcd_remap(blockIdx.x - n_main, gridDim.x - n_main), n_main, n_ct, BM);
    if (T.m0 >= p.M) return;
    igemm2_tile<BM, KW, CIN8, 1, RES>(p, zero_page, T.m0, T.c0, smem);
  }
}

// Split-K form of the 3x3 stride-2 layer with the long K (256 -> 512 channels: 72 K-steps) at 3 .. 4 hypotheses (1 .. 2: conv_small.hip; FP_SMALL=0: 1 .. 4), where the layer is
// 28 .. 100 workgroups that each walk all of K behind one DMA round trip per step (38 us at one hypothesis): 64-pixel tiles,
// p.ksplit workgroups per tile with an equal share of the K-steps each, fp32 sums to p.splitk, splitk_finish_kernel adds them in
// share order (the scheme of conv3x3_halo_splitk_kernel: these batch sizes are the size class with its own last bits).
template <int BM, int KW>
__global__ __launch_bounds__(256, 2) void conv_igemm2_splitk_kernel(ConvArgs p, const f16 *__restrict__ zero_page) {
  extern __shared__ __attribute__((aligned(16))) f16 smem[];
  const int n_ct = p.Cout / BM;
  const CtTile T = ct_grid_split(blockIdx.x, p.ksplit, n_ct, 64, BM);
  if (T.m0 >= p.M) return;
  igemm2_tile<BM, KW, false, 1, false, true>(p, zero_page, T.m0, T.c0, smem, T.ks);
}

template <int BM>
constexpr int igemm2_lds_bytes() { return c2_lds_bytes(BM); }

template <int BM, int KW, bool CIN8>
static void igemm2_lds_both(std::vector<KernelLds> &v) {
  v.push_back({(const void *)conv_igemm2_kernel<BM, KW, CIN8, true>, igemm2_lds_bytes<BM>()});
  v.push_back({(const void *)conv_igemm2_kernel<BM, KW, CIN8, false>, igemm2_lds_bytes<BM>()});
}

void conv_kernel_lds(std::vector<KernelLds> &v) {       // every instantiation launch_conv can reach
  v.push_back({(const void *)conv_igemm2_splitk_kernel<128, 3>, igemm2_lds_bytes<128>()});
  igemm2_lds_both<128, 7, true>(v), igemm2_lds_both<64, 7, true>(v);
  igemm2_lds_both<128, 3, false>(v), igemm2_lds_both<64, 3, false>(v);
  igemm2_lds_both<128, 1, false>(v), igemm2_lds_both<64, 1, false>(v);
}

template <int BM, int KW, bool CIN8, bool RES>
static int launch_two_r(fp_ctx *ctx, const ConvArgs &a, const f16 *zero_page, hipStream_t s) {
  const int n_tiles = ((a.M + C2_BN - 1) / C2_BN) * (a.Cout / BM);
  int n_main, n_tail4;
  halo_split(n_tiles, 2 * ctx->num_cu, conv_knobs(), &n_main, &n_tail4);
  constexpr int lds = igemm2_lds_bytes<BM>();
  FP_REQUIRE(a.out_mode != 0 || (a.out_ld % 8 == 0 && a.coff_hi % 8 == 0), "conv: out_ld/coff must be multiples of 8 for fp16 output");
  hipLaunchKernelGGL((conv_igemm2_kernel<BM, KW, CIN8, RES>), dim3(n_main + n_tail4), dim3(256), lds, s, a, zero_page, n_main);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

template <int BM, int KW, bool CIN8>
static int launch_two(fp_ctx *ctx, const ConvArgs &a, const f16 *zero_page, hipStream_t s) {
  // the residual is added in the fp16-NHWC epilogue only; the other output modes read it directly
  return (a.res && a.out_mode == 0) ? launch_two_r<BM, KW, CIN8, true>(ctx, a, zero_page, s) : launch_two_r<BM, KW, CIN8, false>(ctx, a, zero_page, s);
}

// The knobs of conv_plan.h, read once per process: the only place that names their variables
const ConvKnobs &conv_knobs() {
  static const ConvKnobs knobs = [] {
    ConvKnobs k;
    k.small = (int)fp_env_int("FP_SMALL", k.small);
    k.small_max_wg = (int)fp_env_int("FP_SMALL_MAX_WG", k.small_max_wg);
    k.c128_band = (int)fp_env_int("FP_C128_BAND", k.c128_band);
    k.ksplit_max = (int)fp_env_int("FP_KSPLIT_MAX", k.ksplit_max);
    k.ksplit_min_chunks = (int)fp_env_int("FP_KSPLIT_MIN_CHUNKS", k.ksplit_min_chunks);
    k.halo_tail = fp_env_int("FP_HALO_TAIL", k.halo_tail) != 0;
    k.halo_nt = (int)fp_env_int("FP_HALO_NT", k.halo_nt);
    return k;
  }();
  return knobs;
}

size_t conv_packed_halfs(unsigned packing, int Cout, int Cin) { return packing == CONV_OFFER_SMALL ? small_packed_halfs(Cout, Cin) : s2_packed_halfs(Cout, Cin); }

int conv_pack_weights(unsigned packing, const f16 *d_w, int Cout, int Cin, int Kpad, f16 *d_out, hipStream_t s) {
  if (packing == CONV_OFFER_SMALL) return small_pack_weights(d_w, Cout, Cin, Kpad, d_out, s);
  if (packing == CONV_OFFER_S2) return s2_pack_weights(d_w, Cout, Cin, Kpad, d_out, s);
  FP_REQUIRE(packing == CONV_OFFER_S1B, "conv_pack_weights: packing %u is not one copy", packing);
  return s2_pack_weights(d_w, Cout, Cin, Kpad, d_out, s, 2, 1);      // (conv_s1b.hip: 64 couts per wave group)
}

int launch_conv(fp_ctx *ctx, const ConvArgs &args, hipStream_t s) {
  ConvArgs a = args;
  FP_REQUIRE(a.Cin == 8 || a.Cin % 32 == 0, "conv: Cin=%d must be 8 or a multiple of 32", a.Cin);
  FP_REQUIRE(a.Cout % 64 == 0, "conv: Cout=%d must be a multiple of 64", a.Cout);
  FP_REQUIRE(a.Kpad % CV_BK == 0 && a.Kpad >= a.KH * a.KW * a.Cin, "conv: bad Kpad=%d", a.Kpad);
  FP_REQUIRE(a.KH == a.KW && (a.KW == 1 || a.KW == 3 || a.KW == 7), "conv: kernel %dx%d unsupported (1,3,7)", a.KH, a.KW);
  FP_REQUIRE(a.M == a.Nimg * a.Ho * a.Wo, "conv: M mismatch");
  FP_REQUIRE(a.out_ld % 4 == 0 && a.coff_hi % 4 == 0, "conv: out_ld/coff must be multiples of 4");
  if (a.M == 0) return FP_OK;
  // what the caller holds: the packed copies by their pointers (one wpk: conv_s2.hip's order for a stride-2 layer, conv_s1b.hip's for stride 1), scratch
  const unsigned offer = (a.wsm ? CONV_OFFER_SMALL : 0) | (a.wpk ? (a.stride == 1 ? CONV_OFFER_S1B : CONV_OFFER_S2) : 0) | (a.splitk ? CONV_OFFER_SPLITK : 0);
  const ConvPlan plan = conv_plan(a, ctx->num_cu, offer, conv_knobs());
  a.ksplit = plan.ksplit;                              // the kernels of the one-launch forms see no scratch
  if (plan.ksplit <= 1) a.splitk = nullptr;
  ProfScope ps(ctx, s, plan.cls, plan.flops);
  const f16 *zp = (const f16 *)ctx->zero_page;
  const bool bm128 = (a.Cout % 128 == 0);
  switch (plan.form) {
    case CONV_SMALL: return launch_conv_small(ctx, a, s);
    case CONV_S1B: return launch_conv_s1b(ctx, a, s);
    case CONV_HALO:
    case CONV_HALO_SPLITK: return launch_conv_halo(a, plan, s);
    case CONV_S2_SPLITK: {
      FP_REQUIRE(a.KW == 3 && a.stride == 2 && a.Cout % 128 == 0 && (a.Kpad / C2_BK) % a.ksplit == 0 && a.out_mode == 0, "conv split-K: unsupported layer");
      const int n_t = ((a.M + 63) / 64) * (a.Cout / 128);
      hipLaunchKernelGGL((conv_igemm2_splitk_kernel<128, 3>), dim3(n_t * a.ksplit), dim3(256), igemm2_lds_bytes<128>(), s, a, zp);
      FP_CHECK_HIP(hipGetLastError());
      return launch_splitk_finish(a, s);
    }
    case CONV_STEM: return launch_stem(ctx, a, s);
    case CONV_S2: return launch_conv_s2(ctx, a, s);
    case CONV_IGEMM2:
      if (a.Cin == 8) {
        FP_REQUIRE(a.KW == 7, "conv: Cin=8 path is the 7x7 stem");
        return bm128 ? launch_two<128, 7, true>(ctx, a, zp, s) : launch_two<64, 7, true>(ctx, a, zp, s);
      }
      if (a.KW == 3) return bm128 ? launch_two<128, 3, false>(ctx, a, zp, s) : launch_two<64, 3, false>(ctx, a, zp, s);
      if (a.KW == 1) return bm128 ? launch_two<128, 1, false>(ctx, a, zp, s) : launch_two<64, 1, false>(ctx, a, zp, s);
  }
  FP_REQUIRE(false, "conv: unsupported configuration KW=%d Cin=%d", a.KW, a.Cin);
}

