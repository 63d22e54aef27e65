// 3x3 / stride-1 / pad-1 convolution for gfx950 with the input HALO BAND resident in LDS.
//
// 93 % of the network FLOPs are 3x3 stride-1 convolutions on 40x40 (C=128|256) and 20x20 (C=512) maps
// (learning/models/network_modules.py:73-111 via refine_network.py:37-50).  An im2col-style implicit GEMM re-fetches every
// activation 9 times (once per tap) from L2 into LDS.  Here a workgroup owns a run of consecutive output pixels (flattened
// over images) x 128 output channels and, per 32-channel input chunk,
//   * brings the input rows it needs ONCE into LDS (the "halo band") and feeds all 9 taps from it: a tap shift is just a
//     different LDS address per lane (+-1 pixel, +-1 row; taps outside the image select a zero chunk),
//   * streams the 3 taps of one kernel row of weights at a time (128 co x 32 ci x 3 = 24 KB, double buffered) by LDS-DMA.
// conv3x3_halo_dma_kernel: 8 waves, 512 px, band by LDS-DMA (double buffered), v_mfma_f32_32x32x16_f16.
// Epilogue: accumulators start at the bias; residual (staged through LDS) + ReLU (+ positional embedding) in fp32, one
// rounding to fp16, LDS transpose, 16-byte row-contiguous NHWC stores.
#include "common.h"
#include "conv_tile.h"
#include <cstdlib>

// (HL_BM = 128 couts per tile, HL_CK = 32 input channels per chunk: conv_plan.h; HL_SLD, HaloCfgD and every index rule: conv_tile.h)

#ifdef HALO_STAMP
// diagnostic build only (make -B EXTRA=-DHALO_STAMP): per-wave cycle sums of [wait + barrier] and [group body], see scripts/halo_stamps.py
__device__ unsigned long long g_halo_stamps[4096 * 8 * 8];
extern "C" __attribute__((visibility("default"))) int fp_dbg_halo_stamps(unsigned long long *host, int clear) {
  if (host) (void)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_halo_stamps), sizeof(g_halo_stamps));
  if (clear) {
    static unsigned long long z[4096 * 8 * 8];
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_halo_stamps), z, sizeof(z));
  }
  return 0;
}
#define STAMP(x) x
#else
#define STAMP(x)
#endif

template <int V>
struct IC {
  static constexpr int value = V;
};

// LDS-DMA (glds16) and the counted waits in front of the barriers below: device_util.h

// ------------------------------------------------------------------------------------------------------------------------
// 8-wave tile (512 px x 128 co, one workgroup per CU) with the halo band staged by LDS-DMA as well, double
// buffered:
//   * halo pixels are 64-byte rows of the swizzled row tile of conv_tile.h, fetched by the linear DMA map (instruction h of wave w is
//     slot h*8 + w).  The band's fragment reads are conflict free at every tile alignment and tap shift, in the ds_read_b128 lane
//     groups ({0-3,12-15,20-27}, ...) as in contiguous quarters; border lanes, which take the zero chunk, can make a read two-way (conv_tile.h);
//   * no staging registers, no ds_write of the band, no barrier pair at the top of a chunk: the band of chunk cc+1 streams
//     into the other buffer while chunk cc is multiplied, one DMA instruction per pixel-tile visit;
//   * v_mfma_f32_32x32x16_f16, a wave holds 64 co x 128 px (2 x 4 accumulator tiles); a kernel row is 24 "tile visits" of 2
//     MFMAs, pixel fragments rotate through 4 registers, weight fragments of the next step go to a spare set.
// (A 16x16x32 MFMA form of this tile was measured too: ~7 % more cycles at a ~8 % higher clock, the same time.)
// ------------------------------------------------------------------------------------------------------------------------
// Epilogue of a tile: residual (staged through LDS) + ReLU (+ positional embedding) in fp32, one rounding to fp16,
// LDS transpose, 16-byte row-contiguous NHWC stores.
template <int NT, bool RES, bool POST>
__device__ __forceinline__ void halo_epilogue(const ConvArgs &p, const int m0, const int c0, f16 *lds, floatx16 (&acc)[2][NT]) {
  constexpr int NPW = 4, TM = 32 * NT * NPW, NTH = 128 * NPW, PXW = 32 * NT;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / NPW, wn = wave % NPW;
  const int lr = lane & 31, lh = lane >> 5;
  f16 *stage = lds;   // [TM px][HL_SLD]
  constexpr int NRES = TM * 16 / NTH;
  u32x4 rv[NRES];
  if constexpr (RES) {
#pragma unroll
    for (int u = 0; u < NRES; ++u) {      // row pieces ct_piece_px / ct_piece_c16 (written out: profiles/conv_tile_isa.md)
      const int idx = tid + NTH * u, px = idx >> 4, c16 = idx & 15;
      const int m = min(m0 + px, p.M - 1);
      rv[u] = *reinterpret_cast<const u32x4 *>(p.res + (size_t)m * p.Cout + c0 + c16 * 8);
    }
  }
  const float lo = p.relu ? 0.f : -__builtin_inff();
  __syncthreads();          // every wave is done with the band / weight images: the staging tile may overwrite them
  if constexpr (RES) {
#pragma unroll
    for (int u = 0; u < NRES; ++u) {
      const int idx = tid + NTH * u, px = idx >> 4, c16 = idx & 15;
      *reinterpret_cast<u32x4 *>(&stage[px * HL_SLD + c16 * 8]) = rv[u];
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int pxl = wn * PXW + acc_row_token(j, lr);
    float4 pvs[2][4];
    if constexpr (POST) {
      const int prow = min(m0 + pxl, p.M - 1) % p.post_period;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg)
          pvs[i][rg] = *reinterpret_cast<const float4 *>(p.post_add + (size_t)prow * p.Cout + c0 + wm * 64 + i * 32 + rg * 8 + lh * 4);      // acc_row_chan (written out: profiles/conv_tile_isa.md)
    }
    half4 rq[2][4];
    if constexpr (RES) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) rq[i][rg] = *reinterpret_cast<const half4 *>(&stage[ct_stage_off(HL_BM, pxl, wm * 64 + acc_row_chan(i, rg, lh))]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        float v[4] = {acc[i][j][rg * 4 + 0], acc[i][j][rg * 4 + 1], acc[i][j][rg * 4 + 2], acc[i][j][rg * 4 + 3]};
        if constexpr (RES) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += (float)rq[i][rg][e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], lo);
        if constexpr (POST) {
          const float4 pv = pvs[i][rg];
          v[0] += pv.x;
          v[1] += pv.y;
          v[2] += pv.z;
          v[3] += pv.w;
        }
        half4 hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) hv[e] = (f16)v[e];
        *reinterpret_cast<half4 *>(&stage[ct_stage_off(HL_BM, pxl, wm * 64 + acc_row_chan(i, rg, lh))]) = hv;
      }
    }
  }
  __syncthreads();
  constexpr int NOUT = TM * 16 / NTH, OB = NOUT < 8 ? NOUT : 8;
#pragma unroll
  for (int i0 = 0; i0 < NOUT; i0 += OB) {
    u32x4 ov[OB];
#pragma unroll
    for (int u = 0; u < OB; ++u) {
      if (i0 + u >= NOUT) break;                 // (NOUT = 12 for the 384-pixel tile: the second batch is half full)
      const int idx = tid + NTH * (i0 + u), px = idx >> 4, c16 = idx & 15;
      ov[u] = *reinterpret_cast<const u32x4 *>(&stage[px * HL_SLD + c16 * 8]);
    }
#pragma unroll
    for (int u = 0; u < OB; ++u) {
      if (i0 + u >= NOUT) break;
      const int idx = tid + NTH * (i0 + u), px = idx >> 4, c16 = idx & 15;
      const int m = m0 + px;
      if (m < p.M) {
        const long long orow = ct_out_row(m, p.split_m);
        const int coff = ct_out_col(m, p.split_m, p.coff_hi);
        *reinterpret_cast<u32x4 *>((f16 *)p.out + orow * p.out_ld + coff + c0 + c16 * 8) = ov[u];
      }
    }
  }
}

template <int W, int NT, bool RES, bool POST, bool SPLIT = false>
__device__ __forceinline__ void halo_tile_dma(const ConvArgs &p, const int m0, const int c0, f16 *lds, const int ks = 0) {
  constexpr int NPW = 4, TM = 32 * NT * NPW;
  using C = HaloCfgD<W, TM>;
  constexpr int H = W;
  // (512 threads)
  constexpr int PXW = 32 * NT;          // pixels per wave
  constexpr int HQ = C::HQ;
  constexpr int WQ = HL_WSLOTS / (2 * NPW);    // weight DMA instructions per wave per group
  STAMP(const unsigned long long t_entry = __builtin_amdgcn_s_memtime(); const unsigned long long r_entry = __builtin_amdgcn_s_memrealtime();)
  f16 *wbuf = lds + C::WBUF_OFF;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / NPW, wn = wave % NPW;
  const int lr = lane & 31, lh = lane >> 5;
  // static priority for the second-dispatched half of the workgroup (waves 4-7 are the arbitration loser of each SIMD pair at
  // equal priority): measured A/B in one session, 39.55 / 39.33 -> 38.99 / 38.92 ms per step, 1139 / 1145 -> 1153 / 1157 TF/s
  if (wave >= 4) __builtin_amdgcn_s_setprio(1);
  const int GR0 = hl_gr0(m0, W);
  const int total_rows = p.Nimg * H;
  // input-channel chunks [cbeg, nchunk) of this workgroup: all of them, or (SPLIT) share ks of p.ksplit equal shares
  const int call = p.Cin / HL_CK;
  const int cbeg = SPLIT ? ks * (call / p.ksplit) : 0;
  const int nchunk = SPLIT ? cbeg + call / p.ksplit : call;

  // ---- B fragments: band index of the top-left tap of this lane's pixel in tile 0 (tile j, taps: see load_b) ----
  const int pb = hl_pb(m0 + wn * PXW + lr, GR0, W);
  unsigned vmp[(NT + 2) / 3];          // 9 validity bits (ky*3+kx) per 32-pixel tile, three tiles per register
#pragma unroll
  for (int t = 0; t < (NT + 2) / 3; ++t) vmp[t] = 0;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int m = min(m0 + wn * PXW + j * 32 + lr, p.M - 1);
    const int gr = m / W, ox = m - gr * W, oy = gr % H;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        if (hl_tap_valid(oy, ox, W, ky, kx)) vmp[j / 3] |= 1u << hl_vbit(j, ky, kx);
      }
  }
  // ---- A fragments: row co = wm*64 + i*32 + lr, channel group ks*2 + lh
  const int wa[2] = {ct_frag(wm * 64 + lr, 0, lh), ct_frag(wm * 64 + lr, 1, lh)};

  // ---- halo band by LDS-DMA: instruction h of wave w lands band pixels (h*8 + w)*16 .. +15, lane i = (pixel i/4, position i%4): slot
  // ct_dma_slot(h, 8, w), row ct_dma_row, chunk ct_dma_chunk, source hl_band_src (written out: profiles/conv_tile_isa.md)
  const int hpix_max = total_rows * W - 1;
  auto halo_dma = [&](int cc, int hb, auto hc) __attribute__((always_inline)) {
    constexpr int h = decltype(hc)::value;
    int l4 = lane >> 2;
    asm volatile("" : "+v"(l4));                    // recompute per use: six hoisted offsets would cost six registers
    const int P = (h * 8 + wave) * 16 + l4;
    const int c = (lane & 3) ^ ((P >> 2) & 3);
    const int gp = min(max(GR0 * W + P - 1, 0), hpix_max);      // clamped: what lands from a clamped source is never read (conv_tile.h)
    const unsigned off = (unsigned)(gp * p.Cin + cc * HL_CK + c * 8) * 2u;
    glds16(p.in, off, lds + hb * C::HBUF_HALFS + (h * 8 + wave) * 512);
  };
  // ---- weights: row (g%8)*16 + lane/4 -> (row>>2)&3 = (lane>>4)&3: ct_w_off, hl_w_src, slot g0 + wave (written out: profiles/conv_tile_isa.md)
  const unsigned woff = (unsigned)(((wave * 16 + (lane >> 2)) * p.Kpad + (((lane & 3) ^ ((lane >> 4) & 3)) * 8)) * 2);
  auto wstage = [&](int cc, int ky, int buf, auto q0c, auto q1c) __attribute__((always_inline)) {
    constexpr int Q0 = decltype(q0c)::value, Q1 = decltype(q1c)::value;
#pragma unroll
    for (int q = Q0; q < Q1; ++q) {
      const int g0 = q * 2 * NPW;
      const f16 *sb = p.w + (size_t)(c0 + (g0 & 7) * 16) * p.Kpad + (ky * 3 + (g0 >> 3)) * p.Cin + cc * HL_CK;
      glds16(sb, woff, wbuf + buf * C::WBUF_HALFS + (q * 2 * NPW + wave) * 512);
    }
  };

  // accumulators start at the bias (fp32): a lane owns channels wm*64 + acc_row_chan(i, rg, lh) + (0..3) of its pixels (written out: profiles/conv_tile_isa.md)
  floatx16 acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      float4 bv = *reinterpret_cast<const float4 *>(p.bias + c0 + wm * 64 + i * 32 + rg * 8 + lh * 4);
      if (SPLIT && ks != 0) bv = make_float4(0.f, 0.f, 0.f, 0.f);       // the bias rides in split 0
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        acc[i][j][rg * 4 + 0] = bv.x;
        acc[i][j][rg * 4 + 1] = bv.y;
        acc[i][j][rg * 4 + 2] = bv.z;
        acc[i][j][rg * 4 + 3] = bv.w;
      }
    }

  if (tid < 1) *reinterpret_cast<u32x4 *>(&lds[C::ZERO_OFF]) = u32x4{0, 0, 0, 0};
  {
    auto all = [&](auto hc) __attribute__((always_inline)) {
      if constexpr (decltype(hc)::value < HQ) halo_dma(cbeg, cbeg & 1, hc);
    };
    all(IC<0>{}), all(IC<1>{}), all(IC<2>{}), all(IC<3>{}), all(IC<4>{}), all(IC<5>{}), all(IC<6>{}), all(IC<7>{});
    static_assert(HQ <= 8, "extend the list");
  }
  wstage(cbeg, 0, 0, IC<0>{}, IC<WQ>{});
  int g = 0;
  STAMP(unsigned long long t_wait = 0; unsigned long long t_body = 0; unsigned long long t_prev = __builtin_amdgcn_s_memtime();)
  for (int cc = cbeg; cc < nchunk; ++cc) {
    const f16 *halo = lds + (cc & 1) * C::HBUF_HALFS;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky, ++g) {
      const int buf = g & 1;
      STAMP(unsigned long long ta = __builtin_amdgcn_s_memtime();)
      // weights(g) - and at ky=0 the band of this chunk - must have landed.  The band DMAs of the NEXT chunk, issued in
      // group ky=0, are younger than the weights needed at ky=1: a counted vmcnt leaves them in flight there.
      static_assert(halo_wait_allowed(1, true, HQ) == HQ && halo_wait_allowed(1, false, HQ) == 0 && halo_wait_allowed(0, true, HQ) == 0 && halo_wait_allowed(2, true, HQ) == 0,
                    "the condition below is halo_wait_allowed(ky, cc + 1 < nchunk) != 0 (written out: as a call hipcc took more registers)");
      if (ky == 1 && cc + 1 < nchunk) {
        wait_vm_lgkm<HQ>();
      } else {
        wait_vm_lgkm<0>();
      }
      __builtin_amdgcn_s_barrier();
      STAMP(unsigned long long tb = __builtin_amdgcn_s_memtime(); t_wait += tb - ta;)
      __builtin_amdgcn_sched_barrier(0);
      int ncc = cc, nky = ky + 1;
      if (nky == 3) {
        nky = 0;
        ncc = cc + 1;
      }
      const bool more_w = ncc < nchunk, more_h = (ky == 0) && (cc + 1 < nchunk);
      const f16 *wb = wbuf + buf * C::WBUF_HALFS;
      unsigned vm[(NT + 2) / 3];           // keep the per-tap border selects INSIDE the loop: hoisted, their results would not fit the register file
#pragma unroll
      for (int t = 0; t < (NT + 2) / 3; ++t) {
        vm[t] = vmp[t];
        asm volatile("" : "+v"(vm[t]));
      }
      // 6 steps (kx, k-step) x NT pixel tiles = 6 NT tile visits, 2 MFMAs each; pixel fragments rotate through BD registers
      // (the fragment of visit t+BD is requested right after the MFMAs of visit t), weight fragments of step st+1 go to the
      // spare set at the start of step st.  A tap's swizzle term is the same for all tiles of a step (tiles are 32 px apart).
      constexpr int NV = 6 * NT, BD = NT >= 4 ? 4 : (NT == 3 ? 3 : 2);
      half8 af[2][2], bf[BD];
      int tapb[3][2];                      // half offset of (tap pixel, channel group ks*2 + lh) of tile 0
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int Pt = hl_tap(pb, W, ky, kx);
        tapb[kx][0] = ct_frag(Pt, 0, lh);
        tapb[kx][1] = ct_frag(Pt, 1, lh);
      }
      auto load_a = [&](int st, int set) __attribute__((always_inline)) {
        const int kx = st >> 1, ks = st & 1;
#pragma unroll
        for (int i = 0; i < 2; ++i) af[set][i] = *reinterpret_cast<const half8 *>(&wb[wa[ks] + i * CT_TILE32 + hl_w_tap(kx)]);
      };
      auto load_b = [&](auto tc) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value, st = t / NT, j = t % NT, kx = st >> 1, ks = st & 1;
        constexpr int imm = j * CT_TILE32;
        const bool ok = (vm[j / 3] >> hl_vbit(j, ky, kx)) & 1u;
        const int base = ok ? tapb[kx][ks] : hl_zero_base<C>(cc & 1, imm);
        bf[t % BD] = *reinterpret_cast<const half8 *>(&halo[base + imm]);
      };
      load_a(0, 0);
      load_b(IC<0>{});
      load_b(IC<1>{});
      if constexpr (BD > 2) load_b(IC<2>{});
      if constexpr (BD > 3) load_b(IC<3>{});
      __builtin_amdgcn_sched_barrier(0);
      auto visit = [&](auto tc) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value, st = t / NT, j = t % NT, cur = st & 1;
        if constexpr (j == 0 && st + 1 < 6) {
          load_a(st + 1, cur ^ 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[cur][0], bf[t % BD], acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[cur][1], bf[t % BD], acc[1][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (t + BD < NV) load_b(IC<t + BD>{});
        // weight DMAs of the next group in the first visits, the next chunk's band DMAs right after them
        // (program order "weights, then band": the counted vmcnt at ky=1 relies on it)
        static_assert(WQ + HQ <= NV, "DMA issue slots");
        if constexpr (hl_visit_is_w(t, WQ)) {
          if (more_w) wstage(ncc, nky, buf ^ 1, IC<t>{}, IC<t + 1>{});
        } else if constexpr (hl_visit_is_band(t, WQ, HQ)) {
          if (more_h) halo_dma(cc + 1, (cc + 1) & 1, IC<t - WQ>{});
        }
        __builtin_amdgcn_sched_barrier(0);
      };
#define V4(a) visit(IC<(a) < NV ? (a) : NV - 1>{}); if constexpr ((a) + 1 < NV) visit(IC<(a) + 1 < NV ? (a) + 1 : NV - 1>{}); if constexpr ((a) + 2 < NV) visit(IC<(a) + 2 < NV ? (a) + 2 : NV - 1>{}); if constexpr ((a) + 3 < NV) visit(IC<(a) + 3 < NV ? (a) + 3 : NV - 1>{});
      V4(0) if constexpr (NV > 4) { V4(4) } if constexpr (NV > 8) { V4(8) } if constexpr (NV > 12) { V4(12) } if constexpr (NV > 16) { V4(16) } if constexpr (NV > 20) { V4(20) }
#undef V4
      static_assert(NV <= 24, "visit list covers NT = 1 .. 4");
      STAMP(t_body += __builtin_amdgcn_s_memtime() - tb;)
    }
  }
  STAMP(const unsigned long long t_loop_end = __builtin_amdgcn_s_memtime();)

  if constexpr (SPLIT) {
    // fp32 partial sums of this share; splitk_finish adds the shares in a fixed order and applies residual / ReLU / positional embedding
    ct_splitk_store(p, acc, ks, m0 + wn * PXW, c0, wm * 64, lr, lh);
    return;
  }
  halo_epilogue<NT, RES, POST>(p, m0, c0, lds, acc);
  STAMP(if (lane == 0 && blockIdx.x < 4096) {
    unsigned long long *o = g_halo_stamps + ((size_t)blockIdx.x * 8 + wave) * 8;
    o[0] = t_wait; o[1] = t_body; o[2] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 32; o[3] = t_loop_end - t_prev; o[4] = t_prev - t_entry;
    o[5] = __builtin_amdgcn_s_memtime() - t_loop_end; o[6] = r_entry; o[7] = __builtin_amdgcn_s_memrealtime();
  })
}

// Grid = n_main workgroups of 512 px x 128 co (whole rounds), then the rest of the pixels as tiles of nt_tail x 128 px (halo_plan):
// what is less than a round of 512-pixel tiles is cut so that it fills the chip once.  A pixel's arithmetic does not depend on its tile.
template <int W, bool RES, bool POST>
__global__ __launch_bounds__(512, 1) void conv3x3_halo_dma_kernel(ConvArgs p, int n_main, int tile0, int nt_tail) {
  extern __shared__ __attribute__((aligned(16))) f16 lds[];
  constexpr int TMM = 512;
  const int n_ct = p.Cout / HL_BM;
  // tile0: the logical tile at which this launch starts (0: the launch is the whole layer, as launch_halo_dma always makes it)
  if ((int)blockIdx.x < n_main) {
    const CtTile T = ct_grid_main(tile0 + xcd_remap(blockIdx.x, n_main), n_ct, TMM, HL_BM);
    halo_tile_dma<W, 4, RES, POST>(p, T.m0, T.c0, lds);
  } else {
    const CtTile T = hl_grid_tail(xcd_remap(blockIdx.x - n_main, gridDim.x - n_main), tile0 + n_main, n_ct, nt_tail);
    const int m0 = T.m0, c0 = T.c0;
    if (m0 >= p.M) return;
    if (nt_tail == 1) halo_tile_dma<W, 1, RES, POST>(p, m0, c0, lds);
    else if (nt_tail == 2) halo_tile_dma<W, 2, RES, POST>(p, m0, c0, lds);
    else if (nt_tail == 3) halo_tile_dma<W, 3, RES, POST>(p, m0, c0, lds);
    else halo_tile_dma<W, 4, RES, POST>(p, m0, c0, lds);
  }
}


// Split-K form for launches of a few workgroups (3 .. 4 hypotheses; one and two run conv_small.hip since round 5, FP_SMALL=0: this form): every tile is a 128-pixel quarter tile, p.ksplit workgroups
// per tile each take an equal share of the input-channel chunks.  At one hypothesis a 512-channel layer is 16 workgroups that
// each walk 48 weight groups behind one DMA round trip apiece (40 us); four shares of 12 groups + the finishing pass take a third,
// eight shares of 6 (1 and 2 hypotheses: the grid still fits the chip) another 2 % of a one-hypothesis step.
template <int W>
__global__ __launch_bounds__(512, 1) void conv3x3_halo_splitk_kernel(ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) f16 lds[];
  const int n_ct = p.Cout / HL_BM;
  const CtTile T = ct_grid_split(blockIdx.x, p.ksplit, n_ct, 128, HL_BM);
  if (T.m0 >= p.M) return;
  halo_tile_dma<W, 1, false, false, true>(p, T.m0, T.c0, lds, T.ks);
}

// out = [+ pos.emb.] relu?( sum_ks partial[ks] [+ residual] ), one thread per pixel x 4 channels, shares added in order
__global__ __launch_bounds__(256) void splitk_finish_kernel(ConvArgs p) {
  const int q = blockIdx.x * 256 + threadIdx.x, c4 = p.Cout / 4;
  if (q >= p.M * c4) return;
  const int m = q / c4, c = (q - m * c4) * 4;
  float4 v = *reinterpret_cast<const float4 *>(p.splitk + ct_splitk_index(0, m, c, p.M, p.Cout));
  for (int ks = 1; ks < p.ksplit; ++ks) {
    const float4 w = *reinterpret_cast<const float4 *>(p.splitk + ct_splitk_index(ks, m, c, p.M, p.Cout));
    v.x += w.x, v.y += w.y, v.z += w.z, v.w += w.w;
  }
  ct_finish_quad(p, m, c, v);
}


template <int W>
static void halo_lds_all(std::vector<KernelLds> &v) {
  using C = HaloCfgD<W, 512>;
  v.push_back({(const void *)conv3x3_halo_dma_kernel<W, false, false>, C::LDS_BYTES});
  v.push_back({(const void *)conv3x3_halo_dma_kernel<W, true, false>, C::LDS_BYTES});
  v.push_back({(const void *)conv3x3_halo_dma_kernel<W, false, true>, C::LDS_BYTES});
  v.push_back({(const void *)conv3x3_halo_dma_kernel<W, true, true>, C::LDS_BYTES});
  v.push_back({(const void *)conv3x3_halo_splitk_kernel<W>, HaloCfgD<W, 128>::LDS_BYTES});
}
void conv_halo_kernel_lds(std::vector<KernelLds> &v) { halo_lds_all<40>(v), halo_lds_all<20>(v); }

template <int W, bool RES, bool POST>
static int launch_halo_dma(const ConvArgs &a, const ConvPlan &plan, hipStream_t s) {
  using C = HaloCfgD<W, 512>;
  static_assert(HaloCfgD<W, 128>::LDS_BYTES <= C::LDS_BYTES, "tail tiles fit the main tile's LDS");
  if (plan.n_main + plan.n_tail > 0)
    hipLaunchKernelGGL((conv3x3_halo_dma_kernel<W, RES, POST>), dim3(plan.n_main + plan.n_tail), dim3(512), C::LDS_BYTES, s, a, plan.n_main, 0, plan.nt_tail);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

template <int W>
static int launch_halo_dma_flags(const ConvArgs &a, const ConvPlan &plan, hipStream_t s) {
  if (a.post_add) return a.res ? launch_halo_dma<W, true, true>(a, plan, s) : launch_halo_dma<W, false, true>(a, plan, s);
  return a.res ? launch_halo_dma<W, true, false>(a, plan, s) : launch_halo_dma<W, false, false>(a, plan, s);
}

int launch_splitk_finish(const ConvArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(splitk_finish_kernel, dim3((a.M * (a.Cout / 4) + 255) / 256), dim3(256), 0, s, a);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}

template <int W>
static int launch_halo_splitk(const ConvArgs &a, hipStream_t s) {
  using C = HaloCfgD<W, 128>;
  const int n_q = ((a.M + 127) / 128) * (a.Cout / HL_BM);
  hipLaunchKernelGGL((conv3x3_halo_splitk_kernel<W>), dim3(n_q * a.ksplit), dim3(512), C::LDS_BYTES, s, a);
  FP_CHECK_HIP(hipGetLastError());
  return launch_splitk_finish(a, s);
}

int launch_conv_halo(const ConvArgs &a, const ConvPlan &plan, hipStream_t s) {
  FP_REQUIRE(conv_halo_supported(a), "conv3x3: unsupported layer");
  // lane offsets into the input tensor are 32-bit byte offsets from its base
  FP_REQUIRE((double)a.M * a.Cin * 2.0 < 4294967296.0, "conv3x3: input tensor of %.1f GB exceeds the 4 GB the kernel addresses", (double)a.M * a.Cin * 2e-9);
  if (plan.form == CONV_HALO_SPLITK) {
    FP_REQUIRE(a.splitk && a.ksplit == plan.ksplit && (a.Cin / HL_CK) % a.ksplit == 0 && a.out_ld % 4 == 0 && a.coff_hi % 4 == 0,
               "conv3x3 split-K: %d shares do not divide %d chunks", a.ksplit, a.Cin / HL_CK);
    return a.W == 40 ? launch_halo_splitk<40>(a, s) : launch_halo_splitk<20>(a, s);
  }
  return a.W == 40 ? launch_halo_dma_flags<40>(a, plan, s) : launch_halo_dma_flags<20>(a, plan, s);
}
