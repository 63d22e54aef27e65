// The token GEMMs of the transformer heads (tok_gemm.hip, tok_qkv.hip, head_mlp.hip; conv.hip's V-image writer, pack_tok_weights in
// net.hip): each index rule of their layouts once, and the device pieces they share - tile DMA, weight prefetch, the two K loops, the fp16
// conversion of an accumulator quad, the group-sum store, the V-image store.  The host part is plain C++17 and compiles without HIP (tests/test_tok_tile_host.py checks
// it over the kernels' geometries); the device part is __forceinline__.  A kernel whose registers or waits hipcc changed through a
// piece keeps that piece written out and says so.
//
// TILE: ROWS tokens x 512 fp16 resident in LDS as [k segment of 128][row][256 B]; 16-byte chunk c of a row segment is stored at
//   c ^ (row & 15): the 16 lanes of a quarter of a fragment ds_read_b128 (16 consecutive rows, one chunk) cover all 64 banks once.
// RING (head_mlp128_kernel): a slot is 64 k of ROWS rows, [row][128 B], chunk c (0 .. 7) at c ^ (row & 7).  Two rows share 256 bytes, so
//   rows r and r + 8 of a quarter meet in a bank group: its fragment reads are two-way.
// ACCUMULATORS: v_mfma_f32_32x32x16_f16, lane (lr = lane & 31, lh = lane >> 5), tile (i, j) of a wave whose first column is col0.
//   row layout:  register rg*4 + e holds token j*32 + lr, channel col0 + i*32 + rg*8 + lh*4 + e - four consecutive channels are an
//                8-byte half chunk of the tile layout, so an epilogue can write the next layer's A tile in place;
//   swapped (V): register r holds channel col0 + i*32 + lr, token j*32 + (r & 3) + 8*(r >> 2) + 4*lh.
// WEIGHTS: [wave4 4][k16 32][i4 4][lane 64][8 halfs]: fragment (wave4, k16, i4) is one coalesced 1-KB load; lane (lr, lh) holds
//   W[wave4*128 + i4*32 + lr][k16*16 + lh*8 .. +8].
// V IMAGE: [b][4 heads][128][416], token t of a hypothesis in column vt_col(t), columns tokens .. 415 zero.
// Include order: none for the host part (it needs <stddef.h> only).  The device part includes device_util.h, which includes common.h: a
// kernel file may include this header first.  Everything is in the global namespace, like conv_band.h's rules.
#pragma once
#include <stddef.h>

// ---- host part: the index rules ----
constexpr int TOK_K = 512;                       // columns of a token row, input and output
constexpr int VT_LD = 416;                       // columns of a V image row

// -- tile --
constexpr int tile_seg_bytes(int ROWS) { return ROWS * 256; }
constexpr int tile_chunk(int row, int c) { return c ^ (row & 15); }                        // logical <-> stored chunk of a row segment (an involution)
constexpr int tile_off(int ROWS, int row, int k) {                                         // byte offset of element (row, k)
  return (k >> 7) * tile_seg_bytes(ROWS) + row * 256 + tile_chunk(row, (k >> 3) & 15) * 16 + (k & 7) * 2;
}
// DMA instruction (k segment seg, row quad r4 = wave * (ROWS / 4 / WAVES) + u), lane l: row r4*4 + l/16, stored chunk l & 15 (an LDS-DMA
// destination is lane-linear: the swizzle goes on the source address); rows past M repeat row M - 1
constexpr int tile_dma_r4(int ROWS, int WAVES, int wave, int u) { return wave * (ROWS / 4 / WAVES) + u; }
constexpr int tile_dma_row(int r4, int lane) { return r4 * 4 + (lane >> 4); }
constexpr int tile_dma_chunk(int row, int lane) { return tile_chunk(row, lane & 15); }     // the logical chunk that lands at the lane's 16 bytes
constexpr int tile_dma_lds(int ROWS, int seg, int r4) { return seg * tile_seg_bytes(ROWS) + r4 * 1024; }      // + 16 * lane
constexpr int tok_src_row(int m0, int row, int M) { return m0 + row < M - 1 ? m0 + row : M - 1; }
constexpr size_t tok_src_bytes(int m, int k0, int chunk) { return ((size_t)m * TOK_K + k0 + chunk * 8) * 2; }      // byte offset of element (m, k0 + 8 chunk) of an [M][512] tensor
// fragment (k16, j) of a K loop = rows j*32 + lr, k elements k16*16 + lh*8 .. +8.  Table form: base row lr, plus xo[k16 & 7]
constexpr int tile_frag_xo(int s, int lr, int lh) { return tile_chunk(lr, 2 * s + lh) * 16; }
constexpr int tile_frag_addr(int ROWS, int k16, int j, int lr, int lh) { return lr * 256 + (k16 >> 3) * tile_seg_bytes(ROWS) + j * 8192 + tile_frag_xo(k16 & 7, lr, lh); }
// split form: the odd bit of the XOR and the row sit in the base, the even part (xe) is applied per k-step (one v_xor)
constexpr int tile_frag_base(int lr, int lh) { return lr * 256 + ((lh ^ (lr & 1)) * 16); }
constexpr unsigned tile_frag_xe(int lr) { return (unsigned)(lr & 14); }
constexpr int tile_frag_seg(int ROWS, int k16) { return (k16 >> 3) * tile_seg_bytes(ROWS); }
constexpr unsigned tile_frag_x(int k16, unsigned xe) { return ((unsigned)(2 * (k16 & 7)) ^ xe) << 4; }      // address = base + seg + x + j * 8192
// a wave of WAVES (4 / 8) owns columns wave * 512 / WAVES ..: k segment and chunk of its register quad rg of tile i, and the 8-byte half
// chunk that holds the quad's channels (.. + i*32 + rg*8 + lh*4 .. +3) of `row` - where a lane of the row layout finds / puts them
template <int WAVES> constexpr int quad_seg(int wave) { return WAVES == 4 ? wave : wave >> 1; }
template <int WAVES> constexpr int quad_chunk(int wave, int i, int rg) { return (WAVES == 4 ? 0 : (wave & 1) * 8) + i * 4 + rg; }
template <int ROWS, int WAVES> constexpr int tile_quad_off(int wave, int i, int rg, int row, int lh) {
  return quad_seg<WAVES>(wave) * tile_seg_bytes(ROWS) + row * 256 + tile_chunk(row, quad_chunk<WAVES>(wave, i, rg)) * 16 + lh * 8;
}

// -- ring slot --
constexpr int ring_slot_bytes(int ROWS) { return ROWS * 128; }
constexpr int ring_chunk(int row, int c) { return c ^ (row & 7); }
constexpr int ring_off(int row, int k) { return row * 128 + ring_chunk(row, (k >> 3) & 7) * 16 + (k & 7) * 2; }      // k: 0 .. 63 inside the segment
// DMA instruction r8 = wave*2 + u, lane l: row r8*8 + l/8, stored chunk l & 7; destination r8 * 1024 + 16 * lane
constexpr int ring_dma_row(int r8, int lane) { return r8 * 8 + (lane >> 3); }
constexpr int ring_dma_chunk(int row, int lane) { return ring_chunk(row, lane & 7); }
constexpr int ring_frag_base(int lr, int lh) { return lr * 128 + ((lh ^ (lr & 1)) * 16); }
constexpr unsigned ring_frag_xe(int lr) { return (unsigned)(lr & 6); }
constexpr int ring_frag_slot(int ROWS, int k16) { return ((k16 >> 2) & 1) * ring_slot_bytes(ROWS); }
constexpr unsigned ring_frag_x(int k16, unsigned xe) { return ((unsigned)(2 * (k16 & 3)) ^ xe) << 4; }      // address = base + slot + x + j * 4096

// -- accumulator layout --
constexpr int acc_row_token(int j, int lr) { return j * 32 + lr; }
constexpr int acc_row_chan(int i, int rg, int lh) { return i * 32 + rg * 8 + lh * 4; }    // + e, + col0
constexpr int acc_vt_chan(int i, int lr) { return i * 32 + lr; }                           // + col0
constexpr int acc_vt_token(int j, int r, int lh) { return j * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh; }

// -- weight fragments --
constexpr size_t wfrag(int wave4, int k16, int i4) { return ((size_t)wave4 * 32 + k16) * 4 + i4; }      // fragment number; a fragment is 64 lanes x 8 halfs
constexpr size_t wfrag_src(int wave4, int k16, int i4, int lane) {                         // index in W[512][512] of the first of the lane's 8 elements
  return (size_t)(wave4 * 128 + i4 * 32 + (lane & 31)) * TOK_K + k16 * 16 + (lane >> 5) * 8;
}
// ownership: 4 waves x 128 columns (tok_gemm.hip); 8 waves x 64 columns (tok_qkv_kernel, head_mlp.hip); the few-image kernel's (column
// quarter g, K quarter kq, column half chh) with k = 0 .. 7 inside the quarter
constexpr size_t wfrag_own4(int wave, int k16, int i) { return wfrag(wave, k16, i); }
constexpr size_t wfrag_own8(int wave, int k16, int i) { return wfrag(wave >> 1, k16, (wave & 1) * 2 + i); }
constexpr size_t wfrag_own_small(int g, int kq, int chh, int k, int i) { return wfrag(g, kq * 8 + k, chh * 2 + i); }

// -- V image --
// Column of token t.  Within each group of 16 tokens the order is {0-3, 8-11, 4-7, 12-15}: the 8 keys that one lane half of the attention
// kernel's P^T operand carries (the S^T accumulator registers of a k-step) are then 16 contiguous bytes - one ds_read_b128 per V^T fragment.
constexpr int vt_col(int t) { return (t & ~15) | (((t >> 2) & 1) << 3) | (((t >> 3) & 1) << 2) | (t & 3); }
constexpr size_t vt_row(int b, int col) { return (((size_t)b * 4 + (col >> 7)) * 128 + (col & 127)) * VT_LD; }      // first element of channel col (0 .. 511)
constexpr size_t vt_index(int b, int col, int t) { return vt_row(b, col) + vt_col(t); }
// tokens % 16 == 0: the 16 tokens from m (a multiple of 16) on lie in one hypothesis - m / tokens - and fill columns t .. t + 15 of it
constexpr int vt_group_hyp(int m, int tokens) { return m / tokens; }
constexpr bool vt_group_is_last(int t16, int tokens) { return t16 + 16 == tokens; }       // its writers also zero columns tokens .. 415
// epilogue staging.  The 8-byte writes of the accumulator quads are two-way in all four layouts (lanes lr and lr + 8 of a quarter); the
// 16-byte read-backs are conflict free, but for one pair of lanes per quarter of tok_gemm.hip's V read-back.
// tok_gemm.hip, per wave: rows of 128 columns (256 B + 16 B pad) / channel rows of 64 tokens (128 B + 16 B pad), in halfs
constexpr int TG_STAGE_LD = 136, TG_VT_LD = 72;
constexpr int tg_stage_off(int row, int col) { return row * TG_STAGE_LD + col; }
constexpr int tg_vt_off(int ch, int pos) { return ch * TG_VT_LD + pos; }
// tok_qkv.hip, per wave and 32-token slice, 4 KB (bytes): 32 rows x 64 columns, 16-byte unit u of a row at u ^ (row & 7); 64 channels x 32
// image columns, unit u of a channel row at u ^ ((ch >> 1) & 3)
constexpr int tq_stage_off(int row, int col) { return row * 128 + (((col >> 3) ^ (row & 7)) * 16) + (col & 7) * 2; }
constexpr int tq_vt_off(int ch, int pos) { return ch * 64 + (((pos >> 3) ^ ((ch >> 1) & 3)) * 16) + (pos & 7) * 2; }

#ifdef __HIPCC__
#include "device_util.h"

// ---- lane coordinates.  Filled in by each kernel itself (through a shared init function, by reference or by value, head_mlp_kernel's
// registers and waits change); a helper takes them BY VALUE (by reference the fields are memory its stores may alias until it is
// inlined: other waits) ----
struct TokLane {
  int lane, wave, lr, lh;
};
// ---- tile fill: ROWS rows x 512 fp16 of `src` from row m0 on -> the tile at LDS byte address lds0; ROWS / WAVES instructions per wave.
// PIN_LANE: the lane offsets are recomputed per call - hoisted out of a loop over tiles they would live across the K loops.
template <int ROWS, int WAVES, bool PIN_LANE = false>
__device__ __forceinline__ void tok_tile_dma(const f16 *src, int m0, int M, int wave, int lane, unsigned lds0) {
  constexpr int U = ROWS / 4 / WAVES;
  if constexpr (PIN_LANE) asm volatile("" : "+v"(lane));
#pragma unroll
  for (int seg = 0; seg < 4; ++seg)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r4 = tile_dma_r4(ROWS, WAVES, wave, u), row = tile_dma_row(r4, lane);
      const unsigned voff = (unsigned)tok_src_bytes(tok_src_row(m0, row, M), seg * 128, tile_dma_chunk(row, lane));
      glds16(src, voff, lds0 + tile_dma_lds(ROWS, seg, r4));
    }
}

// ---- weight stream: wp = the wave's fragment (., 0, first i) + lane; fragment (k16, i) from there is wp[wfrag(0, k16, i) * 64] ----
template <int D, int NI>
__device__ __forceinline__ void tok_w_prefetch(u32x4 (&wr)[D][NI], const u32x4 *wp) {
#pragma unroll
  for (int d = 0; d < D; ++d)
#pragma unroll
    for (int i = 0; i < NI; ++i) wr[d][i] = wp[wfrag(0, d, i) * 64];
}

// ---- K loop, double-buffered token fragments (64-token tiles): acc[i][j] += tile (rows j*32 ..) x W^T (the wave's column tile i), weights D
// k-steps ahead (tok_w_prefetch first).  xb = tile + lr * 256.  VT: operands swapped (a lane owns a channel).
template <int NI, int D, bool VT>
__device__ __forceinline__ void tok_kloop_db(u32x4 (&wr)[D][NI], const u32x4 *wp, const unsigned char *xb, const unsigned (&xo)[8], floatx16 (&acc)[NI][2]) {
  half8 bf[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j) bf[0][j] = *reinterpret_cast<const half8 *>(xb + j * 8192 + xo[0]);
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const int cur = k & 1, slot = k % D;
    half8 af[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) af[i] = *reinterpret_cast<half8 *>(&wr[slot][i]);
    __builtin_amdgcn_sched_barrier(0);      // pin the prefetch: hipcc otherwise sinks the loads next to their use (distance 1)
    if (k + D < 32) {
#pragma unroll
      for (int i = 0; i < NI; ++i) wr[slot][i] = wp[wfrag(0, k + D, i) * 64];
    }
    if (k + 1 < 32) {
      const int kn = k + 1;
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[cur ^ 1][j] = *reinterpret_cast<const half8 *>(xb + (kn >> 3) * tile_seg_bytes(64) + j * 8192 + xo[kn & 7]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        if constexpr (VT) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bf[cur][j], af[i], acc[i][j], 0, 0, 0);
        else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[cur][j], acc[i][j], 0, 0, 0);
      }
  }
}

// ---- K loop, 128-token tiles, 8 waves x 64 columns: the four token fragments of a k-step rotate through ONE register set - the fragment
// of (k + 1, j) is requested right behind the MFMAs of (k, j), six MFMAs (192 cycles) cover its latency.  Weights 3 k-steps ahead
// (tok_w_prefetch first).  C0: the C operand of the first k-step's MFMAs (the bias without 128 register copies), or null: what acc holds.
template <bool VT, bool C0>
__device__ __forceinline__ void tok_kloop_rot(u32x4 (&wr)[3][2], const u32x4 *wp, const unsigned char *tile, int lr, int lh, floatx16 (&acc)[2][4], const floatx16 *c0) {
  const unsigned char *xb = tile + tile_frag_base(lr, lh);
  const unsigned xe = tile_frag_xe(lr);
  half8 bf[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bf[j] = *reinterpret_cast<const half8 *>(xb + j * 8192 + tile_frag_x(0, xe));
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const int slot = k % 3;
    half8 af[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<half8 *>(&wr[slot][i]);
    __builtin_amdgcn_sched_barrier(0);      // pin the prefetch (hipcc otherwise sinks the loads next to their use)
    if (k + 3 < 32) {
#pragma unroll
      for (int i = 0; i < 2; ++i) wr[slot][i] = wp[wfrag(0, k + 3, i) * 64];
    }
    const int kn = k + 1;
    const unsigned char *xn = xb + tile_frag_seg(128, kn) + tile_frag_x(kn, xe);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if constexpr (VT) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bf[j], af[i], acc[i][j], 0, 0, 0);
        else if constexpr (C0) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], k == 0 ? c0[i] : acc[i][j], 0, 0, 0);
        else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (kn < 32) bf[j] = *reinterpret_cast<const half8 *>(xn + j * 8192);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// ---- epilogue pieces of the row layout; a wave owns columns wave * NI * 32 .. of the 512 (WAVES * NI == 16) ----
// register quad rg of an accumulator tile -> fp16
__device__ __forceinline__ half4 acc_quad_f16(const floatx16 &a, int rg) {
  half4 hv;
#pragma unroll
  for (int e = 0; e < 4; ++e) hv[e] = (f16)a[rg * 4 + e];
  return hv;
}
__device__ __forceinline__ half4 relu4(half4 hv) { return __builtin_elementwise_max(hv, half4{(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f}); }

// sums of acc * rstd over groups of 16 tokens (lanes lr 0-15 / 16-31 of a token tile = one DPP row each) -> gsum[group][512]; 16 divides the
// tokens of a hypothesis, so a group never spans two
template <int NI>
__device__ __forceinline__ void tok_gsum_store(const TokLane c, const floatx16 (&acc)[NI][2], const float (&rstd)[2], int m0, int M, float *gsum) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = row16_sum(acc[i][j][rg * 4 + e] * rstd[j]);
        const int g = (m0 + j * 32 + (c.lr & 16)) >> 4;          // global 16-token group
        if ((c.lr & 15) == 0 && g * 16 < M)
          // acc_row_chan is linear in (i, rg, lh): the lane's part and the constant part of the column as two terms, constant last (as one
          // term every store forms its own 64-bit address: 31 more adds)
          *reinterpret_cast<float4 *>(gsum + (size_t)g * 512 + c.wave * (NI * 32) + acc_row_chan(0, 0, c.lh) + acc_row_chan(i, rg, 0)) = make_float4(v[0], v[1], v[2], v[3]);
      }
}

// ---- V image: one staged 16-byte unit = 8 image columns of channel `col`, half `hf` (0 / 1) of the 16-token group that holds token m (a
// multiple of 8; the caller checked m < M).  The image is 416 columns wide: the lanes that store a hypothesis' last 16 tokens also zero
// the columns behind them (the attention kernel reads whole 64-key blocks).
__device__ __forceinline__ void vt_store_unit(f16 *img, int col, int m, int tokens, int hf, uint4 v) {
  const int b = vt_group_hyp(m, tokens), t = m - b * tokens;
  f16 *row = img + vt_row(b, col);
  *reinterpret_cast<uint4 *>(row + (t & ~15) + hf * 8) = v;
  if (vt_group_is_last(t & ~15, tokens))
    for (int z = tokens; z < VT_LD; z += 16) *reinterpret_cast<uint4 *>(row + z + hf * 8) = uint4{0u, 0u, 0u, 0u};
}
#endif
