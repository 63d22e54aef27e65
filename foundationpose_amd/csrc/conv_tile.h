// The 3x3 halo kernels (conv_halo.hip), the generic implicit GEMM (conv.hip) and the tail they share with conv_small.hip: each index
// rule once, and the device pieces with two or more callers.  The host part is plain C++17 and compiles without HIP
// (tests/test_conv_tile_host.py checks it over the kernels' geometries: what a read addresses is what the fill put there, banks, and
// every wait by replaying a wave's vector-memory queue); the device part is __forceinline__.  A kernel whose registers or waits hipcc
// changed through a piece keeps that piece written out and says so (profiles/conv_tile_isa.md).
//
// ROW TILE: rows of 32 fp16 = 64 bytes, UNPADDED, so that the 64 lanes x 16 bytes of an LDS-DMA instruction land linearly as 16 rows x 4
//   chunks.  Row r keeps its logical 16-byte chunk c at position c ^ ((r >> 2) & 3); the swizzle goes on the SOURCE address (an LDS-DMA
//   destination is lane-linear).  A fragment ds_read_b128 reads 32 consecutive rows per lane half, one logical chunk.  The hardware
//   serves it in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (and + 32): each is 16 rows with 16 different row mod 16,
//   hence 16 different (r & 3, (r >> 2) & 3) - conflict free wherever the run starts: the weights, igemm2's pixels, and the halo band
//   at every tile alignment and tap shift.  The same holds for four contiguous 16-lane quarters, the model of the earlier host tests;
//   the host test evaluates both groupings and every bank statement of this header is meant for both unless it says otherwise.  What
//   the old comment did not say: a border lane reads the zero chunk instead, one more address in one bank group, and a band read with
//   border lanes is two-way more often than not (counted in both groupings).
// DMA SLOT s of an image: rows 16 s .. 16 s + 15 at half offset 512 s; lane l is (row 16 s + l / 4, position l & 3).  Linear form (weights;
//   the halo band): the slot's source is a scalar base plus one lane offset.  Gather form (igemm2's activations): one address per lane.
// HALO BAND (HaloCfgD): band index P holds global input pixel GR0 * W + P - 1, clamped to the tensor; NB entries are in use, BPX allocated.
//   Output pixel m reads tap (ky, kx) at band index pb + ky * W + kx, pb = m - GR0 * W - W.  What lands from a clamped source is never read
//   by a pixel < M: a band row outside the tensor, the next image's rows behind a y-border tap and the wrapped row ends at the x-borders
//   all have their validity bit clear and read the zero chunk.  The lanes of a ragged last tile whose pixel is >= M carry the validity
//   bits of pixel M - 1 at their own band position and may read such entries (finite tensor data); their sums are never stored.
// WAITS of the halo loop: at the barrier of group (cc, ky) the weights of the group and, at ky == 0, the band of chunk cc must have
//   landed.  Visit t of a group issues weights (t < WQ, next group) and then band (t - WQ < HQ, next chunk, in group ky == 0 only):
//   program order "weights, then band".  So at ky == 1 the youngest HQ operations are the next chunk's band and may stay in flight; at
//   ky == 0 and ky == 2 the group's weights are the youngest operations of the queue.  halo_wait_allowed() is safe and tight at every
//   barrier (the host test replays the queue and asserts both).
// RING of igemm2: stage kt sits in slot kt % 3, DMAW = NT + WQ instructions per wave per stage; at the barrier of step kt only stage
//   kt + 1 (if any) is younger than stage kt (stage kt + 2 is issued behind the barrier): DMAW or 0, tight.  Slot (kt + 2) % 3 was last
//   read in step kt - 1.
// ACCUMULATORS: acc_row_token / acc_row_chan of tok_tile.h (pixel j * 32 + lr, channels wm * WM + i * 32 + rg * 8 + lh * 4 + e).
// STAGED EPILOGUE: rows of BM + 8 halfs; a lane reads (residual) and overwrites (result) the same 8-byte slots, which no other lane
//   touches, so no barrier is needed in between; the tile leaves in 16-byte row pieces.  The 8-byte writes are two-way (lanes lr and
//   lr + 8; ds_write_b64 is served in contiguous quarters).  The 16-byte reads are two-way in the hardware's ds_read_b128 groups at both
//   widths (a group takes lanes of two rows, 272 or 144 bytes apart); in the contiguous-quarter model BM = 128 is conflict free.
// READ BY THE TEST ONLY: a rule marked [restated] below is not what a kernel compiles - the kernel keeps that piece written out
//   (profiles/conv_tile_isa.md) and only the bits fixture of tests/test_gpu_kernels.py ties its text to this statement.  Change both.
// Association of an address sum is part of a rule: helpers that form addresses keep the order of the terms the kernels had.
#pragma once
#include <stddef.h>
#include "conv_plan.h"
#include "tok_tile.h"

// ---- host part: the index rules ----
constexpr int HL_SLD = HL_BM + 8;                // halfs per staged output row of the halo tile (272 B)
constexpr int C2_BN = 256;                       // pixels of igemm2's main tile

// -- 64-byte row tile --
constexpr int ct_chunk(int row, int c) { return c ^ ((row >> 2) & 3); }                     // logical <-> stored chunk (an involution)
constexpr int ct_off(int row, int k) { return row * 32 + ct_chunk(row, k >> 3) * 8 + (k & 7); }      // half offset of element (row, k) [the test's inverse of the maps below]
// fragment (ks, lh) of row: k elements ks * 16 + lh * 8 .. + 8.  Rows + 32 keep the swizzle: tile i / j of a wave is + i * 32 * 32
constexpr int ct_frag(int row, int ks, int lh) { return row * 32 + ct_chunk(row, ks * 2 + lh) * 8; }
constexpr int CT_TILE32 = 32 * 32;               // halfs between the fragments of rows r and r + 32

// -- DMA maps --
constexpr int ct_dma_slot(int q, int waves, int wave) { return q * waves + wave; }          // instruction q of wave `wave`
constexpr int ct_dma_row(int slot, int lane) { return slot * 16 + (lane >> 2); }
constexpr int ct_dma_chunk(int row, int lane) { return ct_chunk(row, lane & 3); }           // the logical chunk that lands at the lane's 16 bytes
constexpr int ct_dma_lds(int slot) { return slot * 512; }                                   // half offset of the slot (+ 8 * lane)
// linear form, [.][ld] rows: byte offset of the lane's 16 bytes from the source of slot 0's row 0, for slot = wave.  A lane's row is
// slot * 16 + lane / 4, so its swizzle term (row >> 2) & 3 = (lane >> 4) & 3 is the same in every slot (hence ct_dma_chunk on the row
// lane / 4 of slot 0): ONE lane offset serves every instruction of a wave, the slot's other rows are a scalar base.  [restated: both
// kernels write woff out]
constexpr unsigned ct_w_off(int wave, int lane, int ld) { return (unsigned)((ct_dma_row(wave, lane) * ld + ct_dma_chunk(lane >> 2, lane) * 8) * 2); }

// -- halo band --
template <int W, int TM>
struct HaloCfgD {
  static constexpr int MAXSLOT = (W - 1 + TM - 1) / W + 1 + 2;     // band rows: the tile's rows and one above, one below
  static constexpr int NB = MAXSLOT * W + 2;                       // band pixels in use (pixel p at index p+1)
  static constexpr int HQ = ((NB + 15) / 16 + 7) / 8;              // halo DMA instructions per wave per chunk (8 waves)
  static constexpr int BPX = HQ * 8 * 16;                          // band pixels allocated
  static constexpr int HBUF_HALFS = BPX * 32;
  static constexpr int ZERO_OFF = 2 * HBUF_HALFS;                  // half offset of the zero chunk
  static constexpr int WBUF_OFF = ZERO_OFF + 8;
  static constexpr int WBUF_HALFS = 3 * HL_BM * HL_CK;
  static constexpr int LDS_HALFS_MAIN = WBUF_OFF + 2 * WBUF_HALFS;
  static constexpr int LDS_HALFS_EPI = TM * HL_SLD;
  static constexpr int LDS_BYTES = 2 * (LDS_HALFS_MAIN > LDS_HALFS_EPI ? LDS_HALFS_MAIN : LDS_HALFS_EPI);
};
constexpr int hl_gr0(int m0, int W) { return m0 / W - 1; }                                  // global input row (n*H + iy) held by band row 0
constexpr int hl_band_pixel(int GR0, int W, int P) { return GR0 * W + P - 1; }              // global input pixel of band index P, unclamped
constexpr int hl_band_src(int GR0, int W, int P, int hpix_max) {                            // ... as the DMA fetches it [restated: halo_dma writes slot, row, chunk and clamp out]
  return hl_band_pixel(GR0, W, P) < 0 ? 0 : (hl_band_pixel(GR0, W, P) > hpix_max ? hpix_max : hl_band_pixel(GR0, W, P));
}
constexpr int hl_pb(int m, int GR0, int W) { return m - GR0 * W - W; }                      // band index of tap (0, 0) of output pixel m
constexpr int hl_tap(int pb, int W, int ky, int kx) { return pb + ky * W + kx; }
constexpr bool hl_tap_valid(int oy, int ox, int W, int ky, int kx) {                        // (square maps: H = W)
  return oy + ky - 1 >= 0 && oy + ky - 1 < W && ox + kx - 1 >= 0 && ox + kx - 1 < W;
}
constexpr int hl_vbit(int j, int ky, int kx) { return (j % 3) * 9 + ky * 3 + kx; }          // bit of tile j's tap in register j / 3
// the zero chunk as a fragment base: what, read at + imm in band buffer hb, addresses the zero chunk
template <class C> constexpr int hl_zero_base(int hb, int imm) { return C::ZERO_OFF - hb * C::HBUF_HALFS - imm; }

// -- weight stage of the halo kernel: a kernel row's 3 taps x 128 co x 32 ci as 24 slots; slot g holds rows (g & 7) * 16 .. of tap kx = g >> 3
// [hl_w_row, hl_w_kx, hl_w_src restated: wstage writes its source out]
constexpr int HL_WSLOTS = 24;
constexpr int hl_w_row(int g) { return (g & 7) * 16; }
constexpr int hl_w_kx(int g) { return g >> 3; }
constexpr size_t hl_w_src(int c0, int g0, int ky, int cc, int Kpad, int Cin) {               // element of w that slot g0's row 0, chunk 0 is
  return (size_t)(c0 + hl_w_row(g0)) * Kpad + (ky * 3 + hl_w_kx(g0)) * Cin + cc * HL_CK;
}
constexpr int hl_w_tap(int kx) { return kx * (HL_BM * HL_CK); }                             // half offset of tap kx's image
// -- wait rule and issue slots of the halo loop --
constexpr int halo_wait_allowed(int ky, bool has_next_chunk, int HQ) { return ky == 1 && has_next_chunk ? HQ : 0; }      // [the kernel's own condition is tied to this by a static_assert]
constexpr bool hl_visit_is_w(int t, int WQ) { return t < WQ; }
constexpr bool hl_visit_is_band(int t, int WQ, int HQ) { return t >= WQ && t - WQ < HQ; }

// -- igemm2: stages and ring --
constexpr int c2_wq(int BM) { return BM / 64; }                                             // weight DMA instructions per wave per stage
constexpr int c2_dmaw(int NT, int BM) { return NT + c2_wq(BM); }
constexpr int c2_slot(int kt) { return kt % 3; }
constexpr int c2_stage_halfs(int NT, int BM) { return 64 * NT * C2_BK + BM * C2_BK; }        // pixels, then weights
constexpr int c2_wait_allowed(int kt, int nk, int DMAW) { return kt + 1 < nk ? DMAW : 0; }
constexpr int c2_lds_bytes(int BM) {
  return 3 * c2_stage_halfs(4, BM) * 2 > C2_BN * (BM + 8) * 2 ? 3 * c2_stage_halfs(4, BM) * 2 : C2_BN * (BM + 8) * 2;
}

// -- staged epilogue --
constexpr int ct_stage_ld(int BM) { return BM + 8; }
constexpr int ct_stage_off(int BM, int px, int col) { return px * ct_stage_ld(BM) + col; }  // a lane's quad: col = wm * WM + acc_row_chan(i, rg, lh)
constexpr int ct_piece_px(int idx, int BM) { return idx / (BM / 8); }                       // 16-byte row piece idx of a tile [both restated: the kernels' loops write idx >> 4, idx / CPR]
constexpr int ct_piece_c16(int idx, int BM) { return idx % (BM / 8); }

// -- split-K scratch [ks][m][Cout], output placement --
constexpr size_t ct_splitk_index(int ks, int m, int c, int M, int Cout) { return ((size_t)ks * M + m) * Cout + c; }
constexpr long long ct_out_row(int m, int split_m) { return m >= split_m ? (long long)(m - split_m) : (long long)m; }
constexpr int ct_out_col(int m, int split_m, int coff_hi) { return m >= split_m ? coff_hi : 0; }

// -- grid maps: logical index (behind xcd_remap, a permutation) -> tile --
struct CtTile {
  int m0, c0, ks;
};
constexpr CtTile ct_grid_main(int L, int n_ct, int TM, int BM) { return {(L / n_ct) * TM, (L % n_ct) * BM, 0}; }
constexpr CtTile ct_grid_split(int b, int ksplit, int n_ct, int TM, int BM) { return {(b / ksplit / n_ct) * TM, (b / ksplit % n_ct) * BM, b % ksplit}; }
// halo: tail tile t of nt_tail x 128 pixels behind `first` main tiles (tile0 + n_main)
constexpr CtTile hl_grid_tail(int t, int first, int n_ct, int nt_tail) { return {(first / n_ct) * 512 + (t / n_ct) * (nt_tail * 128), (t % n_ct) * HL_BM, 0}; }
// igemm2: tail tile t is quarter t & 3 of main-size tile n_main + t / 4
constexpr CtTile c2_grid_tail(int t, int n_main, int n_ct, int BM) {
  return {((n_main + (t >> 2)) / n_ct) * C2_BN + (t & 3) * (C2_BN / 4), ((n_main + (t >> 2)) % n_ct) * BM, 0};
}

#ifdef __HIPCC__
#include "device_util.h"

// ---- first half of output row m's place: rows from split_m on go to row m - split_m, column coff_hi (T: f16 or float rows) ----
template <typename T = f16>
__device__ __forceinline__ T *ct_out_ptr(const ConvArgs &p, int m) {
  return (T *)p.out + ct_out_row(m, p.split_m) * p.out_ld + ct_out_col(m, p.split_m, p.coff_hi);
}

// ---- fp32 partial sums of share ks -> p.splitk[ks][m][Cout], 16-byte stores in the accumulator layout; mw: the wave's first pixel, c0 +
// wcol: its first channel ----
template <int MT, int NT>
__device__ __forceinline__ void ct_splitk_store(const ConvArgs &p, const floatx16 (&acc)[MT][NT], int ks, int mw, int c0, int wcol, int lr, int lh) {
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int m = mw + acc_row_token(j, lr);
    if (m >= p.M) continue;
    float *o = p.splitk + ct_splitk_index(ks, m, 0, p.M, p.Cout) + c0 + wcol + acc_row_chan(0, 0, lh);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg)
        *reinterpret_cast<float4 *>(o + acc_row_chan(i, rg, 0)) = make_float4(acc[i][j][rg * 4 + 0], acc[i][j][rg * 4 + 1], acc[i][j][rg * 4 + 2], acc[i][j][rg * 4 + 3]);
  }
}

// ---- tail of splitk_finish_kernel and conv3x3_small_kernel: fp32 quad of pixel m, channels c .. c + 3 (the bias inside) -> (+ residual)
// -> ReLU -> (+ post-add) -> one rounding to fp16 -> its place ----
__device__ __forceinline__ void ct_finish_quad(const ConvArgs &p, int m, int c, float4 v) {
  if (p.res) {
    const half4 r = *reinterpret_cast<const half4 *>(p.res + (size_t)m * p.Cout + c);
    v.x += (float)r[0], v.y += (float)r[1], v.z += (float)r[2], v.w += (float)r[3];
  }
  const float lo = p.relu ? 0.f : -__builtin_inff();
  v.x = fmaxf(v.x, lo), v.y = fmaxf(v.y, lo), v.z = fmaxf(v.z, lo), v.w = fmaxf(v.w, lo);
  if (p.post_add) {
    const float4 pv = *reinterpret_cast<const float4 *>(p.post_add + (size_t)(m % p.post_period) * p.Cout + c);
    v.x += pv.x, v.y += pv.y, v.z += pv.z, v.w += pv.w;
  }
  half4 hv;
  hv[0] = (f16)v.x, hv[1] = (f16)v.y, hv[2] = (f16)v.z, hv[3] = (f16)v.w;
  *reinterpret_cast<half4 *>(ct_out_ptr(p, m) + c) = hv;
}
#endif
