// The attention kernels of the transformer heads (attn.hip: attention_kernel, attention_small_kernel): each index rule of their layouts, DMA
// slots and wait counts once.  The host part is plain C++17 and compiles without HIP (tests/test_attn_tile_host.py checks it at
// T = 400, 384, 230, 130, 64, 37, 1); the device part holds the pieces the kernels share.  A kernel whose registers, scratch or waits hipcc
// changed through a piece keeps that piece written out and says so.
//
// SOURCES: q | k rows [B*T][1024] fp16, Q of head h at column h*128, K at 512 + h*128; the transposed V image [b][4][128][416] (tok_tile.h),
//   token t in column vt_col(t), columns T .. 415 zero.  Output rows [B*T][512], head h at column h*128.
// ITEMS (attention_kernel): item L = (hypothesis b, head h, block qb of FA_QB = 224 queries), qb fastest; wave w of 7 owns queries
//   qb*224 + w*32 + lr.  Persistent workgroup j walks the virtual ids v = j, j + G, j + 2G, ... (< n_items); L = xcd_remap(v, n_items).
// STAGE (one key block of 64, 32 KB, a ring of FA_NSTAGE = 3 slots): 32 DMA instructions of 1 KB, destination i * 1024 + 16 * lane.
//   i < 16, K block [64 keys][256 B]: position c = i*64 + lane holds key c >> 4, stored chunk c & 15 = logical chunk ^ (key & 15);
//   i >= 16, V^T block [128 dims][128 B] from byte 16384: c = (i-16)*64 + lane holds dim c >> 3, stored chunk c & 7 = logical chunk (8 image
//   columns) ^ ((dim >> 1) & 7).  The swizzle goes on the SOURCE address (an LDS-DMA destination is lane-linear).  Wave w issues the
//   instructions w + 7u (mod 32), u = 0 .. 4: 35 for 32, the 3 surplus ones repeat an earlier one (same bytes) so that every wave issues
//   exactly 5 (the wait counts below).  K rows past T repeat row T - 1 (their scores are masked in the tail block); V^T chunks past column
//   408 repeat the chunk at 408, the last of the zero pad (P is exactly 0 past T: the operand must only be finite).
//   Both fragment reads (a quarter of a ds_read_b128 = 16 consecutive rows, one logical chunk) are conflict free: K rows are 256 bytes, so
//   the bank group is chunk ^ (row & 15); V^T rows are 128 bytes, two per 256, so it is (row & 1) * 8 + (chunk ^ ((row >> 1) & 7)).
// Q^T (per wave 8 KB, fragment order): DMA instruction s, lane (lr, lh) brings dims 16s + 8lh .. + 8 of query row min(w*32 + lr, T-1 - qb*224)
//   of the block to s * 1024 + 16 * lane; fragment s is one lane-linear (conflict-free) ds_read_b128 of the same position.
// ACCUMULATORS (v_mfma_f32_32x32x16_f16, operands swapped: a lane owns a query column lr): S^T register r of key tile kt holds key
//   kt*32 + (r & 3) + 8*(r >> 2) + 4*lh of the block (tok_tile.h's acc_vt_token).  Registers 8*s2 .. 8*s2 + 7 of tile kt ARE the B operand
//   (P^T) of k-step kt*2 + s2: keys 16*(kt*2 + s2) + {4lh .. 4lh+3, 8+4lh .. 8+4lh+3}, which vt_col() puts into the 8 contiguous image
//   columns 16*(kt*2 + s2) + 8lh .. + 8 - the V^T fragment of that k-step and lane half.  O^T register r of dim tile dt holds dim
//   dt*32 + (r & 3) + 8*(r >> 2) + 4*lh of the lane's query.
// STORE TAIL: for dt and the pair of register quads (gq, gq + 1), gq = 0, 2: one v_permlane32_swap per dword exchanges quad gq of lanes
//   32 - 63 with quad gq + 1 of lanes 0 - 31; a lane of half lh then holds the 8 dims dt*32 + (gq + lh)*8 .. + 8 of its query - elements
//   0 .. 3 from register quad gq + lh of the lower half's lane, 4 .. 7 from the same quad of the upper half's - one 16-byte store.
// WAITS (vector-memory operations retire in issue order; a wave's queue): per key block 5 DMA instructions (the block two ahead, issued
//   behind the barrier), 8 for the next item's Q^T (in iteration 0 of an item, behind its S^T phase), 8 stores at the end of an item (none if
//   the wave has no query < T).  fa_wait_allowed() is the number of youngest operations that may stay in flight at the wait in front of
//   barrier (item, kb): block kb must have landed, and at kb 0 the item's Q^T.  It is safe everywhere, and tight (one more would let a needed
//   operation stay in flight) everywhere but twice, where it also waits for 8 operations issued one or two iterations earlier: at kb 1 of a
//   later item for the previous item's stores (issued behind block 1's DMA, not counted), at kb 2 of an item with a successor for the next
//   item's Q^T (issued behind block 2's DMA in iteration 0).  tests/test_attn_tile_host.py replays the queue and asserts exactly this.
// RING: the DMA issued behind barrier p fills the slot of block p - 1 (= block p + 2), which every wave has left; slots and blocks count on
//   across item boundaries.
// FEW IMAGES (attention_small_kernel): workgroup = (b, h, 32-query tile), wave w = key block w.  A wave's LDS area (FS_AREA_BYTES) holds in
//   turn its K block [64 keys][FS_KP halfs], its V^T block [128 dims][FS_VP halfs] and its partial O^T [128 dims][32 queries] floats; behind
//   the 7 areas m and l as [wave][32 queries] floats.  The pads of 8 halfs make the fragment reads conflict free.  Merge: thread
//   tid < 256 = (query tid & 31, dims 16 * (tid >> 5) .. + 16).
#pragma once
#include <stddef.h>
#include "tok_tile.h"

// ---- host part: the index rules ----
// -- geometry --
constexpr int AT_DH = 128;                       // dims per head
constexpr int AT_TP = 416;                       // columns of a V image row
constexpr int AT_MAXT = 400;
static_assert(AT_TP == VT_LD, "the V image of tok_tile.h");
constexpr int FA_WAVES = 7, FA_THREADS = FA_WAVES * 64;
constexpr int FA_QB = FA_WAVES * 32;             // queries per item
constexpr int FA_KB = 64;                        // keys per stage
constexpr int FA_NSTAGE = 3;
constexpr int FA_AHEAD = 2;                      // key blocks the DMA runs ahead
constexpr int FA_STAGE_DMAS = 32, FA_K_DMAS = 16;      // DMA instructions per stage; the first 16 fill the K block
constexpr int FA_DMA_PER_WAVE = 5;               // ceil(32 / 7)
constexpr int FA_STAGE_HALFS = FA_KB * AT_DH * 2;      // K block [64][128] + V^T block [128][64]
constexpr int FA_V_BYTES = FA_KB * AT_DH * 2;    // byte offset of the V^T block in a stage
constexpr int FA_KT_BYTES = 32 * AT_DH * 2, FA_DT_BYTES = 32 * FA_KB * 2;      // a key tile of the K block, a dim tile of the V^T block
constexpr int FA_QW_HALFS = 32 * AT_DH;          // a wave's Q^T area: 8 fragments x 64 lanes x 8 halfs
constexpr int FA_Q_HALFS = FA_NSTAGE * FA_STAGE_HALFS;      // the Q^T areas follow the ring
constexpr int FA_LDS_BYTES = (FA_Q_HALFS + FA_WAVES * FA_QW_HALFS) * 2;
constexpr int fa_nqb(int T) { return (T + FA_QB - 1) / FA_QB; }
constexpr int fa_nkb(int T) { return (T + FA_KB - 1) / FA_KB; }
constexpr int fa_n_items(int B, int T) { return fa_nqb(T) * 4 * B; }
constexpr float AT_C2 = 0.08838834764831845f * 1.4426950408889634f;      // log2(e) / sqrt(128): exp((s - m) / sqrt(128)) = exp2(s * c2 - m * c2)

// -- sources (element indices) --
constexpr size_t qk_row(int b, int T) { return (size_t)b * T * 1024; }                    // first q | k row of hypothesis b
constexpr int qk_q_col(int h) { return h * AT_DH; }
constexpr int qk_k_col(int h) { return 512 + h * AT_DH; }
constexpr size_t vt_head(int b, int h) { return ((size_t)b * 4 + h) * AT_DH * AT_TP; }      // = vt_row(b, h * 128): dim d adds d * AT_TP

// -- items --
struct FaItem {
  int b, h, qb;
};
constexpr FaItem fa_item(int L, int nqb) { return FaItem{L / (nqb * 4), (L / nqb) & 3, L % nqb}; }
constexpr bool fa_walk_has(int v, int n_items) { return v < n_items; }
constexpr int fa_walk_next(int v, int G) { return v + G; }
constexpr int fa_query(int qb, int wave, int lr) { return qb * FA_QB + wave * 32 + lr; }

// -- stage DMA --
constexpr int fa_dma_instr(int wave, int u) { return wave + u * FA_WAVES >= FA_STAGE_DMAS ? wave + u * FA_WAVES - FA_STAGE_DMAS : wave + u * FA_WAVES; }
constexpr bool fa_dma_is_k(int i) { return i < FA_K_DMAS; }
// source byte offset of lane `lane` of instruction i for key block kb = min(kb*64 + sx, limit) * stride + sadd.  K: sx = key in the block,
// limit T - 1, stride 2048; V^T: sx = first image column of the chunk, limit 408, stride 2
struct FaDmaLane {
  unsigned sx, sadd;
};
constexpr FaDmaLane fa_dma_lane(int i, int lane) {
  if (fa_dma_is_k(i)) {
    const int c = i * 64 + lane, kl = c >> 4, chp = c & 15;
    return FaDmaLane{(unsigned)kl, (unsigned)(((chp ^ (kl & 15)) * 8) * 2)};
  }
  const int c = (i - FA_K_DMAS) * 64 + lane, d = c >> 3, chp = c & 7;
  return FaDmaLane{(unsigned)((chp ^ ((d >> 1) & 7)) * 8), (unsigned)(d * AT_TP * 2)};
}
constexpr unsigned FA_V_LAST_CHUNK = 408;
constexpr unsigned fa_dma_x(int kb, FaDmaLane l) { return (unsigned)(kb * FA_KB) + l.sx; }
constexpr unsigned fa_dma_lim(bool is_k, int T) { return is_k ? (unsigned)(T - 1) : FA_V_LAST_CHUNK; }
constexpr unsigned fa_dma_off(bool is_k, unsigned t, FaDmaLane l) { return t * (is_k ? 2048u : 2u) + l.sadd; }      // t = min(x, lim)
constexpr unsigned fa_dma_src(bool is_k, int kb, FaDmaLane l, int T) {
  return fa_dma_off(is_k, fa_dma_x(kb, l) < fa_dma_lim(is_k, T) ? fa_dma_x(kb, l) : fa_dma_lim(is_k, T), l);
}
constexpr int fa_slot(int slot) { return slot * FA_STAGE_HALFS; }                          // halfs: ring slot -> stage
constexpr int fa_dma_lds(int i) { return i * 512; }                                        // halfs within the stage; + 8 * lane.  (Destination = base + fa_slot + fa_dma_lds, two terms)
constexpr int fa_ring_next(int slot) { return slot + 1 == FA_NSTAGE ? 0 : slot + 1; }

// -- fragment reads (byte offsets within a stage) --
constexpr unsigned fa_kfrag(int s, int lr, int lh) { return (lr * AT_DH + (((2 * s + lh) ^ (lr & 15)) * 8)) * 2; }      // k-step s = 0 .. 7 (dims 16s + 8lh ..); key tile kt adds FA_KT_BYTES
constexpr unsigned fa_vfrag(int s, int lr, int lh) { return FA_V_BYTES + (lr * FA_KB + (((2 * s + lh) ^ ((lr >> 1) & 7)) * 8)) * 2; }      // k-step s = 0 .. 3 (16 keys); dim tile dt adds FA_DT_BYTES

// -- Q^T staging --
constexpr unsigned fa_q_row(int wave, int lr) { return wave * 32 + lr; }                   // row of the item's query block
constexpr unsigned fa_q_src(unsigned qrow, int lh, int T, int qb) {                        // byte offset from (first row of the block, Q of the head); instruction s adds 16 s halfs
  return (qrow < (unsigned)(T - 1 - qb * FA_QB) ? qrow : (unsigned)(T - 1 - qb * FA_QB)) * 2048u + lh * 16;
}
constexpr int fa_q_lds(int s) { return s * 512; }                                          // halfs in the wave's area; + 8 * lane, for the DMA and for the fragment read

// -- accumulator maps --
constexpr int fa_s_key(int kt, int r, int lh) { return acc_vt_token(kt, r, lh); }          // key (in the block) of S^T register r of key tile kt
constexpr int fa_p_kstep(int kt, int s2) { return kt * 2 + s2; }                           // the k-step whose P^T operand is ...
constexpr int fa_p_reg(int s2, int j) { return 8 * s2 + j; }                               // ... registers fa_p_reg(s2, 0 .. 7) of tile kt
constexpr int fa_o_dim(int dt, int r, int lh) { return acc_vt_token(dt, r, lh); }          // dim of O^T register r of dim tile dt
// store tail: the lane of half lh stores dims fa_st_dim(dt, gq, lh) .. + 8 (gq = 0, 2); element e comes from register fa_st_reg(gq, lh, e) of
// the lane of half fa_st_half(e) with the same query.  fa_st_dim is linear in (dt, gq, lh).
constexpr int fa_st_dim(int dt, int gq, int lh) { return dt * 32 + gq * 8 + lh * 8; }
constexpr int fa_st_reg(int gq, int lh, int e) { return (gq + lh) * 4 + (e & 3); }
constexpr int fa_st_half(int e) { return e >> 2; }

// -- wait rule --
constexpr int FA_VM_BLOCK = FA_DMA_PER_WAVE, FA_VM_QT = 8, FA_VM_STORES = 8;
constexpr int fa_store_count(bool wave_valid) { return wave_valid ? FA_VM_STORES : 0; }
// inflight: key blocks staged and not consumed yet, this one included; st_prev: fa_store_count of the previous item
constexpr int fa_wait_allowed(int kb, int nkb, bool first, bool has_next, int inflight, int st_prev) {
  int allowed = inflight > 1 ? FA_VM_BLOCK : 0;                  // the next block
  if (kb == 0) allowed = first ? 0 : (nkb == 1 ? st_prev : allowed + st_prev);      // the first item's Q^T is the youngest operation: drain
  else if (kb == 1 && has_next) allowed += FA_VM_QT;             // the next item's Q^T, issued in iteration 0 behind the block two ahead
  return allowed;
}
constexpr int FA_WAIT_SET[] = {0, FA_VM_BLOCK, FA_VM_STORES, FA_VM_BLOCK + FA_VM_STORES};      // every value the rule takes: the waits the kernel instantiates
static_assert(FA_VM_QT == FA_VM_STORES, "FA_WAIT_SET lists 8 once");

// -- few-image kernel --
constexpr int FS_WAVES = 7;
constexpr int FS_KP = 136;                       // halfs per key row of a wave's K block (128 dims + 8)
constexpr int FS_VP = 72;                        // halfs per dim row of its V^T block (64 keys + 8)
constexpr int FS_AREA_BYTES = AT_DH * FS_VP * 2;
constexpr int FS_ML_BYTES = FS_WAVES * FS_AREA_BYTES;      // m [wave][32], then l [wave][32]
constexpr int FS_LDS_BYTES = FS_ML_BYTES + 2 * FS_WAVES * 32 * 4;
static_assert(64 * FS_KP * 2 <= FS_AREA_BYTES && AT_DH * 32 * 4 <= FS_AREA_BYTES, "attention_small: wave area");
constexpr int fs_nqt(int T) { return (T + 31) >> 5; }
constexpr int fs_ld(int lane, int u) { return lane + 64 * u; }                             // 16-byte load u (0 .. 15) of a lane: K: key i >> 4, chunk i & 15; V^T: dim i >> 3, chunk i & 7
constexpr int fs_k_off(int key, int dim) { return key * FS_KP + dim; }                     // halfs in the area
constexpr int fs_v_off(int dim, int col) { return dim * FS_VP + col; }
constexpr int fs_o_off(int dim, int q) { return dim * 32 + q; }                            // floats in the area
constexpr int fs_ml_off(int w, int q) { return w * 32 + q; }
constexpr int fs_merge_q(int tid) { return tid & 31; }
constexpr int fs_merge_dim(int tid) { return (tid >> 5) * 16; }                            // .. + 16; threads 0 .. 255

#ifdef __HIPCC__
#include "device_util.h"

// ---- device part: pieces the kernels share or that read better named ----
// key tail: scores of keys >= T become -1e30 - out of the maximum, exp2 -> exactly 0.  key0 = first key of the block.  (attention_small_kernel
// keeps the same loop written out: through this function it takes one SGPR less)
__device__ __forceinline__ void at_mask_tail(floatx16 (&sacc)[2], int key0, int lh, int T) {
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = key0 + fa_s_key(kt, r, lh);
      sacc[kt][r] = key < T ? sacc[kt][r] : -1.0e30f;
    }
}
// the P^T operand of k-step (kt, s2) from the S^T accumulator of key tile kt
__device__ __forceinline__ half8 at_p_frag(const floatx16 &s, int s2) {
  half8 pf;
#pragma unroll
  for (int j = 0; j < 8; ++j) pf[j] = (f16)s[fa_p_reg(s2, j)];
  return pf;
}
#endif
