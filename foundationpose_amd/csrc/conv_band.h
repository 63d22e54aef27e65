// The band family of convolution kernels (conv_s2.hip, conv_s1b.hip, stem.hip, front.hip): each index rule of their LDS layouts once, and the
// device pieces they share - swizzled band read, band DMA map, weight-fragment ring, K loop, per-wave staged epilogue.
// The host part is plain C++17 and compiles without HIP (tests/test_conv_band_host.py checks it over the kernels' geometries); the device
// part is __forceinline__.  A kernel whose registers or waits hipcc changed through a piece keeps that piece written out and says so.
//
// BAND (3x3 kernels): the input rows an output tile needs, 16 channels deep, as pixel SLOTS of 32 bytes; a band row is P slots.  The two
// 16-byte halves of slot q are swapped when bit 3 of q is set, so with 2P = W_out (mod 16) (stride 2) or P = W (mod 16) (stride 1) every
// 16-lane group of a ds_read_b128 covers all 64 banks once, also across the row breaks of a 32-pixel tile - but not across the break between
// two images inside a stride-2 tile, where the zero row shifts the second image's rows by P slots: that lane group is not conflict free.
//   stride 2: a row is two column-parity planes, even input columns 0, 2, .. in slots 0 .. WO - 1, odd ones -1, 1, .. in slots WO .. 2 WO:
//             the taps of consecutive output pixels are consecutive slots;
//   stride 1: slot c holds input column c - 1.
// REGION (7x7 stem): 16-byte slots (one pixel of 8 channels = one tap's k-slice), a region row is `pitch` slots: even region columns from
// slot 0, odd ones from slot `odd`.  K-step s multiplies tap 2s in the lower lane half and tap 2s + 1 in the upper (tap 49: zero weights).
#pragma once
#include <stddef.h>

// ---- host part: the index rules ----
constexpr int band_addr(int slot, int half) { return (slot << 5) | (half << 4); }         // byte address of a logical half, before the swizzle
constexpr int band_swizzle(int x) { return x ^ ((x >> 4) & 16); }                        // bit 8 of the address = bit 3 of the slot
constexpr int s2_col_slot(int WO, int ix) { return (ix & 1) ? WO + ((ix + 1) >> 1) : ix >> 1; }      // input column -1 .. 2 WO - 1 -> slot of its row
constexpr int s2_slot_col(int WO, int c) { return c < WO ? 2 * c : 2 * (c - WO) - 1; }
constexpr int s1_col_slot(int ix) { return ix + 1; }
constexpr int s1_slot_col(int c) { return c - 1; }
// slot of tap (ky, kx) of an output pixel relative to the pixel's base slot (band row of its tap row 0, slot ox)
constexpr int s2_tap_slots(int P, int WO, int ky, int kx) { return ky * P + s2_col_slot(WO, kx - 1); }      // {WO, 0, WO + 1}[kx]
constexpr int s1_tap_slots(int P, int ky, int kx) { return ky * P + s1_col_slot(kx - 1); }
// stride 2, tiles flattened over images: local output row jr of a tile whose local rows >= jb belong to the next image (a zero row
// between the two) -> band row of its tap row 0
constexpr int s2_tile_row(int jr, int jb) { return 2 * jr + (jr >= jb ? 1 : 0); }

struct BandSrc {          // the input pixel a band slot holds
  int img, iy, ix;        // image relative to the tile's first
  bool ok;                // false: outside the image or past the band -> zero page
};
// band row b <= 2 jb: input row 2 oy0 + b - 1 of the first image; b > 2 jb: row b - 2 jb - 2 of the next one (-1: the zero row), if there is
// one (n_img: images from the tile's first on)
constexpr BandSrc s2_band_src(int P, int WO, int brows, int oy0, int jb, int n_img, int q) {
  const int b = q / P, c = q - b * P, ix = s2_slot_col(WO, c);
  const bool second = b > 2 * jb;
  const int img = second ? 1 : 0, iy = second ? b - 2 * jb - 2 : 2 * oy0 + b - 1;
  return {img, iy, ix, b < brows && iy >= 0 && iy < 2 * WO && ix >= 0 && ix < 2 * WO && img < n_img};
}
// q: slot of one 16-channel plane; band row b holds input row oy0 - 1 + b of a W x W map
constexpr BandSrc s1_band_src(int P, int W, int brows, int oy0, int q) {
  const int b = q / P, c = q - b * P, iy = oy0 - 1 + b, ix = s1_slot_col(c);
  return {0, iy, ix, b < brows && iy >= 0 && iy < W && ix >= 0 && ix < W};
}
// 1-KB DMA instruction u, lane l -> slot 32 u + l / 2, physical half l & 1 (an LDS-DMA destination is lane-linear: the swizzle goes on the source)
constexpr int band_dma_slot(int u, int lane) { return 32 * u + (lane >> 1); }
constexpr int band_dma_half(int q, int lane) { return (band_swizzle(band_addr(q, lane & 1)) >> 4) & 1; }      // the logical half that lands there

constexpr int stem_col_slot(int odd, int j) { return (j & 1) * odd + (j >> 1); }         // region column -> slot of its row
constexpr int stem_slot_col(int odd, int q) { return q < odd ? 2 * q : 2 * (q - odd) + 1; }
constexpr int stem_pixel_slot(int pitch, int row, int col) { return 2 * row * pitch + col; }      // output pixel of the block / tile -> slot of its tap (0, 0)
constexpr int stem_tap_slots(int pitch, int odd, int t) {                                // tap t = ky * 7 + kx -> slots from the pixel's slot
  const int ky = t / 7, kx = t - ky * 7;
  return ky * pitch + stem_col_slot(odd, kx);
}
constexpr int stem_step_tap(int s, int lh) { return 2 * s + lh < 48 ? 2 * s + lh : 48; }  // tap 49 has zero weights: any slot inside the region
// weight fragment (cout tile i, k-step s), lane (lr, lh) = W[i*32 + lr][(2s + lh)*8 .. +8] of the [64][Kpad] image: index of its first element
constexpr size_t stem_frag_src(int Kpad, int i, int s, int lane) { return (size_t)(i * 32 + (lane & 31)) * Kpad + (2 * s + (lane >> 5)) * 8; }

#ifdef __HIPCC__
#include "device_util.h"

// ---- swizzled band read: the B fragment (16 channels of one pixel per lane pair) of one tap.  qb = band_addr(base slot, lh) ----
__device__ __forceinline__ half8 band_read(const unsigned char *plane, int qb, int tap_slots) {
  int x = qb;
  asm volatile("" : "+v"(x));                               // keep the tap addresses out of registers: three VALU ops per read instead
  x += tap_slots << 5;
  return *reinterpret_cast<const half8 *>(plane + band_swizzle(x));
}
template <int P, int WO>
__device__ __forceinline__ half8 band_read_s2(const unsigned char *plane, int qb, int tap) {
  return band_read(plane, qb, s2_tap_slots(P, WO, tap / 3, tap % 3));
}
template <int P>
__device__ __forceinline__ half8 band_read_s1(const unsigned char *plane, int qb, int tap) {
  return band_read(plane, qb, s1_tap_slots(P, tap / 3, tap % 3));
}

// ---- band DMA of a 4-wave workgroup: wave w issues instructions w, w + 4, ..; src_of(slot, logical half) = byte offset of that half in the
// input at chunk 0, or BAND_ZERO: the zero page ----
constexpr unsigned BAND_ZERO = 0xffffffffu;
template <int DPW, typename SrcOf>
__device__ __forceinline__ void band_dma_offsets(unsigned (&src_off)[DPW], int wave, int lane, SrcOf src_of) {
#pragma unroll
  for (int v = 0; v < DPW; ++v) {
    const int q = band_dma_slot(wave + 4 * v, lane);
    src_off[v] = src_of(q, band_dma_half(q, lane));
  }
}

// ---- weight fragments: a wave's stream of 1-KB fragments L2 -> registers, groups of CT in order, three groups ahead (past the end: the
// padding of the packed image) ----
template <int CT>
struct WeightRing {
  const half8 *wp;                                          // first fragment + lane
  half8 aq[3][CT];
  int f = 0;                                                // next group to fetch
  __device__ __forceinline__ void fetch(int slot) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) aq[slot][ct] = wp[(size_t)(f * CT + ct) * 64];
    ++f;
  }
};

// ---- K loop: per chunk STEPS steps of NPT x CT MFMAs; dma(chunk, buffer) fills a band buffer, read(buffer, step, pixel tile) is a B
// fragment.  The B fragment of (step + 1, tile j) is read right behind the MFMAs of (step, tile j): its register is free once they have
// issued, and the MFMAs of the other tiles hide its latency.  Only step 0 of a chunk waits for its reads (the band is new). ----
template <int STEPS, int CT, int NPT, typename Dma, typename Read>
__device__ __forceinline__ void band_k_loop(floatx16 (&acc)[CT][NPT], WeightRing<CT> &ring, int nchunks, Dma dma, Read read) {
  for (int ch = 0; ch < nchunks; ++ch) {
    // this wave's part of chunk ch has landed (everything this wave has in flight: the three prefetched weight groups are needed next
    // anyway); after the barrier every wave's part has, and every wave is done reading the other buffer (chunk ch - 1)
    wait_vm_lgkm<0>();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (ch + 1 < nchunks) dma(ch + 1, (ch + 1) & 1);
    half8 b[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) b[j] = read(ch & 1, 0, j);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
#pragma unroll
      for (int j = 0; j < NPT; ++j) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[ct][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ring.aq[st % 3][ct], b[j], acc[ct][j], 0, 0, 0);
        if (st + 1 < STEPS) b[j] = read(ch & 1, st + 1, j);
        __builtin_amdgcn_sched_barrier(0);
      }
      ring.fetch(st % 3);                                   // step st + 3, possibly of the next chunk
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  wait_vm_lgkm<0>();                                        // the trailing weight prefetches
  __builtin_amdgcn_s_barrier();                             // every wave is done with the bands: staging may overwrite them
  __builtin_amdgcn_sched_barrier(0);
}

// ---- per-wave staged epilogue of pixel tile j: accumulator quads -> convert -> the wave's 32 staging rows of LD halfs; read back as 16-byte
// row pieces, CT * 4 lanes per pixel; dest(pixel of the tile, 16-byte column) = where the piece goes in NHWC, or skip.
// convert(quad, sp) sees the staging address the quad goes to (conv_s1b.hip stages the residual there first).  lr = lane & 31, lh = lane >> 5
// are the caller's values: derived here again they change the callers' register allocation. ----
struct BandDst {
  f16 *p;
  bool store = true;
};
template <bool RES = false>
struct ReluThenRound {                                      // (f16)max(v, lo) as stem7x7_kernel; RES: the staged residual added in fp32 first
  float lo;
  __device__ __forceinline__ half4 operator()(const float (&v)[4], const f16 *sp) const {
    float s[4] = {v[0], v[1], v[2], v[3]};
    if constexpr (RES) {
      const half4 rq = *reinterpret_cast<const half4 *>(sp);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += (float)rq[e];
    }
    return half4{(f16)fmaxf(s[0], lo), (f16)fmaxf(s[1], lo), (f16)fmaxf(s[2], lo), (f16)fmaxf(s[3], lo)};
  }
};
struct RoundThenRelu {                                      // max((f16)v, 0): conv_igemm2_kernel
  __device__ __forceinline__ half4 operator()(const float (&v)[4], const f16 *) const {
    const half4 hv{(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
    return __builtin_elementwise_max(hv, half4{(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f});
  }
};
template <int LD, int CT, int NJ, typename Convert, typename Dest>
__device__ __forceinline__ void band_store_tile(f16 *stage, const floatx16 (&acc)[CT][NJ], int j, int lane, int lr, int lh, Convert convert, Dest dest) {
  constexpr int LPP = CT * 4, PPI = 64 / LPP;               // lanes per pixel row (16 bytes each), pixels per store instruction
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      f16 *sp = &stage[lr * LD + ct * 32 + rg * 8 + lh * 4];
      const float v[4] = {acc[ct][j][rg * 4 + 0], acc[ct][j][rg * 4 + 1], acc[ct][j][rg * 4 + 2], acc[ct][j][rg * 4 + 3]};
      *reinterpret_cast<half4 *>(sp) = convert(v, sp);
    }
  wait_lgkm();                                              // the wave's own staging writes have landed (same-wave LDS operations are in order)
  uint4 v[32 / PPI];
#pragma unroll
  for (int u = 0; u < 32 / PPI; ++u) v[u] = *reinterpret_cast<const uint4 *>(&stage[(u * PPI + lane / LPP) * LD + (lane % LPP) * 8]);
#pragma unroll
  for (int u = 0; u < 32 / PPI; ++u) {
    const BandDst d = dest(u * PPI + lane / LPP, lane % LPP);
    if (d.store) *reinterpret_cast<uint4 *>(d.p) = v[u];
  }
  wait_lgkm();                                              // staging read back before the next tile overwrites it
}
#endif
