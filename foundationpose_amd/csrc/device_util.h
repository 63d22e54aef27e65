// Device-side primitives shared by the gfx950 kernel files: LDS-DMA, counted waits, lane and workgroup reductions and the bias start of
// the MFMA accumulators (token GEMMs and the band convolutions; the families' own pieces are in tok_tile.h and conv_band.h).  Device
// only; include after common.h.  Everything is __forceinline__: a kernel that uses a helper from here compiles to the instructions it
// had with a private copy.
#pragma once
#include "common.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));   // 16-byte register value (plain vector loads / stores in IR)

// ---- LDS-DMA: 16 bytes per lane, global memory -> LDS without passing through registers ----
// Issued from inline asm.  Through __builtin_amdgcn_global_load_lds the compiler marks a "flat access that may touch LDS" as
// pending until the next full drain, and while that mark is up EVERY wait it inserts for an LDS fragment read is
// s_waitcnt lgkmcnt(0) (and every barrier drains vmcnt(0)) - no LDS read can stay in flight under the MFMAs.  Hidden in asm,
// the DMA is outside its bookkeeping: fragment reads get counted lgkmcnt(n), and the DMA's completion is waited for by the
// caller with a counted wait_vm<N>() / wait_vm_lgkm<N>() in front of the barrier that publishes the data (loads, stores and
// LDS-DMA retire in issue order).  m0 = wave-uniform LDS byte address; lane i lands at + 16 i (the destination of an LDS-DMA is
// always lane-linear: a swizzle goes on the source address).
// The destination is an LDS BYTE address or an f16 * into LDS.  A kernel that issues many DMAs casts its LDS array to address
// space 3 once and passes byte addresses: a generic -> LDS cast per call makes hipcc emit a null check against src_shared_base
// per DMA.
__device__ __forceinline__ unsigned lds_addr(const void *l) { return (unsigned)(size_t)(__attribute__((address_space(3))) void *)l; }

// scalar base + 32-bit lane byte offset: no per-lane 64-bit address arithmetic in front of the DMA
__device__ __forceinline__ void glds16(const f16 *sbase, unsigned voff_bytes, unsigned lds_byte) {
  lds_byte = __builtin_amdgcn_readfirstlane(lds_byte);
  asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff_bytes), "s"(sbase), "s"(lds_byte) : "memory");
}
__device__ __forceinline__ void glds16(const f16 *sbase, unsigned voff_bytes, f16 *l) { glds16(sbase, voff_bytes, lds_addr(l)); }
// one 64-bit source address per lane (gathers; out-of-image taps point at a zero page)
__device__ __forceinline__ void glds16(const void *g, unsigned lds_byte) {
  lds_byte = __builtin_amdgcn_readfirstlane(lds_byte);
  asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(lds_byte) : "memory");
}
__device__ __forceinline__ void glds16(const void *g, f16 *l) { glds16(g, lds_addr(l)); }

// ---- counted waits: at most N vector-memory operations (loads, stores, LDS-DMA) of this wave still in flight ----
// wait_vm_lgkm also drains the LDS / scalar-memory counter: the form in front of a raw s_barrier of a DMA ring.
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm_lgkm() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}
// the wave's own LDS operations have completed (same-wave LDS operations are in order); vector-memory operations stay in flight
__device__ __forceinline__ void wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// ---- lane reductions ----
// sum over the 16 lanes of a DPP row (lanes 16r .. 16r+15), result in every lane; fixed order.  quad_perm [1,0,3,2] and
// [2,3,0,1] add within quads, row_half_mirror / row_mirror exchange quads whose four lanes already hold equal sums.
__device__ __forceinline__ float row16_sum(float x) {
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xf, 0xf, false));
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xf, 0xf, false));
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xf, 0xf, false));
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xf, 0xf, false));
  return x;
}

// butterfly over the 64 lanes of a wave, partner distance 32, 16, .. 1; the result is in every lane.  The order is part of the
// documented bit-exact results of the kernels that use it: do not change it.
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, [](T a, T b) { return a + b; }); }
__device__ __forceinline__ int wave_min(int v) { return wave_reduce(v, [](int a, int b) { return min(a, b); }); }
__device__ __forceinline__ int wave_max(int v) { return wave_reduce(v, [](int a, int b) { return max(a, b); }); }
__device__ __forceinline__ float wave_max(float v) { return wave_reduce(v, [](float a, float b) { return fmaxf(a, b); }); }
__device__ __forceinline__ double wave_max(double v) { return wave_reduce(v, [](double a, double b) { return fmax(a, b); }); }

// cnt[r] += 1 for every lane with `on`; called by all lanes of a wave together.  Integer adds: the grouping does not change the sum.
// The counts of ONE component would be an add per lane to one address; a wave whose active lanes all name the same r adds their number
// once instead.
__device__ __forceinline__ void wave_add_one(int *cnt, int r, bool on) {
  const unsigned long long act = __ballot(on);
  if (act == 0) return;
  const int first = __ffsll((long long)act) - 1;
  const int lead = __shfl(r, first, 64);
  const unsigned long long same = __ballot(on && r == lead);
  if (same == act) {
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&cnt[lead], __popcll(act));
  } else if (on) {
    atomicAdd(&cnt[r], 1);
  }
}

// sum over a workgroup of THREADS threads in a fixed order (the butterfly within each wave, then the waves in order), valid in thread 0.
// `red` holds THREADS / 64 doubles of LDS; the first barrier lets the previous sum's `red` be read before it is written again.  The
// butterfly is wave_sum written out: through the call hipcc orders the instructions of pose_errors_kernel (metrics.hip) differently.
template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < THREADS / 64; ++i) s += red[i];
  return s;
}

// ---- bias start of the MFMA accumulators (token GEMMs: tok_tile.h has their other pieces; band convolutions) ----
// Accumulators of a token GEMM or a convolution start at the bias.  col0 is the first of the wave's NI * 32 output columns; acc[i][j] is the
// 32x32 MFMA tile of columns col0 + i*32 .. +31 and tokens (pixels) j*32 .. +31; lr = lane & 31, lh = lane >> 5.
// Row layout: a lane owns one token and channels col0 + i*32 + rg*8 + lh*4 + (0..3) in register quad rg.
template <int NI>
__device__ __forceinline__ void bias_quads(float4 (&bq)[NI][4], const float *bias, int col0, int lh) {
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) bq[i][rg] = *reinterpret_cast<const float4 *>(bias + col0 + i * 32 + rg * 8 + lh * 4);
}
// ... from bias quads already in registers (the persistent kernels of stem.hip and front.hip hold them across their tile loops)
template <int NI, int NJ>
__device__ __forceinline__ void acc_from_bias(floatx16 (&acc)[NI][NJ], const float4 (&bq)[NI][4]) {
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        acc[i][j][rg * 4 + 0] = bq[i][rg].x;
        acc[i][j][rg * 4 + 1] = bq[i][rg].y;
        acc[i][j][rg * 4 + 2] = bq[i][rg].z;
        acc[i][j][rg * 4 + 3] = bq[i][rg].w;
      }
}
template <int NI, int NJ>
__device__ __forceinline__ void acc_from_bias(floatx16 (&acc)[NI][NJ], const float *bias, int col0, int lh) {
  float4 bq[NI][4];
  bias_quads(bq, bias, col0, lh);
  acc_from_bias(acc, bq);
}
// Swapped operands (the transposed V image): a lane owns ONE channel col0 + i*32 + lr and 4 consecutive tokens per register quad.
template <int NI, int NJ>
__device__ __forceinline__ void acc_from_bias_vt(floatx16 (&acc)[NI][NJ], const float *bias, int col0, int lr) {
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const float b = bias[col0 + i * 32 + lr];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = b;
  }
}
