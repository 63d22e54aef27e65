// The attention core of the transformer heads for gfx950: multi-head self-attention over up to 400 tokens (4 heads x 128) on
// v_mfma_f32_32x32x16_f16 - attention_kernel, persistent and flash-style, for the batches; attention_small_kernel, split-K, for the one
// or two hypotheses of a tracking frame - and their launch function.  Every layout, DMA slot and wait count is stated in attn_tile.h
// (checked on the CPU by tests/test_attn_tile_host.py); this file keeps the control flow and the arithmetic.
//
// Reference: nn.TransformerEncoderLayer / nn.MultiheadAttention as used by learning/models/refine_network.py:56-70 and
// score_network.py:53-54,73-88.
#include "attn_tile.h"
#include "common.h"
#include "device_util.h"

// Flash-style multi-head self-attention core.  A work item = one (hypothesis, head, 224-query block): 13 query tiles of 32 split 7 + 6 over
// two items; each of the 7 waves owns 32 queries and keeps Q^T (32 regs), the running max / sum and O^T (4 x 32x32 accumulators) in
// registers.  Keys stream through LDS in blocks of 64 (K block + V^T block = 32 KB) in a 3-deep ring filled by LDS-DMA TWO blocks ahead:
// counted s_waitcnt vmcnt(N) + raw s_barrier keep the later blocks in flight across the barrier (a __syncthreads() would drain them).
// PERSISTENT workgroups (one per CU, 152 KB LDS): workgroup j walks the items j, j + grid, j + 2 grid, ... and the DMA ring does not stop
// at an item boundary - the last two iterations of item i stage the first two key blocks of item i + 1, and the Q^T fragments of item
// i + 1 come by LDS-DMA into a per-wave 8-KB area right after the first S^T phase of item i has consumed its own.  As one item per
// workgroup a workgroup spent 17 k of its 47 k cycles on a start-up nothing covered (stamps: Q 7.5 k, DMA issue 2.9 k, block-0 wait 6.8 k).
//   S^T = K Q^T       : A = K rows from LDS, B = Q^T in registers; the lane that owns query column q sees 16 of each 32 keys, its
//                       partner lane + 32 the rest.
//   online softmax     : per key block, max / sum finish with one xor-32 shuffle; exp((s-m)/sqrt(128)).
//   O^T += V^T P^T     : the S^T accumulator registers ARE the B operand (attn_tile.h, ACCUMULATORS); O^T keeps the query on the lane,
//                       so the rescale is lane-local.
// The loop is bound by vector-instruction ISSUE, not by the matrix pipe (SQ counters: 643 vector instructions per wave per
// key block beside 32 MFMAs, two waves sharing one SIMD's issue port), so the body is written to issue few of them:
// exp2 with the scale folded into one packed fma per two scores, v_max3, packed adds, tail masking only in the last key
// block, O^T rescaled only when some lane's running max moved, LDS fragment offsets and DMA gather offsets precomputed
// per lane (the DMA of a slot is scalar base + min(key, limit) * stride + lane constant - no branches in the loop).
// (Measured and dropped: waves 4-6 running the PV product of block k - 1 at the start of iteration k: the same time.)
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <bool V> struct FaBool { static constexpr bool value = V; };

#ifdef HALO_STAMP
// diagnostic build only (make -B EXTRA=-DHALO_STAMP): per-wave s_memtime stamps of the attention kernel, first 1024 workgroups:
// [0] entry, [31] exit; of the workgroup's SECOND item (its first when it has only one): [1] item start, then per key block
// {barrier passed, S done, softmax done, PV done}, [2] stores issued
__device__ unsigned long long g_attn_stamps[1024 * 7 * 32];
extern "C" __attribute__((visibility("default"))) int fp_dbg_attn_stamps(unsigned long long *host) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_attn_stamps), sizeof(g_attn_stamps)) == hipSuccess ? 0 : -1;
}
#define ASTAMP(i) do { if (blockIdx.x < 1024 && stamp_on) st[(i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define ASTAMP(i) do { } while (0)
#endif

// fmaxf() canonicalises each MFMA output first (one extra v_max per score); v_max3 from asm does not.  The hazard
// recognizer does not look inside asm: an asm instruction must never be the FIRST reader of an MFMA result (the required
// wait states would be missing and it would read a half-written accumulator) - the callers chain every fa_max3 behind a
// compiler-visible instruction that reads the same accumulators (operand `a`).
__device__ __forceinline__ float fa_max3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

__global__ __launch_bounds__(FA_THREADS, 2) void attention_kernel(const f16 *__restrict__ qk, const f16 *__restrict__ vt, int T,
                                                                  f16 *__restrict__ out, int n_items) {
  extern __shared__ __attribute__((aligned(16))) f16 smem[];
  const int nqb = fa_nqb(T);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  const int nkb = fa_nkb(T);
  const int G = gridDim.x;
  f16 *qlds = smem + FA_Q_HALFS + wave * FA_QW_HALFS;
#ifdef HALO_STAMP
  unsigned long long st[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) st[i] = 0;
  bool stamp_on = true;
#endif
  ASTAMP(0);

  // item v (virtual workgroup id: v & 7 = the XCD of this workgroup, the query blocks of one (hypothesis, head) share an XCD L2)
  auto item_of = [&](int v) __attribute__((always_inline)) { return fa_item(xcd_remap(v, n_items), nqb); };

  // the wave's DMA instructions of a stage and their per-lane source constants (attn_tile.h, STAGE)
  FaDmaLane dl[FA_DMA_PER_WAVE];
#pragma unroll
  for (int u = 0; u < FA_DMA_PER_WAVE; ++u) dl[u] = fa_dma_lane(fa_dma_instr(wave, u), lane);
  // staging cursor: the next key block the DMA brings in - (item s_v, block s_kb) into ring slot s_slot
  int s_v = blockIdx.x, s_kb = 0, s_slot = 0;
  const f16 *s_kbase, *s_vsrc;
  auto stage_bases = [&]() __attribute__((always_inline)) {
    const FaItem it = item_of(s_v);
    s_kbase = qk + qk_row(it.b, T) + qk_k_col(it.h);                    // K row `key` starts at kbase + key*1024
    s_vsrc = vt + vt_head(it.b, it.h);
  };
  stage_bases();
  auto stage_next = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < FA_DMA_PER_WAVE; ++u) {              // exactly FA_DMA_PER_WAVE per wave (vmcnt accounting)
      const int i = fa_dma_instr(wave, u);
      const bool is_k = fa_dma_is_k(i);                      // wave-uniform
      // fa_dma_src, its limit written out: through fa_dma_lim hipcc lays the key loop out differently (one wait fewer: not the parent's code)
      const unsigned voff = fa_dma_off(is_k, min(fa_dma_x(s_kb, dl[u]), is_k ? (unsigned)(T - 1) : FA_V_LAST_CHUNK), dl[u]);
      glds16(is_k ? s_kbase : s_vsrc, voff, smem + fa_slot(s_slot) + fa_dma_lds(i));
    }
    s_slot = fa_ring_next(s_slot);
    if (++s_kb == nkb) {
      s_kb = 0;
      s_v = fa_walk_next(s_v, G);
      if (fa_walk_has(s_v, n_items)) stage_bases();
    }
  };
  // Q^T of item v -> this wave's staging area, in fragment order (attn_tile.h, Q^T); query rows past T repeat row T - 1 (finite operands;
  // their columns are never stored)
  const unsigned qrow = fa_q_row(wave, lr);
  auto stage_q = [&](int v) __attribute__((always_inline)) {
    const FaItem it = item_of(v);
    const f16 *qbase = qk + ((size_t)it.b * T + it.qb * FA_QB) * 1024 + qk_q_col(it.h);
    const unsigned voff = fa_q_src(qrow, lh, T, it.qb);
#pragma unroll
    for (int s = 0; s < 8; ++s) glds16(qbase + s * 16, voff, qlds + fa_q_lds(s));
  };

  // LDS fragment offsets (bytes, within a stage)
  unsigned koffb[8], voffb[4];
#pragma unroll
  for (int s = 0; s < 8; ++s) koffb[s] = fa_kfrag(s, lr, lh);
#pragma unroll
  for (int s = 0; s < 4; ++s) voffb[s] = fa_vfrag(s, lr, lh);

  const float c2 = AT_C2;
  const f32x2 c2v = {c2, c2};

  // Prologue of the workgroup (the only start-up nothing covers): two key blocks, then Q^T of the first item.
  int inflight = 0;                                            // key blocks staged and not consumed yet (the current one included)
#pragma unroll
  for (int p = 0; p < FA_AHEAD; ++p)
    if (fa_walk_has(s_v, n_items)) {
      stage_next();
      ++inflight;
    }
  stage_q((int)blockIdx.x);

  half8 qf[8];
  floatx16 oacc[4];
  float m_run, l_run;
  int c_slot = 0;                                              // ring slot of the block being consumed
  int st_prev = 0;                                             // stores this wave issued at the end of the previous item
  bool first = true;

  for (int v = blockIdx.x; fa_walk_has(v, n_items); v = fa_walk_next(v, G)) {
    const FaItem it = item_of(v);
    const size_t rowbase = (size_t)it.b * T;
    const int q = fa_query(it.qb, wave, lr);
    const bool wave_valid = fa_query(it.qb, wave, 0) < T;      // wave-uniform: some query of this wave exists
    const bool has_next = fa_walk_has(fa_walk_next(v, G), n_items);
#ifdef HALO_STAMP
    stamp_on = v == (int)blockIdx.x + G || n_items <= G;
#endif
    ASTAMP(1);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) oacc[dt][e] = 0.f;
    m_run = -1.0e30f;
    l_run = 0.f;

    auto body = [&](const int kb, auto first_c, auto tail_c) __attribute__((always_inline)) {
      constexpr bool KB0 = decltype(first_c)::value;           // kb == 0: this item's Q^T comes out of LDS, the next item's goes in
      constexpr bool TAIL = decltype(tail_c)::value;           // this block may hold keys >= T
      // Block (v, kb) must have landed - and in iteration 0 this item's Q^T (attn_tile.h, WAITS); the ladder is over FA_WAIT_SET
      const int allowed = fa_wait_allowed(KB0 ? 0 : kb, nkb, first, has_next, inflight, st_prev);
      if (allowed == FA_WAIT_SET[0]) wait_vm_lgkm<FA_WAIT_SET[0]>();
      else if (allowed == FA_WAIT_SET[1]) wait_vm_lgkm<FA_WAIT_SET[1]>();
      else if (allowed == FA_WAIT_SET[2]) wait_vm_lgkm<FA_WAIT_SET[2]>();
      else wait_vm_lgkm<FA_WAIT_SET[3]>();
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      ASTAMP(3 + 4 * kb);
      // ring slot of block p - 1: every wave is past it
      if (fa_walk_has(s_v, n_items)) {
        stage_next();
        ++inflight;
      }
      if constexpr (KB0) {
#pragma unroll
        for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const half8 *>(qlds + fa_q_lds(s) + lane * 8);
      }
      const char *sb = reinterpret_cast<const char *>(smem + fa_slot(c_slot));
      floatx16 sacc[2];
      // two independent accumulation chains (key tiles 0/1), fragments fetched four k-steps at a time so that
      // eight LDS reads are in flight before the first MFMA of the group issues
#pragma unroll
      for (int sh = 0; sh < 2; ++sh) {
        half8 kf[2][4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) kf[kt][s] = *reinterpret_cast<const half8 *>(sb + koffb[sh * 4 + s] + kt * FA_KT_BYTES);
        __builtin_amdgcn_sched_barrier(0);                     // all eight reads issue before the first MFMA waits for one
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            if (sh == 0 && s == 0) {
              const floatx16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
              sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[kt][s], qf[0], zero, 0, 0, 0);
            } else {
              sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[kt][s], qf[sh * 4 + s], sacc[kt], 0, 0, 0);
            }
          }
      }
      __builtin_amdgcn_sched_barrier(0);
      ASTAMP(4 + 4 * kb);
      // the S^T MFMAs have consumed all eight Q^T fragments (their ds_reads are complete): the staging area is free for the next item's
      if constexpr (KB0) {
        if (has_next) stage_q(fa_walk_next(v, G));
      }
      // ---- online softmax for query column lr ----
      if constexpr (TAIL) at_mask_tail(sacc, kb * FA_KB, lh, T);
      float bm = fmaxf(sacc[0][15], sacc[1][15]);              // compiler-visible first reader of both accumulators
      bm = fa_max3(bm, sacc[0][0], sacc[1][0]);
#pragma unroll
      for (int r = 1; r < 15; r += 2) bm = fa_max3(bm, sacc[0][r], sacc[0][r + 1]);
#pragma unroll
      for (int r = 1; r < 15; r += 2) bm = fa_max3(bm, sacc[1][r], sacc[1][r + 1]);
      bm = fmaxf(bm, __shfl_xor(bm, 32));
      const float m_new = fmaxf(m_run, bm);
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c2);
      const float nmc = -m_new * c2;
      const f32x2 nmcv = {nmc, nmc};
      f32x2 ps2 = {0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const f32x2 sv = {sacc[kt][r], sacc[kt][r + 1]};
          const f32x2 ev = __builtin_elementwise_fma(sv, c2v, nmcv);
          const f32x2 e = {__builtin_amdgcn_exp2f(ev.x), __builtin_amdgcn_exp2f(ev.y)};
          sacc[kt][r] = e.x;
          sacc[kt][r + 1] = e.y;
          ps2 += e;
        }
      float ps = ps2.x + ps2.y;
      ps += __shfl_xor(ps, 32);
      l_run = l_run * alpha + ps;
      if (__builtin_amdgcn_ballot_w64(m_new != m_run) != 0) {    // some lane's maximum moved: rescale O^T (alpha == 1 elsewhere)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
          for (int e = 0; e < 16; ++e) oacc[dt][e] *= alpha;
      }
      m_run = m_new;
      // ---- P^T, and O^T += V^T P^T ----
      half8 pf[2][2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) pf[kt][s2] = at_p_frag(sacc[kt], s2);
      __builtin_amdgcn_sched_barrier(0);
      ASTAMP(5 + 4 * kb);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        half8 vf[2][4];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) vf[s2][dt] = *reinterpret_cast<const half8 *>(sb + voffb[fa_p_kstep(kt, s2)] + dt * FA_DT_BYTES);
        __builtin_amdgcn_sched_barrier(0);                     // eight V^T reads in flight before the first MFMA waits
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[s2][dt], pf[kt][s2], oacc[dt], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      ASTAMP(6 + 4 * kb);
      c_slot = fa_ring_next(c_slot);
      --inflight;
    };
    // the last block always runs the tail form (the mask is the identity when T is a multiple of 64)
    if (nkb == 1) {
      body(0, FaBool<true>{}, FaBool<true>{});
    } else {
      body(0, FaBool<true>{}, FaBool<false>{});
      for (int kb = 1; kb < nkb - 1; ++kb) body(kb, FaBool<false>{}, FaBool<false>{});
      body(nkb - 1, FaBool<false>{}, FaBool<true>{});
    }

    // Store tail (attn_tile.h): a query's output row is split across the two halves of the wave; one v_permlane32_swap per dword and pair
    // of register quads gives each lane 8 contiguous dims: 8 16-byte stores per lane instead of 16 8-byte ones (the store tail is issue-bound).
    // The swaps need every lane: only the store is masked.
    if (wave_valid) {                                            // wave-uniform: exactly FA_VM_STORES store instructions, or none
      const float inv = 1.f / l_run;
      f16 *orow = out + (rowbase + min(q, T - 1)) * 512 + it.h * AT_DH + fa_st_dim(0, 0, lh);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int gq = 0; gq < 4; gq += 2) {
          half4 ha, hb;
#pragma unroll
          for (int j = 0; j < 4; ++j) ha[j] = (f16)(oacc[dt][fa_st_reg(gq, 0, j)] * inv), hb[j] = (f16)(oacc[dt][fa_st_reg(gq, 1, j)] * inv);
          const uint2 ua = __builtin_bit_cast(uint2, ha), ub = __builtin_bit_cast(uint2, hb);
          const auto r0 = __builtin_amdgcn_permlane32_swap(ua.x, ub.x, false, false);
          const auto r1 = __builtin_amdgcn_permlane32_swap(ua.y, ub.y, false, false);
          const uint4 ov = {r0[0], r1[0], r0[1], r1[1]};
          if (q < T) *reinterpret_cast<uint4 *>(orow + fa_st_dim(dt, gq, 0)) = ov;
        }
    }
    ASTAMP(2);
    st_prev = fa_store_count(wave_valid);
    first = false;
  }
#ifdef HALO_STAMP
  if (blockIdx.x < 1024 && lane == 0) {
    st[31] = __builtin_amdgcn_s_memtime();
    unsigned long long *o = g_attn_stamps + ((size_t)blockIdx.x * 7 + wave) * 32;
#pragma unroll
    for (int i = 0; i < 32; ++i) o[i] = st[i];
  }
#endif
}

// The same attention for ONE or TWO hypotheses (a tracking frame, src/estimater.py:250-268).  There the kernel above is 8 workgroups whose
// waves each walk all seven key blocks of their 32 queries one after the other behind a 17 k-cycle start-up: 19 us for 0.33 GFLOP.
// Here a workgroup is one (hypothesis, head, 32-query tile) - 52 per hypothesis - and its seven waves take ONE key block of 64 each
// (split-K attention): S^T = K Q^T, a block-local softmax (maximum m_w, sum l_w, P in fp16 relative to m_w), O_w^T = V^T P^T, all operands
// through a wave-private LDS area (coalesced loads, fragments by ds_read_b128; attn_tile.h, FEW IMAGES), then the seven partial results are
// merged through LDS: m = max m_w, O = sum_w 2^((m_w - m) c) O_w / sum_w 2^((m_w - m) c) l_w.  Same products and the same fp16 rounding of P
// as above, relative to the block's maximum instead of the running one: a summation order of its own (the few-image size class, like
// conv_small.hip).
__global__ __launch_bounds__(FS_WAVES * 64) void attention_small_kernel(const f16 *__restrict__ qk, const f16 *__restrict__ vt, int T, f16 *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char fs_lds[];     // per wave: K block -> V^T block -> partial O^T [dim][query]; then [wave][query] m and l
  float *fs_m = reinterpret_cast<float *>(fs_lds + FS_ML_BYTES), *fs_l = fs_m + fs_ml_off(FS_WAVES, 0);
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 31, lh = lane >> 5;
  const int nqt = fs_nqt(T), nkb = fa_nkb(T);
  const int qt = blockIdx.x % nqt, h = (blockIdx.x / nqt) & 3, b = blockIdx.x / (nqt * 4);
  const float c2 = AT_C2;
  f16 *area = reinterpret_cast<f16 *>(fs_lds + (size_t)w * FS_AREA_BYTES);
  if (w < nkb) {
    // K block and V^T block of this wave: coalesced 16-byte loads (a key row is 256 contiguous bytes, a dim row of the block 128), all
    // requested up front; (first form, measured: the fragments as per-lane gathers, 40 per wave at the L1's tag rate: 12.3 us)
    u32x4 kq[16], vq[16];
    {
      const f16 *kbase = qk + qk_row(b, T) + qk_k_col(h);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = fs_ld(lane, u), key = min(w * 64 + (i >> 4), T - 1);       // rows past T repeat the last one (masked below)
        kq[u] = *reinterpret_cast<const u32x4 *>(kbase + (size_t)key * 1024 + (i & 15) * 8);
      }
      const f16 *vbase = vt + vt_head(b, h);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = lane + 64 * u, col = min(w * 64 + (i & 7) * 8, (int)FA_V_LAST_CHUNK);      // (fs_ld written out: through it hipcc orders the loads differently - other vmcnt operands)  chunks past the image's zero pad read its last one (P = 0 there)
        vq[u] = *reinterpret_cast<const u32x4 *>(vbase + (size_t)(i >> 3) * AT_TP + col);
      }
    }
    half8 qf[8];
    {
      const f16 *qrow = qk + ((size_t)b * T + min(qt * 32 + lr, T - 1)) * 1024 + qk_q_col(h) + lh * 8;
#pragma unroll
      for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const half8 *>(qrow + s * 16);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = fs_ld(lane, u);
      *reinterpret_cast<u32x4 *>(area + fs_k_off(i >> 4, (i & 15) * 8)) = kq[u];
    }
    wait_lgkm();                 // (the wave reads what it wrote itself: no barrier)
    half8 kf[2][8];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int s = 0; s < 8; ++s) kf[kt][s] = *reinterpret_cast<const half8 *>(area + fs_k_off(kt * 32 + lr, s * 16 + lh * 8));
    floatx16 sacc[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) sacc[kt][e] = 0.f;
#pragma unroll
      for (int s = 0; s < 8; ++s) sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[kt][s], qf[s], sacc[kt], 0, 0, 0);
    }
    // at_mask_tail (key = first key of the block + fa_s_key) written out: through either this kernel comes out with one SGPR less
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = w * 64 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        sacc[kt][r] = key < T ? sacc[kt][r] : -1.0e30f;
      }
    float bm = fmaxf(sacc[0][0], sacc[1][0]);
#pragma unroll
    for (int r = 1; r < 16; ++r) bm = fmaxf(bm, fmaxf(sacc[0][r], sacc[1][r]));
    bm = fmaxf(bm, __shfl_xor(bm, 32));
    const float nmc = -bm * c2;
    float ps = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(fmaf(sacc[kt][r], c2, nmc));
        sacc[kt][r] = e;
        ps += e;
      }
    ps += __shfl_xor(ps, 32);
    // the K fragments are in registers: the area takes the V^T block (rows = dims, the block's 64 keys in the image's token order)
    wait_lgkm();
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = fs_ld(lane, u);
      *reinterpret_cast<u32x4 *>(area + fs_v_off(i >> 3, (i & 7) * 8)) = vq[u];
    }
    wait_lgkm();
    floatx16 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) oacc[dt][e] = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      if (w * 64 + kt * 32 >= T) continue;                    // (wave-uniform) a key tile past T: P is exactly 0
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const half8 pf = at_p_frag(sacc[kt], s2);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8 *>(area + fs_v_off(dt * 32 + lr, fa_p_kstep(kt, s2) * 16 + lh * 8)), pf,
                                                            oacc[dt], 0, 0, 0);
      }
    }
    wait_lgkm();                 // the V^T block is read: the area takes the partial O^T
    float *po = reinterpret_cast<float *>(area) + lr;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) po[fs_o_off(fa_o_dim(dt, r, lh), 0)] = oacc[dt][r];
    if (lh == 0) fs_m[fs_ml_off(w, lr)] = bm, fs_l[fs_ml_off(w, lr)] = ps;
  }
  __syncthreads();
  if (tid >= 256) return;
  const int ql = fs_merge_q(tid), d0 = fs_merge_dim(tid), q = qt * 32 + ql;        // query ql, dims d0 .. + 16
  if (q >= T) return;
  float m = fs_m[ql];
  for (int k = 1; k < nkb; ++k) m = fmaxf(m, fs_m[fs_ml_off(k, ql)]);
  float l = 0.f, o[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;
  for (int k = 0; k < nkb; ++k) {
    const float sc = __builtin_amdgcn_exp2f((fs_m[fs_ml_off(k, ql)] - m) * c2);
    l += fs_l[fs_ml_off(k, ql)] * sc;
    const float *pk = reinterpret_cast<const float *>(fs_lds + (size_t)k * FS_AREA_BYTES) + fs_o_off(d0, ql);
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = fmaf(pk[fs_o_off(i, 0)], sc, o[i]);
  }
  const float inv = 1.f / l;
  half8 h0, h1;
#pragma unroll
  for (int i = 0; i < 8; ++i) h0[i] = (f16)(o[i] * inv), h1[i] = (f16)(o[8 + i] * inv);
  f16 *orow = out + ((size_t)b * T + q) * 512 + h * AT_DH + d0;
  *reinterpret_cast<half8 *>(orow) = h0;
  *reinterpret_cast<half8 *>(orow + 8) = h1;
}

void attn_kernel_lds(std::vector<KernelLds> &v) {
  v.push_back({(const void *)attention_kernel, (int)FA_LDS_BYTES});
  v.push_back({(const void *)attention_small_kernel, (int)FS_LDS_BYTES});
}

int launch_attention(fp_ctx *ctx, const f16 *qk, const f16 *vt, int B, int T, f16 *out, hipStream_t s) {
  FP_REQUIRE(T > 0 && T <= AT_MAXT, "attention: T=%d must be in [1,%d]", T, AT_MAXT);
  if (B == 0) return FP_OK;
  if (attn_form(B, pass_knobs()) == ATTN_SMALL) {
    ProfScope ps(ctx, s, "attention", 4.0 * B * 4 * (double)T * T * AT_DH);
    hipLaunchKernelGGL(attention_small_kernel, dim3(fs_nqt(T) * 4 * B), dim3(FS_WAVES * 64), FS_LDS_BYTES, s, qk, vt, T, out);
    FP_CHECK_HIP(hipGetLastError());
    return FP_OK;
  }
  const int n_items = fa_n_items(B, T);
  const int grid = n_items < ctx->num_cu ? n_items : ctx->num_cu;        // one persistent workgroup per CU (152 KB of LDS each)
  ProfScope ps(ctx, s, "attention", 4.0 * B * 4 * (double)T * T * AT_DH);
  hipLaunchKernelGGL(attention_kernel, dim3(grid), dim3(FA_THREADS), FA_LDS_BYTES, s, qk, vt, T, out, n_items);
  FP_CHECK_HIP(hipGetLastError());
  return FP_OK;
}
