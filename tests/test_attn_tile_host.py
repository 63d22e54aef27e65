"""CPU: the index rules of the attention kernels (foundationpose_amd/csrc/attn_tile.h), checked exhaustively by a stand-alone program that is
compiled against the header alone - no HIP, no GPU - at T = 400, 384, 230, 130, 64, 37 and 1.  The program restates only the kernels'
constants, the order in which a wave of attention_kernel issues its vector-memory operations, and two facts of the hardware (the
32x32 MFMA output layout: register r of lane half lh is row (r & 3) + 8 (r >> 2) + 4 lh; v_permlane32_swap exchanges the first operand's
lanes 32 - 63 with the second's lanes 0 - 31); the rules come from the header the kernels compile.

Every check is of the form "what a read addresses is what the fill put there": the 35 stage DMAs of the 7 waves against the K and V^T
fragment reads, the V^T columns through vt_col against the keys of the S^T registers that form the P^T operand, the tail mask against the
keys the score registers really hold, the Q^T staging against its fragment read, the item map and the walk, the ring slots, the store
tail through the lane swap, and the few-image kernel's three uses of a wave's area and its merge.  Banks as in test_tok_tile_host.py:
every fragment read (K, V^T, Q^T, and the few-image kernel's K and V^T) is conflict free per 16-lane quarter, as the comments said.

Wait counts: one wave's in-order queue of vector-memory operations is replayed over a workgroup's walk (1, 2 and 4 items; 1, 2, 3, 4, 6
and 7 key blocks; waves with and without stores).  At every wait the operations that must have landed - this block, at kb 0 this item's
Q^T, and whatever an earlier wait of the walk already required - must be older than the youngest fa_wait_allowed() ones (safe), and the
count is a member of FA_WAIT_SET.  The count is also TIGHT (the oldest operation it lets stay in flight is the first that is not needed)
at every wait but two, which the old comment ("allows exactly the operations younger than block p") did not mention and the header now
states: at kb 1 of a later item the previous item's stores, issued behind block 1's DMA, are younger than block 1 and the rule does not
count them (5 or 13 where 13 or 21 would do); at kb 2 of an item with a successor the next item's Q^T, issued behind block 2's DMA in
iteration 0, is younger than block 2 (5 where 13 would do).  Both times the wait also requires 8 operations issued one or two whole
iterations earlier.  The program asserts exactly that slack, made of exactly those operations, there and none anywhere else.

Two pieces the kernels keep written out, because routing them through the header changed what hipcc emits (comments in attn.hip): the
limit of the stage DMA's clamp in attention_kernel (the program checks fa_dma_lim, which attn.hip restates) and the tail mask and the
V^T load index of attention_small_kernel.  The kernels' own text is pinned by test_gpu_kernels.py::test_attention_bits_are_the_recorded_ones."""
import os
import re
import subprocess

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CSRC = os.path.join(REPO, 'foundationpose_amd', 'csrc')

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "attn_tile.h"

#define CHECK(c, ...) do { if (!(c)) { printf("FAILED %s:%d %s: ", section, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)
static const char *section = "";

// most lanes of a 16-lane quarter that name different addresses in one bank group (1: conflict free); 16-byte accesses
static int ways(const int (&addr)[64]) {
  int worst = 0;
  for (int q = 0; q < 4; ++q)
    for (int a = 0; a < 16; ++a) {
      int n = 1;
      for (int b = 0; b < 16; ++b) {
        const int x = addr[q * 16 + a], y = addr[q * 16 + b];
        CHECK(x % 16 == 0, "address %d", x);
        if (b != a && x != y && (x / 16) % 16 == (y / 16) % 16) ++n;
      }
      if (n > worst) worst = n;
    }
  return worst;
}
static int imin(int a, int b) { return a < b ? a : b; }
static int mfma_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }      // 32x32 MFMA output: the row register r of lane half lh holds

// the keys of the P^T operand of k-step (kt, s2), lane half lh, against 8 image columns from col on (colmax: the clamp of the loads)
static void check_pt_columns(int key0, int kt, int s2, int lh, int col, int T, int colmax) {
  const int want = key0 + fa_p_kstep(kt, s2) * 16 + 8 * lh;
  CHECK(col + 7 <= 415, "columns %d .. past the image", col);
  if (want > colmax) {                                           // clamped chunk: every key of the operand is >= T (P = 0), the columns are pad
    CHECK(col == colmax && col >= T, "clamped chunk at %d", col);
    for (int j = 0; j < 8; ++j) CHECK(key0 + fa_s_key(kt, fa_p_reg(s2, j), lh) >= T, "key %d of a clamped chunk", key0 + fa_s_key(kt, fa_p_reg(s2, j), lh));
    return;
  }
  CHECK(col == want, "k-step (%d, %d) half %d reads columns %d, wanted %d", kt, s2, lh, col, want);
  for (int j = 0; j < 8; ++j) {
    const int key = key0 + fa_s_key(kt, fa_p_reg(s2, j), lh);
    CHECK(vt_col(key) == col + j, "register %d of tile %d half %d: key %d is column %d, the fragment's element %d is column %d", fa_p_reg(s2, j), kt, lh, key, vt_col(key), j, col + j);
  }
}

struct Held { int kind, row, col; unsigned src; };              // 16 bytes of a stage: kind 0 K (key row, first dim) / 1 V^T (dim row, first image column)

static void stage(int T) {
  section = "stage_fill";
  const int nkb = fa_nkb(T);
  for (int kb = 0; kb < nkb; ++kb) {
    std::vector<Held> lds(FA_STAGE_HALFS * 2 / 16, Held{-1, 0, 0, 0});
    int issued = 0, surplus = 0;
    for (int wave = 0; wave < FA_WAVES; ++wave)
      for (int u = 0; u < FA_DMA_PER_WAVE; ++u) {
        const int i = fa_dma_instr(wave, u);
        CHECK(i >= 0 && i < FA_STAGE_DMAS, "instruction %d", i);
        ++issued;
        for (int lane = 0; lane < 64; ++lane) {
          const bool is_k = fa_dma_is_k(i);
          const FaDmaLane l = fa_dma_lane(i, lane);
          const unsigned src = fa_dma_src(is_k, kb, l, T);
          CHECK(fa_dma_lim(is_k, T) == (is_k ? (unsigned)(T - 1) : FA_V_LAST_CHUNK), "limit");      // what attn.hip writes out
          const int pos = fa_slot(0) * 2 + fa_dma_lds(i) * 2 + 16 * lane;
          Held h;
          if (is_k) h = Held{0, (int)(src / 2048), (int)(src % 2048) / 2, src};      // K row `key` of the head starts at key * 1024 halfs
          else h = Held{1, (int)(src / (AT_TP * 2)), (int)(src % (AT_TP * 2)) / 2, src};
          CHECK(src % 16 == 0 && pos % 16 == 0 && pos + 16 <= FA_STAGE_HALFS * 2, "alignment / extent: source %u, destination %d", src, pos);
          if (is_k) CHECK(h.row < T && h.col + 8 <= AT_DH, "K source row %d dims %d ..", h.row, h.col);
          else CHECK(h.row < AT_DH && h.col + 8 <= AT_TP, "V source dim %d columns %d ..", h.row, h.col);
          Held &d = lds[pos / 16];
          if (d.kind != -1) {
            CHECK(d.src == src && d.kind == h.kind, "position %d written twice with different sources", pos);
            ++surplus;
          }
          d = h;
        }
      }
    CHECK(issued == 35 && surplus == 3 * 64, "%d instructions, %d surplus lanes", issued, surplus);
    for (const Held &h : lds) CHECK(h.kind != -1, "a position of the stage is not filled");
    for (int kt = 0; kt < 2; ++kt)
      for (int s = 0; s < 8; ++s) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
          const int lr = lane & 31, lh = lane >> 5, a = (int)fa_kfrag(s, lr, lh) + kt * FA_KT_BYTES;
          CHECK(a % 16 == 0 && a + 16 <= FA_V_BYTES, "K fragment address %d", a);
          const Held &h = lds[a / 16];
          CHECK(h.kind == 0 && h.row == imin(kb * FA_KB + kt * 32 + lr, T - 1) && h.col == 16 * s + 8 * lh, "K fragment (%d, %d) lane %d reads key %d dims %d", s, kt, lane, h.row, h.col);
          addr[lane] = a;
        }
        CHECK(ways(addr) == 1, "K fragment read (%d, %d): %d-way", s, kt, ways(addr));
      }
    for (int kt = 0; kt < 2; ++kt)
      for (int s2 = 0; s2 < 2; ++s2)
        for (int dt = 0; dt < 4; ++dt) {
          int addr[64];
          for (int lane = 0; lane < 64; ++lane) {
            const int lr = lane & 31, lh = lane >> 5, a = (int)fa_vfrag(fa_p_kstep(kt, s2), lr, lh) + dt * FA_DT_BYTES;
            CHECK(a % 16 == 0 && a >= FA_V_BYTES && a + 16 <= FA_STAGE_HALFS * 2, "V^T fragment address %d", a);
            const Held &h = lds[a / 16];
            CHECK(h.kind == 1 && h.row == dt * 32 + lr, "V^T fragment (%d, %d) lane %d reads dim %d", fa_p_kstep(kt, s2), dt, lane, h.row);
            check_pt_columns(kb * FA_KB, kt, s2, lh, h.col, T, (int)FA_V_LAST_CHUNK);
            addr[lane] = a;
          }
          CHECK(ways(addr) == 1, "V^T fragment read (%d, %d): %d-way", fa_p_kstep(kt, s2), dt, ways(addr));
        }
  }
}

static void tail(int T) {
  section = "tail";
  const int nkb = fa_nkb(T);
  for (int kb = 0; kb + 1 < nkb; ++kb) CHECK(kb * FA_KB + FA_KB - 1 < T, "block %d of %d holds a key >= T", kb, nkb);
  // the key a score register holds: the MFMA row is the lane of the K fragment, which read key min(block + kt*32 + row, T - 1)
  for (int kb = 0; kb < nkb; ++kb)
    for (int kt = 0; kt < 2; ++kt)
      for (int r = 0; r < 16; ++r)
        for (int lh = 0; lh < 2; ++lh) {
          const int true_key = kb * FA_KB + kt * 32 + mfma_row(r, lh), named = kb * FA_KB + fa_s_key(kt, r, lh);
          CHECK(named == true_key, "register %d of tile %d half %d: named key %d, holds key %d", r, kt, lh, named, true_key);
          if (true_key >= T) CHECK(kb == nkb - 1 && named >= T, "key %d >= T outside the mask", true_key);      // at_mask_tail: key0 + fa_s_key >= T, last block only
        }
}

static void qt(int T) {
  section = "qt";
  for (int qb = 0; qb < fa_nqb(T); ++qb)
    for (int wave = 0; wave < FA_WAVES; ++wave) {
      struct Q { int row, dim; };
      std::vector<Q> area(FA_QW_HALFS * 2 / 16, Q{-1, 0});
      for (int s = 0; s < 8; ++s)
        for (int lane = 0; lane < 64; ++lane) {
          const int lr = lane & 31, lh = lane >> 5;
          const unsigned src = fa_q_src(fa_q_row(wave, lr), lh, T, qb) + s * 16 * 2;      // from (row qb*224, Q of the head)
          const int pos = fa_q_lds(s) * 2 + 16 * lane;
          CHECK(src % 16 == 0 && pos + 16 <= FA_QW_HALFS * 2 && area[pos / 16].row == -1, "Q^T destination %d", pos);
          area[pos / 16] = Q{qb * FA_QB + (int)(src / 2048), (int)(src % 2048) / 2};
        }
      for (int s = 0; s < 8; ++s) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
          const int lr = lane & 31, lh = lane >> 5, a = (fa_q_lds(s) + lane * 8) * 2;
          const Q &q = area[a / 16];
          CHECK(q.row == imin(fa_query(qb, wave, lr), T - 1) && q.row >= 0 && q.dim == 16 * s + 8 * lh && q.dim + 8 <= AT_DH, "Q^T fragment %d lane %d reads row %d dims %d", s, lane, q.row, q.dim);
          addr[lane] = a;
        }
        CHECK(ways(addr) == 1, "Q^T fragment read %d: %d-way", s, ways(addr));
      }
    }
}

static void items(int T) {
  section = "items";
  const int nqb = fa_nqb(T);
  CHECK(nqb == (T + 223) / 224 && fa_nkb(T) == (T + 63) / 64, "counts");
  for (int B : {1, 3, 33}) {
    const int n = fa_n_items(B, T);
    CHECK(n == nqb * 4 * B, "n_items");
    for (int L = 0; L < n; ++L) {
      const FaItem it = fa_item(L, nqb);
      CHECK(it.b >= 0 && it.b < B && it.h >= 0 && it.h < 4 && it.qb >= 0 && it.qb < nqb && (it.b * 4 + it.h) * nqb + it.qb == L, "item %d -> (%d, %d, %d)", L, it.b, it.h, it.qb);
      CHECK(qk_row(it.b, T) + qk_k_col(it.h) == ((size_t)it.b * T) * 1024 + 512 + it.h * 128 && qk_q_col(it.h) == it.h * 128 && vt_head(it.b, it.h) == vt_row(it.b, it.h * 128), "sources");
    }
    for (int G : {1, n > 1 ? n - 1 : 1, n, n + 5, 256}) {
      std::vector<int> seen(n, 0);
      for (int j = 0; j < G; ++j)
        for (int v = j; fa_walk_has(v, n); v = fa_walk_next(v, G)) ++seen[v];
      for (int v = 0; v < n; ++v) CHECK(seen[v] == 1, "G = %d: item %d visited %d times", G, v, seen[v]);
    }
  }
}

// one wave's queue of vector-memory operations over a workgroup's walk of n items, in the kernel's issue order; valid[it]: the wave stores
enum { OP_BLOCK, OP_QT, OP_STORE };
struct Op { int type, item, kb; };
static void waits(int nkb, int n, const bool *valid) {
  std::vector<Op> q;
  std::vector<int> slot_of(n * nkb, -1);                         // ring slot a block was staged into
  int s_item = 0, s_kb = 0, s_slot = 0, inflight = 0, c_slot = 0, st_prev = 0, must = -1;
  bool first = true;
  auto stage_next = [&]() {
    for (int u = 0; u < FA_DMA_PER_WAVE; ++u) q.push_back(Op{OP_BLOCK, s_item, s_kb});
    slot_of[s_item * nkb + s_kb] = s_slot;
    const int written = s_slot;
    s_slot = fa_ring_next(s_slot);
    if (++s_kb == nkb) s_kb = 0, ++s_item;
    ++inflight;
    return written;
  };
  auto last_of = [&](int type, int item, int kb) {
    for (int i = (int)q.size() - 1; i >= 0; --i)
      if (q[i].type == type && q[i].item == item && (type != OP_BLOCK || q[i].kb == kb)) return i;
    return -1;
  };
  for (int p = 0; p < FA_AHEAD; ++p)
    if (s_item < n) stage_next();
  for (int e = 0; e < FA_VM_QT; ++e) q.push_back(Op{OP_QT, 0, 0});
  for (int it = 0; it < n; ++it) {
    const bool has_next = it + 1 < n;
    for (int kb = 0; kb < nkb; ++kb) {
      section = "waits";
      const int allowed = fa_wait_allowed(kb, nkb, first, has_next, inflight, st_prev);
      bool member = false;
      for (int w : FA_WAIT_SET) member = member || w == allowed;
      CHECK(member, "item %d kb %d: %d is not a wait the kernel instantiates", it, kb, allowed);
      const int blk = last_of(OP_BLOCK, it, kb), qt_ = kb == 0 ? last_of(OP_QT, it, 0) : -1;
      CHECK(blk >= 0 && (kb != 0 || qt_ >= 0), "item %d kb %d: the block or the Q^T was never issued", it, kb);
      if (blk > must) must = blk;
      if (qt_ > must) must = qt_;
      const int landed = (int)q.size() - allowed;                // operations 0 .. landed - 1 have landed behind this wait
      CHECK(allowed >= 0 && must < landed, "nkb %d items %d, item %d kb %d: allowed %d leaves operation %d (of %d) in flight: NOT SAFE", nkb, n, it, kb, allowed, must, (int)q.size());
      const int slack = landed - (must + 1);                     // operations it waits for that nothing needs yet
      // the two waits that are not tight (attn_tile.h, WAITS): kb 1 of a later item also waits for the previous item's stores (issued behind
      // block 1's DMA), kb 2 of an item with a successor for the next item's Q^T (issued behind block 2's DMA)
      const int want = kb == 1 && !first ? st_prev : kb == 2 && has_next ? FA_VM_QT : 0;
      CHECK(slack == want, "nkb %d items %d, item %d kb %d (first %d, has_next %d): allowed %d waits for %d operations nothing needs yet, expected %d", nkb, n, it, kb, (int)first, (int)has_next, allowed, slack, want);
      for (int i = must + 1; i < landed; ++i)
        CHECK(kb == 1 ? q[i].type == OP_STORE && q[i].item == it - 1 : q[i].type == OP_QT && q[i].item == it + 1, "item %d kb %d waits for operation %d of another kind", it, kb, i);
      section = "ring";
      // barrier p passed: this block is read from c_slot - where it was staged - and the DMA issued now fills the slot of the previous block
      CHECK(slot_of[it * nkb + kb] == c_slot, "item %d kb %d is read from slot %d, was staged into %d", it, kb, c_slot, slot_of[it * nkb + kb]);
      if (s_item < n) {
        const int written = stage_next();
        const int prev = (c_slot + FA_NSTAGE - 1) % FA_NSTAGE, next = fa_ring_next(c_slot);
        CHECK(written == prev && written != c_slot && written != next, "behind the barrier of item %d kb %d (slot %d) the DMA writes slot %d", it, kb, c_slot, written);
        CHECK(inflight <= FA_NSTAGE, "%d blocks in a ring of %d", inflight, FA_NSTAGE);
      }
      if (kb == 0 && has_next)
        for (int e = 0; e < FA_VM_QT; ++e) q.push_back(Op{OP_QT, it + 1, 0});
      c_slot = fa_ring_next(c_slot);
      --inflight;
    }
    for (int e = 0; e < fa_store_count(valid[it]); ++e) q.push_back(Op{OP_STORE, it, 0});
    st_prev = fa_store_count(valid[it]);
    first = false;
  }
}

static void waits_all() {
  section = "waits";
  CHECK(FA_VM_BLOCK == 5 && FA_VM_QT == 8 && fa_store_count(true) == 8 && fa_store_count(false) == 0, "named counts");
  const bool all[4] = {true, true, true, true}, none[4] = {false, false, false, false}, alt[4] = {true, false, true, false}, alt2[4] = {false, true, false, true};
  for (int nkb : {1, 2, 3, 4, 6, 7})
    for (int n : {1, 2, 4})
      for (const bool *v : {all, none, alt, alt2}) waits(nkb, n, v);
  // T = 230: items alternate between the two query blocks (qb is the fastest index); in the second only wave 0 has a query
  const int T = 230;
  for (int wave : {0, 1, 6}) {
    bool v[4];
    for (int it = 0; it < 4; ++it) v[it] = fa_query(fa_item(it, fa_nqb(T)).qb, wave, 0) < T;
    CHECK(v[0] && v[1] == (wave == 0), "T = 230: wave %d", wave);
    waits(fa_nkb(T), 4, v);
    waits(fa_nkb(T), 2, v + 1);
  }
}

static void store_tail() {
  section = "store_tail";
  // value = the dim an O^T register of a lane holds; the swap (hardware): new a = {a of lanes 0-31, b of lanes 0-31}, new b = {a of lanes 32-63, b of lanes 32-63}
  std::vector<int> seen(32 * AT_DH, 0);
  int stores = 0;
  for (int dt = 0; dt < 4; ++dt)
    for (int gq = 0; gq < 4; gq += 2) {
      ++stores;
      for (int lane = 0; lane < 64; ++lane) {
        const int lr = lane & 31, lh = lane >> 5;
        int ov[8];                                               // the 8 halfs a lane stores: {new a (4 halfs), new b (4 halfs)}
        for (int j = 0; j < 4; ++j) {
          const int a_lo = fa_o_dim(dt, fa_st_reg(gq, 0, j), 0), a_hi = fa_o_dim(dt, fa_st_reg(gq, 0, j), 1);      // ha of the lane with this query in half 0 / 1
          const int b_lo = fa_o_dim(dt, fa_st_reg(gq, 1, j), 0), b_hi = fa_o_dim(dt, fa_st_reg(gq, 1, j), 1);      // hb
          ov[j] = lh == 0 ? a_lo : b_lo;
          ov[4 + j] = lh == 0 ? a_hi : b_hi;
        }
        const int dim0 = fa_st_dim(0, 0, lh) + fa_st_dim(dt, gq, 0);
        CHECK(dim0 == fa_st_dim(dt, gq, lh) && (dim0 * 2) % 16 == 0 && (512 * 2) % 16 == 0 && (AT_DH * 2) % 16 == 0, "store of (%d, %d) half %d at dim %d", dt, gq, lh, dim0);
        for (int e = 0; e < 8; ++e) {
          CHECK(ov[e] == dim0 + e, "(dt %d, gq %d) half %d element %d: the register holds dim %d, the store puts it at dim %d", dt, gq, lh, e, ov[e], dim0 + e);
          CHECK(ov[e] == fa_o_dim(dt, fa_st_reg(gq, lh, e), fa_st_half(e)), "(dt %d, gq %d) half %d element %d: not the register the header names", dt, gq, lh, e);
          CHECK(dim0 + e < AT_DH, "dim %d", dim0 + e);
          ++seen[lr * AT_DH + dim0 + e];
        }
      }
    }
  CHECK(stores == FA_VM_STORES, "%d stores per lane", stores);
  for (int n = 0; n < 32 * AT_DH; ++n) CHECK(seen[n] == 1, "query %d dim %d written %d times", n / AT_DH, n % AT_DH, seen[n]);
}

static void few_images(int T) {
  section = "few_images";
  CHECK(64 * FS_KP * 2 <= FS_AREA_BYTES && AT_DH * FS_VP * 2 <= FS_AREA_BYTES && AT_DH * 32 * 4 <= FS_AREA_BYTES, "a wave's area");
  CHECK(FS_ML_BYTES == FS_WAVES * FS_AREA_BYTES && FS_LDS_BYTES == FS_ML_BYTES + 2 * FS_WAVES * 32 * 4 && fa_nkb(T) <= FS_WAVES && fs_nqt(T) == (T + 31) / 32, "sizes");
  for (int w = 0; w < fa_nkb(T); ++w) {
    struct H { int row, col; };
    std::vector<H> k(FS_AREA_BYTES / 16, H{-1, 0}), v(FS_AREA_BYTES / 16, H{-1, 0});
    for (int u = 0; u < 16; ++u)
      for (int lane = 0; lane < 64; ++lane) {
        const int i = fs_ld(lane, u);
        const int ko = fs_k_off(i >> 4, (i & 15) * 8) * 2, vo = fs_v_off(i >> 3, (i & 7) * 8) * 2;
        CHECK(ko % 16 == 0 && ko + 16 <= FS_AREA_BYTES && k[ko / 16].row == -1, "K staging write at %d", ko);
        CHECK(vo % 16 == 0 && vo + 16 <= FS_AREA_BYTES && v[vo / 16].row == -1, "V^T staging write at %d", vo);
        k[ko / 16] = H{imin(w * 64 + (i >> 4), T - 1), (i & 15) * 8};
        v[vo / 16] = H{i >> 3, imin(w * 64 + (i & 7) * 8, (int)FA_V_LAST_CHUNK)};
      }
    for (int kt = 0; kt < 2; ++kt)
      for (int s = 0; s < 8; ++s) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
          const int lr = lane & 31, lh = lane >> 5, a = fs_k_off(kt * 32 + lr, s * 16 + lh * 8) * 2;
          CHECK(a % 16 == 0 && k[a / 16].row == imin(w * 64 + kt * 32 + lr, T - 1) && k[a / 16].col == 16 * s + 8 * lh, "K fragment (%d, %d) lane %d", s, kt, lane);
          addr[lane] = a;
        }
        CHECK(ways(addr) == 1, "K fragment read: %d-way", ways(addr));
      }
    for (int kt = 0; kt < 2; ++kt)
      for (int s2 = 0; s2 < 2; ++s2)
        for (int dt = 0; dt < 4; ++dt) {
          int addr[64];
          for (int lane = 0; lane < 64; ++lane) {
            const int lr = lane & 31, lh = lane >> 5, a = fs_v_off(dt * 32 + lr, fa_p_kstep(kt, s2) * 16 + lh * 8) * 2;
            CHECK(a % 16 == 0 && v[a / 16].row == dt * 32 + lr, "V^T fragment (%d, %d, %d) lane %d", kt, s2, dt, lane);
            check_pt_columns(w * 64, kt, s2, lh, v[a / 16].col, T, (int)FA_V_LAST_CHUNK);
            addr[lane] = a;
          }
          CHECK(ways(addr) == 1, "V^T fragment read: %d-way", ways(addr));
        }
    // keys >= T of this wave's block: named by the mask the kernel writes out (w * 64 + the MFMA row of the register)
    for (int kt = 0; kt < 2; ++kt)
      for (int r = 0; r < 16; ++r)
        for (int lh = 0; lh < 2; ++lh) CHECK(w * 64 + fa_s_key(kt, r, lh) == w * 64 + kt * 32 + mfma_row(r, lh), "score register %d", r);
  }
  // partial O^T of a wave [dim][query] floats, and the merge's reads
  std::vector<int> po(FS_AREA_BYTES / 4, -1);
  for (int dt = 0; dt < 4; ++dt)
    for (int r = 0; r < 16; ++r)
      for (int lane = 0; lane < 64; ++lane) {
        const int lr = lane & 31, lh = lane >> 5, dim = dt * 32 + mfma_row(r, lh), o = fs_o_off(fa_o_dim(dt, r, lh), 0) + lr;
        CHECK(o == fs_o_off(dim, lr) && o >= 0 && o < FS_AREA_BYTES / 4 && po[o] == -1, "partial O^T write of dim %d query %d at %d", dim, lr, o);
        po[o] = dim * 32 + lr;
      }
  std::vector<int> seen(32 * AT_DH, 0);
  for (int tid = 0; tid < 256; ++tid) {
    const int ql = fs_merge_q(tid), d0 = fs_merge_dim(tid);
    CHECK(ql >= 0 && ql < 32 && d0 % 16 == 0 && d0 + 16 <= AT_DH && (d0 * 2) % 16 == 0, "merge thread %d", tid);
    for (int i = 0; i < 16; ++i) {
      const int o = fs_o_off(d0, ql) + fs_o_off(i, 0);
      CHECK(o < FS_AREA_BYTES / 4 && po[o] == (d0 + i) * 32 + ql, "merge thread %d reads element %d for dim %d", tid, o, d0 + i);
      ++seen[ql * AT_DH + d0 + i];
    }
  }
  for (int n = 0; n < 32 * AT_DH; ++n) CHECK(seen[n] == 1, "query %d dim %d merged %d times", n / AT_DH, n % AT_DH, seen[n]);
  std::vector<int> ml(2 * FS_WAVES * 32, 0);                      // m [wave][32], l behind it
  for (int w = 0; w < FS_WAVES; ++w)
    for (int lr = 0; lr < 32; ++lr) ++ml[fs_ml_off(w, lr)], ++ml[fs_ml_off(FS_WAVES, 0) + fs_ml_off(w, lr)];
  for (int x : ml) CHECK(x == 1, "m / l arrays");
  CHECK((FS_ML_BYTES + (int)ml.size() * 4) == FS_LDS_BYTES, "m / l arrays end with the LDS");
}

int main() {
  CHECK(AT_TP == VT_LD && FA_THREADS == 448 && FA_QB == 224 && FA_LDS_BYTES == (3 * 16384 + 7 * 4096) * 2 && FA_Q_HALFS == 3 * FA_STAGE_HALFS, "geometry");
  for (int T : {400, 384, 230, 130, 64, 37, 1}) {
    stage(T);
    tail(T);
    qt(T);
    items(T);
    few_images(T);
  }
  waits_all();
  store_tail();
  printf("ok\n");
  return 0;
}
'''


def build_and_run(tmp, header_dir=CSRC):
  """The compiler beside the hipcc the Makefile names (ROCm's clang++), on attn_tile.h (and tok_tile.h, which it includes) alone."""
  hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC \?= (\S+)', open(os.path.join(CSRC, 'Makefile')).read(), flags=re.M).group(1)
  cxx = os.path.join(os.path.dirname(hipcc), 'amdclang++')
  src, exe = tmp / 'attn.cc', tmp / 'attn'
  src.write_text(PROGRAM)
  subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(header_dir), str(src), '-o', str(exe)], check=True)
  return subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.fixture(scope='module')
def result(tmp_path_factory):
  return build_and_run(tmp_path_factory.mktemp('attn_tile'))


def test_reads_address_what_the_fills_put_there(result):
  assert result.returncode == 0 and result.stdout == 'ok\n', result.stdout + result.stderr
