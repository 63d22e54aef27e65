"""CPU: the index rules of the token GEMMs (foundationpose_amd/csrc/tok_tile.h), checked exhaustively by a stand-alone program that is
compiled against the header alone - no HIP, no GPU - over the geometries of tok_gemm.hip, tok_qkv.hip and head_mlp.hip (the constants below
restate their tile sizes, wave counts and staging sizes; the rules themselves come from the header the kernels compile).

Every check is of the form "what a read addresses is what the fill put there": the tile and ring DMA maps against the fragment reads of both
K-loop forms, the accumulator layout against the next layer's fragment reads (the in-place epilogues), pack_tok_weights' image against the
three ownership rules, the swapped accumulator layout through the three epilogue stagings against the V image, the group sums.

Banks: an LDS access is conflict free when, within each 16-lane quarter, two lanes with different addresses differ in their bank group (16
bytes of 256 for a 16-byte access; 8 of 128 for an 8-byte write, which the LDS takes 16 lanes at a time over 32 banks).  The program
asserts the exact figure of every access:
  * conflict free: every fragment read of the resident tile (both read forms), the row read-backs of tok_gemm.hip and tok_qkv.hip and
    tok_qkv.hip's V read-back;
  * two-way: the fragment reads of head_mlp128_kernel's ring (128-byte rows put two rows into 256 bytes: rows r and r + 8 of a quarter share
    a bank group whatever the XOR with row & 7 does; no comment claimed otherwise), tok_gemm.hip's V read-back (one pair of lanes per
    quarter), and every 8-byte staging WRITE of the accumulator quads (lanes lr and lr + 8 of a quarter).
One comment claimed more than holds and is corrected: TG_STAGE_LD's "256 B + 16 B pad: conflict-free 8-byte writes" - the pad makes the
16-byte read-backs conflict free, not the writes."""
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
#include "tok_tile.h"

#define CHECK(c, ...) do { if (!(c)) { printf("FAILED %s:%d %s: ", section, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)
static const char *section = "";

// most lanes of a 16-lane quarter that name different addresses in one bank group (1: conflict free); unit 16: ds_read_b128, 8: ds_write_b64
static int ways(const int (&addr)[64], int unit) {
  int worst = 0;
  for (int q = 0; q < 4; ++q)
    for (int a = 0; a < 16; ++a) {
      int n = 1;
      for (int b = 0; b < 16; ++b) {
        const int x = addr[q * 16 + a], y = addr[q * 16 + b];
        CHECK(x % unit == 0, "address %d", x);
        if (b != a && x != y && (x / unit) % 16 == (y / unit) % 16) ++n;
      }
      if (n > worst) worst = n;
    }
  return worst;
}

struct Held { int m, k; };      // the 16 bytes at an LDS position: token row m (global), k elements k .. k + 7

// 1 + 2: tile fill against both read forms, banks
template <int ROWS, int WAVES>
static void tile(int m0, int M) {
  section = "tile";
  std::vector<Held> lds(4 * ROWS * 16, Held{-1, -1});
  for (int seg = 0; seg < 4; ++seg)
    for (int wave = 0; wave < WAVES; ++wave)
      for (int u = 0; u < ROWS / 4 / WAVES; ++u)
        for (int lane = 0; lane < 64; ++lane) {
          const int r4 = tile_dma_r4(ROWS, WAVES, wave, u), row = tile_dma_row(r4, lane), chunk = tile_dma_chunk(row, lane);
          const int m = tok_src_row(m0, row, M), pos = tile_dma_lds(ROWS, seg, r4) + 16 * lane;
          CHECK(row < ROWS && m < M && m == (m0 + row < M ? m0 + row : M - 1), "row %d", row);
          CHECK(tok_src_bytes(m, seg * 128, chunk) == ((size_t)m * 512 + seg * 128 + chunk * 8) * 2, "source of (%d, %d)", seg, r4);
          CHECK(pos == tile_off(ROWS, row, seg * 128 + chunk * 8), "DMA of row %d chunk %d lands at %d", row, chunk, pos);
          CHECK(lds[pos / 16].m == -1, "position %d filled twice", pos);
          lds[pos / 16] = Held{m, seg * 128 + chunk * 8};
        }
  for (const Held &h : lds) CHECK(h.m >= 0, "a position is not filled");
  for (int k16 = 0; k16 < 32; ++k16)
    for (int j = 0; j < ROWS / 32; ++j) {
      int addr[64];
      for (int lane = 0; lane < 64; ++lane) {
        const int lr = lane & 31, lh = lane >> 5;
        const int table = tile_frag_addr(ROWS, k16, j, lr, lh);
        const int split = tile_frag_base(lr, lh) + tile_frag_seg(ROWS, k16) + (int)tile_frag_x(k16, tile_frag_xe(lr)) + j * 8192;
        CHECK(table == split, "k16 %d j %d lane %d: table form %d, split form %d", k16, j, lane, table, split);
        const Held &h = lds[table / 16];
        CHECK(h.m == tok_src_row(m0, acc_row_token(j, lr), M) && h.k == k16 * 16 + lh * 8, "k16 %d j %d lane %d reads (%d, %d)", k16, j, lane, h.m, h.k);
        addr[lane] = table;
      }
      CHECK(ways(addr, 16) == 1, "fragment read k16 %d j %d: %d-way", k16, j, ways(addr, 16));
    }
}

// head_mlp128_kernel's ring: 8 segments of 64 k through two slots
static void ring(int m0, int M) {
  section = "ring";
  const int ROWS = 128;
  for (int s8 = 0; s8 < 8; ++s8) {
    const int slot = s8 & 1;
    std::vector<Held> lds(2 * ROWS * 8, Held{-1, -1});
    for (int wave = 0; wave < 8; ++wave)
      for (int u = 0; u < 2; ++u)
        for (int lane = 0; lane < 64; ++lane) {
          const int r8 = wave * 2 + u, row = ring_dma_row(r8, lane), chunk = ring_dma_chunk(row, lane);
          const int pos = slot * ring_slot_bytes(ROWS) + r8 * 1024 + 16 * lane;
          CHECK(pos == slot * ring_slot_bytes(ROWS) + ring_off(row, chunk * 8) && lds[pos / 16].m == -1, "DMA of row %d chunk %d lands at %d", row, chunk, pos);
          CHECK(tok_src_bytes(tok_src_row(m0, row, M), s8 * 64, chunk) == ((size_t)tok_src_row(m0, row, M) * 512 + s8 * 64 + chunk * 8) * 2, "source");
          lds[pos / 16] = Held{tok_src_row(m0, row, M), s8 * 64 + chunk * 8};
        }
    for (int k16 = s8 * 4; k16 < s8 * 4 + 4; ++k16)
      for (int j = 0; j < 4; ++j) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
          const int lr = lane & 31, lh = lane >> 5;
          const int x = ring_frag_base(lr, lh) + ring_frag_slot(ROWS, k16) + j * 4096 + (int)ring_frag_x(k16, ring_frag_xe(lr));
          const Held &h = lds[x / 16];
          CHECK(h.m == tok_src_row(m0, j * 32 + lr, M) && h.k == k16 * 16 + lh * 8, "segment %d k16 %d j %d lane %d reads (%d, %d)", s8, k16, j, lane, h.m, h.k);
          addr[lane] = x;
        }
        // 128-byte rows: two rows per 256 bytes, bank group of (row, chunk c) = (row & 1) * 8 + (c ^ (row & 7)) - rows r and r + 8 of a quarter share it
        CHECK(ways(addr, 16) == 2, "ring read k16 %d j %d: %d-way", k16, j, ways(addr, 16));
      }
  }
}

// 3: the half chunk a lane of the row layout writes (in-place epilogues) or reads (residual) is where the K loop of the next layer reads the
// same channels of the same row as k elements
template <int ROWS, int WAVES>
static void in_place() {
  section = "in_place";
  const int NI = 16 / WAVES;
  for (int wave = 0; wave < WAVES; ++wave)
    for (int i = 0; i < NI; ++i)
      for (int rg = 0; rg < 4; ++rg)
        for (int j = 0; j < ROWS / 32; ++j)
          for (int lane = 0; lane < 64; ++lane) {
            const int lr = lane & 31, lh = lane >> 5, row = acc_row_token(j, lr), col = wave * NI * 32 + acc_row_chan(i, rg, lh);
            const int off = tile_quad_off<ROWS, WAVES>(wave, i, rg, row, lh);
            CHECK(off == tile_off(ROWS, row, col), "wave %d i %d rg %d row %d lh %d: %d", wave, i, rg, row, lh, off);
            // ... and the fragment read that carries k = col: k-step col / 16, lane half (col >> 3) & 1, bytes (col & 7) * 2 .. + 8 of its 16
            const int k16 = col >> 4, rh = (col >> 3) & 1;
            CHECK(off == tile_frag_addr(ROWS, k16, j, lr, rh) + (col & 7) * 2 && (col & 7) * 2 + 8 <= 16, "fragment of column %d", col);
          }
}

// 4: pack_tok_weights' image (fragment wfrag(), lane, element e <- W[wfrag_src() + e]) against the three ownership rules
static void weights() {
  section = "weights";
  std::vector<int> image(512 * 512, -1);                       // packed position -> index in W
  for (int w4 = 0; w4 < 4; ++w4)
    for (int k16 = 0; k16 < 32; ++k16)
      for (int i4 = 0; i4 < 4; ++i4)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 8; ++e) {
            const size_t dst = (wfrag(w4, k16, i4) * 64 + lane) * 8 + e;
            CHECK(dst < image.size() && image[dst] == -1, "packed position %zu", dst);
            image[dst] = (int)wfrag_src(w4, k16, i4, lane) + e;
          }
  // a wave's MFMA A operand of tile i at k-step k16: lane (lr, lh) must hold W[col0 + i*32 + lr][k16*16 + lh*8 + e] - the k the token fragment
  // of the same k-step carries (tile(): k16 * 16 + lh * 8)
  auto check = [&](std::vector<int> &seen, size_t frag, int col0, int i, int k16) {
    for (int lane = 0; lane < 64; ++lane)
      for (int e = 0; e < 8; ++e) {
        const int src = image[(frag * 64 + lane) * 8 + e], c = col0 + i * 32 + (lane & 31), k = k16 * 16 + (lane >> 5) * 8 + e;
        CHECK(src == c * 512 + k, "fragment %zu lane %d element %d holds W index %d, wanted W[%d][%d]", frag, lane, e, src, c, k);
        ++seen[src];
      }
  };
  std::vector<int> s4(512 * 512, 0), s8(512 * 512, 0), ss(512 * 512, 0);
  for (int k16 = 0; k16 < 32; ++k16) {
    for (int wave = 0; wave < 4; ++wave)
      for (int i = 0; i < 4; ++i) check(s4, wfrag_own4(wave, k16, i), wave * 128, i, k16);
    for (int wave = 0; wave < 8; ++wave)
      for (int i = 0; i < 2; ++i) check(s8, wfrag_own8(wave, k16, i), wave * 64, i, k16);
  }
  for (int g = 0; g < 4; ++g)                                  // tok_qkv_small_kernel: workgroup column quarter g, wave (kq, chh), k-steps kq*8 + k
    for (int kq = 0; kq < 4; ++kq)
      for (int chh = 0; chh < 2; ++chh)
        for (int k = 0; k < 8; ++k)
          for (int i = 0; i < 2; ++i) {
            CHECK(wfrag_own_small(g, kq, chh, k, i) == wfrag_own_small(g, kq, 0, 0, 0) + wfrag_own_small(0, 0, chh, 0, 0) + wfrag(0, k, i), "split of the wave's base");
            check(ss, wfrag_own_small(g, kq, chh, k, i), g * 128 + chh * 64, i, kq * 8 + k);
          }
  for (size_t n = 0; n < s4.size(); ++n) CHECK(s4[n] == 1 && s8[n] == 1 && ss[n] == 1, "W index %zu read %d / %d / %d times", n, s4[n], s8[n], ss[n]);
}

// 5: the V image.  What comes from the header: vt_col, vt_row / vt_index, the group rules, the accumulator layout (acc_vt_*), the staging
// offsets (tg_vt_off, tq_vt_off) and - as store_unit() below, line for line - vt_store_unit.  What the three functions RESTATE from the kernel
// files, because it exists only there: the read-back lane maps (tok_gemm.hip: c = u*8 + lane/8, chunk lane & 7; tok_qkv.hip: c = v*16 + lane/4,
// unit lane & 3), the m < M guards, and the whole store of tok_qkv_small_kernel (lo / hi halves, pad in steps of 8), which that kernel keeps
// written out.  For those parts the checks prove the restated copy; the kernels' own text is pinned by the GPU tests
// (test_gpu_kernels.py::test_token_kernels_bits_are_the_recorded_ones and the V image checks beside it).  row_staging() restates the read-back
// lane maps of the row epilogues in the same way.
static void vt_order() {
  section = "vt_col";
  for (int s = 0; s < 26; ++s) {
    bool seen[16] = {};
    for (int t = 16 * s; t < 16 * s + 16; ++t) {
      const int c = vt_col(t);
      CHECK(c >= 16 * s && c < 16 * s + 16 && !seen[c - 16 * s], "token %d -> column %d", t, c);
      seen[c - 16 * s] = true;
    }
    // attn.hip's key order: lane half h of a k-step of 16 keys carries keys 16s + {4h .. 4h+3, 8+4h .. 8+4h+3} as 8 contiguous columns
    for (int h = 0; h < 2; ++h)
      for (int e = 0; e < 8; ++e) CHECK(vt_col(16 * s + (e < 4 ? 4 * h + e : 8 + 4 * h + e - 4)) == 16 * s + 8 * h + e, "key order, group %d half %d", s, h);
  }
}

struct Image {
  int B, tokens;
  std::vector<int> v;              // -1 unwritten, 0 zero, else 1 + (token row m) * 512 + column
  Image(int B_, int tokens_) : B(B_), tokens(tokens_), v((size_t)B_ * 4 * 128 * VT_LD, -1) {}
  void put(size_t idx, int val) {
    CHECK(idx < v.size(), "write past the image: %zu", idx);
    CHECK(v[idx] == -1, "element %zu written twice", idx);
    v[idx] = val;
  }
  void done() const {
    for (int b = 0; b < B; ++b)
      for (int col = 0; col < 512; ++col) {
        for (int t = 0; t < tokens; ++t) CHECK(v[vt_index(b, col, t)] == 1 + (b * tokens + t) * 512 + col, "(%d, %d, %d) holds %d", b, col, t, v[vt_index(b, col, t)]);
        for (int z = tokens; z < VT_LD; ++z) CHECK(v[vt_row(b, col) + z] == 0, "pad column %d of (%d, %d) holds %d", z, b, col, v[vt_row(b, col) + z]);
      }
  }
};
// the store of one staged 16-byte unit (vt_store_unit): 8 image columns, plus the pad behind a hypothesis' last group
static void store_unit(Image &img, int col, int m, int hf, const int (&val)[8]) {
  const int b = vt_group_hyp(m, img.tokens), t = m - b * img.tokens;
  CHECK(m % 8 == 0 && m + 8 <= img.B * img.tokens, "unit at row %d reaches past row M", m);
  CHECK(b < img.B && (t & ~15) + 16 <= img.tokens && vt_group_hyp(m & ~15, img.tokens) == vt_group_hyp((m & ~15) + 15, img.tokens), "group of row %d spans two hypotheses", m);
  for (int e = 0; e < 8; ++e) img.put(vt_row(b, col) + (t & ~15) + hf * 8 + e, val[e]);
  if (vt_group_is_last(t & ~15, img.tokens))
    for (int z = img.tokens; z < VT_LD; z += 16)
      for (int e = 0; e < 8; ++e) img.put(vt_row(b, col) + z + hf * 8 + e, 0);
}

// tok_gemm.hip EPI_VT: 4 waves x 128 channels, 64-token tile through [channel][TG_VT_LD]
static void vt_tok_gemm(int tokens, int B) {
  section = "vt_tok_gemm";
  const int M = tokens * B;
  Image img(B, tokens);
  for (int m0 = 0; m0 < M; m0 += 64)
    for (int wave = 0; wave < 4; ++wave) {
      std::vector<int> vs(128 * TG_VT_LD, -1);
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 2; ++j)
          for (int q = 0; q < 4; ++q) {
            int addr[64];
            for (int lane = 0; lane < 64; ++lane) {
              const int lr = lane & 31, lh = lane >> 5, ch = acc_vt_chan(i, lr);
              for (int e = 0; e < 4; ++e) {
                const int t = acc_vt_token(j, q * 4 + e, lh);
                CHECK(vt_col(t) == vt_col(acc_vt_token(j, q * 4, lh)) + e, "4 consecutive tokens");
                vs[tg_vt_off(ch, vt_col(t))] = 1 + (m0 + t) * 512 + wave * 128 + ch;
              }
              addr[lane] = tg_vt_off(ch, vt_col(acc_vt_token(j, q * 4, lh))) * 2;
            }
            CHECK(ways(addr, 8) == 2, "tok_gemm V staging write: %d-way", ways(addr, 8));      // lanes lr, lr + 8: TG_VT_LD * 2 * 8 = 0 (mod 128)
          }
      for (int u = 0; u < 16; ++u) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
          const int c = u * 8 + (lane >> 3), ch8 = lane & 7, m = m0 + ch8 * 8;
          addr[lane] = tg_vt_off(c, ch8 * 8) * 2;
          if (m >= M) continue;
          int val[8];
          for (int e = 0; e < 8; ++e) val[e] = vs[tg_vt_off(c, ch8 * 8) + e];
          store_unit(img, wave * 128 + c, m, ch8 & 1, val);
        }
        CHECK(ways(addr, 16) == 2, "tok_gemm V read-back: %d-way", ways(addr, 16));      // two channel rows per quarter, 144 bytes apart: one pair of lanes meets
      }
    }
  img.done();
}

// tok_qkv_kernel: 8 waves x 64 channels, 128-token tile in four 32-token slices through the XOR-ed 4-KB staging
static void vt_tok_qkv(int tokens, int B) {
  section = "vt_tok_qkv";
  const int M = tokens * B;
  Image img(B, tokens);
  for (int m0 = 0; m0 < M; m0 += 128)
    for (int wave = 0; wave < 8; ++wave)
      for (int j = 0; j < 4; ++j) {
        std::vector<int> st(2048, -1);                           // halfs
        for (int i = 0; i < 2; ++i)
          for (int q = 0; q < 4; ++q) {
            int addr[64];
            for (int lane = 0; lane < 64; ++lane) {
              const int lr = lane & 31, lh = lane >> 5, ch = acc_vt_chan(i, lr), pos = vt_col(acc_vt_token(0, q * 4, lh));
              CHECK(pos % 4 == 0 && tq_vt_off(ch, pos) % 8 == 0 && tq_vt_off(ch, pos) + 8 <= 4096, "staging offset");
              for (int e = 0; e < 4; ++e) st[tq_vt_off(ch, pos) / 2 + e] = 1 + (m0 + acc_vt_token(j, q * 4 + e, lh)) * 512 + wave * 64 + ch;
              addr[lane] = tq_vt_off(ch, pos);
            }
            CHECK(ways(addr, 8) == 2, "tok_qkv V staging write: %d-way", ways(addr, 8));      // 64-byte channel rows: channels c, c + 8 (the XOR sees (c >> 1) & 3)
          }
        for (int v = 0; v < 4; ++v) {
          int addr[64];
          for (int lane = 0; lane < 64; ++lane) {
            const int c = v * 16 + (lane >> 2), unit = lane & 3, m = m0 + j * 32 + unit * 8;
            addr[lane] = tq_vt_off(c, unit * 8);
            if (m >= M) continue;
            int val[8];
            for (int e = 0; e < 8; ++e) val[e] = st[tq_vt_off(c, unit * 8) / 2 + e];
            store_unit(img, wave * 64 + c, m, unit & 1, val);
          }
          CHECK(ways(addr, 16) == 1, "tok_qkv V read-back: %d-way", ways(addr, 16));
        }
      }
  img.done();
}

// tok_qkv_small_kernel: (32 tokens, 128 columns) per workgroup, thread = (channel, group of 16): both halves of the group and all its pad
static void vt_tok_qkv_small(int tokens, int B) {
  section = "vt_tok_qkv_small";
  const int M = tokens * B;
  Image img(B, tokens);
  for (int m0 = 0; m0 < M; m0 += 32)
    for (int g = 0; g < 4; ++g)
      for (int tid = 0; tid < 256; ++tid) {
        const int ch = tid & 127, grp = tid >> 7, mg = m0 + grp * 16;
        if (mg >= M) continue;
        CHECK(mg + 16 <= M, "group at row %d reaches past row M", mg);
        int lo[8], hi[8];
        for (int t = 0; t < 16; ++t) (vt_col(t) < 8 ? lo[vt_col(t)] : hi[vt_col(t) - 8]) = 1 + (mg + t) * 512 + g * 128 + ch;
        const int b = vt_group_hyp(mg, tokens), t0 = mg - b * tokens;
        for (int e = 0; e < 8; ++e) img.put(vt_row(b, g * 128 + ch) + t0 + e, lo[e]), img.put(vt_row(b, g * 128 + ch) + t0 + 8 + e, hi[e]);
        if (vt_group_is_last(t0, tokens))
          for (int z = tokens; z < VT_LD; z += 8)
            for (int e = 0; e < 8; ++e) img.put(vt_row(b, g * 128 + ch) + z + e, 0);
      }
  img.done();
}

// the row epilogues' stagings: every (token, column) of the wave's block comes back where the 16-byte stores expect it
static void row_staging() {
  section = "row_staging";
  {                                                              // tok_gemm.hip: 64 rows x 128 columns, rows padded to TG_STAGE_LD halfs
    std::vector<int> st(64 * TG_STAGE_LD, -1);
    for (int j = 0; j < 2; ++j)
      for (int i = 0; i < 4; ++i)
        for (int rg = 0; rg < 4; ++rg) {
          int addr[64];
          for (int lane = 0; lane < 64; ++lane) {
            const int lr = lane & 31, lh = lane >> 5, row = acc_row_token(j, lr), col = acc_row_chan(i, rg, lh);
            for (int e = 0; e < 4; ++e) st[tg_stage_off(row, col) + e] = row * 128 + col + e;
            addr[lane] = tg_stage_off(row, col) * 2;
          }
          CHECK(ways(addr, 8) == 2, "tok_gemm row staging write: %d-way", ways(addr, 8));      // lanes lr, lr + 8: TG_STAGE_LD * 2 * 8 = 0 (mod 128)
        }
    for (int u = 0; u < 16; ++u) {
      int addr[64];
      for (int lane = 0; lane < 64; ++lane) {
        const int px = u * 4 + (lane >> 4), c16 = lane & 15;
        for (int e = 0; e < 8; ++e) CHECK(st[tg_stage_off(px, c16 * 8) + e] == px * 128 + c16 * 8 + e, "row %d column %d", px, c16 * 8 + e);
        addr[lane] = tg_stage_off(px, c16 * 8) * 2;
      }
      CHECK(ways(addr, 16) == 1, "tok_gemm row read-back: %d-way", ways(addr, 16));
    }
  }
  {                                                              // tok_qkv.hip: 32 rows x 64 columns per slice, XOR-ed 16-byte units
    std::vector<int> st(2048, -1);
    for (int i = 0; i < 2; ++i)
      for (int rg = 0; rg < 4; ++rg) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
          const int lr = lane & 31, lh = lane >> 5, col = acc_row_chan(i, rg, lh);
          CHECK(tq_stage_off(lr, col) % 8 == 0 && tq_stage_off(lr, col) + 8 <= 4096, "staging offset");
          for (int e = 0; e < 4; ++e) st[tq_stage_off(lr, col) / 2 + e] = lr * 64 + col + e;
          addr[lane] = tq_stage_off(lr, col);
        }
        CHECK(ways(addr, 8) == 2, "tok_qkv row staging write: %d-way", ways(addr, 8));      // 128-byte rows: rows r, r + 8 (the XOR sees row & 7)
      }
    for (int v = 0; v < 4; ++v) {
      int addr[64];
      for (int lane = 0; lane < 64; ++lane) {
        const int row = v * 8 + (lane >> 3), unit = lane & 7;
        for (int e = 0; e < 8; ++e) CHECK(st[tq_stage_off(row, unit * 8) / 2 + e] == row * 64 + unit * 8 + e, "row %d column %d", row, unit * 8 + e);
        addr[lane] = tq_stage_off(row, unit * 8);
      }
      CHECK(ways(addr, 16) == 1, "tok_qkv row read-back: %d-way", ways(addr, 16));
    }
  }
}

// 6: the group sums (tok_gsum_store): gsum[group][column]
template <int WAVES>
static void group_sums(int M, int tokens) {
  section = "group_sums";
  const int NI = 16 / WAVES;
  for (int g = 0; g * 16 < M; ++g) CHECK(vt_group_hyp(g * 16, tokens) == vt_group_hyp(g * 16 + 15, tokens), "group %d spans two hypotheses", g);
  for (int m0 = 0; m0 < M; m0 += 64) {
    std::vector<int> seen(4 * 512, 0);                           // the tile's 4 groups x 512 columns
    for (int wave = 0; wave < WAVES; ++wave)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 2; ++j)
          for (int i = 0; i < NI; ++i)
            for (int rg = 0; rg < 4; ++rg) {
              const int lr = lane & 31, lh = lane >> 5, g = (m0 + acc_row_token(j, lr & 16)) >> 4;
              if ((lr & 15) != 0 || g * 16 >= M) continue;
              for (int e = 0; e < 4; ++e) ++seen[(g - m0 / 16) * 512 + wave * NI * 32 + acc_row_chan(i, rg, lh) + e];
            }
    for (int n = 0; n < 4 * 512; ++n) CHECK(seen[n] == (m0 + (n / 512) * 16 < M ? 1 : 0), "tile %d group %d column %d written %d times", m0, n / 512, n % 512, seen[n]);
  }
}

int main() {
  // M ragged: the last tile ends inside the tile (the min(m0 + row, M - 1) clamp) - 400 = 6 x 64 + 16 = 3 x 128 + 16
  for (int m0 : {0, 384}) {
    tile<64, 4>(m0, 400), tile<64, 8>(m0, 400), tile<128, 8>(m0, 400);
    ring(m0, 400);
  }
  tile<64, 4>(64, 65), tile<128, 8>(0, 1);
  in_place<64, 4>(), in_place<64, 8>(), in_place<128, 8>();
  weights();
  vt_order();
  for (int tokens : {16, 400, 416})
    for (int B : {1, 3}) vt_tok_gemm(tokens, B), vt_tok_qkv(tokens, B), vt_tok_qkv_small(tokens, B);
  row_staging();
  for (int M : {16, 400, 1200}) group_sums<4>(M, M < 400 ? 16 : 400), group_sums<8>(M, M < 400 ? 16 : 400);
  printf("ok\n");
  return 0;
}
'''


@pytest.fixture(scope='module')
def result(tmp_path_factory):
  """The compiler beside the hipcc the Makefile names (ROCm's clang++), on tok_tile.h alone."""
  hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC \?= (\S+)', open(os.path.join(CSRC, 'Makefile')).read(), flags=re.M).group(1)
  cxx = os.path.join(os.path.dirname(hipcc), 'amdclang++')
  d = tmp_path_factory.mktemp('tok_tile')
  src, exe = d / 'tok.cc', d / 'tok'
  src.write_text(PROGRAM)
  subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, str(src), '-o', str(exe)], check=True)
  return subprocess.run([str(exe)], capture_output=True, text=True)


def test_reads_address_what_the_fills_put_there(result):
  assert result.returncode == 0 and result.stdout == 'ok\n', result.stdout + result.stderr
