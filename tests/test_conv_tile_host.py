"""CPU: the index rules of the 3x3 halo kernels and the generic implicit GEMM (foundationpose_amd/csrc/conv_tile.h), checked exhaustively by a
stand-alone program that is compiled against the header alone - no HIP, no GPU.  The program restates only the kernels' constants, their
loop structure (which wave issues which DMA instruction, in which order) and literal versions of the rules it checks the header against;
the rules come from the header the kernels compile.

Sizes: W = 40 and 20, tiles of NT = 1 .. 4 x 128 pixels at every tile start m0 = 128 k (NT = 1, 2, 3: the tail tiles, which start at
512 a + 128 nt b) or 512 k (NT = 4) of batches of 1, 2, 3, 9 and, at W = 20, 32 images.  9 images are 112 starts of 128 and 28 of 512 at
W = 40 and 28 starts of 128 at W = 20, 32 images 25 starts of 512 at W = 20: each more than one period (25) of the start modulo an image;
1 .. 3 images: tiles that cross image boundaries, a ragged last tile.  Cin / 32 = 4, 8, 16 chunks with 2, 4, 8 shares.

Every check is of the form "what a read addresses is what the fill put there".  Sections (a failure names its section):
  band        every valid tap of every pixel < M reads an entry that a DMA of this chunk filled with that input pixel of the same image, in
              the channel group the fragment expects, from an UNCLAMPED source; every other tap reads the zero chunk; every index < NB <= BPX
  lds         zero chunk and weight buffers behind the bands, the staging tile inside LDS_BYTES, the 128-pixel tile's LDS inside the 512's
  weights     the 24 stage instructions of a kernel row land each (co, kx, channel group) once, where the A-fragment read takes it from; the
              same for igemm2's weight and pixel instructions at BM = 64 and 128
  banks       ways() of test_tok_tile_host.py (four contiguous 16-lane quarters) over the band reads (zero-chunk lanes included), weight
              reads, staging writes and reads; every 16-byte read also in the lane groups the hardware documentation gives for
              ds_read_b128 ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32)
  waits       one wave's in-order vector-memory queue replayed over the halo loop (1, 2, 4, 8, 16 chunks; 2, 4, 8 split-K shares) and igemm2's ring
              (nk = 1, 2, 3, 16; NT = 1, 4): what must have landed is older than the youngest *_wait_allowed() operations, and the count
              is tight; the slot refilled in step kt was last read in step kt - 1
  epilogue    staging slots of different lanes are disjoint and cover the tile; row pieces cover it once (NOUT = 12 at NT = 3)
  placement   against a literal restatement, tiles below, above and across split_m
  grids       main, tail and split-K maps cover every (pixel tile, cout tile[, share]) once, for halo_plan / halo_split outputs

What the test found (conv_tile.h and DESIGN.md say so now):
  * the band's fragment reads are conflict free at every tile alignment and tap shift, as the old comment said, in the contiguous quarters
    of the model and in the documented ds_read_b128 groups alike (either way a group is 16 rows with 16 different row mod 16), as long
    as all 16 lanes read band entries.  The comment did not count the border lanes: they read the one zero chunk, one more address in one bank
    group, and a read with border lanes is two-way more often than not (the program prints the counts; never more than two-way);
  * "what lands for rows outside the tensor is never read" holds for pixels < M.  The lanes of a ragged last tile whose pixel is >= M carry
    the validity bits of pixel M - 1 at their own band position and may read entries whose source was clamped; their sums are never stored;
  * both wait rules are safe and tight at every barrier: no slack to state;
  * the 16-byte staging reads are conflict free at BM = 128 and two-way at BM = 64 (two rows per quarter, 144 bytes apart) in the model;
    in the documented groups both are two-way (a group takes lanes of two rows).  The 8-byte staging writes are two-way, like those of
    tok_tile.h (ds_write_b64 is served in contiguous quarters).
Pieces the two MFMA kernels keep written out (comments there, profiles/conv_tile_isa.md) are checked through the header's statement of the
same rule; the kernels' own text is pinned by test_gpu_kernels.py::test_conv_kernels_bits_are_the_recorded_ones."""
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
#include <map>
#include <tuple>
#include <vector>
#include "conv_tile.h"

#define CHECK(c, ...) do { if (!(c)) { printf("FAILED %s:%d %s: ", section, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)
static const char *section = "";
const ConvKnobs &conv_knobs() { static const ConvKnobs k; return k; }

// most DIFFERENT addresses that the lanes of a 16-lane quarter name in one bank group (1: conflict free); unit 16: ds_read_b128, 8:
// ds_write_b64.  The model of test_tok_tile_host.py's ways(); that one counts lanes, which is the same number as long as no two lanes of a
// quarter name the same address - here the border lanes all read the one zero chunk (a broadcast), so addresses are counted once.
static int ways_in(const int (&addr)[64], int unit, const int (&group)[4][16]) {
  int worst = 0;
  for (int q = 0; q < 4; ++q)
    for (int a = 0; a < 16; ++a) {
      int n = 1;
      for (int b = 0; b < 16; ++b) {
        const int x = addr[group[q][a]], y = addr[group[q][b]];
        CHECK(x % unit == 0, "address %d", x);
        bool first = x != y && (x / unit) % 16 == (y / unit) % 16;
        for (int c = 0; c < b; ++c) first &= addr[group[q][c]] != y;
        if (first) ++n;
      }
      if (n > worst) worst = n;
    }
  return worst;
}
// the earlier tests' model: four contiguous quarters (what the hardware does for ds_write_b64)
static const int QUARTERS[4][16] = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31},
                                    {32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47}, {48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63}};
// the lane groups the hardware documentation gives for ds_read_b128 (bank (a / 4) mod 64: the same 16 slots of 16 bytes)
static const int B128_GROUPS[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                       {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59}, {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
static int ways(const int (&addr)[64], int unit) { return ways_in(addr, unit, QUARTERS); }
static int ways_hw(const int (&addr)[64]) { return ways_in(addr, 16, B128_GROUPS); }      // a 16-byte read in the documented groups
static int imin(int a, int b) { return a < b ? a : b; }
template <class M, class K> static int at_or(const M &m, const K &k) { auto it = m.find(k); return it == m.end() ? -1 : it->second; }      // the half offset a piece landed at

struct Held { int gp, chunk; bool filled, clamped; };
static int band_ways_seen[2][3], band_ways_hw_seen[2][3];      // [some lane reads the zero chunk][ways], contiguous quarters / documented groups

template <int W, int NT>
static void band(int Nimg) {
  constexpr int TM = 128 * NT, PXW = 32 * NT;
  using C = HaloCfgD<W, TM>;
  static_assert(C::NB <= C::BPX, "band fits");
  const int M = Nimg * W * W, hpix_max = Nimg * W * W - 1;
  for (int m0 = 0; m0 < M; m0 += (NT < 4 ? 128 : 512)) {      // every start a tail tile (128 k) or a main tile (512 k) can have
    section = "band";
    const int GR0 = hl_gr0(m0, W);
    std::vector<Held> lds(C::BPX * 4, Held{0, 0, false, false});
    for (int wave = 0; wave < 8; ++wave)
      for (int h = 0; h < C::HQ; ++h)
        for (int lane = 0; lane < 64; ++lane) {
          const int slot = ct_dma_slot(h, 8, wave), P = ct_dma_row(slot, lane);
          const int gp = hl_band_src(GR0, W, P, hpix_max), pos = ct_dma_lds(slot) + 8 * lane;
          CHECK(pos >= 0 && pos / 8 < C::BPX * 4 && !lds[pos / 8].filled, "DMA destination %d", pos);
          CHECK(pos == ct_off(P, ct_dma_chunk(P, lane) * 8), "lane-linear destination %d is not the stored place of (row %d, chunk %d)", pos, P, ct_dma_chunk(P, lane));
          lds[pos / 8] = Held{gp, ct_dma_chunk(P, lane), true, gp != hl_band_pixel(GR0, W, P)};
        }
    for (int wn = 0; wn < 4; ++wn)
      for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx)
          for (int ks = 0; ks < 2; ++ks)
            for (int j = 0; j < NT; ++j) {
              int addr[64];
              for (int lane = 0; lane < 64; ++lane) {
                const int lr = lane & 31, lh = lane >> 5;
                const int m = m0 + wn * PXW + acc_row_token(j, lr), mc = imin(m, M - 1);
                const int gr = mc / W, ox = mc - gr * W, oy = gr % W, n = gr / W;
                const bool ok = hl_tap_valid(oy, ox, W, ky, kx);
                CHECK(ok == (oy + ky - 1 >= 0 && oy + ky - 1 < W && ox + kx - 1 >= 0 && ox + kx - 1 < W), "validity");
                const int pb = hl_pb(m0 + wn * PXW + lr, GR0, W);
                const int off = ct_frag(hl_tap(pb, W, ky, kx), ks, lh) + j * CT_TILE32;
                for (int hb = 0; hb < 2; ++hb) CHECK(hl_zero_base<C>(hb, j * CT_TILE32) + j * CT_TILE32 + hb * C::HBUF_HALFS == C::ZERO_OFF, "zero chunk select");
                addr[lane] = (ok ? off : C::ZERO_OFF) * 2;
                if (!ok) continue;
                CHECK(off >= 0 && off / 32 < C::NB && off % 8 == 0, "band index %d of %d", off / 32, C::NB);
                if (m >= M) continue;                              // ragged tile: the lane's pixel does not exist, its sums are never stored
                const Held &e = lds[off / 8];
                const int want = (n * W + oy + ky - 1) * W + ox + kx - 1;
                CHECK(e.filled && !e.clamped, "pixel %d tap (%d, %d): entry %d %s", m, ky, kx, off / 32, e.filled ? "has a clamped source" : "was never filled");
                CHECK(e.gp == want && e.chunk == ks * 2 + lh, "pixel %d tap (%d, %d) k-step %d half %d reads input pixel %d chunk %d, wanted %d chunk %d", m, ky, kx, ks, lh, e.gp, e.chunk, want, ks * 2 + lh);
              }
              section = "banks";
              const int wy = ways(addr, 16), wh = ways_hw(addr);
              CHECK(wy <= 2 && wh <= 2, "band read: %d-way, %d-way in the documented groups", wy, wh);
              bool any_zero = false;
              for (int lane = 0; lane < 64; ++lane) any_zero |= addr[lane] == C::ZERO_OFF * 2;
              ++band_ways_seen[any_zero][wy], ++band_ways_hw_seen[any_zero][wh];
              if (!any_zero) CHECK(wy == 1 && wh == 1, "band read without border lanes: %d-way, %d-way in the documented groups", wy, wh);
              section = "band";
            }
  }
  section = "lds";
  CHECK(C::ZERO_OFF >= 2 * C::HBUF_HALFS && C::WBUF_OFF >= C::ZERO_OFF + 8 && C::WBUF_OFF % 8 == 0, "zero chunk / weights behind the bands");
  CHECK(C::LDS_HALFS_MAIN == C::WBUF_OFF + 2 * 3 * HL_BM * HL_CK && C::LDS_BYTES >= 2 * C::LDS_HALFS_MAIN && C::LDS_BYTES >= 2 * TM * HL_SLD, "extent");
  CHECK((HaloCfgD<W, 128>::LDS_BYTES) <= (HaloCfgD<W, 512>::LDS_BYTES) && C::LDS_BYTES <= 160 * 1024, "tail tiles in the main tile's LDS");
}

static void weights() {
  section = "weights";
  const int Cin = 256, Kpad = 9 * Cin, c0 = 128, ky = 2, cc = 3;
  std::map<std::tuple<int, int, int>, int> at;                     // (co, kx, chunk) -> half offset
  for (int q = 0; q < HL_WSLOTS / 8; ++q)
    for (int wave = 0; wave < 8; ++wave)
      for (int lane = 0; lane < 64; ++lane) {
        const int g0 = q * 8, g = g0 + wave;
        const size_t src = hl_w_src(c0, g0, ky, cc, Kpad, Cin) + ct_w_off(wave, lane, Kpad) / 2;
        const int co = (int)(src / Kpad) - c0, k = (int)(src % Kpad), kx = k / Cin - ky * 3, ch = (k % Cin - cc * HL_CK) / 8;
        CHECK(co >= 0 && co < HL_BM && kx >= 0 && kx < 3 && ch >= 0 && ch < 4 && k % 8 == 0, "slot %d lane %d fetches co %d kx %d chunk %d", g, lane, co, kx, ch);
        CHECK(co == hl_w_row(g) + lane / 4 && kx == hl_w_kx(g), "slot %d holds rows %d .. of tap %d", g, hl_w_row(g), hl_w_kx(g));
        const bool fresh = at.insert({std::make_tuple(co, kx, ch), ct_dma_lds(g) + 8 * lane}).second;
        CHECK(fresh, "(%d, %d, %d) landed twice", co, kx, ch);
      }
  CHECK((int)at.size() == HL_BM * 3 * 4, "%d pieces", (int)at.size());
  for (int wm = 0; wm < 2; ++wm)
    for (int kx = 0; kx < 3; ++kx)
      for (int ks = 0; ks < 2; ++ks)
        for (int i = 0; i < 2; ++i) {
          int addr[64];
          for (int lane = 0; lane < 64; ++lane) {
            const int lr = lane & 31, lh = lane >> 5, off = ct_frag(wm * 64 + lr, ks, lh) + i * CT_TILE32 + hl_w_tap(kx);
            CHECK(at_or(at, std::make_tuple(wm * 64 + i * 32 + lr, kx, ks * 2 + lh)) == off, "A fragment of co %d tap %d k-step %d half %d at %d", wm * 64 + i * 32 + lr, kx, ks, lh, off);
            addr[lane] = off * 2;
          }
          section = "banks";
          CHECK(ways(addr, 16) == 1 && ways_hw(addr) == 1, "weight read: %d-way, %d-way in the documented groups", ways(addr, 16), ways_hw(addr));
          section = "weights";
        }
  for (int BM : {64, 128})                                         // igemm2: weights (linear form) and pixels (gather form), one stage
    for (int NT : {1, 4}) {
      const int WM = BM / 2, kt = 5, Kp = 1024;
      std::map<std::pair<int, int>, int> wat, xat;
      for (int wave = 0; wave < 4; ++wave)
        for (int lane = 0; lane < 64; ++lane) {
          for (int q = 0; q < c2_wq(BM); ++q) {
            const size_t src = (size_t)(q * 64) * Kp + (size_t)kt * C2_BK + ct_w_off(wave, lane, Kp) / 2;
            const int slot = ct_dma_slot(q, 4, wave);
            CHECK((int)(src / Kp) == ct_dma_row(slot, lane) && (int)(src % Kp) - kt * C2_BK == 8 * ct_dma_chunk(ct_dma_row(slot, lane), lane), "weight slot %d lane %d", slot, lane);
            const bool fresh = wat.insert({std::make_pair((int)(src / Kp), ((int)(src % Kp) - kt * C2_BK) / 8), ct_dma_lds(slot) + 8 * lane}).second;
            CHECK(fresh, "twice");
          }
          for (int q = 0; q < NT; ++q) {
            const int slot = ct_dma_slot(q, 4, wave), px = ct_dma_row(slot, lane);
            const bool fresh = xat.insert({std::make_pair(px, ct_dma_chunk(px, lane)), ct_dma_lds(slot) + 8 * lane}).second;
            CHECK(fresh, "twice");
          }
        }
      CHECK((int)wat.size() == BM * 4 && (int)xat.size() == 64 * NT * 4 && c2_dmaw(NT, BM) == NT + BM / 64, "stage of %d + %d rows", BM, 64 * NT);
      CHECK(c2_stage_halfs(NT, BM) == (64 * NT + BM) * C2_BK && c2_lds_bytes(BM) >= 3 * c2_stage_halfs(4, BM) * 2 && c2_lds_bytes(BM) >= C2_BN * ct_stage_ld(BM) * 2, "LDS");
      for (int wave = 0; wave < 4; ++wave)
        for (int ks = 0; ks < 2; ++ks) {
          const int wm = wave >> 1, wn = wave & 1;
          for (int i = 0; i < WM / 32; ++i) {
            int addr[64];
            for (int lane = 0; lane < 64; ++lane) {
              const int lr = lane & 31, lh = lane >> 5, off = ct_frag(wm * WM + lr, ks, lh) + i * CT_TILE32;
              CHECK(at_or(wat, std::make_pair(wm * WM + i * 32 + lr, ks * 2 + lh)) == off, "igemm2 A fragment");
              addr[lane] = off * 2;
            }
            section = "banks";
            CHECK(ways(addr, 16) == 1 && ways_hw(addr) == 1, "igemm2 weight read: %d-way, %d-way in the documented groups", ways(addr, 16), ways_hw(addr));
            section = "weights";
          }
          for (int j = 0; j < NT; ++j) {
            int addr[64];
            for (int lane = 0; lane < 64; ++lane) {
              const int lr = lane & 31, lh = lane >> 5, px = wn * (32 * NT) + acc_row_token(j, lr), off = ct_frag(px, ks, lh);
              CHECK(at_or(xat, std::make_pair(px, ks * 2 + lh)) == off, "igemm2 B fragment");
              addr[lane] = off * 2;
            }
            section = "banks";
            CHECK(ways(addr, 16) == 1 && ways_hw(addr) == 1, "igemm2 pixel read: %d-way, %d-way in the documented groups", ways(addr, 16), ways_hw(addr));
            section = "weights";
          }
        }
    }
}

// one wave's in-order vector-memory queue: ids of the operations issued so far; `need` = the youngest that must have landed
struct Queue {
  std::vector<int> ops;
  void issue(int id, int n) { for (int i = 0; i < n; ++i) ops.push_back(id); }
  int younger_than_last(int id) const {                            // operations behind the last one with this id (-1: none issued)
    for (int i = (int)ops.size() - 1; i >= 0; --i) if (ops[i] == id) return (int)ops.size() - 1 - i;
    return -1;
  }
};
static void waits() {
  section = "waits";
  for (int NT = 1; NT <= 4; ++NT)
    for (int HQ : {HaloCfgD<40, 128>::HQ, HaloCfgD<40, 512>::HQ, HaloCfgD<20, 128>::HQ, HaloCfgD<20, 384>::HQ, HaloCfgD<20, 512>::HQ})
      for (int call : {1, 2, 4, 8, 16})
        for (int ksplit : {1, 2, 4, 8}) {
          if (call % ksplit) continue;
          const int WQ = HL_WSLOTS / 8, NV = 6 * NT;
          if (WQ + HQ > NV) continue;                              // (the kernel's static_assert: not an instantiation)
          for (int ks = 0; ks < ksplit; ++ks) {
            const int cbeg = ks * (call / ksplit), nchunk = cbeg + call / ksplit;
            Queue q;                                               // ids: band of chunk c = 1000 + c, weights of group g = g
            q.issue(1000 + cbeg, HQ);
            q.issue(0, WQ);
            int g = 0;
            for (int cc = cbeg; cc < nchunk; ++cc)
              for (int ky = 0; ky < 3; ++ky, ++g) {
                const int allowed = halo_wait_allowed(ky, cc + 1 < nchunk, HQ);
                int younger = q.younger_than_last(g);
                CHECK(younger >= 0, "weights of group %d never issued", g);
                if (ky == 0) {
                  const int yb = q.younger_than_last(1000 + cc);
                  CHECK(yb >= 0, "band of chunk %d never issued", cc);
                  if (yb < younger) younger = yb;
                }
                CHECK(allowed <= younger, "chunk %d ky %d: vmcnt(%d) leaves a needed operation in flight (%d younger ones)", cc, ky, allowed, younger);
                CHECK(allowed == younger, "chunk %d ky %d: vmcnt(%d) is not tight, %d operations are younger than what is needed", cc, ky, allowed, younger);
                const bool more_w = !(ky == 2 && cc + 1 >= nchunk), more_h = ky == 0 && cc + 1 < nchunk;
                for (int t = 0; t < NV; ++t) {
                  CHECK(!(hl_visit_is_w(t, WQ) && hl_visit_is_band(t, WQ, HQ)), "visit %d issues both", t);
                  if (hl_visit_is_w(t, WQ) && more_w) q.issue(g + 1, 1);
                  if (hl_visit_is_band(t, WQ, HQ) && more_h) q.issue(1000 + cc + 1, 1);
                }
              }
          }
        }
  for (int BM : {64, 128})
    for (int NT : {1, 4})
      for (int nk : {1, 2, 3, 16}) {
        const int DMAW = c2_dmaw(NT, BM);
        Queue q;
        q.issue(0, DMAW);
        if (nk > 1) q.issue(1, DMAW);
        for (int kt = 0; kt < nk; ++kt) {
          const int allowed = c2_wait_allowed(kt, nk, DMAW), younger = q.younger_than_last(kt);
          CHECK(younger >= 0 && allowed <= younger, "ring step %d of %d: vmcnt(%d), %d younger", kt, nk, allowed, younger);
          CHECK(allowed == younger, "ring step %d of %d: vmcnt(%d) is not tight (%d)", kt, nk, allowed, younger);
          if (kt + 2 < nk) {
            CHECK(c2_slot(kt + 2) != c2_slot(kt) && c2_slot(kt + 2) != c2_slot(kt + 1) && (kt == 0 || c2_slot(kt + 2) == c2_slot(kt - 1)), "slot of stage %d", kt + 2);
            q.issue(kt + 2, DMAW);
          }
        }
      }
}

static void epilogue() {
  for (int form = 0; form < 2; ++form)                             // 0: halo (8 waves as 2 x 4, NTH 512), 1: igemm2 (4 waves as 2 x 2, NTH 256)
    for (int BM : {64, 128})
      for (int NT = 1; NT <= 4; ++NT) {
        if (form == 0 && BM != HL_BM) continue;
        if (form == 1 && NT != 1 && NT != 4) continue;
        section = "epilogue";
        const int NPW = form == 0 ? 4 : 2, NTH = 128 * NPW, TM = 32 * NT * NPW, WM = BM / 2, ld = ct_stage_ld(BM);
        CHECK(form == 1 || ld == HL_SLD, "HL_SLD");
        std::vector<int> quad(TM * BM / 4, 0);
        for (int wave = 0; wave < 2 * NPW; ++wave)
          for (int j = 0; j < NT; ++j)
            for (int i = 0; i < WM / 32; ++i)
              for (int rg = 0; rg < 4; ++rg) {
                int addr[64];
                for (int lane = 0; lane < 64; ++lane) {
                  const int wm = wave / NPW, wn = wave % NPW, lr = lane & 31, lh = lane >> 5;
                  const int pxl = wn * (32 * NT) + acc_row_token(j, lr), col = wm * WM + acc_row_chan(i, rg, lh);
                  const int off = ct_stage_off(BM, pxl, col);          // the slot the lane reads the residual from and writes its result to
                  CHECK(off == pxl * (BM + 8) + col && pxl < TM && col + 4 <= BM && col % 4 == 0, "slot of pixel %d column %d", pxl, col);
                  ++quad[pxl * (BM / 4) + col / 4];
                  addr[lane] = off * 2;
                }
                section = "banks";
                CHECK(ways(addr, 8) == 2, "staging write: %d-way", ways(addr, 8));      // lanes lr, lr + 8: 8 rows of BM + 8 halfs = 0 (mod 128 bytes)
                section = "epilogue";
              }
        for (int x : quad) CHECK(x == 1, "an 8-byte slot has %d owners", x);
        const int NOUT = TM * (BM / 8) / NTH;
        CHECK(NOUT * NTH == TM * (BM / 8) && (form == 1 || NT != 3 || NOUT == 12), "row pieces per thread %d", NOUT);
        std::vector<int> piece(TM * (BM / 8), 0);
        for (int u = 0; u < NOUT; ++u)
          for (int w = 0; w < NTH / 64; ++w) {
            int addr[64];
            for (int lane = 0; lane < 64; ++lane) {
              const int idx = w * 64 + lane + NTH * u, px = ct_piece_px(idx, BM), c16 = ct_piece_c16(idx, BM);
              CHECK(px < TM && c16 < BM / 8, "piece %d", idx);
              ++piece[px * (BM / 8) + c16];
              addr[lane] = ct_stage_off(BM, px, c16 * 8) * 2;
            }
            section = "banks";
            // BM 128: a quarter is one row's 16 pieces.  BM 64: two rows of 8 pieces, 144 bytes apart: one pair of lanes meets
            CHECK(ways(addr, 16) == (BM == 128 ? 1 : 2), "staging read: %d-way", ways(addr, 16));
            // in the documented groups both are two-way: lanes 0-3, 12-15 of one row meet lanes 20-27 of the next, 272 / 144 bytes on
            CHECK(ways_hw(addr) == 2, "staging read: %d-way in the documented groups", ways_hw(addr));
            section = "epilogue";
          }
        for (int x : piece) CHECK(x == 1, "a row piece leaves %d times", x);
      }
  section = "placement";
  const int out_ld = 256, coff_hi = 128;
  for (int split_m : {0x7fffffff, 4800, 4700, 0})                  // none; on a tile boundary; inside a tile; everything above
    for (int m = 0; m < 9600; ++m) {
      const long long lit = m >= split_m ? (long long)(m - split_m) * out_ld + coff_hi : (long long)m * out_ld;
      CHECK(ct_out_row(m, split_m) * out_ld + ct_out_col(m, split_m, coff_hi) == lit, "row %d with split_m %d", m, split_m);
    }
  CHECK(ct_splitk_index(3, 17, 40, 1200, 512) == ((size_t)3 * 1200 + 17) * 512 + 40, "split-K scratch [ks][m][Cout]");
}

static void grids() {
  section = "grids";
  const int cases[][3] = {{3, 40, 128}, {37, 40, 128}, {83, 40, 128}, {42, 40, 256}, {2, 40, 256}, {3, 20, 512}, {6, 20, 512}, {32, 20, 512}, {50, 20, 512}, {63, 20, 512}, {83, 20, 512}, {252, 40, 256}};
  for (const auto &c : cases) {
    const int M = c[0] * c[1] * c[1], n_ct = c[2] / HL_BM, qm = (M + 127) / 128;
    int n_main, nt_tail, n_tail;
    halo_plan(M, n_ct, 256, conv_knobs(), &n_main, &nt_tail, &n_tail);
    std::vector<int> seen(qm * n_ct, 0);
    auto mark = [&](CtTile t, int nq) {
      CHECK(t.m0 % 128 == 0 && t.c0 % HL_BM == 0 && t.c0 / HL_BM < n_ct, "tile (%d, %d)", t.m0, t.c0);
      for (int k = 0; k < nq; ++k) if (t.m0 + 128 * k < M) ++seen[(t.m0 / 128 + k) * n_ct + t.c0 / HL_BM];
    };
    for (int L = 0; L < n_main; ++L) mark(ct_grid_main(L, n_ct, 512, HL_BM), 4);
    for (int t = 0; t < n_tail; ++t) mark(hl_grid_tail(t, n_main, n_ct, nt_tail), nt_tail);
    for (int x : seen) CHECK(x == 1, "halo %d x %dx%d x %d: a tile computed %d times (n_main %d, %d tails of %d)", c[0], c[1], c[1], c[2], x, n_main, n_tail, nt_tail);
    for (int ksplit : {2, 4, 8}) {
      std::vector<int> s2(qm * n_ct * ksplit, 0);
      for (int b = 0; b < qm * n_ct * ksplit; ++b) {
        const CtTile t = ct_grid_split(b, ksplit, n_ct, 128, HL_BM);
        CHECK(t.m0 < M && t.ks < ksplit, "share");
        ++s2[(t.m0 / 128 * n_ct + t.c0 / HL_BM) * ksplit + t.ks];
      }
      for (int x : s2) CHECK(x == 1, "split-K share computed %d times", x);
    }
    for (int BM : {64, 128}) {                                       // igemm2 on the same sizes: 256-pixel tiles, the last ones in quarters
      const int nc = c[2] / BM, n_tiles = ((M + C2_BN - 1) / C2_BN) * nc, q64 = (M + 63) / 64;
      int nm, nt4;
      halo_split(n_tiles, 512, conv_knobs(), &nm, &nt4);
      std::vector<int> s3(q64 * nc, 0);
      auto mark2 = [&](CtTile t, int nq) {
        for (int k = 0; k < nq; ++k) if (t.m0 + 64 * k < M) ++s3[(t.m0 / 64 + k) * nc + t.c0 / BM];
      };
      for (int L = 0; L < nm; ++L) mark2(ct_grid_main(L, nc, C2_BN, BM), 4);
      for (int t = 0; t < nt4; ++t) mark2(c2_grid_tail(t, nm, nc, BM), 1);
      for (int x : s3) CHECK(x == 1, "igemm2 BM %d: a tile computed %d times", BM, x);
    }
  }
}

int main() {
  for (int Nimg : {1, 2, 3, 9, 32}) {                            // 9 x 1600 = 28 x 512, 32 x 400 = 25 x 512: a whole period of the 512-pixel starts too
    if (Nimg <= 9) band<40, 1>(Nimg), band<40, 2>(Nimg), band<40, 3>(Nimg), band<40, 4>(Nimg);
    band<20, 1>(Nimg), band<20, 2>(Nimg), band<20, 3>(Nimg), band<20, 4>(Nimg);
  }
  section = "banks";
  printf("band reads: without border lanes %d 1-way %d 2-way, with border lanes %d 1-way %d 2-way\n", band_ways_seen[0][1], band_ways_seen[0][2], band_ways_seen[1][1], band_ways_seen[1][2]);
  printf("band reads, documented groups: without border lanes %d 1-way %d 2-way, with border lanes %d 1-way %d 2-way\n", band_ways_hw_seen[0][1], band_ways_hw_seen[0][2], band_ways_hw_seen[1][1], band_ways_hw_seen[1][2]);
  CHECK(band_ways_hw_seen[0][1] > 0 && band_ways_hw_seen[0][2] == 0 && band_ways_hw_seen[1][1] > 0, "band reads in the documented groups");
  CHECK(band_ways_seen[0][1] > 0 && band_ways_seen[0][2] == 0 && band_ways_seen[1][1] > 0, "band reads");
  weights();
  waits();
  epilogue();
  grids();
  printf("ok\n");
  return 0;
}
'''


def build_and_run(tmp, header_dir=CSRC, flags=()):
  """The compiler beside the hipcc the Makefile names (ROCm's clang++), on conv_tile.h (and conv_plan.h / tok_tile.h, which it includes) alone."""
  hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC \?= (\S+)', open(os.path.join(CSRC, 'Makefile')).read(), flags=re.M).group(1)
  cxx = os.path.join(os.path.dirname(hipcc), 'amdclang++')
  src, exe = tmp / 'conv_tile.cc', tmp / 'conv_tile'
  src.write_text(PROGRAM)
  subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', *flags, '-I', str(header_dir), str(src), '-o', str(exe)], check=True)
  return subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.fixture(scope='module')
def result(tmp_path_factory):
  return build_and_run(tmp_path_factory.mktemp('conv_tile'))


def test_reads_address_what_the_fills_put_there(result):
  assert result.returncode == 0 and result.stdout.endswith('ok\n'), result.stdout + result.stderr


def test_band_reads_are_conflict_free_but_for_the_zero_chunk(result):
  """What the bank model finds, as the program prints it: every fragment read of band entries alone is 1-way at every alignment and tap
  shift; a read whose border lanes take the zero chunk is 1-way or 2-way (the zero chunk sits in one bank group, which a band lane of
  the same quarter may also use), never more."""
  m = re.search(r'band reads: without border lanes (\d+) 1-way (\d+) 2-way, with border lanes (\d+) 1-way (\d+) 2-way', result.stdout)
  assert m, result.stdout
  p1, p2, z1, z2 = map(int, m.groups())
  assert p1 > 0 and p2 == 0 and z1 > 0 and z2 > 0, m.group(0)
  m = re.search(r'band reads, documented groups: without border lanes (\d+) 1-way (\d+) 2-way, with border lanes (\d+) 1-way (\d+) 2-way', result.stdout)
  assert m, result.stdout
  p1, p2, z1, z2 = map(int, m.groups())
  assert p1 > 0 and p2 == 0 and z1 > 0 and z2 > 0, m.group(0)
