"""CPU: the index rules of the band convolution kernels (foundationpose_amd/csrc/conv_band.h), checked exhaustively by a stand-alone program
that is compiled against the header alone - no HIP, no GPU - over the geometries of conv_s2.hip, conv_s1b.hip, stem.hip and front.hip (the
constants below restate S2Cfg<20, 8, .>, the B1_*, ST_* and FR_* defines; the rules themselves come from the header the kernels compile).

Every check is of the form "the LDS position a read addresses is the position the fill put that input pixel at": the fill side is the DMA map
(instruction, lane) -> (slot, logical half) -> input pixel, or front.hip's register-side write; the read side is the pixel's base slot, the tap
rule and the half swizzle.  A B read is conflict free when, within each 16-lane quarter of a ds_read_b128, two lanes either name the same
address (a broadcast: front.hip's clamped tail pixels) or differ in their 16-byte bank group - for distinct addresses that is the file
comments' "all 64 banks once".  One claim did not hold and its comment is corrected: in a conv_s2 tile that straddles two images, the
quarter of a read that holds pixels of both is not conflict free (the zero row between the images shifts the banks); lanes of one image are."""
import os
import re
import subprocess

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CSRC = os.path.join(REPO, 'foundationpose_amd', 'csrc')

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "conv_band.h"

#define CHECK(c, ...) do { if (!(c)) { printf("FAILED %s:%d %s: ", section, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)
static const char *section = "";

struct Held { bool filled, ok; int img, iy, ix, half, plane; };      // what a 16-byte LDS position holds after the fill

// the 16 lanes of each quarter of a B read: same address or different 16-byte bank group.  `part`: lanes of different parts are not
// compared (conv_s2.hip: the two images of a straddling tile)
static void check_banks(const int (&addr)[64], const int *part = nullptr) {
  for (int q = 0; q < 4; ++q)
    for (int a = 0; a < 16; ++a)
      for (int b = a + 1; b < 16; ++b) {
        const int x = addr[q * 16 + a], y = addr[q * 16 + b];
        if (part && part[q * 16 + a] != part[q * 16 + b]) continue;
        CHECK(x % 16 == 0 && (x == y || (x >> 4) % 16 != (y >> 4) % 16), "lanes %d, %d of quarter %d: bytes %d, %d", a, b, q, x, y);
      }
}

// conv_s2.hip: WO = 20, ROWS = 8, P = 42, 18 band rows, 24 DMA instructions; tiles start at flattened output row g0 = 8 pt, so oy0 = g0 % 20;
// every oy0 is walked (jb = 20 - oy0 takes every value from 1 to 20; >= 8: no straddle)
static void conv_s2() {
  section = "conv_s2";
  const int WO = 20, ROWS = 8, P = 42, BROWS = 18, INSTR = 24, HI = 40;
  for (int oy0 = 0; oy0 < WO; ++oy0)
    for (int n_img = 1; n_img <= 2; ++n_img) {                          // the tile's first image is the last one / is not
      const int jb = WO - oy0;
      std::vector<Held> lds(INSTR * 64, Held{});
      for (int u = 0; u < INSTR; ++u)
        for (int l = 0; l < 64; ++l) {
          const int q = band_dma_slot(u, l);
          const BandSrc s = s2_band_src(P, WO, BROWS, oy0, jb, n_img, q);
          lds[u * 64 + l] = Held{true, s.ok, s.img, s.iy, s.ix, band_dma_half(q, l), 0};
        }
      for (int t = 0; t < 9; ++t)
        for (int j = 0; j < ROWS * WO / 32; ++j) {
          int addr[64], image[64];
          for (int lane = 0; lane < 64; ++lane) {
            const int lr = lane & 31, lh = lane >> 5, pl = 32 * j + lr, jr = pl / WO, ox = pl - jr * WO, ky = t / 3, kx = t % 3;
            const int x = band_swizzle(band_addr(s2_tile_row(jr, jb) * P + ox, lh) + (s2_tap_slots(P, WO, ky, kx) << 5));
            addr[lane] = x, image[lane] = jr >= jb;
            const int img = jr >= jb ? 1 : 0, oy = jr >= jb ? jr - jb : oy0 + jr, iy = 2 * oy + ky - 1, ix = 2 * ox + kx - 1;
            const bool inside = iy >= 0 && iy < HI && ix >= 0 && ix < HI && img < n_img;
            CHECK(x >= 0 && x / 16 < INSTR * 64, "read past the band: %d", x);
            const Held &h = lds[x / 16];
            CHECK(h.filled && h.ok == inside, "oy0 %d pixel %d tap %d: inside %d, held %d", oy0, pl, t, inside, h.ok);
            if (inside) CHECK(h.img == img && h.iy == iy && h.ix == ix && h.half == lh, "oy0 %d pixel %d tap %d half %d: holds (%d, %d, %d, %d)", oy0, pl, t, lh, h.img, h.iy, h.ix, h.half);
          }
          // the zero row between two images shifts the second one's rows by P = 10 (mod 16) slots: only lanes of one image are conflict free
          check_banks(addr, image);
        }
    }
}

// conv_s1b.hip: 40x40 maps, 8 output rows per tile, P = 56, 10 band rows, two 16-channel planes of 560 slots, 36 DMA instructions;
// wave (., ph) owns rows 4 ph .. 4 ph + 3
static void conv_s1b() {
  section = "conv_s1b";
  const int W = 40, P = 56, BROWS = 10, PLANE = BROWS * P, INSTR = 36;
  for (int oy0 = 0; oy0 < W; oy0 += 8) {
    std::vector<Held> lds(INSTR * 64, Held{});
    for (int u = 0; u < INSTR; ++u)
      for (int l = 0; l < 64; ++l) {
        const int qq = band_dma_slot(u, l), ks = qq >= PLANE ? 1 : 0;
        const BandSrc s = s1_band_src(P, W, BROWS, oy0, qq - ks * PLANE);
        lds[u * 64 + l] = Held{true, s.ok, 0, s.iy, s.ix, band_dma_half(qq, l), ks};
      }
    for (int ph = 0; ph < 2; ++ph)
      for (int st = 0; st < 18; ++st)
        for (int j = 0; j < 5; ++j) {
          int addr[64];
          for (int lane = 0; lane < 64; ++lane) {
            const int lr = lane & 31, lh = lane >> 5, pl = 32 * j + lr, jr = pl / W, ox = pl - jr * W, t = st >> 1, ks = st & 1, ky = t / 3, kx = t % 3;
            const int x = ks * PLANE * 32 + band_swizzle(band_addr((4 * ph + jr) * P + ox, lh) + (s1_tap_slots(P, ky, kx) << 5));
            addr[lane] = x;
            const int iy = oy0 + 4 * ph + jr + ky - 1, ix = ox + kx - 1;
            const bool inside = iy >= 0 && iy < W && ix >= 0 && ix < W;
            CHECK(x >= 0 && x / 16 < INSTR * 64, "read past the band: %d", x);
            const Held &h = lds[x / 16];
            CHECK(h.filled && h.ok == inside, "oy0 %d ph %d pixel %d step %d: inside %d, held %d", oy0, ph, pl, st, inside, h.ok);
            if (inside) CHECK(h.iy == iy && h.ix == ix && h.half == lh && h.plane == ks, "oy0 %d ph %d pixel %d step %d: holds (%d, %d, %d, %d)", oy0, ph, pl, st, h.iy, h.ix, h.half, h.plane);
          }
          check_banks(addr);
        }
  }
}

// front.hip's a0 tile: 17 rows x 41 columns (row / column 0 = a0 row / column 2 oy0 - 1 / 2 ox0 - 1: the padding), P = 42, four planes of
// 17 x 42 slots; written from registers, read by the stride-2 phase: 160 output pixels x 9 taps x 4 planes
static void front_a0() {
  section = "front_a0";
  const int ROWS = 17, COLS = 41, P = 42, PLANE = ROWS * P * 32;
  std::vector<int> held(PLANE / 16, -1);                                // (row * 64 + column) * 2 + half
  for (int row = 0; row < ROWS; ++row)
    for (int c = 0; c < COLS; ++c)
      for (int lh = 0; lh < 2; ++lh) {
        const int x = band_swizzle(band_addr(row * P + s2_col_slot(20, c - 1), lh));
        CHECK(x >= 0 && x < PLANE && held[x / 16] == -1, "write of (%d, %d, %d) at %d", row, c, lh, x);
        held[x / 16] = (row * 64 + c) * 2 + lh;
      }
  for (int k = 0; k < 36; ++k)
    for (int j = 0; j < 5; ++j) {
      int addr[64];
      for (int lane = 0; lane < 64; ++lane) {
        const int lr = lane & 31, lh = lane >> 5, pl = 32 * j + lr, jr = pl / 20, ox = pl - jr * 20, tap = k >> 2, ky = tap / 3, kx = tap % 3;
        const int x = band_swizzle(band_addr(s2_tile_row(jr, 8) * P + ox, lh) + (s2_tap_slots(P, 20, ky, kx) << 5));
        addr[lane] = (k & 3) * PLANE + x;
        CHECK(x >= 0 && x < PLANE && held[x / 16] == ((2 * jr + ky) * 64 + 2 * ox + kx) * 2 + lh, "pixel %d tap %d half %d reads %d", pl, tap, lh, x);
      }
      check_banks(addr);
    }
}

// the stem's region: row pitch `pitch`, odd columns from slot `odd`, `rows` x `cols` input pixels; outputs `orows` x `ocols` (pixel tiles of 32
// over `flat` columns per row: stem.hip 2 rows of 16; front.hip 17 rows of 42 flattened, the tail clamped to the last pixel)
static void stem_region(const char *name, int pitch, int odd, int rows, int cols, int orows, int ocols, bool clamp) {
  section = name;
  for (int q = 0; q < pitch; ++q)                                       // fill map and column rule are inverse
    if (stem_slot_col(odd, q) < cols) CHECK(stem_col_slot(odd, stem_slot_col(odd, q)) == q, "slot %d", q);
  for (int c = 0; c < cols; ++c) CHECK(stem_col_slot(odd, c) < pitch && stem_slot_col(odd, stem_col_slot(odd, c)) == c, "column %d", c);
  for (int s = 0; s < 25; ++s)
    for (int lh = 0; lh < 2; ++lh) {
      const int t = stem_step_tap(s, lh);
      CHECK(t == (2 * s + lh == 49 ? 48 : 2 * s + lh), "k-step %d half %d: tap %d", s, lh, t);
      for (int row = 0; row < orows; ++row)
        for (int col = 0; col < ocols; ++col) {
          const int slot = stem_pixel_slot(pitch, row, col) + stem_tap_slots(pitch, odd, t), r = slot / pitch, c = stem_slot_col(odd, slot % pitch);
          CHECK(r == 2 * row + t / 7 && c == 2 * col + t % 7 && r < rows && c < cols, "pixel (%d, %d) tap %d: slot %d = (%d, %d)", row, col, t, slot, r, c);
        }
    }
  const int n_pix = orows * ocols;
  for (int tile = 0; tile * 32 < (clamp ? (n_pix + 31) / 32 * 32 + 32 : n_pix); ++tile)
    for (int s = 0; s < 25; ++s) {
      int addr[64];
      for (int lane = 0; lane < 64; ++lane) {
        const int lr = lane & 31, lh = lane >> 5, pa = clamp && tile * 32 + lr > n_pix - 1 ? n_pix - 1 : tile * 32 + lr;
        addr[lane] = (stem_pixel_slot(pitch, pa / ocols, pa % ocols) + stem_tap_slots(pitch, odd, stem_step_tap(s, lh))) * 16;
      }
      check_banks(addr);
    }
}

static void stem_fragments() {
  section = "stem_fragments";
  for (int Kpad = 400; Kpad <= 416; Kpad += 16)
    for (int f = 0; f < 50; ++f)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int s = f >> 1, i = f & 1;                              // front_pack_stem_kernel's order: fragment f = 2 s + i
          CHECK(stem_frag_src(Kpad, i, s, lane) + e == (size_t)(i * 32 + (lane & 31)) * Kpad + (2 * s + (lane >> 5)) * 8 + e, "fragment %d lane %d", f, lane);
          CHECK((2 * s + (lane >> 5)) * 8 + e < Kpad, "k index past the row");
        }
}

int main() {
  conv_s2();
  conv_s1b();
  front_a0();
  stem_region("stem", 40, 20, 37, 37, 16, 16, false);
  stem_region("front_stem", 93, 45, 39, 89, 17, 42, true);
  stem_fragments();
  printf("ok\n");
  return 0;
}
'''


@pytest.fixture(scope='module')
def result(tmp_path_factory):
  """The compiler beside the hipcc the Makefile names (ROCm's clang++), on conv_band.h alone."""
  hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC \?= (\S+)', open(os.path.join(CSRC, 'Makefile')).read(), flags=re.M).group(1)
  cxx = os.path.join(os.path.dirname(hipcc), 'amdclang++')
  d = tmp_path_factory.mktemp('conv_band')
  src, exe = d / 'band.cc', d / 'band'
  src.write_text(PROGRAM)
  subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, str(src), '-o', str(exe)], check=True)
  return subprocess.run([str(exe)], capture_output=True, text=True)


def test_fill_and_read_agree_and_reads_are_conflict_free(result):
  assert result.returncode == 0 and result.stdout == 'ok\n', result.stdout + result.stderr
