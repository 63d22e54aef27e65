// The host side of csrc/stereo.hip - the option checks and the blob layout - under AddressSanitizer and UBSan, without a GPU: a
// stand-alone program that calls only what never touches the device.
//   cd foundationpose_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-omit-frame-pointer stereo.hip ../../scripts/stereo_host_check.cpp -o /tmp/stereo_host_check && /tmp/stereo_host_check
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <limits>

#include "../foundationpose_amd/csrc/common.h"

static char last_error[1024];
void fp_set_error(const char *fmt, ...) {      // api.hip's, which this program does not link
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error, sizeof(last_error), fmt, ap);
  va_end(ap);
}

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, last_error); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static fp_stereo_opts good() {
  fp_stereo_opts o;
  memset(&o, 0, sizeof(o));
  o.struct_size = sizeof(o), o.max_disparity = 128, o.p1 = 8, o.p2 = 32, o.paths = 0xFF, o.lr_max = 1, o.min_disparity = 1, o.subpixel = 1;
  o.fx = 1067.5, o.baseline = 0.12, o.zfar = std::numeric_limits<float>::infinity();
  return o;
}

int main() {
  char fake[64];
  float depth[1];
  fp_stereo_opts out;
  fp_stereo_opts o = good();
  EXPECT(fp_stereo_check(fake, fake, fake, 1, 1200, 1920, 3, &o, depth, nullptr, &out) == FP_OK);
  EXPECT(fp_stereo_sgm(nullptr, (const uint8_t *)fake, (const uint8_t *)fake, 1, 4, 4, 1, &o, nullptr, nullptr, nullptr, nullptr) == FP_EINVAL);
  fp_stereo_debug dbg;
  memset(&dbg, 0, sizeof(dbg));
  dbg.struct_size = sizeof(dbg);
  EXPECT(fp_stereo_check(fake, fake, fake, 7, 1200, 1920, 1, &o, nullptr, &dbg, &out) == FP_OK);
  EXPECT(fp_stereo_check(fake, fake, fake, 8, 1200, 1920, 1, &o, nullptr, &dbg, &out) == FP_EINVAL);      // more than 2^31 cells
  EXPECT(fp_stereo_check(fake, fake, fake, 2147483647, 2147483647, 2147483647, 1, &o, nullptr, nullptr, &out) == FP_EINVAL);
  dbg.struct_size = 8;
  EXPECT(fp_stereo_check(fake, fake, fake, 1, 4, 4, 1, &o, nullptr, &dbg, &out) == FP_EINVAL);
  const int bad_d[] = {0, -64, 63, 96, 320, 2147483647, -2147483647 - 1};
  for (int d : bad_d) {
    o = good(), o.max_disparity = d;
    EXPECT(fp_stereo_sgm((fp_ctx *)fake, (const uint8_t *)fake, (const uint8_t *)fake, 1, 4, 4, 1, &o, nullptr, nullptr, nullptr, nullptr) == FP_EINVAL);
  }
  const int bad_p[][2] = {{33, 32}, {-1, 32}, {8, 8128}, {2147483647, 2147483647}, {0, -1}};
  for (auto &p : bad_p) {
    o = good(), o.p1 = p[0], o.p2 = p[1];
    EXPECT(fp_stereo_check(fake, fake, fake, 1, 4, 4, 1, &o, nullptr, nullptr, &out) == FP_EINVAL);
  }
  o = good(), o.p1 = 8127, o.p2 = 8127;
  EXPECT(fp_stereo_check(fake, fake, fake, 1, 4, 4, 1, &o, nullptr, nullptr, &out) == FP_OK);
  o = good(), o.paths = 0;
  EXPECT(fp_stereo_check(fake, fake, fake, 1, 4, 4, 1, &o, nullptr, nullptr, &out) == FP_EINVAL);
  o = good(), o.paths = 0xFFFFFFFFu;
  EXPECT(fp_stereo_check(fake, fake, fake, 1, 4, 4, 1, &o, nullptr, nullptr, &out) == FP_EINVAL);
  o = good(), o.min_disparity = 128;
  EXPECT(fp_stereo_check(fake, fake, fake, 1, 4, 4, 1, &o, nullptr, nullptr, &out) == FP_EINVAL);
  const double bad_fx[] = {0.0, -1.0, NAN, INFINITY, 1e300};
  for (double fx : bad_fx) {
    o = good(), o.fx = fx;
    EXPECT(fp_stereo_check(fake, fake, fake, 1, 4, 4, 1, &o, depth, nullptr, &out) == FP_EINVAL);
    EXPECT(fp_stereo_check(fake, fake, fake, 1, 4, 4, 1, &o, nullptr, nullptr, &out) == FP_OK);      // read only with d_depth
  }
  o = good(), o.zfar = NAN;
  EXPECT(fp_stereo_check(fake, fake, fake, 1, 4, 4, 1, &o, depth, nullptr, &out) == FP_EINVAL);
  o = good(), o.struct_size = sizeof(o) - 8;
  EXPECT(fp_stereo_check(fake, fake, fake, 1, 4, 4, 1, &o, depth, nullptr, &out) == FP_EINVAL);

  // the layout: consecutive, 256-byte aligned, nothing overlaps, the largest accepted call does not overflow
  const int sizes[][5] = {{1, 1, 1, 64, 1}, {1, 1200, 1920, 128, 3}, {3, 40, 176, 64, 1}, {7, 1200, 1920, 128, 1}, {65535, 1, 1, 256, 3}, {1, 4096, 2048, 256, 3}};
  for (auto &s : sizes) {
    const StereoLayout l = fp_stereo_layout(s[0], s[1], s[2], s[3], s[4]);
    const size_t px = (size_t)s[0] * s[1] * s[2];
    const size_t off[] = {l.o_grey_l, l.o_grey_r, l.o_census_l, l.o_census_r, l.o_sum, l.o_dstar, l.o_dright, l.bytes};
    const size_t len[] = {s[4] == 3 ? px : 0, s[4] == 3 ? px : 0, px * 8, px * 8, px * (size_t)s[3] * 2, px * 4, px * 4};
    for (int i = 0; i < 7; ++i) {
      if (len[i] == 0) continue;
      EXPECT(off[i] % 256 == 0);
      size_t next = l.bytes;
      for (int j = i + 1; j < 8; ++j)
        if (j == 7 || len[j]) {
          next = off[j];
          break;
        }
      EXPECT(off[i] + len[i] <= next);
    }
    EXPECT(l.bytes >= px * (16 + 2 * (size_t)s[3] + 8) && l.bytes <= px * (18 + 2 * (size_t)s[3] + 8) + 8 * 256);
  }
  printf(failures ? "stereo_host_check: %d FAILED\n" : "stereo_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
