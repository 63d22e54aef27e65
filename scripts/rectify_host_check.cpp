// The host side of csrc/rectify.hip - every check of a value of fp_remap - under AddressSanitizer and UBSan, without a GPU: a
// stand-alone program that calls only what never touches the device.
//   cd foundationpose_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-omit-frame-pointer rectify.hip ../../scripts/rectify_host_check.cpp -o /tmp/rectify_host_check && /tmp/rectify_host_check
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

static fp_remap_plan good_plan() {
  fp_remap_plan p;
  memset(&p, 0, sizeof(p));
  p.k_new[0] = p.k_new[1] = p.k_raw[0] = p.k_raw[1] = 500.f;
  p.k_new[2] = p.k_raw[2] = 320.f, p.k_new[3] = p.k_raw[3] = 240.f;
  p.rot[0] = p.rot[4] = p.rot[8] = 1.f;
  p.dist[0] = -0.1f;
  p.r2_max = std::numeric_limits<float>::infinity();
  p.src_h = p.dst_h = 480, p.src_w = p.dst_w = 640;
  return p;
}

static fp_remap_opts good() {
  fp_remap_opts o;
  memset(&o, 0, sizeof(o));
  o.struct_size = sizeof(o), o.mode = FP_REMAP_COLOUR, o.channels = 3, o.n_plans = 2, o.zfar = std::numeric_limits<float>::infinity();
  o.plan[0] = o.plan[1] = good_plan();
  return o;
}

int main() {
  char fake[64];
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  fp_remap_opts o = good();
  fp_remap_debug dbg{sizeof(fp_remap_debug), nullptr, nullptr};
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_OK);
  EXPECT(fp_remap_check(fake, fake, fake, 6, &o, fake, fake, &dbg) == FP_OK);
  EXPECT(fp_remap_check(nullptr, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL);
  EXPECT(fp_remap_check(fake, nullptr, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL);
  EXPECT(fp_remap_check(fake, fake, nullptr, 2, &o, fake, fake, nullptr) == FP_EINVAL);
  EXPECT(fp_remap_check(fake, fake, fake, 2, nullptr, fake, fake, nullptr) == FP_EINVAL);
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, nullptr, fake, nullptr) == FP_EINVAL);
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, nullptr, nullptr) == FP_EINVAL);
  EXPECT(fp_remap_check(fake, fake, fake, 3, &o, fake, fake, nullptr) == FP_EINVAL && strstr(last_error, "multiple of n_plans"));
  EXPECT(fp_remap_check(fake, fake, fake, 0, &o, fake, fake, nullptr) == FP_EINVAL);
  dbg.struct_size = 8;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, &dbg) == FP_EINVAL);
  o.n_plans = 1;      // the second plan and the second pointers are not looked at
  o.plan[1].src_h = -7, o.plan[1].rot[3] = nan;
  EXPECT(fp_remap_check(fake, fake, nullptr, 3, &o, fake, nullptr, nullptr) == FP_OK);
  o = good(), o.struct_size -= 4;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL && strstr(last_error, "struct_size"));
  o = good(), o.mode = 2;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL);
  o = good(), o.channels = 2;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL);
  o = good(), o.mode = FP_REMAP_DEPTH;      // three channels of depth
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL);
  o.channels = 1;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_OK);
  o.zfar = 0.f;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL && strstr(last_error, "zfar"));
  o.zfar = nan;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL);
  o = good(), o.n_plans = 3;
  EXPECT(fp_remap_check(fake, fake, fake, 3, &o, fake, fake, nullptr) == FP_EINVAL);
  o = good(), o.plan[1].dst_w = 641;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL && strstr(last_error, "differ in size"));
  o = good(), o.plan[0].src_h = o.plan[1].src_h = FP_REMAP_MAX_SIDE + 1;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL);
  o.plan[0].src_h = o.plan[1].src_h = FP_REMAP_MAX_SIDE;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_OK);
  o = good(), o.plan[0].dst_h = o.plan[1].dst_h = 0;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL);
  for (int i = 0; i < 25; ++i) {      // every float of a plan but r2_max refuses a NaN and an infinity
    for (float bad : {nan, inf, -inf}) {
      o = good();
      float *v = i < 4 ? &o.plan[1].k_new[i] : i < 13 ? &o.plan[1].rot[i - 4] : i < 17 ? &o.plan[1].k_raw[i - 13] : &o.plan[1].dist[i - 17];
      *v = bad;
      EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL);
    }
  }
  o = good(), o.plan[0].k_raw[1] = 0.f;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL && strstr(last_error, "fx, fy"));
  o = good(), o.plan[0].r2_max = 0.f;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL && strstr(last_error, "r2_max"));
  o.plan[0].r2_max = nan;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_EINVAL);
  o.plan[0].r2_max = 0.8333f;
  EXPECT(fp_remap_check(fake, fake, fake, 2, &o, fake, fake, nullptr) == FP_OK);
  o = good(), o.plan[0].dst_h = o.plan[1].dst_h = o.plan[0].dst_w = o.plan[1].dst_w = FP_REMAP_MAX_SIDE;      // 2^28 pixels an image
  EXPECT(fp_remap_check(fake, fake, fake, 2 * 4096, &o, fake, fake, nullptr) == FP_OK);
  EXPECT(fp_remap_check(fake, fake, fake, 2 * 4098, &o, fake, fake, nullptr) == FP_EINVAL && strstr(last_error, "2^40"));
  printf(failures ? "rectify_host_check: %d FAILED\n" : "rectify_host_check: all passed\n", failures);
  return failures ? 1 : 0;
}
