// The host side of csrc/reproject.hip - every check of a value of fp_depth_reproject - under AddressSanitizer and UBSan, without a GPU: a
// stand-alone program that calls only what never touches the device.
//   cd foundationpose_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-omit-frame-pointer reproject.hip ../../scripts/reproject_host_check.cpp -o /tmp/reproject_host_check && /tmp/reproject_host_check
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <limits>
#include <vector>

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

struct Args {
  // exactly V cameras and transforms, so that a read behind view V - 1 is a heap overflow the sanitizer reports
  std::vector<double> Ks, Ts;
  double Kd[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};
  int n = 1, V = 2, Hs = 480, Ws = 640, Hd = 720, Wd = 1280;
  float zfar = std::numeric_limits<float>::infinity();
  explicit Args(int views = 2) : V(views) {
    for (int s = 0; s < views; ++s) {
      const double K[9] = {400, 0, 319.5, 0, 401, 239.5, 0, 0, 1};
      Ks.insert(Ks.end(), K, K + 9);
      for (int e = 0; e < 16; ++e) Ts.push_back(e % 5 == 0 ? 1.0 : 0.0);
    }
  }
};

// fx, cx, fy, cy are rounded to fp32 and travel to the kernel; of the other entries only what is not finite as a double is refused
static bool k_entry_travels(int e) { return e == 0 || e == 2 || e == 4 || e == 5; }

static char fake[64] __attribute__((aligned(8)));

static int check(const Args &a, const void *ctx = fake, const void *depth = fake, const void *keys = fake, const void *out = fake) {
  return fp_depth_reproject_check(ctx, depth, a.n, a.V, a.Hs, a.Ws, a.Ks.data(), a.Ts.data(), a.Kd, a.Hd, a.Wd, a.zfar, keys, out);
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  Args a;
  EXPECT(check(a) == FP_OK);
  EXPECT(check(Args(1)) == FP_OK);
  EXPECT(check(Args(FP_REPROJECT_MAX_VIEWS)) == FP_OK);
  EXPECT(check(a, nullptr) == FP_EINVAL && strstr(last_error, "null"));
  EXPECT(check(a, fake, nullptr) == FP_EINVAL);
  EXPECT(check(a, fake, fake, nullptr) == FP_EINVAL);
  EXPECT(check(a, fake, fake, fake, nullptr) == FP_EINVAL);
  EXPECT(fp_depth_reproject_check(fake, fake, 1, 2, 480, 640, nullptr, a.Ts.data(), a.Kd, 720, 1280, a.zfar, fake, fake) == FP_EINVAL);
  EXPECT(fp_depth_reproject_check(fake, fake, 1, 2, 480, 640, a.Ks.data(), nullptr, a.Kd, 720, 1280, a.zfar, fake, fake) == FP_EINVAL);
  EXPECT(fp_depth_reproject_check(fake, fake, 1, 2, 480, 640, a.Ks.data(), a.Ts.data(), nullptr, 720, 1280, a.zfar, fake, fake) == FP_EINVAL);
  EXPECT(check(a, fake, fake, fake + 4) == FP_EINVAL && strstr(last_error, "8-byte aligned"));
  EXPECT(check(a, fake, fake, fake + 8) == FP_OK);
  // the counts are refused before an array is read: V = 9 with arrays of 2 views must not touch view 2
  a.V = 0;
  EXPECT(check(a) == FP_EINVAL && strstr(last_error, "V 0"));
  a.V = FP_REPROJECT_MAX_VIEWS + 1;
  EXPECT(check(a) == FP_EINVAL);
  a.V = -3;
  EXPECT(check(a) == FP_EINVAL);
  a = Args(), a.n = 0;
  EXPECT(check(a) == FP_EINVAL && strstr(last_error, "n 0"));
  a.n = -1;
  EXPECT(check(a) == FP_EINVAL);
  a.n = FP_REPROJECT_MAX_FRAMES + 1;
  EXPECT(check(a) == FP_EINVAL);
  a.n = FP_REPROJECT_MAX_FRAMES;
  EXPECT(check(a) == FP_OK);
  for (int which = 0; which < 4; ++which) {
    for (int bad : {0, -1, FP_REMAP_MAX_SIDE + 1, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()}) {
      a = Args();
      (which == 0 ? a.Hs : which == 1 ? a.Ws : which == 2 ? a.Hd : a.Wd) = bad;
      EXPECT(check(a) == FP_EINVAL && strstr(last_error, "each side"));
    }
    a = Args(1);
    (which == 0 ? a.Hs : which == 1 ? a.Ws : which == 2 ? a.Hd : a.Wd) = FP_REMAP_MAX_SIDE;
    EXPECT(check(a) == FP_OK);
  }
  a = Args(8), a.Hs = a.Ws = FP_REMAP_MAX_SIDE;      // 2^31 source pixels a frame
  EXPECT(check(a) == FP_EINVAL && strstr(last_error, "2^31 - 1"));
  a = Args(7), a.Hs = a.Ws = a.Hd = a.Wd = FP_REMAP_MAX_SIDE, a.n = FP_REPROJECT_MAX_FRAMES;      // the largest call there is
  EXPECT(check(a) == FP_OK);
  for (int s = 0; s < 2; ++s) {
    for (double bad : {nan, inf, -inf, 1e300}) {      // 1e300 is finite as a double and an infinity in fp32
      for (int e = 0; e < 9; ++e) {
        a = Args(), a.Ks[s * 9 + e] = bad;
        EXPECT(check(a) == ((k_entry_travels(e) || !std::isfinite(bad)) ? FP_EINVAL : FP_OK));
      }
      for (int e = 0; e < 16; ++e) {
        a = Args(), a.Ts[s * 16 + e] = bad;
        // the last row travels nowhere: only what is not finite as a double is refused there
        EXPECT(check(a) == ((e < 12 || !std::isfinite(bad)) ? FP_EINVAL : FP_OK));
      }
    }
    a = Args(), a.Ks[s * 9] = 0.0;
    EXPECT(check(a) == FP_EINVAL && strstr(last_error, "fx, fy"));
    a = Args(), a.Ks[s * 9 + 4] = -400.0;
    EXPECT(check(a) == FP_EINVAL && strstr(last_error, "fx, fy"));
    a = Args(), a.Ks[s * 9] = 1e-60;      // positive as a double, 0 in fp32
    EXPECT(check(a) == FP_EINVAL);
  }
  for (double bad : {nan, inf, -inf, 1e300}) {
    for (int e = 0; e < 9; ++e) {
      a = Args(), a.Kd[e] = bad;
      if (k_entry_travels(e) || !std::isfinite(bad)) EXPECT(check(a) == FP_EINVAL && strstr(last_error, "K_dst"));
      else EXPECT(check(a) == FP_OK);
    }
  }
  a = Args(), a.Kd[4] = 0.0;
  EXPECT(check(a) == FP_EINVAL && strstr(last_error, "K_dst"));
  for (float bad : {0.f, -1.f, std::numeric_limits<float>::quiet_NaN(), -std::numeric_limits<float>::infinity()}) {
    a = Args(), a.zfar = bad;
    EXPECT(check(a) == FP_EINVAL && strstr(last_error, "zfar"));
  }
  a = Args(), a.zfar = 1e-30f;
  EXPECT(check(a) == FP_OK);
  printf(failures ? "reproject_host_check: %d FAILED\n" : "reproject_host_check: all passed\n", failures);
  return failures ? 1 : 0;
}
