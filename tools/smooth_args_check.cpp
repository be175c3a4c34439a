// Stand-alone host program around the argument checking of csrc/smooth.hip (jrr_pose_smooth, jrr_pose_jitter), for a sanitizer build
// of that host code on a machine without a GPU: every call below is refused, or returns before a launch (an empty position range), so
// no device is touched and no pointer is read.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//         joint-regressor-refinement_amd/csrc/smooth.hip tools/smooth_args_check.cpp -o smooth_args_check && ./smooth_args_check
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/jrr.h"

static char g_err[512];
void jrr_set_error(const char* fmt, ...) {      // api.hip's, which this program does not link
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static int g_failed = 0;
#define EXPECT(call, want, text)                                                                        \
  do {                                                                                                  \
    g_err[0] = 0;                                                                                       \
    const int rc_ = (call);                                                                             \
    if (rc_ != (want) || ((text)[0] && !strstr(g_err, (text)))) {                                       \
      printf("FAILED line %d: rc %d (want %d), message '%s' (want '%s')\n", __LINE__, rc_, (want), g_err, (text)); \
      ++g_failed;                                                                                       \
    }                                                                                                   \
  } while (0)

int main() {
  alignas(16) static float buf[64];
  alignas(16) static int32_t ibuf[16];
  float* f = buf;
  int32_t* i = ibuf;
  float* odd = reinterpret_cast<float*>(reinterpret_cast<char*>(buf) + 4);
  // jrr_pose_smooth(table, n_rows, order, run, m, weights, radius, begin, count, x6d, betas, cam, delta, status, stream)
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 0, 0, f, f, f, f, i, nullptr), JRR_OK, "");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 40, 0, f, f, f, f, i, nullptr), JRR_OK, "");
  EXPECT(jrr_pose_smooth(f, 0, i, i, 0, f, 0, 0, 0, f, f, f, f, i, nullptr), JRR_OK, "");
  EXPECT(jrr_pose_smooth(nullptr, 64, i, i, 40, f, 6, 0, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_smooth(f, 64, nullptr, i, 40, f, 6, 0, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_smooth(f, 64, i, nullptr, 40, f, 6, 0, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, nullptr, 6, 0, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 0, 0, nullptr, f, f, f, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 0, 0, f, nullptr, f, f, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 0, 0, f, f, nullptr, f, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 0, 0, f, f, f, nullptr, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 0, 0, f, f, f, f, nullptr, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 17, 0, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "radius 17");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, -1, 0, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "radius -1");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, INT32_MIN, 0, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "radius");
  EXPECT(jrr_pose_smooth(f, -1, i, i, 40, f, 6, 0, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "n_rows");
  EXPECT(jrr_pose_smooth(f, (int64_t)1 << 31, i, i, 40, f, 6, 0, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "n_rows");
  EXPECT(jrr_pose_smooth(f, INT64_MAX, i, i, 40, f, 6, 0, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "n_rows");
  EXPECT(jrr_pose_smooth(f, 64, i, i, -1, f, 6, 0, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "n_rows");
  EXPECT(jrr_pose_smooth(f, 64, i, i, INT32_MAX, f, 6, 0, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "n_rows");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, -1, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "position range");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 41, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "position range");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 0, 41, f, f, f, f, i, nullptr), JRR_ERR_ARG, "position range");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 30, INT32_MAX, f, f, f, f, i, nullptr), JRR_ERR_ARG, "position range");   // begin + count is never formed
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, INT32_MAX, INT32_MAX, f, f, f, f, i, nullptr), JRR_ERR_ARG, "position range");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 0, -1, f, f, f, f, i, nullptr), JRR_ERR_ARG, "position range");
  EXPECT(jrr_pose_smooth(odd, 64, i, i, 40, f, 6, 0, 0, f, f, f, f, i, nullptr), JRR_ERR_ARG, "8-byte aligned");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 0, 0, odd, f, f, f, i, nullptr), JRR_ERR_ARG, "16-byte aligned");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 0, 0, f + 2, f, f, f, i, nullptr), JRR_ERR_ARG, "16-byte aligned");
  EXPECT(jrr_pose_smooth(f, 64, i, i, 40, f, 6, 0, 0, f, odd, odd, odd, i, nullptr), JRR_OK, "");
  // jrr_pose_jitter(table, n_rows, order, run, m, begin, count, jitter, status, stream)
  EXPECT(jrr_pose_jitter(f, 64, i, i, 40, 0, 0, f, i, nullptr), JRR_OK, "");
  EXPECT(jrr_pose_jitter(f, 64, i, i, 40, 40, 0, f, i, nullptr), JRR_OK, "");
  EXPECT(jrr_pose_jitter(nullptr, 64, i, i, 40, 0, 0, f, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_jitter(f, 64, nullptr, i, 40, 0, 0, f, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_jitter(f, 64, i, nullptr, 40, 0, 0, f, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_jitter(f, 64, i, i, 40, 0, 0, nullptr, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_jitter(f, 64, i, i, 40, 0, 0, f, nullptr, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_pose_jitter(f, 64, i, i, 40, 0, 41, f, i, nullptr), JRR_ERR_ARG, "position range");
  EXPECT(jrr_pose_jitter(f, 64, i, i, 40, 39, INT32_MAX, f, i, nullptr), JRR_ERR_ARG, "position range");
  EXPECT(jrr_pose_jitter(f, -5, i, i, 40, 0, 0, f, i, nullptr), JRR_ERR_ARG, "n_rows");
  EXPECT(jrr_pose_jitter(f, 64, i, i, 40, 0, 0, reinterpret_cast<float*>(reinterpret_cast<char*>(buf) + 2), i, nullptr), JRR_ERR_ARG, "4-byte aligned");
  printf(g_failed ? "%d checks FAILED\n" : "smooth argument checks ok\n", g_failed);
  return g_failed ? 1 : 0;
}
