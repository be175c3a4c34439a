// Stand-alone host program around the argument checking of csrc/views.hip (jrr_view_relrot_accumulate, jrr_view_fuse), for a sanitizer
// build of that host code on a machine without a GPU: every call below is refused, or returns before a launch (an empty position
// range), so no device is touched and no pointer is read.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//         joint-regressor-refinement_amd/csrc/views.hip tools/views_args_check.cpp -o views_args_check && ./views_args_check
#include <cmath>
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
  alignas(16) static int64_t lbuf[16];
  float* f = buf;
  int32_t* i = ibuf;
  int64_t* a = lbuf;
  float* odd = reinterpret_cast<float*>(reinterpret_cast<char*>(buf) + 4);
  int32_t* iodd = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ibuf) + 2);
  int64_t* aodd = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(lbuf) + 4);
  // jrr_view_relrot_accumulate(table, n_rows, order, group, pair, ref_pair, n_pairs, m, begin, count, acc, status, stream)
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, i, 4, 40, 0, 0, a, i, nullptr), JRR_OK, "");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, i, 4, 40, 40, 0, a, i, nullptr), JRR_OK, "");
  EXPECT(jrr_view_relrot_accumulate(f, 0, i, i, i, nullptr, 0, 0, 0, 0, nullptr, i, nullptr), JRR_OK, "");      // no pair: no per-pair array
  EXPECT(jrr_view_relrot_accumulate(nullptr, 64, i, i, i, i, 4, 40, 0, 0, a, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_relrot_accumulate(f, 64, nullptr, i, i, i, 4, 40, 0, 0, a, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, nullptr, i, i, 4, 40, 0, 0, a, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, nullptr, i, 4, 40, 0, 0, a, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, nullptr, 4, 40, 0, 0, a, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, i, 4, 40, 0, 0, nullptr, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, i, 4, 40, 0, 0, a, nullptr, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, i, -1, 40, 0, 0, a, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_relrot_accumulate(f, -1, i, i, i, i, 4, 40, 0, 0, a, i, nullptr), JRR_ERR_ARG, "n_rows");
  EXPECT(jrr_view_relrot_accumulate(f, (int64_t)1 << 31, i, i, i, i, 4, 40, 0, 0, a, i, nullptr), JRR_ERR_ARG, "n_rows");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, i, 4, -1, 0, 0, a, i, nullptr), JRR_ERR_ARG, "n_rows");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, i, 4, INT32_MAX, 0, 0, a, i, nullptr), JRR_ERR_ARG, "n_rows");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, i, 4, 40, -1, 0, a, i, nullptr), JRR_ERR_ARG, "position range");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, i, 4, 40, 41, 0, a, i, nullptr), JRR_ERR_ARG, "position range");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, i, 4, 40, 0, 41, a, i, nullptr), JRR_ERR_ARG, "position range");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, i, 4, 40, 30, INT32_MAX, a, i, nullptr), JRR_ERR_ARG, "position range");   // begin + count is never formed
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, i, 4, 40, 0, -1, a, i, nullptr), JRR_ERR_ARG, "position range");
  EXPECT(jrr_view_relrot_accumulate(odd, 64, i, i, i, i, 4, 40, 0, 0, a, i, nullptr), JRR_ERR_ARG, "8-byte aligned");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, iodd, i, i, 4, 40, 0, 0, a, i, nullptr), JRR_ERR_ARG, "4-byte aligned");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, iodd, 4, 40, 0, 0, a, i, nullptr), JRR_ERR_ARG, "4-byte aligned");
  EXPECT(jrr_view_relrot_accumulate(f, 64, i, i, i, i, 4, 40, 0, 0, aodd, i, nullptr), JRR_ERR_ARG, "8-byte aligned");
  // jrr_view_fuse(table, n_rows, order, group, pair, rel, n_pairs, m, cos_half_max, begin, count, x6d, betas, body, orient, members, dropped, status, stream)
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.9f, 0, 0, f, f, f, f, i, i, i, nullptr), JRR_OK, "");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.f, 40, 0, f, f, f, f, i, i, i, nullptr), JRR_OK, "");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, -1.f, 0, 0, f, f, f, f, i, i, i, nullptr), JRR_OK, "");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, nullptr, 0, 40, 1.f, 0, 0, f, f, f, f, i, i, i, nullptr), JRR_OK, "");
  EXPECT(jrr_view_fuse(nullptr, 64, i, i, i, f, 4, 40, 0.9f, 0, 0, f, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_fuse(f, 64, nullptr, i, i, f, 4, 40, 0.9f, 0, 0, f, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_fuse(f, 64, i, nullptr, i, f, 4, 40, 0.9f, 0, 0, f, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_fuse(f, 64, i, i, nullptr, f, 4, 40, 0.9f, 0, 0, f, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, nullptr, 4, 40, 0.9f, 0, 0, f, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.9f, 0, 0, nullptr, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.9f, 0, 0, f, nullptr, f, f, i, i, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.9f, 0, 0, f, f, nullptr, f, i, i, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.9f, 0, 0, f, f, f, nullptr, i, i, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.9f, 0, 0, f, f, f, f, nullptr, i, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.9f, 0, 0, f, f, f, f, i, nullptr, i, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.9f, 0, 0, f, f, f, f, i, i, nullptr, nullptr), JRR_ERR_ARG, "bad argument");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 1.5f, 0, 0, f, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "cos_half_max");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, NAN, 0, 0, f, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "cos_half_max");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.9f, 0, 41, f, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "position range");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.9f, INT32_MAX, INT32_MAX, f, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "position range");
  EXPECT(jrr_view_fuse(f, INT64_MAX, i, i, i, f, 4, 40, 0.9f, 0, 0, f, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "n_rows");
  EXPECT(jrr_view_fuse(odd, 64, i, i, i, f, 4, 40, 0.9f, 0, 0, f, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "8-byte aligned");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.9f, 0, 0, odd, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "16-byte aligned");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f + 2, 4, 40, 0.9f, 0, 0, f, f, f, f, i, i, i, nullptr), JRR_ERR_ARG, "16-byte aligned");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.9f, 0, 0, f, f, f, f, iodd, i, i, nullptr), JRR_ERR_ARG, "4-byte aligned");
  EXPECT(jrr_view_fuse(f, 64, i, i, i, f, 4, 40, 0.9f, 0, 0, f, odd, odd, odd, i, i, i, nullptr), JRR_OK, "");
  printf(g_failed ? "%d checks FAILED\n" : "views argument checks ok\n", g_failed);
  return g_failed ? 1 : 0;
}
