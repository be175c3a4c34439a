// Stand-alone host program around the argument checking of csrc/jprice.hip (jrr_jfit_price_bytes, jrr_jfit_price), for a sanitizer build
// of that host code on a machine without a GPU: jrr_jfit_price_bytes is host arithmetic alone, and every call of jrr_jfit_price below is
// refused on the host -- the lists are validated there -- before anything is enqueued, so no device is touched and no device pointer is
// read.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//         joint-regressor-refinement_amd/csrc/jprice.hip tools/jprice_args_check.cpp -o jprice_args_check && ./jprice_args_check
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

static int g_failed = 0, g_checks = 0;
#define EXPECT(call, want, text)                                                                        \
  do {                                                                                                  \
    g_err[0] = 0;                                                                                       \
    ++g_checks;                                                                                         \
    const long long rc_ = (long long)(call);                                                            \
    if (rc_ != (long long)(want) || ((text)[0] && !strstr(g_err, (text)))) {                            \
      printf("FAILED line %d: rc %lld (want %lld), message '%s' (want '%s')\n", __LINE__, rc_, (long long)(want), g_err, (text)); \
      ++g_failed;                                                                                       \
    }                                                                                                   \
  } while (0)

int main() {
  alignas(16) static float verts[64], gt[64];
  alignas(16) static double out[64], scratch[64];
  static int32_t vtx[17 * 128], counts[17];
  static double x[17 * 128];
  const float* v2 = reinterpret_cast<const float*>(reinterpret_cast<const char*>(verts) + 2);
  const float* g1 = reinterpret_cast<const float*>(reinterpret_cast<const char*>(gt) + 1);
  double* o4 = reinterpret_cast<double*>(reinterpret_cast<char*>(out) + 4);
  void* w4 = reinterpret_cast<char*>(scratch) + 4;
  const size_t head = 17 * 128 * 4 + 128 + 17 * 128 * 8, slab = (size_t)431 * 256 * 8;
  const size_t big = (size_t)1 << 40;
  // jrr_jfit_price_bytes(batch, scratch_bytes): head + 512 bytes a sample + one slab of 431 tiles per chunk; chunks of a multiple of 4
  // samples, at least 8, at most 38 chunks
  size_t need = 1;
  EXPECT(jrr_jfit_price_bytes(0, &need), 0, "");
  EXPECT(need, 0, "");
  need = 1;
  EXPECT(jrr_jfit_price_bytes(-5, &need), 0, "");
  EXPECT(need, 0, "");
  EXPECT(jrr_jfit_price_bytes(1, &need), JRR_JFIT_PRICE_DOUBLES * 8, "");
  EXPECT(need, head + 512 + slab, "");
  EXPECT(jrr_jfit_price_bytes(8, &need), (16 * 6890 + 64) * 8, "");
  EXPECT(need, head + 8 * 512 + slab, "");
  EXPECT(jrr_jfit_price_bytes(9, &need), (16 * 6890 + 64) * 8, "");
  EXPECT(need, head + 9 * 512 + 2 * slab, "");                                       // 2 chunks of 8: 8 + 1
  EXPECT(jrr_jfit_price_bytes(130, &need), (16 * 6890 + 64) * 8, "");
  EXPECT(need, head + 130 * 512 + 17 * slab, "");                                    // 17 chunks of 8: 16 * 8 + 2
  EXPECT(jrr_jfit_price_bytes(4096, &need), (16 * 6890 + 64) * 8, "");
  EXPECT(need, head + (size_t)4096 * 512 + 38 * slab, "");                           // 38 chunks of 108
  EXPECT(jrr_jfit_price_bytes(305, &need), (16 * 6890 + 64) * 8, "");
  EXPECT(need, head + (size_t)305 * 512 + 26 * slab, "");                            // ceil(305 / 38) = 9 -> chunks of 12: 26 of them
  EXPECT(jrr_jfit_price_bytes(2147483647, &need), (16 * 6890 + 64) * 8, "");
  EXPECT(need, head + (size_t)2147483647 * 512 + 38 * slab, "");
  EXPECT(jrr_jfit_price_bytes(4, nullptr), (16 * 6890 + 64) * 8, "");
  // jrr_jfit_price(verts, gt_mm, batch, vtx, counts, x, mode, delta_m, accumulate, out, scratch, scratch_bytes, stream)
  counts[1] = 2;
  vtx[128] = 5;
  vtx[129] = 6889;
  x[128] = x[129] = 0.5;
  counts[16] = 128;
  for (int e = 0; e < 128; ++e) vtx[16 * 128 + e] = 50 * e;
  const double d = 1e-5;
  EXPECT(jrr_jfit_price(nullptr, gt, 4, vtx, counts, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "are required");
  EXPECT(jrr_jfit_price(verts, nullptr, 4, vtx, counts, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "are required");
  EXPECT(jrr_jfit_price(verts, gt, 4, nullptr, counts, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "are required");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, nullptr, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "are required");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, nullptr, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "are required");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, 0.0, 0, nullptr, scratch, big, nullptr), JRR_ERR_ARG, "are required");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, 0.0, 0, out, nullptr, big, nullptr), JRR_ERR_ARG, "are required");
  EXPECT(jrr_jfit_price(v2, gt, 4, vtx, counts, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "4-byte aligned");
  EXPECT(jrr_jfit_price(verts, g1, 4, vtx, counts, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "4-byte aligned");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, 0.0, 0, o4, scratch, big, nullptr), JRR_ERR_ARG, "8-byte aligned");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, 0.0, 0, out, w4, big, nullptr), JRR_ERR_ARG, "8-byte aligned");
  EXPECT(jrr_jfit_price(verts, gt, 0, vtx, counts, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "batch must be");
  EXPECT(jrr_jfit_price(verts, gt, -3, vtx, counts, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "batch must be");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 2, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "mode must be");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, -1, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "mode must be");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, -d, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "finite and not negative");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, NAN, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "finite and not negative");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, INFINITY, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "finite and not negative");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 1, -d, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "finite and not negative");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 1, NAN, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "finite and not negative");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 1, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "positive in JRR_JFIT_PRICE_NORM");
  counts[3] = 129;
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "a count must lie");
  counts[3] = -1;
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "a count must lie");
  counts[3] = 0;
  vtx[129] = 6890;
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "must lie in 0 .. 6889");
  vtx[129] = -1;
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "must lie in 0 .. 6889");
  vtx[129] = 5;
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "listed twice");
  vtx[129] = 6889;
  vtx[16 * 128 + 127] = 50;                                                          // the last entry of the longest row repeats its second
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "listed twice");
  vtx[16 * 128 + 127] = 5;                                                           // the same vertex in ANOTHER row is fine: see below
  {
    int32_t none[17] = {0};
    EXPECT(jrr_jfit_price(verts, gt, 4, vtx, none, x, 0, 0.0, 0, out, scratch, big, nullptr), JRR_ERR_ARG, "no row has an entry");
  }
  // valid lists (a vertex shared by two rows, a bad index BEHIND a row's count): the scratch is what is missing
  vtx[130] = -77;
  EXPECT(jrr_jfit_price_bytes(4, &need), (16 * 6890 + 64) * 8, "");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 0, 0.0, 0, out, scratch, need - 1, nullptr), JRR_ERR_WORKSPACE, "the scratch needs");
  EXPECT(jrr_jfit_price(verts, gt, 4, vtx, counts, x, 1, d, 1, out, scratch, 0, nullptr), JRR_ERR_WORKSPACE, "the scratch needs");
  printf(g_failed ? "%d of %d checks FAILED\n" : "jprice argument checks ok (%d)\n", g_failed ? g_failed : g_checks, g_checks);
  return g_failed ? 1 : 0;
}
