// The state and the cache of the regressor fit (include/jrr.h, jrr_jfit_*), shared by jfit.hip (prepare, gather, joints, step, scatter,
// set_entries), jmom.hip (the moments of a cache range) and jnorm.hip (the reweighted moments of the MPJPE solve).
//
// State (one caller-owned buffer, JF_* word offsets below): the union cols[NS] of the positive columns of J_init*mask, and the listed
// entries of all rows FLATTENED in row order -- entry idx of row i lives at off[i] <= idx < off[i + 1] -- with, per entry, its row and
// its position in cols (one packed word), its vertex, raw value, mask value, Adam m / v and its current normalised weight.
// Cache: sample-major rows of RL = (3 NS + 51) | 1 floats (support vertices | ground truth in mm | padding).
#pragma once
#include "jrr_common.h"
#include "kernels.h"
#include "../../include/jrr.h"

namespace jrr {

constexpr int JF_CAP = NH * JSUP_CAP;                 // 2176: most listed entries, and most union columns
constexpr int JF_THREADS = 256;
constexpr int JF_SPW = JRR_JFIT_SPW;                  // samples per chunk
constexpr int JF_MAX_WG = JRR_JFIT_MAX_WG;
constexpr int JF_GT = NH * 3;                         // 51

static_assert(JSUP_CAP == JRR_JFIT_ROW_CAP, "row capacity");

// header words (int32)
enum { JF_H_NS = 0, JF_H_E = 1, JF_H_STEP = 2, JF_H_ERR = 3, JF_H_ARRIVE = 4, JF_H_CNT = 8, JF_H_OFF = 32, JF_H_RS = 52, JF_HEAD = 96 };
// JF_H_RS: 17 floats, the rows' current sums of relu(raw * mask)
// JF_H_ERR bits: 1 a row above the cap (prepare), 2 a call with a foreign ns, 4 not a prepared state (host side), 8 a listed row whose
// relu(raw * mask) sums to zero (set_entries)
enum { JF_ERR_CAP = 1, JF_ERR_NS = 2, JF_ERR_STATE = 4, JF_ERR_ROWSUM = 8 };

struct JfState {
  int* head; int* pk; int* vtx; int* cols;
  float* raw; float* mk; float* m; float* v; float* jn;
  double* lpart; double* slab;
};
static size_t jf_state_bytes() {
  return (size_t)JF_HEAD * 4 + (size_t)8 * JF_CAP * 4 + (size_t)JF_MAX_WG * 8 + (size_t)JF_MAX_WG * JF_CAP * 8;
}
__host__ __device__ static inline JfState jf_carve(void* base) {
  JfState s;
  s.head = reinterpret_cast<int*>(base);
  s.pk = s.head + JF_HEAD;
  s.vtx = s.pk + JF_CAP;
  s.cols = s.vtx + JF_CAP;
  s.raw = reinterpret_cast<float*>(s.cols + JF_CAP);
  s.mk = s.raw + JF_CAP;
  s.m = s.mk + JF_CAP;
  s.v = s.m + JF_CAP;
  s.jn = s.v + JF_CAP;
  s.lpart = reinterpret_cast<double*>(s.jn + JF_CAP);      // (96 + 8 * 2176) * 4 bytes: a multiple of 8
  s.slab = s.lpart + JF_MAX_WG;
  return s;
}
static_assert(((JF_HEAD + 8 * JF_CAP) * 4) % 8 == 0, "the doubles of the state are 8-byte aligned");

__host__ __device__ static inline int jf_row_floats(int ns) { return (3 * ns + JF_GT) | 1; }

// the checks every call on a cache shares; NULL: fine
static inline const char* jf_check_cache(const void* state, const void* cache, int64_t n_rows, int ns) {
  if (!state || !cache) return "state and cache are required";
  if ((((uintptr_t)state | (uintptr_t)cache) & 15) != 0) return "state and cache must be 16-byte aligned";
  if (ns < 1 || ns > JF_CAP) return "ns must lie in 1 .. 2176";
  if (n_rows < 0 || n_rows > INT32_MAX) return "n_rows must lie in 0 .. 2^31 - 1";
  return nullptr;
}

}  // namespace jrr
