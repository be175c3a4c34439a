// The grouped int64 accumulator of the report tables (include/jrr.h, JRR_EVAL_ACC_*), stated once for the kernels and
// the entry points of evalrep, regrep, depth, pen, accel, pve, bones and boot.hip (views.hip takes the atomic add alone):
//
//   int64 table[n_groups][row_words], then the trailer: word JRR_EVAL_ACC_TRAILER_IGNORED, word JRR_EVAL_ACC_TRAILER_BAD_GROUP
//   (boot.hip's table carries a third word of its own behind them); 1 <= n_groups <= JRR_EVAL_ACC_MAX_GROUPS.
//
// A pose goes to exactly one place: group < 0 to trailer word 0, group >= n_groups to trailer word 1, any other is counted whole in
// its group's row or lands in the row's BAD word.  Every update is an int64 atomic add: integer adds commute, so a table is a function
// of the multiset of poses alone -- not of their order, of the split into calls or of the sharding over ranks.
#pragma once
#include "jrr_common.h"
#include "fixedpt.h"
#include "../../include/jrr.h"

namespace jrr {

static_assert(JRR_EVAL_ACC_TRAILER == 2 && JRR_EVAL_ACC_TRAILER_IGNORED == 0 && JRR_EVAL_ACC_TRAILER_BAD_GROUP == 1, "trailer words");

// What a pose is to the table.  Kinds below ACC_IGNORED land in the row of the pose's group, and 2 is free for a table's own such kind
// (accel.hip: a position without a triple); ACC_IGNORED + t is trailer word t.
enum { ACC_COUNTED = 0, ACC_BAD = 1, ACC_IGNORED = 3, ACC_BAD_GROUP = 4 };
static_assert(ACC_BAD_GROUP - ACC_IGNORED == JRR_EVAL_ACC_TRAILER_BAD_GROUP - JRR_EVAL_ACC_TRAILER_IGNORED, "kind -> trailer word");

__device__ __forceinline__ void acc_add(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

__device__ __forceinline__ long long* acc_row(long long* acc, int row_words, int g) { return acc + (size_t)g * row_words; }
__device__ __forceinline__ long long* acc_trailer(long long* acc, int row_words, int n_groups) { return acc_row(acc, row_words, n_groups); }

// the group id alone: ACC_IGNORED, ACC_BAD_GROUP, or ACC_COUNTED for a pose that reaches its row (the caller decides COUNTED / BAD there).
// The tile kernels keep this kind in LDS.
__device__ __forceinline__ int acc_group_kind(int g, int n_groups) { return g < 0 ? ACC_IGNORED : (g >= n_groups ? ACC_BAD_GROUP : ACC_COUNTED); }
// the trailer word of a kind >= ACC_IGNORED
__device__ __forceinline__ long long* acc_trailer_word(long long* acc, int row_words, int n_groups, int kind) {
  return acc_trailer(acc, row_words, n_groups) + (kind - ACC_IGNORED);
}
// the same for the kernels that decide per thread (or per wave, per workgroup): the trailer word to bump, nullptr when the pose is scored
__device__ __forceinline__ long long* acc_refused(long long* acc, int row_words, int n_groups, int g) {
  const int kind = acc_group_kind(g, n_groups);
  return kind == ACC_COUNTED ? nullptr : acc_trailer_word(acc, row_words, n_groups, kind);
}

// ---- the entry points' half -----------------------------------------------------------------------------------------------------
inline bool acc_aligned(const void* acc, const void* second = nullptr) { return (((uintptr_t)acc | (uintptr_t)second) & 7) == 0; }
inline bool acc_groups_ok(int n_groups) { return n_groups >= 1 && n_groups <= JRR_EVAL_ACC_MAX_GROUPS; }
// sets `FN: n_groups N: 1 .. MAX` and returns true when n_groups is out of range (depth, pen and boot word the range of a second
// number into the same sentence: they call acc_groups_ok)
inline bool acc_groups_refused(const char* fn, int n_groups) {
  if (acc_groups_ok(n_groups)) return false;
  jrr_set_error("%s: n_groups %d: 1 .. %d", fn, n_groups, (int)JRR_EVAL_ACC_MAX_GROUPS);
  return true;
}

}  // namespace jrr
