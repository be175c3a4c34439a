// The acceleration error along each video sequence (`--eval_accel`): how far the second difference of the predicted joints' motion is
// from the ground truth's, per position of a time order (the lists refined.sequence_runs forms), and its int64 table per group.
// One launch, no engine, no body model, no reference counterpart; include/jrr.h (jrr_accel_error, JRR_ACCEL_*) is the specification.
//
// k_accel_error: a workgroup owns AC_TILE = 32 consecutive positions.  It checks the 32 + 2 entries of `order` around them (slot ->
//   table row or -1), stages the 51 floats of each of those rows of both tables ONCE in LDS (204 contiguous bytes per row, 4-byte
//   coalesced loads; the ground truth already divided by 1000), and works with one thread per (position, joint):
//     x = P - P[0], y = G / 1000 - (G / 1000)[0] per frame;  a = (x[p-1] - 2 x[p]) + x[p+1];  e = |a_pred - a_gt|, s = |a_pred|, g = |a_gt|,
//   NaN where the position has no triple.  The tile's 32 x 17 values of each output are one contiguous piece and thread (position,
//   joint) holds its float number 17 position + joint: they leave as coalesced 4-byte stores.
//   The table: one thread per position decides what the position is (ignored, group out of range, no triple, bad, counted); the
//   (position, joint) threads of a counted one add three fixed-point sums and one bin.  Positions of the tile's FIRST in-range group add
//   into an LDS copy of that group's row (ds atomics), which leaves as at most 205 global atomics per workgroup; positions of any
//   other group add to global memory directly.  Integer adds commute: the table is exact either way, and a function of the multiset
//   of positions alone.
//   A position's result is a function of its triple: slots are addressed relative to the position, nothing depends on M, on the
//   position's place in the tile or on the launch's position range.
// Every floating-point operation is rounded once, in the order written (no product is fused into a sum), so a host restatement
// follows it.
#include "jrr_common.h"
#include "acctab.h"
#include "../../include/jrr.h"

namespace jrr {

constexpr int AC_TILE = JRR_ACCEL_TILE;            // positions per workgroup
constexpr int AC_NS = AC_TILE + 2;                 // slots a tile can see: a halo of 1
constexpr int AC_ROWF = NH * 3;                    // 51 floats per table row
constexpr int AC_THREADS = AC_TILE * NH;           // 544: one thread per (position, joint)
constexpr float AC_FIXED = 16777216.f;             // 2^24
constexpr int AC_NO_TRIPLE = 2;                    // the kind of its own beside acctab.h's: in range, lands in the row's NO_TRIPLE word
static_assert(AC_NO_TRIPLE > ACC_BAD && AC_NO_TRIPLE < ACC_IGNORED, "a kind of the row");

static_assert(JRR_ACCEL_ACC_SUM_ERR == 3 && JRR_ACCEL_ACC_SUM_PRED == JRR_ACCEL_ACC_SUM_ERR + NH &&
              JRR_ACCEL_ACC_SUM_GT == JRR_ACCEL_ACC_SUM_PRED + NH && JRR_ACCEL_ACC_HIST == JRR_ACCEL_ACC_SUM_GT + NH &&
              JRR_ACCEL_ACC_ROW == JRR_ACCEL_ACC_HIST + JRR_ACCEL_ACC_BINS && JRR_ACCEL_ACC_BINS == JRR_EVAL_ACC_BINS &&
              JRR_ACCEL_ACC_TRAILER == JRR_EVAL_ACC_TRAILER, "row layout");
static_assert(AC_THREADS <= 1024 && AC_TILE <= AC_THREADS, "tile shape");

#pragma clang fp contract(off)

__device__ __forceinline__ float ac_len(float v0, float v1, float v2) { return sqrtf((v0 * v0 + v1 * v1) + v2 * v2); }

// grid: ceil(count / 32) workgroups of 544 threads; workgroup b owns positions p0 = begin + 32 b .. min(p0 + 32, begin + count)
__global__ __launch_bounds__(AC_THREADS) void k_accel_error(const float* __restrict__ pred, const float* __restrict__ gt_mm, long long n_rows,
                                                            const int* __restrict__ order, const int* __restrict__ run,
                                                            const int* __restrict__ group, int M, int begin, int count, int n_groups,
                                                            float* __restrict__ err_j, float* __restrict__ acc_pred_j,
                                                            float* __restrict__ acc_gt_j, long long* __restrict__ acc,
                                                            int* __restrict__ status) {
  __shared__ float s_x[2][AC_NS * AC_ROWF];        // 13 872 B: pred | gt / 1000 of the staged rows
  __shared__ float s_out[3][AC_TILE * NH];         // 6 528 B: e | s | g of the tile
  __shared__ long long s_acc[JRR_ACCEL_ACC_ROW];   // 1 640 B: the row of s_group, summed on chip
  __shared__ int s_row[AC_NS], s_run[AC_NS];
  __shared__ int s_kind[AC_TILE], s_gid[AC_TILE];
  __shared__ int s_group;                          // the first in-range group of the tile, -1: none
  const int tid = threadIdx.x;
  const int p0 = begin + (int)blockIdx.x * AC_TILE;
  const int npos = min(AC_TILE, begin + count - p0);

  // slot i <-> position p0 - 1 + i: its table row (-1: outside [0, M), or refused with the status bit) and its run
  for (int i = tid; i < AC_NS; i += AC_THREADS) {
    const int p = p0 - 1 + i;
    int row = -1, r = 0;
    if (p >= 0 && p < M) {
      const int o = order[p];
      if (o < 0 || (long long)o >= n_rows) atomicOr(status, JRR_ACCEL_STATUS_INDEX);
      else { row = o; r = run[p]; }
    }
    s_row[i] = row;
    s_run[i] = r;
  }
  for (int i = tid; i < JRR_ACCEL_ACC_ROW; i += AC_THREADS) s_acc[i] = 0;
  __syncthreads();
  for (int i = tid; i < AC_NS * AC_ROWF; i += AC_THREADS) {
    const int slot = i / AC_ROWF, c = i - slot * AC_ROWF;
    const int row = s_row[slot];
    if (row >= 0) {
      s_x[0][i] = pred[(size_t)row * AC_ROWF + c];
      s_x[1][i] = gt_mm[(size_t)row * AC_ROWF + c] / 1000.f;
    }
  }
  __syncthreads();

  const float nanv = __int_as_float(0x7fc00000);
  const int pp = tid / NH, j = tid - pp * NH;      // thread (pp, j): joint j of position p0 + pp
  const int c = 1 + pp;
  float e = nanv, s = nanv, g = nanv;
  bool triple = false;
  if (pp < npos) {
    triple = s_row[c] >= 0 && s_row[c - 1] >= 0 && s_row[c + 1] >= 0 && s_run[c - 1] == s_run[c] && s_run[c + 1] == s_run[c];
    if (triple) {
      float a[2][3];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float* xa = s_x[t] + (c - 1) * AC_ROWF;
        const float* xb = s_x[t] + c * AC_ROWF;
        const float* xc = s_x[t] + (c + 1) * AC_ROWF;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float va = xa[j * 3 + k] - xa[k], vb = xb[j * 3 + k] - xb[k], vc = xc[j * 3 + k] - xc[k];
          a[t][k] = (va - 2.f * vb) + vc;
        }
      }
      e = ac_len(a[0][0] - a[1][0], a[0][1] - a[1][1], a[0][2] - a[1][2]);
      s = ac_len(a[0][0], a[0][1], a[0][2]);
      g = ac_len(a[1][0], a[1][1], a[1][2]);
    }
    s_out[0][tid] = e;
    s_out[1][tid] = s;
    s_out[2][tid] = g;
  }
  __syncthreads();

  // the per-position rows: thread (pp, j) holds float p0 * 17 + tid of each output, so the tile's piece leaves as coalesced stores
  if (pp < npos) {
    const size_t at = (size_t)p0 * NH + tid;
    if (err_j) err_j[at] = e;
    if (acc_pred_j) acc_pred_j[at] = s;
    if (acc_gt_j) acc_gt_j[at] = g;
  }
  if (!acc) return;                                // uniform

  // what each position is to the table
  if (tid < npos) {
    const int gid = group ? group[p0 + tid] : 0;
    int kind = acc_group_kind(gid, n_groups);
    if (kind == ACC_COUNTED) {
      const int cc = 1 + tid;
      const bool tr = s_row[cc] >= 0 && s_row[cc - 1] >= 0 && s_row[cc + 1] >= 0 && s_run[cc - 1] == s_run[cc] && s_run[cc + 1] == s_run[cc];
      if (!tr) kind = AC_NO_TRIPLE;
      else {
        bool good = true;
        for (int i = 0; i < NH; ++i)               // false for NaN
          good = good && (s_out[0][tid * NH + i] < ERR_CAP) && (s_out[1][tid * NH + i] < ERR_CAP) && (s_out[2][tid * NH + i] < ERR_CAP);
        kind = good ? ACC_COUNTED : ACC_BAD;
      }
    }
    s_kind[tid] = kind;
    s_gid[tid] = gid;
  }
  __syncthreads();
  if (tid == 0) {
    int first = -1;
    for (int i = 0; i < npos && first < 0; ++i)
      if (s_kind[i] <= AC_NO_TRIPLE) first = s_gid[i];
    s_group = first;
  }
  __syncthreads();

  if (tid < npos) {                                // one word per position
    const int kind = s_kind[tid], gid = s_gid[tid];
    if (kind >= ACC_IGNORED) acc_add(acc_trailer_word(acc, JRR_ACCEL_ACC_ROW, n_groups, kind), 1);
    else {
      const int w = kind == ACC_COUNTED ? JRR_ACCEL_ACC_COUNT : (kind == ACC_BAD ? JRR_ACCEL_ACC_BAD : JRR_ACCEL_ACC_NO_TRIPLE);
      if (gid == s_group) acc_add(s_acc + w, 1);
      else acc_add(acc_row(acc, JRR_ACCEL_ACC_ROW, gid) + w, 1);
    }
  }
  if (pp < npos && s_kind[pp] == ACC_COUNTED) {     // three sums and one bin per (position, joint)
    const int gid = s_gid[pp];
    const long long qe = __float2ll_rn(e * AC_FIXED), qs = __float2ll_rn(s * AC_FIXED), qg = __float2ll_rn(g * AC_FIXED);
    const int bin = min((int)floorf(e * 1000.f), JRR_ACCEL_ACC_BINS - 1);    // 0 <= e < the cap here: 0 <= bin
    if (gid == s_group) {                          // the two branches differ in the address space alone
      acc_add(s_acc + JRR_ACCEL_ACC_SUM_ERR + j, qe);
      acc_add(s_acc + JRR_ACCEL_ACC_SUM_PRED + j, qs);
      acc_add(s_acc + JRR_ACCEL_ACC_SUM_GT + j, qg);
      acc_add(s_acc + JRR_ACCEL_ACC_HIST + bin, 1);
    } else {
      long long* row = acc_row(acc, JRR_ACCEL_ACC_ROW, gid);
      acc_add(row + JRR_ACCEL_ACC_SUM_ERR + j, qe);
      acc_add(row + JRR_ACCEL_ACC_SUM_PRED + j, qs);
      acc_add(row + JRR_ACCEL_ACC_SUM_GT + j, qg);
      acc_add(row + JRR_ACCEL_ACC_HIST + bin, 1);
    }
  }
  __syncthreads();
  if (s_group >= 0 && tid < JRR_ACCEL_ACC_ROW) {
    const long long v = s_acc[tid];
    if (v != 0) acc_add(acc_row(acc, JRR_ACCEL_ACC_ROW, s_group) + tid, v);
  }
}

}  // namespace jrr

using namespace jrr;

extern "C" int jrr_accel_error(const float* pred, const float* gt_mm, int64_t n_rows, const int32_t* order, const int32_t* run,
                               const int32_t* group, int m, int begin, int count, int n_groups, float* err_j, float* acc_pred_j,
                               float* acc_gt_j, int64_t* acc, int32_t* status, void* stream) {
  const char* why = nullptr;
  if (!pred || !gt_mm || !order || !run || !status) why = "bad argument (pred, gt_mm, order, run and status are required)";
  else if (n_rows < 0 || n_rows > INT32_MAX || m < 0 || m > JRR_SMOOTH_MAX_POSITIONS) why = "n_rows must lie in 0 .. 2^31 - 1, m in 0 .. 2^30";
  else if (begin < 0 || count < 0 || begin > m || count > m - begin) why = "the position range must lie inside [0, m)";
  else if (!err_j && !acc_pred_j && !acc_gt_j && !acc) why = "no output: err_j, acc_pred_j, acc_gt_j and acc are all NULL";
  else if ((((uintptr_t)pred | (uintptr_t)gt_mm | (uintptr_t)order | (uintptr_t)run | (uintptr_t)group | (uintptr_t)status | (uintptr_t)err_j |
             (uintptr_t)acc_pred_j | (uintptr_t)acc_gt_j) & 3) != 0 || !acc_aligned(acc))
    why = "the float and int32 arrays must be 4-byte aligned, acc 8-byte aligned";
  if (why) {
    jrr_set_error("jrr_accel_error: %s", why);
    return JRR_ERR_ARG;
  }
  if (acc && acc_groups_refused("jrr_accel_error", n_groups)) return JRR_ERR_ARG;
  if (count == 0) return JRR_OK;
  hipLaunchKernelGGL(k_accel_error, dim3((unsigned)((count + AC_TILE - 1) / AC_TILE)), dim3(AC_THREADS), 0, (hipStream_t)stream, pred, gt_mm,
                     (long long)n_rows, order, run, group, m, begin, count, n_groups, err_j, acc_pred_j, acc_gt_j,
                     reinterpret_cast<long long*>(acc), status);
  CHECK_LAUNCH();
  return JRR_OK;
}
