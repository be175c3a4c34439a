// Bone length and direction errors of the 17-joint skeleton (`--eval_bones`): what the skeleton IS, beside the reports that say how
// far its joints are.  Two launches, no engine, no body model, no reference counterpart; include/jrr.h (jrr_bone_error,
// jrr_bone_accumulate, JRR_BONE_*) is the specification.
//
// k_bone_error       one pose per thread, as k_evaluate_joints (evalrep.hip): the pose's 2 x 51 floats in registers, centred on the pelvis;
//                    the moments of the 17 joints in evalk.h's statement order, the rotation by procrustes_fit (procfit.h; its scale and
//                    translation are dead code here); then the 16 bones in ascending order, each with a STATIC parent (bone_step<J>: a
//                    template constant, so no array is indexed at run time and nothing goes to scratch memory).  The
//                    two rebuilt skeletons need only the parent's point, and a parent is the previous joint, the pelvis (0) or the
//                    neck (8): the compiler keeps three points of each alive, not seventeen.
//                    A pose's row is 392 bytes, so a thread's own stores would be 98 scattered dwords: the 64 rows of a workgroup are
//                    one contiguous piece of the output, assembled in LDS (stride 99 floats: odd, conflict-free) and stored as
//                    coalesced dwords.  Every branch is per lane, no value crosses lanes.
// k_bone_accumulate  a workgroup owns 64 poses and stages their rows in LDS; then one thread per WORD of the table row walks the poses and
//                    sums its word in a register, and adds the sum with one atomic whenever the group changes (a pose-per-thread
//                    version spent 0.4 ms at batch 256 on 200 atomics per pose that all met in the same 192 words).  Integer adds
//                    commute and associate: the table is exact whatever the grouping, and a function of the multiset of poses alone.
// Every floating-point operation is rounded once, in the order written (contraction is off for the whole unit, procfit.h included), so
// a host restatement follows it.
#pragma clang fp contract(off)
#include "jrr_common.h"
#include "../../include/jrr.h"
#include "procfit.h"
#include "acctab.h"
#include <utility>

namespace jrr {

constexpr int BN_POSES = 64;                       // poses per workgroup of k_bone_error: one wave
constexpr int BN_VALS = JRR_BONE_VALS;             // 98 floats per pose
constexpr int BN_STRIDE = BN_VALS + 1;             // LDS stride of a pose's row: odd
constexpr int BN_ACC_THREADS = 256;                // k_bone_accumulate: 64 poses per workgroup as well, one thread per table word
constexpr int NBONE = JRR_BONE_BONES;

static_assert(NH == 17 && NBONE == NH - 1 && BN_VALS == 4 * NBONE + 2 * NH, "98 values per pose");
static_assert(JRR_BONE_LEN_GT == JRR_BONE_LEN_PRED + NBONE && JRR_BONE_ANG == JRR_BONE_LEN_GT + NBONE && JRR_BONE_ANG_PA == JRR_BONE_ANG + NBONE &&
              JRR_BONE_ERR_DIR == JRR_BONE_ANG_PA + NBONE && JRR_BONE_ERR_LEN == JRR_BONE_ERR_DIR + NH && BN_VALS == JRR_BONE_ERR_LEN + NH, "value layout");
static_assert(JRR_BONE_ACC_SUM_LEN_PRED == 2 && JRR_BONE_ACC_SUM_LEN_GT == JRR_BONE_ACC_SUM_LEN_PRED + NBONE &&
              JRR_BONE_ACC_SUM_ABS_DLEN == JRR_BONE_ACC_SUM_LEN_GT + NBONE && JRR_BONE_ACC_SUM_ANG == JRR_BONE_ACC_SUM_ABS_DLEN + NBONE &&
              JRR_BONE_ACC_SUM_ANG_PA == JRR_BONE_ACC_SUM_ANG + NBONE && JRR_BONE_ACC_SUM_SQ_PRED == JRR_BONE_ACC_SUM_ANG_PA + NBONE &&
              JRR_BONE_ACC_SUM_SQ_GT == JRR_BONE_ACC_SUM_SQ_PRED + NBONE && JRR_BONE_ACC_SUM_Q_PRED == JRR_BONE_ACC_SUM_SQ_GT + NBONE &&
              JRR_BONE_ACC_SUM_Q_GT == JRR_BONE_ACC_SUM_Q_PRED + NBONE && JRR_BONE_ACC_SUM_ERR_DIR == JRR_BONE_ACC_SUM_Q_GT + NBONE &&
              JRR_BONE_ACC_SUM_ERR_LEN == JRR_BONE_ACC_SUM_ERR_DIR + NH && JRR_BONE_ACC_SUM_ASYM_PRED == JRR_BONE_ACC_SUM_ERR_LEN + NH &&
              JRR_BONE_ACC_SUM_ASYM_GT == JRR_BONE_ACC_SUM_ASYM_PRED + JRR_BONE_PAIRS &&
              JRR_BONE_ACC_ROW == JRR_BONE_ACC_SUM_ASYM_GT + JRR_BONE_PAIRS && JRR_BONE_ACC_TRAILER == JRR_EVAL_ACC_TRAILER, "row layout");
static_assert(JRR_BONE_ACC_ROW + JRR_BONE_ACC_TRAILER <= BN_ACC_THREADS && BN_POSES <= BN_ACC_THREADS, "one thread per word of the row and of the trailer");

// parent = { -1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15 }: the previous joint, but for the chains' roots
__host__ __device__ constexpr int bone_parent(int j) { return (j == 1 || j == 4 || j == 7) ? 0 : ((j == 11 || j == 14) ? 8 : j - 1); }
// the six (left, right) pairs of bones: (4,1) (5,2) (6,3) (11,14) (12,15) (13,16)
__host__ __device__ constexpr int pair_left(int p) { return p < 3 ? 4 + p : 8 + p; }
__host__ __device__ constexpr int pair_right(int p) { return p < 3 ? 1 + p : 11 + p; }
static_assert(bone_parent(16) == 15 && bone_parent(14) == 8 && bone_parent(11) == 8 && bone_parent(7) == 0 && bone_parent(8) == 7, "parents");
static_assert(pair_left(0) == 4 && pair_right(0) == 1 && pair_left(3) == 11 && pair_right(3) == 14 && pair_left(5) == 13 && pair_right(5) == 16, "pairs");

__device__ __forceinline__ float bn_len(const float w[3]) { return sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]); }
__device__ __forceinline__ float bn_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ float bn_angle(const float a[3], const float b[3]) {
  float x[3];
  cross3(a, b, x);
  return atan2f(bn_len(x), bn_dot(a, b));
}

// bone J: its four values, and joint J of the two rebuilt skeletons.  J is a template constant so that every index is static (an
// unrolled loop over the bones did not fold: P and Q went to scratch memory).
template <int J>
__device__ __forceinline__ void bone_step(const float (&P)[NH][3], const float (&Q)[NH][3], const float (&R)[3][3], float (&xd)[NH][3],
                                          float (&xl)[NH][3], float* row) {
  constexpr int p = bone_parent(J);
  float u[3], v[3], ru[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { u[c] = P[J][c] - P[p][c]; v[c] = Q[J][c] - Q[p][c]; }
  const float lp = bn_len(u), lg = bn_len(v);
#pragma unroll
  for (int r = 0; r < 3; ++r) ru[r] = (R[r][0] * u[0] + R[r][1] * u[1]) + R[r][2] * u[2];
  row[JRR_BONE_LEN_PRED + J - 1] = lp;
  row[JRR_BONE_LEN_GT + J - 1] = lg;
  row[JRR_BONE_ANG + J - 1] = bn_angle(u, v);
  row[JRR_BONE_ANG_PA + J - 1] = bn_angle(ru, v);
  const float sd = lg / lp, sl = lp / lg;
  float dd[3], dl[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    xd[J][c] = xd[p][c] + u[c] * sd;
    xl[J][c] = xl[p][c] + v[c] * sl;
    dd[c] = xd[J][c] - Q[J][c];
    dl[c] = xl[J][c] - Q[J][c];
  }
  row[JRR_BONE_ERR_DIR + J] = bn_len(dd);
  row[JRR_BONE_ERR_LEN + J] = bn_len(dl);
}
template <int... I>
__device__ __forceinline__ void bone_steps(const float (&P)[NH][3], const float (&Q)[NH][3], const float (&R)[3][3], float (&xd)[NH][3],
                                           float (&xl)[NH][3], float* row, std::integer_sequence<int, I...>) {
  (bone_step<I + 1>(P, Q, R, xd, xl, row), ...);   // bones 1 .. 16 in ascending order: a parent comes before its child
}

// grid: ceil(B / 64) workgroups of 64 threads
__global__ __launch_bounds__(BN_POSES) void k_bone_error(const float* __restrict__ pred, const float* __restrict__ target_mm,
                                                         float* __restrict__ vals, int B) {
  __shared__ float s_out[BN_POSES * BN_STRIDE];    // 25 344 B
  const int tid = threadIdx.x, b0 = (int)blockIdx.x * BN_POSES, b = b0 + tid;
  if (b < B) {
    float* row = s_out + tid * BN_STRIDE;
    float P[NH][3], Q[NH][3];
#pragma unroll
    for (int i = 0; i < NH; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        P[i][c] = pred[((size_t)b * NH + i) * 3 + c];
        Q[i][c] = target_mm[((size_t)b * NH + i) * 3 + c] / 1000.f;
      }
#pragma unroll
    for (int i = NH - 1; i >= 0; --i)              // x = P - P[0], y = q - q[0]; joint 0 last, so that every joint meets the same pelvis
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        P[i][c] -= P[0][c];
        Q[i][c] -= Q[0][c];
      }
    // the moments of the similarity fit, in evalk.h's statement order
    float mu1[3] = {0.f, 0.f, 0.f}, mu2[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NH; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) { mu1[c] += P[i][c]; mu2[c] += Q[i][c]; }
#pragma unroll
    for (int c = 0; c < 3; ++c) { mu1[c] /= NH; mu2[c] /= NH; }
    float K[3][3] = {{0.f}}, var1 = 0.f;
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      float x1[3], x2[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { x1[c] = P[i][c] - mu1[c]; x2[c] = Q[i][c] - mu2[c]; var1 += x1[c] * x1[c]; }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) K[r][c] += x1[r] * x2[c];
    }
    float R[3][3], scale, t[3];
    procrustes_fit(K, var1, mu1, mu2, R, scale, t);

    float xd[NH][3], xl[NH][3];                    // the direction-only and the length-only skeleton; static indices throughout
#pragma unroll
    for (int c = 0; c < 3; ++c) xd[0][c] = xl[0][c] = 0.f;
    row[JRR_BONE_ERR_DIR] = 0.f;
    row[JRR_BONE_ERR_LEN] = 0.f;
    bone_steps(P, Q, R, xd, xl, row, std::make_integer_sequence<int, NBONE>{});
  }
  __syncthreads();
  const int n = min(BN_POSES, B - b0) * BN_VALS;   // floats of this workgroup's piece
  float* dst = vals + (size_t)b0 * BN_VALS;
  for (int q = tid; q < n; q += BN_POSES) {
    const int pose = q / BN_VALS, k = q - pose * BN_VALS;
    dst[q] = s_out[pose * BN_STRIDE + k];
  }
}

enum { BN_FIXED = 0, BN_ABS_DIFF = 1, BN_SQUARE = 2, BN_Q = 3, BN_KIND = 4 };      // what a word sums

// grid: ceil(B / 64) workgroups of 256 threads; workgroup t owns poses 64 t .. 64 t + 63.  Thread w < 192 owns WORD w of the row, thread
// 192 / 193 the two trailer words: it walks the tile's poses in order and sums its word's contributions in a register for as long as the
// group stays the same, then adds the sum with ONE atomic (a tile of one group: 194 atomics at most; of alternating groups: as many as
// a pose-per-thread kernel would issue, spread over 192 lanes).  No atomic meets another of its own workgroup on the way.
__global__ __launch_bounds__(BN_ACC_THREADS) void k_bone_accumulate(const float* __restrict__ vals, const int* __restrict__ group, int n_groups,
                                                                    long long* __restrict__ acc, int B) {
  __shared__ float s_v[BN_POSES * BN_STRIDE];      // 25 344 B: the tile's rows, stride 99 floats
  __shared__ int s_kind[BN_POSES], s_gid[BN_POSES];
  const int tid = threadIdx.x, b0 = (int)blockIdx.x * BN_POSES, np = min(BN_POSES, B - b0);
  const float* src = vals + (size_t)b0 * BN_VALS;
  for (int q = tid; q < np * BN_VALS; q += BN_ACC_THREADS) {      // coalesced dwords
    const int pose = q / BN_VALS, k = q - pose * BN_VALS;
    s_v[pose * BN_STRIDE + k] = src[q];
  }
  __syncthreads();
  if (tid < np) {                                  // what each pose is to the table
    const int gid = group ? group[b0 + tid] : 0;
    int kind = acc_group_kind(gid, n_groups);
    if (kind == ACC_COUNTED) {
      bool good = true;
      for (int i = 0; i < BN_VALS; ++i) good = good && (s_v[tid * BN_STRIDE + i] < ERR_CAP);      // false for NaN
      kind = good ? ACC_COUNTED : ACC_BAD;
    }
    s_kind[tid] = kind;
    s_gid[tid] = gid;
  }
  __syncthreads();
  const int w = tid;
  if (w >= JRR_BONE_ACC_ROW + JRR_BONE_ACC_TRAILER) return;
  if (w >= JRR_BONE_ACC_ROW) {                     // the trailer: poses ignored on purpose, poses with a group outside the table
    const int want = ACC_IGNORED + (w - JRR_BONE_ACC_ROW);
    int n = 0;
    for (int p = 0; p < np; ++p) n += s_kind[p] == want;
    if (n) acc_add(acc_trailer_word(acc, JRR_BONE_ACC_ROW, n_groups, want), n);
    return;
  }
  // what word w sums: one value, |difference of two|, q * q or q of one
  int cls = BN_KIND, a = 0, c = 0;
  if (w >= JRR_BONE_ACC_SUM_ASYM_PRED) {
    const bool gt = w >= JRR_BONE_ACC_SUM_ASYM_GT;
    const int pr = w - (gt ? JRR_BONE_ACC_SUM_ASYM_GT : JRR_BONE_ACC_SUM_ASYM_PRED), base = gt ? JRR_BONE_LEN_GT : JRR_BONE_LEN_PRED;
    cls = BN_ABS_DIFF; a = base + pair_left(pr) - 1; c = base + pair_right(pr) - 1;
  } else if (w >= JRR_BONE_ACC_SUM_ERR_LEN) { cls = BN_FIXED; a = JRR_BONE_ERR_LEN + (w - JRR_BONE_ACC_SUM_ERR_LEN); }
  else if (w >= JRR_BONE_ACC_SUM_ERR_DIR) { cls = BN_FIXED; a = JRR_BONE_ERR_DIR + (w - JRR_BONE_ACC_SUM_ERR_DIR); }
  else if (w >= JRR_BONE_ACC_SUM_Q_GT) { cls = BN_Q; a = JRR_BONE_LEN_GT + (w - JRR_BONE_ACC_SUM_Q_GT); }
  else if (w >= JRR_BONE_ACC_SUM_Q_PRED) { cls = BN_Q; a = JRR_BONE_LEN_PRED + (w - JRR_BONE_ACC_SUM_Q_PRED); }
  else if (w >= JRR_BONE_ACC_SUM_SQ_GT) { cls = BN_SQUARE; a = JRR_BONE_LEN_GT + (w - JRR_BONE_ACC_SUM_SQ_GT); }
  else if (w >= JRR_BONE_ACC_SUM_SQ_PRED) { cls = BN_SQUARE; a = JRR_BONE_LEN_PRED + (w - JRR_BONE_ACC_SUM_SQ_PRED); }
  else if (w >= JRR_BONE_ACC_SUM_ANG_PA) { cls = BN_FIXED; a = JRR_BONE_ANG_PA + (w - JRR_BONE_ACC_SUM_ANG_PA); }
  else if (w >= JRR_BONE_ACC_SUM_ANG) { cls = BN_FIXED; a = JRR_BONE_ANG + (w - JRR_BONE_ACC_SUM_ANG); }
  else if (w >= JRR_BONE_ACC_SUM_ABS_DLEN) { cls = BN_ABS_DIFF; a = JRR_BONE_LEN_PRED + (w - JRR_BONE_ACC_SUM_ABS_DLEN); c = JRR_BONE_LEN_GT + (w - JRR_BONE_ACC_SUM_ABS_DLEN); }
  else if (w >= JRR_BONE_ACC_SUM_LEN_GT) { cls = BN_FIXED; a = JRR_BONE_LEN_GT + (w - JRR_BONE_ACC_SUM_LEN_GT); }
  else if (w >= JRR_BONE_ACC_SUM_LEN_PRED) { cls = BN_FIXED; a = JRR_BONE_LEN_PRED + (w - JRR_BONE_ACC_SUM_LEN_PRED); }
  long long sum = 0;
  int cur = 0;                                     // the group `sum` belongs to (sum == 0: none yet)
  for (int p = 0; p < np; ++p) {                   // uniform over the workgroup: every thread sees the same kinds and groups
    const int kind = s_kind[p];
    if (kind >= ACC_IGNORED) continue;
    const int g = s_gid[p];                        // 0 <= g < n_groups
    if (g != cur) {
      if (sum != 0) acc_add(acc_row(acc, JRR_BONE_ACC_ROW, cur) + w, sum);
      sum = 0;
      cur = g;
    }
    const float* v = s_v + p * BN_STRIDE;
    if (cls == BN_KIND) sum += (kind == (w == JRR_BONE_ACC_COUNT ? ACC_COUNTED : ACC_BAD)) ? 1 : 0;
    else if (kind == ACC_COUNTED) {
      if (cls == BN_FIXED) sum += err_fixed24(v[a]);
      else if (cls == BN_ABS_DIFF) sum += err_fixed24(fabsf(v[a] - v[c]));
      else {
        const long long q = __float2ll_rn(v[a] * 65536.f);
        sum += cls == BN_SQUARE ? q * q : q;
      }
    }
  }
  if (sum != 0) acc_add(acc_row(acc, JRR_BONE_ACC_ROW, cur) + w, sum);
}

}  // namespace jrr

using namespace jrr;

extern "C" int jrr_bone_error(const float* pred, const float* target_mm, int batch, float* vals, void* stream) {
  const char* why = nullptr;
  if (!pred || !target_mm) why = "bad argument (pred and target_mm are required)";
  else if (!vals) why = "no output: vals is NULL";
  else if (batch < 0) why = "batch must not be negative";
  else if ((((uintptr_t)pred | (uintptr_t)target_mm | (uintptr_t)vals) & 3) != 0) why = "pred, target_mm and vals must be 4-byte aligned";
  if (why) {
    jrr_set_error("jrr_bone_error: %s", why);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  hipLaunchKernelGGL(k_bone_error, dim3((unsigned)((batch + BN_POSES - 1) / BN_POSES)), dim3(BN_POSES), 0, (hipStream_t)stream, pred, target_mm,
                     vals, batch);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_bone_accumulate(const float* vals, const int32_t* group, int batch, int n_groups, int64_t* acc, void* stream) {
  const char* why = nullptr;
  if (!vals || !acc) why = "bad argument (vals and acc are required)";
  else if (batch < 0) why = "batch must not be negative";
  else if ((((uintptr_t)vals | (uintptr_t)group) & 3) != 0 || !acc_aligned(acc))
    why = "vals and group must be 4-byte aligned, acc 8-byte aligned";
  if (why) {
    jrr_set_error("jrr_bone_accumulate: %s", why);
    return JRR_ERR_ARG;
  }
  if (acc_groups_refused("jrr_bone_accumulate", n_groups)) return JRR_ERR_ARG;
  if (batch == 0) return JRR_OK;
  hipLaunchKernelGGL(k_bone_accumulate, dim3((unsigned)((batch + BN_POSES - 1) / BN_POSES)), dim3(BN_ACC_THREADS), 0,
                     (hipStream_t)stream, vals, group, n_groups, reinterpret_cast<long long*>(acc), batch);
  CHECK_LAUNCH();
  return JRR_OK;
}
