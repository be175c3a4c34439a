// The evaluation report under a published protocol (`--eval_protocol`): which joints are scored, where both skeletons are centred
// and in which unit the target comes.  One launch, no engine, no body model:
//
// k_evaluate_protocol    per pose the distances and the Procrustes-aligned distances of the joints of `joint_mask` (M, n = |M|), in
//                        metres, and -- when a table is given -- their addition to the JRR_EVAL_ACC_* table in the same launch.
//                        One pose per thread as k_evaluate_joints (evalrep.hip): 64 poses per workgroup, rows assembled in LDS with
//                        stride 17 and stored 16 bytes per lane with the ragged tail.  The mask, the root and the unit are kernel
//                        arguments, uniform across the wave: every loop over the joints is unrolled under a uniform predicate, so
//                        every joint index is static (no indexed register array, no scratch memory).
//                        A joint that is neither in M nor a root joint is never LOADED: a NaN there changes no output bit (a
//                        regressor row without a positive entry gives NaN joints).  A joint outside M gets +0.0f in both outputs.
//                        The Procrustes statements are those of evalk.h with NH replaced by M: means divided by (float)n, K and var1
//                        summed over M in ascending order, the one-sided Jacobi on K (six sweeps), the static sort and the rank-2 /
//                        rank-1 / rank-0 rules, through evalk.h's own helpers.
//                        The accumulation is k_eval_accumulate's (evalrep.hip) over M alone, through fixedpt.h and acctab.h; each
//                        thread reads back the row it wrote to LDS itself.
#include "jrr_common.h"
#include "evalk.h"
#include "fixedpt.h"
#include "acctab.h"
#include "../../include/jrr.h"

namespace jrr {

constexpr int EP_POSES = 64;                       // poses per workgroup: one wave
constexpr int EP_ROWF = EP_POSES * NH;             // 1088 floats = 272 float4 per output and workgroup
static_assert(EP_ROWF % 4 == 0, "a workgroup's piece of err_j is a whole number of 16-byte stores");
static_assert(JRR_EVAL_MASK_ALL == (1 << NH) - 1 && NH == 17, "one bit per H36M joint");

__global__ __launch_bounds__(EP_POSES) void k_evaluate_protocol(const float* __restrict__ pred, const float* __restrict__ target,
                                                                int target_unit, unsigned mask, int root, const int* __restrict__ group,
                                                                int n_groups, float* __restrict__ err_j, float* __restrict__ err_pa_j,
                                                                long long* __restrict__ acc, int B) {
  __shared__ float4 s_out4[2][EP_ROWF / 4];
  float* s_plain = reinterpret_cast<float*>(s_out4[0]);
  float* s_pa = reinterpret_cast<float*>(s_out4[1]);
  const int tid = threadIdx.x, b0 = (int)blockIdx.x * EP_POSES, b = b0 + tid;
  const bool hips = root == JRR_EVAL_ROOT_HIPS, metres = target_unit == JRR_EVAL_TARGET_M;
  const float n = (float)__popc(mask);
#define EP_IN(i) (((mask >> (i)) & 1u) != 0u)
  if (b < B) {
    float* row = s_plain + tid * NH;
    float* row_pa = s_pa + tid * NH;
    float P[NH][3], Q[NH][3];
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      const bool is_root = hips ? (i == 1 || i == 4) : i == 0;
      if (EP_IN(i) || is_root) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          P[i][c] = pred[((size_t)b * NH + i) * 3 + c];
          const float q = target[((size_t)b * NH + i) * 3 + c];
          Q[i][c] = metres ? q : q / 1000.f;
        }
      } else {                                     // never read below: the registers only need a value
#pragma unroll
        for (int c = 0; c < 3; ++c) { P[i][c] = 0.f; Q[i][c] = 0.f; }
      }
    }
    // centre both on the root (joint 0, or the midpoint of the hips), the plain distance
    float rP[3], rQ[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      rP[c] = hips ? (P[1][c] + P[4][c]) * 0.5f : P[0][c];
      rQ[c] = hips ? (Q[1][c] + Q[4][c]) * 0.5f : Q[0][c];
    }
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      float e = 0.f;
      if (EP_IN(i)) {
        float d2 = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          P[i][c] -= rP[c];
          Q[i][c] -= rQ[c];
          const float d = P[i][c] - Q[i][c];
          d2 += d * d;
        }
        e = sqrtf(d2);
      }
      row[i] = e;
    }
    // Procrustes over M: remove means, K = sum_M x1 x2^T
    float mu1[3] = {0.f, 0.f, 0.f}, mu2[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NH; ++i)
      if (EP_IN(i)) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { mu1[c] += P[i][c]; mu2[c] += Q[i][c]; }
      }
#pragma unroll
    for (int c = 0; c < 3; ++c) { mu1[c] /= n; mu2[c] /= n; }
    float K[3][3] = {{0.f}}, var1 = 0.f;
#pragma unroll
    for (int i = 0; i < NH; ++i)
      if (EP_IN(i)) {
        float x1[3], x2[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { x1[c] = P[i][c] - mu1[c]; x2[c] = Q[i][c] - mu2[c]; var1 += x1[c] * x1[c]; }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) K[r][c] += x1[r] * x2[c];
      }
    // K = U diag(sigma) V^T by one-sided Jacobi on K itself (evalk.h): G = K V with orthogonal columns
    float G[3][3], V[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) G[r][c] = K[r][c];
    for (int sweep = 0; sweep < 6; ++sweep) {
      hestenes_rotate<0, 1>(G, V);
      hestenes_rotate<0, 2>(G, V);
      hestenes_rotate<1, 2>(G, V);
    }
    // sort singular values descending: a compare-exchange network on (sigma, column of G, column of V) with static indices
    float sig[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) sig[k] = sqrtf(G[0][k] * G[0][k] + G[1][k] * G[1][k] + G[2][k] * G[2][k]);
    auto cswap = [&](auto A_, auto B_) __attribute__((always_inline)) {
      constexpr int a = decltype(A_)::value, c = decltype(B_)::value;
      if (sig[a] < sig[c]) {
        const float t = sig[a]; sig[a] = sig[c]; sig[c] = t;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const float g = G[r][a]; G[r][a] = G[r][c]; G[r][c] = g;
          const float u = V[r][a]; V[r][a] = V[r][c]; V[r][c] = u;
        }
      }
    };
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
    cswap(I0{}, I1{}); cswap(I1{}, I2{}); cswap(I0{}, I1{});
    // R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T; rank 1 (sigma_2 <= 1e-6 sigma_1): u2, v2 completed orthogonally; rank 0: R = I
    float R[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
    if (sig[0] > 0.f) {
      float u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) { u1[r] = G[r][0] / sig[0]; v1[r] = V[r][0]; }
      if (sig[1] <= 1e-6f * sig[0]) {
        orthogonal_unit3(u1, u2);
        orthogonal_unit3(v1, v2);
      } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) { u2[r] = G[r][1] / sig[1]; v2[r] = V[r][1]; }
      }
      cross3(u1, u2, u3);
      unit3(u3);
      cross3(u3, u1, u2);
      cross3(v1, v2, v3);
      unit3(v3);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = v1[r] * u1[c] + v2[r] * u2[c] + v3[r] * u3[c];
    }
    // scale = trace(R K) / var1 ; t = mu2 - scale R mu1
    float tr = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) tr += R[r][0] * K[0][r] + R[r][1] * K[1][r] + R[r][2] * K[2][r];
    const float scale = tr / var1;
    float t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = mu2[r] - scale * (R[r][0] * mu1[0] + R[r][1] * mu1[1] + R[r][2] * mu1[2]);
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      float e = 0.f;
      if (EP_IN(i)) {
        float d2 = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const float h = scale * (R[r][0] * P[i][0] + R[r][1] * P[i][1] + R[r][2] * P[i][2]) + t[r];
          const float d = h - Q[i][r];
          d2 += d * d;
        }
        e = sqrtf(d2);
      }
      row_pa[i] = e;
    }
    // the table: k_eval_accumulate's expressions over M alone, on the row this thread has just written
    if (acc) {
      const int g = group ? group[b] : 0;
      if (long long* tw = acc_refused(acc, JRR_EVAL_ACC_ROW, n_groups, g)) {
        acc_add(tw, 1);
      } else {
        long long* arow = acc_row(acc, JRR_EVAL_ACC_ROW, g);
        bool good = true;
        for (int i = 0; i < NH; ++i)
          if (EP_IN(i)) good = good && (row[i] < ERR_CAP) && (row_pa[i] < ERR_CAP);       // false for NaN
        if (!good) {
          acc_add(arow + JRR_EVAL_ACC_BAD, 1);
        } else {
          acc_add(arow + JRR_EVAL_ACC_COUNT, 1);
          for (int i = 0; i < NH; ++i) {
            if (!EP_IN(i)) continue;
#pragma unroll
            for (int o = 0; o < 2; ++o) {
              const float e = o == 0 ? row[i] : row_pa[i];
              acc_add(arow + (o == 0 ? JRR_EVAL_ACC_SUM : JRR_EVAL_ACC_SUM_PA) + i, err_fixed24(e));
              const int bin = max(min((int)floorf(e * 1000.f), JRR_EVAL_ACC_BINS - 1), 0);
              acc_add(arow + (o == 0 ? JRR_EVAL_ACC_HIST : JRR_EVAL_ACC_HIST_PA) + bin, 1);
            }
          }
        }
      }
    }
  }
#undef EP_IN
  __syncthreads();
  const int nf = min(EP_POSES, B - b0) * NH;         // floats of this workgroup's piece (a ragged last one: any multiple of 17)
  const size_t base = (size_t)b0 * NH;               // b0 * 68 bytes: a multiple of 4352
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    float* out = o == 0 ? err_j : err_pa_j;
    if (!out) continue;
    float* dst = out + base;
    const float* src = reinterpret_cast<const float*>(s_out4[o]);
    for (int q = tid; q < nf / 4; q += EP_POSES) reinterpret_cast<float4*>(dst)[q] = s_out4[o][q];
    const int tail = nf & ~3;
    if (tid < nf - tail) dst[tail + tid] = src[tail + tid];
  }
}

}  // namespace jrr

using namespace jrr;

/* the evaluation report under a protocol (--eval_protocol): masked per-joint errors and their table in one launch */
extern "C" int jrr_evaluate_protocol(const float* pred, const float* target, int target_unit, uint32_t joint_mask, int root,
                                     const int32_t* group, int batch, int n_groups, float* err_j, float* err_pa_j, int64_t* acc,
                                     void* stream) {
  if (!pred || !target) {
    jrr_set_error("jrr_evaluate_protocol: pred and target must not be NULL");
    return JRR_ERR_ARG;
  }
  if (!err_j && !err_pa_j && !acc) {
    jrr_set_error("jrr_evaluate_protocol: no output: err_j, err_pa_j and acc are all NULL");
    return JRR_ERR_ARG;
  }
  if (joint_mask == 0 || (joint_mask & ~(uint32_t)JRR_EVAL_MASK_ALL) != 0) {
    jrr_set_error("jrr_evaluate_protocol: joint_mask 0x%x: at least one of the 17 joint bits, none at or above bit 17", (unsigned)joint_mask);
    return JRR_ERR_ARG;
  }
  if (root != JRR_EVAL_ROOT_JOINT0 && root != JRR_EVAL_ROOT_HIPS) {
    jrr_set_error("jrr_evaluate_protocol: root %d: JRR_EVAL_ROOT_JOINT0 or JRR_EVAL_ROOT_HIPS", root);
    return JRR_ERR_ARG;
  }
  if (target_unit != JRR_EVAL_TARGET_MM && target_unit != JRR_EVAL_TARGET_M) {
    jrr_set_error("jrr_evaluate_protocol: target_unit %d: JRR_EVAL_TARGET_MM or JRR_EVAL_TARGET_M", target_unit);
    return JRR_ERR_ARG;
  }
  if (batch < 0) {
    jrr_set_error("jrr_evaluate_protocol: batch %d is negative", batch);
    return JRR_ERR_ARG;
  }
  if (acc && acc_groups_refused("jrr_evaluate_protocol", n_groups)) return JRR_ERR_ARG;
  if ((((uintptr_t)err_j | (uintptr_t)err_pa_j) & 15) != 0 || !acc_aligned(acc)) {
    jrr_set_error("jrr_evaluate_protocol: err_j and err_pa_j must be 16-byte aligned, acc 8-byte aligned");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  hipLaunchKernelGGL(k_evaluate_protocol, dim3((unsigned)((batch + EP_POSES - 1) / EP_POSES)), dim3(EP_POSES), 0, (hipStream_t)stream, pred, target,
                     target_unit, (unsigned)joint_mask, root, group, n_groups, err_j, err_pa_j, reinterpret_cast<long long*>(acc), batch);
  CHECK_LAUNCH();
  return JRR_OK;
}
