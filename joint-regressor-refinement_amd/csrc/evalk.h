// `evaluate` for ONE pose, shared by k_evaluate (per-pose means, eval.hip) and k_evaluate_joints (the per-joint distances those
// means are formed from, evalrep.hip):
//   evaluate                                   scripts/utils.py:117-145 of the reference
//   batch_compute_similarity_transform_torch   scripts/eval_utils.py:7-58
// The 3x3 SVD of K = X1 X2^T is a one-sided (Hestenes) Jacobi iteration on K itself: six sweeps of plane rotations make the columns of
// G = K V orthogonal, so sigma_k = |g_k| and u_k = g_k / sigma_k, each as accurate RELATIVE TO ITSELF as float32 allows (K^T K is never
// formed: that would square the condition number, and a body is 0.15 x 0.5 x 0.05 m, a lifted or T pose nearly flat).  The rotation is
//   R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T,
// which is the reference's V diag(1, 1, sign det(U V^T)) U^T without a division by sigma_3 and without a determinant.  Guarantees:
//   rank 3, rank 2 (a flat pred, a flat target, both, mirrored or not): the unique proper rotation torch.svd + the sign fix reaches
//   rank 1 (sigma_2 <= 1e-6 sigma_1, a pred or a target on a line): u2, v2 completed orthogonally; the rotation about the line is not
//          defined, the 17 aligned distances are, and they are the reference's
//   rank 0 (K = 0): R = I; a constant target gives scale 0 and aligned distances of exactly 0, a constant pred 0/0 = NaN in its own 17
//          aligned distances (the reference's values) and finite plain distances
// Every branch is taken per lane and no value crosses lanes: a pose's result does not depend on its neighbours in the wave.
//
// Included normally, this header gives the helpers.  Included a second time INSIDE a kernel with JRR_EVAL_BODY defined, it expands
// to the body itself, as statements: the kernel has `pred`, `target_mm` and the pose index `b` in scope and says what happens to the
// distances through six macros --
//   JRR_EVAL_PLAIN_BEGIN / JRR_EVAL_PLAIN(i, d) / JRR_EVAL_PLAIN_END     joints i = 16 down to 0, d = |pred_i - target_i|
//   JRR_EVAL_PA_BEGIN    / JRR_EVAL_PA(i, d)    / JRR_EVAL_PA_END        joints i = 0 up to 16, d = |s R pred_i + t - target_i|
// A textual body and not an inlined function: the same statements wrapped in a __forceinline__ function cost k_evaluate 4 to 8 more
// registers (measured with the K^T K body it had then: 224 -> 228 / 232).  With the present body k_evaluate compiles to 224 VGPRs
// (as before it) and k_evaluate_joints to 252 (228 before), both at two waves per SIMD, without scratch memory or spills.
#ifndef JRR_EVAL_BODY
#ifndef JRR_EVALK_H
#define JRR_EVALK_H
#include "jrr_common.h"
#include <type_traits>

namespace jrr {

// One step of the one-sided (Hestenes) Jacobi iteration on columns p and q of G, accumulated in V: afterwards the two columns of G
// are orthogonal.  p and q are template constants so that every index is static (an index array would go to scratch memory).
template <int p, int q>
__device__ __forceinline__ void hestenes_rotate(float G[3][3], float V[3][3]) {
  const float al = G[0][p] * G[0][p] + G[1][p] * G[1][p] + G[2][p] * G[2][p];
  const float be = G[0][q] * G[0][q] + G[1][q] * G[1][q] + G[2][q] * G[2][q];
  const float ga = G[0][p] * G[0][q] + G[1][p] * G[1][q] + G[2][p] * G[2][q];
  if (!(fabsf(ga) > 1e-9f * (sqrtf(al) * sqrtf(be)))) return;   // orthogonal already (also: a zero column, NaN)
  const float zeta = (be - al) / (2.f * ga);
  const float t = copysignf(1.f, zeta) / (fabsf(zeta) + sqrtf(zeta * zeta + 1.f));
  const float c = 1.f / sqrtf(t * t + 1.f), s = t * c;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float gp = G[r][p], gq = G[r][q];
    G[r][p] = c * gp - s * gq;
    G[r][q] = s * gp + c * gq;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float vp = V[r][p], vq = V[r][q];
    V[r][p] = c * vp - s * vq;
    V[r][q] = s * vp + c * vq;
  }
}

__device__ __forceinline__ void cross3(const float a[3], const float b[3], float o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void unit3(float w[3]) {
  const float n = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  w[0] /= n; w[1] /= n; w[2] /= n;
}

// a unit vector orthogonal to the unit vector a: a x (the coordinate axis of a's smallest component), as a chain of selects
__device__ __forceinline__ void orthogonal_unit3(const float a[3], float o[3]) {
  const float ax = fabsf(a[0]), ay = fabsf(a[1]), az = fabsf(a[2]);
  const bool first = ax <= ay && ax <= az, second = ay <= az;
  o[0] = first ? 0.f : (second ? -a[2] : a[1]);
  o[1] = first ? a[2] : (second ? 0.f : -a[0]);
  o[2] = first ? -a[1] : (second ? a[0] : 0.f);
  unit3(o);
}

}  // namespace jrr
#endif  // JRR_EVALK_H

#else  // JRR_EVAL_BODY: the statements
  float P[NH][3], Q[NH][3];
#pragma unroll
  for (int i = 0; i < NH; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      P[i][c] = pred[((size_t)b * NH + i) * 3 + c];
      Q[i][c] = target_mm[((size_t)b * NH + i) * 3 + c] / 1000.f;
    }
  // pelvis-centre both (utils.py:127-131), MPJPE
  JRR_EVAL_PLAIN_BEGIN
#pragma unroll
  for (int i = NH - 1; i >= 0; --i) {
    float d2 = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      P[i][c] -= P[0][c];
      Q[i][c] -= Q[0][c];
      const float d = P[i][c] - Q[i][c];
      d2 += d * d;
    }
    JRR_EVAL_PLAIN(i, sqrtf(d2))
  }
  JRR_EVAL_PLAIN_END
  // Procrustes: remove means, K = sum_n x1 x2^T
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
  // K = U diag(sigma) V^T by one-sided Jacobi on K itself: G = K V with orthogonal columns, sigma_k = |g_k|, u_k = g_k / sigma_k
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
  // sort singular values descending (torch.svd order): the completion below rebuilds the SMALLEST axis.  A compare-exchange network
  // on (sigma, column of G, column of V) with static indices (an index array would put them into scratch memory)
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
  // R = V Z U^T with Z = diag(1, 1, sign(det(U V^T)))   (eval_utils.py:38-44) = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T, because
  // u1 x u2 = det(U) u3 and v1 x v2 = det(V) v3: the third pair is never divided by sigma_3 and carries the det sign by itself.
  // Rank 1 (sigma_2 <= 1e-6 sigma_1): u2, v2 are any unit vectors orthogonal to u1, v1 -- the 17 distances do not depend on the choice.
  // Rank 0 (K = 0): R = I; the scale below is then 0 (a constant target: PA error 0) or 0/0 (a constant pred: NaN), as in the reference.
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
  JRR_EVAL_PA_BEGIN
#pragma unroll
  for (int i = 0; i < NH; ++i) {
    float d2 = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float h = scale * (R[r][0] * P[i][0] + R[r][1] * P[i][1] + R[r][2] * P[i][2]) + t[r];
      const float d = h - Q[i][r];
      d2 += d * d;
    }
    JRR_EVAL_PA(i, sqrtf(d2))
  }
  JRR_EVAL_PA_END
#endif
