// The similarity fit of csrc/evalk.h as a FUNCTION of the moments: rotation, scale and translation from K = sum (x - mu1)(y - mu2)^T,
// var1 = sum |x - mu1|^2 and the two means, for point sets of any size (csrc/pve.hip forms the moments of 6890 vertices in double and
// rounds them to fp32; evalk.h forms those of 17 joints in fp32 inside its own body and stays as it is).
//   batch_compute_similarity_transform_torch   scripts/eval_utils.py:31-52 of the reference
// The statements below are evalk.h's, in its order: one-sided (Hestenes) Jacobi on K itself, six sweeps over the column pairs (0,1),
// (0,2), (1,2); the compare-exchange sort of (sigma, column of G, column of V); R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T with the
// rank-1 rule (sigma_2 <= 1e-6 sigma_1: u2, v2 completed orthogonally) and the rank-0 rule (K = 0: R = I, so a constant target gives
// scale 0 and a constant pred 0/0 = NaN); scale = trace(R K) / var1; t = mu2 - scale R mu1.  Every operation is rounded once in fp32
// in the order written: a translation unit that includes this header switches contraction off (#pragma clang fp contract(off)) when
// a host restatement is to follow it.  No value crosses lanes.
#ifndef JRR_PROCFIT_H
#define JRR_PROCFIT_H
#include "evalk.h"

namespace jrr {

__device__ __forceinline__ void procrustes_fit(const float K[3][3], float var1, const float mu1[3], const float mu2[3], float R[3][3],
                                               float& scale, float t[3]) {
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
  float sig[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) sig[k] = sqrtf(G[0][k] * G[0][k] + G[1][k] * G[1][k] + G[2][k] * G[2][k]);
  auto cswap = [&](auto A_, auto B_) __attribute__((always_inline)) {
    constexpr int a = decltype(A_)::value, c = decltype(B_)::value;
    if (sig[a] < sig[c]) {
      const float s = sig[a]; sig[a] = sig[c]; sig[c] = s;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float g = G[r][a]; G[r][a] = G[r][c]; G[r][c] = g;
        const float u = V[r][a]; V[r][a] = V[r][c]; V[r][c] = u;
      }
    }
  };
  using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
  cswap(I0{}, I1{}); cswap(I1{}, I2{}); cswap(I0{}, I1{});
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) R[r][c] = r == c ? 1.f : 0.f;
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
  float tr = 0.f;
#pragma unroll
  for (int r = 0; r < 3; ++r) tr += R[r][0] * K[0][r] + R[r][1] * K[1][r] + R[r][2] * K[2][r];
  scale = tr / var1;
#pragma unroll
  for (int r = 0; r < 3; ++r) t[r] = mu2[r] - scale * (R[r][0] * mu1[0] + R[r][1] * mu1[1] + R[r][2] * mu1[2]);
}

}  // namespace jrr
#endif  // JRR_PROCFIT_H
