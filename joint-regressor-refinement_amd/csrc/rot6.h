// 6-D rotation representation -> rotation matrix (rot6d_to_rotmat, /root/reference/scripts/utils.py:190-204): the ONE definition
// shared by the loop's kernels (chaink.h, rot.hip) and the pose export (export.hip), which must see the matrices the loop saw.  Its
// adjoint rot6d_bwd serves the operator (rot.hip) and the fused pose update (chaink.h).
#pragma once

namespace jrr {

struct Rot6 {
  float b1[3], b2[3], a2[3];
  float n1, nu, s;   // |a1|, |u|, b1.a2
};

__device__ __forceinline__ void rot6d_fwd(const float x[6], float R[9], Rot6& c) {
  const float eps = 1e-12f;
  float a1[3] = {x[0], x[2], x[4]};
  c.a2[0] = x[1]; c.a2[1] = x[3]; c.a2[2] = x[5];
  c.n1 = sqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
  float d1 = fmaxf(c.n1, eps);
#pragma unroll
  for (int i = 0; i < 3; ++i) c.b1[i] = a1[i] / d1;
  c.s = c.b1[0] * c.a2[0] + c.b1[1] * c.a2[1] + c.b1[2] * c.a2[2];
  float u[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) u[i] = c.a2[i] - c.s * c.b1[i];
  c.nu = sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  float d2 = fmaxf(c.nu, eps);
#pragma unroll
  for (int i = 0; i < 3; ++i) c.b2[i] = u[i] / d2;
  float b3[3] = {c.b1[1] * c.b2[2] - c.b1[2] * c.b2[1], c.b1[2] * c.b2[0] - c.b1[0] * c.b2[2],
                 c.b1[0] * c.b2[1] - c.b1[1] * c.b2[0]};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    R[r * 3 + 0] = c.b1[r];
    R[r * 3 + 1] = c.b2[r];
    R[r * 3 + 2] = b3[r];
  }
}

__device__ __forceinline__ void rot6d_bwd(const Rot6& c, const float dR[9], float dx[6]) {
  const float eps = 1e-12f;
  float db1[3], db2[3], db3[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) { db1[r] = dR[r * 3 + 0]; db2[r] = dR[r * 3 + 1]; db3[r] = dR[r * 3 + 2]; }
  // b3 = b1 x b2
  db1[0] += c.b2[1] * db3[2] - c.b2[2] * db3[1];
  db1[1] += c.b2[2] * db3[0] - c.b2[0] * db3[2];
  db1[2] += c.b2[0] * db3[1] - c.b2[1] * db3[0];
  db2[0] += db3[1] * c.b1[2] - db3[2] * c.b1[1];
  db2[1] += db3[2] * c.b1[0] - db3[0] * c.b1[2];
  db2[2] += db3[0] * c.b1[1] - db3[1] * c.b1[0];
  // b2 = u / max(|u|, eps)
  float du[3];
  if (c.nu >= eps) {
    float t = c.b2[0] * db2[0] + c.b2[1] * db2[1] + c.b2[2] * db2[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) du[i] = (db2[i] - c.b2[i] * t) / c.nu;
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) du[i] = db2[i] / eps;
  }
  // u = a2 - (b1.a2) b1
  float t2 = c.b1[0] * du[0] + c.b1[1] * du[1] + c.b1[2] * du[2];
  float da2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    da2[i] = du[i] - c.b1[i] * t2;
    db1[i] += -c.a2[i] * t2 - c.s * du[i];
  }
  // b1 = a1 / max(|a1|, eps)
  float da1[3];
  if (c.n1 >= eps) {
    float t = c.b1[0] * db1[0] + c.b1[1] * db1[1] + c.b1[2] * db1[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) da1[i] = (db1[i] - c.b1[i] * t) / c.n1;
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) da1[i] = db1[i] / eps;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) { dx[2 * i] = da1[i]; dx[2 * i + 1] = da2[i]; }
}

}  // namespace jrr
