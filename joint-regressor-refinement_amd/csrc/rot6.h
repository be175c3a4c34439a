// 6-D rotation representation -> rotation matrix (rot6d_to_rotmat, /root/reference/scripts/utils.py:190-204): the ONE definition
// shared by the loop's kernels (prep.hip) and the pose export (export.hip), which must see the matrices the loop saw.
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

}  // namespace jrr
