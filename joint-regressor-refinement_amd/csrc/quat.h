// Unit quaternions of the refined-pose table's joints: the helpers the time-axis filter (smooth.hip) and the view fusion (views.hip)
// share, so that both see the same quaternion of the same six values.
// unit quaternion of a joint: the loop's own rot6d_fwd (rot6.h) of the row's six values, Shepperd's unnormalised quaternion of that
//   matrix (the branch rotmat_log of export.hip takes: of tr, R00, R11, R22 the largest, ties in that order), divided by its norm.
//   No canonical sign.
#pragma once
#include "rot6.h"

namespace jrr {

constexpr float SM_DEG = 57.29577951308232f;                  // 180 / pi

struct Quat { float w, x, y, z; };

// rot6d_fwd, included above, keeps the default contraction it has in the loop's kernels; everything below -- in this header and in the
// file that includes it -- is rounded once per operation, in the order written
#pragma clang fp contract(off)

__device__ __forceinline__ Quat unit_quat(const float R[9]) {
  const float r00 = R[0], r11 = R[4], r22 = R[8];
  const float tr = r00 + r11 + r22;
  Quat q;
  if (tr >= r00 && tr >= r11 && tr >= r22) {
    q.w = 1.f + tr;             q.x = R[7] - R[5];            q.y = R[2] - R[6];            q.z = R[3] - R[1];
  } else if (r00 >= r11 && r00 >= r22) {
    q.w = R[7] - R[5];          q.x = 1.f + r00 - r11 - r22;  q.y = R[1] + R[3];            q.z = R[2] + R[6];
  } else if (r11 >= r22) {
    q.w = R[2] - R[6];          q.x = R[1] + R[3];            q.y = 1.f + r11 - r00 - r22;  q.z = R[5] + R[7];
  } else {
    q.w = R[3] - R[1];          q.x = R[2] + R[6];            q.y = R[5] + R[7];            q.z = 1.f + r22 - r00 - r11;
  }
  const float n = sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  q.w = q.w / n; q.x = q.x / n; q.y = q.y / n; q.z = q.z / n;
  return q;
}

__device__ __forceinline__ float qdot(const Quat& a, const Quat& b) { return a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z; }

// conj(a) (x) b
__device__ __forceinline__ Quat conj_mul(const Quat& a, const Quat& b) {
  Quat e;
  e.w = qdot(a, b);
  e.x = a.w * b.x - b.w * a.x - (a.y * b.z - a.z * b.y);
  e.y = a.w * b.y - b.w * a.y - (a.z * b.x - a.x * b.z);
  e.z = a.w * b.z - b.w * a.z - (a.x * b.y - a.y * b.x);
  return e;
}

__device__ __forceinline__ float angle_deg(const Quat& e) {
  return 2.f * atan2f(sqrtf(e.x * e.x + e.y * e.y + e.z * e.z), fabsf(e.w)) * SM_DEG;
}

}  // namespace jrr
