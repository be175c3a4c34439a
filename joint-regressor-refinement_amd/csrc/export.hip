// Refined poses as SMPL axis-angle records (`--save_refined`; the pseudo-ground truth the reference's scripts/create_smpl_gt.py
// was meant to produce): the inverse of k_rodrigues_fwd, and the per-sample store.
//
// rotmat_log: R (row-major 3 x 3, assumed a rotation) -> axis-angle, without acosf and without a division by sin(theta):
//   1. the unnormalised quaternion by Shepperd's choice -- of tr, R00, R11, R22 the largest (ties in that order) selects
//        (w,x,y,z) = (1+tr, R21-R12, R02-R20, R10-R01)  |  (R21-R12, 1+R00-R11-R22, R01+R10, R02+R20)  |  the two cyclic analogues,
//      so the component the others are measured against is never a cancelled sum;
//   2. canonical sign: negated when w < 0, and when w == 0 and the first non-zero of (x,y,z) is negative: the angle lies in
//      [0, pi] and a half-turn has ONE answer;
//   3. s = |(x,y,z)|, aa = (x,y,z) * f with f = 2 atan2f(s, w) / s, or the series (2/w)(1 - (s/w)^2 / 3) when s <= 1e-4 w
//      (the exact identity gives exactly zero).  s and f carry their rounding residuals (fmaf), so every component of aa is rounded
//      once and the vector is never longer than fl(pi) + one ulp.
//   Non-finite input falls through the comparisons into the last branch and gives non-finite output; nothing is indexed by data.
// k_rotmat_log: the operator, one thread per rotation.
// k_pose_export: ONE launch per outer batch and shard: per (pose, joint) the loop's own rot6d_fwd (rot6.h), then rotmat_log; the
//   240-float rows of include/jrr.h (JRR_EXPORT_*) are assembled in LDS and scattered into the table by dataset index, 16 bytes per
//   lane along the row.  676 B read and 960 B written per pose; no engine, no engine state.
#include "jrr_common.h"
#include "rot6.h"
#include "../../include/jrr.h"

namespace jrr {

constexpr int EX_POSES = 8;                                  // poses per workgroup
constexpr int EX_THREADS = EX_POSES * JRR_NUM_JOINTS;        // 192: one thread per (pose, joint)
constexpr int EX_ROW4 = JRR_EXPORT_ROW / 4;                  // 60 float4 per row
static_assert(JRR_EXPORT_ROW % 4 == 0 && JRR_EXPORT_ROW - JRR_EXPORT_BETAS == JRR_NUM_JOINTS, "one tail float per joint thread");
static_assert(JRR_EXPORT_EXTRA + JRR_EXPORT_MAX_EXTRA == JRR_EXPORT_ROW && JRR_EXPORT_POSE6D == 3 * JRR_NUM_JOINTS, "row layout");

// rotmat_log: every operation is rounded once, in the order written, products meet sums only where fmaf is written (the host restatement in
// tests/refined_cases.py repeats it).  rot6d_fwd, included above, keeps the default contraction it has in the loop's kernels.
#pragma clang fp contract(off)

__device__ __forceinline__ void rotmat_log(const float R[9], float aa[3]) {
  const float r00 = R[0], r11 = R[4], r22 = R[8];
  const float tr = r00 + r11 + r22;
  float w, x, y, z;
  if (tr >= r00 && tr >= r11 && tr >= r22) {
    w = 1.f + tr;               x = R[7] - R[5];            y = R[2] - R[6];            z = R[3] - R[1];
  } else if (r00 >= r11 && r00 >= r22) {
    w = R[7] - R[5];            x = 1.f + r00 - r11 - r22;  y = R[1] + R[3];            z = R[2] + R[6];
  } else if (r11 >= r22) {
    w = R[2] - R[6];            x = R[1] + R[3];            y = 1.f + r11 - r00 - r22;  z = R[5] + R[7];
  } else {
    w = R[3] - R[1];            x = R[2] + R[6];            y = R[5] + R[7];            z = 1.f + r22 - r00 - r11;
  }
  const float first = x != 0.f ? x : (y != 0.f ? y : z);
  if (w < 0.f || (w == 0.f && first < 0.f)) { w = -w; x = -x; y = -y; z = -z; }
  // s*s = x*x + y*y + z*z as an unevaluated sum t + lo (error-free products and sums), so that s + s_lo is the norm far below an ulp
  const float xx = x * x, yy = y * y, zz = z * z;
  const float t1 = xx + yy, v1 = t1 - xx, e1 = (xx - (t1 - v1)) + (yy - v1);
  const float t = t1 + zz, v2 = t - t1, e2 = (t1 - (t - v2)) + (zz - v2);
  const float lo = ((fmaf(x, x, -xx) + fmaf(y, y, -yy)) + fmaf(z, z, -zz)) + (e1 + e2);
  const float s = sqrtf(t);
  if (s <= 1e-4f * w) {
    const float q = s / w;
    const float f = (2.f / w) * (1.f - q * q / 3.f);
    aa[0] = x * f; aa[1] = y * f; aa[2] = z * f;
    return;
  }
  // f + f_lo = theta / (s + s_lo): each component is then rounded ONCE, and |aa| <= theta (1 + 2^-24) <= fl(pi) + one ulp
  const float s_lo = (fmaf(-s, s, t) + lo) / (2.f * s);
  const float th = 2.f * atan2f(s, w);
  const float f = th / s;
  const float f_lo = (fmaf(-f, s, th) - f * s_lo) / s;
  aa[0] = fmaf(x, f, x * f_lo); aa[1] = fmaf(y, f, y * f_lo); aa[2] = fmaf(z, f, z * f_lo);
}

__global__ __launch_bounds__(256) void k_rotmat_log(const float* __restrict__ R, float* __restrict__ aa, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float Rv[9], a[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) Rv[k] = R[(size_t)i * 9 + k];
  rotmat_log(Rv, a);
#pragma unroll
  for (int k = 0; k < 3; ++k) aa[(size_t)i * 3 + k] = a[k];
}

// grid: ceil(B / 8) workgroups of 192 threads; thread (p, j) owns joint j of pose 8 * blockIdx + p and float 216 + j of its row
__global__ __launch_bounds__(EX_THREADS) void k_pose_export(const float* __restrict__ x6d, const float* __restrict__ betas,
                                                            const float* __restrict__ cam, const float* __restrict__ extra, int n_extra,
                                                            const long long* __restrict__ index, float* __restrict__ table,
                                                            long long n_rows, int* __restrict__ status, int B) {
  __shared__ float4 s_row4[EX_POSES * EX_ROW4];
  __shared__ long long s_idx[EX_POSES];
  float* s_row = reinterpret_cast<float*>(s_row4);
  const int tid = threadIdx.x, p = tid / JRR_NUM_JOINTS, j = tid - p * JRR_NUM_JOINTS;
  const int b = (int)blockIdx.x * EX_POSES + p;
  if (b < B) {
    float* row = s_row + p * JRR_EXPORT_ROW;
    float xv[6], Rv[9], a[3];
    Rot6 c;
    const float2* x2 = reinterpret_cast<const float2*>(x6d + ((size_t)b * JRR_NUM_JOINTS + j) * 6);      // 24 B per joint: 8-byte aligned
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float2 v = x2[k]; xv[2 * k] = v.x; xv[2 * k + 1] = v.y; }
    rot6d_fwd(xv, Rv, c);
    rotmat_log(Rv, a);
#pragma unroll
    for (int k = 0; k < 3; ++k) row[JRR_EXPORT_POSE + j * 3 + k] = a[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) row[JRR_EXPORT_POSE6D + j * 6 + k] = xv[k];
    float t;                                                   // float 216 + j: betas | cam | marker | extra, zero-padded
    if (j < JRR_NUM_BETAS) t = betas[(size_t)b * JRR_NUM_BETAS + j];
    else if (j < JRR_NUM_BETAS + 3) t = cam[(size_t)b * 3 + (j - JRR_NUM_BETAS)];
    else if (j == JRR_EXPORT_MARKER - JRR_EXPORT_BETAS) t = 1.0f;
    else {
      const int e = j - (JRR_EXPORT_EXTRA - JRR_EXPORT_BETAS);
      t = (extra != nullptr && e < n_extra) ? extra[(size_t)b * n_extra + e] : 0.f;
    }
    row[JRR_EXPORT_BETAS + j] = t;
  }
  if (j == 0) {                                                // one lane per pose: where the row goes, and whether it may
    long long idx = -1;
    if (b < B) {
      idx = index[b];
      if (idx < 0 || idx >= n_rows) {
        idx = -1;
        atomicOr(status, JRR_EXPORT_STATUS_INDEX);
      } else {
        // claim the row (marker <- 1.0f): a marker already set, by an earlier launch or by another pose of this one, means the
        // sample comes twice
        const int old = atomicExch(reinterpret_cast<int*>(table + (size_t)idx * JRR_EXPORT_ROW + JRR_EXPORT_MARKER), 0x3f800000);
        if (old != 0) atomicOr(status, JRR_EXPORT_STATUS_TWICE);
      }
    }
    s_idx[p] = idx;
  }
  __syncthreads();
  float4* table4 = reinterpret_cast<float4*>(table);
  for (int i = tid; i < EX_POSES * EX_ROW4; i += EX_THREADS) {
    const int pp = i / EX_ROW4, q = i - pp * EX_ROW4;
    const long long idx = s_idx[pp];
    if (idx >= 0) table4[(size_t)idx * EX_ROW4 + q] = s_row4[i];
  }
}

}  // namespace jrr

using namespace jrr;

/* the log map and the refined-pose table (--save_refined) */
extern "C" int jrr_rotmat_to_axis_angle(const float* R, float* aa, int n, void* stream) {
  if (!R || !aa || n < 0) {
    jrr_set_error("jrr_rotmat_to_axis_angle: bad argument");
    return JRR_ERR_ARG;
  }
  if (n == 0) return JRR_OK;
  hipLaunchKernelGGL(k_rotmat_log, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, R, aa, n);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_pose_export(const float* x6d, const float* betas, const float* cam, const float* extra, int n_extra, const int64_t* index,
                               float* table, int64_t n_rows, int32_t* status, int batch, void* stream) {
  if (!x6d || !betas || !cam || !index || !table || !status || batch < 0 || n_rows < 0) {
    jrr_set_error("jrr_pose_export: bad argument");
    return JRR_ERR_ARG;
  }
  if (n_extra < 0 || n_extra > JRR_EXPORT_MAX_EXTRA) {
    jrr_set_error("jrr_pose_export: n_extra %d: 0 .. %d", n_extra, (int)JRR_EXPORT_MAX_EXTRA);
    return JRR_ERR_ARG;
  }
  if (((uintptr_t)table & 15) != 0 || ((uintptr_t)x6d & 7) != 0 || ((uintptr_t)index & 7) != 0 || ((uintptr_t)status & 3) != 0) {
    jrr_set_error("jrr_pose_export: the table must be 16-byte aligned (x6d and index 8-byte, status 4-byte)");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  hipLaunchKernelGGL(k_pose_export, dim3((unsigned)((batch + EX_POSES - 1) / EX_POSES)), dim3(EX_THREADS), 0, (hipStream_t)stream, x6d, betas, cam,
                     n_extra > 0 ? extra : nullptr, n_extra, reinterpret_cast<const long long*>(index), table, (long long)n_rows, status, batch);
  CHECK_LAUNCH();
  return JRR_OK;
}
