// Joint loss and camera: the pelvis-centred 3-D joint loss (+ the 2-D reprojection term) of the loop and as a stand-alone operator, the
// projection of joints to the screen, and the camera pre-fit.
//
// Reference arithmetic restated here:
//   move_pelvis + MSELoss      scripts/utils.py:106-114, scripts/optimize.py:238-239
//   Adam                       torch.optim.Adam defaults, scripts/optimize.py:201-202,263-265
#include "jrr_common.h"
#include "kernels.h"
#include "proj.h"

namespace jrr {

constexpr int PP = 32;   // poses per block of k_joints_loss, as the (pose, joint)-parallel kernels of the chain (chaink.h)

// ------------------------------------------------------------------------------------------
// Perspective projection of the regressed joints (scripts/renderer.py:35-49 with pytorch3d 0.3.0
// PerspectiveCameras, R = I, T = cam, focal 5000/224 in NDC, principal point 0, 224x224 screen;
// SURVEY.md Appendix B):  X = -2x + tx, Y = -2y + ty, Z = 2z + tz ;  x_ndc = f X / Z ;
// x_screen = (W-1)/2 (1 - x_ndc)  (same for y).
// ------------------------------------------------------------------------------------------
// (project_point / project_point_bwd / Reproj: proj.h -- shared with the support-vertex iteration, supk.h)

// ------------------------------------------------------------------------------------------
// k_joints_loss: joints (from the reduced partials [3][17][BP]) -> joints (B,17,3), per-pose squared
// error, and the adjoint dJT [3][18][BP] of
//     weight * mean((move_pelvis(j) - gt/1000)^2)   [+ weight2d * mean((gt_j2d - project(j, cam))^2)]
//   scale = 2*weight/(batch_norm*51).  If djoints_in != NULL it is used as the adjoint instead
//   (operator-level backward), transposed into dJT.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PP * NH) void k_joints_loss(const float* __restrict__ JP, int nvc, int jp_rows,
                                                         const float* __restrict__ gt_mm,
                                                         const float* __restrict__ djoints_in, float scale,
                                                         float* __restrict__ joints_out, float* __restrict__ sqerr,
                                                         float* __restrict__ dJT, Reproj rp, int B, int BP,
                                                         const int* __restrict__ one_slab_flag) {
  // one thread per (pose, H36M joint): block = 32 poses x 17 joints, lanes over poses
  if (one_slab_flag && *one_slab_flag) nvc = 1;       // the support-restricted re-regression wrote ONE complete slab
  __shared__ float red[NH][8][PP];   // per-joint partials: 0..2 g, 3 err, 4 e2d, 5..7 gcam
  __shared__ float pel[3][PP];
  const int bl = threadIdx.x & (PP - 1), i = threadIdx.x / PP;
  const int b = blockIdx.x * PP + bl;
  const bool ok = b < B;
  float j[3] = {0.f, 0.f, 0.f};
  if (JP) {
    // per-vertex-chunk partials, summed in chunk order; four chunks' loads (12) in flight together
    int ch = 0;
    for (; ch + 4 <= nvc; ch += 4) {
      float t[4][3];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < 3; ++c) t[u][c] = JP[(size_t)(((ch + u) * 3 + c) * jp_rows + i) * BP + b];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < 3; ++c) j[c] += t[u][c];
    }
    for (; ch < nvc; ++ch)
#pragma unroll
      for (int c = 0; c < 3; ++c) j[c] += JP[(size_t)((ch * 3 + c) * jp_rows + i) * BP + b];
    if (joints_out && ok) {
#pragma unroll
      for (int c = 0; c < 3; ++c) joints_out[((size_t)b * NH + i) * 3 + c] = j[c];
    }
  }
  if (djoints_in) {      // operator-level backward: transpose the caller's adjoint
    if (dJT) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        dJT[(size_t)(c * NHP + i) * BP + b] = ok ? djoints_in[((size_t)b * NH + i) * 3 + c] : 0.f;
        if (i == 0) dJT[(size_t)(c * NHP + NH) * BP + b] = 0.f;
      }
    }
    return;
  }
  if (!gt_mm) return;
  if (i == 0) { pel[0][bl] = j[0]; pel[1][bl] = j[1]; pel[2][bl] = j[2]; }
  __syncthreads();
  float g[3], err = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float gtv = ok ? gt_mm[((size_t)b * NH + i) * 3 + c] / 1000.f : 0.f;
    // joint 0: the centred value is identically 0; gt is pelvis-centred by the caller (optimize.py:162)
    const float d = (i == 0) ? -gtv : (j[c] - pel[c][bl]) - gtv;
    err += d * d;
    g[c] = (i == 0) ? 0.f : scale * d;
    red[i][c][bl] = g[c];
  }
  float e2 = 0.f, gc[3] = {0.f, 0.f, 0.f}, g2[3] = {0.f, 0.f, 0.f};
  if (rp.gt_j2d && ok) {     // 2-D reprojection term on the UN-centred joints (optimize.py:231-233)
    float t[3] = {rp.cam[(size_t)b * 3], rp.cam[(size_t)b * 3 + 1], rp.cam[(size_t)b * 3 + 2]};
    float xs, ys, invZ, X, Y;
    project_point(j, t, xs, ys, invZ, X, Y);
    const float dx = xs - rp.gt_j2d[((size_t)b * NH + i) * 2], dy = ys - rp.gt_j2d[((size_t)b * NH + i) * 2 + 1];
    e2 = dx * dx + dy * dy;
    project_point_bwd(rp.scale2d * dx, rp.scale2d * dy, invZ, X, Y, g2, gc);
  }
  red[i][3][bl] = err;
  red[i][4][bl] = e2;
#pragma unroll
  for (int c = 0; c < 3; ++c) red[i][5 + c][bl] = gc[c];
  __syncthreads();
  if (i == 0) {       // fixed-order sums over the 17 joints (deterministic)
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < NH; ++q)
#pragma unroll
      for (int k = 0; k < 8; ++k) s[k] += red[q][k][bl];
    if (ok) {
      if (sqerr) sqerr[b] = s[3];
      if (rp.gt_j2d) {
        if (rp.sq2d) rp.sq2d[b] = s[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) rp.gcam[(size_t)b * 3 + c] = s[5 + c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = -s[c];     // move_pelvis adjoint: -sum_i g_i
  }
  if (dJT) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      dJT[(size_t)(c * NHP + i) * BP + b] = ok ? g[c] + g2[c] : 0.f;
      if (i == 0) dJT[(size_t)(c * NHP + NH) * BP + b] = 0.f;
    }
  }
}
int launch_joints_loss(const float* JP, int nvc, const float* gt_mm, const float* djoints_in, float scale,
                       float* joints_out, float* sqerr, float* dJT, int B, int BP, hipStream_t s, const Reproj& rp,
                       int jp_rows, const int* one_slab_flag) {
  hipLaunchKernelGGL(k_joints_loss, dim3(BP / PP), dim3(PP * NH), 0, s, JP, nvc, jp_rows, gt_mm, djoints_in, scale, joints_out,
                     sqerr, dJT, rp, B, BP, one_slab_flag);
  return 0;
}

// return_2d_joints core: joints (B,17,3), cam (B,3) -> screen coordinates (B,17,2)
__global__ void k_project_joints(const float* __restrict__ joints, const float* __restrict__ cam, float* __restrict__ out,
                                 int n) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;   // over B*17
  if (idx >= n) return;
  const int b = idx / NH;
  float p[3] = {joints[(size_t)idx * 3], joints[(size_t)idx * 3 + 1], joints[(size_t)idx * 3 + 2]};
  float t[3] = {cam[(size_t)b * 3], cam[(size_t)b * 3 + 1], cam[(size_t)b * 3 + 2]};
  float xs, ys, invZ, X, Y;
  project_point(p, t, xs, ys, invZ, X, Y);
  out[(size_t)idx * 2] = xs;
  out[(size_t)idx * 2 + 1] = ys;
}
int launch_project_joints(const float* joints, const float* cam, float* out, int B, hipStream_t s) {
  const int n = B * NH;
  hipLaunchKernelGGL(k_project_joints, dim3((n + 255) / 256), dim3(256), 0, s, joints, cam, out, n);
  return 0;
}

// Camera pre-fit (scripts/optimize.py:187-199): n Adam steps on the camera translation only, against the
// 2-D joints.  The reference re-runs the whole SMPL forward every step although the joints do not depend
// on the camera; here the joints are computed once and each thread runs its pose's n steps in registers.
__global__ __launch_bounds__(64) void k_camera_fit(const float* __restrict__ joints, const float* __restrict__ gt_j2d, float* __restrict__ cam,
                             float scale2d, int nsteps, float lr, float* __restrict__ sq2d, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float j[NH][3], q[NH][2];
#pragma unroll
  for (int i = 0; i < NH; ++i) {
#pragma unroll
    for (int c = 0; c < 3; ++c) j[i][c] = joints[((size_t)b * NH + i) * 3 + c];
    q[i][0] = gt_j2d[((size_t)b * NH + i) * 2];
    q[i][1] = gt_j2d[((size_t)b * NH + i) * 2 + 1];
  }
  float t[3] = {cam[(size_t)b * 3], cam[(size_t)b * 3 + 1], cam[(size_t)b * 3 + 2]};
  float m[3] = {0.f, 0.f, 0.f}, v[3] = {0.f, 0.f, 0.f};
  double b1p = 1.0, b2p = 1.0;
  float e2 = 0.f;
  for (int s = 1; s <= nsteps; ++s) {
    float gt3[3] = {0.f, 0.f, 0.f}, dummy[3] = {0.f, 0.f, 0.f};
    e2 = 0.f;
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      float xs, ys, invZ, X, Y;
      project_point(j[i], t, xs, ys, invZ, X, Y);
      const float dx = xs - q[i][0], dy = ys - q[i][1];
      e2 += dx * dx + dy * dy;
      project_point_bwd(scale2d * dx, scale2d * dy, invZ, X, Y, dummy, gt3);
    }
    b1p *= 0.9; b2p *= 0.999;
    AdamScalars sc;
    sc.step_size = (float)((double)lr / (1.0 - b1p));
    sc.bc2_sqrt = (float)sqrt(1.0 - b2p);
    sc.beta1 = 0.9f; sc.beta2 = 0.999f; sc.eps = 1e-8f;
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = adam_update(t[c], gt3[c], m[c], v[c], sc);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) cam[(size_t)b * 3 + c] = t[c];
  if (sq2d) sq2d[b] = e2;     // error at the LAST evaluated camera (before the final update), as the reference's loss
}
int launch_camera_fit(const float* joints, const float* gt_j2d, float* cam, float scale2d, int nsteps, float lr, float* sq2d,
                      int B, hipStream_t s) {
  hipLaunchKernelGGL(k_camera_fit, dim3((B + 63) / 64), dim3(64), 0, s, joints, gt_j2d, cam, scale2d, nsteps, lr, sq2d, B);
  return 0;
}

// standalone joint loss on (B,17,3) joints (operator-level API: jrr_joint_loss)
__global__ void k_joint_loss_plain(const float* __restrict__ joints, const float* __restrict__ gt_mm, float scale,
                                   float* __restrict__ sqerr, float* __restrict__ djoints, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float err = 0.f;
  for (int c = 0; c < 3; ++c) {
    float j0 = joints[((size_t)b * NH) * 3 + c];
    float gsum = 0.f;
    for (int i = 1; i < NH; ++i) {
      float d = (joints[((size_t)b * NH + i) * 3 + c] - j0) - gt_mm[((size_t)b * NH + i) * 3 + c] / 1000.f;
      err += d * d;
      float g = scale * d;
      gsum += g;
      if (djoints) djoints[((size_t)b * NH + i) * 3 + c] = g;
    }
    float d0 = -gt_mm[((size_t)b * NH) * 3 + c] / 1000.f;
    err += d0 * d0;
    if (djoints) djoints[((size_t)b * NH) * 3 + c] = -gsum;
  }
  if (sqerr) sqerr[b] = err;
}
int launch_joint_loss_plain(const float* joints, const float* gt_mm, float scale, float* sqerr, float* djoints, int B,
                            hipStream_t s) {
  hipLaunchKernelGGL(k_joint_loss_plain, dim3((B + 63) / 64), dim3(64), 0, s, joints, gt_mm, scale, sqerr, djoints, B);
  return 0;
}

}  // namespace jrr
