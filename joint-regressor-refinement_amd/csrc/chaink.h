// Device bodies of the kinematic chain, one thread per (pose, joint): 6-D rotation -> R, blend features and the chain forward
// (prep_fwd_body), its adjoint with the fused per-pose Adam update (chain_bwd_body, pose_update_*).  Each body runs as a kernel of its
// own (k_prep_fwd, k_prep_fwd_dconv, k_chain_bwd) or composes with the support-vertex body inside one launch (k_sup_step), as supk.h's
// sup_body does; all of them are chain.hip's.
//
// Reference arithmetic restated here:
//   rot6d_to_rotmat            /root/reference/scripts/utils.py:190-204
//   rigid chain / A matrices   smplx 0.1.26 lbs.batch_rigid_transform
//   Adam                       torch.optim.Adam defaults, scripts/optimize.py:201-202,263-265
#pragma once
#include "jrr_common.h"
#include "kernels.h"
#include "rot6.h"

namespace jrr {

// ------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));
// The per-(pose, joint) records of the pose-major API tensors ((B,24,6) poses / gradients, (B,154) Adam state) are 6
// contiguous floats at an even float offset: three 8-byte accesses instead of six 4-byte ones (lanes are 576 / 616 bytes
// apart, so every access is its own memory transaction: their count is what these kernels pay for).
__device__ __forceinline__ void load6(const float* __restrict__ p, float v[6]) {
  const f32x2* q = reinterpret_cast<const f32x2*>(p);
  const f32x2 a = q[0], b = q[1], c = q[2];
  v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1]; v[4] = c[0]; v[5] = c[1];
}
__device__ __forceinline__ void store6(float* __restrict__ p, const float v[6]) {
  f32x2* q = reinterpret_cast<f32x2*>(p);
  q[0] = f32x2{v[0], v[1]}; q[1] = f32x2{v[2], v[3]}; q[2] = f32x2{v[4], v[5]};
}
__device__ __forceinline__ void load_rot(const float* __restrict__ x6d, const float* __restrict__ Rin, int b, int j,
                                         float R[9], Rot6& c) {
  if (Rin) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rin[((size_t)b * NJ + j) * 9 + k];
  } else {
    float xv[6];
    load6(x6d + ((size_t)b * NJ + j) * 6, xv);
    rot6d_fwd(xv, R, c);
  }
}

__device__ __forceinline__ void rest_joint(const float* __restrict__ Jt, const float* __restrict__ JS, int j,
                                           const float beta[NB], float J[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float acc = Jt[j * 3 + c];
#pragma unroll
    for (int l = 0; l < NB; ++l) acc = fmaf(JS[(j * 3 + c) * NB + l], beta[l], acc);
    J[c] = acc;
  }
}

// ------------------------------------------------------------------------------------------
// k_prep_fwd: 6-D rotation -> R, blend features FT [KFP][BP], kinematic chain -> skinning transforms
// AT [12][24][BP] (A_j = G_j - [0 | G_j.R J_j], entry e = r*4+c), R0T [9][BP].
// One thread per (pose, joint): block = 32 poses x 24 joints, lanes run over poses (coalesced
// feature-major stores).  The chain is walked level by level of the kinematic tree (depth <= 9 for
// SMPL) with the world transforms exchanged through LDS.  Poses b >= B are written as zeros.
// ------------------------------------------------------------------------------------------
constexpr int PP = 32;   // poses per block of the (pose, joint)-parallel kernels
constexpr int PREP_FWD_LDS = NJ * 15 * PP;      // floats: world transforms [24][12][PP] + rest joints [24][3][PP]

__device__ __forceinline__ void prep_fwd_body(int blk, const float* __restrict__ x6d, const float* __restrict__ Rin,
                                              const float* __restrict__ betas, const float* __restrict__ Jt,
                                              const float* __restrict__ JS, const Parents& par, float* __restrict__ FT,
                                              float* __restrict__ AT, float* __restrict__ R0T, int B, int BP,
                                              int32_t* step_inc, float* __restrict__ FTq, float* __restrict__ sh) {
  // FTq: the same features in K-quads [KFP / 4][BP][4] -- the B operand of k_lbs_fwd's blend product (one 16-byte LDS read = four
  // K steps); the row-major FT stays for the chain adjoint and the folded-regressor product
  // sh: PREP_FWD_LDS floats of the caller's LDS (the composed kernel k_sup_step hands every phase the same pool)
  float (*Gs)[12][PP] = reinterpret_cast<float (*)[12][PP]>(sh);
  float (*Js)[3][PP] = reinterpret_cast<float (*)[3][PP]>(sh + NJ * 12 * PP);
  const int bl = threadIdx.x & (PP - 1), j = threadIdx.x / PP;
  const int b = blk * PP + bl;
  auto fq = [&](int k) -> float& { return FTq[((size_t)(k >> 2) * BP + b) * 4 + (k & 3)]; };
  if (step_inc && blk == 0 && threadIdx.x == 0) step_inc[0] += 1;   // Adam step count of this iteration
  const bool ok = b < B;
  float R[9], J[3] = {0.f, 0.f, 0.f}, beta[NB];
  Rot6 c;
  if (ok) {
    load_rot(x6d, Rin, b, j, R, c);
#pragma unroll
    for (int l = 0; l < NB; ++l) beta[l] = betas[(size_t)b * NB + l];
    rest_joint(Jt, JS, j, beta, J);
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = 0.f;
#pragma unroll
    for (int l = 0; l < NB; ++l) beta[l] = 0.f;
  }
  // blend features: F[(j-1)*9 + k] = R_j[k] - I  (j >= 1), shape rows, template row, zero padding
  if (j > 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float f = ok ? R[k] - ((k == 0 || k == 4 || k == 8) ? 1.f : 0.f) : 0.f;
      FT[(size_t)((j - 1) * 9 + k) * BP + b] = f;
      fq((j - 1) * 9 + k) = f;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) R0T[(size_t)k * BP + b] = R[k];
#pragma unroll
    for (int l = 0; l < NB; ++l) { FT[(size_t)(207 + l) * BP + b] = beta[l]; fq(207 + l) = beta[l]; }
    FT[(size_t)217 * BP + b] = ok ? 1.f : 0.f;
    fq(217) = ok ? 1.f : 0.f;
    for (int k = KF; k < KFP; ++k) { FT[(size_t)k * BP + b] = 0.f; fq(k) = 0.f; }
  }
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) Js[j][cc][bl] = J[cc];
  __syncthreads();
  // world transforms, one tree level per step
  float G[12];
  const int dj = par.depth[j];
  for (int d = 0; d <= par.maxd; ++d) {
    if (dj == d) {
      if (d == 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) G[r * 4 + cc] = R[r * 3 + cc];
          G[r * 4 + 3] = J[r];
        }
      } else {
        const int p = par.p[j];
        float Gp[12], rel[3];
#pragma unroll
        for (int e = 0; e < 12; ++e) Gp[e] = Gs[p][e][bl];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) rel[cc] = J[cc] - Js[p][cc][bl];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int cc = 0; cc < 3; ++cc)
            G[r * 4 + cc] = Gp[r * 4 + 0] * R[0 * 3 + cc] + Gp[r * 4 + 1] * R[1 * 3 + cc] + Gp[r * 4 + 2] * R[2 * 3 + cc];
          G[r * 4 + 3] = Gp[r * 4 + 0] * rel[0] + Gp[r * 4 + 1] * rel[1] + Gp[r * 4 + 2] * rel[2] + Gp[r * 4 + 3];
        }
      }
#pragma unroll
      for (int e = 0; e < 12; ++e) Gs[j][e][bl] = G[e];
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) AT[(size_t)((r * 4 + cc) * NJ + j) * BP + b] = ok ? G[r * 4 + cc] : 0.f;
    AT[(size_t)((r * 4 + 3) * NJ + j) * BP + b] =
        ok ? G[r * 4 + 3] - (G[r * 4 + 0] * J[0] + G[r * 4 + 1] * J[1] + G[r * 4 + 2] * J[2]) : 0.f;
  }
}

// ------------------------------------------------------------------------------------------
// Adjoint of k_prep_fwd, in two kernels:
//
// k_chain_bwd (one pose per lane, children before parents): dL/dA^T [288][BP] and dL/dF^T [224][BP]
//   -> dL/dR^T [24*9][BP] and dL/dbeta^T [10][BP].  Every global access is pose-contiguous
//   (coalesced): R comes back from the feature rows F^T (+ identity) / R0T, the world rotations
//   G_j.R from the rotation part of A^T, so nothing of the forward chain is recomputed.  LDS holds
//   only the dG accumulators (12 floats per joint per lane).
//
// The same threads then finish the per-pose update (pose_update_*): 6-D rotation adjoint, extra (discriminator)
//   gradients, then either the gradient outputs or the fused Adam update -- dL/dR never leaves registers.
// ------------------------------------------------------------------------------------------
// (PoseUpdateArgs, the kernel-argument half of a PrepBwdLaunch: kernels.h)

// joint j of pose b: dL/dR_j (9) -> 6-D rotation adjoint (+ the discriminator's gradient) -> gradient output or Adam
__device__ __forceinline__ void pose_update_joint(const PoseUpdateArgs& a, int b, int j, const float dRi[9], const AdamScalars& sc) {
  if (!a.x6d_in) {
    if (a.dR) {
#pragma unroll
      for (int k = 0; k < 9; ++k) a.dR[((size_t)b * NJ + j) * 9 + k] = dRi[k];
    }
    return;
  }
  float xv[6], R[9], dx[6];
  Rot6 c;
  load6(a.x6d_in + ((size_t)b * NJ + j) * 6, xv);
  rot6d_fwd(xv, R, c);
  rot6d_bwd(c, dRi, dx);
  if (a.gx_extra) {
    float gx[6];
    load6(a.gx_extra + ((size_t)b * NJ + j) * 6, gx);
#pragma unroll
    for (int k = 0; k < 6; ++k) dx[k] += gx[k];
  }
  if (a.dx6d) store6(a.dx6d + ((size_t)b * NJ + j) * 6, dx);
  if (a.x6d_io) {
    const size_t si = (size_t)b * NPARAM + j * 6;
    float mm[6], vv[6], xn[6];
    load6(a.adam_m + si, mm);
    load6(a.adam_v + si, vv);
#pragma unroll
    for (int k = 0; k < 6; ++k) xn[k] = adam_update(xv[k], dx[k], mm[k], vv[k], sc);
    store6(a.x6d_io + ((size_t)b * NJ + j) * 6, xn);
    store6(a.adam_m + si, mm);
    store6(a.adam_v + si, vv);
  }
}
// shape coefficient l of pose b
__device__ __forceinline__ void pose_update_beta(const PoseUpdateArgs& a, int b, int l, float g, const AdamScalars& sc) {
  if (a.gb_extra) g += a.gb_extra[(size_t)b * NB + l];
  if (a.dbetas) a.dbetas[(size_t)b * NB + l] = g;
  if (a.x6d_io) {
    const size_t si = (size_t)b * NPARAM + JRR_POSE6D + l;
    float mm = a.adam_m[si], vv = a.adam_v[si];
    a.betas_io[(size_t)b * NB + l] = adam_update(a.betas_io[(size_t)b * NB + l], g, mm, vv, sc);
    a.adam_m[si] = mm;
    a.adam_v[si] = vv;
  }
}
// camera component cc of pose b: Adam over [pose, orient, betas, cam] (optimize.py:201-202)
__device__ __forceinline__ void pose_update_cam(const PoseUpdateArgs& a, int b, int cc, const AdamScalars& sc) {
  const size_t si = (size_t)b * 3 + cc;
  float mm = a.cam_m[si], vv = a.cam_v[si];
  a.cam_io[si] = adam_update(a.cam_io[si], a.gcam[si], mm, vv, sc);
  a.cam_m[si] = mm;
  a.cam_v[si] = vv;
}

constexpr int PPB = 32;   // poses per block of k_chain_bwd (16 halves the coalescing width: measured 1.5x slower)
// LDS pool of the chain adjoint (floats): dG | Js | dBs | Jts | JSs | adam scalars (8) | child list (24 bytes in 8 floats)
constexpr int CB_DG = 0, CB_JS = CB_DG + NJ * 12 * PPB, CB_DBS = CB_JS + NJ * 3 * PPB, CB_JTS = CB_DBS + NJ * NB * PPB,
              CB_JSS = CB_JTS + NJ * 3, CB_ADAM = CB_JSS + NJ * 3 * NB, CB_CHILD = CB_ADAM + 8, CHAIN_BWD_LDS = CB_CHILD + 8;
static_assert(sizeof(AdamScalars) <= 8 * sizeof(float), "adam scalars slot");
__device__ __forceinline__ void chain_bwd_body(int blk, const float* __restrict__ FT, const float* __restrict__ R0T,
                                               const float* __restrict__ AT, const float* __restrict__ Jt,
                                               const float* __restrict__ JS, const Parents& par,
                                               const float* __restrict__ dA_, int nslabA, size_t strideA,
                                               const float* __restrict__ dF_, const PoseUpdateArgs& ua, int B, int BP,
                                               const unsigned* __restrict__ dmask, float* __restrict__ sh, int step_now = -1) {
  // step_now >= 0 (thread 0 only; the composed kernel k_sup_step): Adam's step count of this iteration, instead of ua.step[0]
  constexpr int PP = PPB;
  AdamScalars& adam_sc = *reinterpret_cast<AdamScalars*>(sh + CB_ADAM);
  // one thread per (pose, joint); levels of the kinematic tree are processed deepest first.  Each child
  // leaves its contribution to the parent's dG in its own LDS slot; the parent sums its children in
  // index order (no atomics: bitwise reproducible).
  float (*dG)[12][PP] = reinterpret_cast<float (*)[12][PP]>(sh + CB_DG);
  float (*Js)[3][PP] = reinterpret_cast<float (*)[3][PP]>(sh + CB_JS);
  float (*dBs)[NB][PP] = reinterpret_cast<float (*)[NB][PP]>(sh + CB_DBS);
  const int bl = threadIdx.x & (PP - 1), j = threadIdx.x / PP;
  const int b = blk * PP + bl;
  const bool ok = b < B;
  const size_t bb = ok ? (size_t)b : 0;      // padded lanes read pose 0 and write nothing
  const int p = par.p[j];
  // this joint's children (ascending) from the model's child lists.  (Searching them -- "for q > j: if parent[q] == j"
  // -- indexes the kernel arguments with a per-lane q: 23 dependent memory loads per working wave and tree level,
  // ~2 us per level, measured with wall-clock stamps: 17.6 of the kernel's 34 us.)
  const int c_lo = par.child_off[j], c_hi = par.child_off[j + 1];
  unsigned char* const childs = reinterpret_cast<unsigned char*>(sh + CB_CHILD);
  if (threadIdx.x < NJ) childs[threadIdx.x] = par.child[threadIdx.x];
  // the rest-joint tables (72 + 720 floats) are read with per-lane (joint) indices: from LDS, not from memory
  float* const Jts = sh + CB_JTS;
  float* const JSs = sh + CB_JSS;
  for (int i = threadIdx.x; i < NJ * 3 * NB; i += PP * NJ) JSs[i] = JS[i];
  if (threadIdx.x < NJ * 3) Jts[threadIdx.x] = Jt[threadIdx.x];
  float beta[NB], dbeta[NB], Ji[3];
  // Row addressing of the [row][BP] arrays: a scalar base + ONE 32-bit byte offset per lane, rows stepped by scalar
  // multiples of the row pitch (a 64-bit per-lane multiply-add per element -- what `array[(size_t)row * BP + b]` with a
  // per-lane row compiles to -- is quarter-rate: ~400 VALU instructions for this kernel's 94 loads).
  const unsigned pitch = (unsigned)BP * 4u, lane_b = (unsigned)bb * 4u;
  auto ld = [](const float* base, unsigned byte_off) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
  };
#pragma unroll
  for (int l = 0; l < NB; ++l) { beta[l] = ld(FT, (unsigned)(207 + l) * pitch + lane_b); dbeta[l] = 0.f; }
  // everything this joint needs from global memory, issued up front (independent, pose-contiguous; joint 0 reads
  // valid rows it does not use instead of branching around the loads)
  float dA[12], GiR[9], R[9], Gp[9], dFj[9];
  const unsigned oj = (unsigned)j * pitch + lane_b;                         // row j
  const unsigned opj = (unsigned)(p > 0 ? p : 0) * pitch + lane_b;          // row of the parent
  const unsigned ofj = (unsigned)(j > 0 ? (j - 1) * 9 : 0) * pitch + lane_b;   // first pose-feature row of joint j
  // dA^T arrives as per-vertex-chunk partial slabs [nslabA][12][24][BP]: summed here, in slab order (deterministic)
  // (two slabs' loads -- 24 -- in flight together).  dmask (k_lbs_bwd16): bit j of word [slab][b / 64] says whether the slab holds
  // rows for joint j at all -- rows of joints its chunk never touched are neither written nor read (x + 0 = x: same sums)
  {
    const int n_bt = BP / 64, bt = (int)(blk * PP) / 64;
#pragma unroll
    for (int e = 0; e < 12; ++e) dA[e] = 0.f;
    for (int sl = 0; sl < nslabA; sl += 2) {
      float t[12], u[12];
      const bool two = sl + 1 < nslabA;
      const bool v0 = !dmask || ((dmask[sl * n_bt + bt] >> j) & 1u);
      const bool v1 = two && (!dmask || ((dmask[(sl + 1) * n_bt + bt] >> j) & 1u));
      const float* s0 = dA_ + (size_t)sl * strideA;
      const float* s1 = s0 + strideA;
#pragma unroll
      for (int e = 0; e < 12; ++e) t[e] = v0 ? ld(s0, oj + (unsigned)(e * NJ) * pitch) : 0.f;
#pragma unroll
      for (int e = 0; e < 12; ++e) u[e] = v1 ? ld(s1, oj + (unsigned)(e * NJ) * pitch) : 0.f;
#pragma unroll
      for (int e = 0; e < 12; ++e) dA[e] += t[e];
      if (two) {
#pragma unroll
        for (int e = 0; e < 12; ++e) dA[e] += u[e];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      GiR[r * 3 + cc] = ld(AT, oj + (unsigned)((r * 4 + cc) * NJ) * pitch);
      const float gp = ld(AT, opj + (unsigned)((r * 4 + cc) * NJ) * pitch);
      Gp[r * 3 + cc] = (j > 0) ? gp : 0.f;
    }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float f = ld(FT, ofj + (unsigned)k * pitch), df = ld(dF_, ofj + (unsigned)k * pitch);
    R[k] = (j > 0) ? f + ((k == 0 || k == 4 || k == 8) ? 1.f : 0.f) : 0.f;
    dFj[k] = (j > 0) ? df : 0.f;
  }
  // Adam's bias corrections (two fp64 pow: ~400 instructions, one thread) under the loads issued above, not before them
  if (ua.x6d_io && threadIdx.x == 0) adam_sc = adam_scalars(step_now >= 0 ? step_now : ua.step[0], ua.lr, ua.beta1, ua.beta2, ua.eps);
  __syncthreads();                              // tables staged
  rest_joint(Jts, JSs, j, beta, Ji);
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) Js[j][cc][bl] = Ji[cc];
  __syncthreads();

  float dRi[9];
  const int dj = par.depth[j];
  for (int d = par.maxd; d >= 0; --d) {
    if (dj == d) {
      // dG_i = own (A.R = G.R ; A.t = G.t - G.R J) + the contributions of the children (one level deeper)
      float dGi[12];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) dGi[r * 4 + cc] = dA[r * 4 + cc] - dA[r * 4 + 3] * Ji[cc];
        dGi[r * 4 + 3] = dA[r * 4 + 3];
      }
      for (int k = c_lo; k < c_hi; ++k) {
        const int q = childs[k];
#pragma unroll
        for (int e = 0; e < 12; ++e) dGi[e] += dG[q][e][bl];
      }
      float dJ[3];
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) dJ[cc] = -(GiR[0 * 3 + cc] * dA[3] + GiR[1 * 3 + cc] * dA[7] + GiR[2 * 3 + cc] * dA[11]);
      if (j == 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) dRi[r * 3 + cc] = dGi[r * 4 + cc];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) dJ[cc] += dGi[cc * 4 + 3];   // G_0.t = J_0
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
#pragma unroll
          for (int l = 0; l < NB; ++l) dbeta[l] = fmaf(dJ[cc], JSs[(0 * 3 + cc) * NB + l], dbeta[l]);
      } else {
        float rel[3], drel[3];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) rel[cc] = Ji[cc] - Js[p][cc][bl];
        // G_i.R = Gp.R R_i ; G_i.t = Gp.R rel + Gp.t ;  F[(i-1)*9+k] = R_i[k] - I
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int cc = 0; cc < 3; ++cc)
            dRi[r * 3 + cc] = Gp[0 * 3 + r] * dGi[0 * 4 + cc] + Gp[1 * 3 + r] * dGi[1 * 4 + cc] + Gp[2 * 3 + r] * dGi[2 * 4 + cc] +
                              dFj[r * 3 + cc];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
          drel[cc] = Gp[0 * 3 + cc] * dGi[0 * 4 + 3] + Gp[1 * 3 + cc] * dGi[1 * 4 + 3] + Gp[2 * 3 + cc] * dGi[2 * 4 + 3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) {
            const float add = dGi[r * 4 + 0] * R[cc * 3 + 0] + dGi[r * 4 + 1] * R[cc * 3 + 1] + dGi[r * 4 + 2] * R[cc * 3 + 2] +
                              dGi[r * 4 + 3] * rel[cc];
            dG[j][r * 4 + cc][bl] = add;                 // this joint's contribution to dG of its parent
          }
          dG[j][r * 4 + 3][bl] = dGi[r * 4 + 3];
        }
        // J_i enters through -G_i.R J_i (dJ) and rel = J_i - J_p (drel)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
#pragma unroll
          for (int l = 0; l < NB; ++l)
            dbeta[l] = fmaf(dJ[cc] + drel[cc], JSs[(j * 3 + cc) * NB + l], fmaf(-drel[cc], JSs[(p * 3 + cc) * NB + l], dbeta[l]));
      }
    }
    __syncthreads();
  }
  // dL/dbeta: sum the per-joint contributions of each pose (fixed order: deterministic)
#pragma unroll
  for (int l = 0; l < NB; ++l) dBs[j][l][bl] = dbeta[l];
  __syncthreads();           // (also orders thread 0's adam_sc before its readers)
  // ---- fused per-pose update (formerly a second kernel over the same (pose, joint) threads): 6-D rotation adjoint,
  //      the discriminators' extra gradients, then either the gradient outputs or torch's Adam in place ----
  const AdamScalars sc = adam_sc;
  if (ok) {
    pose_update_joint(ua, b, j, dRi, sc);
    if (j < NB) {
      float acc = dF_[(size_t)(207 + j) * BP + b];
#pragma unroll
      for (int q = 0; q < NJ; ++q) acc += dBs[q][j][bl];
      pose_update_beta(ua, b, j, acc, sc);
    } else if (j < NB + 3 && ua.x6d_io && ua.cam_io) {
      pose_update_cam(ua, b, j - NB, sc);
    }
  }
}

}  // namespace jrr
