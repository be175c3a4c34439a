// Every kernel built from the kinematic chain's bodies (chaink.h): chain forward, the posed SMPL joints with their adjoint, the chain
// adjoint with the fused per-pose Adam update; the two horizontally fused launches of the chain iterations (chain forward || per-joint
// MLP forward, per-joint MLP adjoint || dF^T slab sum); and k_sup_step, the ONE launch that is the default inner iteration, composed of
// the chain bodies, the support-vertex body (supk.h) and the per-joint MLP bodies (dconv.h).
//
// These kernels share one translation unit on purpose.  The compiler's code for a kernel that inlines a shared body depends on which
// other kernels of the same file inline it too: taking k_sup_step, k_prep_fwd_dconv or k_dconv_bwd_reduce out of the file of k_prep_fwd
// and k_chain_bwd (or putting k_sup_iter, sup.hip, into it) changes their instruction schedule and register allocation
// (profiles/ab_split_prep.txt).  Moving one of them is therefore a measured change, not a refactor.
#include "jrr_common.h"
#include "kernels.h"
#include "chaink.h"
#include "supk.h"
#include "dconv.h"

namespace jrr {

__global__ __launch_bounds__(PP * NJ) void k_prep_fwd(const float* __restrict__ x6d, const float* __restrict__ Rin,
                                                      const float* __restrict__ betas, const float* __restrict__ Jt,
                                                      const float* __restrict__ JS, Parents par, float* __restrict__ FT,
                                                      float* __restrict__ AT, float* __restrict__ R0T, int B, int BP,
                                                      int32_t* step_inc, float* __restrict__ FTq) {
  __shared__ float sh[PREP_FWD_LDS];
  prep_fwd_body(blockIdx.x, x6d, Rin, betas, Jt, JS, par, FT, AT, R0T, B, BP, step_inc, FTq, sh);
}
int launch_prep_fwd(const Model& m, const float* x6d, const float* Rin, const float* betas, float* FT, float* FTq, float* AT,
                    float* R0T, int B, int BP, int32_t* step_inc, hipStream_t s) {
  hipLaunchKernelGGL(k_prep_fwd, dim3(BP / PP), dim3(PP * NJ), 0, s, x6d, Rin, betas, m.Jt, m.JS, m.parents, FT, AT, R0T,
                     B, BP, step_inc, FTq);
  return 0;
}

// The 24 posed SMPL joints of the most recent chain forward (smplx lbs(): J_transformed = G_j[:3, 3], the `joints` field of the
// operator's output, /root/reference/scripts/smpl.py:69-84): G_j t = A_j t + A_j R . J_j(beta) from the stored skinning transforms
// AT [12][24][BP] and the folded rest-joint tables.  One thread per (pose, joint); out (B,24,3).
__global__ __launch_bounds__(256) void k_posed_joints(const float* __restrict__ AT, const float* __restrict__ betas,
                                                      const float* __restrict__ Jt, const float* __restrict__ JS,
                                                      float* __restrict__ out, int B, int BP) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;      // b fastest: coalesced reads of AT
  if (idx >= B * NJ) return;
  const int b = idx % B, j = idx / B;
  float beta[NB], J[3];
#pragma unroll
  for (int l = 0; l < NB; ++l) beta[l] = betas[(size_t)b * NB + l];
  rest_joint(Jt, JS, j, beta, J);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    float acc = AT[(size_t)((r * 4 + 3) * NJ + j) * BP + b];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc = fmaf(AT[(size_t)((r * 4 + c) * NJ + j) * BP + b], J[c], acc);
    out[((size_t)b * NJ + j) * 3 + r] = acc;
  }
}
int launch_posed_joints(const Model& m, const float* AT, const float* betas, float* out, int B, int BP, hipStream_t s) {
  hipLaunchKernelGGL(k_posed_joints, dim3((B * NJ + 255) / 256), dim3(256), 0, s, AT, betas, m.Jt, m.JS, out, B, BP);
  return 0;
}

// Adjoint of k_posed_joints: joints24[b][j][r] = A_{r,3}[j] + sum_c A_{r,c}[j] J_j(beta)[c]  ->  the skinning-transform adjoint dA^T
// [288][BP] (ONE slab for k_chain_bwd) and the direct shape term through the rest joints, gb (B,10) = sum_{j,c} (sum_r A_{r,c}[j] dj_r) JS
// (k_chain_bwd's gb_extra).  One thread per pose (a surface path: smpl(...).joints of scripts/smpl.py:69-84 is read by no caller).
__global__ __launch_bounds__(256) void k_posed_joints_bwd(const float* __restrict__ AT, const float* __restrict__ betas,
                                                          const float* __restrict__ Jt, const float* __restrict__ JS,
                                                          const float* __restrict__ dj24, float* __restrict__ dA,
                                                          float* __restrict__ gb, int B, int BP) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float beta[NB], g[NB];
#pragma unroll
  for (int l = 0; l < NB; ++l) { beta[l] = betas[(size_t)b * NB + l]; g[l] = 0.f; }
  for (int j = 0; j < NJ; ++j) {
    float J[3], d[3];
    rest_joint(Jt, JS, j, beta, J);
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = dj24[((size_t)b * NJ + j) * 3 + r];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) dA[(size_t)((r * 4 + c) * NJ + j) * BP + b] = d[r] * J[c];
      dA[(size_t)((r * 4 + 3) * NJ + j) * BP + b] = d[r];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float dJ = 0.f;
#pragma unroll
      for (int r = 0; r < 3; ++r) dJ = fmaf(AT[(size_t)((r * 4 + c) * NJ + j) * BP + b], d[r], dJ);
#pragma unroll
      for (int l = 0; l < NB; ++l) g[l] = fmaf(dJ, JS[(j * 3 + c) * NB + l], g[l]);
    }
  }
#pragma unroll
  for (int l = 0; l < NB; ++l) gb[(size_t)b * NB + l] = g[l];
}
int launch_posed_joints_bwd(const Model& m, const float* AT, const float* betas, const float* dj24, float* dA, float* gb, int B, int BP,
                            hipStream_t s) {
  hipLaunchKernelGGL(k_posed_joints_bwd, dim3((B + 255) / 256), dim3(256), 0, s, AT, betas, m.Jt, m.JS, dj24, dA, gb, B, BP);
  return 0;
}

// Horizontal fusion (fused inner loop with the pose discriminator): the chain forward and the discriminator's per-joint MLP
// both depend on x6d only and are both latency-bound with few workgroups (128 + 256 at 4096 poses) -- one launch, different
// CUs.  Every launch costs ~3.8 us of fixed time on this stack (a one-thread kernel measures that), so two independent small
// kernels side by side in one launch save one of those and the shorter kernel's whole duration.
struct DconvFwdArgs { const float* img; float* H2T; float* out; };
__global__ __launch_bounds__(PP * NJ) void k_prep_fwd_dconv(const float* __restrict__ x6d, const float* __restrict__ betas,
                                                            const float* __restrict__ Jt, const float* __restrict__ JS,
                                                            Parents par, float* __restrict__ FT, float* __restrict__ AT,
                                                            float* __restrict__ R0T, int B, int BP, int32_t* step_inc,
                                                            DconvFwdArgs d, int nprep, float* __restrict__ FTq) {
  // (one pool: a workgroup is either a chain-forward or a per-joint-MLP workgroup)
  __shared__ __attribute__((aligned(16))) float L[PREP_FWD_LDS > CL_FLOATS ? PREP_FWD_LDS : CL_FLOATS];
  if ((int)blockIdx.x < nprep) prep_fwd_body(blockIdx.x, x6d, nullptr, betas, Jt, JS, par, FT, AT, R0T, B, BP, step_inc, FTq, L);
  else dconv_fwd_body<true>(L, blockIdx.x - nprep, d.img, x6d, d.H2T, d.out, B, BP);
}
int launch_prep_fwd_dconv(const Model& m, const float* x6d, const float* betas, float* FT, float* FTq, float* AT, float* R0T, int B,
                          int BP, int32_t* step_inc, const float* img, float* H2T, float* out, hipStream_t s) {
  const int nprep = BP / PP;
  DconvFwdArgs d{img, H2T, out};
  hipLaunchKernelGGL(k_prep_fwd_dconv, dim3(nprep + (BP / 32) * 2), dim3(PP * NJ), 0, s, x6d, betas, m.Jt, m.JS, m.parents, FT, AT,
                     R0T, B, BP, step_inc, d, nprep, FTq);
  return 0;
}

// the chain adjoint + per-pose update (chain_bwd_body): the PoseUpdateArgs half of the launch record IS the kernel's argument
__global__ __launch_bounds__(PPB * NJ) void k_chain_bwd(const float* __restrict__ FT, const float* __restrict__ R0T,
                                                        const float* __restrict__ AT, const float* __restrict__ Jt,
                                                        const float* __restrict__ JS, Parents par,
                                                        const float* __restrict__ dA_, int nslabA, size_t strideA,
                                                        const float* __restrict__ dF_, PoseUpdateArgs ua, int B, int BP,
                                                        const unsigned* __restrict__ dmask) {
  __shared__ __attribute__((aligned(16))) float sh[CHAIN_BWD_LDS];
  chain_bwd_body(blockIdx.x, FT, R0T, AT, Jt, JS, par, dA_, nslabA, strideA, dF_, ua, B, BP, dmask, sh);
}
int launch_prep_bwd(const PrepBwdLaunch& L, const Model& m, hipStream_t s) {
  const PoseUpdateArgs& ua = L;
  hipLaunchKernelGGL(k_chain_bwd, dim3((L.B + PPB - 1) / PPB), dim3(PPB * NJ), 0, s, L.FT, L.R0T, L.AT, m.Jt, m.JS, m.parents,
                     L.dATp, L.nslabA, L.strideA, L.dFTp, ua, L.B, L.BP, L.dmaskA);
  return 0;
}

// Horizontal fusion of the two independent kernels that precede k_chain_bwd in the fused loop: the split-K slab sum of
// dF^T (bandwidth-bound, 58 MB) and the per-joint MLP adjoint of the discriminator (latency-bound).  Blocks [0, ndc) are the
// MLP workgroups (the longer dependency chain: dispatched first -- measured 2 us better than last), the rest stride over the
// slab sum.
struct DconvBwdArgs { const float* img; const float* x6d; const float* dH2T; const float* gout; float scale, target; float* gx; float* sqj; };
__global__ __launch_bounds__(256) void k_dconv_bwd_reduce(DconvBwdArgs d, int ndc, int B, int BP, const f32x4* __restrict__ P,
                                                          int nslab, size_t stride4, f32x4* __restrict__ out, size_t n4) {
  __shared__ __attribute__((aligned(16))) float L[CL_FLOATS];
  if ((int)blockIdx.x < ndc) {
    dconv_bwd_body<true>(L, blockIdx.x, d.img, d.x6d, d.dH2T, d.gout, d.scale, d.target, d.gx, B, BP, d.sqj);
  } else {
    const size_t nb = gridDim.x - ndc;
    for (size_t i = (size_t)(blockIdx.x - ndc) * blockDim.x + threadIdx.x; i < n4; i += nb * blockDim.x) {
      f32x4 acc = P[i];
      for (int sl = 1; sl < nslab; ++sl) acc += P[(size_t)sl * stride4 + i];
      out[i] = acc;
    }
  }
}
int launch_dconv_bwd_reduce(const float* img, const float* x6d, const float* dH2T, const float* gout, float scale, float target,
                            float* gx, float* sqj, int B, int BP, const float* P, int nslab, size_t stride, float* out, size_t n,
                            hipStream_t s) {
  const size_t n4 = n / 4;
  int rblocks = (int)((n4 + 255) / 256);
  if (rblocks > 4096) rblocks = 4096;
  const int ndc = (BP / 32) * 6;
  DconvBwdArgs d{img, x6d, dH2T, gout, scale, target, gx, sqj};
  hipLaunchKernelGGL(k_dconv_bwd_reduce, dim3(ndc + rblocks), dim3(256), 0, s, d, ndc, B, BP, (const f32x4*)P, nslab, stride / 4,
                     (f32x4*)out, n4);
  return 0;
}

// ------------------------------------------------------------------------------------------
// k_sup_step: ONE inner iteration of a 32-pose group in one workgroup (round 6; supk.h) -- the support-vertex form of
// scripts/optimize.py:220-265 without the silhouette and 2-D terms:
//   chain forward (k_prep_fwd's body) -> support-vertex SMPL forward, joint loss, backward (sup_body) -> [per-joint MLP adjoint of the
//   pose discriminator, whose four GEMM launches PRECEDE this kernel] -> chain adjoint + 6-D rotation adjoint + Adam (k_chain_bwd's
//   body) -> [per-joint MLP forward of the NEXT iteration on the updated poses].
// The phases hand F^T / A^T / dA^T / dF^T / gx over through global memory (the arrays their stand-alone kernels use; a workgroup reads
// only what it wrote itself, behind a workgroup barrier) and share one LDS pool.  With the discriminator an iteration is 4 GEMM
// launches + this one (13 launches on the tile lists); without it, this launch alone.
// Adam's step count: every workgroup reads the pre-increment value; the LAST workgroup to arrive (an agent-scope counter in the
// engine workspace, reset by that workgroup) stores value + 1 -- after every other workgroup has read.
// ------------------------------------------------------------------------------------------
struct SupStepArgs {
  const float* x6d; const float* betas; float* FT; float* FTq; float* AT; float* R0T;
  SupArgs sup;
  const float* conv_img;     // LDS image of the per-joint MLP, NULL without the pose discriminator
  const float* dH2T; float dscale; float* gx; float* dsq; float* H2T_next;
  PoseUpdateArgs ua;
  int32_t* step; int* arrive;
};
constexpr int SUP_STEP_LDS = SUPL_FLOATS > CHAIN_BWD_LDS ? (SUPL_FLOATS > PREP_FWD_LDS ? SUPL_FLOATS : PREP_FWD_LDS)
                                                         : (CHAIN_BWD_LDS > PREP_FWD_LDS ? CHAIN_BWD_LDS : PREP_FWD_LDS);
static_assert(SUP_STEP_LDS >= CL_FLOATS && SUP_PP == PP && SUP_PP == PPB && SUP_THREADS == PP * NJ, "one geometry for every phase");
// PHASE 0: the whole iteration.  PHASE 1 / 2 (JRR_SUP_OVERLAP, api.hip): its two halves as launches of their own -- 1 = everything that
// does not read the discriminator GEMMs' results (chain forward, support-vertex forward / loss / backward), on a second stream beside
// those GEMMs; 2 = the rest (per-joint MLP adjoint, chain adjoint + Adam, the next iteration's per-joint MLP forward), behind both.
constexpr int SUP_TAIL_CONV = CHAIN_BWD_LDS > PREP_FWD_LDS ? CHAIN_BWD_LDS : PREP_FWD_LDS;      // phase 2: the MLP image behind the chain pool
constexpr int SUP_TAIL_LDS = SUP_TAIL_CONV + CL_FLOATS;
template <int PHASE>
__global__ __launch_bounds__(SUP_THREADS) void k_sup_step(SupStepArgs a, const float* __restrict__ Jt, const float* __restrict__ JS,
                                                          Parents par) {
  extern __shared__ __attribute__((aligned(16))) float pool[];
  const int blk = blockIdx.x, B = a.sup.B, BP = a.sup.BP;
  int step_now = -1;
  if (PHASE != 1 && threadIdx.x == 0 && a.step) {
    const int s0 = __hip_atomic_load(a.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the value is in: only now may this workgroup count as arrived
    step_now = s0 + 1;
    const int prev = __hip_atomic_fetch_add(a.arrive, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == (int)gridDim.x - 1) {
      __hip_atomic_store(a.arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(a.step, step_now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  constexpr int CONV_AT = PHASE == 2 ? SUP_TAIL_CONV : SUPL_CONV;
  if (PHASE != 2) {
    prep_fwd_body(blk, a.x6d, nullptr, a.betas, Jt, JS, par, a.FT, a.AT, a.R0T, B, BP, nullptr, a.FTq, pool);
    __syncthreads();
    sup_body(pool, blk, a.sup);
    if (PHASE == 1) return;
    __syncthreads();
    // (the per-joint MLP adjoint closed the support body: one interleaved pair of joints per wave, supk.h)
  } else if (a.conv_img) {      // phase 2 opens with that adjoint (the first phase's launch ran the support body without it)
    conv_stage_params(a.conv_img, pool + CONV_AT);
    __syncthreads();
    // (two single tiles per wave, not dconv_bwd_pair: outside sup_body the compiler's back end refuses the pair's row pointers --
    // "illegal VGPR to SGPR copy" -- with any run-time joint index; the pair is 2.5 us faster where it compiles, sup_body)
    dconv_bwd_body<true, true>(pool + CONV_AT, 2 * blk, a.conv_img, a.x6d, a.dH2T, nullptr, a.dscale, 1.f, a.gx, B, BP, a.dsq);
    dconv_bwd_body<true, true>(pool + CONV_AT, 2 * blk + 1, a.conv_img, a.x6d, a.dH2T, nullptr, a.dscale, 1.f, a.gx, B, BP, a.dsq);
    __syncthreads();
  }
  chain_bwd_body(blk, a.FT, a.R0T, a.AT, Jt, JS, par, a.sup.dA, 1, 0, a.sup.dF, a.ua, B, BP, nullptr, pool, step_now);
  if (a.conv_img && a.H2T_next) {      // the updated poses of this group are complete: their per-joint MLP forward for the next iteration
    __syncthreads();
    // (the image the support body staged for the adjoint is still in place: the chain adjoint's pool ends far below it)
    static_assert(CHAIN_BWD_LDS <= SUPL_CONV && PREP_FWD_LDS <= SUPL_CONV, "the per-joint MLP image survives the chain phases");
    dconv_fwd_body<true, true>(pool + CONV_AT, 2 * blk, a.conv_img, a.ua.x6d_io, a.H2T_next, nullptr, B, BP);
    dconv_fwd_body<true, true>(pool + CONV_AT, 2 * blk + 1, a.conv_img, a.ua.x6d_io, a.H2T_next, nullptr, B, BP);
  }
  __syncthreads();
}

int launch_sup_step(const Model& m, const SupStepLaunch& q, const PrepBwdLaunch& L, hipStream_t s, int phase) {
  static const bool attr = [] {
    return hipFuncSetAttribute((const void*)k_sup_step<0>, hipFuncAttributeMaxDynamicSharedMemorySize, SUP_STEP_LDS * 4) == hipSuccess &&
           hipFuncSetAttribute((const void*)k_sup_step<1>, hipFuncAttributeMaxDynamicSharedMemorySize, SUP_STEP_LDS * 4) == hipSuccess &&
           hipFuncSetAttribute((const void*)k_sup_step<2>, hipFuncAttributeMaxDynamicSharedMemorySize, SUP_TAIL_LDS * 4) == hipSuccess;
  }();
  if (!attr) { jrr_set_error("k_sup_step: %d bytes of LDS refused", SUP_STEP_LDS * 4); return JRR_ERR_HIP; }
  SupStepArgs a;
  a.x6d = L.x6d_in; a.betas = L.betas_in; a.FT = q.FT; a.FTq = q.FTq; a.AT = q.AT; a.R0T = q.R0T;
  a.sup = SupArgs{q.t, q.nsv, q.Jn_vi, q.FTq, q.AT, q.gt_mm, q.scale, q.joints_out, q.sqerr, q.dA, q.dF, L.B, L.BP, q.rp,
                  phase == 0 ? q.conv_img : nullptr, L.x6d_in, q.dH2T, q.dscale, q.gx, q.dsq};      // (phases 1 / 2: the adjoint opens phase 2)
  a.conv_img = q.conv_img; a.dH2T = q.dH2T; a.dscale = q.dscale; a.gx = q.gx; a.dsq = q.dsq; a.H2T_next = q.H2T_next;
  a.ua = L;      // (its PoseUpdateArgs half)
  a.step = q.step; a.arrive = q.arrive;
  const dim3 grid((L.B + SUP_PP - 1) / SUP_PP), block(SUP_THREADS);
  if (phase == 1) hipLaunchKernelGGL(k_sup_step<1>, grid, block, SUP_STEP_LDS * 4, s, a, m.Jt, m.JS, m.parents);
  else if (phase == 2) hipLaunchKernelGGL(k_sup_step<2>, grid, block, SUP_TAIL_LDS * 4, s, a, m.Jt, m.JS, m.parents);
  else hipLaunchKernelGGL(k_sup_step<0>, grid, block, SUP_STEP_LDS * 4, s, a, m.Jt, m.JS, m.parents);
  return 0;
}

}  // namespace jrr
