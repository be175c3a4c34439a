// C ABI (include/jrr.h): the fused inner loop (jrr_refine_run*) and the J step (jrr_j_*, jrr_engine_support_*).
#include <algorithm>
#include <cstring>
#include <vector>

#include "engine.h"

using namespace jrr;

// joints^T partials from the STORED vertices: JPv[split][r][32][BP] = sum_{v in split} Jn[i,v] verts_r[v,b]
// (both operands in vertex quads: Jn_q [VP/4][32][4], VTb [3][VP/4][BP][4]; rows i >= 17 of Jn_q are zero)
int jrr::joints_from_stored_verts(jrr_engine* e, hipStream_t s, int32_t* step_inc) {
  // slab layout [split][plane][32][BP], what k_joints_loss reads with jp_rows = 32.  The support-restricted kernel writes ONE
  // complete slab (slab 0) when the regressor's support lists fit (device flag jsup.flag, which k_joints_loss also reads to
  // sum one slab only); otherwise it returns at once and the dense product below does the work -- and vice versa.
  if (e->st.have_jsup()) launch_rejoints_sparse(e->jsup, e->VTb, e->dFTp, e->BP, s, step_inc);
  // the host KNOWS that the lists fit (jrr_j_support_info; J steps only shrink the support): the dense product need not even be
  // enqueued (an idle launch still costs ~4.7 us of stream time)
  if (e->st.support_known()) return 0;
  return launch_gemm_q32(e->Jn_q, 32, 0, e->VTb, e->BP, (size_t)VP * e->BP, e->dFTp, e->BP, (size_t)3 * 32 * e->BP,
                         (size_t)32 * e->BP, e->BP, VP, 3, e->nsplit, s, e->st.have_jsup() ? e->jsup.flag : nullptr);
}

// =============================================================================================
// fused inner loop (scripts/optimize.py:220-265)
// =============================================================================================
// k-th record of the loss history: the five weighted terms of scripts/optimize.py:252-253 as this rank's share of the
// global means (sum over the local poses / the global denominators), from the per-pose sums the iteration left behind
__global__ void __launch_bounds__(1024) k_loss_record(const float* __restrict__ sqj, const float* __restrict__ sq2d,
                                                      const float* __restrict__ sqsil, const float* __restrict__ dsq,
                                                      const float* __restrict__ ssq, int B, int BP, float bnorm,
                                                      float* __restrict__ rec, float npix) {
  __shared__ float red[5][1024];
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b = threadIdx.x; b < B; b += 1024) {
    if (sq2d) acc[0] += sq2d[b];
    if (sqsil) acc[1] += sqsil[b];
    acc[2] += sqj[b];
    if (dsq) { float a = 0.f; for (int k = 0; k < 25; ++k) a += dsq[(size_t)k * BP + b]; acc[3] += a; }
    if (ssq) acc[4] += ssq[b];
  }
  for (int t = 0; t < 5; ++t) red[t][threadIdx.x] = acc[t];
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) for (int t = 0; t < 5; ++t) red[t][threadIdx.x] += red[t][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    rec[0] = red[0][0] / (bnorm * 34.f) * 0.01f;            // loss_j2d / 100
    rec[1] = red[1][0] / (bnorm * npix) * 100.f;            // silhouette_loss * 100
    rec[2] = red[2][0] / (bnorm * 51.f) * 10000.f;          // joint_loss * 10000
    rec[3] = red[3][0] / (bnorm * 25.f) * 10.f;             // pose_discriminated_loss * 10
    rec[4] = red[4][0] / bnorm * 10.f;                      // shape_discriminated_loss * 10
  }
}

// Shared-parameter state of the in-call J steps (jrr_refine_run_j_steps)
struct JStepArgs { int every; float* J; float* m; float* v; int32_t* step; float lr; const float* mask; float* sqerr; bool reuse; };

// What every iteration of one call shares
struct RefineCtx {
  jrr_engine* e;
  float *x6d, *betas; const float* gt_mm; float *adam_m, *adam_v; int32_t* step; float lr;      // the caller's
  float* sqerr;                                  // the caller's per-pose joint errors, or the engine's own
  bool pd, sd;                                   // adversarial terms active
  float jscale, dscale, sscale, scale2d;         // d(weighted mean)/d(squared error) of the joint, pose-D, shape-D and 2-D terms
  hipStream_t s;
};

// ---- pieces every iteration shape is made of ----
// the 2-D reprojection term (weight 1/100) as the joint-loss kernels take it; without 2-D ground truth it is off
static Reproj reproj_term(const RefineCtx& c) {
  jrr_engine* e = c.e;
  return e->gt_j2d ? Reproj{e->gt_j2d, e->cam, e->gcam, e->sq2d, c.scale2d} : Reproj{};
}

// pose-D forward + input adjoint (four GEMMs) and the shape-D launch.  conv_done: the per-joint MLP forward is in H2T already;
// skip_conv: its adjoint runs in a later launch of the caller's
static int adversarial_terms(const RefineCtx& c, bool conv_done, bool skip_conv) {
  jrr_engine* e = c.e;
  if (c.pd) {
    prof_mark(e, 5, c.s);
    int rc = disc_forward(e, c.x6d, nullptr, c.s, true, conv_done);
    if (rc) return rc;
    rc = disc_backward_input(e, c.x6d, nullptr, nullptr, c.dscale, 1.f, e->gx, c.s, e->dsq, skip_conv);
    prof_mark(e, 5, c.s);
    if (rc) return rc;
  }
  if (c.sd) {
    prof_mark(e, 6, c.s);
    launch_shape_disc(e->Ps, c.betas, nullptr, e->gb, c.sscale, 1.f, e->B, c.s, nullptr, e->ssq);
    prof_mark(e, 6, c.s);
  }
  return 0;
}

// scripts/optimize.py:255-261: the five weighted terms every `hist_every`-th iteration
static void record_history(const RefineCtx& c, const float* sqsil) {
  jrr_engine* e = c.e;
  if (!e->hist) return;
  if (e->hist_iter % e->hist_every == 0 && e->hist_n < e->hist_cap) {
    hipLaunchKernelGGL(k_loss_record, dim3(1), dim3(1024), 0, c.s, c.sqerr, e->gt_j2d ? e->sq2d : nullptr, sqsil, c.pd ? e->dsq : nullptr,
                       c.sd ? e->ssq : nullptr, e->B, e->BP, (float)e->bnorm, e->hist + (size_t)e->hist_n * 5, (float)(e->sil * e->sil));
    ++e->hist_n;
  }
  ++e->hist_iter;
}

// scripts/optimize.py:300-312 inside the call (single process: no collective)
static int in_call_j_step(const RefineCtx& c, const JStepArgs& js, bool& reuse_next) {
  jrr_engine* e = c.e;
  int rc = j_step_local(e, c.x6d, c.betas, c.gt_mm, e->dJraw, js.sqerr, c.s, nullptr, nullptr, true);
  if (rc) return rc;
  rc = j_step_apply(e, js.J, e->dJraw, js.m, js.v, js.step, js.lr, js.mask, c.s);
  if (rc) return rc;
  reuse_next = js.reuse;
  if (!js.reuse) e->st.workspace_overwritten();
  return 0;
}

// the pose update's side of a chain adjoint (k_chain_bwd + Adam): the caller's buffers, the adversarial gradients, and the camera
// translation when a term moves it -- a parameter of the same Adam (2-D term, optimize.py:231-233,252; silhouette)
static void fill_chain_adjoint(const RefineCtx& c, PrepBwdLaunch& L, bool sil) {
  jrr_engine* e = c.e;
  L.x6d_in = c.x6d; L.betas_in = c.betas; L.gx_extra = c.pd ? e->gx : nullptr; L.gb_extra = c.sd ? e->gb : nullptr;
  L.x6d_io = c.x6d; L.betas_io = c.betas; L.adam_m = c.adam_m; L.adam_v = c.adam_v; L.step = c.step; L.lr = c.lr; L.B = e->B; L.BP = e->BP;
  if (e->gt_j2d || sil) { L.gcam = e->gcam; L.cam_io = e->cam; L.cam_m = e->cam_m; L.cam_v = e->cam_v; }
}

// the side stream and its two events: all three or none
static int ensure_side_stream(jrr_engine* e) {
  if (e->side) return JRR_OK;
  hipStream_t side = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  hipError_t he = hipStreamCreateWithFlags(&side, hipStreamNonBlocking);
  if (he != hipSuccess) side = nullptr;
  if (he == hipSuccess && (he = hipEventCreateWithFlags(&fork, hipEventDisableTiming)) != hipSuccess) fork = nullptr;
  if (he == hipSuccess && (he = hipEventCreateWithFlags(&join, hipEventDisableTiming)) != hipSuccess) join = nullptr;
  if (he != hipSuccess) {
    if (join) (void)hipEventDestroy(join);
    if (fork) (void)hipEventDestroy(fork);
    if (side) (void)hipStreamDestroy(side);
    jrr_set_error("side stream: %s", hipGetErrorString(he));
    return JRR_ERR_HIP;
  }
  e->side = side; e->ev_fork = fork; e->ev_join = join;
  return JRR_OK;
}

// ---- iteration shapes ----
// Support-vertex iteration (supk.h): forward, loss, backward and pose update of a 32-pose group in ONE launch per iteration
// (+ the four discriminator GEMMs before it): chain.hip k_sup_step.  h2t_ready: the previous iteration's launch left the per-joint
// MLP forward of the current poses in H2T; `last`: no iteration of this call follows.
static int iter_support_step(const RefineCtx& c, bool last, bool& h2t_ready) {
  jrr_engine* e = c.e;
  hipStream_t s = c.s;
  prof_mark(e, 0, s);
  // per-joint MLP forward: left behind by the previous iteration's launch, except before the first one of a call
  if (c.pd && !h2t_ready) launch_disc_conv_fwd(e->convL, c.x6d, e->H2T, nullptr, e->B, e->BP, s, 1);
  prof_mark(e, 0, s);
  // Small batches with the pose discriminator: the iteration's GEMM-independent half (k_sup_step<1>: chain forward, support-vertex
  // forward / loss / backward -- 38 of the launch's 70 us, on B / 32 workgroups) runs on the engine's side stream BESIDE the four GEMM
  // launches, the rest (k_sup_step<2>) behind both.  Fork: the side stream waits for everything enqueued on `s` so far (the previous
  // iteration's pose update); join: `s` waits for the side launch before the second half.  Same bits as the composed kernel.  Same
  // box, ms per iteration composed -> overlapped: 256 poses 0.134 -> 0.112, 512: 0.135 -> 0.126, 1024: 0.162 -> 0.160, 4096:
  // 0.336 -> 0.345 (the half-chip launch takes CUs from GEMMs that fill the chip): on up to 512 poses.  JRR_SUP_OVERLAP=0 / 1: never / always.
  const int want = knobs().sup_overlap;
  const bool overlap = c.pd && (want < 0 ? e->B <= 512 : want == 1);
  if (overlap) { int rc = ensure_side_stream(e); if (rc) return rc; }
  SupStepLaunch q;
  q.t = e->sup; q.nsv = e->st.sup_nsv(); q.Jn_vi = e->Jn_vi; q.gt_mm = c.gt_mm; q.scale = c.jscale;
  q.FT = e->FT; q.FTq = e->FTq; q.AT = e->AT; q.R0T = e->R0T; q.joints_out = e->joints; q.sqerr = c.sqerr;
  q.dA = e->dA; q.dF = e->dF;
  if (c.pd) {
    q.conv_img = e->convL; q.dH2T = e->dH2T; q.dscale = c.dscale; q.gx = e->gx; q.dsq = e->dsq;
    q.H2T_next = last ? nullptr : e->H2T;
  }
  q.step = c.step; q.arrive = e->step_scratch;
  q.rp = reproj_term(c);
  PrepBwdLaunch L;
  fill_chain_adjoint(c, L, false);
  if (overlap) {
    JRR_HIP(hipEventRecord(e->ev_fork, s));
    JRR_HIP(hipStreamWaitEvent(e->side, e->ev_fork, 0));
    int rc = launch_sup_step(e->m, q, L, e->side, 1);
    if (rc) return rc;
    JRR_HIP(hipEventRecord(e->ev_join, e->side));
  }
  int rc = adversarial_terms(c, true, true);
  if (rc) return rc;
  if (overlap) JRR_HIP(hipStreamWaitEvent(s, e->ev_join, 0));
  prof_mark(e, 1, s);
  rc = launch_sup_step(e->m, q, L, s, overlap ? 2 : 0);
  if (rc) return rc;
  h2t_ready = c.pd && q.H2T_next != nullptr;
  prof_mark(e, 1, s);
  return 0;
}

// chain forward (+ Adam's step count) of the chain iterations; with the pose discriminator its per-joint MLP rides in the same launch
// (two independent latency-bound kernels side by side: chain.hip).  reuse: the forward of the J step before stands; only the count moves.
static void chain_forward(const RefineCtx& c, bool reuse) {
  jrr_engine* e = c.e;
  prof_mark(e, 0, c.s);
  if (reuse) { if (!e->st.have_jsup()) launch_step_inc(c.step, c.s); }      // (with support lists the count rides in k_rejoints_sparse)
  else if (c.pd) launch_prep_fwd_dconv(e->m, c.x6d, c.betas, e->FT, e->FTq, e->AT, e->R0T, e->B, e->BP, c.step, e->convL, e->H2T, nullptr, c.s);
  else launch_prep_fwd(e->m, c.x6d, nullptr, c.betas, e->FT, e->FTq, e->AT, e->R0T, e->B, e->BP, c.step, c.s);
  prof_mark(e, 0, c.s);
}

// joints from `nslab` partial slabs of `rows` rows, joint (+ 2-D) loss and the joint adjoint dJT
static void joints_loss(const RefineCtx& c, const float* partials, int nslab, int rows, const int* one_slab_flag) {
  jrr_engine* e = c.e;
  launch_joints_loss(partials, nslab, c.gt_mm, nullptr, c.jscale, e->joints, c.sqerr, e->dJT, e->B, e->BP, c.s, reproj_term(c), rows, one_slab_flag);
}

// the pose update from COMPLETE adjoints dA^T / dF^T (L.dATp / L.dFTp set by the caller) and the forward the chain kept
static void pose_update(const RefineCtx& c, PrepBwdLaunch& L, bool sil) {
  jrr_engine* e = c.e;
  fill_chain_adjoint(c, L, sil);
  L.FT = e->FT; L.R0T = e->R0T; L.AT = e->AT; L.dRT = e->dRT; L.dbT = e->dbT;
  launch_prep_bwd(L, e->m, c.s);
  prof_mark(e, 7, c.s);
}

// Folded regressor (fold.hip): the joints straight from the blend features, no vertices
static int iter_folded(const RefineCtx& c) {
  jrr_engine* e = c.e;
  hipStream_t s = c.s;
  chain_forward(c, false);
  prof_mark(e, 1, s);
  GemmArgs g;   // M^T[(i,j,c)][b] = sum_k H[(i,j,c)][k] F^T[k][b]
  g.A = e->Hk; g.lda = FOLD_M; g.Bm = e->FT; g.ldb = e->BP; g.Out = e->MT; g.ldo = e->BP;
  g.bias = nullptr; g.mask = nullptr; g.split_stride = 0; g.M = FOLD_M; g.N = e->BP; g.K = KFP;
  int rc = launch_gemm_128x64(g, EPI_STORE, 1, s);
  if (rc) return rc;
  launch_fold_fwd(e->MT, e->AT, e->G0, e->Jsum, e->BP, s);
  prof_mark(e, 1, s);
  prof_mark(e, 2, s);
  joints_loss(c, e->Jsum, 1, NH, nullptr);
  prof_mark(e, 2, s);
  prof_mark(e, 3, s);
  launch_fold_bwd(e->dJT, e->AT, e->MT, e->G0, e->dMT, e->dA, e->BP, s);
  prof_mark(e, 3, s);
  prof_mark(e, 4, s);
  GemmArgs h;   // dF^T[k][b] = sum_m H[m][k] dM^T[m][b]   (split over m, partial slabs)
  h.A = e->Hm; h.lda = KFP; h.Bm = e->dMT; h.ldb = e->BP; h.Out = e->dFTp; h.ldo = e->BP;
  h.bias = nullptr; h.mask = nullptr; h.split_stride = (size_t)KFP * e->BP; h.M = KFP; h.N = e->BP; h.K = FOLD_M;
  rc = launch_gemm_224(h, EPI_STORE, e->nsplit, s);
  prof_mark(e, 4, s);
  if (rc) return rc;
  rc = adversarial_terms(c, c.pd, false);
  if (rc) return rc;
  prof_mark(e, 7, s);
  launch_reduce_slabs(e->dFTp, e->nsplit, (size_t)KFP * e->BP, e->dF, (size_t)KFP * e->BP, s);
  PrepBwdLaunch L;
  L.dATp = e->dA; L.dFTp = e->dF;
  pose_update(c, L, false);
  return 0;
}

// JRR_SUPPORT_FUSED=2 (verification / A-B knob): the support-vertex iteration as separate launches (chain forward, k_sup_iter, per-joint
// MLP adjoint, chain adjoint) instead of the composed kernel k_sup_step.  The empty profile brackets keep the classes' counts in step.
static int iter_support_split(const RefineCtx& c) {
  jrr_engine* e = c.e;
  hipStream_t s = c.s;
  chain_forward(c, false);
  prof_mark(e, 1, s);
  int rc = launch_sup_iter(e->sup, e->st.sup_nsv(), e->Jn_vi, e->FTq, e->AT, c.gt_mm, c.jscale, e->joints, c.sqerr, e->dA, e->dF, e->B, e->BP, s,
                           reproj_term(c));
  if (rc) return rc;
  prof_mark(e, 1, s);
  for (int cls = 2; cls <= 4; ++cls) { prof_mark(e, cls, s); prof_mark(e, cls, s); }
  rc = adversarial_terms(c, c.pd, true);
  if (rc) return rc;
  prof_mark(e, 7, s);
  // dA^T / dF^T arrive complete: nothing to sum; the per-joint MLP adjoint runs alone
  if (c.pd) launch_disc_conv_bwd(e->convL, c.x6d, e->dH2T, nullptr, c.dscale, 1.f, e->gx, e->B, e->BP, s, e->dsq, 1);
  PrepBwdLaunch L;
  L.dATp = e->dA; L.dFTp = e->dF;
  pose_update(c, L, false);
  return 0;
}

// The LBS chain: k_lbs_fwd -> joint loss (-> silhouette) -> k_lbs_bwd -> blend adjoint -> slab sums -> pose update.
// listed: on the tiles of the regressor's support only; reuse: the joints are re-regressed from the vertices the J step before stored
// (jrr_refine_run_after_j_step) instead of repeating the forward; sil: with the silhouette term.
static int iter_chain(const RefineCtx& c, bool listed, bool reuse, bool sil) {
  jrr_engine* e = c.e;
  hipStream_t s = c.s;
  const int* tl = listed ? e->act_list : nullptr;
  const int ntl = listed ? e->st.nact() : 0;
  // split-K of the blend adjoint: its K range is 6 chunks per listed tile -- at least JRR_ADJ_CHUNKS (6) chunks per split, so that a
  // handful of tiles does not leave 16 slabs of 3.7 MB (at 4096 poses) for the slab sum to read (6 tiles, 4096 poses: 6 splits
  // 0.3575 ms per iteration, 16 splits 0.3623, 4 splits 0.3618, 2 splits 0.377)
  // (and never fewer than ~128 workgroups in the launch: small batches have few 128-pose tiles)
  const int adj_chunks = knobs().adj_chunks;
  const int ns_adj = listed ? std::max(1, std::min(e->nsplit, std::max((6 * ntl + adj_chunks - 1) / adj_chunks, (128 * 128 + e->BP - 1) / e->BP))) : 0;
  chain_forward(c, reuse);
  prof_mark(e, 1, s);
  if (reuse) {
    int rc = joints_from_stored_verts(e, s, c.step);
    if (rc) return rc;
  } else {
    // (silhouette iterations: the vertices go to the pose-major buffer the rasteriser reads; VTb then only receives the
    // rasteriser's vertex adjoint -- its stored vertices are no longer those of this forward: verts_partial)
    const bool silf = e->sil_mask != nullptr;
    int rc = launch_lbs_fwd(e->m, e->Jn_vi, e->FTq, e->AT, e->VPb, e->JP, silf ? e->VPM : nullptr, e->B, e->BP, e->nvc, s,
                            e->profiling ? e->probe : nullptr, nullptr, tl, ntl, silf ? 1 : 0);
    if (rc) return rc;
  }
  prof_mark(e, 1, s);
  prof_mark(e, 2, s);
  if (reuse) joints_loss(c, e->dFTp, e->nsplit, 32, e->st.have_jsup() ? e->jsup.flag : nullptr);
  else joints_loss(c, e->JP, e->nvc, NH, nullptr);
  prof_mark(e, 2, s);
  if (sil) {   // 100 * mean((silhouette - mask)^2), optimize.py:234-237,252
    prof_mark(e, 8, s);
    const float silscale = (float)(2.0 * 100.0 / ((double)e->bnorm * (double)e->sil * (double)e->sil));
    if (!e->st.smask_valid()) { launch_mask_sq(e->sil_mask, e->smask, e->B, s, e->sil); e->st.mask_sums_computed(); }
    // projection, rasterisation, loss and adjoint in one kernel, straight from / into the row-quad vertex buffer
    launch_sil_raster_adj(e->VTb, e->BP, e->cam, e->m.faces_int_pk ? e->m.faces_int_pk : e->m.faces_pk, e->m.nfaces, e->sil_mask, e->smask, e->cover, e->ncover, e->sqsil,
                          silscale, e->gcam, e->gt_j2d ? 1 : 0, e->B, s, e->sil, e->VPM);
    prof_mark(e, 8, s);
  }
  prof_mark(e, 3, s);
  int rc = launch_lbs_bwd(e->m, e->Jn_iv, e->AT, e->VPb, e->dJT, sil ? e->VTb : nullptr, e->DVP, e->dATp, e->BP, e->nvcb, s, tl, ntl, slab_masks(e));
  if (rc) return rc;
  prof_mark(e, 3, s);
  prof_mark(e, 4, s);
  rc = blend_adjoint_gemm(e, s, tl, ntl, ns_adj);
  prof_mark(e, 4, s);
  if (rc) return rc;
  rc = adversarial_terms(c, c.pd && !reuse, true);
  if (rc) return rc;
  prof_mark(e, 7, s);
  reduce_adjoint_partials(e, s, c.pd ? c.x6d : nullptr, c.dscale, ns_adj);      // (with the pose discriminator: + the per-joint MLP adjoint)
  PrepBwdLaunch L;
  set_adjoint_slabs(e, L);
  pose_update(c, L, sil);
  return 0;
}

static int refine_run_impl(jrr_engine_t* e, float* x6d, float* betas, const float* gt_mm, float* adam_m,
                           float* adam_v, int32_t* step, float lr, int n_iters, float* sqerr, bool reuse_first,
                           const JStepArgs* js, void* stream) {
  if (!e || !x6d || !betas || !gt_mm || !adam_m || !adam_v || !step || n_iters < 0) { jrr_set_error("refine_run: bad argument"); return JRR_ERR_ARG; }
  if (!e->st.have_J()) { jrr_set_error("J_regressor not set"); return JRR_ERR_STATE; }
  RefineCtx c;
  c.e = e; c.x6d = x6d; c.betas = betas; c.gt_mm = gt_mm; c.adam_m = adam_m; c.adam_v = adam_v; c.step = step; c.lr = lr;
  c.sqerr = sqerr ? sqerr : e->sqerr;
  c.pd = (e->flags & JRR_FLAG_POSE_DISC) && e->have_pd;
  c.sd = (e->flags & JRR_FLAG_SHAPE_DISC) && e->have_sd;
  c.jscale = (float)(2.0 * 10000.0 / ((double)e->bnorm * 51.0));   // optimize.py:252 weight 10000
  c.dscale = (float)(2.0 * 10.0 / ((double)e->bnorm * 25.0));      // optimize.py:253 weight 10
  c.sscale = (float)(2.0 * 10.0 / ((double)e->bnorm * 1.0));
  c.scale2d = (float)(2.0 * 0.01 / ((double)e->bnorm * 34.0));     // optimize.py:231-233,252 weight 1/100
  c.s = (hipStream_t)stream;
  if (reuse_first) {
    // the caller states that the previous call on this engine was the J step on exactly these poses and that nothing
    // has written them since; everything the engine can check is checked
    if (!(e->st.stored_forward_is(x6d, betas) && e->VTb != nullptr)) {
      jrr_set_error("refine_run_after_j_step: the previous call on this engine was not jrr_j_regressor_grad on the same pose buffers");
      return JRR_ERR_STATE;
    }
  }
  bool reuse_next = reuse_first;      // the J step before this iteration left its forward (v_posed, skinning transforms, vertices) of exactly these poses
  bool h2t_ready = false;             // (iter_support_step)
  for (int it = 0; it < n_iters; ++it) {
    const bool folded = e->st.folded_active();
    const bool listed = use_tile_list(e);
    const bool supv = use_sup_vertices(e);
    const bool sil = e->sil_mask != nullptr && !folded;
    int rc;
    if (supv) {
      // its forward costs less than re-regressing the stored vertices: a pending reuse is dropped, not taken
      e->st.workspace_overwritten(); reuse_next = false;
      rc = knobs().support_fused == 2 ? iter_support_split(c) : iter_support_step(c, it + 1 == n_iters, h2t_ready);
    } else {
      const bool reuse = reuse_next && e->st.fwd_cached() && !folded && e->sil_mask == nullptr && e->st.stored_verts_usable();
      reuse_next = false;
      e->st.workspace_overwritten();
      rc = folded ? iter_folded(c) : iter_chain(c, listed, reuse, sil);
    }
    if (rc) return rc;
    record_history(c, sil ? e->sqsil : nullptr);
    if (js && (it + 1) % js->every == 0) {
      rc = in_call_j_step(c, *js, reuse_next);
      if (rc) return rc;
    }
  }
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_refine_run(jrr_engine_t* e, float* x6d, float* betas, const float* gt_mm, float* adam_m,
                              float* adam_v, int32_t* step, float lr, int n_iters, float* sqerr, void* stream) {
  return refine_run_impl(e, x6d, betas, gt_mm, adam_m, adam_v, step, lr, n_iters, sqerr, false, nullptr, stream);
}

extern "C" int jrr_refine_run_after_j_step(jrr_engine_t* e, float* x6d, float* betas, const float* gt_mm, float* adam_m,
                                           float* adam_v, int32_t* step, float lr, int n_iters, float* sqerr, void* stream) {
  return refine_run_impl(e, x6d, betas, gt_mm, adam_m, adam_v, step, lr, n_iters, sqerr, true, nullptr, stream);
}

extern "C" int jrr_refine_run_j_steps(jrr_engine_t* e, float* x6d, float* betas, const float* gt_mm, float* adam_m,
                                      float* adam_v, int32_t* step, float lr, int n_iters, float* sqerr, int j_every,
                                      float* J, float* J_m, float* J_v, int32_t* J_step, float j_lr, const float* mask,
                                      float* j_sqerr, int after_j_step, void* stream) {
  if (!e || j_every <= 0 || !J || !J_m || !J_v || !J_step) { jrr_set_error("refine_run_j_steps: bad argument"); return JRR_ERR_ARG; }
  if (!(e->flags & JRR_FLAG_KEEP_VERTS)) { jrr_set_error("J step requires JRR_FLAG_KEEP_VERTS"); return JRR_ERR_STATE; }
  JStepArgs js{j_every, J, J_m, J_v, J_step, j_lr, mask, j_sqerr, (after_j_step & 2) == 0};
  return refine_run_impl(e, x6d, betas, gt_mm, adam_m, adam_v, step, lr, n_iters, sqerr, (after_j_step & 1) != 0, &js, stream);
}

extern "C" int jrr_refine_aux_losses(jrr_engine_t* e, float* pose_disc_sq, float* shape_disc_sq, void* stream) {
  if (!e) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  hipStream_t s = (hipStream_t)stream;
  if (pose_disc_sq) {
    if (!((e->flags & JRR_FLAG_POSE_DISC) && e->have_pd)) { jrr_set_error("pose discriminator term not active"); return JRR_ERR_STATE; }
    launch_colsum(e->dsq, 25, e->BP, pose_disc_sq, e->B, s);
  }
  if (shape_disc_sq) {
    if (!((e->flags & JRR_FLAG_SHAPE_DISC) && e->have_sd)) { jrr_set_error("shape discriminator term not active"); return JRR_ERR_STATE; }
    JRR_HIP(hipMemcpyAsync(shape_disc_sq, e->ssq, (size_t)e->B * 4, hipMemcpyDeviceToDevice, s));
  }
  CHECK_LAUNCH();
  return JRR_OK;
}

// =============================================================================================
// J step (scripts/optimize.py:300-312)
// =============================================================================================
// dJn[i][v] = sum over the (plane, pose-split) slabs P[s][i][v]
__global__ void k_djn_reduce(const float* __restrict__ P, int nslab, float* __restrict__ dJn, const int* __restrict__ skip) {
  if (skip && *skip) return;                   // the support-restricted product wrote dJn itself
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= NH * VP) return;
  int i = idx / VP, v = idx % VP;
  float acc = 0.f;
  for (int s = 0; s < nslab; ++s) acc += P[((size_t)s * 32 + i) * VP + v];
  dJn[idx] = acc;
}

// dJ from the joint adjoint dJT [3][18][BP] (already in the engine) and the stored vertices VTb [3][VP][BP]
int jrr::j_grad_from_verts(jrr_engine* e, float* dJ, hipStream_t s, float* dJs) {
  if (!(e->flags & JRR_FLAG_KEEP_VERTS)) { jrr_set_error("dJ requires an engine created with JRR_FLAG_KEEP_VERTS"); return JRR_ERR_STATE; }
  if (!e->st.stored_verts_usable()) {
    jrr_set_error("dJ: the stored vertices are those of a J step over the regressor's support; run jrr_find_joints_forward first");
    return JRR_ERR_STATE;
  }
  // over the regressor's support when its lists fit (jreg.hip, "J step over the regressor's SUPPORT"), else the dense product
  const int* sflag = e->st.have_jsup() ? e->jsup.flag : nullptr;
  if (e->st.have_jsup()) launch_jgrad_sparse(e->jsup, e->dJT, e->VTb, e->dJn, e->BP, s);
  if (!e->st.support_known()) {      // (known to fit: the dense product and its slab sum are not even enqueued)
    int rc = launch_jgrad_q(e->dJT, e->VTb, e->dJnp, e->BP, e->nsplitJ, s, sflag);
    if (rc) return rc;
    hipLaunchKernelGGL(k_djn_reduce, dim3((NH * VP + 255) / 256), dim3(256), 0, s, e->dJnp, 3 * e->nsplitJ, e->dJn, sflag);
  }
  launch_jreg_bwd(e->Jraw, e->st.have_mask() ? e->Jmask : nullptr, e->Jn, e->rowsum, e->dJn, VP, dJ, e->m.v2p, s,
                  dJs ? &e->jsup : nullptr, e->m.p2v, dJs);      // dJs: the same gradient on the support lists, same launch
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_j_regressor_grad(jrr_engine_t* e, const float* x6d, const float* betas, const float* gt_mm,
                                    float* dJ, float* sqerr, float* joints, void* stream) {
  if (!e || !x6d || !betas || !gt_mm || !dJ) return JRR_ERR_ARG;
  if (!e->st.have_J()) { jrr_set_error("J_regressor not set"); return JRR_ERR_STATE; }
  if (!(e->flags & JRR_FLAG_KEEP_VERTS)) { jrr_set_error("J step requires JRR_FLAG_KEEP_VERTS"); return JRR_ERR_STATE; }
  return j_step_local(e, x6d, betas, gt_mm, dJ, sqerr, (hipStream_t)stream, joints);
}

// find_joints on the poses of the J step that preceded, with the CURRENT (stepped) regressor, from that step's stored vertices: the
// joints the driver evaluates after the step (scripts/optimize.py:317-321) without a second SMPL forward
extern "C" int jrr_find_joints_after_j_step(jrr_engine_t* e, const float* x6d, const float* betas, float* joints, void* stream) {
  if (!e || !x6d || !betas || !joints) { jrr_set_error("find_joints_after_j_step: null"); return JRR_ERR_ARG; }
  if (!e->st.have_J()) { jrr_set_error("J_regressor not set"); return JRR_ERR_STATE; }
  if (!(e->st.stored_forward_is(x6d, betas) && e->VTb != nullptr && e->st.stored_verts_usable())) {
    jrr_set_error("find_joints_after_j_step: the previous forward on this engine was not a J step (jrr_j_regressor_grad*) on the same pose buffers");
    return JRR_ERR_STATE;
  }
  hipStream_t s = (hipStream_t)stream;
  int rc = joints_from_stored_verts(e, s);
  if (rc) return rc;
  launch_joints_loss(e->dFTp, e->nsplit, nullptr, nullptr, 0.f, joints, nullptr, nullptr, e->B, e->BP, s, Reproj{}, 32,
                     e->st.have_jsup() ? e->jsup.flag : nullptr);
  CHECK_LAUNCH();
  return JRR_OK;
}

// ---- the J step's all-reduce payload restricted to the regressor's support (include/jrr.h) ----
extern "C" int jrr_j_support_info(jrr_engine_t* e, int32_t* counts_host, int32_t* fits_host, void* stream) {
  if (!e || !fits_host) return JRR_ERR_ARG;
  if (!e->st.have_jsup() || !e->st.have_J()) { jrr_set_error("j_support_info: needs JRR_FLAG_KEEP_VERTS and a regressor"); return JRR_ERR_STATE; }
  int32_t cnt[32] = {0}, flag = 0;
  JRR_HIP(hipStreamSynchronize((hipStream_t)stream));
  JRR_HIP(hipMemcpy(cnt, e->jsup.cnt, NH * sizeof(int32_t), hipMemcpyDeviceToHost));
  JRR_HIP(hipMemcpy(&flag, e->jsup.flag, sizeof(int32_t), hipMemcpyDeviceToHost));
  {   // sticky device error: since the last call the support left the tiles reported then / stopped fitting the lists, while the engine
      // enqueued support-restricted work only (the caller changed J or the mask IN PLACE instead of announcing it through
      // jrr_engine_set_j_regressor): every result since then is suspect.  Cleared by reporting it.
    int32_t err = 0;
    JRR_HIP(hipMemcpy(&err, e->jsup.flag + JSUP_ERR, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (err) {
      JRR_HIP(hipMemset(e->jsup.flag + JSUP_ERR, 0, 2 * sizeof(int32_t)));      // error word and KNOWN
      e->st.support_grew_unannounced();
      jrr_set_error("the J_regressor's support GREW behind the engine's back (%s): J or its mask was edited in place after "
                    "jrr_j_support_info; results since then are invalid -- announce a changed regressor with jrr_engine_set_j_regressor",
                    (err & 2) ? "a row no longer fits the support lists" : "entries outside the reported tiles");
      return JRR_ERR_STATE;
    }
  }
  if (counts_host) for (int i = 0; i < NH; ++i) counts_host[i] = cnt[i];
  *fits_host = flag;
  e->st.support_reported(flag != 0);
  {   // the baseline the device checks later supports against (k_jsup_tilemask)
    const int32_t known = flag ? 1 : 0;
    if (flag) JRR_HIP(hipMemcpy(e->jsup.tknown, e->jsup.tmask, VT * sizeof(int32_t), hipMemcpyDeviceToDevice));
    JRR_HIP(hipMemcpy(e->jsup.flag + JSUP_KNOWN, &known, sizeof(int32_t), hipMemcpyHostToDevice));
  }
  if (flag && (e->flags & JRR_FLAG_SUPPORT_TILES)) {      // the support's tiles, for the kernels of the joint-loss iteration
    int32_t tm[VT], list[VT];
    JRR_HIP(hipMemcpy(tm, e->jsup.tmask, VT * sizeof(int32_t), hipMemcpyDeviceToHost));
    int n = 0;
    for (int t = 0; t < VT; ++t) if (tm[t]) list[n++] = t;
    if (n > 0) {
      JRR_HIP(hipMemcpy(e->act_list, list, n * sizeof(int32_t), hipMemcpyHostToDevice));
      e->st.tile_list_built(n);
    }
    // the support's VERTICES (union of the rows' lists): up to SUP_NSV of them run the per-vertex iteration (supk.h).  J steps only
    // shrink the support, so the set stays a superset; the regressor's values are read live (Jn_vi) at every iteration.
    if (n > 0 && knobs().support_fused != 0) {
      std::vector<int32_t> col((size_t)NH * JSUP_CAP);
      JRR_HIP(hipMemcpy(col.data(), e->jsup.col, col.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      std::vector<char> seen(VP, 0);
      bool in_range = true;
      for (int i = 0; i < NH; ++i)
        for (int k = 0; k < cnt[i] && k < JSUP_CAP; ++k) {
          const int r = col[(size_t)i * JSUP_CAP + k];
          if (r < 0 || r >= VP) { in_range = false; break; }
          seen[r] = 1;
        }
      std::vector<int32_t> rows;
      for (int r = 0; r < VP; ++r) if (seen[r]) rows.push_back(r);
      if (in_range && !rows.empty() && (int)rows.size() <= SUP_NSV) {
        JRR_HIP(hipMemcpy(e->sup.rows, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        launch_sup_gather(e->m, e->sup, (int)rows.size(), (hipStream_t)stream);
        JRR_HIP(hipStreamSynchronize((hipStream_t)stream));
        e->st.support_tables_built((int)rows.size());
      }
    }
  }
  return JRR_OK;
}

extern "C" int jrr_engine_support_tiles(const jrr_engine_t* e, int32_t* n_tiles_host) {
  if (!e) return JRR_ERR_ARG;
  const bool on = use_tile_list(e);
  if (n_tiles_host) *n_tiles_host = on ? e->st.nact() : VT;
  return on ? 1 : 0;
}

extern "C" int jrr_engine_support_vertices(const jrr_engine_t* e, int32_t* n_vertices_host) {
  if (!e) return JRR_ERR_ARG;
  const bool on = use_sup_vertices(e);
  if (n_vertices_host) *n_vertices_host = on ? e->st.sup_nsv() : 0;
  return on ? 1 : 0;
}

extern "C" int jrr_j_regressor_grad_support(jrr_engine_t* e, const float* x6d, const float* betas, const float* gt_mm,
                                            float* dJs, float* sqerr, float* joints, void* stream) {
  if (!e || !x6d || !betas || !gt_mm || !dJs) return JRR_ERR_ARG;
  if (!e->st.have_J()) { jrr_set_error("J_regressor not set"); return JRR_ERR_STATE; }
  if (!(e->flags & JRR_FLAG_KEEP_VERTS)) { jrr_set_error("J step requires JRR_FLAG_KEEP_VERTS"); return JRR_ERR_STATE; }
  if (!e->st.support_known()) { jrr_set_error("j_regressor_grad_support: call jrr_j_support_info first (it must report fits = 1)"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  return j_step_local(e, x6d, betas, gt_mm, e->dJraw, sqerr, s, joints, dJs, true);
}

extern "C" int jrr_j_step_apply_support(jrr_engine_t* e, float* J, const float* dJs, float* m, float* v, int32_t* step, float lr,
                                        const float* mask, void* stream) {
  if (!e || !J || !dJs || !m || !v || !step) { jrr_set_error("j_step_apply_support: null"); return JRR_ERR_ARG; }
  if (!e->st.support_known()) { jrr_set_error("j_step_apply_support: call jrr_j_support_info first (KEEP_VERTS engine, fits = 1)"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  // the dense gradient the optimiser sees: zero outside the support (exactly what the dense path holds there), the
  // all-reduced values on it (scattered inside the update kernel).  Adam itself stays dense: entries that left the support
  // keep coasting on their momentum.
  return j_step_apply(e, J, nullptr, m, v, step, lr, mask, s, dJs);
}

// torch.optim.Adam on the raw regressor with the (all-reduced) gradient, then J*mask -> ReLU -> row-normalise into the
// engine's layouts: the second half of the J step in ONE call (step counter incremented on the device).  The forward
// cached by jrr_j_regressor_grad stays valid: it does not depend on the regressor.
extern "C" int jrr_j_step_apply(jrr_engine_t* e, float* J, const float* dJ, float* m, float* v, int32_t* step, float lr,
                                const float* mask, void* stream) {
  if (!e || !J || !dJ || !m || !v || !step) { jrr_set_error("j_step_apply: null"); return JRR_ERR_ARG; }
  if (!e->has_model) { jrr_set_error("engine was created without an SMPL model (discriminators only)"); return JRR_ERR_STATE; }
  return j_step_apply(e, J, dJ, m, v, step, lr, mask, (hipStream_t)stream);
}

int jrr::j_step_apply(jrr_engine* e, float* J, const float* dJ, float* m, float* v, int32_t* step, float lr, const float* mask, hipStream_t s,
                      const float* dJs) {
  if (!e->st.support_known_under(mask) && e->st.have_jsup()) JRR_HIP(hipMemsetAsync(e->jsup.flag + JSUP_KNOWN, 0, sizeof(int32_t), s));   // (another mask: no baseline to hold the new support against)
  if (e->st.have_jsup() && e->st.have_J() && e->st.tab_static()) {
    // Adam, the engine's copy, the row sums, the normalised layouts and the support lists in ONE launch (jreg.hip k_jstep_update)
    JStepUpdate a;
    a.J = J; a.dJ = dJ; a.dJs = dJs; a.m = m; a.v = v; a.step = step; a.lr = lr;
    a.mask = mask; a.Jraw = e->Jraw; a.Jmask = e->Jmask; a.rowsum = e->rowsum; a.Jn = e->Jn; a.Jn_vi = e->Jn_vi; a.Jn_iv = e->Jn_iv;
    a.Jn_q = e->Jn_q; a.p2v = e->m.p2v; a.v2p = e->m.v2p; a.r16 = uses_r16(e->m) ? 1 : 0;
    a.sup = e->jsup; a.sync = e->jsup.flag + 1;
    launch_jstep_update(a, s);
    e->st.regressor_stepped(mask);
    if (e->st.folded()) { int rcf = fold_rebuild(e, s); if (rcf) return rcf; }
    CHECK_LAUNCH();
    return JRR_OK;
  }
  if (!dJ) {      // (no support lists: jrr_j_step_apply_support has refused already; kept for completeness)
    JRR_HIP(hipMemsetAsync(e->dJraw, 0, (size_t)NH * V * sizeof(float), s));
    launch_jsup_scatter(e->jsup, dJs, e->m.p2v, e->dJraw, s);
    dJ = e->dJraw;
  }
  // Adam with step + 1; the counter itself is incremented by the normalisation's first launch (one launch less per J step)
  launch_adam_flat(J, dJ, m, v, (size_t)NH * V, step, lr, 0.9f, 0.999f, 1e-8f, s, 1);
  return set_j_regressor_impl(e, J, mask, (void*)s, step);      // (step != NULL: the rules of a J step, EngineState::regressor_stepped)
}

int jrr::j_step_local(jrr_engine* e, const float* x6d, const float* betas, const float* gt_mm, float* dJ, float* sqerr, hipStream_t s,
                      float* joints, float* dJs, bool support_verts) {
  // v_posed kept: the next inner iteration may reuse this forward.  The vertices (support_verts: the callers whose second half of
  // the step is the engine's own -- the in-call J steps and the support-sized pair): when the regressor's support is known to fit
  // the lists, both consumers (k_jgrad_sparse here, k_rejoints_sparse in the reusing iteration) read support rows only -- the forward
  // stores the tiles that hold one (a few dozen of 216) instead of 340 MB at 4096 poses
  const bool few = support_verts && e->st.support_known();
  const bool listed = use_tile_list(e);             // ... and with JRR_FLAG_SUPPORT_TILES nothing but those tiles is computed (any caller: the engine was created for it)
  smpl_forward(e, x6d, nullptr, betas, true, true, nullptr, s, few ? e->jsup.tmask : nullptr, listed ? e->act_list : nullptr, listed ? e->st.nact() : 0);
  e->st.forward_stored(x6d, betas);
  const float scale = (float)(2.0 * 1.0 / ((double)e->bnorm * 51.0));   // optimize.py:307 unweighted MSE
  launch_joints_loss(e->JP, e->nvc, gt_mm, nullptr, scale, joints ? joints : e->joints, sqerr ? sqerr : e->sqerr, e->dJT, e->B, e->BP, s);
  return j_grad_from_verts(e, dJ, s, dJs);
}
