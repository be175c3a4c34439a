// Internal (never installed): the engine's state and the host helpers shared by the translation units that work on an engine --
// model.hip (body-model re-layout), api.hip (knobs, engine lifecycle and workspace, regressor upload, SMPL operators), refine.hip (fused
// inner loop, J step), disc.hip (discriminator operators and parameter upload), sil.hip (silhouette operators).  The engine-less feature
// files need jrr_common.h only.
#pragma once
#include <vector>

#include "engine_state.h"
#include "jrr_common.h"
#include "kernels.h"

struct jrr_engine {
  jrr::Model m;
  jrr::EngineState st;                               // what of the stored results may still be used (engine_state.h)
  int B, BP, bnorm, flags;
  int sil;                                           // silhouette image size: 224, or 256 with JRR_FLAG_SIL_256
  int nvc, nvcb, nsplit, nsplitJ;
  bool have_pd, have_sd, has_model;
  // workspace sections
  float *rowsum, *Jraw, *Jmask, *Jn, *Jn_vi, *Jn_iv, *Jn_q;
  float *FT, *FTq, *AT, *VPb, *JP, *dJT, *DVP, *dATp, *dFTp, *joints, *sqerr, *Jsum, *dA, *dF, *R0T, *dRT, *dbT;
  unsigned* dmask;                                   // [slab][BP / 64] joint masks of the dA slabs (k_lbs_bwd16 -> k_chain_bwd)
  float *convL;                                      // LDS image of the per-joint MLP parameters (k_conv_image)
  float *W2s, *zpart;                                // fc2.w rows scaled by fc4.w; partial fc4 dots [16][BP]
  float *W0Tq, *W2Tq, *W2sq, *W0q;                   // the four GEMM weight operands in quads [k/4][m][4]
  float *Pd, *W0T, *W2T, *H2T, *A1T, *A2T, *dA2T, *dA1T, *dH2T, *gx, *TrA, *TrB, *dz0, *dsc, *wgs;
  float *Ps, *gb;
  float *dsq, *ssq;                                  // per-pose squared adversarial errors of the last iteration [25][BP], [BP]
  long long* probe;                                  // shader-clock probe of k_lbs_fwd (profiling)
  float *ndc, *sqsil, *VPM; unsigned* cover; int* ncover;   // soft silhouette (JRR_FLAG_SILHOUETTE)
  const float* sil_mask; float* smask;      // target masks, per-pose sum(mask^2)
  float *JW, *Hm, *Hk, *G0, *MT, *dMT;      // folded regressor (JRR_FLAG_FOLDED)
  float* Dsplit;                            // the blend basis as bf16 hi | lo chunks (JRR_FLAG_BLEND_BF16X3)
  float* dJraw;                                      // (17,6890) gradient scratch of the in-call J steps (jrr_refine_run_j_steps)
  jrr::JSupport jsup;                                // support lists of the normalised regressor (KEEP_VERTS engines; jreg.hip)
  float* hist; int hist_cap, hist_every, hist_n; long long hist_iter;   // loss history (jrr_engine_set_loss_history)
  float *VTb;       // [3][VP][BP] vertices / transposed vertex adjoint (KEEP_VERTS or SILHOUETTE)
  float *dVTb, *dJnp, *dJn;   // transposed external vertex adjoint [3][VP][BP]; J-gradient partial slabs [3*nsplitJ][32][VP]
  int32_t* step_scratch;      // arrival counter of k_sup_step's step-count protocol (chain.hip), its only user
  bool profiling;
  // JRR_FLAG_SUPPORT_TILES: the 32-vertex tiles that hold an entry of the regressor's support (ascending), taken when
  // jrr_j_support_info reports that the support fits; J steps only shrink the support, so the list stays a superset
  int* act_list;
  // ... and, when the support has at most SUP_NSV vertices, the joint-loss iteration runs per VERTEX in one workgroup per 32-pose group
  // (supk.h): the gathered basis rows and skinning lists of the support, built with the tile list
  jrr::SupTables sup;
  // JRR_SUP_OVERLAP: a second stream for the half of the support-vertex iteration that does not read the discriminator GEMMs' results,
  // and the two events that fork / join it (all three or none: refine.hip ensure_side_stream, created on first use)
  hipStream_t side; hipEvent_t ev_fork, ev_join;
  std::vector<hipEvent_t>* ev[JRR_PROF_CLASSES];
  const float* gt_j2d; float* cam; float* cam_m; float* cam_v;   // 2-D reprojection term (nullable)
  float *gcam, *sq2d;
};

// RAII-less bracket helper: records an event on the stream if profiling is on
static inline void prof_mark(jrr_engine* e, int cls, hipStream_t s) {
  if (!e->profiling) return;
  hipEvent_t ev;
  if (hipEventCreate(&ev) != hipSuccess) return;
  (void)hipEventRecord(ev, s);
  e->ev[cls]->push_back(ev);
}

// the model runs k_lbs_bwd16: the regressor's part of the backward operand records is written in its R16 layout
static inline bool uses_r16(const jrr::Model& m) { return m.kjs && m.bwd16; }
// EngineState's two iteration choices with what they need from outside the state
static inline bool use_tile_list(const jrr_engine* e) {
  return e->st.use_tile_list((e->flags & JRR_FLAG_SUPPORT_TILES) != 0, e->sil_mask != nullptr, uses_r16(e->m));
}
static inline bool use_sup_vertices(const jrr_engine* e) {
  return e->st.use_sup_vertices((e->flags & JRR_FLAG_SUPPORT_TILES) != 0, e->sil_mask != nullptr, uses_r16(e->m));
}

namespace jrr {

// Every JRR_* variable the library reads (verification and A/B knobs: DESIGN.md section 3), read in one function (api.hip
// read_knobs).  gemm.hip reads JRR_DISC_NARROW itself.
struct Knobs {
  // -- body-model re-layout (model.hip): a fresh snapshot per jrr_model_create*, so that one process can build variant models --
  bool vertex_order_sorted;   // JRR_VERTEX_ORDER=sorted: store the vertices in the joint-sorted order even when the file order fits
  bool dense_skinning;        // JRR_DENSE_SKINNING=1: the dense skinning kernels instead of the joint-sparse ones
  bool skin_joints_12;        // JRR_SKIN_JOINTS=12: the 12-slot joint-sparse kernels where 8 slots would be chosen
  bool bwd16;                 // JRR_BWD16=0 clears it: the role backward kernel instead of k_lbs_bwd16
  // -- launch geometry (api.hip plan_geometry): a fresh snapshot per workspace plan; 0 = not set (or out of range) --
  int fwd_chunk_cap;          // JRR_FWD_CHUNK_CAP (1 .. 216): most vertex chunks of k_lbs_fwd
  bool fwd_round;             // JRR_FWD_ROUND=0 clears it: k_lbs_fwd's grid need not be one round of 512 paired workgroups
  int nsplit;                 // JRR_NSPLIT (1 .. 256): split-K slabs of the blend adjoint
  int nvcb16;                 // JRR_NVCB16 (1 .. 36): vertex chunks of k_lbs_bwd16
  // -- fused inner loop (refine.hip): once per process (knobs()) --
  int adj_chunks;             // JRR_ADJ_CHUNKS (>= 1, default 6): K chunks per split of the tile-listed blend adjoint
  int support_fused;          // JRR_SUPPORT_FUSED: 0 = no support-vertex iteration, 2 = as separate launches, else 1 = composed (k_sup_step)
  int sup_overlap;            // JRR_SUP_OVERLAP: 0 / 1 = the side-stream halves of k_sup_step never / always, -1 (unset) = on up to 512 poses
};
Knobs read_knobs();           // the environment as it is now
const Knobs& knobs();         // the environment as it was at the first call: what the loop uses

// ---- api.hip ----
// step_inc (J step only): the Adam step counter, incremented by the first launch of the normalisation
int set_j_regressor_impl(jrr_engine* e, const float* J, const float* mask, void* stream, int32_t* step_inc);
// conv_x6d != NULL (fused loop with the pose discriminator): the per-joint MLP adjoint shares the launch of the dF^T sum.
void reduce_adjoint_partials(jrr_engine* e, hipStream_t s, const float* conv_x6d = nullptr, float dscale = 0.f, int nsplit = 0);
unsigned* slab_masks(jrr_engine* e);
void set_adjoint_slabs(jrr_engine* e, PrepBwdLaunch& L);
// verts_pm: the vertices go pose-major into e->VPM (what the fused rasteriser reads) instead of the row quads of e->VTb
int smpl_forward(jrr_engine* e, const float* x6d, const float* R, const float* betas, bool keep_vp, bool keep_verts, int32_t* step_inc,
                 hipStream_t s, const int* vmask = nullptr, const int* tl = nullptr, int ntl = 0, bool verts_pm = false);
int blend_adjoint_gemm(jrr_engine* e, hipStream_t s, const int* tl = nullptr, int ntl = 0, int nsplit = 0);
int fold_rebuild(jrr_engine* e, hipStream_t s);

// ---- disc.hip ----
// conv_done: the per-joint MLP already ran (fused into the chain-forward launch, launch_prep_fwd_dconv)
int disc_forward(jrr_engine* e, const float* x6d, float* out, hipStream_t s, bool quad = true, bool conv_done = false);
// skip_conv: the caller runs the per-joint MLP adjoint itself (fused with the dF^T slab sum, launch_dconv_bwd_reduce)
int disc_backward_input(jrr_engine* e, const float* x6d, float* out, const float* gout, float scale, float target, float* gx, hipStream_t s,
                        float* sq = nullptr, bool skip_conv = false);

// ---- refine.hip ----
int joints_from_stored_verts(jrr_engine* e, hipStream_t s, int32_t* step_inc = nullptr);
int j_grad_from_verts(jrr_engine* e, float* dJ, hipStream_t s, float* dJs = nullptr);
int j_step_local(jrr_engine* e, const float* x6d, const float* betas, const float* gt_mm, float* dJ, float* sqerr, hipStream_t s,
                 float* joints = nullptr, float* dJs = nullptr, bool support_verts = false);
int j_step_apply(jrr_engine* e, float* J, const float* dJ, float* m, float* v, int32_t* step, float lr, const float* mask, hipStream_t s,
                 const float* dJs = nullptr);

}  // namespace jrr
