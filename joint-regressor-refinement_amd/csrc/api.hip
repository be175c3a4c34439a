// The engine behind the C ABI (include/jrr.h): error plumbing, run-time knobs, engine / workspace planning, the regressor upload, the
// SMPL operators, and the small operators whose kernels live in rot.hip, chain.hip, loss.hip and flat.hip.  Every other entry point sits in the file
// of the kernels it launches; the body-model re-layout is model.hip, the fused inner loop and the J step refine.hip (shared: engine.h).
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>

#include "engine.h"
#include "lbs_tile.h"

using namespace jrr;

static thread_local char g_err[512] = "";
void jrr_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* jrr_last_error(void) { return g_err; }
extern "C" int jrr_version(void) { return 106; }      // 100 + round: entry points were added in rounds 2-6, none changed or removed

// =============================================================================================
// run-time knobs (engine.h struct Knobs says what each is for)
// =============================================================================================
Knobs jrr::read_knobs() {
  Knobs k;
  auto str = [](const char* v) { return v ? v : ""; };
  auto in_range = [](const char* v, int lo, int hi) { const int n = v ? atoi(v) : 0; return (n >= lo && n <= hi) ? n : 0; };
  k.vertex_order_sorted = strcmp(str(getenv("JRR_VERTEX_ORDER")), "sorted") == 0;
  k.dense_skinning = str(getenv("JRR_DENSE_SKINNING"))[0] == '1';
  k.skin_joints_12 = atoi(str(getenv("JRR_SKIN_JOINTS"))) == 12;
  k.bwd16 = str(getenv("JRR_BWD16"))[0] != '0';
  k.fwd_chunk_cap = in_range(getenv("JRR_FWD_CHUNK_CAP"), 1, 216);
  k.fwd_round = str(getenv("JRR_FWD_ROUND"))[0] != '0';
  k.nsplit = in_range(getenv("JRR_NSPLIT"), 1, 256);
  k.nvcb16 = in_range(getenv("JRR_NVCB16"), 1, 36);
  { const char* v = getenv("JRR_ADJ_CHUNKS"); k.adj_chunks = v ? std::max(1, atoi(v)) : 6; }
  { const char c = str(getenv("JRR_SUPPORT_FUSED"))[0]; k.support_fused = c == '0' ? 0 : c == '2' ? 2 : 1; }
  { const char* v = getenv("JRR_SUP_OVERLAP"); k.sup_overlap = v ? (v[0] == '1' ? 1 : 0) : -1; }
  return k;
}
const Knobs& jrr::knobs() {
  static const Knobs k = read_knobs();
  return k;
}

// =============================================================================================
// engine
// =============================================================================================

// number of vertex chunks such that the grid fills whole "rounds" of the chip's resident
// workgroup slots (256 CUs x 2 workgroups): a grid of 1.1 rounds costs 2 rounds of time.
static int pick_chunks(int wg_per_chunk, int max_chunks) {
  const int slots = 512;
  int best = 1;
  double best_score = -1.0;
  for (int n = 1; n <= max_chunks; ++n) {
    const int total = wg_per_chunk * n;
    const int rounds = (total + slots - 1) / slots;
    const double fill = (double)total / ((double)rounds * slots);
    // tiles per chunk differ by at most one: the longest chunk sets the time of its round
    const double tiles = 216.0 / n;
    const double balance = tiles / (double)((216 + n - 1) / n);
    const double score = fill * balance - 0.0002 * n;   // prefer fewer chunks at equal efficiency
    if (score > best_score) { best_score = score; best = n; }
  }
  return best;
}

static void plan_geometry(int BP, int& nvc, int& nvcb, int& nvcb16, int& nsplit, int& nsplitJ) {
  const Knobs kn = read_knobs();
  const int nbg = BP / BG;
  // forward: one workgroup per (128 poses, chunk).  At most 54 chunks (4 tiles each) -- 108 for batches of up to 256 poses (round 6), whose
  // one or two pose groups would otherwise put 54 / 108 workgroups on 512 slots with 4 tiles to walk each (256 poses, the reference's
  // default batch, all five terms: k_lbs_fwd 67 -> 40 us, k_joints_loss 12 -> 17 us for twice the partials, the iteration 0.390 -> 0.367 ms;
  // 216 chunks: 0.378; at 512 poses 108 chunks are two workgroups per CU and gain nothing: tools/exp/fwd_chunk_cap_ab.sh).
  // JRR_FWD_CHUNK_CAP (experiments) overrides the cap.
  int fwd_cap = nbg <= 2 ? 108 : 54;
  if (kn.fwd_chunk_cap) fwd_cap = kn.fwd_chunk_cap;
  nvc = pick_chunks(nbg, fwd_cap);
  // exactly one round of 512 workgroups with an even chunk count lets k_lbs_fwd pair the two workgroups of a CU (lbs_tile.h)
  if (kn.fwd_round && 512 % nbg == 0 && 512 / nbg <= 64 && pairs_one_round(nbg, 512 / nbg)) nvc = 512 / nbg;
  nvcb = pick_chunks(BP / BT, 36);                  // backward, role kernel: one workgroup per (32 poses, chunk)
  nvcb16 = pick_chunks(BP / 64, 36);                // backward, k_lbs_bwd16: one workgroup per (64 poses, chunk)
  // ... but exactly one round of 512 workgroups with an even chunk count lets the kernel pair the two workgroups of a CU on
  // one pose group (lbs_tile.h), which is worth more than the last per cent of tile balance
  if (512 % (BP / 64) == 0 && 512 / (BP / 64) <= 36 && pairs_one_round(BP / 64, 512 / (BP / 64))) nvcb16 = 512 / (BP / 64);
  nsplit = (512 + nbg - 1) / nbg;
  // at most 32 slabs -- 64 for batches of up to 512 poses, whose 32 x (BP / 128) workgroups leave most of the chip idle (256 poses, the
  // reference's default batch: blend adjoint 81 -> 46 us, the iteration 0.383 -> 0.357 ms; at 1024 poses 64 slabs gain the product
  // nothing and cost the slab sum 10 us: DESIGN.md section 8)
  const int cap = nbg <= 4 ? 64 : 32;
  if (nsplit > cap) nsplit = cap;
  if (nsplit < 1) nsplit = 1;
  // (experiment knobs, tools/exp: the split-K slab count of the blend adjoint and the vertex chunks of k_lbs_bwd16)
  if (kn.nsplit) nsplit = kn.nsplit;
  if (kn.nvcb16) nvcb16 = kn.nvcb16;
  nsplitJ = 3;                                      // pose splits per plane of the J-gradient product: 162 x 3 workgroups
  if (BP / 32 < nsplitJ) nsplitJ = BP / 32;         // = 0.95 of one round of the chip's 512 workgroup slots
}

struct Carver {
  char* base; size_t off;
  float* take(size_t nfloats) {
    float* p = base ? (float*)(base + off) : nullptr;
    off += round_up(nfloats * sizeof(float), 256);
    return p;
  }
};

// silhouette image size of an engine: JRR_FLAG_SIL_SIZE(size) if given, else 256 with JRR_FLAG_SIL_256, else 224
static int sil_size_of(int flags) {
  const int k = (flags & JRR_FLAG_SIL_SIZE_MASK) >> 16;
  return k ? 32 * k : (flags & JRR_FLAG_SIL_256) ? 256 : 224;
}

static size_t carve(jrr_engine* e, void* ws, int B, int flags) {
  const int BP = (int)round_up((size_t)B, BG);
  int nvc, nvcb, nvcb16, nsplit, nsplitJ;
  plan_geometry(BP, nvc, nvcb, nvcb16, nsplit, nsplitJ);
  Carver c{(char*)ws, 0};
  jrr_engine tmp;
  jrr_engine* t = e ? e : &tmp;
  t->rowsum = c.take(32);
  t->probe = (long long*)c.take(16);   // 3 x int64 used
  if (!(flags & JRR_FLAG_NO_MODEL)) {  // SMPL sections (~230 KB per pose): not carved for a discriminator-only engine
    t->Jraw = c.take((size_t)NH * V);
    t->Jmask = c.take((size_t)NH * V);
    t->Jn = c.take((size_t)NH * V);
    t->Jn_vi = c.take((size_t)VT * 1024);
    t->Jn_iv = c.take((size_t)VT * 2560);   // backward per-tile operand records [Jn | W^T | W | pad]
    t->Jn_q = c.take((size_t)VP * 32);      // normalised regressor in vertex quads [VP/4][32][4]
    t->FT = c.take((size_t)KFP * BP);
    t->FTq = c.take((size_t)KFP * BP);      // the features in K-quads: B operand of k_lbs_fwd's blend product
    t->AT = c.take((size_t)12 * NJ * BP);
    t->VPb = c.take((size_t)3 * VP * BP);
    t->JP = c.take((size_t)nvc * 3 * NH * BP);
    t->dJT = c.take((size_t)3 * NHP * BP);
    t->DVP = c.take((size_t)3 * VP * BP);
    t->dATp = c.take((size_t)(nvcb > nvcb16 ? nvcb : nvcb16) * 12 * NJ * BP);     // slabs of either backward kernel
    t->dmask = (unsigned*)c.take((size_t)(nvcb > nvcb16 ? nvcb : nvcb16) * (BP / 64));   // joints present in each slab (k_lbs_bwd16)
    t->dFTp = c.take((size_t)nsplit * KFP * BP);
    t->Jsum = c.take((size_t)3 * NH * BP);
    t->dA = c.take((size_t)12 * NJ * BP);
    t->dF = c.take((size_t)KFP * BP);
    t->R0T = c.take((size_t)16 * BP);
    t->dRT = c.take((size_t)NJ * 9 * BP);
    t->dbT = c.take((size_t)16 * BP);
  }
  t->joints = c.take((size_t)BP * NH * 3);
  t->sqerr = c.take((size_t)BP);
  t->step_scratch = (int32_t*)c.take(64);
  t->gcam = c.take((size_t)BP * 3);
  t->sq2d = c.take((size_t)BP);
  if (flags & JRR_FLAG_POSE_DISC) {
    t->Pd = c.take(DP_TOTAL);
    t->W0T = c.take((size_t)768 * 1024);
    t->W2T = c.take((size_t)1024 * 1024);
    t->W2s = c.take((size_t)1024 * 1024);
    t->W0Tq = c.take((size_t)768 * 1024);
    t->W2Tq = c.take((size_t)1024 * 1024);
    t->W2sq = c.take((size_t)1024 * 1024);
    t->W0q = c.take((size_t)1024 * 768);
    t->zpart = c.take((size_t)16 * BP);
    t->convL = c.take(CONV_IMAGE_FLOATS);
    t->H2T = c.take((size_t)768 * BP);
    t->A1T = c.take((size_t)1024 * BP);
    t->A2T = c.take((size_t)1024 * BP);
    t->dA2T = c.take((size_t)1024 * BP);
    t->dA1T = c.take((size_t)1024 * BP);
    t->dH2T = c.take((size_t)768 * BP);
    t->gx = c.take((size_t)BP * JRR_POSE6D);
    t->TrA = c.take((size_t)BP * 1024);
    t->TrB = c.take((size_t)BP * 1024);
    {   // weight-gradient partial slabs: 8 pose-splits of a 1024x1024 layer, or one conv/head slab per wave
      const size_t conv = (size_t)(BP / 64) * (NJ * 1280 + 792) + (size_t)NJ * 1280, fc = (size_t)8 * 1024 * 1024;
      t->wgs = c.take(conv > fc ? conv : fc);
    }
    t->dz0 = c.take((size_t)BP);
    t->dsc = c.take((size_t)BP * 25);
    t->dsq = c.take((size_t)BP * 25);
  }
  if (flags & JRR_FLAG_SHAPE_DISC) {
    t->Ps = c.take(256);
    t->gb = c.take((size_t)BP * NB);
    t->ssq = c.take((size_t)BP);
  }
  if (flags & (JRR_FLAG_SILHOUETTE | JRR_FLAG_KEEP_VERTS)) t->VTb = c.take((size_t)3 * VP * BP);
  if (flags & JRR_FLAG_SILHOUETTE) {
    t->ndc = c.take((size_t)BP * V * 4);
    const size_t S = (size_t)sil_size_of(flags);
    t->cover = (unsigned*)c.take((size_t)BP * S * S);
    t->ncover = (int*)c.take((size_t)BP);
    t->sqsil = c.take((size_t)BP);
    t->smask = c.take((size_t)BP);
    t->VPM = c.take((size_t)BP * 3 * VP);      // the vertices of a silhouette iteration, pose-major (k_lbs_fwd -> fused rasteriser)
  }
  if (flags & JRR_FLAG_FOLDED) {
    t->JW = c.take((size_t)VP * FOLD_MJ);
    t->Hm = c.take((size_t)FOLD_M * KFP);
    t->Hk = c.take((size_t)KFP * FOLD_M);
    t->G0 = c.take(FOLD_MJ);
    t->MT = c.take((size_t)FOLD_M * BP);
    t->dMT = c.take((size_t)FOLD_M * BP);
  }
  if ((flags & JRR_FLAG_BLEND_BF16X3) && !(flags & JRR_FLAG_NO_MODEL)) t->Dsplit = c.take(blend_basis_split_bytes() / sizeof(float));
  if (flags & JRR_FLAG_KEEP_VERTS) {
    t->dVTb = c.take((size_t)3 * VP * BP);
    t->dJnp = c.take((size_t)3 * nsplitJ * 32 * VP);
    t->dJn = c.take((size_t)NH * VP);
    t->dJraw = c.take((size_t)NH * V);
    t->jsup.flag = (int*)c.take(64);
    t->jsup.cnt = (int*)c.take(64);
    t->jsup.col = (int*)c.take((size_t)NH * JSUP_CAP);
    t->jsup.val = c.take((size_t)NH * JSUP_CAP);
    t->jsup.tmask = (int*)c.take(256);
    t->jsup.tknown = (int*)c.take(256);
    t->act_list = (int*)c.take(256);
    if (flags & JRR_FLAG_SUPPORT_TILES) { float* sb = c.take(sup_tables_floats()); if (sb) sup_tables_carve(t->sup, sb); }
  }
  if (e) {
    e->BP = BP; e->nvc = nvc; e->nvcb = (e->has_model && uses_r16(e->m)) ? nvcb16 : nvcb; e->nsplit = nsplit; e->nsplitJ = nsplitJ;
  }
  return c.off;
}

extern "C" size_t jrr_engine_workspace_bytes(int batch, int flags) {
  if (batch <= 0) return 0;
  return carve(nullptr, nullptr, batch, flags);
}

extern "C" int jrr_engine_create(const jrr_model_t* model, int batch, int batch_norm, void* ws, size_t ws_bytes,
                                 int flags, jrr_engine_t** out) {
  if (!ws || !out || batch <= 0) { jrr_set_error("jrr_engine_create: bad argument"); return JRR_ERR_ARG; }
  if ((flags & (JRR_FLAG_SIL_256 | JRR_FLAG_SIL_SIZE_MASK)) && !(flags & JRR_FLAG_SILHOUETTE)) { jrr_set_error("jrr_engine_create: a silhouette size without JRR_FLAG_SILHOUETTE"); return JRR_ERR_ARG; }
  if ((flags & JRR_FLAG_SIL_SIZE_MASK) && ((flags & JRR_FLAG_SIL_256) || ((flags & JRR_FLAG_SIL_SIZE_MASK) >> 16) > 8)) {
    jrr_set_error("jrr_engine_create: JRR_FLAG_SIL_SIZE takes a multiple of 32 up to 256 (and excludes JRR_FLAG_SIL_256)");
    return JRR_ERR_ARG;
  }
  if (!model && (flags & ~(JRR_FLAG_POSE_DISC | JRR_FLAG_SHAPE_DISC | JRR_FLAG_NO_MODEL))) {
    jrr_set_error("jrr_engine_create: a model-less engine serves the discriminators only");
    return JRR_ERR_ARG;
  }
  if (model && (flags & JRR_FLAG_NO_MODEL)) { jrr_set_error("jrr_engine_create: JRR_FLAG_NO_MODEL with a model"); return JRR_ERR_ARG; }
  if ((flags & JRR_FLAG_SUPPORT_TILES) && !(flags & JRR_FLAG_KEEP_VERTS)) { jrr_set_error("jrr_engine_create: JRR_FLAG_SUPPORT_TILES needs JRR_FLAG_KEEP_VERTS (the support lists live there)"); return JRR_ERR_ARG; }
  if (((uintptr_t)ws & 255) != 0) { jrr_set_error("workspace must be 256-byte aligned"); return JRR_ERR_ARG; }
  const size_t need = jrr_engine_workspace_bytes(batch, flags);
  if (ws_bytes < need) { jrr_set_error("workspace too small: %zu < %zu", ws_bytes, need); return JRR_ERR_WORKSPACE; }
  jrr_engine* e = new jrr_engine();
  memset((void*)e, 0, sizeof(*e));
  if (model) e->m = model->d;
  e->has_model = model != nullptr;
  e->B = batch;
  e->bnorm = batch_norm > 0 ? batch_norm : batch;
  e->flags = flags;
  e->sil = sil_size_of(flags);
  carve(e, ws, batch, flags);
  e->st.engine_created((flags & JRR_FLAG_KEEP_VERTS) != 0);
  if (flags & JRR_FLAG_BLEND_BF16X3) {      // side mode: the basis is split once, here
    launch_split_blend_basis(e->m.Dq, e->Dsplit, nullptr);
    const hipError_t he = hipStreamSynchronize(nullptr);
    if (he != hipSuccess) { jrr_set_error("jrr_engine_create: splitting the blend basis failed: %s", hipGetErrorString(he)); delete e; return JRR_ERR_HIP; }
  }
  *out = e;
  return JRR_OK;
}

static void clear_events(jrr_engine* e) {
  for (int c = 0; c < JRR_PROF_CLASSES; ++c) {
    if (!e->ev[c]) continue;
    for (hipEvent_t ev : *e->ev[c]) (void)hipEventDestroy(ev);
    e->ev[c]->clear();
  }
}

extern "C" void jrr_engine_destroy(jrr_engine_t* e) {
  if (!e) return;
  clear_events(e);
  for (int c = 0; c < JRR_PROF_CLASSES; ++c) delete e->ev[c];
  if (e->side) { (void)hipStreamSynchronize(e->side); (void)hipStreamDestroy(e->side); }
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->ev_join) (void)hipEventDestroy(e->ev_join);
  delete e;
}

extern "C" int jrr_engine_set_profiling(jrr_engine_t* e, int enabled) {
  if (!e) return JRR_ERR_ARG;
  e->profiling = enabled != 0;
  for (int c = 0; c < JRR_PROF_CLASSES; ++c)
    if (!e->ev[c]) e->ev[c] = new std::vector<hipEvent_t>();
  if (!e->profiling) clear_events(e);
  return JRR_OK;
}

extern "C" int jrr_engine_probe_read(jrr_engine_t* e, int64_t* out_host) {
  if (!e || !out_host) return JRR_ERR_ARG;
  long long v[3] = {0, 0, 0};
  JRR_HIP(hipMemcpy(v, e->probe, sizeof(v), hipMemcpyDeviceToHost));
  out_host[0] = v[0]; out_host[1] = v[1];
  out_host[2] = 2;          // waves resident per SIMD (2 workgroups of 4 waves per CU: launch bounds + 70 KB LDS)
  out_host[3] = 16 * 4;     // issue clocks per v_mfma_f32_32x32x2_f32 (16 passes of 4 clocks)
  out_host[4] = v[2] * 10;  // the interval of out[0] in ns (s_memrealtime, 100 MHz)
  return JRR_OK;
}

extern "C" int jrr_engine_profile_read(jrr_engine_t* e, float* ms_host, int32_t* counts_host) {
  if (!e || !ms_host) return JRR_ERR_ARG;
  for (int c = 0; c < JRR_PROF_CLASSES; ++c) {
    double tot = 0;
    int n = 0;
    if (e->ev[c]) {
      for (size_t i = 0; i + 1 < e->ev[c]->size(); i += 2) {
        float ms = 0.f;
        JRR_HIP(hipEventSynchronize((*e->ev[c])[i + 1]));
        JRR_HIP(hipEventElapsedTime(&ms, (*e->ev[c])[i], (*e->ev[c])[i + 1]));
        tot += ms;
        ++n;
      }
    }
    ms_host[c] = n ? (float)(tot / n) : 0.f;
    if (counts_host) counts_host[c] = n;
  }
  clear_events(e);
  return JRR_OK;
}


extern "C" int jrr_engine_set_batch_norm(jrr_engine_t* e, int bn) {
  if (!e || bn <= 0) return JRR_ERR_ARG;
  e->bnorm = bn;
  return JRR_OK;
}

extern "C" int jrr_engine_info(const jrr_engine_t* e, int32_t* out, int n) {
  if (!e || !out) return JRR_ERR_ARG;
  int32_t v[9] = {e->B, e->BP, e->bnorm, e->nvc, e->nvcb, e->nsplit, e->nsplitJ, e->flags, e->has_model ? e->m.kjs : 0};
  for (int i = 0; i < n && i < 9; ++i) out[i] = v[i];
  return JRR_OK;
}

// loss history of the fused inner loop (refine.hip record_history)
extern "C" int jrr_engine_set_loss_history(jrr_engine_t* e, float* hist_dev, int capacity_records, int every) {
  if (!e || (hist_dev && (capacity_records <= 0 || every <= 0))) return JRR_ERR_ARG;
  e->hist = hist_dev; e->hist_cap = hist_dev ? capacity_records : 0; e->hist_every = every; e->hist_n = 0; e->hist_iter = 0;
  return JRR_OK;
}
extern "C" int jrr_engine_loss_history_count(const jrr_engine_t* e) { return e ? e->hist_n : JRR_ERR_ARG; }

// H[(i,j,c)][k] = sum_v Jn[i,v] W[v,j] D_c[k,v]  and  G0 (fold.hip); both layouts of H
int jrr::fold_rebuild(jrr_engine* e, hipStream_t s) {
  launch_fold_jw(e->Jn, e->m.Wjv, e->JW, e->G0, e->m.p2v, s);
  for (int c = 0; c < 3; ++c) {
    GemmArgs g;
    g.A = e->JW; g.lda = FOLD_MJ;                          // A[k = v][m = (i,j)]
    g.Bm = e->m.Dn + (size_t)c * VP * KFP; g.ldb = KFP;    // Bm[k = v][n = feature]
    g.Out = e->Hm + (size_t)c * KFP; g.ldo = 3 * KFP;      // row (i,j) of plane c = row (i*24+j)*3 + c of Hm
    g.bias = nullptr; g.mask = nullptr; g.split_stride = 0;
    g.M = NH * NJ; g.N = KFP; g.K = VP;
    int rc = launch_gemm_128x32(g, EPI_STORE, 1, s);
    if (rc) return rc;
  }
  launch_transpose(e->Hm, e->Hk, NH * NJ * 3, KFP, s, KFP, FOLD_M);
  e->st.fold_rebuilt();
  return 0;
}

extern "C" int jrr_engine_set_folded(jrr_engine_t* e, int enabled, void* stream) {
  if (!e) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  if (enabled && !(e->flags & JRR_FLAG_FOLDED)) { jrr_set_error("engine created without JRR_FLAG_FOLDED"); return JRR_ERR_STATE; }
  e->st.folded_set(enabled != 0);
  if (e->st.folded() && e->st.have_J() && !e->st.fold_valid()) {
    int rc = fold_rebuild(e, (hipStream_t)stream);
    if (rc) return rc;
    CHECK_LAUNCH();
  }
  return JRR_OK;
}

extern "C" int jrr_engine_set_j_regressor(jrr_engine_t* e, const float* J, const float* mask, void* stream) {
  return set_j_regressor_impl(e, J, mask, stream, nullptr);
}
int jrr::set_j_regressor_impl(jrr_engine* e, const float* J, const float* mask, void* stream, int32_t* step_inc) {
  if (!e || !J) { jrr_set_error("set_j_regressor: null"); return JRR_ERR_ARG; }
  if (!e->has_model) { jrr_set_error("engine was created without an SMPL model (discriminators only)"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  e->st.regressor_uploaded(mask, step_inc != nullptr);
  if (e->st.have_jsup() && !step_inc) JRR_HIP(hipMemsetAsync(e->jsup.flag + JSUP_KNOWN, 0, sizeof(int32_t), s));   // (a J step keeps the baseline: step_inc != NULL)
  JRR_HIP(hipMemcpyAsync(e->Jraw, J, (size_t)NH * V * 4, hipMemcpyDeviceToDevice, s));
  if (mask) JRR_HIP(hipMemcpyAsync(e->Jmask, mask, (size_t)NH * V * 4, hipMemcpyDeviceToDevice, s));
  if (!e->st.tab_static()) {                                                                     // model-only: once per engine
    launch_bwd_tab_static(e->m, e->Jn_iv, s); e->st.static_tables_written();
    // the support-restricted J step writes dJn on the support only: everything else must be finite (it meets Jn = 0)
    if (e->st.have_jsup()) JRR_HIP(hipMemsetAsync(e->dJn, 0, (size_t)NH * VP * sizeof(float), s));
  }
  launch_jreg_normalize(e->Jraw, e->st.have_mask() ? e->Jmask : nullptr, e->rowsum, e->Jn, e->Jn_vi, e->Jn_iv, e->Jn_q, e->m.p2v, s,
                        uses_r16(e->m) ? 1 : 0, e->m.v2p, e->st.have_jsup() ? &e->jsup : nullptr, step_inc);
  if (e->st.folded()) {
    int rc = fold_rebuild(e, s);
    if (rc) return rc;
  }
  CHECK_LAUNCH();
  e->st.regressor_ready();
  return JRR_OK;
}

// =============================================================================================
// operator-level entry points
// =============================================================================================
extern "C" int jrr_rot6d_forward(const float* x, float* R, int n, void* stream) {
  if (!x || !R || n < 0) return JRR_ERR_ARG;
  if (n == 0) return JRR_OK;
  launch_rot6d_fwd(x, R, n, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_rot6d_backward(const float* x, const float* dR, float* dx, int n, void* stream) {
  if (!x || !dR || !dx || n < 0) return JRR_ERR_ARG;
  if (n == 0) return JRR_OK;
  launch_rot6d_bwd(x, dR, dx, n, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

/* smplx batch_rodrigues (pose2rot=True branch of the SMPL operator) */
extern "C" int jrr_rodrigues_forward(const float* aa, float* R, int n, void* stream) {
  if (!aa || !R || n < 0) return JRR_ERR_ARG;
  if (n == 0) return JRR_OK;
  launch_rodrigues_fwd(aa, R, n, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_rodrigues_backward(const float* aa, const float* dR, float* daa, int n, void* stream) {
  if (!aa || !dR || !daa || n < 0) return JRR_ERR_ARG;
  if (n == 0) return JRR_OK;
  launch_rodrigues_bwd(aa, dR, daa, n, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

// The per-vertex-chunk joint partials JP [nvc][3][17][BP] and skinning-adjoint partials dATp [nvcb][12][24][BP] are summed
// by their consumers (k_joints_loss, k_chain_bwd: a few pose-contiguous loads per thread); the 16 split-K slabs of
// dF^T (58 MB at 4096 poses) keep a wide reduction kernel of their own -- and so do the dA slabs when there are many of
// them (small batches: 16 slabs at 1024 poses, where k_chain_bwd has only 32 blocks to sum them with).
constexpr int MAX_SLABS_IN_CONSUMER = 8;
void jrr::reduce_adjoint_partials(jrr_engine* e, hipStream_t s, const float* conv_x6d, float dscale, int nsplit) {
  if (nsplit <= 0) nsplit = e->nsplit;      // (the support-tile iterations split the blend adjoint's short K range fewer ways)
  if (conv_x6d)
    launch_dconv_bwd_reduce(e->convL, conv_x6d, e->dH2T, nullptr, dscale, 1.f, e->gx, e->dsq, e->B, e->BP, e->dFTp, nsplit,
                            (size_t)KFP * e->BP, e->dF, (size_t)KFP * e->BP, s);
  else if (e->nvcb > MAX_SLABS_IN_CONSUMER) {      // both slab sums in one launch
    launch_reduce_slabs2(e->dFTp, nsplit, (size_t)KFP * e->BP, e->dF, (size_t)KFP * e->BP, e->dATp, e->nvcb, (size_t)12 * NJ * e->BP, e->dA,
                         (size_t)12 * NJ * e->BP, s);
    return;
  } else launch_reduce_slabs(e->dFTp, nsplit, (size_t)KFP * e->BP, e->dF, (size_t)KFP * e->BP, s);
  if (e->nvcb > MAX_SLABS_IN_CONSUMER)
    launch_reduce_slabs(e->dATp, e->nvcb, (size_t)12 * NJ * e->BP, e->dA, (size_t)12 * NJ * e->BP, s);
}
// k_lbs_bwd16's slabs carry joint masks instead of zero rows when k_chain_bwd sums them itself (a slab-sum launch reads every row)
unsigned* jrr::slab_masks(jrr_engine* e) {
  return (uses_r16(e->m) && e->nvcb <= MAX_SLABS_IN_CONSUMER) ? e->dmask : nullptr;
}
void jrr::set_adjoint_slabs(jrr_engine* e, PrepBwdLaunch& L) {
  const bool pre = e->nvcb > MAX_SLABS_IN_CONSUMER;
  L.dATp = pre ? e->dA : e->dATp; L.nslabA = pre ? 1 : e->nvcb; L.strideA = (size_t)12 * NJ * e->BP; L.dFTp = e->dF;
  L.dmaskA = slab_masks(e);
}

int jrr::smpl_forward(jrr_engine* e, const float* x6d, const float* R, const float* betas, bool keep_vp, bool keep_verts, int32_t* step_inc,
                      hipStream_t s, const int* vmask, const int* tl, int ntl, bool verts_pm) {
  launch_prep_fwd(e->m, x6d, R, betas, e->FT, e->FTq, e->AT, e->R0T, e->B, e->BP, step_inc, s);
  launch_lbs_fwd(e->m, e->Jn_vi, e->FTq, e->AT, keep_vp ? e->VPb : nullptr, e->JP, verts_pm ? e->VPM : keep_verts ? e->VTb : nullptr, e->B, e->BP,
                 e->nvc, s, nullptr, tl ? nullptr : vmask, tl, ntl, verts_pm ? 1 : 0);
  if (keep_verts && !verts_pm) e->st.verts_stored(vmask != nullptr || tl != nullptr);
  return 0;
}

extern "C" int jrr_find_joints_forward(jrr_engine_t* e, const float* x6d, const float* R, const float* betas,
                                       float* joints, float* verts, void* stream) {
  if (!e || !betas || !joints || ((x6d == nullptr) == (R == nullptr))) { jrr_set_error("find_joints_forward: bad argument"); return JRR_ERR_ARG; }
  if (!e->st.have_J()) { jrr_set_error("J_regressor not set"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  e->st.workspace_overwritten();
  const bool kv = (e->flags & JRR_FLAG_KEEP_VERTS) != 0;
  if (verts && !e->VTb) { jrr_set_error("return_verts needs an engine created with JRR_FLAG_KEEP_VERTS"); return JRR_ERR_STATE; }
  smpl_forward(e, x6d, R, betas, true, kv || verts, nullptr, s);
  if (verts) launch_verts_untranspose(e->VTb, verts, V * 3, V, nullptr, nullptr, e->B, e->BP, s, e->m.p2v);
  launch_joints_loss(e->JP, e->nvc, nullptr, nullptr, 0.f, joints, nullptr, nullptr, e->B, e->BP, s);
  CHECK_LAUNCH();
  return JRR_OK;
}

int jrr::blend_adjoint_gemm(jrr_engine* e, hipStream_t s, const int* tl, int ntl, int nsplit) {
  if ((e->flags & JRR_FLAG_BLEND_BF16X3) && !tl)      // side mode (include/jrr.h): split-bf16 operands, fp32 accumulation
    return launch_blend_adjoint_bf16x3(e->Dsplit, e->DVP, e->dFTp, (size_t)KFP * e->BP, e->BP, nsplit > 0 ? nsplit : e->nsplit, s);
  return launch_blend_adjoint(e->m.Dq, e->DVP, e->dFTp, (size_t)KFP * e->BP, e->BP, nsplit > 0 ? nsplit : e->nsplit, s, tl, ntl);
}

extern "C" int jrr_find_joints_backward(jrr_engine_t* e, const float* x6d, const float* R, const float* betas,
                                        const float* djoints, float* dx6d, float* dR, float* dbetas, float* dJ,
                                        void* stream) {
  if (!e || !betas || !djoints || ((x6d == nullptr) == (R == nullptr))) { jrr_set_error("find_joints_backward: bad argument"); return JRR_ERR_ARG; }
  if (!e->st.have_J()) { jrr_set_error("J_regressor not set"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  e->st.workspace_overwritten();
  launch_joints_loss(nullptr, 0, nullptr, djoints, 0.f, nullptr, nullptr, e->dJT, e->B, e->BP, s);   // (B,17,3) -> [3][18][BP]
  if (dx6d || dR || dbetas) {
    launch_lbs_bwd(e->m, e->Jn_iv, e->AT, e->VPb, e->dJT, nullptr, e->DVP, e->dATp, e->BP, e->nvcb, s, nullptr, 0, slab_masks(e));
    int rc = blend_adjoint_gemm(e, s);
    if (rc) return rc;
    reduce_adjoint_partials(e, s);
    PrepBwdLaunch L;
    L.x6d_in = x6d; L.R_in = R; L.betas_in = betas;
    set_adjoint_slabs(e, L); L.FT = e->FT; L.R0T = e->R0T; L.AT = e->AT; L.dRT = e->dRT; L.dbT = e->dbT;
    L.dx6d = dx6d; L.dR = dR; L.dbetas = dbetas;
    L.B = e->B; L.BP = e->BP;
    launch_prep_bwd(L, e->m, s);
    CHECK_LAUNCH();
  }
  if (dJ) {
    int rc = j_grad_from_verts(e, dJ, s);
    if (rc) return rc;
  }
  return JRR_OK;
}

extern "C" int jrr_smpl_vertices_backward(jrr_engine_t* e, const float* x6d, const float* R, const float* betas,
                                          const float* dverts, float* dx6d, float* dR, float* dbetas, void* stream) {
  if (!e || !betas || !dverts || ((x6d == nullptr) == (R == nullptr))) { jrr_set_error("smpl_vertices_backward: bad argument"); return JRR_ERR_ARG; }
  if (!(e->flags & JRR_FLAG_KEEP_VERTS)) { jrr_set_error("smpl_vertices_backward requires JRR_FLAG_KEEP_VERTS"); return JRR_ERR_STATE; }
  if (!e->st.have_J()) { jrr_set_error("J_regressor not set"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  e->st.workspace_overwritten();
  // the caller's adjoint, transposed into its own [3][VP][BP] buffer (the stored vertices stay valid for a later dJ)
  launch_dverts_transpose(dverts, V * 3, e->dVTb, e->B, e->BP, s, e->m.p2v);
  launch_lbs_bwd(e->m, e->Jn_iv, e->AT, e->VPb, nullptr, e->dVTb, e->DVP, e->dATp, e->BP, e->nvcb, s, nullptr, 0, slab_masks(e));
  int rc = blend_adjoint_gemm(e, s);
  if (rc) return rc;
  reduce_adjoint_partials(e, s);
  PrepBwdLaunch L;
  L.x6d_in = x6d; L.R_in = R; L.betas_in = betas;
  set_adjoint_slabs(e, L); L.FT = e->FT; L.R0T = e->R0T; L.AT = e->AT; L.dRT = e->dRT; L.dbT = e->dbT;
  L.dx6d = dx6d; L.dR = dR; L.dbetas = dbetas;
  L.B = e->B; L.BP = e->BP;
  launch_prep_bwd(L, e->m, s);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_smpl_posed_joints(jrr_engine_t* e, const float* betas, float* joints24, void* stream) {
  if (!e || !betas || !joints24) { jrr_set_error("smpl_posed_joints: null"); return JRR_ERR_ARG; }
  if (e->flags & JRR_FLAG_NO_MODEL) { jrr_set_error("smpl_posed_joints: engine created without a body model"); return JRR_ERR_STATE; }
  // (reads AT and writes the caller's buffer only: a J step's stored forward stays)
  launch_posed_joints(e->m, e->AT, betas, joints24, e->B, e->BP, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

// adjoint of jrr_smpl_posed_joints through the kinematic chain (the chain forward's F^T / A^T of the most recent forward are reused)
extern "C" int jrr_smpl_posed_joints_backward(jrr_engine_t* e, const float* x6d, const float* R, const float* betas, const float* djoints24,
                                              float* dx6d, float* dR, float* dbetas, void* stream) {
  if (!e || !betas || !djoints24 || ((x6d == nullptr) == (R == nullptr))) { jrr_set_error("smpl_posed_joints_backward: bad argument"); return JRR_ERR_ARG; }
  if (e->flags & JRR_FLAG_NO_MODEL) { jrr_set_error("smpl_posed_joints_backward: engine created without a body model"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  e->st.workspace_overwritten();
  launch_posed_joints_bwd(e->m, e->AT, betas, djoints24, e->dA, e->dbT, e->B, e->BP, s);
  JRR_HIP(hipMemsetAsync(e->dF, 0, (size_t)KFP * e->BP * sizeof(float), s));      // the posed joints do not read the blend features
  PrepBwdLaunch L;
  L.x6d_in = x6d; L.R_in = R; L.betas_in = betas;
  L.dATp = e->dA; L.nslabA = 1; L.strideA = (size_t)12 * NJ * e->BP; L.dFTp = e->dF; L.dmaskA = nullptr;
  L.FT = e->FT; L.R0T = e->R0T; L.AT = e->AT; L.dRT = e->dRT; L.dbT = e->dbT;
  L.gb_extra = e->dbT;                                                             // (B,10): the direct term through J_j(beta)
  L.dx6d = dx6d; L.dR = dR; L.dbetas = dbetas;
  L.B = e->B; L.BP = e->BP;
  launch_prep_bwd(L, e->m, s);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_joint_loss(const float* joints, const float* gt_mm, float weight, int batch, int batch_norm,
                              float* sqerr, float* djoints, void* stream) {
  if (!joints || !gt_mm || batch <= 0 || batch_norm <= 0) return JRR_ERR_ARG;
  const float scale = (float)(2.0 * (double)weight / ((double)batch_norm * 51.0));
  launch_joint_loss_plain(joints, gt_mm, scale, sqerr, djoints, batch, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_adam_step(float* p, const float* g, float* m, float* v, size_t n, const int32_t* step, float lr,
                             float beta1, float beta2, float eps, void* stream) {
  if (!p || !g || !m || !v || !step) return JRR_ERR_ARG;
  if (n == 0) return JRR_OK;
  launch_adam_flat(p, g, m, v, n, step, lr, beta1, beta2, eps, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

// =============================================================================================
// 2-D reprojection (row f1)
// =============================================================================================
extern "C" int jrr_project_joints(const float* joints, const float* cam, float* j2d, int batch, void* stream) {
  if (!joints || !cam || !j2d || batch <= 0) return JRR_ERR_ARG;
  launch_project_joints(joints, cam, j2d, batch, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_engine_set_reprojection(jrr_engine_t* e, const float* gt_j2d, float* cam, float* cam_m, float* cam_v) {
  if (!e) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  if (gt_j2d && (!cam || !cam_m || !cam_v)) { jrr_set_error("set_reprojection: cam / cam_m / cam_v required"); return JRR_ERR_ARG; }
  e->gt_j2d = gt_j2d; e->cam = cam; e->cam_m = cam_m; e->cam_v = cam_v;
  return JRR_OK;
}

extern "C" int jrr_camera_prefit(jrr_engine_t* e, const float* x6d, const float* betas, const float* gt_j2d, float* cam,
                                 int n_steps, float lr, float* sq2d, void* stream) {
  if (!e || !x6d || !betas || !gt_j2d || !cam || n_steps < 0) return JRR_ERR_ARG;
  if (!e->st.have_J()) { jrr_set_error("J_regressor not set"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  e->st.workspace_overwritten();
  smpl_forward(e, x6d, nullptr, betas, false, false, nullptr, s);
  launch_joints_loss(e->JP, e->nvc, nullptr, nullptr, 0.f, e->joints, nullptr, nullptr, e->B, e->BP, s);
  const float scale2d = (float)(2.0 / ((double)e->bnorm * 34.0));     // optimize.py:193 unweighted MSE
  launch_camera_fit(e->joints, gt_j2d, cam, scale2d, n_steps, lr, sq2d, e->B, s);
  CHECK_LAUNCH();
  return JRR_OK;
}
