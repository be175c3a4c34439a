// C ABI (include/jrr.h): error plumbing, run-time knobs, engine / workspace planning, and the launch sequences of the operator-level
// entry points.  The body-model re-layout is model.hip, the fused inner loop and the J step refine.hip (shared state: engine.h).
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>

#include "engine.h"

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
  // exactly one round of 512 workgroups with an even chunk count lets k_lbs_fwd pair the two workgroups of a CU (lbs.hip)
  if (kn.fwd_round && 512 % nbg == 0 && 512 / nbg <= 64 && ((512 / nbg) & 1) == 0 && 32 % (512 / nbg / 2) == 0) nvc = 512 / nbg;
  nvcb = pick_chunks(BP / BT, 36);                  // backward, role kernel: one workgroup per (32 poses, chunk)
  nvcb16 = pick_chunks(BP / 64, 36);                // backward, k_lbs_bwd16: one workgroup per (64 poses, chunk)
  // ... but exactly one round of 512 workgroups with an even chunk count lets the kernel pair the two workgroups of a CU on
  // one pose group (lbs.hip), which is worth more than the last per cent of tile balance
  if (512 % (BP / 64) == 0 && 512 / (BP / 64) <= 36 && ((512 / (BP / 64)) & 1) == 0 && 32 % (512 / (BP / 64) / 2) == 0) nvcb16 = 512 / (BP / 64);
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
    e->BP = BP; e->nvc = nvc; e->nvcb = (e->has_model && e->m.kjs && e->m.bwd16) ? nvcb16 : nvcb; e->nsplit = nsplit; e->nsplitJ = nsplitJ;
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
  e->have_jsup = (flags & JRR_FLAG_KEEP_VERTS) != 0;
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
  e->fold_valid = true;
  return 0;
}

extern "C" int jrr_engine_set_folded(jrr_engine_t* e, int enabled, void* stream) {
  if (!e) return JRR_ERR_ARG;
  e->fwd_cached = false;
  if (enabled && !(e->flags & JRR_FLAG_FOLDED)) { jrr_set_error("engine created without JRR_FLAG_FOLDED"); return JRR_ERR_STATE; }
  e->folded = enabled != 0;
  if (e->folded && e->have_J && !e->fold_valid) {
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
  e->jsup_fits_known = false;      // a regressor from outside: its support is not known to fit until jrr_j_support_info says so
  if (e->verts_partial) e->fwd_cached = false;      // the stored vertices cover the OLD regressor's support tiles only
  e->act_valid = false; e->sup_valid = false;
  if (e->have_jsup && !step_inc) JRR_HIP(hipMemsetAsync(e->jsup.flag + JSUP_KNOWN, 0, sizeof(int32_t), s));   // (a J step keeps the baseline: step_inc != NULL)
  JRR_HIP(hipMemcpyAsync(e->Jraw, J, (size_t)NH * V * 4, hipMemcpyDeviceToDevice, s));
  if (mask) JRR_HIP(hipMemcpyAsync(e->Jmask, mask, (size_t)NH * V * 4, hipMemcpyDeviceToDevice, s));
  e->have_mask = mask != nullptr;
  if (mask != e->jsup_mask) e->jsup_fits_known = false;      // a different mask may un-mask entries: the support may have grown
  e->jsup_mask = mask;
  if (!e->tab_static) {                                                                     // model-only: once per engine
    launch_bwd_tab_static(e->m, e->Jn_iv, s); e->tab_static = true;
    // the support-restricted J step writes dJn on the support only: everything else must be finite (it meets Jn = 0)
    if (e->have_jsup) JRR_HIP(hipMemsetAsync(e->dJn, 0, (size_t)NH * VP * sizeof(float), s));
  }
  launch_jreg_normalize(e->Jraw, e->have_mask ? e->Jmask : nullptr, e->rowsum, e->Jn, e->Jn_vi, e->Jn_iv, e->Jn_q, e->m.p2v, s,
                        (e->m.kjs && e->m.bwd16) ? 1 : 0, e->m.v2p, e->have_jsup ? &e->jsup : nullptr, step_inc);
  e->fold_valid = false;
  if (e->folded) {
    int rc = fold_rebuild(e, s);
    if (rc) return rc;
  }
  CHECK_LAUNCH();
  e->have_J = true;
  return JRR_OK;
}

extern "C" int jrr_engine_set_pose_disc(jrr_engine_t* e, const float* P, void* stream) {
  if (!e || !P) return JRR_ERR_ARG;
  e->fwd_cached = false;
  if (!(e->flags & JRR_FLAG_POSE_DISC)) { jrr_set_error("engine created without JRR_FLAG_POSE_DISC"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  JRR_HIP(hipMemcpyAsync(e->Pd, P, (size_t)DP_TOTAL * 4, hipMemcpyDeviceToDevice, s));
  launch_transpose(e->Pd + DP_FC0_W, e->W0T, 1024, 768, s);    // [out][in] -> [in][out]
  launch_transpose(e->Pd + DP_FC2_W, e->W2T, 1024, 1024, s);
  launch_scale_rows(e->Pd + DP_FC2_W, e->Pd + DP_FC4_W, e->W2s, 1024, 1024, s);   // row n of fc2.w times fc4.w[n]
  launch_to_quads(e->W0T, 1024, e->W0Tq, 768, 1024, s);                // A operands A[k][m] of the four loop GEMMs, in quads
  launch_to_quads(e->W2T, 1024, e->W2Tq, 1024, 1024, s);
  launch_to_quads(e->W2s, 1024, e->W2sq, 1024, 1024, s);
  launch_to_quads(e->Pd + DP_FC0_W, 768, e->W0q, 1024, 768, s);
  launch_conv_image(e->Pd, e->convL, s);
  CHECK_LAUNCH();
  e->have_pd = true;
  return JRR_OK;
}

extern "C" int jrr_engine_set_shape_disc(jrr_engine_t* e, const float* P, void* stream) {
  if (!e || !P) return JRR_ERR_ARG;
  e->fwd_cached = false;
  if (!(e->flags & JRR_FLAG_SHAPE_DISC)) { jrr_set_error("engine created without JRR_FLAG_SHAPE_DISC"); return JRR_ERR_STATE; }
  JRR_HIP(hipMemcpyAsync(e->Ps, P, (size_t)JRR_SHAPE_DISC_PARAMS * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  e->have_sd = true;
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

/* find_crop on uint8 frames (scripts/data.py:220-271) and the mask preparation (scripts/data.py:121,130-132) */
extern "C" int jrr_image_crop(const uint8_t* pix, size_t pix_bytes, const int64_t* desc, const float* bboxes, int batch, const float* mean,
                              const float* stdv, int size0, float* out0, int size1, float* out1, int32_t* status, void* stream) {
  if (!pix || !desc || !bboxes || !out0 || !status || batch < 0 || batch > 65535 || (size1 != 0 && !out1) || ((mean == nullptr) != (stdv == nullptr))) {
    jrr_set_error("jrr_image_crop: bad argument");
    return JRR_ERR_ARG;
  }
  auto bad_size = [](int n) { return n < 4 || n > IC_MAX_SIZE || n % 4 != 0; };
  if (bad_size(size0) || (size1 != 0 && bad_size(size1))) {
    jrr_set_error("jrr_image_crop: crop sizes %d, %d: one or two sizes, multiples of 4, at most %d", size0, size1, IC_MAX_SIZE);
    return JRR_ERR_ARG;
  }
  if (((uintptr_t)pix & 15) != 0 || pix_bytes % 16 != 0 || pix_bytes == 0) {
    jrr_set_error("jrr_image_crop: the pixel buffer must be 16-byte aligned and a non-zero multiple of 16 bytes long");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  launch_image_crop(pix, pix_bytes, desc, bboxes, batch, mean, stdv, size0, out0, size1, out1, status, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_mask_prepare(const uint8_t* masks, int batch, int h, int w, float* out, int32_t* valid, void* stream) {
  if (!masks || !out || !valid || batch < 0 || h <= 0 || w <= 0 || (((uintptr_t)masks | (uintptr_t)out) & 15) != 0) {
    jrr_set_error("jrr_mask_prepare: bad argument");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  launch_mask_prepare(masks, batch, h, w, out, valid, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

/* the fit report: viz() of scripts/optimize.py:35-48 around the inner loop (:204-218, :268-274) */
extern "C" int jrr_silhouette_compare(const float* alpha, const float* mask, int batch, int h, int w, float thr_render, float thr_mask,
                                      int32_t* counts, void* stream) {
  if (!alpha || !mask || !counts || batch < 0 || batch > (1 << 24) || h <= 0 || w <= 0 || (long long)h * w > (1LL << 30)) {
    jrr_set_error("jrr_silhouette_compare: bad argument");
    return JRR_ERR_ARG;
  }
  if (((long long)h * w) % 4 != 0 || (((uintptr_t)alpha | (uintptr_t)mask) & 15) != 0 || ((uintptr_t)counts & 3) != 0) {
    jrr_set_error("jrr_silhouette_compare: %d x %d: h * w must be a multiple of 4 and the images 16-byte aligned", h, w);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  JRR_HIP(hipMemsetAsync(counts, 0, (size_t)batch * 4 * sizeof(int32_t), (hipStream_t)stream));
  launch_sil_compare(alpha, mask, batch, h, w, thr_render, thr_mask, counts, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_fit_overlay(const float* alpha, const float* mask, const float* image, const float* mean, const float* stdv,
                               const float* joints2d, int n_sets, int batch, int size, float thr_render, float thr_mask, float radius,
                               uint8_t* rgb, void* stream) {
  if (!alpha || !mask || !rgb || batch < 0 || batch > (1 << 24) || n_sets < 0 || n_sets > 3 || (n_sets > 0 && !joints2d) ||
      ((mean == nullptr) != (stdv == nullptr)) || (mean && !image)) {
    jrr_set_error("jrr_fit_overlay: bad argument");
    return JRR_ERR_ARG;
  }
  if (size < 4 || size > 256 || size % 4 != 0) {
    jrr_set_error("jrr_fit_overlay: size %d: a multiple of 4, at most 256", size);
    return JRR_ERR_ARG;
  }
  if ((((uintptr_t)alpha | (uintptr_t)mask | (uintptr_t)image) & 15) != 0 || ((uintptr_t)rgb & 3) != 0) {
    jrr_set_error("jrr_fit_overlay: alpha, mask and image must be 16-byte aligned, the output 4-byte aligned");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  launch_fit_overlay(alpha, mask, image, mean, stdv, joints2d, n_sets, batch, size, thr_render, thr_mask, radius, rgb, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

/* the fit report's shaded views (--fit_report_mesh): no engine, no body model */
extern "C" int jrr_vertex_normals(const float* verts, const int32_t* faces, const int32_t* adj_offset, const int32_t* adj_face, int batch,
                                  int n_verts, int n_faces, float* normals, void* stream) {
  if (!verts || !faces || !adj_offset || !adj_face || !normals || batch < 0 || n_verts < 1 || n_faces < 1 || n_faces > (1 << 28) ||
      (long long)batch * n_verts > (1LL << 30)) {
    jrr_set_error("jrr_vertex_normals: bad argument");
    return JRR_ERR_ARG;
  }
  if ((((uintptr_t)verts | (uintptr_t)faces | (uintptr_t)adj_offset | (uintptr_t)adj_face | (uintptr_t)normals) & 3) != 0) {
    jrr_set_error("jrr_vertex_normals: every array must be 4-byte aligned");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  launch_vertex_normals(verts, faces, adj_offset, adj_face, normals, batch, n_verts, n_faces, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_mesh_shade(const float* verts, const float* normals, const int32_t* faces, const float* cam, const int32_t* pix_to_face,
                              const float* image, const float* mean, const float* stdv, int batch, int n_verts, int n_faces, int size,
                              const float* colour_host, float opacity, float ambient, const float* light_host, float background,
                              uint8_t* rgb, float* depth, float* normal, int32_t* status, void* stream) {
  if (!verts || !normals || !faces || !cam || !pix_to_face || !colour_host || !light_host || !rgb || batch < 0 || batch > (1 << 24) ||
      n_verts < 1 || n_faces < 1 || n_faces > (1 << 28) || (long long)batch * n_verts > (1LL << 30) ||
      ((mean == nullptr) != (stdv == nullptr)) || (mean && !image)) {
    jrr_set_error("jrr_mesh_shade: bad argument");
    return JRR_ERR_ARG;
  }
  if (size < 4 || size > 256 || size % 4 != 0) {
    jrr_set_error("jrr_mesh_shade: size %d: a multiple of 4, at most 256", size);
    return JRR_ERR_ARG;
  }
  if ((((uintptr_t)pix_to_face | (uintptr_t)image | (uintptr_t)depth | (uintptr_t)normal) & 15) != 0 ||
      (((uintptr_t)verts | (uintptr_t)normals | (uintptr_t)faces | (uintptr_t)cam | (uintptr_t)rgb | (uintptr_t)status) & 3) != 0) {
    jrr_set_error("jrr_mesh_shade: pix_to_face, image, depth and normal must be 16-byte aligned, everything else 4-byte aligned");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  launch_mesh_shade(verts, normals, faces, cam, pix_to_face, image, mean, stdv, batch, n_verts, n_faces, size, colour_host, opacity, ambient,
                    light_host, background, rgb, depth, normal, status, (hipStream_t)stream);
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

/* the log map and the refined-pose table (--save_refined) */
extern "C" int jrr_rotmat_to_axis_angle(const float* R, float* aa, int n, void* stream) {
  if (!R || !aa || n < 0) {
    jrr_set_error("jrr_rotmat_to_axis_angle: bad argument");
    return JRR_ERR_ARG;
  }
  if (n == 0) return JRR_OK;
  launch_rotmat_log(R, aa, n, (hipStream_t)stream);
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
  launch_pose_export(x6d, betas, cam, n_extra > 0 ? extra : nullptr, n_extra, index, table, n_rows, status, batch, (hipStream_t)stream);
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
  return (e->m.kjs && e->m.bwd16 && e->nvcb <= MAX_SLABS_IN_CONSUMER) ? e->dmask : nullptr;
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
  if (keep_verts && !verts_pm) e->verts_partial = vmask != nullptr || tl != nullptr;
  return 0;
}

extern "C" int jrr_find_joints_forward(jrr_engine_t* e, const float* x6d, const float* R, const float* betas,
                                       float* joints, float* verts, void* stream) {
  if (!e || !betas || !joints || ((x6d == nullptr) == (R == nullptr))) { jrr_set_error("find_joints_forward: bad argument"); return JRR_ERR_ARG; }
  if (!e->have_J) { jrr_set_error("J_regressor not set"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  e->fwd_cached = false;
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
  if (!e->have_J) { jrr_set_error("J_regressor not set"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  e->fwd_cached = false;
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
  if (!e->have_J) { jrr_set_error("J_regressor not set"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  e->fwd_cached = false;
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
  e->fwd_cached = false;
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

// ---- pose discriminator --------------------------------------------------------------------
// Six launches per forward + input gradient (scripts/discriminator.py:32-54 and its adjoint):
//   k_dconv_fwd (per-joint MLP, MFMA)  ->  fc0 GEMM (+bias, ReLU)  ->  fc2 GEMM (+bias, ReLU, the fc4 dot product
//   w4 . a2 as per-column partials in the epilogue; what it stores is relu'(a2) as 0 / 1: nothing else of a2 is read again)
//   ->  fc2 adjoint GEMM on that indicator (dz from the partial dots in the prologue multiplies the finished column sums
//   in the epilogue; fc2.w pre-scaled by w4: the rank-one output-layer adjoint is never materialised)  ->  fc0 adjoint
//   GEMM  ->  k_dconv_bwd.
// All four GEMMs: exact 128x64 tiles (512 workgroups at 4096 poses), 3-deep LDS-DMA ring.
// The loop path keeps every activation in quads [row/4][pose][4] (k_disc_gemm); the weight-gradient path of the outer
// step (disc_backward_params) needs row-major activations for its transposes / row sums and runs the row-major kernels.
// conv_done: the per-joint MLP already ran (fused into the chain-forward launch, launch_prep_fwd_dconv)
int jrr::disc_forward(jrr_engine* e, const float* x6d, float* out, hipStream_t s, bool quad, bool conv_done) {
  if (!conv_done) launch_disc_conv_fwd(e->convL, x6d, e->H2T, out, e->B, e->BP, s, quad ? 1 : 0);
  GemmArgs g;
  g.mask = nullptr; g.split_stride = 0; g.N = e->BP; g.ldb = e->BP; g.ldo = e->BP;
  g.A = quad ? e->W0Tq : e->W0T; g.lda = 1024; g.Bm = e->H2T; g.Out = e->A1T; g.bias = e->Pd + DP_FC0_B; g.M = 1024; g.K = 768;
  int rc = quad ? launch_disc_gemm_q(g, EPI_BIAS_RELU, 0, s) : launch_gemm_128x64(g, EPI_BIAS_RELU, 1, s);
  if (rc) return rc;
  g.A = quad ? e->W2Tq : e->W2T; g.lda = 1024; g.Bm = e->A1T; g.Out = e->A2T; g.bias = e->Pd + DP_FC2_B; g.M = 1024; g.K = 1024;
  if (!quad) return launch_gemm_128x64(g, EPI_BIAS_RELU, 1, s);
  g.dotw = e->Pd + DP_FC4_W; g.dot_out = e->zpart;
  return launch_disc_gemm_q(g, EPI_BIAS_RELU_DOT, 0, s);
}

// skip_conv: the caller runs the per-joint MLP adjoint itself (fused with the dF^T slab sum, launch_dconv_bwd_reduce)
int jrr::disc_backward_input(jrr_engine* e, const float* x6d, float* out, const float* gout, float scale, float target, float* gx,
                             hipStream_t s, float* sq, bool skip_conv) {
  GemmArgs g;
  g.bias = nullptr; g.split_stride = 0; g.N = e->BP; g.ldb = e->BP; g.ldo = e->BP;
  // dA1T[k][b] = relu'(A1T) * sum_n (fc4.w[n] fc2.w[n][k]) relu'(A2T[n][b]) dz[b]
  g.A = e->W2sq; g.lda = 1024; g.Bm = e->A2T; g.Out = e->dA1T; g.mask = e->A1T; g.M = 1024; g.K = 1024;
  g.zpart = e->zpart; g.nzpart = 16; g.zbias = e->Pd + DP_FC4_B; g.gout = gout; g.gout_ld = 25; g.scale = scale; g.target = target;
  g.nvalid = e->B; g.sq0 = sq; g.out0 = out; g.out0_ld = 25;
  int rc = launch_disc_gemm_q(g, EPI_MASK, 2, s);
  if (rc) return rc;
  // dH2T[k][b] = sum_n fc0.w[n][k] dA1T[n][b]
  GemmArgs h;
  h.bias = nullptr; h.split_stride = 0; h.N = e->BP; h.ldb = e->BP; h.ldo = e->BP;
  h.A = e->W0q; h.lda = 768; h.Bm = e->dA1T; h.Out = e->dH2T; h.mask = nullptr; h.M = 768; h.K = 1024;
  rc = launch_disc_gemm_q(h, EPI_STORE, 0, s);
  if (rc) return rc;
  if (!skip_conv) launch_disc_conv_bwd(e->convL, x6d, e->dH2T, gout, scale, target, gx, e->B, e->BP, s, sq, 1);
  return 0;
}

extern "C" int jrr_pose_disc_forward(jrr_engine_t* e, const float* x6d, float* out, void* stream) {
  if (!e || !x6d || !out) return JRR_ERR_ARG;
  e->fwd_cached = false;
  if (!e->have_pd) { jrr_set_error("pose discriminator not set"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  int rc = disc_forward(e, x6d, out, s);
  if (rc) return rc;
  launch_disc_z_finish(e->zpart, 16, e->BP, e->Pd + DP_FC4_B, out, e->B, s);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_pose_disc_backward_input(jrr_engine_t* e, const float* x6d, float weight, float target, float* dx,
                                            void* stream) {
  if (!e || !x6d || !dx) return JRR_ERR_ARG;
  e->fwd_cached = false;
  if (!e->have_pd) { jrr_set_error("pose discriminator not set"); return JRR_ERR_STATE; }
  const float scale = (float)(2.0 * (double)weight / ((double)e->bnorm * 25.0));
  int rc = disc_backward_input(e, x6d, nullptr, nullptr, scale, target, dx, (hipStream_t)stream);
  if (rc) return rc;
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_pose_disc_vjp_input(jrr_engine_t* e, const float* x6d, const float* gout, float* dx, void* stream) {
  if (!e || !x6d || !gout || !dx) return JRR_ERR_ARG;
  e->fwd_cached = false;
  if (!e->have_pd) { jrr_set_error("pose discriminator not set"); return JRR_ERR_STATE; }
  int rc = disc_backward_input(e, x6d, nullptr, gout, 0.f, 0.f, dx, (hipStream_t)stream);
  if (rc) return rc;
  CHECK_LAUNCH();
  return JRR_OK;
}

// weight gradients of the pose discriminator: either of the MSE against `target` (gout == NULL; scale = 2/(bnorm*25))
// or the vector-Jacobian product for an arbitrary upstream gradient gout (B,25)
static int disc_backward_params(jrr_engine* e, const float* x6d, const float* gout, float scale, float target, float* dP,
                                float* sqerr, hipStream_t s) {
  int rc = disc_forward(e, x6d, e->dsc, s, false);        // row-major activations for the transposes / row sums below
  if (rc) return rc;
  launch_disc_out(e->Pd, e->A2T, e->dsc, e->dA2T, gout, scale, target, e->B, e->BP, s, e->dz0);
  if (sqerr) launch_sqerr_rows(e->dsc, 25, target, sqerr, e->B, s);
  // fc4: dw[n] += sum_b A2T[n][b] dz0[b] ; db += sum_b dz0[b]
  launch_rowdot_accum(e->A2T, e->BP, e->dz0, dP + DP_FC4_W, 1024, e->BP, s);
  launch_rowdot_accum(e->dz0, e->BP, nullptr, dP + DP_FC4_B, 1, e->BP, s);
  // fc2: dW[n][k] += sum_b dA2T[n][b] A1T[k][b] (pose-major copies feed the K-major GEMM) ; db[n] += sum_b dA2T[n][b]
  launch_transpose(e->dA2T, e->TrA, 1024, e->BP, s);
  launch_transpose(e->A1T, e->TrB, 1024, e->BP, s);
  GemmArgs g;
  g.bias = nullptr; g.mask = nullptr; g.split_stride = 0;
  // the pose dimension is the reduction: split it so that the 64 output tiles become >= 512 workgroups; partial
  // slabs, then a wide accumulate-reduce into the flat gradient (deterministic, no atomics)
  const int wsplit = e->BP >= 4096 ? 8 : e->BP >= 1024 ? 4 : e->BP >= 256 ? 2 : 1;
  g.A = e->TrA; g.lda = 1024; g.Bm = e->TrB; g.ldb = 1024; g.Out = e->wgs; g.ldo = 1024; g.M = 1024; g.N = 1024; g.K = e->BP;
  g.split_stride = (size_t)1024 * 1024;
  rc = launch_gemm_128(g, EPI_STORE, wsplit, s);
  if (rc) return rc;
  launch_reduce_slabs(e->wgs, wsplit, (size_t)1024 * 1024, dP + DP_FC2_W, (size_t)1024 * 1024, s, 1);
  g.split_stride = 0;
  launch_rowdot_accum(e->dA2T, e->BP, nullptr, dP + DP_FC2_B, 1024, e->BP, s);
  // back through fc2
  g.A = e->Pd + DP_FC2_W; g.lda = 1024; g.Bm = e->dA2T; g.ldb = e->BP; g.Out = e->dA1T; g.ldo = e->BP; g.mask = e->A1T;
  g.M = 1024; g.N = e->BP; g.K = 1024;
  rc = launch_gemm_128x64(g, EPI_MASK, 1, s);
  if (rc) return rc;
  // fc0
  launch_transpose(e->dA1T, e->TrA, 1024, e->BP, s);
  launch_transpose(e->H2T, e->TrB, 768, e->BP, s);
  g.mask = nullptr;
  g.A = e->TrA; g.lda = 1024; g.Bm = e->TrB; g.ldb = 768; g.Out = e->wgs; g.ldo = 768; g.M = 1024; g.N = 768; g.K = e->BP;
  g.split_stride = (size_t)1024 * 768;
  rc = launch_gemm_128(g, EPI_STORE, wsplit, s);
  if (rc) return rc;
  launch_reduce_slabs(e->wgs, wsplit, (size_t)1024 * 768, dP + DP_FC0_W, (size_t)1024 * 768, s, 1);
  g.split_stride = 0;
  launch_rowdot_accum(e->dA1T, e->BP, nullptr, dP + DP_FC0_B, 1024, e->BP, s);
  g.A = e->Pd + DP_FC0_W; g.lda = 768; g.Bm = e->dA1T; g.ldb = e->BP; g.Out = e->dH2T; g.ldo = e->BP; g.M = 768; g.N = e->BP; g.K = 1024;
  rc = launch_gemm_128x64(g, EPI_STORE, 1, s);
  if (rc) return rc;
  {   // conv / head weight gradients: one slab per wave [pose group][joint][1280], reduced in two wide steps
      // (over the pose groups, then over the joints) into the flat gradient
    const int ng = e->BP / 64;
    float* slab_shared = e->wgs;
    float* slab_heads = slab_shared + (size_t)NJ * ng * 1280;
    float* tmp = slab_heads + (size_t)ng * 792;
    launch_disc_conv_bwd_params(e->Pd, x6d, e->dH2T, gout, scale, target, slab_shared, slab_heads, e->B, e->BP, s);
    launch_reduce_slabs(slab_shared, ng, (size_t)NJ * 1280, tmp, (size_t)NJ * 1280, s, 0);
    launch_reduce_slabs(tmp, NJ, 1280, dP + DP_CONV0_W, 1280, s, 1);
    launch_reduce_slabs(slab_heads, ng, 792, dP + DP_HEADS, 792, s, 1);
  }
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_pose_disc_backward_params(jrr_engine_t* e, const float* x6d, float target, float* dP, float* sqerr,
                                             void* stream) {
  if (!e || !x6d || !dP) return JRR_ERR_ARG;
  e->fwd_cached = false;
  if (!e->have_pd) { jrr_set_error("pose discriminator not set"); return JRR_ERR_STATE; }
  return disc_backward_params(e, x6d, nullptr, (float)(2.0 / ((double)e->bnorm * 25.0)), target, dP, sqerr, (hipStream_t)stream);
}

extern "C" int jrr_pose_disc_vjp_params(jrr_engine_t* e, const float* x6d, const float* gout, float* dP, void* stream) {
  if (!e || !x6d || !gout || !dP) return JRR_ERR_ARG;
  e->fwd_cached = false;
  if (!e->have_pd) { jrr_set_error("pose discriminator not set"); return JRR_ERR_STATE; }
  return disc_backward_params(e, x6d, gout, 0.f, 0.f, dP, nullptr, (hipStream_t)stream);
}

extern "C" int jrr_shape_disc_vjp_params(jrr_engine_t* e, const float* betas, const float* gout, float* dP, void* stream) {
  if (!e || !betas || !gout || !dP) return JRR_ERR_ARG;
  e->fwd_cached = false;
  if (!e->have_sd) { jrr_set_error("shape discriminator not set"); return JRR_ERR_STATE; }
  launch_shape_disc_bwd_params(e->Ps, betas, gout, 0.f, 0.f, dP, nullptr, e->B, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_shape_disc_backward_params(jrr_engine_t* e, const float* betas, float target, float* dP, float* sqerr,
                                              void* stream) {
  if (!e || !betas || !dP) return JRR_ERR_ARG;
  e->fwd_cached = false;
  if (!e->have_sd) { jrr_set_error("shape discriminator not set"); return JRR_ERR_STATE; }
  const float scale = (float)(2.0 / ((double)e->bnorm * 1.0));
  launch_shape_disc_bwd_params(e->Ps, betas, nullptr, scale, target, dP, sqerr, e->B, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_shape_disc_forward(jrr_engine_t* e, const float* betas, float* out, void* stream) {
  if (!e || !betas || !out) return JRR_ERR_ARG;
  e->fwd_cached = false;
  if (!e->have_sd) { jrr_set_error("shape discriminator not set"); return JRR_ERR_STATE; }
  launch_shape_disc(e->Ps, betas, out, nullptr, 0.f, 0.f, e->B, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_shape_disc_vjp_input(jrr_engine_t* e, const float* betas, const float* gout, float* dbetas, void* stream) {
  if (!e || !betas || !gout || !dbetas) return JRR_ERR_ARG;
  e->fwd_cached = false;
  if (!e->have_sd) { jrr_set_error("shape discriminator not set"); return JRR_ERR_STATE; }
  launch_shape_disc(e->Ps, betas, nullptr, dbetas, 0.f, 0.f, e->B, (hipStream_t)stream, gout);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_refine_aux_losses(jrr_engine_t* e, float* pose_disc_sq, float* shape_disc_sq, void* stream) {
  if (!e) return JRR_ERR_ARG;
  e->fwd_cached = false;
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

extern "C" int jrr_adam_step(float* p, const float* g, float* m, float* v, size_t n, const int32_t* step, float lr,
                             float beta1, float beta2, float eps, void* stream) {
  if (!p || !g || !m || !v || !step) return JRR_ERR_ARG;
  if (n == 0) return JRR_OK;
  launch_adam_flat(p, g, m, v, n, step, lr, beta1, beta2, eps, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_evaluate(const float* pred, const float* target_mm, float* err, float* err_pa, int batch, void* stream) {
  if (!pred || !target_mm || !err || !err_pa || batch <= 0) return JRR_ERR_ARG;
  launch_evaluate(pred, target_mm, err, err_pa, batch, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

/* the evaluation report (--eval_report / --eval_vertices): per-joint errors, joints of foreign meshes, the int64 accumulator */
extern "C" int jrr_evaluate_joints(const float* pred, const float* target_mm, float* err_j, float* err_pa_j, int batch, void* stream) {
  if (!pred || !target_mm || !err_j || !err_pa_j || batch < 0) {
    jrr_set_error("jrr_evaluate_joints: bad argument");
    return JRR_ERR_ARG;
  }
  if ((((uintptr_t)err_j | (uintptr_t)err_pa_j) & 15) != 0) {
    jrr_set_error("jrr_evaluate_joints: err_j and err_pa_j must be 16-byte aligned");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  launch_evaluate_joints(pred, target_mm, err_j, err_pa_j, batch, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" size_t jrr_regress_joints_workspace_bytes(int n_reg) {
  return (n_reg < 1 || n_reg > JRR_REGRESS_MAX_REG) ? 0 : regress_workspace_bytes(n_reg);
}
extern "C" int jrr_regress_joints_prepare(const float* J, int n_reg, const float* mask, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  if (!J || !workspace || n_reg < 1 || n_reg > JRR_REGRESS_MAX_REG || ((uintptr_t)workspace & 15) != 0) {
    jrr_set_error("jrr_regress_joints_prepare: bad argument (1 <= n_reg <= %d, workspace 16-byte aligned)", (int)JRR_REGRESS_MAX_REG);
    return JRR_ERR_ARG;
  }
  if (workspace_bytes < regress_workspace_bytes(n_reg)) {
    jrr_set_error("jrr_regress_joints_prepare: the workspace needs jrr_regress_joints_workspace_bytes(%d) = %zu bytes", n_reg,
                  regress_workspace_bytes(n_reg));
    return JRR_ERR_WORKSPACE;
  }
  launch_regress_prepare(J, mask, n_reg, workspace, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_regress_joints(const float* verts, int batch, const void* workspace, int n_reg, float* joints, void* stream) {
  if (!verts || !workspace || !joints || batch < 0 || n_reg < 1 || n_reg > JRR_REGRESS_MAX_REG || ((uintptr_t)verts & 7) != 0 ||
      ((uintptr_t)workspace & 15) != 0) {
    jrr_set_error("jrr_regress_joints: bad argument (1 <= n_reg <= %d, verts 8-byte aligned)", (int)JRR_REGRESS_MAX_REG);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  if (launch_regress_joints(verts, workspace, n_reg, joints, batch, (hipStream_t)stream) != 0) {
    jrr_set_error("jrr_regress_joints: the device refuses %d bytes of LDS per workgroup", V * 3 * 4);
    return JRR_ERR_HIP;
  }
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_eval_accumulate(const float* err_j, const float* err_pa_j, const int32_t* group, int batch, int n_groups, int64_t* acc,
                                   void* stream) {
  if (!err_j || !err_pa_j || !group || !acc || batch < 0 || ((uintptr_t)acc & 7) != 0) {
    jrr_set_error("jrr_eval_accumulate: bad argument");
    return JRR_ERR_ARG;
  }
  if (n_groups < 1 || n_groups > JRR_EVAL_ACC_MAX_GROUPS) {
    jrr_set_error("jrr_eval_accumulate: n_groups %d: 1 .. %d", n_groups, (int)JRR_EVAL_ACC_MAX_GROUPS);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  launch_eval_accumulate(err_j, err_pa_j, group, n_groups, acc, batch, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_regressor_shift_accumulate(const float* joints_a, const float* joints_b, const int32_t* group, int batch, int n_groups,
                                              int64_t* acc, void* stream) {
  if (!joints_a || !joints_b || !acc || batch < 0 || ((uintptr_t)acc & 7) != 0) {
    jrr_set_error("jrr_regressor_shift_accumulate: bad argument");
    return JRR_ERR_ARG;
  }
  if (n_groups < 1 || n_groups > JRR_EVAL_ACC_MAX_GROUPS) {
    jrr_set_error("jrr_regressor_shift_accumulate: n_groups %d: 1 .. %d", n_groups, (int)JRR_EVAL_ACC_MAX_GROUPS);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  launch_shift_accumulate(joints_a, joints_b, group, n_groups, acc, batch, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_draw_discs(uint8_t* rgb, int batch, int h, int w, const float* points, const float* radius_dev, float radius,
                              const uint8_t* colours_host, int n_sets, int n_pts, void* stream) {
  if (!rgb || !points || !colours_host || batch < 0 || h < 1 || w < 1 || (long long)h * w > (1ll << 28)) {
    jrr_set_error("jrr_draw_discs: bad argument (h, w >= 1, h * w <= 2^28)");
    return JRR_ERR_ARG;
  }
  if (n_sets < 1 || n_sets > JRR_DISCS_MAX_SETS || n_pts < 1 || n_pts > JRR_DISCS_MAX_POINTS) {
    jrr_set_error("jrr_draw_discs: %d sets of %d points: 1 .. %d sets of 1 .. %d points", n_sets, n_pts, (int)JRR_DISCS_MAX_SETS,
                  (int)JRR_DISCS_MAX_POINTS);
    return JRR_ERR_ARG;
  }
  if ((long long)batch * (((long long)h * w + 255) / 256) > 0x7fffffffll) {
    jrr_set_error("jrr_draw_discs: batch %d of %d x %d pictures: more workgroups than one launch takes", batch, h, w);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  launch_draw_discs(rgb, batch, h, w, points, radius_dev, radius, colours_host, n_sets, n_pts, (hipStream_t)stream);
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
  e->fwd_cached = false;
  if (gt_j2d && (!cam || !cam_m || !cam_v)) { jrr_set_error("set_reprojection: cam / cam_m / cam_v required"); return JRR_ERR_ARG; }
  e->gt_j2d = gt_j2d; e->cam = cam; e->cam_m = cam_m; e->cam_v = cam_v;
  return JRR_OK;
}

extern "C" int jrr_camera_prefit(jrr_engine_t* e, const float* x6d, const float* betas, const float* gt_j2d, float* cam,
                                 int n_steps, float lr, float* sq2d, void* stream) {
  if (!e || !x6d || !betas || !gt_j2d || !cam || n_steps < 0) return JRR_ERR_ARG;
  if (!e->have_J) { jrr_set_error("J_regressor not set"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  e->fwd_cached = false;
  smpl_forward(e, x6d, nullptr, betas, false, false, nullptr, s);
  launch_joints_loss(e->JP, e->nvc, nullptr, nullptr, 0.f, e->joints, nullptr, nullptr, e->B, e->BP, s);
  const float scale2d = (float)(2.0 / ((double)e->bnorm * 34.0));     // optimize.py:193 unweighted MSE
  launch_camera_fit(e->joints, gt_j2d, cam, scale2d, n_steps, lr, sq2d, e->B, s);
  CHECK_LAUNCH();
  return JRR_OK;
}

// =============================================================================================
// soft silhouette (row f2)
// =============================================================================================
static int sil_check(jrr_engine* e) {
  if (!(e->flags & JRR_FLAG_SILHOUETTE)) { jrr_set_error("engine created without JRR_FLAG_SILHOUETTE"); return JRR_ERR_STATE; }
  if (!e->m.faces) { jrr_set_error("model has no faces (jrr_model_set_faces)"); return JRR_ERR_STATE; }
  return 0;
}

extern "C" int jrr_silhouette_forward(jrr_engine_t* e, const float* verts, const float* cam, float* alpha, void* stream) {
  if (!e || !verts || !cam || !alpha) return JRR_ERR_ARG;
  int rc = sil_check(e);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  e->fwd_cached = false;
  launch_sil_project(verts, V * 3, cam, e->ndc, e->B, s, e->sil);
  launch_sil_raster(e->ndc, e->m.faces_pk, e->m.nfaces, e->cover, e->ncover, alpha, e->B, s, e->sil);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_silhouette_backward(jrr_engine_t* e, const float* galpha, float* dverts, float* dcam, void* stream) {
  if (!e || !galpha || !dverts || !dcam) return JRR_ERR_ARG;
  int rc = sil_check(e);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  e->fwd_cached = false;
  launch_sil_bwd(e->ndc, e->m.faces, e->cover, e->ncover, nullptr, galpha, 0.f, dverts, V * 3, dcam, 0, e->B, s, e->sil);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_silhouette_pix_to_face(jrr_engine_t* e, int32_t* p2f, void* stream) {
  if (!e || !p2f) return JRR_ERR_ARG;
  int rc = sil_check(e);
  if (rc) return rc;
  launch_sil_pix_to_face(e->cover, e->ncover, p2f, e->B, (hipStream_t)stream, e->sil);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_engine_set_silhouette(jrr_engine_t* e, const float* mask, float* cam, float* cam_m, float* cam_v) {
  if (!e) return JRR_ERR_ARG;
  e->fwd_cached = false;
  if (mask) {
    int rc = sil_check(e);
    if (rc) return rc;
    if (!cam || !cam_m || !cam_v) { jrr_set_error("set_silhouette: cam / cam_m / cam_v required"); return JRR_ERR_ARG; }
    if (e->sil != 224 && e->sil != 256) {
      jrr_set_error("set_silhouette: the silhouette term inside the loop is built for 224 x 224 and 256 x 256 images (this engine: %d); "
                    "the other sizes serve the stand-alone renderer", e->sil);
      return JRR_ERR_STATE;
    }
    e->cam = cam; e->cam_m = cam_m; e->cam_v = cam_v;
  }
  e->sil_mask = mask;
  e->smask_valid = false;          // sum(mask^2) per pose: recomputed on the stream of the next jrr_refine_run
  return JRR_OK;
}

// The silhouette term exactly as the fused inner loop evaluates it (k_sil_raster<true>: in-kernel projection from the
// row-quad vertex buffer, packed fixed-point adjoint, write-back over the vertex pieces), as an operator: SMPL forward of
// (x6d, betas), then loss and gradient w.r.t. the vertices and the camera.
extern "C" int jrr_silhouette_loss_grad(jrr_engine_t* e, const float* x6d, const float* betas, const float* cam,
                                        const float* mask, float* sqsil, float* dverts, float* dcam, void* stream) {
  if (!e || !x6d || !betas || !cam || !mask) { jrr_set_error("silhouette_loss_grad: null"); return JRR_ERR_ARG; }
  int rc = sil_check(e);
  if (rc) return rc;
  if (!e->have_J) { jrr_set_error("J_regressor not set"); return JRR_ERR_STATE; }
  if (!e->VTb) { jrr_set_error("silhouette_loss_grad needs JRR_FLAG_KEEP_VERTS"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  e->fwd_cached = false;
  smpl_forward(e, x6d, nullptr, betas, true, true, nullptr, s, nullptr, nullptr, 0, true);      // vertices pose-major, as in the loop
  launch_mask_sq(mask, e->smask, e->B, s, e->sil);
  e->smask_valid = false;
  const float silscale = (float)(2.0 * 100.0 / ((double)e->bnorm * (double)e->sil * (double)e->sil));      // optimize.py:252 weight 100
  { int rcs = launch_sil_raster_adj(e->VTb, e->BP, cam, e->m.faces_int_pk ? e->m.faces_int_pk : e->m.faces_pk, e->m.nfaces, mask, e->smask, e->cover,
                                    e->ncover, e->sqsil, silscale, e->gcam, 0, e->B, s, e->sil, e->VPM);
    if (rcs) return rcs; }      // (sizes other than 224 / 256: the stand-alone forward / backward pair only)
  if (sqsil) JRR_HIP(hipMemcpyAsync(sqsil, e->sqsil, (size_t)e->B * 4, hipMemcpyDeviceToDevice, s));
  if (dverts) launch_verts_untranspose(e->VTb, dverts, V * 3, V, nullptr, nullptr, e->B, e->BP, s, e->m.p2v);
  if (dcam) JRR_HIP(hipMemcpyAsync(dcam, e->gcam, (size_t)e->B * 3 * 4, hipMemcpyDeviceToDevice, s));
  CHECK_LAUNCH();
  return JRR_OK;
}

