// Internal (never installed): what an engine may still use of what it stored -- the regressor's layouts, the J step's forward, the
// support lists and tables, the folded tables, the mask sums -- and the rules by which calls keep or drop it.  Plain C++17, no HIP: a
// host compiler builds it alone (tools/engine_state_check.cpp runs the rules without a GPU).  The facts are private: entry points
// read them through the accessors and predicates and change them through the named transitions only.
#pragma once

namespace jrr {

class EngineState {
 public:
  // ---- what is stored ----
  bool have_J() const { return have_J_; }                // a regressor has been uploaded and normalised
  bool have_mask() const { return have_mask_; }          // ... with a mask (the engine's copy is in Jmask)
  bool tab_static() const { return tab_static_; }        // the W parts of the backward operand records are in place
  bool have_jsup() const { return have_jsup_; }          // the engine keeps support lists of the normalised regressor (KEEP_VERTS)
  bool folded() const { return folded_; }                // folded mode asked for (jrr_engine_set_folded)
  bool fold_valid() const { return fold_valid_; }        // the folded tables are those of the current regressor
  bool folded_active() const { return folded_ && fold_valid_; }
  bool fwd_cached() const { return fwd_cached_; }        // a J step's forward (v_posed, skinning transforms, vertices) is in the workspace
  bool verts_partial() const { return verts_partial_; }  // VTb holds the support tiles of the last J step only
  bool smask_valid() const { return smask_valid_; }      // smask holds sum(mask^2) of the silhouette masks that are set
  int nact() const { return nact_; }                     // tiles in act_list
  int sup_nsv() const { return sup_nsv_; }               // vertices in the support tables

  // ---- predicates ----
  // the stored forward is that of exactly these pose buffers
  bool stored_forward_is(const float* x6d, const float* betas) const { return fwd_cached_ && fc_x6d_ == x6d && fc_betas_ == betas; }
  // jrr_j_support_info has seen fits = 1 for the current regressor lineage: the host KNOWS that the support lists fit
  bool support_known() const { return have_jsup_ && jsup_fits_known_; }
  // ... and a J step with this mask keeps that knowledge (another mask may un-mask entries: the support may grow)
  bool support_known_under(const float* mask) const { return jsup_fits_known_ && mask == jsup_mask_; }
  // the stored vertices serve a regressor product: all of them are there, or the support's tiles are and only those are read
  bool stored_verts_usable() const { return !verts_partial_ || support_known(); }
  // the joint-loss iteration on the regressor's support tiles only (JRR_FLAG_SUPPORT_TILES).  From outside the
  // state: the engine's flag, whether a silhouette term is set, whether the model runs k_lbs_bwd16 (uses_r16)
  bool use_tile_list(bool support_tiles_flag, bool sil_mask_set, bool r16) const {
    return support_tiles_flag && act_valid_ && support_known() && !sil_mask_set && r16 && !folded_active();
  }
  // ... per support VERTEX in one workgroup per 32-pose group (supk.h): the same condition and the support's vertex tables built
  bool use_sup_vertices(bool support_tiles_flag, bool sil_mask_set, bool r16) const {
    return use_tile_list(support_tiles_flag, sil_mask_set, r16) && sup_valid_;
  }

  // ---- transitions ----
  void engine_created(bool keep_verts) { have_jsup_ = keep_verts; }
  // FT / AT / VPb / VTb or another section a reusing call reads is about to be overwritten, or the call may run between a J step
  // and its reuse: the stored forward is gone
  void workspace_overwritten() { fwd_cached_ = false; }
  // a J step's forward of these pose buffers is in the workspace
  void forward_stored(const float* x6d, const float* betas) { fwd_cached_ = true; fc_x6d_ = x6d; fc_betas_ = betas; }
  // a forward wrote VTb: all vertices, or (partial) the tiles that hold a support entry only
  void verts_stored(bool partial) { verts_partial_ = partial; }
  // A regressor arrived.  From outside: nothing is known about its support until jrr_j_support_info says so, so the tile list and the
  // support tables go, the folded tables are stale, and stored vertices that cover the OLD support's tiles only are useless (all
  // 6890 of them do not depend on the regressor: that forward stays).  Through a J step (the unfused second half): regressor_stepped.
  void regressor_uploaded(const float* mask, bool from_j_step) {
    if (from_j_step) { regressor_stepped(mask); return; }
    jsup_fits_known_ = false; act_valid_ = false; sup_valid_ = false;
    if (verts_partial_) fwd_cached_ = false;
    have_mask_ = mask != nullptr; jsup_mask_ = mask;
    fold_valid_ = false;
  }
  // A J step moved the regressor.  The stored forward does not depend on the regressor: it survives.  The stepped support is a subset
  // of the old one under the same mask (ReLU' = 0 outside it: Adam never re-activates an entry), so what is known about it survives
  // too, and the tile list and support tables stay supersets; another mask drops the knowledge.  The folded tables are stale.
  void regressor_stepped(const float* mask) {
    jsup_fits_known_ = support_known_under(mask);
    have_mask_ = mask != nullptr; jsup_mask_ = mask;
    fold_valid_ = false;
  }
  void static_tables_written() { tab_static_ = true; }
  void regressor_ready() { have_J_ = true; }             // the upload's launches went through
  // jrr_j_support_info read the device's answer: the tile list and the support tables are rebuilt from it (or not at all)
  void support_reported(bool fits) { jsup_fits_known_ = fits; act_valid_ = false; sup_valid_ = false; }
  void tile_list_built(int n) { nact_ = n; act_valid_ = true; }
  void support_tables_built(int nsv) { sup_nsv_ = nsv; sup_valid_ = true; }
  // the device saw the support leave what was reported (J or its mask edited in place): nothing derived from it holds
  void support_grew_unannounced() { jsup_fits_known_ = false; act_valid_ = false; sup_valid_ = false; fwd_cached_ = false; }
  void folded_set(bool on) { folded_ = on; }
  void fold_rebuilt() { fold_valid_ = true; }
  // the silhouette masks changed, or smask was overwritten with another mask's sums: recomputed by the next iteration that needs them
  void silhouette_mask_changed() { smask_valid_ = false; }
  void mask_sums_computed() { smask_valid_ = true; }

 private:
  bool have_J_ = false, have_mask_ = false, tab_static_ = false;
  bool folded_ = false, fold_valid_ = false;
  bool fwd_cached_ = false; const float *fc_x6d_ = nullptr, *fc_betas_ = nullptr;
  bool verts_partial_ = false;
  bool have_jsup_ = false, jsup_fits_known_ = false; const float* jsup_mask_ = nullptr;
  bool act_valid_ = false; int nact_ = 0;
  bool sup_valid_ = false; int sup_nsv_ = 0;
  bool smask_valid_ = false;
};

}  // namespace jrr
