// What the three LBS sources share (lbs_fwd.hip, lbs_bwd.hip, jreg.hip): the layout of the per-tile operand records, the LDS-DMA
// copies, the pairing of the two workgroups of a CU (device arithmetic and the host's condition for it) and the dispatch from a model's
// joint-sparse class to the kernels' template arguments.  Everything else is private to its file.
#pragma once
#include <type_traits>

#include "jrr_common.h"

namespace jrr {

constexpr int W_FLOATS = NJ * 32;             // 768
constexpr int JN_FLOATS = 32 * 32;            // 1024
// per-tile operand record of the backward kernel: [Jn 18x32 | W^T 24x32 | W 32x32(j) | pad] = 10 KB
constexpr int TB_JN = 0, TB_WJV = NHP * 32, TB_WVJ = TB_WJV + W_FLOATS, TB_FLOATS = 2560;
// joint-sparse variants: the W block holds the segment-window weights W16 [16 n][36] (576 floats, jrr_common.h) instead of
// [32 v][32 j]; the record then ends at 1920 floats: 8 of the 10 DMA pieces
constexpr int TB_W16_FLOATS = 16 * 36, TB_PIECES_SPARSE = 8;
// record of k_lbs_bwd16 (lbs_bwd.hip): JN | WT | WD | JL, 7 DMA pieces
constexpr int R16_JN = 0, R16_WT = 640, R16_WD = 1024, R16_JL = 1536, R16_WX = 1552, R16_FLOATS = 1792, R16_PIECES = 7;   // WX: K step 3 of WT
// v_mfma_f32_16x16x1_4b_f32: four independent 16x16 outer products per instruction (block = lane / 16), 8 passes = half the
// issue time of v_mfma_f32_32x32x2_f32 (33 vs 64 clocks measured, tools/probe/mfma16_probe.hip):
//   A: lane l holds A_blk[row l % 16],  B: lane l holds B_blk[col l % 16],  blk = l / 16
//   D: register 4 blk + i of lane l holds D_blk[row 4 (l / 16) + i][col l % 16]
// (k_lbs_fwd's regressor product and the role kernel k_lbs_bwd's joint-window products)
__device__ __forceinline__ f32x16 mfma16(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_16x16x1f32(a, b, c, 0, 0, 0); }

// one wave-instruction: 64 lanes x 16 B from per-lane global addresses into LDS [dst, dst + 1 KB)
__device__ __forceinline__ void dma16(const float* gsrc_lane, float* lds_dst_wave) {
  __builtin_amdgcn_global_load_lds(JRR_GLB(gsrc_lane), JRR_LDS(lds_dst_wave), 16, 0, 0);
}
// same with the address split as (wave-uniform base, 32-bit per-lane offset in floats).  The base is
// laundered through an SGPR so the compiler keeps it scalar (saddr form) and cannot fold it into a
// per-copy VGPR offset or hoist it out of the tile loop (either costs ~2 VGPRs per copy).
__device__ __forceinline__ void dma16u(const float* base_uniform, unsigned lane_off, float* lds_dst_wave) {
  asm volatile("" : "+s"(base_uniform));
  __builtin_amdgcn_global_load_lds(JRR_GLB(base_uniform + lane_off), JRR_LDS(lds_dst_wave), 16, 0, 0);
}

// ---- pairing: the two workgroups of a CU share a pair of vertex chunks (k_lbs_fwd, k_lbs_bwd16) ----
// Host: `groups` pose groups x `nvc` vertex chunks are exactly one round of two workgroups per CU (512 slots) with an even number of
// chunks and whole pose groups per XCD.  The planner (api.hip plan_geometry) picks chunk counts for which this holds and the launchers
// turn the pairing on where it does: one condition, or the pairing silently does not happen.
inline bool pairs_one_round(int groups, int nvc) { return groups * nvc == 512 && (nvc & 1) == 0 && 32 % (nvc / 2) == 0; }
// Device: the work of this workgroup in such a launch.  The two workgroups of a CU are the dispatch slots j and j + per_xcd / 2 of an
// XCD; they take the pose group `group` and the chunks vc = 2 vcp, 2 vcp + 1 of one pair, whose NT tiles [P0, P1) the first-dispatched
// one splits at `paired` thousandths: it walks [t_begin, t_end) = [P0, mid), its partner [mid, P1).  (Why, and the measured shares:
// at the two call sites.)
__device__ __forceinline__ void pair_chunks(int paired, int NT, int nvc, int& group, int& vc, int& t_begin, int& t_end) {
  const int per_xcd = gridDim.x >> 3, xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int p = j % (per_xcd / 2), slot = j / (per_xcd / 2);
  const int npair = nvc / 2, groups_per_xcd = (per_xcd / 2) / npair;
  group = xcd * groups_per_xcd + p / npair;
  const int vcp = p % npair;
  vc = 2 * vcp + slot;
  const int P0 = (int)((long)NT * vcp / npair), P1 = (int)((long)NT * (vcp + 1) / npair);
  const int mid = P0 + ((P1 - P0) * paired + 500) / 1000;      // `paired` = the first workgroup's share in thousandths
  t_begin = slot ? mid : P0;
  t_end = slot ? P1 : mid;
}

// ---- a model's joint-sparse class as template arguments ----
// f(KJ, WIDE) with KJ = std::integral_constant<int, 8 | 12> and WIDE = std::bool_constant<wide> for a joint-sparse class (Model::kjs,
// Model::wide_tiles), f(0, false) for the dense form: the five classes the kernels are built for, decided in one place.
template <class F>
inline void with_skin_class(int kjs, bool wide, F&& f) {
  auto with_wide = [&](auto KJ) {
    if (wide) f(KJ, std::true_type{});
    else f(KJ, std::false_type{});
  };
  if (kjs == 8) with_wide(std::integral_constant<int, 8>{});
  else if (kjs == 12) with_wide(std::integral_constant<int, 12>{});
  else f(std::integral_constant<int, 0>{}, std::false_type{});
}

}  // namespace jrr
