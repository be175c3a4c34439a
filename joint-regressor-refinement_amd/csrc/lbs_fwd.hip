// SMPL linear blend skinning + H36M joint regression on the fp32 matrix cores.
//
// Restates (SURVEY.md Appendix A steps 1,3,5 = smplx 0.1.26 lbs(); /root/reference call sites
// scripts/utils.py:94-98):
//   v_posed = v_template + shapedirs.beta + posedirs.(R-I)      -> one K=218 product  D . F
//   T_v     = sum_j W[v,j] A_j                                   -> K=24 products      W . A
//   verts   = T_v[:3,:3] v_posed + T_v[:3,3]
//   joints  = Jn @ verts                                         -> K=6890 product
//
// Every tile lives in the accumulator layout of v_mfma_f32_32x32x2_f32 with
//   rows = 32 vertices (registers), columns = 32 poses (lanes),
// so the three products chain without leaving registers: the blend product and the skinning
// product both produce (vertex, pose) tiles, the per-element affine combine is plain VALU on
// matching registers, and the regressor product consumes the vertex tile as its B operand
// (it sums over the tile's ROW index, guide section 3 "accumulator tile as the next operand").
// (the backward kernels: lbs_bwd.hip; the regressor's normalisation and the J step's bookkeeping: jreg.hip; shared: lbs_tile.h)
#include "jrr_common.h"
#include "kernels.h"
#include "lbs_tile.h"

namespace jrr {

// ------------------------------------------------------------------------------------------
// forward
//   grid.x = (BP/128) * nvc workgroups of 256 threads; wave w owns poses [bg*128 + 32w, +32)
//   and loops over the vertex tiles of chunk vc.
//
//   EVERY MFMA operand is read from LDS.  Operands are staged by LDS-DMA (global_load_lds_dwordx4:
//   no VGPR round trip, asynchronous) into a 2-deep ring, one stage ahead of the MFMAs, one
//   workgroup barrier per stage.  Per vertex tile there are 13 stages:
//     s = 0..6   blend product, K chunk kc = s: basis rows D[32 k][3][32 v] (12 KB, shared by the
//                four waves) + feature rows F^T[32 k][128 poses] (16 KB)        48 MFMA / wave
//     s = 7..12  skinning, half-stage (r, h): two A^T blocks [24 j][128 poses] (24 KB):
//                h = 0: translation column c = 3 and c = 0;  h = 1: c = 1, 2, then the
//                regressor product  joints^T += Jn . verts_r                 24 (+16) MFMA / wave
//   The skinning-weight / regressor tiles (W^T, Jn) ride with stage 0 into a per-tile-parity
//   region.  outputs: JP [nvc][3][17][BP] joint partials; optional VPb [3][VP/4][BP][4] (v_posed in row quads,
//   kept for the backward pass) and VTb [3][VP/4][BP][4] (the vertices, same layout; k_verts_untranspose turns
//   them into the reference's (B,6890,3) and/or projects them for the silhouette renderer).
// ------------------------------------------------------------------------------------------
constexpr int STG_FLOATS = KCH * 96 + KCH * BG;   // 3072 (D chunk) + 4096 (F chunk) = 7168
constexpr int WJ_FLOATS = W_FLOATS + JN_FLOATS;   // 1792
constexpr int NSTAGE = NKCH + 6;                  // 13
// v_mfma_f32_32x32x2_f32 instructions per wave and vertex tile: 109 K-pairs x 3 planes + 12 x 24 / 2 + 3 x 16
constexpr int LBS_FWD_MFMA_PER_TILE = (KF / 2) * 3 + 6 * 24 + 3 * 16;

// KJ > 0 (joint-sparse skinning, Model::kjs = 8 or 12): a tile's skinning product only runs over the tile's own <= KJ
// joints -- Wjv then is the compacted W^T [VT][KJ][32], jl the joint lists -- in THREE stages per tile (r = 0, 1, 2:
// the four A^T blocks (r, c) of the listed joints, 16 KB; T_{r,3}, T_{r,0}, T_{r,1}, T_{r,2} = 4 x KJ/2 MFMA; combine;
// regressor 16 MFMA) instead of six half-stages of 24 (+16) MFMA: with KJ = 8, 423 instead of 519 MFMA per tile and 48
// instead of 144 KB of A^T streamed per tile (KJ = 12: 447 MFMA, 72 KB).  Skipped terms are exact zeros: the result is the dense product's up to the
// grouping of the K pairs.
// WIDE: the model has tiles with more than KJ joints (per-tile classes: such a tile runs a second pass over slots KJ .. 2 KJ - 1).
// A separate instantiation: the branches of the second pass cost the stage loop ~2 % even when never taken (measured: 0.361 vs
// 0.369 ms at B = 4096), so a model without wide tiles runs the kernel without them.
template <bool STORE_VP, bool STORE_VERTS, int KJ, bool WIDE, bool LIST = false>
__global__ __launch_bounds__(256, 2) void k_lbs_fwd(const float* __restrict__ Dk, const float* __restrict__ Wjv,
                                                    const float* __restrict__ Jn_vi, const float* __restrict__ FT,
                                                    const float* __restrict__ AT, float* __restrict__ VPb,
                                                    float* __restrict__ JP, float* __restrict__ VTb, int B, int BP,
                                                    int nvc, long long* __restrict__ probe, int paired,
                                                    const int* __restrict__ jl, const int* __restrict__ tnj,
                                                    const int* __restrict__ vmask, const int* __restrict__ tl, int ntl, int vpm) {
  // vpm (STORE_VERTS only): VTb is a POSE-MAJOR buffer [BP][3][VP] -- what the fused rasteriser reads (round 5).  A pose's 32 rows of
  // a tile sit in two lanes (l and l + 32: rows 8 g + 4 half + 0..3), whose four 16-byte stores per plane complete one 128-byte
  // line of that pose; the rasteriser then loads a pose's 83 KB contiguously instead of 5184 pieces out of 5184 cache lines.
  // LIST: the launch covers the ntl tiles tl[0 .. ntl) only (ascending) -- the tiles that hold an entry of the regressor's support.
  // Every other tile multiplies its vertices by a zero block of the regressor: it adds exact zeros to the joints, and nothing else
  // of it is read by the joint-loss iteration (the backward kernels skip the same tiles).
  const int NT = LIST ? ntl : VT;
  // vmask (STORE_VERTS only, nullable): vertices leave the chip only for the tiles with vmask[tile] != 0 -- the J step over the
  // regressor's support reads a few dozen vertex rows, not 340 MB
  constexpr bool SPARSE = KJ > 0;
  constexpr int KJS = SPARSE ? KJ : 8;                       // (8: keeps the dead sparse branch of the dense variant well-formed)
  constexpr int NST = SPARSE ? NKCH + 3 : NSTAGE;            // stages per vertex tile
  constexpr int WT_FLOATS = SPARSE ? KJS * 32 : W_FLOATS;    // W^T rows staged per tile (a WIDE tile: 2 KJS rows)
  constexpr int WT_COPIES = (WT_FLOATS + 255) / 256, WT_COPIES_WIDE = (2 * WT_FLOATS + 255) / 256;
  __shared__ float lds[2 * STG_FLOATS + 2 * WJ_FLOATS];
  // shader-clock probe (profiling only), see jrr_engine_probe_read
  const long long probe_t0 = probe ? clock64() : 0, probe_w0 = probe ? wall_clock64() : 0;
  float* const ring = lds;
  float* const wj = lds + 2 * STG_FLOATS;

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  int bg = L / nvc, vc = L % nvc;
  int t_begin = (int)((long)NT * vc / nvc), t_end = (int)((long)NT * (vc + 1) / nvc);
  if (paired) {
    // One full round of 512 workgroups = two per CU, and the two do NOT progress evenly: the first-dispatched one
    // wins the issue arbitration and would finish ~20 % earlier, leaving its partner alone (one wave per SIMD) for
    // the tail (measured with per-workgroup s_memrealtime stamps).  So the two workgroups of a CU
    // -- dispatch slots j and j + per_xcd/2 of an XCD -- share one PAIR of vertex chunks of the same pose group and
    // the first one takes the larger share of the pair's tiles (16 : 11 at B = 4096, launcher).  Static, hence still bitwise reproducible;
    // if the hardware paired differently the split would merely be uneven.
    pair_chunks(paired, NT, nvc, bg, vc, t_begin, t_end);
  }
  const int b0 = bg * BG + wave * BT;
  const size_t bcol = (size_t)b0 + l31;
  const unsigned qoff = (unsigned)half * (unsigned)BP + (unsigned)bcol;          // lane part of a (row quad, pose) address, in quads
  // DMA addressing = wave-uniform base pointer (SGPR pair) + one 32-bit per-lane offset (VGPR), so
  // the 78 copies per tile cost scalar address arithmetic only.  Row-pair pattern: lanes 0-31
  // fetch row 2o, lanes 32-63 row 2o+1, 16 B per lane.
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const unsigned lane_rp = (unsigned)half * (unsigned)BP + (unsigned)l31 * 4u;   // floats
  const unsigned lane_ln = (unsigned)lane * 4u;                                  // floats
  const float* const Fbg = FT + (size_t)bg * BG * 4;            // FT in K-quads [KFP / 4][BP][4] (k_prep_fwd writes it beside the row-major copy)
  const float* const Abg = AT + (size_t)bg * BG;
  unsigned lane_jl[2] = {0, 0};   // SPARSE: (row of this lane's joint of the current tile) * BP + pose offset, floats
  unsigned lane_jx[2] = {0, 0};   // ... of the SECOND pass of a wide tile (slots KJS .. 2 KJS - 1)
  int wide = 0, wide_next = 0;    // this tile / the next tile has more than KJS joints (wave-uniform)
  long long n_extra = 0;          // second passes run (probe)

  // ---- DMA issue for stage s of tile vt into ring slot `slot` ----
  auto issue = [&](int vt, int s, int slot, int pass = 0, int wide_w = 0, int par = 0) {      // par: W / Jn buffer of the tile (s == 0)
    float* dst = ring + slot * STG_FLOATS;
    if (s < NKCH) {
      // K chunk s of the basis, K-QUADS [8 quads][3][32 v][4]: one contiguous 12 KB block of Dk
      const float* dsrc = Dk + ((size_t)vt * KFP + s * KCH) * 96;
#pragma unroll
      for (int i = 0; i < 3; ++i) { const int o = wv + 4 * i; dma16u(dsrc + o * 256, lane_ln, dst + o * 256); }
      // ... and of the features, K-quads [8 quads][128 poses][4]: piece o = (quad o / 2, poses (o % 2) * 64 + lane)
      float* fdst = dst + KCH * 96;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = wv + 4 * i;
        dma16u(Fbg + ((size_t)(s * (KCH / 4) + (o >> 1)) * BP + (o & 1) * 64) * 4, lane_ln, fdst + o * 256);
      }
      if (s == 0) {
        float* wdst = wj + par * WJ_FLOATS;
        // (the table holds NJ slot rows per tile; a wide tile -- `wide_w`, wave-uniform -- stages 2 KJS of them)
        if (wv < ((SPARSE && wide_w) ? WT_COPIES_WIDE : WT_COPIES)) dma16u(Wjv + (size_t)vt * W_FLOATS + wv * 256, lane_ln, wdst + wv * 256);
        dma16u(Jn_vi + (size_t)vt * JN_FLOATS + wv * 256, lane_ln, wdst + W_FLOATS + wv * 256);
      }
    } else if (SPARSE) {
      // four blocks [KJS joints][128 poses] of A^T, components (r, 3), (r, 0), (r, 1), (r, 2); this wave copies row pair
      // wv of each -- the rows of joints jl[2 wv], jl[2 wv + 1] (lane offset `lane_jl[0]`, set per tile) -- and, with 12
      // joints, waves 0 and 1 also row pair 4 + wv (`lane_jl[1]`)
      const int r = s - NKCH;
      const unsigned o0 = pass ? lane_jx[0] : lane_jl[0], o1 = pass ? lane_jx[1] : lane_jl[1];
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const int c = (ci == 0) ? 3 : ci - 1;
        dma16u(Abg + (size_t)((r * 4 + c) * NJ) * BP, o0, dst + ci * (KJS * BG) + wv * 256);
        if (KJS > 8 && wv < KJS / 2 - 4) dma16u(Abg + (size_t)((r * 4 + c) * NJ) * BP, o1, dst + ci * (KJS * BG) + (4 + wv) * 256);
      }
    } else {
      const int h = s - NKCH, r = h >> 1;
      const int c0 = (h & 1) ? 1 : 3, c1 = (h & 1) ? 2 : 0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int o = wv + 4 * i;   // 12 row pairs per block
        dma16u(Abg + (size_t)((r * 4 + c0) * NJ + 2 * o) * BP, lane_rp, dst + o * 256);
        dma16u(Abg + (size_t)((r * 4 + c1) * NJ + 2 * o) * BP, lane_rp, dst + NJ * BG + o * 256);
      }
    }
  };

  // H36M joints 0..15 as block accumulators of v_mfma_f32_16x16x1_4b_f32 (17 joint rows in a 32-row product waste 47 % of
  // it; 16 rows on the four-block instruction take half the issue time), joint 16 as a per-lane partial on the vector ALU
  f32x16 jacc[3] = {zero16(), zero16(), zero16()};
  float j16[3] = {0.f, 0.f, 0.f};
  f32x16 vp[3];
  f32x16 vr;

  // joints^T[i, b] += sum_v Jn[i, v] verts_r[v, b] for the tile in `vr`: A operand Jn[i = lane % 16][v = acc_row(q, half)]
  // (the [v][32 i] tile of the record, read with i = lane % 16), B operand register q of the vertex tile; one four-block
  // instruction adds the two rows acc_row(q, 0), acc_row(q, 1) for all 32 pose columns (blocks 0 + 2: columns 0..15,
  // 1 + 3: 16..31).  Operands four steps ahead (an instruction is 32 clocks).
  // (the first four A operands are requested by the caller -- `ra`, before anything that would fence the schedule: in the WIDE
  // instantiation the second-pass branch sits between the skinning products and this product, and operands requested behind it
  // exposed ~200 clocks of LDS latency per stage)
  auto regress_operands = [&](const float* ldsJ, float (&ra)[4]) __attribute__((always_inline)) {
    const float* jp = ldsJ + half * 128 + (lane & 15);
#pragma unroll
    for (int q = 0; q < 4; ++q) ra[q] = jp[acc_row_u(q) * 32];
  };
  auto regress = [&](auto R_, const float* ldsJ, const float (&ra)[4]) __attribute__((always_inline)) {
    constexpr int r = decltype(R_)::value;
    const float* jp = ldsJ + half * 128 + (lane & 15);              // row acc_row(q, half) = acc_row_u(q) + 4 half
    float a0 = ra[0], a1 = ra[1], a2 = ra[2], a3 = ra[3];
    // (a second accumulator chain -- even / odd rows, added at the end -- fits since the quad-operand blend stage and was measured
    // SLOWER: 0.3641 vs 0.3614 ms; the single chain's dependent issue is covered by the SIMD's other wave)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float ac = a0;
      a0 = a1; a1 = a2; a2 = a3;
      __builtin_amdgcn_sched_barrier(0);
      jacc[r] = mfma16(ac, vr[q], jacc[r]);
      __builtin_amdgcn_sched_barrier(0);
      if (q + 4 < 16) a3 = jp[acc_row_u(q + 4) * 32];
    }
    // joint 16 on the vector ALU: Jn[16][v] verts[v][b] over this lane's rows (the two lane halves are summed at the end)
    const float* sp = ldsJ + half * 128 + 16;
    float p16 = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) p16 = fmaf(sp[acc_row_u(q) * 32], vr[q], p16);
    j16[r] += p16;
  };

  // pose-major vertex store (vpm): wave-uniform row base + a 32-bit lane offset formed AT the store from a laundered lane index
  // (hoisted out of the tile loop it costs the WIDE instantiations registers they do not have)
  auto pm_store = [&](int r, int vt, int g4, const f32x4& t) __attribute__((always_inline)) {
    const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const unsigned lo = ((unsigned)b0 + (unsigned)(ln & 31)) * (3u * VP) + 4u * (unsigned)(ln >> 5);
    float* base = VTb + ((size_t)r * VP + vt * 32 + 8 * g4);
    asm volatile("" : "+s"(base));
    *(JRR_GPTR(f32x4))(base + lo) = t;
  };
  const int t_first = (t_begin < t_end) ? (LIST ? tl[t_begin] : t_begin) : 0;
  if (SPARSE && WIDE && t_begin < t_end) wide_next = tnj[t_first] > KJS;
  if (t_begin < t_end) issue(t_first, 0, 0, 0, wide_next, t_begin & 1);
  int g = 0;   // global stage counter: ring slot = g & 1
  for (int ix = t_begin; ix < t_end; ++ix) {
    const int vt = LIST ? tl[ix] : ix;                                       // the tile (wave-uniform)
    const int vtn = LIST ? ((ix + 1 < t_end) ? tl[ix + 1] : 0) : ix + 1;      // the next one (used under ix + 1 < t_end only)
    const float* ldsW = wj + (ix & 1) * WJ_FLOATS;
    const float* ldsJ = ldsW + W_FLOATS;
    const bool stv = STORE_VERTS && (!vmask || vmask[vt] != 0);      // wave-uniform
    if (SPARSE) {      // the skinning copies of this tile are issued from its stage NKCH - 1 on
      if (WIDE) {
        wide = wide_next;
        wide_next = (ix + 1 < t_end) ? (tnj[vtn] > KJS) : 0;                    // wave-uniform: scalar loads
      }
      const int j0 = jl[vt * NJ + 2 * wv], j1 = jl[vt * NJ + 2 * wv + 1];
      lane_jl[0] = (unsigned)(half ? j1 : j0) * (unsigned)BP + (unsigned)l31 * 4u;
      if (KJS > 8 && wv < KJS / 2 - 4) {
        const int j2 = jl[vt * NJ + 8 + 2 * wv], j3 = jl[vt * NJ + 8 + 2 * wv + 1];
        lane_jl[1] = (unsigned)(half ? j3 : j2) * (unsigned)BP + (unsigned)l31 * 4u;
      }
      if (WIDE && wide) {      // second pass: slots KJS .. 2 KJS - 1
        const int k0 = jl[vt * NJ + KJS + 2 * wv], k1 = jl[vt * NJ + KJS + 2 * wv + 1];
        lane_jx[0] = (unsigned)(half ? k1 : k0) * (unsigned)BP + (unsigned)l31 * 4u;
        if (KJS > 8 && wv < KJS / 2 - 4) {
          const int k2 = jl[vt * NJ + KJS + 8 + 2 * wv], k3 = jl[vt * NJ + KJS + 8 + 2 * wv + 1];
          lane_jx[1] = (unsigned)(half ? k3 : k2) * (unsigned)BP + (unsigned)l31 * 4u;
        }
        ++n_extra;
      }
    }
    static_for<0, NST>([&](auto S_) {
      constexpr int s = decltype(S_)::value;
      // Stage g landed; slot (g+1)&1 is free again.  The copies of stage g were issued at the start of the previous
      // stage, BEFORE that stage's v_posed / vertex stores: exactly those stores are left in flight (they get one more
      // stage to retire instead of stalling this barrier; barrier_keep_vm).  First stage of the kernel: nothing younger.
      {
        constexpr int sp = (s == 0) ? NST - 1 : s - 1;                    // previous stage
        constexpr int hp = sp - NKCH;                                      // its skinning (half-)stage, if any
        constexpr int nst = (hp < 0) ? 0
                            : SPARSE ? (STORE_VP ? 4 : 0) + (STORE_VERTS ? 4 : 0)
                                     : (STORE_VP ? 2 : 0) + ((STORE_VERTS && (hp & 1)) ? 4 : 0);
        // (with a tile mask the vertex stores of the previous stage may not exist: count the v_posed stores only -- waiting for
        // more than necessary is always safe)
        constexpr int nst_vp = (hp < 0) ? 0 : SPARSE ? (STORE_VP ? 4 : 0) : (STORE_VP ? 2 : 0);
        if (s == 0 && ix == t_begin) barrier_keep_vm<0>();
        else if (STORE_VERTS && nst != nst_vp && vmask) barrier_keep_vm<nst_vp>();
        else barrier_keep_vm<nst>();
      }
      // the stage that follows this one: a wide tile's skinning stage r is followed by its second pass over the same r
      if (SPARSE && WIDE && s >= NKCH && wide) issue(vt, s, (g + 1) & 1, 1);
      else if (s + 1 < NST) issue(vt, s + 1, (g + 1) & 1);
      else if (ix + 1 < t_end) issue(vtn, 0, (g + 1) & 1, 0, wide_next, (ix + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);   // the counted wait above relies on: copies first, this stage's stores after
      const float* buf = ring + (g & 1) * STG_FLOATS;
      if constexpr (s < NKCH) {
        if (s == 0) { vp[0] = zero16(); vp[1] = zero16(); vp[2] = zero16(); }
        // Both operands arrive in K-QUADS: a lane's ds_read_b128 is FOUR K steps (a K pair may take any two k as long as both
        // operands agree: step t of group g takes k = 8 g + t and 8 g + 4 + t, the lane half picks the quad 2 g + half) --
        // 4 LDS reads per 12 matrix instructions instead of 16.  The last chunk holds k = 192 .. 217: its group 3 has only the
        // steps t = 0, 1 (k = 216, 217 against zero rows).  Operands of group g + 1 are requested right after the first
        // instruction of group g.
        // (Entering stage s + 1 INSIDE the last group of stage s -- barrier, first operand reads and the copies of stage s + 2 behind
        // the group's first instruction, so that its other eleven cover the reads -- was built and measured SLOWER, 0.3527 -> 0.3610
        // ms: the barrier then asks for the next stage's copies eleven instructions earlier, a quarter of the one stage the 2-deep ring
        // gives them.  Reading group 3 of the last chunk (two live steps) as four 8-byte reads, instead of the 16-byte reads the compiler
        // narrows into overlapping registers with a wait between each two, was measured too: 0.3507 -> 0.3520 ms.  DESIGN.md section 8.)
        constexpr int ngroups = 4;
        const f32x4* dq = reinterpret_cast<const f32x4*>(buf) + half * 96 + l31;                          // quad q, plane c: + (q * 3 + c) * 32
        const f32x4* fq = reinterpret_cast<const f32x4*>(buf + KCH * 96) + half * BG + wave * BT + l31;   // quad q: + q * 128
        f32x4 a0 = dq[0], a1 = dq[32], a2 = dq[64], bq = fq[0];
        f32x4 n0 = a0, n1 = a1, n2 = a2, nb = bq;
#pragma unroll
        for (int gq = 0; gq < ngroups; ++gq) {
          constexpr int last_steps = KF - (NKCH - 1) * KCH - 24;      // valid steps of group 3 of the last chunk: 218 - 192 - 24 = 2
          const int nsteps = (s == NKCH - 1 && gq == ngroups - 1) ? last_steps : 4;
          const f32x4 c0 = a0, c1 = a1, c2 = a2, cb = bq;
          __builtin_amdgcn_sched_barrier(0);
          vp[0] = mfma(c0[0], cb[0], vp[0]);
          __builtin_amdgcn_sched_barrier(0);
          if (gq + 1 < ngroups) {
            n0 = dq[(2 * gq + 2) * 96]; n1 = dq[(2 * gq + 2) * 96 + 32]; n2 = dq[(2 * gq + 2) * 96 + 64];
            nb = fq[(2 * gq + 2) * BG];
          }
          __builtin_amdgcn_sched_barrier(0);
          vp[1] = mfma(c1[0], cb[0], vp[1]);
          vp[2] = mfma(c2[0], cb[0], vp[2]);
#pragma unroll
          for (int t = 1; t < 4; ++t) {
            if (t >= nsteps) break;
            vp[0] = mfma(c0[t], cb[t], vp[0]);
            vp[1] = mfma(c1[t], cb[t], vp[1]);
            vp[2] = mfma(c2[t], cb[t], vp[2]);
          }
          a0 = n0; a1 = n1; a2 = n2; bq = nb;
        }
      } else if constexpr (SPARSE) {
        constexpr int r = s - NKCH;
        if (STORE_VP) {   // v_posed plane r leaves with skinning stage r: four 16-byte row quads
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 t = {vp[r][4 * g4], vp[r][4 * g4 + 1], vp[r][4 * g4 + 2], vp[r][4 * g4 + 3]};
            *quad_ptr(VPb, (size_t)r * (VP / 4) + vt * 8, g4, BP, qoff) = t;
          }
        }
        const float* wp = ldsW + half * 32 + l31;                       // W^T rows of the listed joints: row 2 p + half
        const float* ab = buf + half * BG + wave * BT + l31;             // block ci at + ci * KJS * BG, row pair p at + 2 p BG
        float w[KJS / 2], x0[KJS / 2], x1[KJS / 2];
#pragma unroll
        for (int pq = 0; pq < KJS / 2; ++pq) {
          w[pq] = wp[2 * pq * 32];
          x0[pq] = (WIDE && KJS > 8) ? 0.f : ab[2 * pq * BG];
          x1[pq] = (WIDE && KJS > 8) ? 0.f : ab[KJS * BG + 2 * pq * BG];
        }
        f32x16 T = zero16(), U = zero16();
        // TIGHT (12 slots AND wide tiles: a body whose best order still has a 13-joint tile): 30 operand registers per block pair
        // and the regressor operands held across the second-pass branch do not fit 256 registers (7 .. 12 spilled) -- that one
        // instantiation reads the second block pair's operands where they are used and requests the regressor operands behind the
        // branch (exposed LDS latency instead of scratch traffic; no other instantiation changes)
        constexpr bool TIGHT = WIDE && KJS > 8;
        float y0[KJS / 2], y1[KJS / 2];
#pragma unroll
        for (int pq = 0; pq < KJS / 2; ++pq) {                            // T_{r,3}, T_{r,0}; the next two blocks' operands meanwhile
          if (TIGHT) { x0[pq] = ab[2 * pq * BG]; x1[pq] = ab[KJS * BG + 2 * pq * BG]; }
          T = mfma(w[pq], x0[pq], T);
          if (!TIGHT) { y0[pq] = ab[2 * KJS * BG + 2 * pq * BG]; y1[pq] = ab[3 * KJS * BG + 2 * pq * BG]; }
          U = mfma(w[pq], x1[pq], U);
        }
        vr = T + U * vp[0];                      // T_{r,3} + T_{r,0} v_x
        T = zero16(); U = zero16();
#pragma unroll
        for (int pq = 0; pq < KJS / 2; ++pq) {                            // T_{r,1}, T_{r,2}
          if (TIGHT) { y0[pq] = ab[2 * KJS * BG + 2 * pq * BG]; y1[pq] = ab[3 * KJS * BG + 2 * pq * BG]; }
          T = mfma(w[pq], y0[pq], T);
          U = mfma(w[pq], y1[pq], U);
        }
        vr += T * vp[1];                         // T_{r,1} v_y
        vr += U * vp[2];                         // T_{r,2} v_z
        float ra[4];
        if (!TIGHT) regress_operands(ldsJ, ra);
        if (WIDE && wide) {
          // ---- second pass of a WIDE tile (more than KJS joints): the same four products over slots KJS .. 2 KJS - 1,
          //      added to vr.  Its own ring stage: every copy and store of this wave is drained at its barrier (rare path).
          ++g;
          barrier_keep_vm<0>();
          if (s + 1 < NST) issue(vt, s + 1, (g + 1) & 1);
          else if (ix + 1 < t_end) issue(vtn, 0, (g + 1) & 1, 0, wide_next, (ix + 1) & 1);
          __builtin_amdgcn_sched_barrier(0);
          const float* bx = ring + (g & 1) * STG_FLOATS + half * BG + wave * BT + l31;
          const float* wx = ldsW + (KJS + half) * 32 + l31;
          // (two accumulators at a time, like the first pass: the register budget of the hot path is the kernel's)
          T = zero16(); U = zero16();
#pragma unroll
          for (int pq = 0; pq < KJS / 2; ++pq) {
            const float wq = wx[2 * pq * 32];
            T = mfma(wq, bx[2 * pq * BG], T);
            U = mfma(wq, bx[KJS * BG + 2 * pq * BG], U);
          }
          vr += T;
          vr += U * vp[0];
          T = zero16(); U = zero16();
#pragma unroll
          for (int pq = 0; pq < KJS / 2; ++pq) {
            const float wq = wx[2 * pq * 32];
            T = mfma(wq, bx[2 * KJS * BG + 2 * pq * BG], T);
            U = mfma(wq, bx[3 * KJS * BG + 2 * pq * BG], U);
          }
          vr += T * vp[1];
          vr += U * vp[2];
        }
        if (STORE_VERTS && stv) {
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 t = {vr[4 * g4], vr[4 * g4 + 1], vr[4 * g4 + 2], vr[4 * g4 + 3]};
            if (vpm) pm_store(r, vt, g4, t);
            else *quad_ptr(VTb, (size_t)r * (VP / 4) + vt * 8, g4, BP, qoff) = t;
          }
        }
        if (TIGHT) regress_operands(ldsJ, ra);
        regress(std::integral_constant<int, r>{}, ldsJ, ra);
        // after a second pass the next stage's counted wait (which assumes this stage's stores are all younger than its
        // copies) no longer holds: drain
        if (WIDE && wide) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else {
        constexpr int h = s - NKCH, r = h >> 1;
        if (STORE_VP) {   // spread the v_posed stores over the six skinning stages: two 16-byte row quads each
          constexpr int c = h >> 1, g0 = (h & 1) * 2;
#pragma unroll
          for (int g = g0; g < g0 + 2; ++g) {
            const f32x4 t = {vp[c][4 * g], vp[c][4 * g + 1], vp[c][4 * g + 2], vp[c][4 * g + 3]};
            *quad_ptr(VPb, (size_t)c * (VP / 4) + vt * 8, g, BP, qoff) = t;
          }
        }
        const float* wp = ldsW + half * 32 + l31;
        const float* a0 = buf + half * BG + wave * BT + l31;
        const float* a1 = a0 + NJ * BG;
        // two accumulator chains per half-stage, interleaved (a back-to-back MFMA on the SAME accumulator issues
        // every 112 clocks instead of 64: tools/probe/clock_probe.hip), operands of joint pair jp+1 requested
        // right after the first MFMA of pair jp
        f32x16 T = zero16();
        f32x16 U = zero16();
        {   // operands two joint pairs ahead (a pair is only two MFMAs = 128 clocks)
          float w0 = wp[0], x00 = a0[0], x01 = a1[0];
          float w1 = wp[2 * 32], x10 = a0[2 * BG], x11 = a1[2 * BG];
#pragma unroll
          for (int jp = 0; jp < 12; ++jp) {
            const float wc = w0, c0 = x00, c1 = x01;
            w0 = w1; x00 = x10; x01 = x11;
            __builtin_amdgcn_sched_barrier(0);
            T = mfma(wc, c0, T);
            __builtin_amdgcn_sched_barrier(0);
            if (jp + 2 < 12) { w1 = wp[(2 * jp + 4) * 32]; x10 = a0[(2 * jp + 4) * BG]; x11 = a1[(2 * jp + 4) * BG]; }
            __builtin_amdgcn_sched_barrier(0);
            U = mfma(wc, c1, U);
          }
        }
        if ((h & 1) == 0) {
          vr = T + U * vp[0];                    // T_{r,3} + T_{r,0} v_x
        } else {
          vr += T * vp[1];                       // T_{r,1} v_y
          vr += U * vp[2];                       // T_{r,2} v_z
          if (STORE_VERTS && stv) {      // vertices, in the row-quad layout of v_posed: four 16-byte stores per lane
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const f32x4 t = {vr[4 * g], vr[4 * g + 1], vr[4 * g + 2], vr[4 * g + 3]};
              if (vpm) pm_store(r, vt, g, t);
              else *quad_ptr(VTb, (size_t)r * (VP / 4) + vt * 8, g, BP, qoff) = t;
            }
          }
          float ra[4];
          regress_operands(ldsJ, ra);
          regress(std::integral_constant<int, r>{}, ldsJ, ra);
        }
      }
      ++g;
    });
  }
  // (the output addresses are formed HERE, from the hardware lane count and the scalar wave index: hoisted above the tile loop --
  // or from a thread index kept alive across it -- they cost the 12-slot WIDE instantiations spilled registers)
  const int le = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));      // the lane index, from no live register
  const size_t b0e = (size_t)(bg * BG + wv * BT);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int u = 0; u < 4; ++u) {        // block layout: register 4 blk + u = joint 4 (lane / 16) + u, pose column lane % 16 (+ 16)
      const int i = 4 * (le >> 4) + u;
      float* dst = JP + ((size_t)(vc * 3 + r) * NH + i) * BP + b0e + (le & 15);
      dst[0] = jacc[r][u] + jacc[r][8 + u];
      dst[16] = jacc[r][4 + u] + jacc[r][12 + u];
    }
#pragma unroll
  for (int r = 0; r < 3; ++r) {          // joint 16: the two lane halves hold the partial sums over their rows
    const float t = j16[r] + __shfl_xor(j16[r], 32);
    if (le < 32) JP[((size_t)(vc * 3 + r) * NH + 16) * BP + b0e + (le & 31)] = t;
  }
  if (probe && blockIdx.x == 0 && wv == 0 && le == 0) {
    probe[0] = clock64() - probe_t0;                 // shader clocks this wave was resident
    probe[1] = (long long)(t_end - t_begin) * (SPARSE ? (KF / 2) * 3 + 3 * 2 * KJS + 3 * 16 : LBS_FWD_MFMA_PER_TILE) + n_extra * 3 * 2 * KJS;   // MFMA instructions it issued
    probe[2] = wall_clock64() - probe_w0;            // the same interval on the constant 100 MHz counter
  }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
int launch_lbs_fwd(const Model& m, const float* Jn_vi, const float* FT, const float* AT, float* VPb, float* JP,
                   float* verts, int B, int BP, int nvc, hipStream_t s, long long* probe, const int* vmask, const int* tl, int ntl,
                   int verts_pose_major) {
  dim3 grid((BP / BG) * nvc), block(256);
  if (tl && !(m.kjs && VPb)) { jrr_set_error("lbs_fwd: the tile list serves the joint-sparse kernels with v_posed kept"); return JRR_ERR_ARG; }
  // exactly one round of two workgroups per CU, an even number of chunks and whole pose groups per XCD
  constexpr int fwd_split = 593;   // 16 : 11 tiles at B = 4096 (re-swept late in round 4: 0.3613 ms against 0.3633 at 15 : 12 and 0.3630 at 17 : 10)
  const int paired = pairs_one_round(BP / BG, nvc) ? fwd_split : 0;
  // SVP / SVT: v_posed / the vertices leave the chip; LIST: the listed tiles only (all of them keep v_posed; with `verts`, their
  // vertices -- joint-sparse classes only: no dense LIST kernel is built)
  auto launch = [&](auto SVP, auto SVT, auto LIST) {
    with_skin_class(m.kjs, m.wide_tiles, [&](auto KJ, auto WD) {
      constexpr int kj = decltype(KJ)::value;
      constexpr bool list = decltype(LIST)::value;
      if constexpr (kj > 0 || !list)
        hipLaunchKernelGGL((k_lbs_fwd<decltype(SVP)::value, decltype(SVT)::value, kj, decltype(WD)::value, list>), grid, block, 0, s, m.Dk,
                           kj ? m.Wc : m.Wjv, Jn_vi, FT, AT, VPb, JP, verts, B, BP, nvc, probe, paired, m.jl, m.tnj,
                           (verts && !list) ? vmask : nullptr, list ? tl : nullptr, list ? ntl : 0, verts_pose_major);
    });
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (tl) { if (verts) launch(yes, yes, yes); else launch(yes, no, yes); }
  else if (VPb && verts) launch(yes, yes, no);
  else if (VPb) launch(yes, no, no);
  else if (verts) launch(no, yes, no);
  else launch(no, no, no);
  return 0;
}

}  // namespace jrr
