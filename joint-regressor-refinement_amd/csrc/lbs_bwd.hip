// The adjoint of the skinning forward (lbs_fwd.hip): to v_posed and to the skinning transforms.  Two kernels -- the role kernel
// k_lbs_bwd and, for the joint-sparse models, the symmetric k_lbs_bwd16 --, the static parts of their per-tile operand records
// (k_bwd_tab_static; the regressor's part is written by jreg.hip), and the two layout kernels between the row quads and the
// caller's (B,6890,3) vertices.  Record layout, LDS-DMA copies, workgroup pairing: lbs_tile.h.
#include "jrr_common.h"
#include "kernels.h"
#include "lbs_tile.h"

namespace jrr {

// ------------------------------------------------------------------------------------------
// backward (to v_posed and to the skinning transforms)
//   one workgroup of four waves per (pose tile bt of 32 poses, vertex chunk vc); per vertex tile:
//     dverts_r[v,b] = sum_i Jn[i,v] dj[b,i,r]                (K = 18)        -- and / or loaded (DV, row quads)
//     T_{r,c}[v,b]  = sum_j W[v,j] A[b,j,r,c]                (K = 24, recomputed)
//     dvp_c[v,b]    = sum_r T_{r,c} dverts_r                  -> DVP [3][VP/4][BP][4] (row quads)
//     dA_{r,c}[j,b] += sum_v W[v,j] dverts_r[v,b] vp_c[v,b]   (sums over the tile's ROW index)
//     dA_{c,3}[j,b] += sum_v W[v,j] dverts_c[v,b]
//   Wave roles.  Waves 0..2 are the PLANE waves c = 0, 1, 2: T_{r,c} for the three r (36 MFMA), dvp_c, dA_{r,c} for the
//   three r (48 MFMA) -- they need the vertex adjoint dverts_r of all three r.  Wave 3 is the VERTEX-ADJOINT wave: it
//   computes dverts_r once per tile for the whole workgroup (27 MFMA; each plane wave used to recompute all of it),
//   hands the three tiles to the plane waves through LDS (48 floats per lane, 16-byte pieces, conflict-free), and
//   takes the translation column dA_{c,3} of all three c off them (48 MFMA; it only needs dverts).  84 : 84 : 84 : 75
//   MFMA per tile instead of 4 x 127 per 4/3 tiles.  The vertex-adjoint wave runs ONE TILE AHEAD of the plane waves:
//   while they work on tile t it computes dverts (and dA_{.,3}) of tile t + 1, so the hand-off costs two short barriers
//   per tile (tile published / tile consumed) and no waiting on MFMA work.  The per-tile operand records `Tb` = [Jn 18x32 | W^T 24x32 | W 32x32(j) | pad] (10 KB) ride a 3-deep
//   LDS-DMA ring (tile t for the plane waves, t + 1 for wave 3, t + 2 in flight); each plane wave keeps its slice of
//   A^T (36 operand vectors) in LDS for the whole kernel and register-prefetches its v_posed tile one tile ahead.
//   outputs: DVP, dATp [nvc][12][24][BP] partials.
// ------------------------------------------------------------------------------------------
// DV: 0 = vertex adjoint from the joint adjoint dJT (Jn^T dj), 1 = loaded from dVT, 2 = both (sum)
constexpr int BWD_RING = 3;
constexpr int DVBUF_FLOATS = 3 * 16 * 64;        // three 32x32 tiles as [r][register quad][lane][4]
// KJ > 0 (Model::kjs): T_{r,c} is recomputed over the tile's own <= KJ joints only (the record's W^T block then
// holds the KJ compacted rows, written by k_bwd_tab_static): with KJ = 8, 12 instead of 36 MFMA per plane wave and tile.
template <int DV, int KJ>
__global__ __launch_bounds__(256, 2) void k_lbs_bwd(const float* __restrict__ Tb, const float* __restrict__ AT,
                                                    const float* __restrict__ VPb, const float* __restrict__ dJT,
                                                    const float* __restrict__ dVT, float* __restrict__ DVP,
                                                    float* __restrict__ dATp, int BP, int nvc, int n_bt,
                                                    const int* __restrict__ jl, const int* __restrict__ segid,
                                                    const int* __restrict__ segj) {
  constexpr bool SPARSE = KJ > 0;
  constexpr int KJS = SPARSE ? KJ : 8;
  __shared__ __attribute__((aligned(16))) float lds[BWD_RING * TB_FLOATS + DVBUF_FLOATS + 3 * 36 * 64 + 27 * 64];
  float* const ring = lds;
  f32x4* const dvbuf = reinterpret_cast<f32x4*>(lds + BWD_RING * TB_FLOATS);
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const bool plane = wv < 3;
  const int c = wv;                                   // coordinate plane of a plane wave
  float* const ldsA = lds + BWD_RING * TB_FLOATS + DVBUF_FLOATS + (plane ? wv : 0) * 36 * 64;
  float* const ldsDj = lds + BWD_RING * TB_FLOATS + DVBUF_FLOATS + 3 * 36 * 64;   // wave 3: dj operands [r * 9 + ip][lane]
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int vc = L / n_bt, bt = L % n_bt;
  // (a 5 : 4 split of chunk pairs between the two workgroups of a CU, which gains 6 % in k_lbs_fwd, measured equal here)
  const int t_begin = (int)((long)VT * vc / nvc), t_end = (int)((long)VT * (vc + 1) / nvc);
  const int b0 = bt * BT;
  const size_t bcol = (size_t)b0 + l31;
  const unsigned lane_ln = (unsigned)lane * 4u;

  auto issue = [&](int vt, int slot) {
    const float* src = Tb + (size_t)vt * TB_FLOATS;
    float* dst = ring + slot * TB_FLOATS;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int o = wv + 4 * i;
      if (o < (SPARSE ? TB_PIECES_SPARSE : TB_FLOATS / 256)) dma16u(src + o * 256, lane_ln, dst + o * 256);
    }
  };
  // The two roles are two separate code paths (each with its own accumulators: the register allocation is the larger
  // of the two, not their union); both execute the same barrier sequence: one __syncthreads, then two per tile.
  issue(t_begin, 0);
  if (t_begin + 1 < t_end) issue(t_begin + 1, 1);

  if (plane) {
    // ================= plane wave c: T_{r,c}, dvp_c, dA_{r,c} (joint-sparse: + dA_{c,3}) =================
    f32x16 acc3[3] = {zero16(), zero16(), zero16()};
    // joint-sparse: the four products (0,c), (1,c), (2,c), (c,3) over the segment's 16-row joint window, as block
    // accumulators of v_mfma_f32_16x16x1_4b_f32 (blocks 0 + 2 = pose columns 0..15, blocks 1 + 3 = 16..31)
    f32x16 acc4 = zero16();
    int cur_seg = SPARSE ? segid[t_begin] : 0;
    int seg_tile = t_begin;                  // a tile of the open segment (its window is segj[seg_tile])
    unsigned seen = 0u;                      // joints whose slab rows this wave has written
    // close a segment: add its accumulators into this workgroup's dA slab (first touch of a joint stores, later ones add;
    // the slab rows belong to this wave alone) and start the next one
    auto flush_window = [&]() {
      if constexpr (SPARSE) {
        if (seen != 0u) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // earlier slab stores of this wave have landed (first flush: nothing to re-read)
        const int* sj = segj + seg_tile * 16;
        const int col = b0 + (lane & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = sj[4 * (lane >> 4) + i];
          if (j >= 0) {
            const bool add = (seen >> j) & 1u;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
              const f32x16& a = p == 0 ? acc3[0] : p == 1 ? acc3[1] : p == 2 ? acc3[2] : acc4;
              const int e = p < 3 ? p * 4 + c : c * 4 + 3;
              float* dst = dATp + ((size_t)(vc * 12 + e) * NJ + j) * BP + col;
              float lo = a[i] + a[8 + i], hi = a[4 + i] + a[12 + i];
              if (add) {      // agent-scope loads (L1 bypassed): what an earlier flush of this wave stored, whichever lane stored it
                lo += __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                hi += __hip_atomic_load(dst + 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              }
              // agent-scope stores: a later flush of this wave re-reads them (possibly from another lane) with agent-scope loads
              __hip_atomic_store(dst, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              __hip_atomic_store(dst + 16, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          }
        }
#pragma unroll
        for (int n = 0; n < 16; ++n) {
          const int j = sj[n];                                       // wave-uniform
          if (j >= 0) seen |= 1u << j;
        }
        acc3[0] = zero16(); acc3[1] = zero16(); acc3[2] = zero16(); acc4 = zero16();
      }
    };
    // this wave's A^T operand vectors (r, j-pair) -> LDS, once
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int jp = 0; jp < 12; ++jp)
        ldsA[(r * 12 + jp) * 64 + lane] = AT[(size_t)((r * 4 + c) * NJ + 2 * jp + half) * BP + bcol];
    const unsigned qoff = (unsigned)half * (unsigned)BP + (unsigned)bcol;     // lane part of a (row quad, pose) address
    auto load_vp = [&](int vt, f32x16& dstv) {      // four 16-byte row quads (jrr_common.h)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 t = *quad_ptr(VPb, (size_t)c * (VP / 4) + vt * 8, g, BP, qoff);
        dstv[4 * g] = t[0]; dstv[4 * g + 1] = t[1]; dstv[4 * g + 2] = t[2]; dstv[4 * g + 3] = t[3];
      }
    };
    f32x16 vpA = zero16(), vpB = zero16();            // v_posed tiles, ping-pong: the next tile's loads fly for a whole tile
    load_vp(t_begin, vpA);
    __syncthreads();                                  // records of the first two tiles landed
    int slot = 0;                                     // ring slot of tile vt
    auto tile = [&](int vt, const f32x16& vpc, f32x16& vpn) {
      // dverts of tile vt published; record vt + 1 landed; everybody is done with tile vt - 1.  This wave's record
      // copies are older than its 4 v_posed prefetch loads and its 4 dvp stores of the previous tile: both stay in
      // flight across the barrier (the prefetch is consumed in the second half of THIS tile, the stores never).
      barrier_keep_vm<8>();
      const int slot1 = (slot + 1 == BWD_RING) ? 0 : slot + 1, slot2 = (slot1 + 1 == BWD_RING) ? 0 : slot1 + 1;
      if (vt + 2 < t_end) issue(vt + 2, slot2);
      __builtin_amdgcn_sched_barrier(0);     // the counted wait relies on: record copies first, loads / stores after
      const float* tab = ring + slot * TB_FLOATS;
      f32x16 dv[3];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 t = dvbuf[(r * 4 + g) * 64 + lane];
          dv[r][4 * g] = t[0]; dv[r][4 * g + 1] = t[1]; dv[r][4 * g + 2] = t[2]; dv[r][4 * g + 3] = t[3];
        }
      if (vt + 1 < t_end) load_vp(vt + 1, vpn);
      // every plane wave holds dverts of tile vt in registers: the buffer may take tile vt + 1 (short barrier: the
      // plane waves reach it right after their 12 LDS reads, wave 3 at once)
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      // T_{r,c} for the three r as three interleaved accumulator chains sharing the W operand; operands of joint pair
      // jp + 1 are requested right after the first MFMA of pair jp (a wave never parks on lgkmcnt between products)
      f32x16 T0 = zero16(), T1 = zero16(), T2 = zero16();
      if constexpr (SPARSE) {
        // operand of joint j for this lane half: ldsA[(r * 12 + j / 2) * 64 + (j % 2) * 32 + l31] = ldsA[r * 768 + 32 j + l31]
        const float* wp = tab + TB_WJV + half * 32 + l31;
        float w[KJS / 2], a0[KJS / 2], a1[KJS / 2], a2[KJS / 2];
#pragma unroll
        for (int pq = 0; pq < KJS / 2; ++pq) {
          const int j0 = jl[vt * NJ + 2 * pq], j1 = jl[vt * NJ + 2 * pq + 1];            // wave-uniform: scalar loads
          const float* ap = ldsA + (half ? j1 : j0) * 32 + l31;
          w[pq] = wp[2 * pq * 32]; a0[pq] = ap[0]; a1[pq] = ap[12 * 64]; a2[pq] = ap[24 * 64];
        }
#pragma unroll
        for (int pq = 0; pq < KJS / 2; ++pq) {
          T0 = mfma(w[pq], a0[pq], T0);
          T1 = mfma(w[pq], a1[pq], T1);
          T2 = mfma(w[pq], a2[pq], T2);
        }
      } else {
        const float* wp = tab + TB_WJV + half * 32 + l31;
        const float* ap = ldsA + lane;
        float w = wp[0], a0 = ap[0], a1 = ap[12 * 64], a2 = ap[24 * 64];
#pragma unroll
        for (int jp = 0; jp < 12; ++jp) {
          const float wc = w, c0 = a0, c1 = a1, c2 = a2;
          __builtin_amdgcn_sched_barrier(0);
          T0 = mfma(wc, c0, T0);
          __builtin_amdgcn_sched_barrier(0);
          if (jp + 1 < 12) {
            w = wp[(2 * jp + 2) * 32];
            a0 = ap[(jp + 1) * 64]; a1 = ap[(12 + jp + 1) * 64]; a2 = ap[(24 + jp + 1) * 64];
          }
          __builtin_amdgcn_sched_barrier(0);
          T1 = mfma(wc, c1, T1);
          T2 = mfma(wc, c2, T2);
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {                      // dvp_c = sum_r T_{r,c} dverts_r, stored as 16-byte row quads
        f32x4 t;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int q = 4 * g + u;
          t[u] = fmaf(T2[q], dv[2][q], fmaf(T1[q], dv[1][q], T0[q] * dv[0][q]));
        }
        *quad_ptr(DVP, (size_t)c * (VP / 4) + vt * 8, g, BP, qoff) = t;
      }
      if constexpr (SPARSE) {
        // dA over the segment's 16-row joint window.  A operand: W16[n = lane % 16][v = acc_row(q, half)], four 16-byte
        // reads per tile (rows padded to 36 floats: conflict-free); B operand: this lane's register q of the accumulator
        // layout; one 4-block instruction adds rows acc_row(q, 0) and acc_row(q, 1) for all 32 pose columns.
        const int sg = segid[vt];                                    // wave-uniform
        if (sg != cur_seg) { flush_window(); cur_seg = sg; }
        seg_tile = vt;
        const f32x4* w16 = reinterpret_cast<const f32x4*>(tab + TB_WVJ + (lane & 15) * 36 + 4 * half);
        f32x4 wq[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) wq[g] = w16[2 * g];
        const f32x16& dvc = c == 0 ? dv[0] : c == 1 ? dv[1] : dv[2];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float wvj = wq[q >> 2][q & 3];
          const float p0 = dv[0][q] * vpc[q], p1 = dv[1][q] * vpc[q], p2 = dv[2][q] * vpc[q];
          acc3[0] = mfma16(wvj, p0, acc3[0]);
          acc3[1] = mfma16(wvj, p1, acc3[1]);
          acc3[2] = mfma16(wvj, p2, acc3[2]);
          acc4 = mfma16(wvj, dvc[q], acc4);
        }
      } else {
        const float* wvp = tab + TB_WVJ + l31;
        float wn = wvp[acc_row(0, half) * 32];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float wvj = wn;
          const float p0 = dv[0][q] * vpc[q], p1 = dv[1][q] * vpc[q], p2 = dv[2][q] * vpc[q];
          __builtin_amdgcn_sched_barrier(0);
          acc3[0] = mfma(wvj, p0, acc3[0]);
          __builtin_amdgcn_sched_barrier(0);
          if (q + 1 < 16) wn = wvp[acc_row(q + 1, half) * 32];
          __builtin_amdgcn_sched_barrier(0);
          acc3[1] = mfma(wvj, p1, acc3[1]);
          acc3[2] = mfma(wvj, p2, acc3[2]);
        }
      }
      slot = slot1;
    };
    for (int vt = t_begin; vt < t_end; vt += 2) {
      tile(vt, vpA, vpB);
      if (vt + 1 < t_end) tile(vt + 1, vpB, vpA);
    }
    if constexpr (SPARSE) {
      flush_window();
      // joints no tile of this chunk touches: their slab rows are zero
#pragma unroll 1
      for (int j = 0; j < NJ; ++j) {
        if ((seen >> j) & 1u) continue;
        if (lane < 32) {
#pragma unroll
          for (int p = 0; p < 4; ++p) dATp[((size_t)(vc * 12 + (p < 3 ? p * 4 + c : c * 4 + 3)) * NJ + j) * BP + bcol] = 0.f;
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int j = acc_row(q, half);
        if (j < NJ) {
#pragma unroll
          for (int r = 0; r < 3; ++r) dATp[((size_t)(vc * 12 + r * 4 + c) * NJ + j) * BP + bcol] = acc3[r][q];
        }
      }
    }
  } else {
    // ================= wave 3: dverts of the next tile for everybody, dA_{r,3} =================
    f32x16 acc3[3] = {zero16(), zero16(), zero16()};
    f32x16 dv[3];
    const unsigned qoffh = (unsigned)half * (unsigned)BP + (unsigned)bcol;    // lane part of a (row quad, pose) address
    // vertex adjoint of tile vt: Jn^T dj on the matrix cores and / or the caller's adjoint from memory
    auto compute_dv = [&](int vt, const float* tab) {
      if (DV != 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 t = *quad_ptr(dVT, (size_t)r * (VP / 4) + vt * 8, g, BP, qoffh);
            dv[r][4 * g] = t[0]; dv[r][4 * g + 1] = t[1]; dv[r][4 * g + 2] = t[2]; dv[r][4 * g + 3] = t[3];
          }
      } else {
        dv[0] = zero16(); dv[1] = zero16(); dv[2] = zero16();
      }
      if (DV != 1) {
        const float* jp_ = tab + TB_JN + half * 32 + l31;
        const float* dp_ = ldsDj + lane;
        float jn = jp_[0], d0 = dp_[0], d1 = dp_[9 * 64], d2 = dp_[18 * 64];
#pragma unroll
        for (int ip = 0; ip < 9; ++ip) {
          const float jc = jn, c0 = d0, c1 = d1, c2 = d2;
          __builtin_amdgcn_sched_barrier(0);
          dv[0] = mfma(jc, c0, dv[0]);
          __builtin_amdgcn_sched_barrier(0);
          if (ip + 1 < 9) {
            jn = jp_[(2 * ip + 2) * 32];
            d0 = dp_[(ip + 1) * 64]; d1 = dp_[(9 + ip + 1) * 64]; d2 = dp_[(18 + ip + 1) * 64];
          }
          __builtin_amdgcn_sched_barrier(0);
          dv[1] = mfma(jc, c1, dv[1]);
          dv[2] = mfma(jc, c2, dv[2]);
        }
      }
    };
    auto publish_dv = [&]() {
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 t = {dv[r][4 * g], dv[r][4 * g + 1], dv[r][4 * g + 2], dv[r][4 * g + 3]};
          dvbuf[(r * 4 + g) * 64 + lane] = t;
        }
    };
    // dA_{r,3}[j,b] += sum_v W[v,j] dverts_r[v,b]
    auto accumulate_dA3 = [&](const float* tab) {
      const float* wvp = tab + TB_WVJ + l31;
      float wn = wvp[acc_row(0, half) * 32];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float wvj = wn;
        __builtin_amdgcn_sched_barrier(0);
        acc3[0] = mfma(wvj, dv[0][q], acc3[0]);
        __builtin_amdgcn_sched_barrier(0);
        if (q + 1 < 16) wn = wvp[acc_row(q + 1, half) * 32];
        __builtin_amdgcn_sched_barrier(0);
        acc3[1] = mfma(wvj, dv[1][q], acc3[1]);
        acc3[2] = mfma(wvj, dv[2][q], acc3[2]);
      }
    };
    if (DV != 1) {
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int ip = 0; ip < 9; ++ip) ldsDj[(r * 9 + ip) * 64 + lane] = dJT[(size_t)(r * NHP + 2 * ip + half) * BP + bcol];
    }
    __syncthreads();                                  // records of the first two tiles landed
    compute_dv(t_begin, ring);
    publish_dv();
    if constexpr (!SPARSE) accumulate_dA3(ring);      // joint-sparse: the plane waves take dA_{c,3} (16-row products)
    int slot = 0;
    for (int vt = t_begin; vt < t_end; ++vt) {
      barrier_keep_vm<0>();                           // nothing younger than this wave's record copies is in flight
      const int slot1 = (slot + 1 == BWD_RING) ? 0 : slot + 1, slot2 = (slot1 + 1 == BWD_RING) ? 0 : slot1 + 1;
      if (vt + 2 < t_end) issue(vt + 2, slot2);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (vt + 1 < t_end) {      // this wave's whole tile (27 + 48 MFMA) runs beside the plane waves' 84
        compute_dv(vt + 1, ring + slot1 * TB_FLOATS);
        publish_dv();
        if constexpr (!SPARSE) accumulate_dA3(ring + slot1 * TB_FLOATS);
      }
      slot = slot1;
    }
    if constexpr (!SPARSE) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int j = acc_row(q, half);
        if (j < NJ) {
#pragma unroll
          for (int r = 0; r < 3; ++r) dATp[((size_t)(vc * 12 + r * 4 + 3) * NJ + j) * BP + bcol] = acc3[r][q];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// backward, joint-sparse models: FOUR SYMMETRIC WAVES, each alone with 16 poses
//   The role kernel above splits a 32-pose tile over three plane waves and a vertex-adjoint wave: one wave is always late,
//   and two barriers per tile tie the four together.  With 16x16 matrix tiles (v_mfma_f32_16x16x4_f32, the same FLOP per clock
//   as 32x32x2) a (32 vertices x 16 poses) tile is 8 registers instead of 16 per lane, the twelve dA accumulators of a
//   16-row joint window are 48 registers instead of 192 -- and ONE wave can hold everything for its own 16 poses: vertex
//   adjoint, T recompute, dvp, all twelve dA products.  No roles, no hand-off through LDS, no imbalance; the four waves of a
//   workgroup (64 poses) only share the per-tile operand records (LDS-DMA ring, ONE barrier per tile).
//   16x16x4:  A: lane l holds A[m = l % 16][k = l / 16]   B: lane l holds B[k = l / 16][n = l % 16]
//             D: register i of lane l holds D[row 4 (l / 16) + i][col l % 16]
//   so register i of a lane group g = l / 16 is vertex row 16 blk + 4 g + i of its pose column: four consecutive rows = one
//   16-byte row quad of VPb / DVP (one dwordx4 per (plane, blk)), and -- as the B operand of a product that sums over the
//   tile's rows -- K index g of the step (blk, i), whose A operand therefore is W16[n][16 blk + 4 g + i].
//   Record R16 of a tile (k_jreg_tiles / k_bwd_tab_static write it in place of the role kernel's):
//     JN [blk][s < 5][64 lanes]   Jn[i = 4 s + g][16 blk + m]            A operands of dverts  (i >= 17: 0)
//     WT [blk][s < 3][64 lanes]   W[16 blk + m][joint slot 4 s + g]       A operands of T       (slots >= KJ: 0)
//     WD [blk][g][n][4]           W16[n][16 blk + 4 g + 0..3]             A operands of dA, one ds_read_b128 per blk
//     JL [16]                     16 * joint of slot k (ints)              row offsets into the wave's A^T slice
//     WX [blk][64 lanes]          K step 3 of WT (joint slots 12 .. 15)   a WIDE tile's T recompute runs ceil(joints / 4) K steps:
//   the kernel is built for S = KJ / 4 of them; a tile with more joints (tnj[vt] > KJ, at most 16) runs the extra steps in a
//   rare wave-uniform branch -- it costs itself, nobody else.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

template <int DV, int KJ, bool WIDE, bool LIST = false>      // WIDE, LIST: as in k_lbs_fwd (WIDE: 0.184 vs 0.187 ms)
__global__ __launch_bounds__(256, 2) void k_lbs_bwd16(const float* __restrict__ Tb, const float* __restrict__ AT,
                                                      const float* __restrict__ VPb, const float* __restrict__ dJT,
                                                      const float* __restrict__ dVT, float* __restrict__ DVP,
                                                      float* __restrict__ dATp, int BP, int nvc, int n_bt,
                                                      const int* __restrict__ segid, const int* __restrict__ segj, int paired,
                                                      const int* __restrict__ tnj, const int* __restrict__ tl, int ntl,
                                                      unsigned* __restrict__ dmask) {
  // dmask (nullable): [chunk][64-pose group] bit j = this workgroup wrote the rows of joint j of its dA slab.  The rows of the joints
  // no tile of the chunk touches are then NOT zero-filled (and not read: k_chain_bwd takes the mask) -- at 4096 poses the eight slabs
  // are 37.7 MB, about half of it rows of zeros (timing-only ablation of flush + fill: 18 us of the launch).
  // LIST: the ntl tiles tl[] only.  A tile without a support entry of the regressor has a zero vertex adjoint (DV == 0: no adjoint
  // from outside): its dvp and its dA contributions are exact zeros, and the blend adjoint skips its rows of DVP as well.
  const int NT = LIST ? ntl : VT;
  constexpr int S = KJ / 4;                          // K steps of the T product (4 joint slots each)
  constexpr int ASL = 9 * NJ * 16;                   // floats of one wave's A^T slice [(r,c)][24 joints][16 poses]
  __shared__ __attribute__((aligned(16))) float lds[BWD_RING * R16_FLOATS + 4 * ASL];
  float* const ring = lds;
  const int tid = threadIdx.x;
  const int lane = tid & 63, n = lane & 15, g = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* const ldsA = lds + BWD_RING * R16_FLOATS + wv * ASL;
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  // default mapping: an XCD's contiguous range of L = one vertex chunk x all pose groups (chunk-major inside a pose group instead
  // was measured equal or slower: 0.200 vs 0.203 ms at B = 4096, 0.069 vs 0.066 ms at B = 1024)
  int vc = L / n_bt, bt = L % n_bt;
  int t_begin = (int)((long)NT * vc / nvc), t_end = (int)((long)NT * (vc + 1) / nvc);
  if (paired > 0) {
    // Exactly one round of two workgroups per CU (k_lbs_fwd's geometry, see there): the two workgroups of a CU -- dispatch
    // slots j and j + per_xcd / 2 of an XCD -- take the two halves of a PAIR of vertex chunks of the SAME pose group.
    // Measured (B = 4096): 0.204 -> 0.184 ms; what matters is that the two share the pose group (the chunk-major mapping
    // without pairing gains nothing), the split itself is flat around even: `paired` = the first-dispatched workgroup's
    // share of the pair's tiles in thousandths (launcher default).  Static: bitwise reproducible.
    pair_chunks(paired, NT, nvc, bt, vc, t_begin, t_end);
  }
  const size_t bcol = (size_t)bt * 64 + wv * 16 + n;          // this lane's pose column
  const unsigned lane_ln = (unsigned)lane * 4u;

  auto issue = [&](int vt, int slot) {
    const float* src = Tb + (size_t)vt * TB_FLOATS;
    float* dst = ring + slot * R16_FLOATS;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int o = wv + 4 * i;
      if (o < R16_PIECES) dma16u(src + o * 256, lane_ln, dst + o * 256);
    }
  };
  auto tile_of = [&](int ix) { return LIST ? tl[ix] : ix; };      // wave-uniform (scalar load)
  if (t_begin < t_end) issue(tile_of(t_begin), 0);
  if (t_begin + 1 < t_end) issue(tile_of(t_begin + 1), 1);

  // this wave's A^T slice (the 3x3 rotation part; the translation column is not needed for T) -> LDS, once
#pragma unroll
  for (int rc = 0; rc < 9; ++rc)
#pragma unroll
    for (int jj = 0; jj < NJ / 4; ++jj) {
      const int j = 4 * jj + g;
      ldsA[(rc * NJ + j) * 16 + n] = AT[(size_t)(((rc / 3) * 4 + rc % 3) * NJ + j) * BP + bcol];
    }
  // joint adjoint as B operands of the vertex-adjoint product: dj[r][s] = dJ^T[r][i = 4 s + g][pose]
  float dj[3][5];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s5 = 0; s5 < 5; ++s5) {
      const int i = 4 * s5 + g;
      dj[r][s5] = (DV != 1 && i < NHP) ? dJT[(size_t)(r * NHP + i) * BP + bcol] : 0.f;
    }

  // row quad (plane, tile, blk) of this lane: rows 32 vt + 16 blk + 4 g + 0..3 of its pose
  auto qidx = [&](int plane, int vt, int blk) { return ((size_t)plane * (VP / 4) + vt * 8 + 4 * blk + g) * BP + bcol; };
  f32x4* const DVP4 = reinterpret_cast<f32x4*>(DVP);
  // The six row quads of a tile (v_posed, or the caller's vertex adjoint) go out from inline asm and are waited for by hand with a
  // COUNTED vmcnt (jrr_common.h, quad_load / quads_landed): six vector-memory operations, in this order, behind whatever precedes
  // the call.  The wave-uniform part of the address (plane, tile, blk) is the scalar base, the lane's part a 32-bit byte offset.
  const unsigned quad_lane = (unsigned)(((size_t)g * BP + bcol) * 16);
  auto load_quads = [&](const float* src, int vt, f32x4 (&dst)[3][2], auto nt) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
        quad_load<decltype(nt)::value>(dst[c][blk], quad_lane, src + ((size_t)c * (VP / 4) + vt * 8 + 4 * blk) * BP * 4);
  };
  // v_posed is read once: nt, it must not displace the operands in L2
  auto load_vp = [&](int vt, f32x4 (&dst)[3][2]) __attribute__((always_inline)) { load_quads(VPb, vt, dst, std::true_type{}); };

  f32x4 acc[12];                                   // dA_{r,c} at 3 r + c (c < 3), dA_{r,3} at 9 + r: 16 window rows x 16 poses
#pragma unroll
  for (int e = 0; e < 12; ++e) acc[e] = zero4();
  int cur_seg = (t_begin < t_end) ? segid[tile_of(t_begin)] : 0;
  int seg_tile = (t_begin < t_end) ? tile_of(t_begin) : 0;
  unsigned seen = 0u;
  // close a segment: add the accumulators into this workgroup's dA slab (first touch of a joint stores, later ones add;
  // the 16 pose columns belong to this wave alone)
  auto flush_window = [&]() __attribute__((always_inline)) {
    // a later flush re-reads slab rows an earlier one stored: those stores must have landed.  The FIRST flush of a workgroup (seen == 0,
    // wave-uniform: most workgroups lie inside one segment and flush once, at the end) reads nothing and need not wait for the tile's
    // last dvp stores
    if (seen != 0u) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int* sj = segj + seg_tile * 16;
    // rows an earlier flush of this workgroup stored are read back FIRST, all of them in flight together (one agent-scope load per
    // row and entry: issued one by one between the stores they feed, 48 dependent L2 round trips made the flush the largest fixed
    // cost of the launch), then everything is stored
    int jr[4];
    float* rowp[4];
    float oldv[4][12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      jr[i] = sj[4 * g + i];
      rowp[i] = dATp + ((size_t)(vc * 12) * NJ + (jr[i] >= 0 ? jr[i] : 0)) * BP + bcol;
      const bool add = jr[i] >= 0 && ((seen >> jr[i]) & 1u);
#pragma unroll
      for (int e = 0; e < 12; ++e) {
        const int ent = e < 9 ? (e / 3) * 4 + e % 3 : (e - 9) * 4 + 3;
        // L1 bypassed: an earlier flush of this wave stored it, possibly from another lane
        oldv[i][e] = add ? __hip_atomic_load(rowp[i] + (size_t)ent * NJ * BP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
      }
    }
    // every read-back retires inside the flush, on every path (a row of a joint the window does not hold is loaded by no lane and
    // stored by none): a load still pending where the flush joins the tile again costs the tile loop a vmcnt(0) in front of the next
    // write of its register
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 12; ++e) asm volatile("" : "+v"(oldv[i][e]));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (jr[i] >= 0) {
        const bool add = (seen >> jr[i]) & 1u;
#pragma unroll
        for (int e = 0; e < 12; ++e) {
          const int ent = e < 9 ? (e / 3) * 4 + e % 3 : (e - 9) * 4 + 3;
          const float val = add ? acc[e][i] + oldv[i][e] : acc[e][i];
          __hip_atomic_store(rowp[i] + (size_t)ent * NJ * BP, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // paired with the agent-scope re-read of a later flush
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = zero4();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int j = sj[k];
      if (j >= 0) seen |= 1u << j;
    }
  };

  f32x4 vpA[3][2], vpB[3][2];
#pragma unroll
  for (int c = 0; c < 3; ++c) { vpA[c][0] = vpA[c][1] = zero4(); vpB[c][0] = vpB[c][1] = zero4(); }
  if (t_begin < t_end) load_vp(tile_of(t_begin), vpA);
  // Everything the prologue loaded is retired HERE, where the compiler's wait insertion sees it: a load it still holds pending at the
  // loop header cannot be counted inside the loop and costs a vmcnt(0) in front of its first reader in every tile.  The first tile
  // needs all of it anyway (the A^T slice already went through registers into LDS above).
  if (DV != 1) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s5 = 0; s5 < 5; ++s5) asm volatile("" : "+v"(dj[r][s5]));
  }
  quads_landed<0>(vpA);
  int slot = 0;
  // Vector-memory operations of one wave in issue order (ONE in-order counter for LDS-DMA, loads and stores); NA = 6 loads of the
  // caller's adjoint if DV != 0, else none:
  //   tile ix - 1:  barrier | DMA(ix + 1) x 0..2 | adjoint(ix - 1) x NA | v_posed(ix) x 6 | ... | dvp(ix - 1) x 6
  //   tile ix    :  barrier | DMA(ix + 2) x 0..2 | adjoint(ix) x NA     | v_posed(ix + 1) x 6 | ...
  //       wait for adjoint(ix): 6 younger                    (in front of the vertex-adjoint products)
  //       wait for v_posed(ix): 6 + NA + 6 younger, + DMA    (in front of the dA products of plane 0)
  //   ... | dvp(ix) x 6
  // The prefetch is UNCONDITIONAL -- the last tile of a chunk loads itself again and nobody reads the result -- so both counts hold
  // on every path without a branch around a wait.  The DMA pieces (wave 3 copies one fewer, the last two tiles none) and a
  // flush (rare) only add operations younger than v_posed(ix); the count leaves them out, which in the steady state asks for the
  // first two dvp stores of the previous tile, a whole tile old, as well.
  constexpr int NA = (DV != 0) ? 6 : 0;
  auto tile = [&](int ix, f32x4 (&vpc)[3][2], f32x4 (&vpn)[3][2]) __attribute__((always_inline)) {
    const int vt = tile_of(ix);
    // record vt has landed (it was issued two tiles ago: older than the 6 prefetch loads and the 6 dvp stores of the previous
    // tile, which stay in flight) and every wave is done with the slot the next copy overwrites
    barrier_keep_vm<12>();
    const int slot1 = (slot + 1 == BWD_RING) ? 0 : slot + 1, slot2 = (slot1 + 1 == BWD_RING) ? 0 : slot1 + 1;
    if (ix + 2 < t_end) issue(tile_of(ix + 2), slot2);
    __builtin_amdgcn_sched_barrier(0);
    const float* tab = ring + slot * R16_FLOATS;
    // ---- vertex adjoint of the tile: dverts_r = Jn^T dj_r and / or the caller's ----
    f32x4 dv[3][2];
#pragma unroll
    for (int r = 0; r < 3; ++r) dv[r][0] = dv[r][1] = zero4();
    if (DV != 0) load_quads(dVT, vt, dv, std::false_type{});
    load_vp(tile_of(ix + 1 < t_end ? ix + 1 : t_end - 1), vpn);
    if (DV != 0) quads_landed<6>(dv);      // all six in flight together, the v_posed prefetch behind them stays in flight
    if (DV != 1) {
#pragma unroll
      for (int s5 = 0; s5 < 5; ++s5)
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
          const float a = tab[R16_JN + (blk * 5 + s5) * 64 + lane];
#pragma unroll
          for (int r = 0; r < 3; ++r) dv[r][blk] = mfma4(a, dj[r][s5], dv[r][blk]);
        }
    }
    // ---- operands shared by the planes: W^T (A of T), W16 (A of dA), the A^T row offsets of the tile's joint slots ----
    float wt[2][S];
    int jo[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      jo[s] = reinterpret_cast<const int*>(tab + R16_JL)[4 * s + g];
#pragma unroll
      for (int blk = 0; blk < 2; ++blk) wt[blk][s] = tab[R16_WT + (blk * 3 + s) * 64 + lane];
    }
    f32x4 wd[2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) wd[blk] = *reinterpret_cast<const f32x4*>(tab + R16_WD + ((blk * 4 + g) * 16 + n) * 4);
    const int sg = segid[vt];                                      // wave-uniform
    const int s_tile = WIDE ? (tnj[vt] + 3) >> 2 : 0;              // K steps this tile's joints need (wave-uniform)
    if (sg != cur_seg) { flush_window(); cur_seg = sg; }
    seg_tile = vt;
    // ---- translation column: dA_{r,3} += W16^T dverts_r ----
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 3; ++r) acc[9 + r] = mfma4(wd[blk][i], dv[r][blk][i], acc[9 + r]);
    // ---- per plane c: T_{r,c} (recomputed), dvp_c = sum_r T_{r,c} dverts_r, dA_{r,c} += W16^T (dverts_r * vp_c) ----
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      f32x4 T[3][2];
#pragma unroll
      for (int r = 0; r < 3; ++r) { T[r][0] = zero4(); T[r][1] = zero4(); }
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const float at = ldsA[(r * 3 + c) * (NJ * 16) + jo[s] + n];
          T[r][0] = mfma4(wt[0][s], at, T[r][0]);
          T[r][1] = mfma4(wt[1][s], at, T[r][1]);
        }
      if (WIDE && s_tile > S) {                                     // WIDE tile: the K steps beyond the kernel's S (slots 4 S .. 15)
#pragma unroll 1
        for (int s = S; s < s_tile && s < 4; ++s) {
          const int jox = reinterpret_cast<const int*>(tab + R16_JL)[4 * s + g];
          const float w0 = s < 3 ? tab[R16_WT + (0 * 3 + s) * 64 + lane] : tab[R16_WX + lane];
          const float w1 = s < 3 ? tab[R16_WT + (1 * 3 + s) * 64 + lane] : tab[R16_WX + 64 + lane];
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const float at = ldsA[(r * 3 + c) * (NJ * 16) + jox + n];
            T[r][0] = mfma4(w0, at, T[r][0]);
            T[r][1] = mfma4(w1, at, T[r][1]);
          }
        }
      }
#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        f32x4 t;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          t[i] = fmaf(T[2][blk][i], dv[2][blk][i], fmaf(T[1][blk][i], dv[1][blk][i], T[0][blk][i] * dv[0][blk][i]));
        __builtin_nontemporal_store(t, &DVP4[qidx(c, vt, blk)]);      // streamed (340 MB per launch): nt, measured -2.5 us
      }
      if (c == 0) quads_landed<12 + NA>(vpc);      // first use of this tile's v_posed, loaded a tile ago
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 3; ++r) acc[3 * r + c] = mfma4(wd[blk][i], dv[r][blk][i] * vpc[c][blk][i], acc[3 * r + c]);
    }
    slot = slot1;
  };
  if (t_begin < t_end) {
    for (int ix = t_begin; ix < t_end; ix += 2) {
      tile(ix, vpA, vpB);
      if (ix + 1 < t_end) tile(ix + 1, vpB, vpA);
    }
    // the last tile's prefetch, which nobody reads, has to land before its registers go to other uses: only that tile's six dvp
    // stores are younger, and it is a whole tile old
    quads_landed<6>(vpA, vpB);
  }
  flush_window();
  if (dmask) {      // one word per (chunk, 64-pose group)
    if (tid == 0) dmask[vc * n_bt + bt] = seen;
    return;
  }
  // joints no tile of this chunk touches: zero rows
#pragma unroll 1
  for (int j = 0; j < NJ; ++j) {
    if ((seen >> j) & 1u) continue;
    if (lane < 16) {
#pragma unroll
      for (int ent = 0; ent < 12; ++ent) dATp[((size_t)(vc * 12 + ent) * NJ + j) * BP + bcol] = 0.f;
    }
  }
}

// static (W) parts of the per-tile backward operand records
// (Wc != NULL: the W^T block takes the kjs compacted rows of the joint-sparse path, zeros behind them)
__global__ void k_bwd_tab_static(const float* __restrict__ Wjv, const float* __restrict__ Wvj, float* __restrict__ Tb,
                                 const float* __restrict__ Wc, int kjs, const float* __restrict__ W16,
                                 const int* __restrict__ jl, int r16) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;   // over VT * 2048
  if (idx >= VT * 2048) return;
  const int vt = idx >> 11, k = idx & 2047;
  float* dst = Tb + (size_t)vt * TB_FLOATS;
  if (r16) {      // record R16 of k_lbs_bwd16 (everything but its JN block, which k_jreg_tiles writes)
    if (k >= R16_FLOATS - R16_WT) return;
    const int o = R16_WT + k;
    // joint slots: the NJ-slot tables of the model (Wc [VT][NJ][32], jl [VT][NJ]); 16 of them fit the record
    if (o < R16_WD) {               // WT [blk][s < 3][g][m] = W[16 blk + m][slot 4 s + g]
      const int q = o - R16_WT, blk = q / 192, s = (q / 64) % 3, g = (q >> 4) & 3, m = q & 15;
      const int slot = 4 * s + g;
      dst[o] = Wc[((size_t)vt * NJ + slot) * 32 + 16 * blk + m];
    } else if (o < R16_JL) {        // WD [blk][g][n][i] = W16[n][16 blk + 4 g + i]
      const int q = o - R16_WD, blk = q >> 8, g = (q >> 6) & 3, n = (q >> 2) & 15, i = q & 3;
      dst[o] = W16[(size_t)vt * TB_W16_FLOATS + n * 36 + 16 * blk + 4 * g + i];
    } else if (o < R16_WX) {        // JL [16]: 16 * joint of slot k (row offset into a wave's A^T slice), as an int
      const int q = o - R16_JL;
      reinterpret_cast<int*>(dst)[o] = 16 * jl[vt * NJ + q];
    } else if (o < R16_WX + 128) {  // WX [blk][g][m] = W[16 blk + m][slot 12 + g]: K step 3
      const int q = o - R16_WX, blk = q >> 6, g = (q >> 4) & 3, m = q & 15;
      dst[o] = Wc[((size_t)vt * NJ + 12 + g) * 32 + 16 * blk + m];
    } else dst[o] = 0.f;
    return;
  }
  if (k < W_FLOATS) dst[TB_WJV + k] = Wc ? (k < kjs * 32 ? Wc[(size_t)vt * W_FLOATS + k] : 0.f) : Wjv[(size_t)vt * W_FLOATS + k];
  else if (k < W_FLOATS + 1024) {
    const int kk = k - W_FLOATS;
    dst[TB_WVJ + kk] = Wc ? (kk < TB_W16_FLOATS ? W16[(size_t)vt * TB_W16_FLOATS + kk] : 0.f) : Wvj[(size_t)vt * 1024 + kk];
  }
  else if (k - W_FLOATS - 1024 < TB_FLOATS - TB_WVJ - 1024) dst[TB_WVJ + 1024 + (k - W_FLOATS - 1024)] = 0.f;
}

// [3][VP/4][BP][4] vertices (row quads) -> pose-major (B, ldv) rows of (v, xyz) and/or projected (x_ndc, y_ndc, Z, 0)
// records for the silhouette renderer (scripts/optimize.py:80-82 flip/scale + scripts/mesh_renderer.py:52-57 camera).
// One 32-vertex x 32-pose tile per block through LDS; every global access is contiguous (16 bytes per thread on the
// quad side).
// (p2v != NULL: row v of the buffer is vertex p2v[v] of the caller's mesh -- the store then is per vertex, 12 bytes)
__global__ void k_verts_untranspose(const float* __restrict__ VTb, float* __restrict__ verts, int ldv, int vlimit,
                                    const float* __restrict__ cam, f32x4* __restrict__ ndc, float focal, int B, int BP,
                                    const int* __restrict__ p2v) {
  __shared__ float tile[32][97];
  const int v0 = blockIdx.x * 32, bb0 = blockIdx.y * 32;
  const f32x4* VTq = reinterpret_cast<const f32x4*>(VTb);
  for (int idx = threadIdx.x; idx < 3 * 8 * 32; idx += blockDim.x) {
    const int r = idx >> 8, vq = (idx >> 5) & 7, bl = idx & 31;
    const f32x4 t = VTq[((size_t)r * (VP / 4) + (v0 >> 2) + vq) * BP + bb0 + bl];
#pragma unroll
    for (int u = 0; u < 4; ++u) tile[bl][(vq * 4 + u) * 3 + r] = t[u];
  }
  __syncthreads();
  if (verts) {
    for (int idx = threadIdx.x; idx < 32 * 96; idx += blockDim.x) {
      const int bl = idx / 96, rem = idx % 96;
      const int b = bb0 + bl, v = v0 + rem / 3;
      if (p2v) {
        const int vo = v < V ? p2v[v] : -1;
        if (b < B && vo >= 0 && vo < vlimit) verts[(size_t)b * ldv + vo * 3 + rem % 3] = tile[bl][rem];
      } else if (b < B && v < vlimit) verts[(size_t)b * ldv + v0 * 3 + rem] = tile[bl][rem];
    }
  }
  if (ndc) {
    for (int idx = threadIdx.x; idx < 32 * 32; idx += blockDim.x) {
      const int bl = idx / 32, vv = idx % 32;
      const int b = bb0 + bl, v = v0 + vv;
      const int vo = (v < V) ? (p2v ? p2v[v] : v) : -1;
      if (b < B && vo >= 0) {
        const float X = -2.f * tile[bl][vv * 3] + cam[(size_t)b * 3], Y = -2.f * tile[bl][vv * 3 + 1] + cam[(size_t)b * 3 + 1];
        const float Z = 2.f * tile[bl][vv * 3 + 2] + cam[(size_t)b * 3 + 2];
        f32x4 o = {focal * X / Z, focal * Y / Z, Z, 0.f};
        ndc[(size_t)b * V + vo] = o;
      }
    }
  }
}

int launch_verts_untranspose(const float* VTb, float* verts, int ldv, int vlimit, const float* cam, float* ndc, int B, int BP,
                             hipStream_t s, const int* p2v) {
  hipLaunchKernelGGL(k_verts_untranspose, dim3(VT, BP / 32), dim3(256), 0, s, VTb, verts, ldv, vlimit, cam, (f32x4*)ndc,
                     5000.f / 224.f, B, BP, p2v);
  return 0;
}

// (B,6890,3) -> [3][VP/4][BP][4] (row quads) transpose of an external vertex adjoint (operator-level SMPL backward,
// silhouette adjoint)
__global__ void k_dverts_transpose(const float* __restrict__ dverts, int ldv, float* __restrict__ dVT, int B, int BP,
                                   const int* __restrict__ p2v) {
  __shared__ float tile[32][97];
  const int v0 = blockIdx.x * 32, bb0 = blockIdx.y * 32;
  for (int idx = threadIdx.x; idx < 32 * 96; idx += blockDim.x) {
    int bl = idx / 96, rem = idx % 96;   // rem = vv*3 + r
    int b = bb0 + bl, v = v0 + rem / 3;
    float val = 0.f;
    if (b < B && v < V) val = p2v ? dverts[(size_t)b * ldv + p2v[v] * 3 + rem % 3] : dverts[(size_t)b * ldv + v0 * 3 + rem];
    tile[bl][rem] = val;
  }
  __syncthreads();
  f32x4* dVq = reinterpret_cast<f32x4*>(dVT);
  for (int idx = threadIdx.x; idx < 3 * 8 * 32; idx += blockDim.x) {
    const int r = idx >> 8, vq = (idx >> 5) & 7, bl = idx & 31;
    f32x4 t;
#pragma unroll
    for (int u = 0; u < 4; ++u) t[u] = tile[bl][(vq * 4 + u) * 3 + r];
    dVq[((size_t)r * (VP / 4) + (v0 >> 2) + vq) * BP + bb0 + bl] = t;
  }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
template <int N> using dv_mode = std::integral_constant<int, N>;      // the kernels' DV argument (above), chosen from the adjoints given

int launch_lbs_bwd(const Model& m, const float* Tb, const float* AT, const float* VPb, const float* dJT,
                   const float* dVT, float* DVP, float* dATp, int BP, int nvc, hipStream_t s, const int* tl, int ntl, unsigned* dmask) {
  if (tl && !(m.kjs && m.bwd16 && !dVT)) { jrr_set_error("lbs_bwd: the tile list serves k_lbs_bwd16 without an outside vertex adjoint"); return JRR_ERR_ARG; }
  if (m.kjs && m.bwd16) {                       // four symmetric waves: one workgroup per (64 poses, vertex chunk)
    const int n_bt16 = BP / 64;
    dim3 grid16(n_bt16 * nvc), block16(256);
    // share of the first-dispatched workgroup of a CU in thousandths (540 since the slab flush
    // reads back in one batch: 0.1777 ms against 0.1797 at 520, 0.1782 at 560; before that 520: round 4, with
    // the non-temporal streams -- 0.1797 ms against 0.1815 at 480, 0.186 at 560; shader-clock stamps: the first-dispatched workgroup's
    // tiles take ~12 300 clocks, its partner's ~14 000 while both run and 7 400 once it is alone), 0 = no
    // pairing (the geometry is not one round of two workgroups per CU)
    constexpr int pair_split = 540;
    const int paired16 = pairs_one_round(n_bt16, nvc) ? pair_split : 0;
    auto launch16 = [&](auto DVM, auto LIST) {      // LIST: the listed tiles only (DV = 0)
      with_skin_class(m.kjs, m.wide_tiles, [&](auto KJ, auto WD) {
        constexpr bool list = decltype(LIST)::value;
        if constexpr (decltype(KJ)::value > 0)      // (m.kjs != 0 here)
          hipLaunchKernelGGL((k_lbs_bwd16<decltype(DVM)::value, decltype(KJ)::value, decltype(WD)::value, list>), grid16, block16, 0, s, Tb,
                             AT, VPb, dJT, dVT, DVP, dATp, BP, nvc, n_bt16, m.segid, m.segj, paired16, m.tnj, list ? tl : nullptr,
                             list ? ntl : 0, dmask);
      });
    };
    if (tl) launch16(dv_mode<0>{}, std::true_type{});
    else if (dVT && dJT) launch16(dv_mode<2>{}, std::false_type{});
    else if (dVT) launch16(dv_mode<1>{}, std::false_type{});
    else launch16(dv_mode<0>{}, std::false_type{});
    return 0;
  }
  const int n_bt = BP / BT;                     // one workgroup per (pose tile, vertex chunk)
  dim3 grid(n_bt * nvc), block(256);
  // (the role kernel has no per-tile classes: one wide tile sends it to its dense form, Model::role_kjs = 0)
  auto launch = [&](auto DVM) {
    with_skin_class(m.role_kjs, false, [&](auto KJ, auto) {
      hipLaunchKernelGGL((k_lbs_bwd<decltype(DVM)::value, decltype(KJ)::value>), grid, block, 0, s, Tb, AT, VPb, dJT, dVT, DVP, dATp, BP,
                         nvc, n_bt, m.jl, m.segid, m.segj);
    });
  };
  if (dVT && dJT) launch(dv_mode<2>{});
  else if (dVT) launch(dv_mode<1>{});
  else launch(dv_mode<0>{});
  return 0;
}

int launch_dverts_transpose(const float* dverts, int ldv, float* dVT, int B, int BP, hipStream_t s, const int* p2v) {
  hipLaunchKernelGGL(k_dverts_transpose, dim3(VT, BP / 32), dim3(256), 0, s, dverts, ldv, dVT, B, BP, p2v);
  return 0;
}

int launch_bwd_tab_static(const Model& m, float* Tb, hipStream_t s) {
  const bool r16 = m.kjs && m.bwd16;
  hipLaunchKernelGGL(k_bwd_tab_static, dim3(VT * 2048 / 256), dim3(256), 0, s, m.Wjv, m.Wvj, Tb, (r16 || m.role_kjs) ? m.Wc : nullptr,
                     r16 ? m.kjs : m.role_kjs, m.W16, m.jl, r16 ? 1 : 0);
  return 0;
}

}  // namespace jrr
