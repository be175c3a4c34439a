// The self-penetration report (`--eval_penetration`): is a mesh a possible body at all.  Every vertex is pushed a little under the skin
// and asked for the winding number of the whole surface around it: 1 for sound skin, 2 or more where that piece of skin lies inside
// another piece of the body, 0 where the body is thinner than the push.  Two launches, no engine, no body model (the caller brings the
// faces):
//
// k_mesh_winding            one workgroup of 16 waves per (pose, block of 1024 points).  The pose's vertices are staged into dynamic LDS
//                           as depth.hip holds them (12 bytes per vertex, up to 96 KiB).  One point per lane, in registers; EVERY wave
//                           walks ALL the faces, four per trip.  The face is wave-uniform: its three indices come through the scalar
//                           cache (asked for one trip ahead), its corners are broadcast reads of LDS, and every lane does the solid-angle
//                           arithmetic of depth.hip on its own point.  Four double accumulators per lane: face f goes to f mod 4.  A lane
//                           shares nothing with another, so a point's bits do not depend on where it stands.
//                           One point per lane and not two: a pair costs about a hundred vector instructions (three square roots, atan2f,
//                           a conversion and a double add) against nine broadcast LDS dwords and three scalar dwords per WAVE -- the
//                           vector ALU is the limit by two orders of magnitude, and a second point would halve traffic that is not in
//                           the way while doubling the live registers of atan2f.
// k_penetration_accumulate  one workgroup per pose: the three per-pose counts, then the pose's row of the group table (include/jrr.h,
//                           JRR_PEN_ACC_*) and the per-vertex counts.  Integer atomics only: the tables do not depend on the order, the
//                           split into calls or the sharding over ranks.
#include "jrr_common.h"
#include "acctab.h"
#include "../../include/jrr.h"

namespace jrr {

constexpr int PN_THREADS = 1024;                                      // points per workgroup: one per lane
constexpr int PN_UNROLL = 4;                                          // faces per trip = partial sums per point
constexpr int PN_OFF_FLAG = 0;                                        // int: a non-finite vertex in this pose
constexpr int PN_OFF_VERTS = 16;                                      // float [n_verts][3]
constexpr int PN_LDS_MAX = PN_OFF_VERTS + JRR_DEPTH_MAX_VERTS * 12;   // 98 320 bytes of the CU's 160 KiB
constexpr int PN_ACC_THREADS = 256;
constexpr float PN_FINITE = 3.402823466e+38f;                         // FLT_MAX: |x| <= PN_FINITE: neither NaN nor infinite
constexpr double PN_FOUR_PI = 12.566370614359172;

static_assert(PN_OFF_VERTS % 16 == 0 && PN_LDS_MAX <= 160 * 1024, "LDS carve");
static_assert(JRR_WINDING_MAX_POINTS == 65536 && JRR_WINDING_MAX_POINTS / PN_THREADS <= 65535, "grid.y");
static_assert(JRR_PEN_ACC_POSES_PEN == 2 && JRR_PEN_ACC_POSES_PEN8 == 3 && JRR_PEN_ACC_SUM_PEN == 4 && JRR_PEN_ACC_SUM_THIN == 5 &&
              JRR_PEN_ACC_SUM_UNSURE == 6 && JRR_PEN_ACC_HIST == 7 && JRR_PEN_ACC_PART == JRR_PEN_ACC_HIST + JRR_PEN_ACC_BINS &&
              JRR_PEN_ACC_ROW == JRR_PEN_ACC_PART + JRR_PEN_ACC_PARTS && JRR_PEN_ACC_TRAILER == JRR_EVAL_ACC_TRAILER, "row layout");

struct WindingArgs {
  const float* verts; const int* faces; const float* points;
  float* wind; int* status;
  int n_verts, n_faces, n_points;
};

__device__ __forceinline__ bool pn_finite(float x) { return fabsf(x) <= PN_FINITE; }
__device__ __forceinline__ float pn_dot(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// the solid angle of the face (i0, i1, i2) of the staged pose seen from p (van Oosterom and Strackee 1983), as depth.hip forms it
__device__ __forceinline__ float pn_omega(const float* s_v, int i0, int i1, int i2, const float* p) {
  float A[3], B[3], C[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    A[c] = s_v[i0 * 3 + c] - p[c]; B[c] = s_v[i1 * 3 + c] - p[c]; C[c] = s_v[i2 * 3 + c] - p[c];
  }
  const float la = __builtin_amdgcn_sqrtf(pn_dot(A, A)), lb = __builtin_amdgcn_sqrtf(pn_dot(B, B)), lc = __builtin_amdgcn_sqrtf(pn_dot(C, C));   // v_sqrt_f32, 1 ulp
  const float cr[3] = {B[1] * C[2] - B[2] * C[1], B[2] * C[0] - B[0] * C[2], B[0] * C[1] - B[1] * C[0]};
  const float num = pn_dot(A, cr);
  const float dn = la * lb * lc + pn_dot(A, B) * lc + pn_dot(B, C) * la + pn_dot(C, A) * lb;
  return 2.0f * atan2f(num, dn);
}

// grid: (pose, block of PN_THREADS points)
__global__ __launch_bounds__(PN_THREADS) void k_mesh_winding(WindingArgs q) {
  extern __shared__ __attribute__((aligned(16))) char pn_lds[];
  int* s_flag = reinterpret_cast<int*>(pn_lds + PN_OFF_FLAG);
  float* s_v = reinterpret_cast<float*>(pn_lds + PN_OFF_VERTS);
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const int pt = blockIdx.y * PN_THREADS + tid;

  if (tid == 0) s_flag[0] = 0;
  __syncthreads();
  {                                              // the pose's vertices, once per workgroup; a non-finite one poisons the whole pose
    const float* src = q.verts + b * (size_t)q.n_verts * 3;
    const int n3 = q.n_verts * 3;
    bool bad = false;
    for (int i = tid; i < n3; i += PN_THREADS) {
      const float x = src[i];
      bad = bad || !pn_finite(x);
      s_v[i] = x;
    }
    if (bad) s_flag[0] = 1;
  }
  // a lane beyond n_points repeats the last point (its result is never stored)
  const float* pp = q.points + (b * (size_t)q.n_points + (size_t)min(pt, q.n_points - 1)) * 3;
  const float p[3] = {pp[0], pp[1], pp[2]};
  __syncthreads();

  double sum[PN_UNROLL] = {0.0, 0.0, 0.0, 0.0};
  bool oob = false;
  const unsigned nv = (unsigned)q.n_verts;
  const int whole = q.n_faces - q.n_faces % PN_UNROLL;
  int nx[PN_UNROLL * 3];                         // the next trip's corners, asked for one trip ahead of their use
#pragma unroll
  for (int k = 0; k < PN_UNROLL * 3; ++k) nx[k] = 0;
  if (whole > 0) {
#pragma unroll
    for (int k = 0; k < PN_UNROLL * 3; ++k) nx[k] = q.faces[k];
  }
  for (int f = 0; f < whole; f += PN_UNROLL) {   // uniform over the whole workgroup: scalar loads, broadcast LDS reads
    int ix[PN_UNROLL * 3];
#pragma unroll
    for (int k = 0; k < PN_UNROLL * 3; ++k) ix[k] = nx[k];
    if (f + PN_UNROLL < whole) {
      const int* fi = q.faces + (size_t)(f + PN_UNROLL) * 3;
#pragma unroll
      for (int k = 0; k < PN_UNROLL * 3; ++k) nx[k] = fi[k];
    }
#pragma unroll
    for (int u = 0; u < PN_UNROLL; ++u) {
      const int i0 = ix[3 * u], i1 = ix[3 * u + 1], i2 = ix[3 * u + 2];
      if ((unsigned)i0 >= nv || (unsigned)i1 >= nv || (unsigned)i2 >= nv) { oob = true; continue; }
      sum[u] += (double)pn_omega(s_v, i0, i1, i2, p);
    }
  }
  for (int f = whole; f < q.n_faces; ++f) {      // the last n_faces mod 4 faces: face f still goes to partial sum f mod 4
    const int* fi = q.faces + (size_t)f * 3;
    const int i0 = fi[0], i1 = fi[1], i2 = fi[2];
    if ((unsigned)i0 >= nv || (unsigned)i1 >= nv || (unsigned)i2 >= nv) { oob = true; continue; }
    const double o = (double)pn_omega(s_v, i0, i1, i2, p);
    const int u = f - whole;
    if (u == 0) sum[0] += o; else if (u == 1) sum[1] += o; else sum[2] += o;
  }
  if (oob && tid == 0) atomicOr(q.status, JRR_DEPTH_STATUS_INDEX);
  if (pt >= q.n_points) return;
  const bool poisoned = s_flag[0] != 0 || !pn_finite(p[0]) || !pn_finite(p[1]) || !pn_finite(p[2]);
  const double total = (sum[0] + sum[1]) + (sum[2] + sum[3]);
  q.wind[b * (size_t)q.n_points + pt] = poisoned ? __int_as_float(0x7fc00000) : (float)(total / PN_FOUR_PI);
}

#pragma clang fp contract(off)

// bit 0: penetrating, bit 1: thin, bit 2: unsure, bit 3: not finite
__device__ __forceinline__ int pn_classify(float w) {
  const float aw = fabsf(w), k = rintf(aw);
  return (k >= 2.f ? 1 : 0) | (k == 0.f ? 2 : 0) | (fabsf(aw - k) > 0.1f ? 4 : 0) | (pn_finite(w) ? 0 : 8);
}

struct PenAccArgs {
  const float* wind; const int* part; const int* group;
  long long* acc; long long* per_vertex; int* n_pen; int* n_thin; int* n_unsure;
  int n_verts, n_groups;
};

// grid: one workgroup per pose
__global__ __launch_bounds__(PN_ACC_THREADS) void k_penetration_accumulate(PenAccArgs q) {
  __shared__ int s_cnt[4];                       // penetrating, thin, unsure, not finite
  __shared__ int s_part[JRR_PEN_ACC_PARTS];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const float* w = q.wind + b * (size_t)q.n_verts;
  if (tid < 4) s_cnt[tid] = 0;
  if (tid < JRR_PEN_ACC_PARTS) s_part[tid] = 0;
  __syncthreads();
  int c[4] = {0, 0, 0, 0};
  for (int v = tid; v < q.n_verts; v += PN_ACC_THREADS) {
    const int m = pn_classify(w[v]);
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] += (m >> k) & 1;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c[k]) atomicAdd(&s_cnt[k], c[k]);
  __syncthreads();
  const int n_pen = s_cnt[0], n_thin = s_cnt[1], n_unsure = s_cnt[2];
  const bool bad = s_cnt[3] != 0;
  if (tid == 0) {                                // the per-pose counts: for every pose, whatever its group
    if (q.n_pen) q.n_pen[b] = n_pen;
    if (q.n_thin) q.n_thin[b] = n_thin;
    if (q.n_unsure) q.n_unsure[b] = n_unsure;
  }
  const int g = q.group ? q.group[b] : 0;
  if (long long* t = acc_refused(q.acc, JRR_PEN_ACC_ROW, q.n_groups, g)) { if (tid == 0) acc_add(t, 1); return; }
  long long* row = acc_row(q.acc, JRR_PEN_ACC_ROW, g);
  if (bad) { if (tid == 0) acc_add(row + JRR_PEN_ACC_BAD, 1); return; }      // a pose is counted whole or not at all
  if (tid == 0) {
    acc_add(row + JRR_PEN_ACC_COUNT, 1);
    if (n_pen >= 1) acc_add(row + JRR_PEN_ACC_POSES_PEN, 1);
    if (n_pen >= 8) acc_add(row + JRR_PEN_ACC_POSES_PEN8, 1);
    if (n_pen) acc_add(row + JRR_PEN_ACC_SUM_PEN, n_pen);
    if (n_thin) acc_add(row + JRR_PEN_ACC_SUM_THIN, n_thin);
    if (n_unsure) acc_add(row + JRR_PEN_ACC_SUM_UNSURE, n_unsure);
    acc_add(row + JRR_PEN_ACC_HIST + min(JRR_PEN_ACC_BINS - 1, 32 - __clz(n_pen)), 1);      // the number of bits of n_pen; __clz(0) = 32
  }
  if (n_pen == 0) return;
  for (int v = tid; v < q.n_verts; v += PN_ACC_THREADS) {
    if (!(pn_classify(w[v]) & 1)) continue;
    if (q.per_vertex) acc_add(q.per_vertex + v, 1);
    const int pl = q.part ? q.part[v] : 0;
    atomicAdd(&s_part[(unsigned)pl < (unsigned)JRR_PEN_ACC_PARTS ? pl : JRR_PEN_ACC_PARTS - 1], 1);
  }
  __syncthreads();
  if (tid < JRR_PEN_ACC_PARTS && s_part[tid]) acc_add(row + JRR_PEN_ACC_PART + tid, s_part[tid]);
}

}  // namespace jrr

using namespace jrr;

extern "C" int jrr_mesh_winding(const float* verts, int batch, int n_verts, const int32_t* faces, int n_faces, const float* points, int n_points,
                                float* wind, int32_t* status, void* stream) {
  if (!verts || !faces || !points || !wind || !status || batch < 0) {
    jrr_set_error("jrr_mesh_winding: bad argument (verts, faces, points, wind and status must not be NULL, batch >= 0)");
    return JRR_ERR_ARG;
  }
  if (n_points < 1 || n_points > JRR_WINDING_MAX_POINTS || n_verts < 1 || n_verts > JRR_DEPTH_MAX_VERTS || n_faces < 1) {
    jrr_set_error("jrr_mesh_winding: %d points, %d vertices, %d faces: 1 .. %d points, 1 .. %d vertices, 1 or more faces", n_points, n_verts, n_faces,
                  (int)JRR_WINDING_MAX_POINTS, (int)JRR_DEPTH_MAX_VERTS);
    return JRR_ERR_ARG;
  }
  if ((((uintptr_t)verts | (uintptr_t)faces | (uintptr_t)points | (uintptr_t)wind | (uintptr_t)status) & 3) != 0) {
    jrr_set_error("jrr_mesh_winding: misaligned pointer (4 bytes)");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  static const bool attr = hipFuncSetAttribute((const void*)k_mesh_winding, hipFuncAttributeMaxDynamicSharedMemorySize, PN_LDS_MAX) == hipSuccess;
  if (!attr) { jrr_set_error("k_mesh_winding: %d bytes of LDS refused", PN_LDS_MAX); return JRR_ERR_HIP; }
  WindingArgs q{verts, faces, points, wind, status, n_verts, n_faces, n_points};
  hipLaunchKernelGGL(k_mesh_winding, dim3((unsigned)batch, (unsigned)((n_points + PN_THREADS - 1) / PN_THREADS)), dim3(PN_THREADS),
                     (size_t)(PN_OFF_VERTS + n_verts * 12), (hipStream_t)stream, q);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_penetration_accumulate(const float* wind, const int32_t* part, const int32_t* group, int batch, int n_verts, int n_groups,
                                          int64_t* acc, int64_t* per_vertex, int32_t* n_pen, int32_t* n_thin, int32_t* n_unsure, void* stream) {
  if (!wind || !acc || batch < 0 || !acc_aligned(acc, per_vertex) ||
      (((uintptr_t)wind | (uintptr_t)part | (uintptr_t)group | (uintptr_t)n_pen | (uintptr_t)n_thin | (uintptr_t)n_unsure) & 3) != 0) {
    jrr_set_error("jrr_penetration_accumulate: bad argument (wind and acc must not be NULL, batch >= 0, the tables 8-byte aligned, the others 4)");
    return JRR_ERR_ARG;
  }
  if (!acc_groups_ok(n_groups) || n_verts < 1 || n_verts > JRR_WINDING_MAX_POINTS) {
    jrr_set_error("jrr_penetration_accumulate: %d groups of %d vertices: 1 .. %d groups, 1 .. %d vertices", n_groups, n_verts,
                  (int)JRR_EVAL_ACC_MAX_GROUPS, (int)JRR_WINDING_MAX_POINTS);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  PenAccArgs q{wind, part, group, reinterpret_cast<long long*>(acc), reinterpret_cast<long long*>(per_vertex), n_pen, n_thin, n_unsure, n_verts, n_groups};
  hipLaunchKernelGGL(k_penetration_accumulate, dim3((unsigned)batch), dim3(PN_ACC_THREADS), 0, (hipStream_t)stream, q);
  CHECK_LAUNCH();
  return JRR_OK;
}
