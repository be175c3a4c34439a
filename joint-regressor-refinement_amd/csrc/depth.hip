// The depth section of the regressor report (`--regressor_report_depth`): is a regressed joint still under the skin, and how deep.
// A row of the regressor lies on the simplex, so its joint lies in the convex hull of its support vertices -- which is not the body.
// Two launches, no engine, no body model (the caller brings the faces):
//
// k_point_mesh_depth   one workgroup of 16 waves per pose.  The pose's vertices are staged once into dynamic LDS (12 bytes per vertex,
//                      up to 96 KiB).  Lane l of every wave owns point l (up to 64 points: one wave-width); wave w walks the faces
//                      w, w + 16, w + 32, ... in ascending order.  The face is wave-uniform: its three indices come through the scalar
//                      cache, its corners are broadcast reads of LDS, and every lane does the same closest-point and solid-angle
//                      arithmetic on its own point -- the seven regions are selects, not branches, so a wave never diverges.  Per lane
//                      three accumulators: the smallest squared distance, its face, and the sum of the solid angles in double.  Then
//                      one fixed tree over the 16 waves in LDS.  Which wave sums which faces, and the tree, depend on n_faces alone.
// k_depth_accumulate   one wave per pose, lane k owns point column k: the signed depth as fixed-point sums, counts and 4-mm histograms
//                      per group (include/jrr.h, JRR_DEPTH_ACC_*).  Integer atomics only, as k_shift_accumulate: the table does not
//                      depend on the order, the split into calls or the sharding over ranks.
#include "jrr_common.h"
#include "acctab.h"
#include "../../include/jrr.h"

namespace jrr {

constexpr int DP_WAVES = 16;
constexpr int DP_THREADS = DP_WAVES * 64;
constexpr int DP_SLOTS = DP_WAVES * 64;                               // (wave, point) partial results
constexpr int DP_OFF_SUM = 0;                                         // double [16][64]
constexpr int DP_OFF_BEST = DP_OFF_SUM + DP_SLOTS * 8;                // float  [16][64]
constexpr int DP_OFF_FACE = DP_OFF_BEST + DP_SLOTS * 4;               // int    [16][64]
constexpr int DP_OFF_FLAG = DP_OFF_FACE + DP_SLOTS * 4;               // int: a non-finite vertex in this pose
constexpr int DP_OFF_VERTS = DP_OFF_FLAG + 16;                        // float  [n_verts][3]
constexpr int DP_LDS_MAX = DP_OFF_VERTS + JRR_DEPTH_MAX_VERTS * 12;   // 114 704 bytes of the CU's 160 KiB
constexpr int DP_ACC_THREADS = 256;
constexpr float DP_FINITE = 3.402823466e+38f;                         // FLT_MAX: |x| <= DP_FINITE: neither NaN nor infinite
constexpr float DP_FIXED = 16777216.f;                                // 2^24
constexpr double DP_FOUR_PI = 12.566370614359172;

static_assert(JRR_DEPTH_MAX_POINTS == 64, "one lane per point");
static_assert(DP_OFF_VERTS % 16 == 0 && DP_LDS_MAX <= 160 * 1024, "LDS carve");
static_assert(JRR_DEPTH_ACC_OUTSIDE == 2 && JRR_DEPTH_ACC_UNSURE == JRR_DEPTH_ACC_OUTSIDE + JRR_DEPTH_MAX_POINTS &&
              JRR_DEPTH_ACC_SUM == JRR_DEPTH_ACC_UNSURE + JRR_DEPTH_MAX_POINTS && JRR_DEPTH_ACC_HIST == JRR_DEPTH_ACC_SUM + JRR_DEPTH_MAX_POINTS &&
              JRR_DEPTH_ACC_ROW == JRR_DEPTH_ACC_HIST + JRR_DEPTH_MAX_POINTS * JRR_DEPTH_ACC_BINS && JRR_DEPTH_ACC_TRAILER == JRR_EVAL_ACC_TRAILER,
              "row layout");

struct DepthArgs {
  const float* verts; const int* faces; const float* points;
  float* dist; float* wind; int* face; int* status;
  int n_verts, n_faces, n_points;
};

__device__ __forceinline__ bool dp_finite(float x) { return fabsf(x) <= DP_FINITE; }
__device__ __forceinline__ float dp_dot(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// grid: one workgroup per pose
__global__ __launch_bounds__(DP_THREADS) void k_point_mesh_depth(DepthArgs q) {
  extern __shared__ __attribute__((aligned(16))) char dp_lds[];
  double* s_sum = reinterpret_cast<double*>(dp_lds + DP_OFF_SUM);
  float* s_best = reinterpret_cast<float*>(dp_lds + DP_OFF_BEST);
  int* s_face = reinterpret_cast<int*>(dp_lds + DP_OFF_FACE);
  int* s_flag = reinterpret_cast<int*>(dp_lds + DP_OFF_FLAG);
  float* s_v = reinterpret_cast<float*>(dp_lds + DP_OFF_VERTS);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t b = blockIdx.x;

  if (tid == 0) s_flag[0] = 0;
  __syncthreads();
  {                                              // the pose's vertices, once; a non-finite one poisons the whole pose
    const float* src = q.verts + b * (size_t)q.n_verts * 3;
    const int n3 = q.n_verts * 3;
    bool bad = false;
    for (int i = tid; i < n3; i += DP_THREADS) {
      const float x = src[i];
      bad = bad || !dp_finite(x);
      s_v[i] = x;
    }
    if (bad) s_flag[0] = 1;
  }
  // lane l owns point l; a lane beyond n_points repeats the last point (its result is never stored)
  const float* pp = q.points + (b * (size_t)q.n_points + (size_t)min(lane, q.n_points - 1)) * 3;
  const float p[3] = {pp[0], pp[1], pp[2]};
  __syncthreads();

  float best = __int_as_float(0x7f800000);       // +inf: the first finite squared distance wins, a NaN never does
  int bestf = -1;
  double sum = 0.0;
  bool oob = false;
  const unsigned nv = (unsigned)q.n_verts;
  int n0 = 0, n1 = 0, n2 = 0;                    // the next face's corners, asked for one face ahead of their use
  if (w < q.n_faces) { const int* fi = q.faces + (size_t)w * 3; n0 = fi[0]; n1 = fi[1]; n2 = fi[2]; }
  for (int f = w; f < q.n_faces; f += DP_WAVES) {                  // wave-uniform: scalar loads, broadcast LDS reads
    const int i0 = n0, i1 = n1, i2 = n2;
    if (f + DP_WAVES < q.n_faces) { const int* fi = q.faces + (size_t)(f + DP_WAVES) * 3; n0 = fi[0]; n1 = fi[1]; n2 = fi[2]; }
    if ((unsigned)i0 >= nv || (unsigned)i1 >= nv || (unsigned)i2 >= nv) { oob = true; continue; }
    float A[3], B[3], C[3], ab[3], ac[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float xa = s_v[i0 * 3 + c], xb = s_v[i1 * 3 + c], xc = s_v[i2 * 3 + c];
      ab[c] = xb - xa; ac[c] = xc - xa;
      A[c] = xa - p[c]; B[c] = xb - p[c]; C[c] = xc - p[c];
    }
    // ---- closest point of the closed triangle (the seven Voronoi regions; d_k as in Ericson, Real-Time Collision Detection 5.1.5,
    // with ap = -A, bp = -B, cp = -C) ----
    const float d1 = -dp_dot(ab, A), d2 = -dp_dot(ac, A), d3 = -dp_dot(ab, B), d4 = -dp_dot(ac, B), d5 = -dp_dot(ab, C), d6 = -dp_dot(ac, C);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    const bool in_a = d1 <= 0.f && d2 <= 0.f;
    const bool in_b = d3 >= 0.f && d4 <= d3;
    const bool in_ab = vc <= 0.f && d1 >= 0.f && d3 <= 0.f;
    const bool in_c = d6 >= 0.f && d5 <= d6;
    const bool in_ac = vb <= 0.f && d2 >= 0.f && d6 <= 0.f;
    const bool in_bc = va <= 0.f && d43 >= 0.f && d56 >= 0.f;
    // the region is the first that holds, in the order a, b, ab, c, ac, bc, interior; one reciprocal serves whichever it is.  Selects,
    // not branches: closest point = a + v ab + u ac with (v, u) = (num_v, num_u) / den
    const float den_ab = d1 - d3, den_ac = d2 - d6, den_bc = d43 + d56, den_in = va + vb + vc;
    const float den = in_ab ? den_ab : in_ac ? den_ac : in_bc ? den_bc : den_in;
    const float num_v = in_ab ? d1 : in_ac ? 0.f : in_bc ? d56 : vb;
    const float num_u = in_ab ? 0.f : in_ac ? d2 : in_bc ? d43 : vc;
    const float r = __builtin_amdgcn_rcpf(den);                    // v_rcp_f32, 1 ulp: v and u move by 1e-7 of an edge
    const float v = num_v * r, u = num_u * r;
    float dl[3];
    const bool at_a = in_a, at_b = !in_a && in_b, at_c = !in_a && !in_b && !in_ab && in_c;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float e = A[c] + v * ab[c] + u * ac[c];
      dl[c] = at_a ? A[c] : at_b ? B[c] : at_c ? C[c] : e;          // a corner region takes the corner itself
    }
    const float d2f = dp_dot(dl, dl);
    if (d2f < best) { best = d2f; bestf = f; }                     // ascending f: among equal values the smallest index stays
    // ---- solid angle (van Oosterom and Strackee 1983) ----
    const float la = __builtin_amdgcn_sqrtf(dp_dot(A, A)), lb = __builtin_amdgcn_sqrtf(dp_dot(B, B)), lc = __builtin_amdgcn_sqrtf(dp_dot(C, C));   // v_sqrt_f32, 1 ulp
    const float cr[3] = {B[1] * C[2] - B[2] * C[1], B[2] * C[0] - B[0] * C[2], B[0] * C[1] - B[1] * C[0]};
    const float num = dp_dot(A, cr);
    const float dn = la * lb * lc + dp_dot(A, B) * lc + dp_dot(B, C) * la + dp_dot(C, A) * lb;
    sum += (double)(2.0f * atan2f(num, dn));
  }
  if (oob && lane == 0) atomicOr(q.status, JRR_DEPTH_STATUS_INDEX);

  s_sum[w * 64 + lane] = sum;
  s_best[w * 64 + lane] = best;
  s_face[w * 64 + lane] = bestf;
  __syncthreads();
  if (tid >= q.n_points) return;                 // wave 0, lane = point
  double t[DP_WAVES];
#pragma unroll
  for (int i = 0; i < DP_WAVES; ++i) t[i] = s_sum[i * 64 + lane];
#pragma unroll
  for (int n = DP_WAVES / 2; n >= 1; n >>= 1)    // (t0 + t1), (t2 + t3), ... then the pairs of those, four levels
#pragma unroll
    for (int i = 0; i < n; ++i) t[i] = t[2 * i] + t[2 * i + 1];
  best = s_best[lane]; bestf = s_face[lane];
#pragma unroll
  for (int i = 1; i < DP_WAVES; ++i) {
    const float d = s_best[i * 64 + lane];
    const int f = s_face[i * 64 + lane];
    if (d < best || (d == best && f < bestf)) { best = d; bestf = f; }
  }
  const bool poisoned = s_flag[0] != 0 || !dp_finite(p[0]) || !dp_finite(p[1]) || !dp_finite(p[2]);
  const float nan = __int_as_float(0x7fc00000);
  const size_t o = b * (size_t)q.n_points + lane;
  if (q.dist) q.dist[o] = poisoned ? nan : sqrtf(best);
  if (q.wind) q.wind[o] = poisoned ? nan : (float)(t[0] / DP_FOUR_PI);
  if (q.face) q.face[o] = poisoned ? -1 : bestf;
}

#pragma clang fp contract(off)

// one wave per pose, lane k = point column k; every update is an int64 atomic
__global__ __launch_bounds__(DP_ACC_THREADS) void k_depth_accumulate(const float* __restrict__ dist, const float* __restrict__ wind,
                                                                     const int* __restrict__ group, int n_points, int n_groups,
                                                                     long long* __restrict__ acc, int B) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (DP_ACC_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= B) return;
  const int g = group ? group[b] : 0;
  if (long long* t = acc_refused(acc, JRR_DEPTH_ACC_ROW, n_groups, g)) { if (lane == 0) acc_add(t, 1); return; }
  long long* row = acc_row(acc, JRR_DEPTH_ACC_ROW, g);
  const bool mine = lane < n_points;
  const float d = mine ? dist[(size_t)b * n_points + lane] : 0.f;
  const float wn = mine ? wind[(size_t)b * n_points + lane] : 0.f;
  const bool bad = !(dp_finite(d) && dp_finite(wn) && d < ERR_CAP);
  if (__any(bad)) { if (lane == 0) acc_add(row + JRR_DEPTH_ACC_BAD, 1); return; }   // a pose is counted whole or not at all
  if (lane == 0) acc_add(row + JRR_DEPTH_ACC_COUNT, 1);
  if (!mine) return;
  const float aw = fabsf(wn);
  const bool inside = aw > 0.5f;
  const float depth = inside ? d : -d;
  if (!inside) acc_add(row + JRR_DEPTH_ACC_OUTSIDE + lane, 1);
  if (fabsf(aw - rintf(aw)) > 0.1f) acc_add(row + JRR_DEPTH_ACC_UNSURE + lane, 1);
  acc_add(row + JRR_DEPTH_ACC_SUM + lane, __float2ll_rn(depth * DP_FIXED));
  const float t = depth + 0.064f;
  const int bin = max(min((int)floorf(t * 250.0f), JRR_DEPTH_ACC_BINS - 1), 0);
  acc_add(row + JRR_DEPTH_ACC_HIST + lane * JRR_DEPTH_ACC_BINS + bin, 1);
}

}  // namespace jrr

using namespace jrr;

extern "C" int jrr_point_mesh_depth(const float* verts, int batch, int n_verts, const int32_t* faces, int n_faces, const float* points,
                                    int n_points, float* dist, float* wind, int32_t* face, int32_t* status, void* stream) {
  if (!verts || !faces || !points || !status || batch < 0) {
    jrr_set_error("jrr_point_mesh_depth: bad argument (verts, faces, points and status must not be NULL, batch >= 0)");
    return JRR_ERR_ARG;
  }
  if (!dist && !wind && !face) {
    jrr_set_error("jrr_point_mesh_depth: dist, wind and face are all NULL: nothing to compute");
    return JRR_ERR_ARG;
  }
  if (n_points < 1 || n_points > JRR_DEPTH_MAX_POINTS || n_verts < 1 || n_verts > JRR_DEPTH_MAX_VERTS || n_faces < 1) {
    jrr_set_error("jrr_point_mesh_depth: %d points, %d vertices, %d faces: 1 .. %d points, 1 .. %d vertices, 1 or more faces", n_points, n_verts,
                  n_faces, (int)JRR_DEPTH_MAX_POINTS, (int)JRR_DEPTH_MAX_VERTS);
    return JRR_ERR_ARG;
  }
  if (((uintptr_t)verts & 7) != 0 || (((uintptr_t)faces | (uintptr_t)points | (uintptr_t)dist | (uintptr_t)wind | (uintptr_t)face | (uintptr_t)status) & 3) != 0) {
    jrr_set_error("jrr_point_mesh_depth: misaligned pointer (verts: 8 bytes, the others: 4)");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  static const bool attr =
      hipFuncSetAttribute((const void*)k_point_mesh_depth, hipFuncAttributeMaxDynamicSharedMemorySize, DP_LDS_MAX) == hipSuccess;
  if (!attr) { jrr_set_error("k_point_mesh_depth: %d bytes of LDS refused", DP_LDS_MAX); return JRR_ERR_HIP; }
  DepthArgs q{verts, faces, points, dist, wind, face, status, n_verts, n_faces, n_points};
  hipLaunchKernelGGL(k_point_mesh_depth, dim3((unsigned)batch), dim3(DP_THREADS), (size_t)(DP_OFF_VERTS + n_verts * 12), (hipStream_t)stream, q);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_depth_accumulate(const float* dist, const float* wind, const int32_t* group, int batch, int n_points, int n_groups,
                                    int64_t* acc, void* stream) {
  if (!dist || !wind || !acc || batch < 0 || !acc_aligned(acc)) {
    jrr_set_error("jrr_depth_accumulate: bad argument");
    return JRR_ERR_ARG;
  }
  if (!acc_groups_ok(n_groups) || n_points < 1 || n_points > JRR_DEPTH_MAX_POINTS) {
    jrr_set_error("jrr_depth_accumulate: %d groups of %d points: 1 .. %d groups, 1 .. %d points", n_groups, n_points, (int)JRR_EVAL_ACC_MAX_GROUPS,
                  (int)JRR_DEPTH_MAX_POINTS);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  const int per = DP_ACC_THREADS / 64;
  hipLaunchKernelGGL(k_depth_accumulate, dim3((unsigned)((batch + per - 1) / per)), dim3(DP_ACC_THREADS), 0, (hipStream_t)stream, dist, wind, group,
                     n_points, n_groups, reinterpret_cast<long long*>(acc), batch);
  CHECK_LAUNCH();
  return JRR_OK;
}
