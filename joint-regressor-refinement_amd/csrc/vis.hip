// What the real camera sees of a placed body (`--visible_refined`): per query point the number of faces of the pose's own mesh that
// cross the ray from the camera centre in front of it, the pixel against the window, and the report's table.  Two launches, no engine,
// no body model (the caller brings the faces).  include/jrr.h (jrr_point_visibility, jrr_visibility_accumulate, JRR_VIS_*) is the
// specification; DESIGN.md section 3v has the reasons.
//
// k_point_visibility        one workgroup of 4 waves per (pose, block of 256 queries), one query per lane, in registers.  The faces
//                           come in chunks of 256: thread t gathers face 256 c + t of the pose (three indices, nine floats, asked for
//                           one chunk ahead of their use), forms what the ray test needs of the FACE ALONE -- a, e1 = b - a,
//                           e2 = c - a, q = e1 x a, s = e2 . q, with b and c swapped where that makes s positive -- and leaves it in
//                           LDS as a record of 16 dwords with the three indices.  Every wave then walks the 256 records with four
//                           broadcast 16-byte reads each and does the Moeller-Trumbore test with origin 0 on its lane's query:
//                           h = p x e2, det = e1 . h, the three barycentric numerators, and the depth test as a sign, no division.
//                           s > 0 in the record makes `det > 0` the only sign a crossing can have.  A face that must add nothing
//                           (index out of range, non-finite corner, zero normal, s <= 0) is a record of zeros: det = 0 for it.
//                           Per-lane integer counts, no cross-lane step: a query's result does not know the batch, its column or
//                           the launch.  The arithmetic works on differences (e1, e2) and on a; no triple product of raw
//                           camera-frame corners is formed.
// k_visibility_accumulate   one workgroup per pose: the pose's vertex counts and part counts in LDS, then its row of the group table
//                           (JRR_VIS_ACC_*) and the per-vertex counts.  Integer atomics only: the tables do not depend on the order,
//                           the split into calls or the sharding over ranks.
#pragma clang fp contract(off)
#include "jrr_common.h"
#include "acctab.h"
#include "../../include/jrr.h"

namespace jrr {

constexpr int VS_THREADS = 256;                    // queries per workgroup: one per lane
constexpr int VS_CHUNK = 256;                      // faces per chunk: one record per thread, 16 KiB of LDS
constexpr int VS_ACC_THREADS = 256;
constexpr float VS_FINITE = 3.402823466e+38f;      // FLT_MAX: |x| <= VS_FINITE: neither NaN nor infinite
constexpr float VS_ERR_CAP = 1.0e5f;               // mm: an error that fails e < VS_ERR_CAP (NaN, inf, absurd) makes its pose bad

static_assert(VS_CHUNK == VS_THREADS, "one record per thread");
static_assert(JRR_VIS_MAX_POINTS == 65536 && JRR_VIS_MAX_POINTS / VS_THREADS <= 65535, "grid.y");
static_assert(JRR_VIS_ACC_SUM_VERT_SEEN == 2 && JRR_VIS_ACC_SUM_VERT_OCCLUDED == 3 && JRR_VIS_ACC_SUM_VERT_OUTSIDE == 4 && JRR_VIS_ACC_J_SEEN == 5 &&
              JRR_VIS_ACC_J_OCCLUDED == JRR_VIS_ACC_J_SEEN + NH && JRR_VIS_ACC_J_OUTSIDE == JRR_VIS_ACC_J_OCCLUDED + NH &&
              JRR_VIS_ACC_SUM_ERR_SEEN == JRR_VIS_ACC_J_OUTSIDE + NH && JRR_VIS_ACC_SUM_ERR_OCCLUDED == JRR_VIS_ACC_SUM_ERR_SEEN + NH &&
              JRR_VIS_ACC_PART_SEEN == JRR_VIS_ACC_SUM_ERR_OCCLUDED + NH && JRR_VIS_ACC_PART_ALL == JRR_VIS_ACC_PART_SEEN + JRR_VIS_ACC_PARTS &&
              JRR_VIS_ACC_ROW == JRR_VIS_ACC_PART_ALL + JRR_VIS_ACC_PARTS && JRR_VIS_ACC_TRAILER == JRR_EVAL_ACC_TRAILER && NH == JRR_VIS_JOINTS,
              "row layout");
static_assert(JRR_VIS_OCCLUDED == 1 && JRR_VIS_OUTSIDE == 2 && JRR_VIS_INVALID == 4, "code bits");

struct VisArgs {
  const float* verts; const int* faces; const float* points; const float* K; const float* rect;
  int* count; unsigned char* code; int* status;
  float margin;
  int n_verts, n_faces, n_points, min_crossings;
};

__device__ __forceinline__ bool vs_finite(float x) { return fabsf(x) <= VS_FINITE; }

// a face as thread t holds it between its gather and its record
struct VsRaw {
  int i0, i1, i2;
  float a[3], b[3], c[3];
  bool there;                                      // the face exists and its indices are in range
};

__device__ __forceinline__ VsRaw vs_gather(const VisArgs& q, const float* V, int f, bool& oob) {
  VsRaw r;
  r.i0 = r.i1 = r.i2 = -1;
  r.there = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) r.a[k] = r.b[k] = r.c[k] = 0.f;
  if (f < q.n_faces) {
    const int* fi = q.faces + (size_t)f * 3;
    r.i0 = fi[0]; r.i1 = fi[1]; r.i2 = fi[2];
    const unsigned nv = (unsigned)q.n_verts;
    if ((unsigned)r.i0 < nv && (unsigned)r.i1 < nv && (unsigned)r.i2 < nv) {
      r.there = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        r.a[k] = V[(size_t)r.i0 * 3 + k]; r.b[k] = V[(size_t)r.i1 * 3 + k]; r.c[k] = V[(size_t)r.i2 * 3 + k];
      }
    } else {
      oob = true;
    }
  }
  return r;
}

// the record of a face: [e1.x a.x e1.y a.y] [e1.z a.z e2.x e2.y] [e2.z q.x q.y q.z] [s i0 i1 i2] (e1 and a side by side: det and a . h
// are one packed multiply-add chain); zeros for a face that adds nothing
__device__ __forceinline__ void vs_record(const VsRaw& r, float4* rec) {
  bool ok = r.there;
#pragma unroll
  for (int k = 0; k < 3; ++k) ok = ok && vs_finite(r.a[k]) && vs_finite(r.b[k]) && vs_finite(r.c[k]);
  float e1[3], e2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { e1[k] = r.b[k] - r.a[k]; e2[k] = r.c[k] - r.a[k]; }
  const float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  ok = ok && (n[0] != 0.f || n[1] != 0.f || n[2] != 0.f);
  // s = e2 . (e1 x a) = -(a . n): the sign every crossing's det shares.  Swapping b and c turns both around.
  const bool swap = (r.a[0] * n[0] + r.a[1] * n[1] + r.a[2] * n[2]) > 0.f;
  if (swap) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float t = e1[k]; e1[k] = e2[k]; e2[k] = t; }
  }
  const float q[3] = {e1[1] * r.a[2] - e1[2] * r.a[1], e1[2] * r.a[0] - e1[0] * r.a[2], e1[0] * r.a[1] - e1[1] * r.a[0]};
  const float s = e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2];
  ok = ok && s > 0.f && vs_finite(s);
  const float z = 0.f;
  rec[0] = ok ? make_float4(e1[0], r.a[0], e1[1], r.a[1]) : make_float4(z, z, z, z);
  rec[1] = ok ? make_float4(e1[2], r.a[2], e2[0], e2[1]) : make_float4(z, z, z, z);
  rec[2] = ok ? make_float4(e2[2], q[0], q[1], q[2]) : make_float4(z, z, z, z);
  rec[3] = make_float4(ok ? s : z, __int_as_float(r.i0), __int_as_float(r.i1), __int_as_float(r.i2));
}

// grid: (pose, block of VS_THREADS queries).  SELF: the queries are the pose's own vertices, and a face that names the query is skipped
template <bool SELF>
__global__ __launch_bounds__(VS_THREADS) void k_point_visibility(VisArgs q) {
  __shared__ float4 s_rec[VS_CHUNK * 4];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const int pt = blockIdx.y * VS_THREADS + tid;
  const float* V = q.verts + b * (size_t)q.n_verts * 3;
  // a lane beyond n_points repeats the last query (its result is never stored)
  const float* pp = (SELF ? V : q.points + b * (size_t)q.n_points * 3) + (size_t)min(pt, q.n_points - 1) * 3;
  const float px = pp[0], py = pp[1], pz = pp[2];
  const float dm = pz - q.margin;                  // a crossing lies in front when its depth s d stays below this

  int cnt = 0;
  bool oob = false;
  const int n_chunks = (q.n_faces + VS_CHUNK - 1) / VS_CHUNK;
  VsRaw raw = vs_gather(q, V, tid, oob);
  for (int c = 0; c < n_chunks; ++c) {             // uniform over the workgroup
    __syncthreads();                               // the walk of the chunk before is over
    vs_record(raw, s_rec + tid * 4);
    __syncthreads();
    if (c + 1 < n_chunks) raw = vs_gather(q, V, (c + 1) * VS_CHUNK + tid, oob);      // in flight during the walk
    const int nf = min(VS_CHUNK, q.n_faces - c * VS_CHUNK);
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(4)
    for (int k = 0; k < nf; ++k) {
      const float4 r0 = s_rec[4 * k], r1 = s_rec[4 * k + 1], r2 = s_rec[4 * k + 2], r3 = s_rec[4 * k + 3];
      const float e1x = r0.x, ax = r0.y, e1y = r0.z, ay = r0.w, e1z = r1.x, az = r1.y, e2x = r1.z, e2y = r1.w, e2z = r2.x;
      const float hx = fmaf(py, e2z, -(pz * e2y)), hy = fmaf(pz, e2x, -(px * e2z)), hz = fmaf(px, e2y, -(py * e2x));
      const float det = fmaf(e1z, hz, fmaf(e1y, hy, e1x * hx));
      const float ah = fmaf(az, hz, fmaf(ay, hy, ax * hx));                  // -lambda1 det
      const float vn = fmaf(pz, r2.w, fmaf(py, r2.z, px * r2.y));            // lambda2 det
      const float wn = (det + ah) - vn;                                      // lambda0 det
      const float front = fmaf(dm, det, -(r3.x * pz));                       // (d - margin - s d) det
      int hit = (int)(fminf(fminf(-ah, vn), wn) >= 0.f) & (int)(fminf(det, front) > 0.f);      // no branch: the counts stay per lane
      if (SELF) hit &= (int)(__float_as_int(r3.y) != pt) & (int)(__float_as_int(r3.z) != pt) & (int)(__float_as_int(r3.w) != pt);
      cnt += hit;
    }
  }
  if (oob && blockIdx.y == 0) atomicOr(q.status, JRR_DEPTH_STATUS_INDEX);
  if (pt >= q.n_points) return;
  const bool invalid = !(vs_finite(px) && vs_finite(py) && vs_finite(pz) && pz > 0.f);
  int code = invalid ? JRR_VIS_INVALID : (cnt >= q.min_crossings ? JRR_VIS_OCCLUDED : 0);
  if (q.K && !invalid) {                           // the pixel of jrr_project_points with the translation already in the point
    const float* k = q.K + b * 9;
    const float* w = q.rect + b * 4;
    const float u = (k[0] * px) / pz + k[2], v = (k[4] * py) / pz + k[5];
    const bool inside = w[0] <= u && u < w[2] && w[1] <= v && v < w[3];
    code |= inside ? 0 : JRR_VIS_OUTSIDE;
  }
  const size_t at = b * (size_t)q.n_points + pt;
  if (q.count) q.count[at] = invalid ? 0 : cnt;
  q.code[at] = (unsigned char)code;
}

struct VisAccArgs {
  const unsigned char* vcode; const unsigned char* jcode; const float* err; const int* part; const int* pose_status; const int* group;
  long long* acc; long long* per_vertex;
  int n_verts, n_groups;
};

// grid: one workgroup per pose
__global__ __launch_bounds__(VS_ACC_THREADS) void k_visibility_accumulate(VisAccArgs q) {
  __shared__ int s_cnt[4];                         // seen, occluded, outside, codes that void the pose
  __shared__ int s_seen[JRR_VIS_ACC_PARTS], s_all[JRR_VIS_ACC_PARTS];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const int g = q.group ? q.group[b] : 0;
  if (long long* t = acc_refused(q.acc, JRR_VIS_ACC_ROW, q.n_groups, g)) { if (tid == 0) acc_add(t, 1); return; }      // uniform
  const unsigned char* vc = q.vcode + b * (size_t)q.n_verts;
  if (tid < 4) s_cnt[tid] = 0;
  if (tid < JRR_VIS_ACC_PARTS) s_seen[tid] = s_all[tid] = 0;
  __syncthreads();
  int c[4] = {0, 0, 0, 0};
  for (int v = tid; v < q.n_verts; v += VS_ACC_THREADS) {
    const int m = vc[v];
    c[0] += m == 0; c[1] += m & 1; c[2] += (m >> 1) & 1; c[3] += (m & ~3) != 0;
    const int pl = q.part ? q.part[v] : 0;
    const int w = (unsigned)pl < (unsigned)JRR_VIS_ACC_PARTS ? pl : JRR_VIS_ACC_PARTS - 1;
    atomicAdd(&s_all[w], 1);
    if (m == 0) atomicAdd(&s_seen[w], 1);
  }
  if (tid < NH) {                                  // the 17 joints: a code or an error that voids the pose
    const int m = q.jcode[b * NH + tid];
    c[3] += (m & ~3) != 0;
    if (q.err) c[3] += !(q.err[b * NH + tid] < VS_ERR_CAP);
  }
  if (tid == 0 && q.pose_status) c[3] += (q.pose_status[b] & JRR_PLACE_BAD_BITS) != 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c[k]) atomicAdd(&s_cnt[k], c[k]);
  __syncthreads();
  long long* row = acc_row(q.acc, JRR_VIS_ACC_ROW, g);
  if (s_cnt[3] != 0) { if (tid == 0) acc_add(row + JRR_VIS_ACC_BAD, 1); return; }      // a pose is counted whole or not at all
  if (tid == 0) {
    acc_add(row + JRR_VIS_ACC_COUNT, 1);
    if (s_cnt[0]) acc_add(row + JRR_VIS_ACC_SUM_VERT_SEEN, s_cnt[0]);
    if (s_cnt[1]) acc_add(row + JRR_VIS_ACC_SUM_VERT_OCCLUDED, s_cnt[1]);
    if (s_cnt[2]) acc_add(row + JRR_VIS_ACC_SUM_VERT_OUTSIDE, s_cnt[2]);
  }
  if (tid < NH) {
    const int m = q.jcode[b * NH + tid];
    const bool seen = m == 0, occluded = (m & 3) == JRR_VIS_OCCLUDED;
    if (seen) acc_add(row + JRR_VIS_ACC_J_SEEN + tid, 1);
    if (occluded) acc_add(row + JRR_VIS_ACC_J_OCCLUDED + tid, 1);
    if (m & JRR_VIS_OUTSIDE) acc_add(row + JRR_VIS_ACC_J_OUTSIDE + tid, 1);
    if (q.err && (seen || occluded))
      acc_add(row + (seen ? JRR_VIS_ACC_SUM_ERR_SEEN : JRR_VIS_ACC_SUM_ERR_OCCLUDED) + tid, err_fixed24(q.err[b * NH + tid]));
  }
  if (tid < JRR_VIS_ACC_PARTS) {
    if (s_seen[tid]) acc_add(row + JRR_VIS_ACC_PART_SEEN + tid, s_seen[tid]);
    if (s_all[tid]) acc_add(row + JRR_VIS_ACC_PART_ALL + tid, s_all[tid]);
  }
  if (q.per_vertex)
    for (int v = tid; v < q.n_verts; v += VS_ACC_THREADS)
      if (vc[v] == 0) acc_add(q.per_vertex + v, 1);
}

}  // namespace jrr

using namespace jrr;

extern "C" int jrr_point_visibility(const float* verts, int batch, int n_verts, const int32_t* faces, int n_faces, const float* points, int n_points,
                                    const float* K, const float* rect, float margin_m, int min_crossings, int32_t* count, uint8_t* code,
                                    int32_t* status, void* stream) {
  const char* why = nullptr;
  if (!verts || !faces) why = "bad argument (verts and faces are required)";
  else if (!code || !status) why = "no output: code and status are required";
  else if (batch < 0 || n_verts < 1 || n_faces < 0 || n_points < 0) why = "batch, n_faces and n_points must not be negative, n_verts at least 1";
  else if (n_points > JRR_VIS_MAX_POINTS) why = "more than 65536 points per pose";
  else if (!points && n_points != n_verts) why = "points NULL: the queries are the vertices, n_points must be n_verts";
  else if ((K == nullptr) != (rect == nullptr)) why = "K and rect go together: both or neither";
  else if ((((uintptr_t)verts | (uintptr_t)faces | (uintptr_t)points | (uintptr_t)K | (uintptr_t)rect | (uintptr_t)count | (uintptr_t)status) & 3) != 0)
    why = "misaligned pointer (4 bytes)";
  else if (!(margin_m >= 0.f && margin_m <= VS_FINITE)) why = "margin_m must be finite and not negative";
  if (why) {
    jrr_set_error("jrr_point_visibility: %s", why);
    return JRR_ERR_ARG;
  }
  if (min_crossings < 1 || min_crossings > 255) {
    jrr_set_error("jrr_point_visibility: min_crossings %d: 1 .. 255", min_crossings);
    return JRR_ERR_ARG;
  }
  if (batch == 0 || n_points == 0) return JRR_OK;
  VisArgs q{verts, faces, points, K, rect, count, code, status, margin_m, n_verts, n_faces, n_points, min_crossings};
  const dim3 grid((unsigned)batch, (unsigned)((n_points + VS_THREADS - 1) / VS_THREADS));
  if (points) hipLaunchKernelGGL(k_point_visibility<false>, grid, dim3(VS_THREADS), 0, (hipStream_t)stream, q);
  else hipLaunchKernelGGL(k_point_visibility<true>, grid, dim3(VS_THREADS), 0, (hipStream_t)stream, q);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_visibility_accumulate(const uint8_t* vert_code, const uint8_t* joint_code, const float* err_j, const int32_t* part,
                                         const int32_t* pose_status, const int32_t* group, int batch, int n_verts, int n_groups, int64_t* acc,
                                         int64_t* per_vertex, void* stream) {
  const char* why = nullptr;
  if (!vert_code || !joint_code || !acc) why = "bad argument (vert_code, joint_code and acc are required)";
  else if (batch < 0) why = "batch must not be negative";
  else if ((((uintptr_t)err_j | (uintptr_t)part | (uintptr_t)pose_status | (uintptr_t)group) & 3) != 0 || !acc_aligned(acc, per_vertex))
    why = "acc and per_vertex must be 8-byte aligned, err_j, part, pose_status and group 4-byte aligned";
  if (why) {
    jrr_set_error("jrr_visibility_accumulate: %s", why);
    return JRR_ERR_ARG;
  }
  if (!acc_groups_ok(n_groups) || n_verts < 1 || n_verts > JRR_VIS_MAX_POINTS) {
    jrr_set_error("jrr_visibility_accumulate: %d groups of %d vertices: 1 .. %d groups, 1 .. %d vertices", n_groups, n_verts,
                  (int)JRR_EVAL_ACC_MAX_GROUPS, (int)JRR_VIS_MAX_POINTS);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  VisAccArgs q{vert_code, joint_code, err_j, part, pose_status, group, reinterpret_cast<long long*>(acc), reinterpret_cast<long long*>(per_vertex),
               n_verts, n_groups};
  hipLaunchKernelGGL(k_visibility_accumulate, dim3((unsigned)batch), dim3(VS_ACC_THREADS), 0, (hipStream_t)stream, q);
  CHECK_LAUNCH();
  return JRR_OK;
}
