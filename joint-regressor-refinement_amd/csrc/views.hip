// Refined poses across the camera views of one instant (`--fuse_refined`): the constant relative orientation of each camera to its
// scene's reference camera, and the views of every frame fused into one body pose.  Both kernels read the refined-pose table of
// export.hip (include/jrr.h, JRR_EXPORT_*) through host-made lists -- `order` (table rows sorted by scene, frame, camera), `group` (the
// (scene, frame) of each position) and `pair` (its (scene, camera), or -1) -- and never write it.
//
// A position is VALID when its `order` entry lies in the table, the row's marker is 1.0f, its pair id is below n_pairs and no position
//   8 places before or behind it carries its group id; every other position raises its status bit (JRR_FUSE_STATUS_*), is nobody's
//   member, and its own outputs are NaN or 0.  The MEMBERS of a position's group are the valid positions within 7 places of it that carry
//   its group id, in ascending position order: at most JRR_FUSE_MAX_VIEWS = 8.
// unit quaternion of a joint: quat.h, exactly as smooth.hip computes it.
// k_view_relrot: one thread per position p with c = pair[p] >= 0 and ref_pair[c] != c.  The first member whose pair is ref_pair[c]
//   gives e = q_ref(joint 0) (x) conj(q_p(joint 0)), the quaternion of R_ref R_p^T; acc[c] += 1 and llrintf((e_i * e_j) * 2^24) for the
//   ten products ww wx wy wz xx xy xz yy yz zz -- even in e, so its sign does not matter.  Integer atomics only: the table is a function of
//   the multiset of positions.  A non-finite e is not counted.
// k_view_fuse: a workgroup owns VF_TILE = 32 consecutive positions.  It stages the 32 + 2 x 7 slots around them (row or -1, group,
//   pair), their unit quaternions (46 x 24 x 16 B), for joint 0 the rig-corrected q' = d_pair (x) q with d = rel[pair] (and whether the
//   slot is a candidate there: pair >= 0 and d non-zero), and their betas ONCE in LDS, and then works with one thread per (position,
//   joint); see include/jrr.h for the definition.  The 6-D rows leave through LDS as float4, as in k_pose_smooth.
//   A position's result is a function of its group alone: slots are addressed relative to the position, nothing depends on M, on the
//   position's place in the tile or on the launch's position range.
#include "jrr_common.h"
#include "rot6.h"
#include "quat.h"
#include "acctab.h"
#include "../../include/jrr.h"

// rot6d_fwd, included above, keeps the default contraction it has in the loop's kernels; everything below is rounded once per operation,
// in the order written (quat.h says so for its helpers; said again here for this file's own arithmetic)
#pragma clang fp contract(off)

namespace jrr {

constexpr int VF_TILE = JRR_FUSE_TILE;                        // positions per workgroup
constexpr int VF_HALO = JRR_FUSE_MAX_VIEWS - 1;               // 7: how far a member can lie from its position
constexpr int VF_THREADS = VF_TILE * JRR_NUM_JOINTS;          // 768: one thread per (position, joint)
constexpr int VF_SLOTS = VF_TILE + 2 * VF_HALO;               // 46 rows a tile can see
constexpr int VF_X4 = JRR_NUM_JOINTS * 6 / 4;                 // 36 float4 per 6-D output row
constexpr int VF_RR_THREADS = 64;
constexpr float VF_FIX = 16777216.f;                          // 2^24
static_assert(JRR_FUSE_TILE == 32 && JRR_FUSE_MAX_VIEWS == 8 && JRR_FUSE_ACC_ROW == 12, "include/jrr.h");
static_assert((JRR_EXPORT_ROW * 4) % 8 == 0 && (JRR_EXPORT_POSE6D * 4) % 8 == 0, "the 6-D values of a joint are 8-byte aligned");
static_assert(VF_THREADS <= 1024 && JRR_NUM_JOINTS * 6 % 4 == 0, "tile shape");

// position p of the lists: its table row, group and pair; -1 when p lies outside [0, M) or is refused with a status bit
__device__ __forceinline__ int view_row(const float* __restrict__ table, long long n_rows, const int* __restrict__ order,
                                        const int* __restrict__ group, const int* __restrict__ pair, int n_pairs, int M, int p,
                                        int* __restrict__ status, int& g, int& c) {
  g = 0;
  c = -1;
  if (p < 0 || p >= M) return -1;
  const int o = order[p], gp = group[p], cp = pair[p];
  int bits = 0;
  if (o < 0 || (long long)o >= n_rows) bits |= JRR_FUSE_STATUS_INDEX;
  else if (table[(size_t)o * JRR_EXPORT_ROW + JRR_EXPORT_MARKER] != 1.0f) bits |= JRR_FUSE_STATUS_MARKER;
  if (cp >= n_pairs) bits |= JRR_FUSE_STATUS_PAIR;
  if ((p >= JRR_FUSE_MAX_VIEWS && group[p - JRR_FUSE_MAX_VIEWS] == gp) || (p < M - JRR_FUSE_MAX_VIEWS && group[p + JRR_FUSE_MAX_VIEWS] == gp))
    bits |= JRR_FUSE_STATUS_WIDE;
  if (bits) {
    atomicOr(status, bits);
    return -1;
  }
  g = gp;
  c = cp < 0 ? -1 : cp;
  return o;
}

__device__ __forceinline__ Quat joint_quat(const float* __restrict__ table, int row, int j) {
  const float2* x2 = reinterpret_cast<const float2*>(table + (size_t)row * JRR_EXPORT_ROW + JRR_EXPORT_POSE6D + j * 6);
  float xv[6], Rv[9];
  Rot6 c;
#pragma unroll
  for (int k = 0; k < 3; ++k) { const float2 v = x2[k]; xv[2 * k] = v.x; xv[2 * k + 1] = v.y; }
  rot6d_fwd(xv, Rv, c);
  return unit_quat(Rv);
}

// a (x) b
__device__ __forceinline__ Quat qmul(const Quat& a, const Quat& b) {
  Quat e;
  e.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  e.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  e.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
  e.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
  return e;
}

__device__ __forceinline__ Quat load_quat(const float4* s_q, int i) {
  const float4 v = s_q[i];
  Quat q; q.w = v.x; q.x = v.y; q.y = v.z; q.z = v.w;
  return q;
}

// grid: ceil(count / 64) workgroups of 64 threads, one position per thread
__global__ __launch_bounds__(VF_RR_THREADS) void k_view_relrot(const float* __restrict__ table, long long n_rows, const int* __restrict__ order,
                                                               const int* __restrict__ group, const int* __restrict__ pair,
                                                               const int* __restrict__ ref_pair, int n_pairs, int M, int begin, int count,
                                                               long long* __restrict__ acc, int* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int p = begin + i;
  int g, c;
  const int row = view_row(table, n_rows, order, group, pair, n_pairs, M, p, status, g, c);
  if (row < 0 || c < 0) return;
  const int r = ref_pair[c];
  if (r == c) return;
  if (r < 0 || r >= n_pairs) {
    atomicOr(status, JRR_FUSE_STATUS_PAIR);
    return;
  }
  int row_ref = -1;
  for (int k = -VF_HALO; k <= VF_HALO && row_ref < 0; ++k) {
    const int n = p + k;
    if (k == 0 || n < 0 || n >= M || group[n] != g || pair[n] != r) continue;
    int gn, cn;
    row_ref = view_row(table, n_rows, order, group, pair, n_pairs, M, n, status, gn, cn);
  }
  if (row_ref < 0) return;
  const Quat qr = joint_quat(table, row_ref, 0), qp = joint_quat(table, row, 0);
  Quat qc;
  qc.w = qp.w; qc.x = -qp.x; qc.y = -qp.y; qc.z = -qp.z;
  const Quat e = qmul(qr, qc);
  const float ev[4] = {e.w, e.x, e.y, e.z};
  if (!(fabsf(e.w) <= 2.f && fabsf(e.x) <= 2.f && fabsf(e.y) <= 2.f && fabsf(e.z) <= 2.f)) return;
  long long* out = acc + (size_t)c * JRR_FUSE_ACC_ROW;
  acc_add(out, 1);
  int w = 1;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = a; b < 4; ++b) {
      const float prod = ev[a] * ev[b];
      acc_add(out + w, llrintf(prod * VF_FIX));
      ++w;
    }
}

// grid: ceil(count / 32) workgroups of 768 threads; workgroup b owns positions p0 = begin + 32 b .. min(p0 + 32, begin + count)
__global__ __launch_bounds__(VF_THREADS) void k_view_fuse(const float* __restrict__ table, long long n_rows, const int* __restrict__ order,
                                                          const int* __restrict__ group, const int* __restrict__ pair,
                                                          const float* __restrict__ rel, int n_pairs, int M, float cos_half_max, int begin,
                                                          int count, float* __restrict__ x6d_out, float* __restrict__ betas_out,
                                                          float* __restrict__ delta_body_deg, float* __restrict__ delta_orient_deg,
                                                          int* __restrict__ members_out, int* __restrict__ dropped_out,
                                                          int* __restrict__ status) {
  __shared__ float4 s_q[VF_SLOTS * JRR_NUM_JOINTS];           // 17 664 B
  __shared__ float4 s_x4[VF_TILE * VF_X4];                    // 18 432 B: the tile's 6-D output rows
  __shared__ float4 s_q0[VF_SLOTS], s_d[VF_SLOTS];            // joint 0 in the reference camera's frame; the slot's d
  __shared__ float s_ang[VF_TILE * JRR_NUM_JOINTS];
  __shared__ int s_drop[VF_TILE * JRR_NUM_JOINTS];
  __shared__ float s_b[VF_SLOTS * JRR_NUM_BETAS];
  __shared__ int s_row[VF_SLOTS], s_grp[VF_SLOTS], s_cand0[VF_SLOTS];
  const int tid = threadIdx.x;
  const int p0 = begin + (int)blockIdx.x * VF_TILE;
  const int npos = min(VF_TILE, begin + count - p0);
  for (int i = tid; i < VF_SLOTS; i += VF_THREADS) {
    int g, c;
    s_row[i] = view_row(table, n_rows, order, group, pair, n_pairs, M, p0 - VF_HALO + i, status, g, c);
    s_grp[i] = g;
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c >= 0) d = reinterpret_cast<const float4*>(rel)[c];
    s_d[i] = d;
    s_cand0[i] = (c >= 0 && (d.x != 0.f || d.y != 0.f || d.z != 0.f || d.w != 0.f)) ? 1 : 0;
  }
  __syncthreads();
  for (int i = tid; i < VF_SLOTS * JRR_NUM_JOINTS; i += VF_THREADS) {
    const int slot = i / JRR_NUM_JOINTS, j = i - slot * JRR_NUM_JOINTS;
    const int row = s_row[slot];
    if (row < 0) continue;
    const Quat q = joint_quat(table, row, j);
    s_q[i] = make_float4(q.w, q.x, q.y, q.z);
    if (j == 0) {
      const Quat e = qmul(load_quat(s_d, slot), q);
      s_q0[slot] = make_float4(e.w, e.x, e.y, e.z);
    }
  }
  for (int i = tid; i < VF_SLOTS * JRR_NUM_BETAS; i += VF_THREADS) {
    const int slot = i / JRR_NUM_BETAS, v = i - slot * JRR_NUM_BETAS;
    const int row = s_row[slot];
    if (row >= 0) s_b[i] = table[(size_t)row * JRR_EXPORT_ROW + JRR_EXPORT_BETAS + v];
  }
  __syncthreads();

  const float nanv = __int_as_float(0x7fc00000);
  {                                                           // thread (pp, j): joint j of position p0 + pp
    const int pp = tid / JRR_NUM_JOINTS, j = tid - pp * JRR_NUM_JOINTS;
    const int c = VF_HALO + pp;
    if (pp < npos) {
      float x[6] = {nanv, nanv, nanv, nanv, nanv, nanv}, ang = nanv;
      int drop = 0;
      const int row = s_row[c];
      if (row >= 0) {
        const int g0 = s_grp[c];
        const float4* qs = j == 0 ? s_q0 : s_q + j;           // the candidates' quaternions: qs[slot * stride]
        const int stride = j == 0 ? 1 : JRR_NUM_JOINTS;
        unsigned cand = 0;                                    // bit k + 7: offset k is a candidate
        for (int k = -VF_HALO; k <= VF_HALO; ++k) {
          const int slot = c + k;
          if (s_row[slot] >= 0 && s_grp[slot] == g0 && (j != 0 || s_cand0[slot])) cand |= 1u << (k + VF_HALO);
        }
        const bool own = (cand >> VF_HALO) & 1u;
        const float2* in2 = reinterpret_cast<const float2*>(table + (size_t)row * JRR_EXPORT_ROW + JRR_EXPORT_POSE6D + j * 6);
        if (!own) {                                           // joint 0 of a view whose camera has no known d: not fused
#pragma unroll
          for (int k = 0; k < 3; ++k) { const float2 v = in2[k]; x[2 * k] = v.x; x[2 * k + 1] = v.y; }
        } else {
          int ka = 31 - __clz(cand & (0u - cand));            // the anchor's bit: the first candidate, or the medoid
          if (cos_half_max > 0.f) {
            float best = 0.f;
            bool have = false;
            for (int k = 0; k <= 2 * VF_HALO; ++k) {
              if (!((cand >> k) & 1u)) continue;
              const Quat qk = load_quat(qs, (c + k - VF_HALO) * stride);
              float cost = 0.f;
              for (int m = 0; m <= 2 * VF_HALO; ++m) {
                if (m == k || !((cand >> m) & 1u)) continue;
                cost = cost + (1.f - fabsf(qdot(qk, load_quat(qs, (c + m - VF_HALO) * stride))));
              }
              if (!have || cost < best) { best = cost; ka = k; have = true; }
            }
          }
          const Quat qa = load_quat(qs, (c + ka - VF_HALO) * stride);
          Quat s = {0.f, 0.f, 0.f, 0.f};
          int taken = 0;
          bool own_taken = false, first = true;
          for (int k = 0; k <= 2 * VF_HALO; ++k) {
            if (!((cand >> k) & 1u)) continue;
            Quat q = load_quat(qs, (c + k - VF_HALO) * stride);
            const float d = qdot(q, qa);
            if (cos_half_max > 0.f && !(fabsf(d) >= cos_half_max)) continue;
            if (d < 0.f) { q.w = -q.w; q.x = -q.x; q.y = -q.y; q.z = -q.z; }
            if (first) s = q;
            else { s.w = s.w + q.w; s.x = s.x + q.x; s.y = s.y + q.y; s.z = s.z + q.z; }
            first = false;
            ++taken;
            if (k == VF_HALO) own_taken = true;
          }
          drop = own_taken ? 0 : 1;
          const float n = sqrtf(s.w * s.w + s.x * s.x + s.y * s.y + s.z * s.z);
          s.w = s.w / n; s.x = s.x / n; s.y = s.y / n; s.z = s.z / n;
          ang = angle_deg(conj_mul(load_quat(qs, c * stride), s));
          if (taken == 1 && own_taken) {                      // nothing to fuse with: the row's own values, bit for bit
#pragma unroll
            for (int k = 0; k < 3; ++k) { const float2 v = in2[k]; x[2 * k] = v.x; x[2 * k + 1] = v.y; }
          } else {
            if (j == 0) s = conj_mul(load_quat(s_d, c), s);   // back into this view's camera frame
            // columns 0 and 1 of R(s), in rot6.h's layout: x[0], x[2], x[4] is column 0
            x[0] = 1.f - 2.f * (s.y * s.y + s.z * s.z);  x[1] = 2.f * (s.x * s.y - s.w * s.z);
            x[2] = 2.f * (s.x * s.y + s.w * s.z);        x[3] = 1.f - 2.f * (s.x * s.x + s.z * s.z);
            x[4] = 2.f * (s.x * s.z - s.w * s.y);        x[5] = 2.f * (s.y * s.z + s.w * s.x);
          }
        }
      }
      float2* o2 = reinterpret_cast<float2*>(s_x4) + (size_t)tid * 3;      // 24 B per (position, joint)
#pragma unroll
      for (int k = 0; k < 3; ++k) o2[k] = make_float2(x[2 * k], x[2 * k + 1]);
      s_ang[tid] = ang;
      s_drop[tid] = drop;
    }
  }
  // betas: thread (pp, v)
  for (int i = tid; i < npos * JRR_NUM_BETAS; i += VF_THREADS) {
    const int pp = i / JRR_NUM_BETAS, v = i - pp * JRR_NUM_BETAS;
    const int c = VF_HALO + pp;
    float out = nanv;
    if (s_row[c] >= 0) {
      const int g0 = s_grp[c];
      float acc = 0.f;
      int n = 0;
      for (int k = -VF_HALO; k <= VF_HALO; ++k) {
        const int slot = c + k;
        if (s_row[slot] < 0 || s_grp[slot] != g0) continue;
        const float t = s_b[slot * JRR_NUM_BETAS + v];
        acc = n == 0 ? t : acc + t;
        ++n;
      }
      out = acc / (float)n;
    }
    betas_out[(size_t)(p0 + pp) * JRR_NUM_BETAS + v] = out;
  }
  __syncthreads();
  if (tid < npos) {
    const int c = VF_HALO + tid;
    int n = 0, drop = 0;
    if (s_row[c] >= 0)
      for (int k = -VF_HALO; k <= VF_HALO; ++k)
        if (s_row[c + k] >= 0 && s_grp[c + k] == s_grp[c]) ++n;
    float sum = s_ang[tid * JRR_NUM_JOINTS + 1];
    for (int j = 2; j < JRR_NUM_JOINTS; ++j) sum = sum + s_ang[tid * JRR_NUM_JOINTS + j];
    for (int j = 0; j < JRR_NUM_JOINTS; ++j) drop += s_drop[tid * JRR_NUM_JOINTS + j];
    delta_body_deg[p0 + tid] = sum / (float)(JRR_NUM_JOINTS - 1);
    delta_orient_deg[p0 + tid] = s_ang[tid * JRR_NUM_JOINTS];
    members_out[p0 + tid] = n;
    dropped_out[p0 + tid] = drop;
  }
  float4* out4 = reinterpret_cast<float4*>(x6d_out) + (size_t)p0 * VF_X4;
  for (int i = tid; i < npos * VF_X4; i += VF_THREADS) out4[i] = s_x4[i];
}

}  // namespace jrr

using namespace jrr;

// what both entry points ask of the lists and the position range; NULL when everything is in order
static const char* view_lists_error(const float* table, int64_t n_rows, const int32_t* order, const int32_t* group, const int32_t* pair,
                                    const void* per_pair, int n_pairs, int m, int begin, int count, const int32_t* status) {
  if (!table || !order || !group || !pair || !status || n_pairs < 0 || (n_pairs > 0 && !per_pair)) return "bad argument";
  if (n_rows < 0 || n_rows > INT32_MAX || m < 0 || m > JRR_SMOOTH_MAX_POSITIONS) return "n_rows must lie in 0 .. 2^31 - 1, m in 0 .. 2^30";
  if (begin < 0 || count < 0 || begin > m || count > m - begin) return "the position range must lie inside [0, m)";
  if (((uintptr_t)table & 7) != 0 || (((uintptr_t)order | (uintptr_t)group | (uintptr_t)pair | (uintptr_t)status) & 3) != 0)
    return "the table must be 8-byte aligned, order, group, pair and status 4-byte aligned";
  return nullptr;
}

extern "C" int jrr_view_relrot_accumulate(const float* table, int64_t n_rows, const int32_t* order, const int32_t* group, const int32_t* pair,
                                          const int32_t* ref_pair, int n_pairs, int m, int begin, int count, int64_t* acc, int32_t* status,
                                          void* stream) {
  const char* why = view_lists_error(table, n_rows, order, group, pair, ref_pair, n_pairs, m, begin, count, status);
  if (!why && n_pairs > 0 && !acc) why = "bad argument";
  if (!why && (((uintptr_t)ref_pair & 3) != 0 || ((uintptr_t)acc & 7) != 0)) why = "ref_pair must be 4-byte aligned, acc 8-byte aligned";
  if (why) {
    jrr_set_error("jrr_view_relrot_accumulate: %s", why);
    return JRR_ERR_ARG;
  }
  if (count == 0) return JRR_OK;
  hipLaunchKernelGGL(k_view_relrot, dim3((unsigned)((count + VF_RR_THREADS - 1) / VF_RR_THREADS)), dim3(VF_RR_THREADS), 0, (hipStream_t)stream,
                     table, (long long)n_rows, order, group, pair, ref_pair, n_pairs, m, begin, count, reinterpret_cast<long long*>(acc), status);
  JRR_HIP(hipGetLastError());
  return JRR_OK;
}

extern "C" int jrr_view_fuse(const float* table, int64_t n_rows, const int32_t* order, const int32_t* group, const int32_t* pair,
                             const float* rel, int n_pairs, int m, float cos_half_max, int begin, int count, float* x6d_out, float* betas_out,
                             float* delta_body_deg, float* delta_orient_deg, int32_t* members_out, int32_t* dropped_out, int32_t* status,
                             void* stream) {
  const char* why = view_lists_error(table, n_rows, order, group, pair, rel, n_pairs, m, begin, count, status);
  if (!why && (!x6d_out || !betas_out || !delta_body_deg || !delta_orient_deg || !members_out || !dropped_out)) why = "bad argument";
  if (!why && !(cos_half_max <= 1.f)) why = "cos_half_max must be at most 1 (0 or less: the plain mean)";
  if (!why && ((((uintptr_t)x6d_out | (uintptr_t)rel) & 15) != 0 || (((uintptr_t)betas_out | (uintptr_t)delta_body_deg | (uintptr_t)delta_orient_deg |
                                                                      (uintptr_t)members_out | (uintptr_t)dropped_out) & 3) != 0))
    why = "x6d_out and rel must be 16-byte aligned, the other arrays 4-byte aligned";
  if (why) {
    jrr_set_error("jrr_view_fuse: %s", why);
    return JRR_ERR_ARG;
  }
  if (count == 0) return JRR_OK;
  hipLaunchKernelGGL(k_view_fuse, dim3((unsigned)((count + VF_TILE - 1) / VF_TILE)), dim3(VF_THREADS), 0, (hipStream_t)stream, table,
                     (long long)n_rows, order, group, pair, rel, n_pairs, m, cos_half_max, begin, count, x6d_out, betas_out, delta_body_deg,
                     delta_orient_deg, members_out, dropped_out, status);
  JRR_HIP(hipGetLastError());
  return JRR_OK;
}
