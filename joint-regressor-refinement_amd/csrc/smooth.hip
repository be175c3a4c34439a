// Refined poses along the time axis (`--smooth_refined`): a Gaussian filter over each run of consecutive frames, and the jitter it
// removes.  Both kernels read the refined-pose table of export.hip (include/jrr.h, JRR_EXPORT_*) through two host-made lists --
// `order` (table rows in time order) and `run` (the run of each position) -- and never write it.
//
// unit quaternion of a joint: the loop's own rot6d_fwd (rot6.h) of the row's six values, Shepperd's unnormalised quaternion of that
//   matrix (the branch rotmat_log of export.hip takes: of tr, R00, R11, R22 the largest, ties in that order), divided by its norm.
//   No canonical sign: every use below is invariant under q -> -q of any sample.
// k_pose_smooth: a workgroup owns SM_TILE = 32 consecutive positions.  It checks the 32 + 2 radius entries of `order` around them
//   (slot -> table row or -1), computes the unit quaternions of those rows ONCE into LDS (at most 64 rows x 24 joints x 16 B), stages
//   their betas | cam, and then filters from LDS with one thread per (position, joint):
//     s = sum_k w[|k|] * sign(q_k . q_0) q_k  over the offsets k = -radius .. radius (ascending) whose slot is a valid row of the
//     centre's run;  s . q_0 >= w[0] > 0, so |s| > 0;   q~ = s / |s|;   6-D out = the first two columns of R(q~);
//     angle = 2 atan2(|e_xyz|, |e_w|) 180 / pi of e = conj(q_0) (x) q~;   delta_deg = (sum of the 24 angles in joint order) / 24.
//   betas | cam: (sum_k w[|k|] v_k) / (sum_k w[|k|]) over the same offsets in the same order, one thread per (position, value); the sums
//   START from the first term, so radius 0 and runs of length 1 give v * 1.0f / 1.0f = v to the bit (-0.0 included).
//   The 6-D rows of a tile leave through LDS as float4 (a position's 144 floats are 36 x 16 B, whatever the position); betas, cam and
//   delta_deg rows are 40, 12 and 4 bytes, so they leave as coalesced 4-byte stores.
//   A position's result is a function of its window alone: slots are addressed relative to the position, nothing depends on M, on the
//   position's place in the tile or on the launch's position range.
// k_pose_jitter: the same staging with a halo of 1; per (position, joint) the second difference of the rotation,
//   d1 = conj(q_{p-1}) (x) q_p, d2 = conj(q_p) (x) q_{p+1}, e = conj(d1) (x) d2, the angle of e as above, the mean over the joints in
//   joint order; NaN where p - 1 or p + 1 is not a valid row of p's run.
// Status bits (JRR_SMOOTH_STATUS_*): an `order` entry outside [0, n_rows), a listed row whose marker is not 1.0f.  Such a position is
//   nobody's neighbour and its own outputs are NaN.
#include "jrr_common.h"
#include "rot6.h"
#include "quat.h"
#include "../../include/jrr.h"

namespace jrr {

constexpr int SM_TILE = 32;                                   // positions per workgroup
constexpr int SM_THREADS = SM_TILE * JRR_NUM_JOINTS;          // 768: one thread per (position, joint)
constexpr int SM_SLOTS = SM_TILE + 2 * JRR_SMOOTH_MAX_RADIUS; // 64 rows a tile can see
constexpr int SM_BC = JRR_NUM_BETAS + 3;                      // betas | cam: 13 contiguous floats of a row
constexpr int SM_X4 = JRR_NUM_JOINTS * 6 / 4;                 // 36 float4 per 6-D output row
static_assert(JRR_EXPORT_CAM == JRR_EXPORT_BETAS + JRR_NUM_BETAS && JRR_EXPORT_MARKER == JRR_EXPORT_CAM + 3, "betas | cam | marker are contiguous");
static_assert((JRR_EXPORT_ROW * 4) % 8 == 0 && (JRR_EXPORT_POSE6D * 4) % 8 == 0, "the 6-D values of a joint are 8-byte aligned");
static_assert(SM_THREADS <= 1024 && JRR_NUM_JOINTS * 6 % 4 == 0, "tile shape");

// slot i <-> position first + i: its table row (-1: outside [0, M), or refused with a status bit) and its run
__device__ __forceinline__ void stage_slots(const float* __restrict__ table, long long n_rows, const int* __restrict__ order,
                                            const int* __restrict__ run, int M, int first, int nslots, int* s_row, int* s_run,
                                            int* __restrict__ status) {
  for (int i = threadIdx.x; i < nslots; i += blockDim.x) {
    const int p = first + i;
    int row = -1, r = 0;
    if (p >= 0 && p < M) {
      const int o = order[p];
      if (o < 0 || (long long)o >= n_rows) atomicOr(status, JRR_SMOOTH_STATUS_INDEX);
      else if (table[(size_t)o * JRR_EXPORT_ROW + JRR_EXPORT_MARKER] != 1.0f) atomicOr(status, JRR_SMOOTH_STATUS_MARKER);
      else { row = o; r = run[p]; }
    }
    s_row[i] = row;
    s_run[i] = r;
  }
}

// quat.h switched contraction off: everything below is rounded once per operation, in the order written

// the unit quaternions of the staged slots' rows: s_q[slot * 24 + joint] (untouched for a slot without row: never read)
__device__ __forceinline__ void stage_quats(const float* __restrict__ table, int nslots, const int* s_row, float4* s_q) {
  for (int i = threadIdx.x; i < nslots * JRR_NUM_JOINTS; i += blockDim.x) {
    const int slot = i / JRR_NUM_JOINTS, j = i - slot * JRR_NUM_JOINTS;
    const int row = s_row[slot];
    if (row < 0) continue;
    const float2* x2 = reinterpret_cast<const float2*>(table + (size_t)row * JRR_EXPORT_ROW + JRR_EXPORT_POSE6D + j * 6);
    float xv[6], Rv[9];
    Rot6 c;
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float2 v = x2[k]; xv[2 * k] = v.x; xv[2 * k + 1] = v.y; }
    rot6d_fwd(xv, Rv, c);
    const Quat q = unit_quat(Rv);
    s_q[i] = make_float4(q.w, q.x, q.y, q.z);
  }
}

__device__ __forceinline__ Quat load_quat(const float4* s_q, int i) {
  const float4 v = s_q[i];
  Quat q; q.w = v.x; q.x = v.y; q.y = v.z; q.z = v.w;
  return q;
}

// grid: ceil(count / 32) workgroups of 768 threads; workgroup b owns positions p0 = begin + 32 b .. min(p0 + 32, begin + count)
__global__ __launch_bounds__(SM_THREADS) void k_pose_smooth(const float* __restrict__ table, long long n_rows, const int* __restrict__ order,
                                                            const int* __restrict__ run, int M, const float* __restrict__ weights, int radius,
                                                            int begin, int count, float* __restrict__ x6d_out, float* __restrict__ betas_out,
                                                            float* __restrict__ cam_out, float* __restrict__ delta_deg, int* __restrict__ status) {
  __shared__ float4 s_q[SM_SLOTS * JRR_NUM_JOINTS];           // 24 576 B
  __shared__ float4 s_x4[SM_TILE * SM_X4];                    // 18 432 B: the tile's 6-D output rows
  __shared__ float s_ang[SM_TILE * JRR_NUM_JOINTS];
  __shared__ float s_bc[SM_SLOTS * SM_BC];
  __shared__ int s_row[SM_SLOTS], s_run[SM_SLOTS];
  __shared__ float s_w[JRR_SMOOTH_MAX_RADIUS + 1];
  const int tid = threadIdx.x;
  const int p0 = begin + (int)blockIdx.x * SM_TILE;
  const int npos = min(SM_TILE, begin + count - p0);
  const int nslots = SM_TILE + 2 * radius;
  if (tid <= radius) s_w[tid] = weights[tid];
  stage_slots(table, n_rows, order, run, M, p0 - radius, nslots, s_row, s_run, status);
  __syncthreads();
  stage_quats(table, nslots, s_row, s_q);
  for (int i = tid; i < nslots * SM_BC; i += SM_THREADS) {
    const int slot = i / SM_BC, c = i - slot * SM_BC;
    const int row = s_row[slot];
    if (row >= 0) s_bc[i] = table[(size_t)row * JRR_EXPORT_ROW + JRR_EXPORT_BETAS + c];
  }
  __syncthreads();

  const float nanv = __int_as_float(0x7fc00000);
  {                                                           // thread (pp, j): joint j of position p0 + pp
    const int pp = tid / JRR_NUM_JOINTS, j = tid - pp * JRR_NUM_JOINTS;
    const int c = radius + pp;
    if (pp < npos) {
      float x[6] = {nanv, nanv, nanv, nanv, nanv, nanv}, ang = nanv;
      if (s_row[c] >= 0) {
        const int r0 = s_run[c];
        const Quat q0 = load_quat(s_q, c * JRR_NUM_JOINTS + j);
        Quat s = {0.f, 0.f, 0.f, 0.f};
        for (int k = -radius; k <= radius; ++k) {
          const int slot = c + k;
          if (s_row[slot] < 0 || s_run[slot] != r0) continue;
          Quat q = load_quat(s_q, slot * JRR_NUM_JOINTS + j);
          if (qdot(q, q0) < 0.f) { q.w = -q.w; q.x = -q.x; q.y = -q.y; q.z = -q.z; }
          const float w = s_w[k < 0 ? -k : k];
          s.w = s.w + w * q.w; s.x = s.x + w * q.x; s.y = s.y + w * q.y; s.z = s.z + w * q.z;
        }
        const float n = sqrtf(s.w * s.w + s.x * s.x + s.y * s.y + s.z * s.z);
        s.w = s.w / n; s.x = s.x / n; s.y = s.y / n; s.z = s.z / n;
        // columns 0 and 1 of R(s), in rot6.h's layout: x[0], x[2], x[4] is column 0
        x[0] = 1.f - 2.f * (s.y * s.y + s.z * s.z);  x[1] = 2.f * (s.x * s.y - s.w * s.z);
        x[2] = 2.f * (s.x * s.y + s.w * s.z);        x[3] = 1.f - 2.f * (s.x * s.x + s.z * s.z);
        x[4] = 2.f * (s.x * s.z - s.w * s.y);        x[5] = 2.f * (s.y * s.z + s.w * s.x);
        ang = angle_deg(conj_mul(q0, s));
      }
      float2* o2 = reinterpret_cast<float2*>(s_x4) + (size_t)tid * 3;      // 24 B per (position, joint)
#pragma unroll
      for (int k = 0; k < 3; ++k) o2[k] = make_float2(x[2 * k], x[2 * k + 1]);
      s_ang[tid] = ang;
    }
  }
  // betas | cam: thread (pp, v)
  for (int i = tid; i < npos * SM_BC; i += SM_THREADS) {
    const int pp = i / SM_BC, v = i - pp * SM_BC;
    const int c = radius + pp, p = p0 + pp;
    float out = nanv;
    if (s_row[c] >= 0) {
      const int r0 = s_run[c];
      float acc = 0.f, wsum = 0.f;
      bool first = true;
      for (int k = -radius; k <= radius; ++k) {
        const int slot = c + k;
        if (s_row[slot] < 0 || s_run[slot] != r0) continue;
        const float w = s_w[k < 0 ? -k : k], t = w * s_bc[slot * SM_BC + v];
        acc = first ? t : acc + t;
        wsum = first ? w : wsum + w;
        first = false;
      }
      out = acc / wsum;
    }
    if (v < JRR_NUM_BETAS) betas_out[(size_t)p * JRR_NUM_BETAS + v] = out;
    else cam_out[(size_t)p * 3 + (v - JRR_NUM_BETAS)] = out;
  }
  __syncthreads();
  if (tid < npos) {
    float sum = s_ang[tid * JRR_NUM_JOINTS];
    for (int j = 1; j < JRR_NUM_JOINTS; ++j) sum = sum + s_ang[tid * JRR_NUM_JOINTS + j];
    delta_deg[p0 + tid] = sum / (float)JRR_NUM_JOINTS;
  }
  float4* out4 = reinterpret_cast<float4*>(x6d_out) + (size_t)p0 * SM_X4;
  for (int i = tid; i < npos * SM_X4; i += SM_THREADS) out4[i] = s_x4[i];
}

// grid and ownership as k_pose_smooth; halo 1
__global__ __launch_bounds__(SM_THREADS) void k_pose_jitter(const float* __restrict__ table, long long n_rows, const int* __restrict__ order,
                                                            const int* __restrict__ run, int M, int begin, int count,
                                                            float* __restrict__ jitter_deg, int* __restrict__ status) {
  constexpr int NS = SM_TILE + 2;
  __shared__ float4 s_q[NS * JRR_NUM_JOINTS];
  __shared__ float s_ang[SM_TILE * JRR_NUM_JOINTS];
  __shared__ int s_row[NS], s_run[NS];
  const int tid = threadIdx.x;
  const int p0 = begin + (int)blockIdx.x * SM_TILE;
  const int npos = min(SM_TILE, begin + count - p0);
  stage_slots(table, n_rows, order, run, M, p0 - 1, NS, s_row, s_run, status);
  __syncthreads();
  stage_quats(table, NS, s_row, s_q);
  __syncthreads();
  const int pp = tid / JRR_NUM_JOINTS, j = tid - pp * JRR_NUM_JOINTS;
  const int c = 1 + pp;
  if (pp < npos) {
    float ang = __int_as_float(0x7fc00000);
    if (s_row[c] >= 0 && s_row[c - 1] >= 0 && s_row[c + 1] >= 0 && s_run[c - 1] == s_run[c] && s_run[c + 1] == s_run[c]) {
      const Quat qa = load_quat(s_q, (c - 1) * JRR_NUM_JOINTS + j), qb = load_quat(s_q, c * JRR_NUM_JOINTS + j),
                 qc = load_quat(s_q, (c + 1) * JRR_NUM_JOINTS + j);
      ang = angle_deg(conj_mul(conj_mul(qa, qb), conj_mul(qb, qc)));
    }
    s_ang[tid] = ang;
  }
  __syncthreads();
  if (tid < npos) {
    float sum = s_ang[tid * JRR_NUM_JOINTS];
    for (int k = 1; k < JRR_NUM_JOINTS; ++k) sum = sum + s_ang[tid * JRR_NUM_JOINTS + k];
    jitter_deg[p0 + tid] = sum / (float)JRR_NUM_JOINTS;
  }
}

}  // namespace jrr

using namespace jrr;

// what both entry points ask of the lists and the position range; NULL when everything is in order
static const char* smooth_lists_error(const float* table, int64_t n_rows, const int32_t* order, const int32_t* run, int m, int begin, int count,
                                      const int32_t* status) {
  if (!table || !order || !run || !status) return "bad argument";
  if (n_rows < 0 || n_rows > INT32_MAX || m < 0 || m > JRR_SMOOTH_MAX_POSITIONS) return "n_rows must lie in 0 .. 2^31 - 1, m in 0 .. 2^24";
  if (begin < 0 || count < 0 || begin > m || count > m - begin) return "the position range must lie inside [0, m)";
  if (((uintptr_t)table & 7) != 0 || (((uintptr_t)order | (uintptr_t)run | (uintptr_t)status) & 3) != 0)
    return "the table must be 8-byte aligned, order, run and status 4-byte aligned";
  return nullptr;
}

extern "C" int jrr_pose_smooth(const float* table, int64_t n_rows, const int32_t* order, const int32_t* run, int m, const float* weights,
                               int radius, int begin, int count, float* x6d_out, float* betas_out, float* cam_out, float* delta_deg,
                               int32_t* status, void* stream) {
  const char* why = smooth_lists_error(table, n_rows, order, run, m, begin, count, status);
  if (!why && (!weights || !x6d_out || !betas_out || !cam_out || !delta_deg)) why = "bad argument";
  if (why) {
    jrr_set_error("jrr_pose_smooth: %s", why);
    return JRR_ERR_ARG;
  }
  if (radius < 0 || radius > JRR_SMOOTH_MAX_RADIUS) {
    jrr_set_error("jrr_pose_smooth: radius %d: 0 .. %d", radius, (int)JRR_SMOOTH_MAX_RADIUS);
    return JRR_ERR_ARG;
  }
  if (((uintptr_t)x6d_out & 15) != 0 || (((uintptr_t)weights | (uintptr_t)betas_out | (uintptr_t)cam_out | (uintptr_t)delta_deg) & 3) != 0) {
    jrr_set_error("jrr_pose_smooth: x6d_out must be 16-byte aligned, the other arrays 4-byte aligned");
    return JRR_ERR_ARG;
  }
  if (count == 0) return JRR_OK;
  hipLaunchKernelGGL(k_pose_smooth, dim3((unsigned)((count + SM_TILE - 1) / SM_TILE)), dim3(SM_THREADS), 0, (hipStream_t)stream, table,
                     (long long)n_rows, order, run, m, weights, radius, begin, count, x6d_out, betas_out, cam_out, delta_deg, status);
  JRR_HIP(hipGetLastError());
  return JRR_OK;
}

extern "C" int jrr_pose_jitter(const float* table, int64_t n_rows, const int32_t* order, const int32_t* run, int m, int begin, int count,
                               float* jitter_deg, int32_t* status, void* stream) {
  const char* why = smooth_lists_error(table, n_rows, order, run, m, begin, count, status);
  if (!why && !jitter_deg) why = "bad argument";
  if (!why && ((uintptr_t)jitter_deg & 3) != 0) why = "jitter_deg must be 4-byte aligned";
  if (why) {
    jrr_set_error("jrr_pose_jitter: %s", why);
    return JRR_ERR_ARG;
  }
  if (count == 0) return JRR_OK;
  hipLaunchKernelGGL(k_pose_jitter, dim3((unsigned)((count + SM_TILE - 1) / SM_TILE)), dim3(SM_THREADS), 0, (hipStream_t)stream, table,
                     (long long)n_rows, order, run, m, begin, count, jitter_deg, status);
  JRR_HIP(hipGetLastError());
  return JRR_OK;
}
