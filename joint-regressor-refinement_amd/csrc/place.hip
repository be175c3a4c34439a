// Placing a posed body in the real camera (`--place_refined`): the camera-frame translation of the 17 joints under per-pose
// intrinsics, the pinhole projection itself, and the report's table.  Three launches, no engine, no body model; the reference's
// create_smpl_gt.py leaves this step commented out.  include/jrr.h (jrr_place_translation, jrr_project_points, jrr_place_accumulate,
// JRR_PLACE_*) is the specification; DESIGN.md section 3u has the reasons.
//
// k_place_translation  one pose per thread, 64 poses (one wave) per workgroup.  A pose's inputs are 51 + 34 + 9 + 17 floats at strides
//                      of 204 / 136 / 36 / 68 bytes, but the 64 poses of a workgroup are ONE contiguous piece of each array: the
//                      workgroup copies the four pieces into LDS with coalesced dwords, and every thread then walks its own row
//                      there (row strides 51, 35, 9 and 17 floats: odd, conflict-free).  The joints are read from LDS again in every
//                      Levenberg-Marquardt step instead of living in 2 x 51 registers as doubles; no array is indexed in registers,
//                      nothing goes to scratch memory.  All arithmetic is fp64 with contraction off -- the depth is read off the
//                      pixel extent of a body two metres across at 3 .. 7 m, and +, -, *, / and sqrt are rounded once each, so a
//                      host restatement that keeps the order follows it.  The two (64,17) error pieces go back through LDS the same
//                      way; the translation is three doubles per lane, 1536 contiguous bytes per wave.  Every branch is per lane,
//                      no value crosses lanes: a pose's result does not know the batch.
// k_project_points     256 consecutive points of the flat (B N) list per workgroup: their 768 floats through LDS (coalesced dwords in,
//                      stride 3 out: odd), one point per thread in fp32, the 512 floats of uv back through LDS.  20 bytes a point.
// k_place_accumulate   the tile kernel of k_bone_accumulate (bones.hip): a workgroup owns 64 poses, one thread per WORD of the table
//                      row walks them and adds its sum with one atomic whenever the group changes.  Integer adds commute: the table
//                      is a function of the multiset of poses alone.
#pragma clang fp contract(off)
#include "jrr_common.h"
#include "../../include/jrr.h"
#include "acctab.h"

namespace jrr {

constexpr int PL_POSES = 64;                       // poses per workgroup of k_place_translation and k_place_accumulate: one wave
constexpr int PL_J = NH * 3;                       // 51 floats of joints per pose
constexpr int PL_P = NH * 2, PL_PS = PL_P + 1;     // 34 floats of pixels per pose, at an LDS stride of 35
constexpr int PL_K = 9;                            // the 3x3 matrix
constexpr int PJ_POINTS = 256;                     // points per workgroup of k_project_points
constexpr double PL_LAMBDA0 = 1e-3, PL_LAMBDA_MIN = 1e-7, PL_LAMBDA_MAX = 1e7;

static_assert(NH == 17 && (PL_J & 1) && (PL_PS & 1) && (PL_K & 1) && (NH & 1), "odd LDS row strides");
static_assert(JRR_PLACE_ACC_STEP_PIVOT == 2 && JRR_PLACE_ACC_SUM_TZ == 3 && JRR_PLACE_ACC_JOINTS == 4 &&
              JRR_PLACE_ACC_SUM_ERR_LIN == JRR_PLACE_ACC_JOINTS + NH && JRR_PLACE_ACC_SUM_ERR == JRR_PLACE_ACC_SUM_ERR_LIN + NH &&
              JRR_PLACE_ACC_ROW == JRR_PLACE_ACC_SUM_ERR + NH && JRR_PLACE_ACC_TRAILER == JRR_EVAL_ACC_TRAILER, "row layout");
static_assert(JRR_PLACE_ACC_ROW + JRR_PLACE_ACC_TRAILER <= PL_POSES, "one thread per word of the row and of the trailer");
static_assert(JRR_PLACE_BAD_BITS == (JRR_PLACE_FEW_OR_NONFINITE | JRR_PLACE_LINEAR_PIVOT | JRR_PLACE_LINEAR_BEHIND), "the bits that void a pose");

// A x = y for the symmetric A given by its upper triangle, by A = L D L^T; false when a pivot fails d > 0 (x is then not written)
__device__ __forceinline__ bool pl_solve(double a00, double a01, double a02, double a11, double a12, double a22, double y0, double y1, double y2,
                                         double& x0, double& x1, double& x2) {
  const double d0 = a00;
  if (!(d0 > 0.0)) return false;
  const double l10 = a01 / d0, l20 = a02 / d0;
  const double d1 = a11 - l10 * a01;
  if (!(d1 > 0.0)) return false;
  const double m = a12 - l20 * a01;
  const double l21 = m / d1;
  const double d2 = (a22 - l20 * a02) - l21 * m;
  if (!(d2 > 0.0)) return false;
  const double z0 = y0, z1 = y1 - l10 * z0, z2 = (y2 - l20 * z0) - l21 * z1;
  x2 = z2 / d2;
  x1 = z1 / d1 - l21 * x2;
  x0 = (z0 / d0 - l10 * x1) - l20 * x2;
  return true;
}

struct PlPose {                                    // a thread's view of its pose: rows in LDS and the camera
  const float* S;                                  // 51
  const float* uv;                                 // 34
  const float* w;                                  // 17, or nullptr: ones
  unsigned part;                                   // bit j: joint j takes part
  double fx, fy, cx, cy;
};

// the cost at t; `front`: every taking-part joint has Z + t2 > 0; err (nullable): the 17 pixel distances, an LDS row
__device__ __forceinline__ double pl_cost(const PlPose& p, double t0, double t1, double t2, bool& front, float* err) {
  double c = 0.0;
  front = true;
  for (int j = 0; j < NH; ++j) {
    const double X = (double)p.S[3 * j] + t0, Y = (double)p.S[3 * j + 1] + t1, Z = (double)p.S[3 * j + 2] + t2;
    const double ru = ((p.fx * X) / Z + p.cx) - (double)p.uv[2 * j], rv = ((p.fy * Y) / Z + p.cy) - (double)p.uv[2 * j + 1];
    const double e2 = ru * ru + rv * rv;
    if (err) err[j] = (float)sqrt(e2);
    if ((p.part >> j) & 1u) {
      const double w = p.w ? (double)p.w[j] : 1.0;
      c = c + w * e2;
      front = front && (Z > 0.0);
    }
  }
  return c;
}

// grid: ceil(B / 64) workgroups of 64 threads
__global__ __launch_bounds__(PL_POSES) void k_place_translation(const float* __restrict__ joints, const float* __restrict__ j2d,
                                                                const float* __restrict__ K, const float* __restrict__ weight, int B, int n_iters,
                                                                double* __restrict__ trans, float* __restrict__ err_lin, float* __restrict__ err,
                                                                int* __restrict__ status) {
  __shared__ float s_j[PL_POSES * PL_J];           // 13 056 B
  __shared__ float s_p[PL_POSES * PL_PS];          //  8 960 B
  __shared__ float s_k[PL_POSES * PL_K];           //  2 304 B
  __shared__ float s_w[PL_POSES * NH];             //  4 352 B
  __shared__ float s_el[PL_POSES * NH];            //  4 352 B: err_lin
  __shared__ float s_e[PL_POSES * NH];             //  4 352 B: err
  const int tid = threadIdx.x, b0 = (int)blockIdx.x * PL_POSES, np = min(PL_POSES, B - b0), b = b0 + tid;
  {                                                // the workgroup's piece of each input: coalesced dwords
    const float* src = joints + (size_t)b0 * PL_J;
    for (int q = tid; q < np * PL_J; q += PL_POSES) s_j[q] = src[q];
    src = j2d + (size_t)b0 * PL_P;
    for (int q = tid; q < np * PL_P; q += PL_POSES) {
      const int pose = q / PL_P;
      s_p[pose * PL_PS + (q - pose * PL_P)] = src[q];
    }
    src = K + (size_t)b0 * PL_K;
    for (int q = tid; q < np * PL_K; q += PL_POSES) s_k[q] = src[q];
    if (weight) {
      src = weight + (size_t)b0 * NH;
      for (int q = tid; q < np * NH; q += PL_POSES) s_w[q] = src[q];
    }
  }
  __syncthreads();
  if (b < B) {
    PlPose p;
    p.S = s_j + tid * PL_J;
    p.uv = s_p + tid * PL_PS;
    p.w = weight ? s_w + tid * NH : nullptr;
    const float* k = s_k + tid * PL_K;
    p.fx = (double)k[0]; p.fy = (double)k[4]; p.cx = (double)k[2]; p.cy = (double)k[5];
    float* row_lin = s_el + tid * NH;
    float* row = s_e + tid * NH;
    bool finite = isfinite(k[0]) && isfinite(k[4]) && isfinite(k[2]) && isfinite(k[5]);
    for (int i = 0; i < PL_J; ++i) finite = finite && isfinite(p.S[i]);
    for (int i = 0; i < PL_P; ++i) finite = finite && isfinite(p.uv[i]);
    p.part = 0u;
    int n_part = 0;
    for (int j = 0; j < NH; ++j) {
      const bool in = !p.w || (isfinite(p.w[j]) && p.w[j] > 0.f);
      p.part |= in ? (1u << j) : 0u;
      n_part += in ? 1 : 0;
    }
    int st = (n_part < 2 || !finite) ? JRR_PLACE_FEW_OR_NONFINITE : 0;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    if (!st) {                                     // the linear start
      double a00 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, y0 = 0.0, y1 = 0.0, y2 = 0.0;
      for (int j = 0; j < NH; ++j) {
        if (!((p.part >> j) & 1u)) continue;
        const double w = p.w ? (double)p.w[j] : 1.0;
        const double X = (double)p.S[3 * j], Y = (double)p.S[3 * j + 1], Z = (double)p.S[3 * j + 2];
        const double a = (double)p.uv[2 * j] - p.cx, bb = (double)p.uv[2 * j + 1] - p.cy;
        const double r1 = a * Z - p.fx * X, r2 = bb * Z - p.fy * Y;
        a00 = a00 + w * p.fx * p.fx;
        a02 = a02 - w * p.fx * a;
        a11 = a11 + w * p.fy * p.fy;
        a12 = a12 - w * p.fy * bb;
        a22 = a22 + w * (a * a + bb * bb);
        y0 = y0 + w * p.fx * r1;
        y1 = y1 + w * p.fy * r2;
        y2 = y2 - w * (a * r1 + bb * r2);
      }
      if (!pl_solve(a00, 0.0, a02, a11, a12, a22, y0, y1, y2, t0, t1, t2)) st = JRR_PLACE_LINEAR_PIVOT;
    }
    if (!st) {
      bool front;
      double c = pl_cost(p, t0, t1, t2, front, row_lin);
      if (!front) st = JRR_PLACE_LINEAR_BEHIND;
      else {
        double lambda = PL_LAMBDA0;
        for (int it = 0; it < n_iters; ++it) {
          double h00 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
          for (int j = 0; j < NH; ++j) {
            if (!((p.part >> j) & 1u)) continue;
            const double w = p.w ? (double)p.w[j] : 1.0;
            const double X = (double)p.S[3 * j] + t0, Y = (double)p.S[3 * j + 1] + t1, Z = (double)p.S[3 * j + 2] + t2;
            const double ru = ((p.fx * X) / Z + p.cx) - (double)p.uv[2 * j], rv = ((p.fy * Y) / Z + p.cy) - (double)p.uv[2 * j + 1];
            const double q = 1.0 / Z;
            const double ju0 = p.fx * q, jv1 = p.fy * q;
            const double ju2 = -(ju0 * X) * q, jv2 = -(jv1 * Y) * q;
            h00 = h00 + w * ju0 * ju0;
            h02 = h02 + w * ju0 * ju2;
            h11 = h11 + w * jv1 * jv1;
            h12 = h12 + w * jv1 * jv2;
            h22 = h22 + w * (ju2 * ju2 + jv2 * jv2);
            g0 = g0 + w * ju0 * ru;
            g1 = g1 + w * jv1 * rv;
            g2 = g2 + w * (ju2 * ru + jv2 * rv);
          }
          double d0, d1, d2;
          bool accept = false;
          double cn = c, n0 = t0, n1 = t1, n2 = t2;
          if (pl_solve(h00 + lambda * h00, 0.0, h02, h11 + lambda * h11, h12, h22 + lambda * h22, -g0, -g1, -g2, d0, d1, d2)) {
            n0 = t0 + d0; n1 = t1 + d1; n2 = t2 + d2;
            bool fr;
            cn = pl_cost(p, n0, n1, n2, fr, nullptr);
            accept = (cn < c) && fr;
          } else st |= JRR_PLACE_STEP_PIVOT;
          if (accept) {
            t0 = n0; t1 = n1; t2 = n2; c = cn;
            lambda = fmax(lambda / 10.0, PL_LAMBDA_MIN);
          } else lambda = fmin(10.0 * lambda, PL_LAMBDA_MAX);
        }
        pl_cost(p, t0, t1, t2, front, row);
      }
    }
    if (st & JRR_PLACE_BAD_BITS) {
      const float nan = __builtin_nanf("");
      for (int j = 0; j < NH; ++j) { row_lin[j] = nan; row[j] = nan; }
      t0 = t1 = t2 = __builtin_nan("");
    }
    trans[(size_t)b * 3] = t0;
    trans[(size_t)b * 3 + 1] = t1;
    trans[(size_t)b * 3 + 2] = t2;
    status[b] = st;
  }
  __syncthreads();
  const size_t at = (size_t)b0 * NH;                // the two (np,17) pieces: coalesced dwords
  for (int q = tid; q < np * NH; q += PL_POSES) {
    if (err_lin) err_lin[at + q] = s_el[q];
    err[at + q] = s_e[q];
  }
}

// grid: ceil(B N / 256) workgroups of 256 threads; workgroup t owns points 256 t .. 256 t + 255 of the flat list
__global__ __launch_bounds__(PJ_POINTS) void k_project_points(const float* __restrict__ points, const double* __restrict__ trans,
                                                              const float* __restrict__ K, int total, int N, float* __restrict__ uv,
                                                              float* __restrict__ depth) {
  __shared__ float s_in[PJ_POINTS * 3];
  __shared__ float s_uv[PJ_POINTS * 2];
  const int tid = threadIdx.x, p0 = (int)blockIdx.x * PJ_POINTS, np = min(PJ_POINTS, total - p0), pt = p0 + tid;
  const float* src = points + (size_t)p0 * 3;
  for (int q = tid; q < np * 3; q += PJ_POINTS) s_in[q] = src[q];
  __syncthreads();
  if (tid < np) {
    const int pose = pt / N;
    const double* t = trans + (size_t)pose * 3;
    const float* k = K + (size_t)pose * PL_K;
    const float tx = (float)t[0], ty = (float)t[1], tz = (float)t[2];
    const float fx = k[0], fy = k[4], cx = k[2], cy = k[5];
    const float X = s_in[3 * tid] + tx, Y = s_in[3 * tid + 1] + ty, d = s_in[3 * tid + 2] + tz;
    const bool front = d > 0.f;
    const float nan = __builtin_nanf("");
    s_uv[2 * tid] = front ? (fx * X) / d + cx : nan;
    s_uv[2 * tid + 1] = front ? (fy * Y) / d + cy : nan;
    if (depth) depth[pt] = d;
  }
  __syncthreads();
  float* dst = uv + (size_t)p0 * 2;
  for (int q = tid; q < np * 2; q += PJ_POINTS) dst[q] = s_uv[q];
}

// grid: ceil(B / 64) workgroups of 64 threads; workgroup t owns poses 64 t .. 64 t + 63.  Thread w < 55 owns WORD w of the row, thread
// 55 / 56 the two trailer words (k_bone_accumulate, bones.hip, has the reasons).
__global__ __launch_bounds__(PL_POSES) void k_place_accumulate(const double* __restrict__ trans, const float* __restrict__ err_lin,
                                                               const float* __restrict__ err, const float* __restrict__ weight,
                                                               const int* __restrict__ status, const int* __restrict__ group, int n_groups,
                                                               long long* __restrict__ acc, int B) {
  __shared__ float s_el[PL_POSES * NH], s_e[PL_POSES * NH], s_w[PL_POSES * NH];
  __shared__ long long s_tz[PL_POSES];
  __shared__ unsigned s_part[PL_POSES];
  __shared__ int s_kind[PL_POSES], s_gid[PL_POSES], s_b3[PL_POSES];
  const int tid = threadIdx.x, b0 = (int)blockIdx.x * PL_POSES, np = min(PL_POSES, B - b0);
  const size_t at = (size_t)b0 * NH;
  for (int q = tid; q < np * NH; q += PL_POSES) {   // coalesced dwords
    s_e[q] = err[at + q];
    if (err_lin) s_el[q] = err_lin[at + q];
    if (weight) s_w[q] = weight[at + q];
  }
  __syncthreads();
  if (tid < np) {                                  // what each pose is to the table
    const int b = b0 + tid, gid = group ? group[b] : 0, st = status[b];
    int kind = acc_group_kind(gid, n_groups);
    unsigned part = 0u;
    for (int j = 0; j < NH; ++j) {
      const float w = weight ? s_w[tid * NH + j] : 1.f;
      part |= (isfinite(w) && w > 0.f) ? (1u << j) : 0u;
    }
    const float tz = (float)trans[(size_t)b * 3 + 2];
    if (kind == ACC_COUNTED) {
      bool good = !(st & JRR_PLACE_BAD_BITS) && (fabsf(tz) < ERR_CAP);      // false for NaN
      for (int j = 0; j < NH; ++j)
        if ((part >> j) & 1u) good = good && (s_e[tid * NH + j] < ERR_CAP) && (!err_lin || s_el[tid * NH + j] < ERR_CAP);
      kind = good ? ACC_COUNTED : ACC_BAD;
    }
    s_kind[tid] = kind;
    s_gid[tid] = gid;
    s_part[tid] = part;
    s_b3[tid] = (st & JRR_PLACE_STEP_PIVOT) ? 1 : 0;
    s_tz[tid] = kind == ACC_COUNTED ? err_fixed24(tz) : 0;
  }
  __syncthreads();
  const int w = tid;
  if (w >= JRR_PLACE_ACC_ROW + JRR_PLACE_ACC_TRAILER) return;
  if (w >= JRR_PLACE_ACC_ROW) {                    // the trailer: poses ignored on purpose, poses with a group outside the table
    const int want = ACC_IGNORED + (w - JRR_PLACE_ACC_ROW);
    int n = 0;
    for (int p = 0; p < np; ++p) n += s_kind[p] == want;
    if (n) acc_add(acc_trailer_word(acc, JRR_PLACE_ACC_ROW, n_groups, want), n);
    return;
  }
  if (!err_lin && w >= JRR_PLACE_ACC_SUM_ERR_LIN && w < JRR_PLACE_ACC_SUM_ERR) return;
  const int j = w >= JRR_PLACE_ACC_SUM_ERR ? w - JRR_PLACE_ACC_SUM_ERR
                                           : (w >= JRR_PLACE_ACC_SUM_ERR_LIN ? w - JRR_PLACE_ACC_SUM_ERR_LIN : w - JRR_PLACE_ACC_JOINTS);      // w >= 4
  long long sum = 0;
  int cur = 0;                                     // the group `sum` belongs to (sum == 0: none yet)
  for (int p = 0; p < np; ++p) {                   // uniform over the workgroup: every thread sees the same kinds and groups
    const int kind = s_kind[p];
    if (kind >= ACC_IGNORED) continue;
    const int g = s_gid[p];                        // 0 <= g < n_groups
    if (g != cur) {
      if (sum != 0) acc_add(acc_row(acc, JRR_PLACE_ACC_ROW, cur) + w, sum);
      sum = 0;
      cur = g;
    }
    if (w == JRR_PLACE_ACC_BAD) sum += kind == ACC_BAD ? 1 : 0;
    else if (kind == ACC_COUNTED) {
      if (w == JRR_PLACE_ACC_COUNT) sum += 1;
      else if (w == JRR_PLACE_ACC_STEP_PIVOT) sum += s_b3[p];
      else if (w == JRR_PLACE_ACC_SUM_TZ) sum += s_tz[p];
      else if ((s_part[p] >> j) & 1u) {
        if (w >= JRR_PLACE_ACC_SUM_ERR) sum += err_fixed24(s_e[p * NH + j]);
        else if (w >= JRR_PLACE_ACC_SUM_ERR_LIN) sum += err_fixed24(s_el[p * NH + j]);
        else sum += 1;
      }
    }
  }
  if (sum != 0) acc_add(acc_row(acc, JRR_PLACE_ACC_ROW, cur) + w, sum);
}

}  // namespace jrr

using namespace jrr;

extern "C" int jrr_place_translation(const float* joints, const float* j2d, const float* K, const float* weight, int batch, int n_iters,
                                     double* trans, float* err_lin, float* err, int32_t* status, void* stream) {
  const char* why = nullptr;
  if (!joints || !j2d || !K) why = "bad argument (joints, j2d and K are required)";
  else if (!trans || !err || !status) why = "no output: trans, err and status are required";
  else if (batch < 0) why = "batch must not be negative";
  else if ((((uintptr_t)joints | (uintptr_t)j2d | (uintptr_t)K | (uintptr_t)weight | (uintptr_t)err_lin | (uintptr_t)err | (uintptr_t)status) & 3) != 0 ||
           ((uintptr_t)trans & 7) != 0)
    why = "trans must be 8-byte aligned, every other array 4-byte aligned";
  if (why) {
    jrr_set_error("jrr_place_translation: %s", why);
    return JRR_ERR_ARG;
  }
  if (n_iters < 0 || n_iters > JRR_PLACE_MAX_ITERS) {
    jrr_set_error("jrr_place_translation: n_iters %d: 0 .. %d", n_iters, (int)JRR_PLACE_MAX_ITERS);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  hipLaunchKernelGGL(k_place_translation, dim3((unsigned)((batch + PL_POSES - 1) / PL_POSES)), dim3(PL_POSES), 0, (hipStream_t)stream, joints, j2d, K,
                     weight, batch, n_iters, trans, err_lin, err, status);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_project_points(const float* points, const double* trans, const float* K, int batch, int n_points, float* uv, float* depth,
                                  void* stream) {
  const char* why = nullptr;
  if (!points || !trans || !K) why = "bad argument (points, trans and K are required)";
  else if (!uv) why = "no output: uv is NULL";
  else if (batch < 0) why = "batch must not be negative";
  else if (n_points < 0) why = "n_points must not be negative";
  else if ((long long)batch * n_points >= (1ll << 31)) why = "batch * n_points must stay below 2^31";
  else if ((((uintptr_t)points | (uintptr_t)K | (uintptr_t)uv | (uintptr_t)depth) & 3) != 0 || ((uintptr_t)trans & 7) != 0)
    why = "trans must be 8-byte aligned, every other array 4-byte aligned";
  if (why) {
    jrr_set_error("jrr_project_points: %s", why);
    return JRR_ERR_ARG;
  }
  const int total = batch * n_points;
  if (total == 0) return JRR_OK;
  hipLaunchKernelGGL(k_project_points, dim3((unsigned)((total + PJ_POINTS - 1) / PJ_POINTS)), dim3(PJ_POINTS), 0, (hipStream_t)stream, points, trans, K,
                     total, n_points, uv, depth);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_place_accumulate(const double* trans, const float* err_lin, const float* err, const float* weight, const int32_t* status,
                                    const int32_t* group, int batch, int n_groups, int64_t* acc, void* stream) {
  const char* why = nullptr;
  if (!trans || !err || !status || !acc) why = "bad argument (trans, err, status and acc are required)";
  else if (batch < 0) why = "batch must not be negative";
  else if ((((uintptr_t)err_lin | (uintptr_t)err | (uintptr_t)weight | (uintptr_t)status | (uintptr_t)group) & 3) != 0 || !acc_aligned(acc, trans))
    why = "trans and acc must be 8-byte aligned, every other array 4-byte aligned";
  if (why) {
    jrr_set_error("jrr_place_accumulate: %s", why);
    return JRR_ERR_ARG;
  }
  if (acc_groups_refused("jrr_place_accumulate", n_groups)) return JRR_ERR_ARG;
  if (batch == 0) return JRR_OK;
  hipLaunchKernelGGL(k_place_accumulate, dim3((unsigned)((batch + PL_POSES - 1) / PL_POSES)), dim3(PL_POSES), 0, (hipStream_t)stream, trans, err_lin,
                     err, weight, status, group, n_groups, reinterpret_cast<long long*>(acc), batch);
  CHECK_LAUNCH();
  return JRR_OK;
}
