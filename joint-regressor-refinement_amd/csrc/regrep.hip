// The regressor report (`--regressor_report`): what the retrained J_regressor did to each H36M joint, and the picture of it.
// The reference's teaser.png draws the joints of the accepted regressor, of the retrained one and the ground truth on the fitted mesh;
// its code keeps only the errors of the two sets (scripts/test.py:107-123).  Two launches, no engine, no body model:
//
// k_shift_accumulate  per pose the displacement b - a of the 17 joints in a frame fixed to the body (built from A's hips, pelvis and
//                     neck: a foreign mesh has no pose to take a frame from), as fixed-point sums, second moments, lengths and 2-mm
//                     histograms per group (include/jrr.h, JRR_SHIFT_ACC_*).  One pose per thread, 102 floats in, 205 int64 atomics
//                     out; integer atomics only, as k_eval_accumulate: the table does not depend on the order, the split into calls
//                     or the sharding over ranks.
// k_draw_discs        filled discs into an existing uint8 picture of any size.  One thread owns one pixel; the pose's points wait in
//                     LDS as (x, y, r * r), a point that draws nothing as r * r = -1; the thread walks them in order and keeps the last
//                     one that covers its pixel, then stores three bytes -- or nothing: an uncovered pixel is never written.
// Every floating-point operation is stated in include/jrr.h and rounded once, in the order written (no product is fused into a sum), so
// a host restatement follows it.
#include "jrr_common.h"
#include "acctab.h"
#include "../../include/jrr.h"

namespace jrr {

constexpr int RR_THREADS = 256;
constexpr float RR_FINITE = 3.402823466e+38f;    // FLT_MAX: |x| <= RR_FINITE: neither NaN nor infinite
constexpr float RR_FIXED = 16777216.f;           // 2^24

static_assert(JRR_SHIFT_ACC_MOM == JRR_SHIFT_ACC_SUM + NH * 3 && JRR_SHIFT_ACC_ABS == JRR_SHIFT_ACC_MOM + NH * 6 &&
              JRR_SHIFT_ACC_ABS_REL == JRR_SHIFT_ACC_ABS + NH && JRR_SHIFT_ACC_HIST == JRR_SHIFT_ACC_ABS_REL + NH &&
              JRR_SHIFT_ACC_ROW == JRR_SHIFT_ACC_HIST + NH * JRR_SHIFT_ACC_BINS && JRR_SHIFT_ACC_TRAILER == JRR_EVAL_ACC_TRAILER,
              "row layout");

#pragma clang fp contract(off)

__device__ __forceinline__ bool rr_finite(float x) { return fabsf(x) <= RR_FINITE; }
__device__ __forceinline__ float rr_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void rr_cross(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// one pose per thread; every update is an int64 atomic
__global__ __launch_bounds__(RR_THREADS) void k_shift_accumulate(const float* __restrict__ ja, const float* __restrict__ jb,
                                                                 const int* __restrict__ group, int n_groups, long long* __restrict__ acc,
                                                                 int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int g = group ? group[b] : 0;
  if (long long* t = acc_refused(acc, JRR_SHIFT_ACC_ROW, n_groups, g)) { acc_add(t, 1); return; }
  long long* row = acc_row(acc, JRR_SHIFT_ACC_ROW, g);
  const float* pa = ja + (size_t)b * NH * 3;
  const float* pb = jb + (size_t)b * NH * 3;

  bool good = true;
  for (int i = 0; i < NH * 3; ++i) good = good && rr_finite(pa[i]) && rr_finite(pb[i]);
  float xh[3], yh[3], zh[3];
  if (good) {
    float x[3], u[3], z[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { x[c] = pa[4 * 3 + c] - pa[1 * 3 + c]; u[c] = pa[8 * 3 + c] - pa[c]; }
    const float lx = sqrtf(rr_dot(x, x));
    good = lx >= 1e-4f;
#pragma unroll
    for (int c = 0; c < 3; ++c) xh[c] = x[c] / lx;
    rr_cross(xh, u, z);
    const float lu = sqrtf(rr_dot(u, u)), lz = sqrtf(rr_dot(z, z));
    good = good && lz >= 1e-4f * lu;
#pragma unroll
    for (int c = 0; c < 3; ++c) zh[c] = z[c] / lz;
    rr_cross(zh, xh, yh);
  }
  if (good) {                                    // the cap, before anything is added: a pose is counted whole or not at all
    for (int j = 0; j < NH; ++j) {
      const float d[3] = {pb[j * 3] - pa[j * 3], pb[j * 3 + 1] - pa[j * 3 + 1], pb[j * 3 + 2] - pa[j * 3 + 2]};
      good = good && fabsf(rr_dot(d, xh)) < 4.0f && fabsf(rr_dot(d, yh)) < 4.0f && fabsf(rr_dot(d, zh)) < 4.0f;
    }
  }
  if (!good) { acc_add(row + JRR_SHIFT_ACC_BAD, 1); return; }
  acc_add(row + JRR_SHIFT_ACC_COUNT, 1);
  const float d0[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
  for (int j = 0; j < NH; ++j) {
    const float d[3] = {pb[j * 3] - pa[j * 3], pb[j * 3 + 1] - pa[j * 3 + 1], pb[j * 3 + 2] - pa[j * 3 + 2]};
    const long long q[3] = {__float2ll_rn(rr_dot(d, xh) * RR_FIXED), __float2ll_rn(rr_dot(d, yh) * RR_FIXED),
                            __float2ll_rn(rr_dot(d, zh) * RR_FIXED)};
    int m = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      acc_add(row + JRR_SHIFT_ACC_SUM + j * 3 + i, q[i]);
#pragma unroll
      for (int k = i; k < 3; ++k, ++m) acc_add(row + JRR_SHIFT_ACC_MOM + j * 6 + m, (q[i] * q[k]) >> 16);
    }
    const float len = sqrtf(rr_dot(d, d));
    const float r[3] = {d[0] - d0[0], d[1] - d0[1], d[2] - d0[2]};
    const float rel = sqrtf(rr_dot(r, r));
    acc_add(row + JRR_SHIFT_ACC_ABS + j, __float2ll_rn(len * RR_FIXED));
    acc_add(row + JRR_SHIFT_ACC_ABS_REL + j, __float2ll_rn(rel * RR_FIXED));
    const int bin = max(min((int)floorf(len * 500.0f), JRR_SHIFT_ACC_BINS - 1), 0);
    acc_add(row + JRR_SHIFT_ACC_HIST + j * JRR_SHIFT_ACC_BINS + bin, 1);
  }
}

struct DiscArgs {
  uint8_t* rgb; const float* pts; const float* rad; float radius;
  int B, h, w, n_sets, n_pts;
  unsigned char colour[JRR_DISCS_MAX_SETS][3];
};

// grid: B * nblk workgroups; workgroup (b, k) owns pixels [256 k, 256 k + 256) of picture b, row-major
__global__ __launch_bounds__(RR_THREADS) void k_draw_discs(DiscArgs a, int nblk) {
  __shared__ float s_p[JRR_DISCS_MAX_SETS * JRR_DISCS_MAX_POINTS * 3];       // (x, y, r * r); r * r = -1: draws nothing
  const int tid = threadIdx.x, b = (int)blockIdx.x / nblk, k = (int)blockIdx.x - b * nblk;
  const int n = a.n_sets * a.n_pts;
  for (int i = tid; i < n; i += RR_THREADS) {
    const int set = i / a.n_pts, p = i - set * a.n_pts;
    const size_t at = ((size_t)set * a.B + b) * a.n_pts + p;
    const float px = a.pts[at * 2], py = a.pts[at * 2 + 1];
    const float r = a.rad ? a.rad[at] : a.radius;
    const bool draws = rr_finite(px) && rr_finite(py) && rr_finite(r) && r >= 0.f;
    s_p[i * 3] = px; s_p[i * 3 + 1] = py; s_p[i * 3 + 2] = draws ? r * r : -1.f;
  }
  __syncthreads();
  const int idx = k * RR_THREADS + tid;
  if (idx >= a.h * a.w) return;
  const int y = idx / a.w, x = idx - y * a.w;
  const float fx = (float)x, fy = (float)y;
  int hit = -1;
  for (int i = 0; i < n; ++i) {
    const float r2 = s_p[i * 3 + 2];
    const float dy = fy - s_p[i * 3 + 1], dy2 = dy * dy;
    if (!(dy2 <= r2)) continue;                  // dx * dx >= 0 and rounding is monotonic: the sum cannot be smaller
    const float dx = fx - s_p[i * 3];
    if (dx * dx + dy2 <= r2) hit = i;
  }
  if (hit < 0) return;
  const int set = hit / a.n_pts;
  uint8_t* o = a.rgb + ((size_t)b * a.h * a.w + idx) * 3;
  o[0] = a.colour[set][0]; o[1] = a.colour[set][1]; o[2] = a.colour[set][2];
}

static int launch_draw_discs(uint8_t* rgb, int B, int h, int w, const float* pts, const float* rad, float radius, const uint8_t* colours,
                      int n_sets, int n_pts, hipStream_t s) {
  DiscArgs a;
  a.rgb = rgb; a.pts = pts; a.rad = rad; a.radius = radius; a.B = B; a.h = h; a.w = w; a.n_sets = n_sets; a.n_pts = n_pts;
  for (int i = 0; i < JRR_DISCS_MAX_SETS; ++i)
    for (int c = 0; c < 3; ++c) a.colour[i][c] = i < n_sets ? colours[i * 3 + c] : 0;
  const int nblk = (h * w + RR_THREADS - 1) / RR_THREADS;
  hipLaunchKernelGGL(k_draw_discs, dim3((unsigned)((size_t)B * nblk)), dim3(RR_THREADS), 0, s, a, nblk);
  return 0;
}

}  // namespace jrr

using namespace jrr;

extern "C" int jrr_regressor_shift_accumulate(const float* joints_a, const float* joints_b, const int32_t* group, int batch, int n_groups,
                                              int64_t* acc, void* stream) {
  if (!joints_a || !joints_b || !acc || batch < 0 || !acc_aligned(acc)) {
    jrr_set_error("jrr_regressor_shift_accumulate: bad argument");
    return JRR_ERR_ARG;
  }
  if (acc_groups_refused("jrr_regressor_shift_accumulate", n_groups)) return JRR_ERR_ARG;
  if (batch == 0) return JRR_OK;
  hipLaunchKernelGGL(k_shift_accumulate, dim3((unsigned)((batch + RR_THREADS - 1) / RR_THREADS)), dim3(RR_THREADS), 0, (hipStream_t)stream, joints_a,
                     joints_b, group, n_groups, reinterpret_cast<long long*>(acc), batch);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_draw_discs(uint8_t* rgb, int batch, int h, int w, const float* points, const float* radius_dev, float radius,
                              const uint8_t* colours_host, int n_sets, int n_pts, void* stream) {
  if (!rgb || !points || !colours_host || batch < 0 || h < 1 || w < 1 || (long long)h * w > (1ll << 28)) {
    jrr_set_error("jrr_draw_discs: bad argument (h, w >= 1, h * w <= 2^28)");
    return JRR_ERR_ARG;
  }
  if (n_sets < 1 || n_sets > JRR_DISCS_MAX_SETS || n_pts < 1 || n_pts > JRR_DISCS_MAX_POINTS) {
    jrr_set_error("jrr_draw_discs: %d sets of %d points: 1 .. %d sets of 1 .. %d points", n_sets, n_pts, (int)JRR_DISCS_MAX_SETS,
                  (int)JRR_DISCS_MAX_POINTS);
    return JRR_ERR_ARG;
  }
  if ((long long)batch * (((long long)h * w + 255) / 256) > 0x7fffffffll) {
    jrr_set_error("jrr_draw_discs: batch %d of %d x %d pictures: more workgroups than one launch takes", batch, h, w);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  launch_draw_discs(rgb, batch, h, w, points, radius_dev, radius, colours_host, n_sets, n_pts, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}
