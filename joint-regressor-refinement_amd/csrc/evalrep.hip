// The evaluation report (`--eval_report`, `--eval_vertices`): where the error is, and joints of meshes that did not come from this
// library's SMPL forward.  Three launches, no engine, no body model:
//
// k_evaluate_joints      evaluate (/root/reference/scripts/utils.py:127-138, scripts/eval_utils.py:7-58) WITHOUT its mean over the
//                        joints: the 17 distances and the 17 Procrustes-aligned distances per pose, in metres.  One pose per thread,
//                        the body is k_evaluate's (evalk.h).  A pose's row is 68 bytes, so a thread's own stores would be 17 scattered
//                        dwords: the 64 rows of a workgroup are one contiguous 4352-byte piece of each output, assembled in LDS (stride 17
//                        floats: odd, conflict-free) and stored 16 bytes per lane.
// k_regress_prepare      J*mask -> ReLU -> division of each row by its sum (scripts/utils.py:87-92; scripts/test.py:206-212), once per
//                        regressor set: per (regressor, row) the positive columns in ascending order and their normalised values.
//                        The row sum is accumulated in double in a fixed tree, then rounded to float ONCE; the division is the
//                        reference's fp32 division.  A NaN entry stays in the list (ReLU(NaN) = NaN poisons its row, as in the
//                        reference); a row without a positive entry has an empty list and gives NaN joints (the reference's 0/0).
// k_regress_joints<LDS>  J_norm @ vertices (scripts/utils.py:96-98; scripts/test.py:255-283 on somebody else's vertices): one
//                        workgroup per pose, one wave per (regressor, joint) row at a time.  Lane l takes the list's entries
//                        l, l + 64, ... in ascending order, products and sums in double (a float x float product is exact there),
//                        then ONE xor tree over the 64 lanes and ONE rounding to float: the order is a function of the list alone,
//                        not of the launch geometry, the batch size or n_reg.
//                        <false>: every list has at most 64 entries (the shipped 62-entry regressor: at most 9 per row) -- the
//                        vertices are gathered from global memory, ~0.7 KB per pose.  <true>: otherwise -- the pose's 82 680 bytes
//                        are read ONCE for all n_reg regressors into LDS (8-byte loads: a pose's block is only 8-byte aligned).
//                        Both are launched; the lists' lengths decide on the device which one works (no host synchronisation), the
//                        other returns at once.  Same per-row procedure, same bits.
// k_eval_accumulate      per group (action / subject) the counts, the fixed-point sums of the per-joint errors and the 1-mm histograms
//                        of include/jrr.h (JRR_EVAL_ACC_*), int64, integer atomics only: independent of order, of the split into calls
//                        and of the sharding over ranks.
#include "jrr_common.h"
#include "evalk.h"
#include "fixedpt.h"
#include "acctab.h"
#include "../../include/jrr.h"

namespace jrr {

constexpr int EJ_POSES = 64;                       // poses per workgroup of k_evaluate_joints: one wave
constexpr int EJ_ROWF = EJ_POSES * NH;             // 1088 floats = 272 float4 per output and workgroup
static_assert(EJ_ROWF % 4 == 0, "a workgroup's piece of err_j is a whole number of 16-byte stores");

__global__ __launch_bounds__(EJ_POSES) void k_evaluate_joints(const float* __restrict__ pred, const float* __restrict__ target_mm,
                                                              float* __restrict__ err_j, float* __restrict__ err_pa_j, int B) {
  __shared__ float4 s_out4[2][EJ_ROWF / 4];
  float* s_plain = reinterpret_cast<float*>(s_out4[0]);
  float* s_pa = reinterpret_cast<float*>(s_out4[1]);
  const int tid = threadIdx.x, b0 = (int)blockIdx.x * EJ_POSES, b = b0 + tid;
  if (b < B) {
    float* row = s_plain + tid * NH;
    float* row_pa = s_pa + tid * NH;
#define JRR_EVAL_PLAIN_BEGIN
#define JRR_EVAL_PLAIN(i, d) row[i] = d;
#define JRR_EVAL_PLAIN_END
#define JRR_EVAL_PA_BEGIN
#define JRR_EVAL_PA(i, d) row_pa[i] = d;
#define JRR_EVAL_PA_END
#define JRR_EVAL_BODY
#include "evalk.h"
#undef JRR_EVAL_BODY
#undef JRR_EVAL_PLAIN_BEGIN
#undef JRR_EVAL_PLAIN
#undef JRR_EVAL_PLAIN_END
#undef JRR_EVAL_PA_BEGIN
#undef JRR_EVAL_PA
#undef JRR_EVAL_PA_END
  }
  __syncthreads();
  const int n = min(EJ_POSES, B - b0) * NH;          // floats of this workgroup's piece (a ragged last one: any multiple of 17)
  const size_t base = (size_t)b0 * NH;               // b0 * 68 bytes: a multiple of 4352
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    float* dst = (o == 0 ? err_j : err_pa_j) + base;
    const float* src = reinterpret_cast<const float*>(s_out4[o]);
    for (int q = tid; q < n / 4; q += EJ_POSES) reinterpret_cast<float4*>(dst)[q] = s_out4[o][q];
    const int tail = n & ~3;
    if (tid < n - tail) dst[tail + tid] = src[tail + tid];
  }
}

// ---- regress: workspace = int32 head[RG_HEAD] | float vals[n_reg][17][V] | int32 cols[n_reg][17][V] -----------------------------
constexpr int RG_HEAD = 128;                       // head[r * 17 + j] = entries of row j of regressor r (at most 4 * 17 = 68 used)
constexpr int RG_THREADS = 256;
constexpr int RG_CHUNK = (V + RG_THREADS - 1) / RG_THREADS;      // 27 consecutive columns per thread of k_regress_prepare
constexpr int RG_SPARSE_MAX = 64;                  // longest list k_regress_joints<false> takes: one entry per lane
static_assert(JRR_REGRESS_MAX_REG * NH <= RG_HEAD, "the head holds every row's count");

static size_t regress_workspace_bytes(int n_reg) { return (size_t)RG_HEAD * 4 + (size_t)n_reg * NH * V * 8; }

__device__ __forceinline__ float* rg_vals(void* ws) { return reinterpret_cast<float*>(reinterpret_cast<int*>(ws) + RG_HEAD); }
__device__ __forceinline__ const float* rg_vals(const void* ws) {
  return reinterpret_cast<const float*>(reinterpret_cast<const int*>(ws) + RG_HEAD);
}

// grid (17, n_reg): one workgroup per row
__global__ __launch_bounds__(RG_THREADS) void k_regress_prepare(const float* __restrict__ J, const float* __restrict__ mask, int n_reg,
                                                                void* __restrict__ ws) {
  __shared__ double s_sum[RG_THREADS];
  __shared__ int s_cnt[RG_THREADS];
  const int tid = threadIdx.x, j = blockIdx.x, r = blockIdx.y;
  const float* row = J + ((size_t)r * NH + j) * V;
  const float* mrow = mask ? mask + (size_t)j * V : nullptr;
  const int c0 = tid * RG_CHUNK, c1 = min(c0 + RG_CHUNK, V);
  double sum = 0.0;
  int cnt = 0;
  for (int c = c0; c < c1; ++c) {
    const float x = mrow ? row[c] * mrow[c] : row[c];
    if (!(x <= 0.f)) { sum += (double)x; ++cnt; }    // positive, or NaN: ReLU keeps both
  }
  s_sum[tid] = sum;
  s_cnt[tid] = cnt;
  __syncthreads();
  for (int o = 1; o < RG_THREADS; o <<= 1) {         // inclusive scan of the counts
    const int t = tid >= o ? s_cnt[tid - o] : 0;
    __syncthreads();
    s_cnt[tid] += t;
    __syncthreads();
  }
  for (int o = RG_THREADS / 2; o > 0; o >>= 1) {     // the row sum: one fixed tree
    if (tid < o) s_sum[tid] += s_sum[tid + o];
    __syncthreads();
  }
  const float total = (float)s_sum[0];
  int at = s_cnt[tid] - cnt;
  float* vals = rg_vals(ws) + ((size_t)r * NH + j) * V;
  int* cols = reinterpret_cast<int*>(rg_vals(ws) + (size_t)n_reg * NH * V) + ((size_t)r * NH + j) * V;
  for (int c = c0; c < c1; ++c) {
    const float x = mrow ? row[c] * mrow[c] : row[c];
    if (!(x <= 0.f)) { vals[at] = x / total; cols[at] = c; ++at; }
  }
  if (tid == RG_THREADS - 1) reinterpret_cast<int*>(ws)[r * NH + j] = s_cnt[tid];
}

// grid: one workgroup of 4 waves per pose.  USE_LDS selects the vertex source and which lists this instantiation works on.
template <bool USE_LDS>
__global__ __launch_bounds__(RG_THREADS) void k_regress_joints(const float* __restrict__ verts, const void* __restrict__ ws, int n_reg,
                                                               float* __restrict__ joints, int B) {
  extern __shared__ __attribute__((aligned(8))) float s_v[];      // USE_LDS: [V][3]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int* head = reinterpret_cast<const int*>(ws);
  const int n_rows = n_reg * NH;
  int longest = 0;
  for (int i = 0; i < n_rows; ++i) longest = max(longest, head[i]);          // uniform: <= 68 scalar loads
  if ((longest > RG_SPARSE_MAX) != USE_LDS) return;
  const float* pv = verts + (size_t)b * V * 3;
  if constexpr (USE_LDS) {
    const float2* g2 = reinterpret_cast<const float2*>(pv);                  // 82 680 B per pose: 8-byte aligned, 10 335 float2
    float2* s2 = reinterpret_cast<float2*>(s_v);
    for (int i = tid; i < V * 3 / 2; i += RG_THREADS) s2[i] = g2[i];
    __syncthreads();
    pv = s_v;
  }
  const float* vals = rg_vals(ws);
  const int* cols = reinterpret_cast<const int*>(vals + (size_t)n_reg * NH * V);
  for (int row = wave; row < n_rows; row += RG_THREADS / 64) {
    const int cnt = min(max(head[row], 0), V);
    const float* rv = vals + (size_t)row * V;
    const int* rc = cols + (size_t)row * V;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int k = lane; k < cnt; k += 64) {
      const double w = (double)rv[k];
      const int c = min((unsigned)rc[k], (unsigned)(V - 1));
      a0 += w * (double)pv[c * 3 + 0];
      a1 += w * (double)pv[c * 3 + 1];
      a2 += w * (double)pv[c * 3 + 2];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      a0 += __shfl_xor(a0, o);
      a1 += __shfl_xor(a1, o);
      a2 += __shfl_xor(a2, o);
    }
    if (lane < 3) {
      const double a = lane == 0 ? a0 : (lane == 1 ? a1 : a2);
      // row = r * 17 + j  ->  joints[r][b][j][lane]
      const int r = row / NH, j = row - r * NH;
      joints[(((size_t)r * B + b) * NH + j) * 3 + lane] = cnt > 0 ? (float)a : __int_as_float(0x7fc00000);
    }
  }
}

static bool regress_attributes() {
  static const bool ok = hipFuncSetAttribute((const void*)k_regress_joints<true>, hipFuncAttributeMaxDynamicSharedMemorySize, V * 3 * 4) ==
                         hipSuccess;
  return ok;
}

// joints (n_reg,B,17,3) <- normalised regressors of ws x verts (B,6890,3); -1 when the device refuses the LDS the dense path needs
static int launch_regress_joints(const float* verts, const void* ws, int n_reg, float* joints, int B, hipStream_t s) {
  if (!regress_attributes()) return -1;
  hipLaunchKernelGGL(k_regress_joints<false>, dim3((unsigned)B), dim3(RG_THREADS), 0, s, verts, ws, n_reg, joints, B);
  hipLaunchKernelGGL(k_regress_joints<true>, dim3((unsigned)B), dim3(RG_THREADS), V * 3 * 4, s, verts, ws, n_reg, joints, B);
  return 0;
}

// ---- accumulate -------------------------------------------------------------------------------------------------------------------
static_assert(JRR_EVAL_ACC_ROW == JRR_EVAL_ACC_HIST_PA + JRR_EVAL_ACC_BINS && JRR_EVAL_ACC_SUM_PA == JRR_EVAL_ACC_SUM + NH &&
              JRR_EVAL_ACC_HIST == JRR_EVAL_ACC_SUM_PA + NH && JRR_EVAL_ACC_HIST_PA == JRR_EVAL_ACC_HIST + JRR_EVAL_ACC_BINS, "row layout");

// one pose per thread; every update is an int64 atomic
__global__ __launch_bounds__(256) void k_eval_accumulate(const float* __restrict__ err_j, const float* __restrict__ err_pa_j,
                                                         const int* __restrict__ group, int n_groups, long long* __restrict__ acc, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int g = group[b];
  if (long long* t = acc_refused(acc, JRR_EVAL_ACC_ROW, n_groups, g)) { acc_add(t, 1); return; }
  long long* row = acc_row(acc, JRR_EVAL_ACC_ROW, g);
  const float* e0 = err_j + (size_t)b * NH;
  const float* e1 = err_pa_j + (size_t)b * NH;
  bool good = true;
  for (int i = 0; i < NH; ++i) good = good && (e0[i] < ERR_CAP) && (e1[i] < ERR_CAP);       // false for NaN
  if (!good) { acc_add(row + JRR_EVAL_ACC_BAD, 1); return; }
  acc_add(row + JRR_EVAL_ACC_COUNT, 1);
  for (int i = 0; i < NH; ++i) {
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const float e = o == 0 ? e0[i] : e1[i];
      acc_add(row + (o == 0 ? JRR_EVAL_ACC_SUM : JRR_EVAL_ACC_SUM_PA) + i, err_fixed24(e));
      // distances are never negative; a negative value a caller passes anyway lands in bin 0 (no index below the row)
      const int bin = max(min((int)floorf(e * 1000.f), JRR_EVAL_ACC_BINS - 1), 0);
      acc_add(row + (o == 0 ? JRR_EVAL_ACC_HIST : JRR_EVAL_ACC_HIST_PA) + bin, 1);
    }
  }
}

}  // namespace jrr

using namespace jrr;

/* the evaluation report (--eval_report / --eval_vertices): per-joint errors, joints of foreign meshes, the int64 accumulator */
extern "C" int jrr_evaluate_joints(const float* pred, const float* target_mm, float* err_j, float* err_pa_j, int batch, void* stream) {
  if (!pred || !target_mm || !err_j || !err_pa_j || batch < 0) {
    jrr_set_error("jrr_evaluate_joints: bad argument");
    return JRR_ERR_ARG;
  }
  if ((((uintptr_t)err_j | (uintptr_t)err_pa_j) & 15) != 0) {
    jrr_set_error("jrr_evaluate_joints: err_j and err_pa_j must be 16-byte aligned");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  hipLaunchKernelGGL(k_evaluate_joints, dim3((unsigned)((batch + EJ_POSES - 1) / EJ_POSES)), dim3(EJ_POSES), 0, (hipStream_t)stream, pred, target_mm,
                     err_j, err_pa_j, batch);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" size_t jrr_regress_joints_workspace_bytes(int n_reg) {
  return (n_reg < 1 || n_reg > JRR_REGRESS_MAX_REG) ? 0 : regress_workspace_bytes(n_reg);
}
extern "C" int jrr_regress_joints_prepare(const float* J, int n_reg, const float* mask, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  if (!J || !workspace || n_reg < 1 || n_reg > JRR_REGRESS_MAX_REG || ((uintptr_t)workspace & 15) != 0) {
    jrr_set_error("jrr_regress_joints_prepare: bad argument (1 <= n_reg <= %d, workspace 16-byte aligned)", (int)JRR_REGRESS_MAX_REG);
    return JRR_ERR_ARG;
  }
  if (workspace_bytes < regress_workspace_bytes(n_reg)) {
    jrr_set_error("jrr_regress_joints_prepare: the workspace needs jrr_regress_joints_workspace_bytes(%d) = %zu bytes", n_reg,
                  regress_workspace_bytes(n_reg));
    return JRR_ERR_WORKSPACE;
  }
  hipLaunchKernelGGL(k_regress_prepare, dim3(NH, n_reg), dim3(RG_THREADS), 0, (hipStream_t)stream, J, mask, n_reg, workspace);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_regress_joints(const float* verts, int batch, const void* workspace, int n_reg, float* joints, void* stream) {
  if (!verts || !workspace || !joints || batch < 0 || n_reg < 1 || n_reg > JRR_REGRESS_MAX_REG || ((uintptr_t)verts & 7) != 0 ||
      ((uintptr_t)workspace & 15) != 0) {
    jrr_set_error("jrr_regress_joints: bad argument (1 <= n_reg <= %d, verts 8-byte aligned)", (int)JRR_REGRESS_MAX_REG);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  if (launch_regress_joints(verts, workspace, n_reg, joints, batch, (hipStream_t)stream) != 0) {
    jrr_set_error("jrr_regress_joints: the device refuses %d bytes of LDS per workgroup", V * 3 * 4);
    return JRR_ERR_HIP;
  }
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_eval_accumulate(const float* err_j, const float* err_pa_j, const int32_t* group, int batch, int n_groups, int64_t* acc,
                                   void* stream) {
  if (!err_j || !err_pa_j || !group || !acc || batch < 0 || !acc_aligned(acc)) {
    jrr_set_error("jrr_eval_accumulate: bad argument");
    return JRR_ERR_ARG;
  }
  if (acc_groups_refused("jrr_eval_accumulate", n_groups)) return JRR_ERR_ARG;
  if (batch == 0) return JRR_OK;
  hipLaunchKernelGGL(k_eval_accumulate, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, err_j, err_pa_j, group, n_groups,
                     reinterpret_cast<long long*>(acc), batch);
  CHECK_LAUNCH();
  return JRR_OK;
}
