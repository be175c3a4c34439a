// The per-vertex error of meshes (`--eval_pve`): PVE / MPVPE and its Procrustes-aligned form, per pose, per vertex, and the int64 tables
// of a report.  One launch, no engine, no body model; include/jrr.h (jrr_vertex_error, JRR_PVE_*) is the specification.
//
// k_vertex_error<SMALL>: a workgroup of PV_T = 256 threads owns the poses blockIdx.x, blockIdx.x + gridDim.x, ... one after the other;
//   thread tid owns vertices tid, tid + 256, ... of each.  A pose is three walks over its vertices:
//     A  x = P - root_pred, y = Q - root_gt, d = |x - y| (err_v, its fixed-point sum, its part sums) and the double sums of x and y
//     B  K = sum (x - mu1)(y - mu2)^T and var1 = sum |x - mu1|^2 in double, mu1 / mu2 the double means of walk A
//     C  e = |scale R x + t - y| (err_pa_v, its sum, its part sums) after csrc/procfit.h on the moments rounded to fp32 -- every lane
//        computes the same 3x3 fit, nothing is broadcast
//     walks A and C also add their fixed-point values to the per-vertex table when the pose's group can be counted; a pose whose means
//     turn out NaN (rare) then takes a walk
//     D  d and e again, as fixed point, OUT of the per-vertex table: integer adds cancel exactly, the table ends as if never touched
//   SMALL (n_verts <= PV_SMALL = 7168): walk A keeps the thread's 28 x 6 coordinates in registers (one wave per SIMD: a lane has all 512
//     registers) and walks B, C, D read those: both meshes cross the memory system once.  The per-vertex table is summed over the
//     workgroup's poses in LDS (2 x 7168 int64 = 112 KB) and leaves as one global atomic per non-zero word per WORKGROUP.
//   otherwise: walks B, C, D read the meshes again (L2 / the memory-side cache), the per-vertex table takes global atomics per pose.
//   The double sums: a thread adds its vertices in ascending order, a wave combines its 64 lanes by an xor butterfly (every lane ends
//   with the same bits), the 4 wave sums are added in wave order by every thread: the order is a function of n_verts alone, and a
//   pose's values do not depend on the batch, on its place in it or on the grid.
//   The tables take integer atomics only; a pose's part sums are formed per wave in LDS (ds atomics) and added by one thread per part.
// Every floating-point operation is rounded once, in the order written (no product is fused into a sum), so a host restatement
// follows it.
#pragma clang fp contract(off)
#include "jrr_common.h"
#include "acctab.h"
#include "../../include/jrr.h"
#include "procfit.h"

namespace jrr {

constexpr int PV_T = 256;                          // threads per workgroup
constexpr int PV_W = PV_T / 64;                    // 4 waves
constexpr int PV_NPT = 28;                         // vertices a thread keeps in registers (SMALL)
constexpr int PV_SMALL = PV_NPT * PV_T;            // 7168
constexpr int PV_GRID_SMALL = 256, PV_GRID_LARGE = 512;
constexpr float PV_FIXED = 16777216.f;             // 2^24
constexpr int PV_PARTS = JRR_PVE_MAX_PARTS;

static_assert(JRR_PVE_ACC_COUNT == 0 && JRR_PVE_ACC_BAD == 1 && JRR_PVE_ACC_SUM == 2 && JRR_PVE_ACC_SUM_PA == 3 && JRR_PVE_ACC_HIST == 4 &&
              JRR_PVE_ACC_HIST_PA == JRR_PVE_ACC_HIST + JRR_PVE_ACC_BINS && JRR_PVE_ACC_PART == JRR_PVE_ACC_HIST_PA + JRR_PVE_ACC_BINS &&
              JRR_PVE_ACC_PART_PA == JRR_PVE_ACC_PART + JRR_PVE_MAX_PARTS && JRR_PVE_ACC_ROW == JRR_PVE_ACC_PART_PA + JRR_PVE_MAX_PARTS &&
              JRR_PVE_ACC_BINS == JRR_EVAL_ACC_BINS && JRR_PVE_ACC_TRAILER == JRR_EVAL_ACC_TRAILER, "row layout");
static_assert(PV_SMALL >= 6890 && JRR_PVE_MAX_VERTS == 65536, "sizes");

// sum over the workgroup of each of v[0 .. N): on return every thread holds the same N sums.  s_red: PV_W * N words.
template <class T, int N>
__device__ __forceinline__ void pv_block_sum(T (&v)[N], T* s_red, int tid) {
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off);
  __syncthreads();                                 // the previous use of s_red is over
  if ((tid & 63) == 0)
#pragma unroll
    for (int k = 0; k < N; ++k) s_red[(tid >> 6) * N + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    T a = s_red[k];
    for (int w = 1; w < PV_W; ++w) a += s_red[w * N + k];
    v[k] = a;
  }
}

// d = |x - y|
__device__ __forceinline__ float pv_plain(const float x[3], const float y[3]) {
  const float dx = x[0] - y[0], dy = x[1] - y[1], dz = x[2] - y[2];
  return sqrtf((dx * dx + dy * dy) + dz * dz);
}
// e = |scale R x + t - y|, the statements of evalk.h
__device__ __forceinline__ float pv_aligned(const float x[3], const float y[3], const float R[3][3], float scale, const float t[3]) {
  float d2 = 0.f;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float h = scale * (R[r][0] * x[0] + R[r][1] * x[1] + R[r][2] * x[2]) + t[r];
    const float d = h - y[r];
    d2 += d * d;
  }
  return sqrtf(d2);
}
// the fixed-point value of a distance; 0 for one that fails v < ERR_CAP (its pose is then not counted)
__device__ __forceinline__ long long pv_fixed(float v) { return v < ERR_CAP ? __float2ll_rn(v * PV_FIXED) : 0ll; }

template <bool SMALL>
__global__ __launch_bounds__(PV_T) void k_vertex_error(const float* __restrict__ pred, const float* __restrict__ gt,
                                                       const float* __restrict__ root_pred, const float* __restrict__ root_gt,
                                                       const int* __restrict__ group, const int* __restrict__ part, int n_parts, int batch,
                                                       int n, int n_groups, float* __restrict__ pve, float* __restrict__ pa_pve,
                                                       float* __restrict__ err_v, float* __restrict__ err_pa_v,
                                                       long long* __restrict__ acc, long long* __restrict__ acc_v) {
  __shared__ long long s_v[SMALL ? 2 * PV_SMALL : 1];      // SMALL: the workgroup's share of the per-vertex table
  __shared__ double s_red[PV_W * 10];
  __shared__ long long s_redi[PV_W * 2];
  __shared__ long long s_part[2][PV_W][PV_PARTS];          // per wave: plain | aligned fixed-point sums of the pose's parts
  __shared__ int s_np[PV_PARTS];                           // vertices of each part
  const int tid = threadIdx.x, wave = tid >> 6;
  const float nanv = __int_as_float(0x7fc00000);

  if (SMALL && acc_v)
    for (int i = tid; i < 2 * PV_SMALL; i += PV_T) s_v[i] = 0;
  if (part) {
    if (tid < PV_PARTS) s_np[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += PV_T) {
      const int p = part[i];
      if (p >= 0 && p < n_parts) atomicAdd(&s_np[p], 1);
    }
  }
  __syncthreads();

  for (int b = blockIdx.x; b < batch; b += gridDim.x) {
    const float* P = pred + (size_t)b * n * 3;
    const float* Q = gt + (size_t)b * n * 3;
    float rp[3] = {0.f, 0.f, 0.f}, rg[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (root_pred) rp[c] = root_pred[(size_t)b * 3 + c];
      if (root_gt) rg[c] = root_gt[(size_t)b * 3 + c];
    }
    if (part) {                                            // uniform
      for (int i = tid; i < 2 * PV_W * PV_PARTS; i += PV_T) (&s_part[0][0][0])[i] = 0;      // read last before the previous pose's final barrier
      __syncthreads();
    }

    float cx[SMALL ? PV_NPT : 1][3], cy[SMALL ? PV_NPT : 1][3];      // SMALL: x, y of the thread's vertices
    // f(i, x, y) for each of the thread's vertices in ascending order; FIRST: from memory (and into the registers), else from wherever they are
    auto each = [&](auto first, auto&& f) __attribute__((always_inline)) {
      constexpr bool FIRST = decltype(first)::value;
      if constexpr (SMALL) {
        if constexpr (FIRST) {                             // every load in flight at once: a slot past the mesh reads vertex n - 1 and is not used
#pragma unroll
          for (int k = 0; k < PV_NPT; ++k) {
            const int i = min(tid + k * PV_T, n - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              cx[k][c] = P[(size_t)i * 3 + c];
              cy[k][c] = Q[(size_t)i * 3 + c];
            }
          }
#pragma unroll
          for (int k = 0; k < PV_NPT; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) { cx[k][c] -= rp[c]; cy[k][c] -= rg[c]; }
        }
#pragma unroll
        for (int k = 0; k < PV_NPT; ++k) {
          const int i = tid + k * PV_T;
          if (i < n) f(i, cx[k], cy[k]);
          __builtin_amdgcn_sched_barrier(0);               // one vertex at a time: interleaving the 14 bodies costs more registers than there are
        }
      } else {
        for (int i = tid; i < n; i += PV_T) {
          float x[3], y[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            x[c] = P[(size_t)i * 3 + c] - rp[c];
            y[c] = Q[(size_t)i * 3 + c] - rg[c];
          }
          f(i, x, y);
        }
      }
    };
    using First = std::true_type; using Again = std::false_type;

    // whether the pose can reach the per-vertex table is known now; whether its means are NaN only after walk C
    const int gid = group ? group[b] : 0;
    const bool in_range = acc_group_kind(gid, n_groups) == ACC_COUNTED;
    const bool want_v = acc_v && (in_range || (!acc && !group));
    auto add_v = [&](int i, long long qd, long long qe) __attribute__((always_inline)) {
      if constexpr (SMALL) {
        s_v[i] += qd;                                      // vertex i belongs to this thread alone
        s_v[PV_SMALL + i] += qe;
      } else {
        if (qd != 0) acc_add(acc_v + i, qd);
        if (qe != 0) acc_add(acc_v + (size_t)n + i, qe);
      }
    };

    // walk A: the plain error, the sums of x and y
    double sm[6] = {0., 0., 0., 0., 0., 0.};
    long long si[2] = {0, 0};                              // the fixed-point sum; vertices that fail d < ERR_CAP
    each(First{}, [&](int i, const float* x, const float* y) __attribute__((always_inline)) {
      const float d = pv_plain(x, y);
      if (err_v) err_v[(size_t)b * n + i] = d;
      const long long q = pv_fixed(d);
      si[0] += q;
      si[1] += d < ERR_CAP ? 0 : 1;
      if (want_v) add_v(i, q, 0);
      if (part) {
        const int p = part[i];
        if (p >= 0 && p < n_parts) acc_add(&s_part[0][wave][p], q);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) { sm[c] += (double)x[c]; sm[3 + c] += (double)y[c]; }
    });
    pv_block_sum(sm, s_red, tid);
    pv_block_sum(si, s_redi, tid);
    const long long S = si[0];
    const bool plain_ok = si[1] == 0;
    const float v_pve = plain_ok ? (float)((double)S / ((double)n * 16777216.0)) : nanv;
    double m1[3], m2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { m1[c] = sm[c] / (double)n; m2[c] = sm[3 + c] / (double)n; }

    // walk B: K and var1 about the double means
    double sk[10] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
    each(Again{}, [&](int, const float* x, const float* y) __attribute__((always_inline)) {
      double a[3], c2[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { a[c] = (double)x[c] - m1[c]; c2[c] = (double)y[c] - m2[c]; }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) sk[r * 3 + c] += a[r] * c2[c];
      sk[9] += (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    });
    pv_block_sum(sk, s_red, tid);
    float K[3][3], mu1[3], mu2[3], R[3][3], scale, t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      mu1[r] = (float)m1[r];
      mu2[r] = (float)m2[r];
#pragma unroll
      for (int c = 0; c < 3; ++c) K[r][c] = (float)sk[r * 3 + c];
    }
    procrustes_fit(K, (float)sk[9], mu1, mu2, R, scale, t);

    // walk C: the aligned error
    si[0] = 0; si[1] = 0;
    each(Again{}, [&](int i, const float* x, const float* y) __attribute__((always_inline)) {
      const float e = pv_aligned(x, y, R, scale, t);
      if (err_pa_v) err_pa_v[(size_t)b * n + i] = e;
      const long long q = pv_fixed(e);
      si[0] += q;
      si[1] += e < ERR_CAP ? 0 : 1;
      if (want_v) add_v(i, 0, q);
      if (part) {
        const int p = part[i];
        if (p >= 0 && p < n_parts) acc_add(&s_part[1][wave][p], q);
      }
    });
    pv_block_sum(si, s_redi, tid);                         // its barriers also order the ds atomics of s_part before the reads below
    const float v_pa = si[1] == 0 ? (float)((double)si[0] / ((double)n * 16777216.0)) : nanv;
    if (tid == 0) {
      if (pve) pve[b] = v_pve;
      if (pa_pve) pa_pve[b] = v_pa;
    }

    // the tables (uniform branches: every thread holds the same values)
    const bool counted = (in_range || (!acc && !group)) && v_pve == v_pve && v_pa == v_pa;
    if (acc) {
      long long* row = acc_row(acc, JRR_PVE_ACC_ROW, in_range ? gid : 0);
      if (tid == 0) {
        if (long long* t = acc_refused(acc, JRR_PVE_ACC_ROW, n_groups, gid)) acc_add(t, 1);
        else if (!counted) acc_add(row + JRR_PVE_ACC_BAD, 1);
        else {
          acc_add(row + JRR_PVE_ACC_COUNT, 1);
          acc_add(row + JRR_PVE_ACC_SUM, __float2ll_rn(v_pve * PV_FIXED));
          acc_add(row + JRR_PVE_ACC_SUM_PA, __float2ll_rn(v_pa * PV_FIXED));
          acc_add(row + JRR_PVE_ACC_HIST + min((int)floorf(v_pve * 1000.f), JRR_PVE_ACC_BINS - 1), 1);
          acc_add(row + JRR_PVE_ACC_HIST_PA + min((int)floorf(v_pa * 1000.f), JRR_PVE_ACC_BINS - 1), 1);
        }
      }
      if (part && counted && in_range && tid >= 64 && tid < 64 + 2 * PV_PARTS) {      // one thread per (plain | aligned, part), off wave 0
        const int which = (tid - 64) / PV_PARTS, p = (tid - 64) % PV_PARTS;
        if (p < n_parts && s_np[p] > 0) {
          long long s = 0;
          for (int w = 0; w < PV_W; ++w) s += s_part[which][w][p];
          const float m = (float)((double)s / ((double)s_np[p] * 16777216.0));
          acc_add(row + (which ? JRR_PVE_ACC_PART_PA : JRR_PVE_ACC_PART) + p, __float2ll_rn(m * PV_FIXED));
        }
      }
    }
    // walk D, for a pose whose means turned out NaN: what walks A and C added to the per-vertex table is taken out again (the same
    // statements on the same values give the same integers; integer adds cancel exactly)
    if (want_v && !counted) {
      each(Again{}, [&](int i, const float* x, const float* y) __attribute__((always_inline)) {
        add_v(i, -pv_fixed(pv_plain(x, y)), -pv_fixed(pv_aligned(x, y, R, scale, t)));
      });
    }
    __syncthreads();                                       // s_part is zeroed again at the top
  }

  if (SMALL && acc_v)
    for (int i = tid; i < n; i += PV_T) {                  // the thread's own words: no barrier needed
      const long long qd = s_v[i], qe = s_v[PV_SMALL + i];
      if (qd != 0) acc_add(acc_v + i, qd);
      if (qe != 0) acc_add(acc_v + (size_t)n + i, qe);
    }
}

}  // namespace jrr

using namespace jrr;

extern "C" int jrr_vertex_error(const float* pred, const float* gt, const float* root_pred, const float* root_gt, const int32_t* group,
                                const int32_t* part, int n_parts, int batch, int n_verts, int n_groups, float* pve, float* pa_pve,
                                float* err_v, float* err_pa_v, int64_t* acc, int64_t* acc_v, void* stream) {
  const char* why = nullptr;
  if (!pred || !gt) why = "bad argument (pred and gt are required)";
  else if (!pve && !pa_pve && !err_v && !err_pa_v && !acc && !acc_v) why = "no output: pve, pa_pve, err_v, err_pa_v, acc and acc_v are all NULL";
  else if (batch < 0 || n_verts < 1 || n_verts > JRR_PVE_MAX_VERTS) why = "batch must be >= 0, n_verts in 1 .. 65536";
  else if (part && (n_parts < 1 || n_parts > JRR_PVE_MAX_PARTS)) why = "n_parts must lie in 1 .. 32 when part is given";
  else if ((((uintptr_t)pred | (uintptr_t)gt | (uintptr_t)root_pred | (uintptr_t)root_gt | (uintptr_t)group | (uintptr_t)part | (uintptr_t)pve |
             (uintptr_t)pa_pve | (uintptr_t)err_v | (uintptr_t)err_pa_v) & 3) != 0 || !acc_aligned(acc, acc_v))
    why = "the float and int32 arrays must be 4-byte aligned, acc and acc_v 8-byte aligned";
  if (why) {
    jrr_set_error("jrr_vertex_error: %s", why);
    return JRR_ERR_ARG;
  }
  if ((acc || (acc_v && group)) && acc_groups_refused("jrr_vertex_error", n_groups)) return JRR_ERR_ARG;
  if (batch == 0) return JRR_OK;
  long long* a = reinterpret_cast<long long*>(acc);
  long long* av = reinterpret_cast<long long*>(acc_v);
  if (n_verts <= PV_SMALL)
    hipLaunchKernelGGL(k_vertex_error<true>, dim3((unsigned)min(batch, PV_GRID_SMALL)), dim3(PV_T), 0, (hipStream_t)stream, pred, gt, root_pred,
                       root_gt, group, part, n_parts, batch, n_verts, n_groups, pve, pa_pve, err_v, err_pa_v, a, av);
  else
    hipLaunchKernelGGL(k_vertex_error<false>, dim3((unsigned)min(batch, PV_GRID_LARGE)), dim3(PV_T), 0, (hipStream_t)stream, pred, gt, root_pred,
                       root_gt, group, part, n_parts, batch, n_verts, n_groups, pve, pa_pve, err_v, err_pa_v, a, av);
  CHECK_LAUNCH();
  return JRR_OK;
}
