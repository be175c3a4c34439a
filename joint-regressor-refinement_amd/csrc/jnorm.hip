// The reweighted second moments of a range of cache rows of the regressor fit (`--fit_solve --fit_solve_loss mpjpe`; include/jrr.h,
// jrr_jfit_norm_moments): one pass gives the smoothed MPJPE of the weights x, its exact gradient, the Frank-Wolfe gap and the quadratic
// majoriser whose minimiser is the next iterate (regressor_solve.py, solve_norm).  State and cache: jfitk.h.  Only the LISTS of the state
// are read (the rows' counts, and each entry's position in the union); the weights are the caller's doubles x[17][128].
//
// Per cache row s and joint i = 1 .. 16 with entries:  r = x_i . v - x_0 . v - gt_i / 1000  (3 doubles, m),  rho = sqrt(r.r + delta^2),
// w = 1 / rho (INV) or 1 (UNIT).  The points p_a of joint i are the vertices of row i's entries, then those of row 0's: K_i = cnt_i + cnt_0.
//   A_i[a][b] = sum_s w sum_c p_a,c p_b,c      b_i[a] = sum_s w sum_c r_c p_a,c      and the scalars sum rho, sum |r|, sum w, samples.
// b is computed as one more column of A: the residual r joins the points as the VIRTUAL point K_i, so that the extended Gram
// A~[a][K_i] = b[a] comes out of the same products (A~[K_i][K_i] = sum w |r|^2 is not stored).
//
// k_jnorm_partial  grid (item blocks, row chunks), 256 threads.  An item is one 16 x 16 upper-triangular tile of one joint's extended
//   Gram (T_i = ceil((K_i + 1) / 16) tiles a side, numbered row by row, the joints in order); an item block is JN_IPB = 16 consecutive
//   items, four per wave, each a 4-double accumulator per lane.  The workgroup stages its chunk in LDS in runs of whole cache rows with
//   the odd stride, exactly as k_jmom_partial.  Per staged run:
//     residuals  for every (sample, joint of this block's items): P lanes (1, 4 or 16 by the longest point list: a function of the
//                counts alone) share the K_i entries, entry e to lane e mod P, each sum in list order, then a butterfly over the P lanes;
//                r and w go to LDS.  In LDS and not in a first launch into a scratch array: for the shipped support one item
//                block holds every joint, so each residual is computed once either way, and a scratch of 4 doubles per (sample, joint)
//                would add 512 bytes of traffic per row to the 900 the pass reads.  A wide support recomputes them in every item block
//                (6 blocks at NS = 380), which is why the entries of one residual are spread over P lanes there.
//     scalars    thread (joint, k < 3) adds w / rho / |r| (the last two formed again from r: the same bits) over the run's samples in
//                order into a register it keeps;
//     products   v_mfma_f64_16x16x4_f64 with k = 4 consecutive staged samples of one axis: lane l holds A = w * point (16 ti + (l & 15)),
//                B = point (16 tj + (l & 15)) of sample s0 + (l >> 4); C/D: col = l & 15, row = (l >> 4) + 4 reg -- the f64 map.
//   The workgroup writes slab[chunk][item]; the block that owns a joint's first item also writes the joint's three scalars into the
//   pseudo-item NT of its chunk.
// k_jnorm_finish   one workgroup per item (and one for the scalars), k_jmom_finish's four groups of chunks in chunk order; writes
//   A_i[gi][gj] and its mirror from the same sum, b_i[gi] from column K_i, the scalars and the sample count.
// No floating-point atomics, no scratch memory, plain vector stores: the output is a function of the rows, the lists, x, mode, delta,
// begin and count alone.
#include "jfitk.h"

#include <cmath>

namespace jrr {

constexpr int JN_TPW = 4;                             // items per wave
constexpr int JN_IPB = JN_TPW * (JF_THREADS / 64);    // 16 items per workgroup
constexpr int JN_STAGE = 7680;                        // floats of staged cache rows (30 720 B): 32 rows of the shipped support
constexpr int JN_ROWS = 32;                           // most rows per staging pass
constexpr int JN_NJ = NH - 1;                         // 16 joints with a block
constexpr int JN_RW = 4;                              // doubles per (sample, joint) in LDS: r[3], w
constexpr int JN_FIN_GROUPS = 4;
constexpr int JN_FIN_THREADS = 256 * JN_FIN_GROUPS;
constexpr int JN_CHUNK_ROWS = 64;
constexpr int JN_MAX_CHUNKS = 1024;
constexpr int JN_MIN_CHUNKS = 4;
constexpr size_t JN_SLAB_BUDGET = (size_t)32 << 20;

static_assert(JN_STAGE >= 3 * JF_CAP + JF_GT + 1, "one cache row of the widest support must fit the staging area");
static_assert(JN_STAGE * 4 + JN_ROWS * JN_NJ * JN_RW * 8 + 1024 <= 48 * 1024, "static LDS");

typedef double jn_d4 __attribute__((ext_vector_type(4)));

// the layout: K_i, tiles a side, items, offsets -- functions of the counts alone
struct JnLayout {
  int K[NH], T[NH], first[NH + 1];                    // first[i]: the first item of joint i; first[NH] = NT
  long long off[NH + 1];                              // off[i]: the first double of joint i's block; off[NH]: the total
  int maxK;
};
__host__ __device__ static inline bool jn_layout(const int* counts, JnLayout& L) {
  int nt = 0;
  long long o = 0;
  L.maxK = 0;
  L.K[0] = L.T[0] = 0;
  L.first[0] = 0;
  L.off[0] = 0;
  bool ok = counts[0] >= 0 && counts[0] <= JSUP_CAP;
  for (int i = 1; i < NH; ++i) {
    const int c = counts[i];
    if (c < 0 || c > JSUP_CAP) ok = false;
    const int K = (ok && c > 0) ? c + counts[0] : 0;
    L.K[i] = K;
    L.T[i] = K > 0 ? (K + 1 + 15) >> 4 : 0;
    L.first[i] = nt;
    L.off[i] = o;
    nt += L.T[i] * (L.T[i] + 1) / 2;
    o += (long long)K * K + K + 4;
    if (K > L.maxK) L.maxK = K;
  }
  L.first[NH] = nt;
  L.off[NH] = o;
  return ok;
}
static inline int jn_max_chunks(int NT) {
  const size_t slab = (size_t)(NT + 1) * 256 * 8;
  const size_t fit = JN_SLAB_BUDGET / slab;
  return (int)(fit < (size_t)JN_MIN_CHUNKS ? (size_t)JN_MIN_CHUNKS : (fit > (size_t)JN_MAX_CHUNKS ? (size_t)JN_MAX_CHUNKS : fit));
}
// lanes per (sample, joint) of the residual phase
static inline int jn_lanes(int maxK) { return maxK <= 16 ? 1 : (maxK <= 64 ? 4 : 16); }

__device__ static inline void jn_tile(int t, int T, int& ti, int& tj) {
  int i = 0;
  while (t >= T - i) { t -= T - i; ++i; }
  ti = i;
  tj = i + t;
}
// item t -> its joint (1 .. 16) and tile
__device__ static inline void jn_item(const int* first, const int* T, int t, int& joint, int& ti, int& tj) {
  int i = 1;
  while (i < NH - 1 && t >= first[i + 1]) ++i;
  joint = i;
  jn_tile(t - first[i], T[i], ti, tj);
}

// the lists of the state, clamped so that nothing reads behind the state whatever it holds: one thread fills the shared arrays
// (blk nullable: the first double of each joint's block)
__device__ static inline void jn_lists(const JfState& st, int* cnt, int* off, int* T, int* first, long long* blk) {
  const int E = min(max(st.head[JF_H_E], 0), JF_CAP);
  int nt = 0;
  long long o8 = 0;
  int c0 = 0;
  for (int i = 0; i < NH; ++i) {
    const int o = min(max(st.head[JF_H_OFF + i], 0), E);
    const int c = min(min(max(st.head[JF_H_CNT + i], 0), JSUP_CAP), E - o);
    if (i == 0) c0 = c;
    off[i] = o;
    cnt[i] = c;
    const int K = (i > 0 && c > 0) ? c + c0 : 0;
    const int t = K > 0 ? (K + 1 + 15) >> 4 : 0;
    T[i] = t;
    first[i] = nt;
    if (blk) blk[i] = o8;
    nt += t * (t + 1) / 2;
    o8 += (long long)K * K + K + (i > 0 ? 4 : 0);
  }
  first[NH] = nt;
}

__global__ __launch_bounds__(JF_THREADS) void k_jnorm_partial(void* state, const float* __restrict__ cache, long long begin, int count, int ns,
                                                              int rpc, int NT, int P, const double* __restrict__ x, int mode, double delta,
                                                              double* __restrict__ slabs) {
  __shared__ float s_stage[JN_STAGE];
  __shared__ double s_rw[JN_ROWS * JN_NJ * JN_RW];
  __shared__ int s_cnt[NH], s_off[NH], s_T[NH], s_first[NH + 1];
  const JfState st = jf_carve(state);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (st.head[JF_H_NS] != ns) {                       // uniform over the launch; k_jnorm_finish writes NaN
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) atomicOr(&st.head[JF_H_ERR], JF_ERR_NS);
    return;
  }
  if (tid == 0) jn_lists(st, s_cnt, s_off, s_T, s_first, nullptr);
  __syncthreads();
  if (s_first[NH] != NT) return;                      // (the lists changed behind the host's back: uniform; the slabs stay as they are)
  const int RL = jf_row_floats(ns);
  const int sub = min(JN_ROWS, JN_STAGE / RL);        // >= 1 (static_assert above)
  const int chunk = blockIdx.y, r0 = chunk * rpc, rn = min(rpc, count - r0);
  const int q = lane >> 4, l15 = lane & 15;
  const int t_first = (int)blockIdx.x * JN_IPB, t_last = min(t_first + JN_IPB, NT) - 1;
  int jlo, jhi, d0, d1;
  jn_item(s_first, s_T, t_first, jlo, d0, d1);
  jn_item(s_first, s_T, t_last, jhi, d0, d1);
  const int nj = jhi - jlo + 1;                       // 1 .. 16 joints, empty ones between them included
  const int cnt0 = s_cnt[0], off0 = s_off[0];

  // the wave's items: the lane's A and B points as float offsets in a staged row; -1: behind the list (zero), -2: the residual
  int oa[JN_TPW], ob[JN_TPW], jl[JN_TPW];
  bool has[JN_TPW];
#pragma unroll
  for (int j = 0; j < JN_TPW; ++j) {
    const int t = t_first + wave * JN_TPW + j;
    has[j] = t < NT;
    int joint = jlo, ti = 0, tj = 0;
    if (has[j]) jn_item(s_first, s_T, t, joint, ti, tj);
    jl[j] = joint - jlo;
    const int ci = s_cnt[joint], K = ci + cnt0;
    const int pa = 16 * ti + l15, pb = 16 * tj + l15;
    int o[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int p = h ? pb : pa;
      if (p < K) {
        const int idx = p < ci ? s_off[joint] + p : off0 + (p - ci);
        o[h] = 3 * min(st.pk[idx] & 0xffff, ns - 1);
      } else {
        o[h] = p == K ? -2 : -1;
      }
    }
    oa[j] = o[0];
    ob[j] = o[1];
  }
  jn_d4 acc[JN_TPW];
#pragma unroll
  for (int j = 0; j < JN_TPW; ++j) acc[j] = jn_d4{0.0, 0.0, 0.0, 0.0};
  double scal = 0.0;                                  // thread (joint tid >> 2, k = tid & 3 < 3): sum w, sum rho, sum |r|
  const int sj = tid >> 2, sk = tid & 3;
  const double d2 = delta * delta;
  const int part = tid & (P - 1), pairs_per_pass = JF_THREADS / P;

  for (int s0 = 0; s0 < rn; s0 += sub) {
    const int sn = min(sub, rn - s0);
    const float* src = cache + (size_t)(begin + r0 + s0) * RL;
    for (int k = tid; k < sn * RL; k += JF_THREADS) s_stage[k] = src[k];
    __syncthreads();
    // residuals: pair = (sample, joint of the block), P lanes per pair
    for (int pair0 = 0; pair0 < sn * nj; pair0 += pairs_per_pass) {
      const int pair = pair0 + tid / P;
      const bool on = pair < sn * nj;
      const int s = on ? pair / nj : 0, jj = on ? pair - s * nj : 0, joint = jlo + jj;
      const int ci = on ? s_cnt[joint] : 0, K = ci > 0 ? ci + cnt0 : 0, offi = s_off[joint];
      const float* vs = s_stage + s * RL;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0;
      for (int e = part; e < K; e += P) {
        const bool own = e < ci;
        const int idx = own ? offi + e : off0 + (e - ci);
        const double wt = own ? x[joint * JSUP_CAP + e] : -x[e - ci];
        const int p = 3 * min(st.pk[idx] & 0xffff, ns - 1);
        a0 += wt * (double)vs[p];
        a1 += wt * (double)vs[p + 1];
        a2 += wt * (double)vs[p + 2];
      }
      for (int o = P >> 1; o > 0; o >>= 1) {          // (P lanes of one pair are neighbours inside a wave)
        a0 += __shfl_xor(a0, o);
        a1 += __shfl_xor(a1, o);
        a2 += __shfl_xor(a2, o);
      }
      if (on && part == 0) {
        double* o = s_rw + (s * JN_NJ + jj) * JN_RW;
        if (K > 0) {
          const float* g = vs + 3 * ns + 3 * joint;
          const double r0_ = a0 - (double)g[0] / 1000.0, r1_ = a1 - (double)g[1] / 1000.0, r2_ = a2 - (double)g[2] / 1000.0;
          const double rr = r0_ * r0_ + r1_ * r1_ + r2_ * r2_;
          const double rho = sqrt(rr + d2), w = mode == JRR_JFIT_NORM_INV ? 1.0 / rho : 1.0;
          o[0] = r0_; o[1] = r1_; o[2] = r2_; o[3] = w;
        } else {
          o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0;
        }
      }
    }
    __syncthreads();
    if (sj < nj && sk < 3 && s_cnt[jlo + sj] > 0) {
      for (int s = 0; s < sn; ++s) {
        const double* rw = s_rw + (s * JN_NJ + sj) * JN_RW;
        const double rr = rw[0] * rw[0] + rw[1] * rw[1] + rw[2] * rw[2];
        scal += sk == 0 ? rw[3] : sqrt(sk == 1 ? rr + d2 : rr);
      }
    }
    for (int k0 = 0; k0 < sn; k0 += 4) {
      const bool ok = k0 + q < sn;
      const int srow = ok ? k0 + q : 0, base = srow * RL;
#pragma unroll
      for (int j = 0; j < JN_TPW; ++j) {
        if (has[j]) {                                 // uniform over the wave
          const double* rw = s_rw + (srow * JN_NJ + jl[j]) * JN_RW;
          const double w = rw[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float fa = s_stage[oa[j] >= 0 ? base + oa[j] + c : 0], fb = s_stage[ob[j] >= 0 ? base + ob[j] + c : 0];
            const double rc = rw[c];
            double a = oa[j] >= 0 ? (double)fa : (oa[j] == -2 ? rc : 0.0);
            double b = ob[j] >= 0 ? (double)fb : (ob[j] == -2 ? rc : 0.0);
            a = ok ? a * w : 0.0;
            b = ok ? b : 0.0;
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < JN_TPW; ++j) {
    if (has[j]) {
      const int t = t_first + wave * JN_TPW + j;
      double* o = slabs + ((size_t)chunk * (NT + 1) + t) * 256;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[lane + 64 * r] = acc[j][r];
    }
  }
  // the scalars of the joints whose FIRST item lies in this block: word 4 joint' + k of the chunk's pseudo-item NT (joint' = joint - 1)
  if (sj < nj && sk < 3) {
    const int joint = jlo + sj;
    if (s_T[joint] > 0 && s_first[joint] >= t_first && s_first[joint] <= t_last)
      slabs[((size_t)chunk * (NT + 1) + NT) * 256 + 4 * (joint - 1) + sk] = scal;
  }
}

__global__ __launch_bounds__(JN_FIN_THREADS) void k_jnorm_finish(void* state, const double* __restrict__ slabs, int nc, int ns, int NT,
                                                                 long long count, double* __restrict__ out) {
  __shared__ double s_part[JN_FIN_GROUPS][256];
  __shared__ int s_cnt[NH], s_off[NH], s_T[NH], s_first[NH + 1];
  __shared__ long long s_o[NH];
  const JfState st = jf_carve(state);
  const int t = blockIdx.x, el = threadIdx.x & 255, grp = threadIdx.x >> 8;
  const bool foreign = st.head[JF_H_NS] != ns;        // uniform
  if (threadIdx.x == 0) jn_lists(st, s_cnt, s_off, s_T, s_first, s_o);
  const bool scalars = t == NT;
  const bool used = !scalars || el < 4 * JN_NJ;
  const int per = (nc + JN_FIN_GROUPS - 1) / JN_FIN_GROUPS, k1 = min(nc, (grp + 1) * per);
  double sum = 0.0;
  if (!foreign && used) {
    const double* p = slabs + (size_t)t * 256 + el;
    const size_t stride = (size_t)(NT + 1) * 256;
    int k = grp * per;
    for (; k + 8 <= k1; k += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(k + u) * stride];
#pragma unroll
      for (int u = 0; u < 8; ++u) sum += v[u];
    }
    for (; k < k1; ++k) sum += p[(size_t)k * stride];
  }
  s_part[grp][el] = sum;
  __syncthreads();
  if (grp != 0 || !used || s_first[NH] != NT) return;
#pragma unroll
  for (int g = 1; g < JN_FIN_GROUPS; ++g) sum += s_part[g][el];
  const double nanv = __longlong_as_double(0x7ff8000000000000ll);
  if (scalars) {
    const int joint = 1 + (el >> 2), k = el & 3;
    const int K = s_T[joint] > 0 ? s_cnt[joint] + s_cnt[0] : 0;
    double* o = out + s_o[joint] + (long long)K * K + K;
    // order in the block: sum rho, sum |r|, sum w, samples; the slab words are sum w, sum rho, sum |r|
    double v;
    if (K == 0) v = 0.0;
    else if (k == 3) v = (double)count;
    else v = sum;
    if (foreign) v = nanv;
    const int dst = k == 0 ? 2 : (k == 1 ? 0 : (k == 2 ? 1 : 3));
    o[dst] = v;
    return;
  }
  if (foreign) sum = nanv;
  int joint, ti, tj;
  jn_item(s_first, s_T, t, joint, ti, tj);
  const int K = s_cnt[joint] + s_cnt[0];
  const int i = el >> 4, j = el & 15, gi = 16 * ti + i, gj = 16 * tj + j;
  if (gi >= K || gj > K || (ti == tj && i > j)) return;
  double* A = out + s_o[joint];
  if (gj == K) {
    A[(long long)K * K + gi] = sum;                   // b_i
  } else {
    A[(long long)gi * K + gj] = sum;
    A[(long long)gj * K + gi] = sum;
  }
}

}  // namespace jrr

using namespace jrr;

extern "C" size_t jrr_jfit_norm_bytes(const int32_t* counts, size_t* scratch_bytes) {
  if (scratch_bytes) *scratch_bytes = 0;
  if (!counts) return 0;
  int cs[NH];
  for (int i = 0; i < NH; ++i) cs[i] = counts[i];
  JnLayout L;
  if (!jn_layout(cs, L)) return 0;
  const int NT = L.first[NH];
  if (scratch_bytes) *scratch_bytes = (size_t)jn_max_chunks(NT) * (NT + 1) * 256 * 8;
  return (size_t)L.off[NH] * 8;
}

extern "C" int jrr_jfit_norm_moments(void* state, const void* cache, int64_t n_rows, int64_t begin, int64_t count, int ns, const double* x,
                                     int mode, double delta_m, double* out, void* scratch, size_t scratch_bytes, void* stream) {
  const char* why = jf_check_cache(state, cache, n_rows, ns);
  if (!why && (!x || !out || !scratch || (((uintptr_t)x | (uintptr_t)out | (uintptr_t)scratch) & 7) != 0))
    why = "x, out and scratch are required, 8-byte aligned";
  if (!why && (count < 0 || begin < 0 || begin > n_rows || count > n_rows - begin)) why = "rows [begin, begin + count) must lie inside the cache";
  if (!why && mode != JRR_JFIT_NORM_UNIT && mode != JRR_JFIT_NORM_INV) why = "mode must be JRR_JFIT_NORM_UNIT or JRR_JFIT_NORM_INV";
  if (!why && !(std::isfinite(delta_m) && delta_m >= 0.0)) why = "delta_m must be finite and not negative";
  if (!why && mode == JRR_JFIT_NORM_INV && !(delta_m > 0.0)) why = "delta_m must be positive in JRR_JFIT_NORM_INV mode";
  if (why) {
    jrr_set_error("jrr_jfit_norm_moments: %s", why);
    return JRR_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  // the layout is a function of the rows' counts, which live in the state: read them back (synchronises the stream)
  int32_t head[JF_H_CNT + NH];
  JRR_HIP(hipMemcpyAsync(head, state, sizeof(head), hipMemcpyDeviceToHost, s));
  JRR_HIP(hipStreamSynchronize(s));
  int cs[NH];
  for (int i = 0; i < NH; ++i) cs[i] = head[JF_H_CNT + i];
  JnLayout L;
  if (head[JF_H_NS] < 1 || head[JF_H_NS] > JF_CAP || head[JF_H_E] < 1 || head[JF_H_E] > JF_CAP || !jn_layout(cs, L)) {
    jrr_set_error("jrr_jfit_norm_moments: the state is not a prepared one");
    return JRR_ERR_ARG;
  }
  const int NT = L.first[NH], max_chunks = jn_max_chunks(NT);
  const size_t need = (size_t)max_chunks * (NT + 1) * 256 * 8;
  if (scratch_bytes < need) {
    jrr_set_error("jrr_jfit_norm_moments: the scratch needs the %zu bytes jrr_jfit_norm_bytes gives for these counts", need);
    return JRR_ERR_WORKSPACE;
  }
  if (count == 0) {
    JRR_HIP(hipMemsetAsync(out, 0, (size_t)L.off[NH] * 8, s));
    return JRR_OK;
  }
  int64_t nc = (count + JN_CHUNK_ROWS - 1) / JN_CHUNK_ROWS;
  if (nc > max_chunks) nc = max_chunks;
  const int64_t rpc = (count + nc - 1) / nc;          // rows per chunk; every chunk is non-empty
  nc = (count + rpc - 1) / rpc;
  if (NT > 0) {
    hipLaunchKernelGGL(k_jnorm_partial, dim3((unsigned)((NT + JN_IPB - 1) / JN_IPB), (unsigned)nc), dim3(JF_THREADS), 0, s, state,
                       reinterpret_cast<const float*>(cache), (long long)begin, (int)count, ns, (int)rpc, NT, jn_lanes(L.maxK), x, mode, delta_m,
                       reinterpret_cast<double*>(scratch));
    CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_jnorm_finish, dim3((unsigned)(NT + 1)), dim3(JN_FIN_THREADS), 0, s, state, reinterpret_cast<const double*>(scratch), (int)nc,
                     ns, NT, (long long)count, out);
  CHECK_LAUNCH();
  return JRR_OK;
}
