// The second moments of a range of cache rows of the regressor fit (`--fit_solve`; include/jrr.h, jrr_jfit_moments): with the meshes
// fixed the loss of jrr_jfit_run is a quadratic in the normalised weights whose data are the sums below, so one pass over the table
// gives the exact constrained solve (regressor_solve.py) everything it needs.  State and cache: jfitk.h.
//
// A cache row is W = ns + 17 points (the support vertices, then the ground truth in mm) of 3 floats.  For rows [begin, begin + count)
//   M[w][w'] = sum over rows and axes c of row[3 w + c] * row[3 w' + c]                  (W x W doubles, symmetric)
// i.e. M = X^T X with X[(sample, axis)][w].  A product of two fp32 values is exact in fp64, so the only rounding is in the sums.
//
// k_jmom_partial  grid (tile blocks, row chunks), 256 threads.  M is cut into 16 x 16 tiles, of which the T (T + 1) / 2 upper-triangular
//   ones (T = ceil(W / 16)) are numbered row by row; a tile block is JM_TPB = 16 consecutive tiles, four per wave, each a 4-double
//   accumulator per lane.  The workgroup stages its chunk of rows in LDS in runs of whole cache rows (contiguous: coalesced 4-byte
//   loads; 32 rows at once for the shipped support, fewer for a wide one; 30 KB, so that several workgroups share a CU and one's loads
//   run under another's products) and feeds v_mfma_f64_16x16x4_f64 from there: the k index of
//   one instruction is 4 consecutive staged samples of one axis, lane l holds A[i = l & 15][k = l >> 4] = X[(s0 + (l >> 4), c)][16 ti + i]
//   and B[k = l >> 4][j = l & 15] = X[(s0 + (l >> 4), c)][16 tj + j], one LDS float each, converted on the way (the odd row stride and
//   the stride-3 point index keep the 16 x 4 reads on different banks); a sample behind the run and a point behind W read as zero.
//   D: col j = l & 15, row i = (l >> 4) + 4 reg -- the f64 map, NOT the f32 one -- so element (i, j) of the tile is word l + 64 reg
//   of the tile's 256-double slab entry.  The workgroup writes slab[chunk][tile].
// k_jmom_finish   one workgroup per tile, four threads per element: thread g adds the g-th quarter of the chunks' slabs in chunk order
//   (eight loads in flight), thread 0 then adds the four quarters in order and writes M[gi][gj] and its mirror M[gj][gi] (of a diagonal
//   tile only the elements with i <= j, so that the two triangles hold the same bits).  The order is a function of the chunk count alone.
// No floating-point atomics: M is a function of the rows, begin and count alone.
#include "jfitk.h"

namespace jrr {

constexpr int JM_TPW = 4;                             // tiles per wave
constexpr int JM_TPB = JM_TPW * (JF_THREADS / 64);    // 16 tiles per workgroup
constexpr int JM_STAGE = 7680;                        // floats of staged cache rows (30 720 B): 32 rows of the shipped support
constexpr int JM_ROWS = 32;                           // most rows per staging pass
constexpr int JM_FIN_GROUPS = 4;                      // k_jmom_finish: the chunks are added in four consecutive groups, then the groups
constexpr int JM_FIN_THREADS = 256 * JM_FIN_GROUPS;
constexpr int JM_CHUNK_ROWS = JRR_JFIT_MOM_CHUNK;     // rows per chunk at most, unless the chunk count is capped
constexpr int JM_MAX_CHUNKS = JRR_JFIT_MOM_MAX_CHUNKS;
constexpr int JM_MIN_CHUNKS = 4;
constexpr size_t JM_SLAB_BUDGET = (size_t)32 << 20;   // the scratch holds as many chunks' slabs as fit this, 4 .. 1024

static_assert(JM_STAGE >= 3 * JF_CAP + JF_GT + 1, "one cache row of the widest support must fit the staging area");
static_assert(JM_STAGE * 4 <= 64 * 1024, "static LDS");

typedef double jm_d4 __attribute__((ext_vector_type(4)));

__host__ __device__ static inline int jm_tiles_1d(int ns) { return (ns + NH + 15) >> 4; }
__host__ __device__ static inline int jm_tiles(int ns) { const int T = jm_tiles_1d(ns); return T * (T + 1) / 2; }
static inline int jm_max_chunks(int ns) {
  const size_t slab = (size_t)jm_tiles(ns) * 256 * 8;
  const size_t fit = JM_SLAB_BUDGET / slab;
  return (int)(fit < (size_t)JM_MIN_CHUNKS ? (size_t)JM_MIN_CHUNKS : (fit > (size_t)JM_MAX_CHUNKS ? (size_t)JM_MAX_CHUNKS : fit));
}
// tile t of the row-by-row numbering of the upper triangle -> (ti, tj), ti <= tj
__device__ static inline void jm_tile(int t, int T, int& ti, int& tj) {
  int i = 0;
  while (t >= T - i) { t -= T - i; ++i; }
  ti = i;
  tj = i + t;
}

__global__ __launch_bounds__(JF_THREADS) void k_jmom_partial(void* state, const float* __restrict__ cache, long long begin, int count, int ns,
                                                             int rpc, int NT, double* __restrict__ slabs) {
  __shared__ float s_stage[JM_STAGE];
  const JfState st = jf_carve(state);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (st.head[JF_H_NS] != ns) {                       // uniform over the launch; k_jmom_finish writes NaN
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) atomicOr(&st.head[JF_H_ERR], JF_ERR_NS);
    return;
  }
  const int W = ns + NH, T = jm_tiles_1d(ns), RL = jf_row_floats(ns);
  const int sub = min(JM_ROWS, JM_STAGE / RL);        // >= 1 (static_assert above)
  const int chunk = blockIdx.y, r0 = chunk * rpc, rn = min(rpc, count - r0);
  const int q = lane >> 4, l15 = lane & 15;
  int oa[JM_TPW], ob[JM_TPW];                         // float offsets of the lane's A and B points in a staged row; -1: behind W
  bool has[JM_TPW];
#pragma unroll
  for (int j = 0; j < JM_TPW; ++j) {
    const int t = (int)blockIdx.x * JM_TPB + wave * JM_TPW + j;
    has[j] = t < NT;
    int ti = 0, tj = 0;
    if (has[j]) jm_tile(t, T, ti, tj);
    const int wa = 16 * ti + l15, wb = 16 * tj + l15;
    oa[j] = wa < W ? 3 * wa : -1;
    ob[j] = wb < W ? 3 * wb : -1;
  }
  jm_d4 acc[JM_TPW];
#pragma unroll
  for (int j = 0; j < JM_TPW; ++j) acc[j] = jm_d4{0.0, 0.0, 0.0, 0.0};

  for (int s0 = 0; s0 < rn; s0 += sub) {
    const int sn = min(sub, rn - s0);
    const float* src = cache + (size_t)(begin + r0 + s0) * RL;
    for (int x = tid; x < sn * RL; x += JF_THREADS) s_stage[x] = src[x];
    __syncthreads();
    for (int k0 = 0; k0 < sn; k0 += 4) {
      const bool ok = k0 + q < sn;
      const int base = ok ? (k0 + q) * RL : 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int j = 0; j < JM_TPW; ++j) {
          if (has[j]) {                               // uniform over the wave
            const bool ua = ok && oa[j] >= 0, ub = ok && ob[j] >= 0;
            const float fa = s_stage[ua ? base + oa[j] + c : 0], fb = s_stage[ub ? base + ob[j] + c : 0];
            const double a = ua ? (double)fa : 0.0, b = ub ? (double)fb : 0.0;
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < JM_TPW; ++j) {
    if (has[j]) {
      const int t = (int)blockIdx.x * JM_TPB + wave * JM_TPW + j;
      double* o = slabs + ((size_t)chunk * NT + t) * 256;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[lane + 64 * r] = acc[j][r];
    }
  }
}

__global__ __launch_bounds__(JM_FIN_THREADS) void k_jmom_finish(void* state, const double* __restrict__ slabs, int nc, int ns, int NT,
                                                                double* __restrict__ M) {
  __shared__ double s_part[JM_FIN_GROUPS][256];
  const JfState st = jf_carve(state);
  const int t = blockIdx.x, el = threadIdx.x & 255, grp = threadIdx.x >> 8;        // one workgroup per tile
  const bool foreign = st.head[JF_H_NS] != ns;        // uniform
  // group g adds the chunks [g per, (g + 1) per) in order, eight loads in flight at a time
  const int per = (nc + JM_FIN_GROUPS - 1) / JM_FIN_GROUPS, k1 = min(nc, (grp + 1) * per);
  double sum = 0.0;
  if (!foreign) {
    const double* p = slabs + (size_t)t * 256 + el;
    const size_t stride = (size_t)NT * 256;
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
  if (grp != 0) return;
#pragma unroll
  for (int g = 1; g < JM_FIN_GROUPS; ++g) sum += s_part[g][el];
  if (foreign) sum = __longlong_as_double(0x7ff8000000000000ll);
  const int W = ns + NH, T = jm_tiles_1d(ns);
  int ti, tj;
  jm_tile(t, T, ti, tj);
  const int i = el >> 4, j = el & 15, gi = 16 * ti + i, gj = 16 * tj + j;
  if (gi >= W || gj >= W || (ti == tj && i > j)) return;
  M[(size_t)gi * W + gj] = sum;
  M[(size_t)gj * W + gi] = sum;
}

}  // namespace jrr

using namespace jrr;

extern "C" size_t jrr_jfit_moments_bytes(int ns, size_t* scratch_bytes) {
  if (scratch_bytes) *scratch_bytes = 0;
  if (ns < 1 || ns > JF_CAP) return 0;
  if (scratch_bytes) *scratch_bytes = (size_t)jm_max_chunks(ns) * jm_tiles(ns) * 256 * 8;
  return (size_t)(ns + NH) * (ns + NH) * 8;
}

extern "C" int jrr_jfit_moments(void* state, const void* cache, int64_t n_rows, int64_t begin, int64_t count, int ns, double* M, void* scratch,
                                size_t scratch_bytes, void* stream) {
  const char* why = jf_check_cache(state, cache, n_rows, ns);
  if (!why && (!M || !scratch || (((uintptr_t)M | (uintptr_t)scratch) & 7) != 0)) why = "M and scratch are required, 8-byte aligned";
  if (!why && (count < 0 || begin < 0 || begin > n_rows || count > n_rows - begin)) why = "rows [begin, begin + count) must lie inside the cache";
  if (why) {
    jrr_set_error("jrr_jfit_moments: %s", why);
    return JRR_ERR_ARG;
  }
  const int NT = jm_tiles(ns), max_chunks = jm_max_chunks(ns);
  const size_t need = (size_t)max_chunks * NT * 256 * 8;
  if (scratch_bytes < need) {
    jrr_set_error("jrr_jfit_moments: the scratch needs the %zu bytes jrr_jfit_moments_bytes gives for ns = %d", need, ns);
    return JRR_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const int W = ns + NH;
  if (count == 0) {
    JRR_HIP(hipMemsetAsync(M, 0, (size_t)W * W * 8, s));
    return JRR_OK;
  }
  int64_t nc = (count + JM_CHUNK_ROWS - 1) / JM_CHUNK_ROWS;
  if (nc > max_chunks) nc = max_chunks;
  const int64_t rpc = (count + nc - 1) / nc;          // rows per chunk; every chunk [k rpc, min((k + 1) rpc, count)) is non-empty
  nc = (count + rpc - 1) / rpc;
  hipLaunchKernelGGL(k_jmom_partial, dim3((unsigned)((NT + JM_TPB - 1) / JM_TPB), (unsigned)nc), dim3(JF_THREADS), 0, s, state,
                     reinterpret_cast<const float*>(cache), (long long)begin, (int)count, ns, (int)rpc, NT, reinterpret_cast<double*>(scratch));
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_jmom_finish, dim3((unsigned)NT), dim3(JM_FIN_THREADS), 0, s, state, reinterpret_cast<const double*>(scratch), (int)nc, ns, NT, M);
  CHECK_LAUNCH();
  return JRR_OK;
}
