// The price of every mesh vertex in the regressor solve (`--fit_solve --fit_grow R`; include/jrr.h, jrr_jfit_price): for a batch of
// meshes, the rows' lists and the caller's fp64 weights x, the sums
//     S[i][u] = sum_s sum_c a_i,c(s) v[s][u][c]        i = 1 .. 16, u = 0 .. 6889
// from which the host forms the gradient of the loss with respect to a weight on ANY vertex (regressor_solve.price_gradients), and per
// joint sum r.r, sum rho, sum |r| and the samples counted.  r_i = q_i - q_0 - gt_i / 1000 (m), q_i = sum_e x_i[e] v[vtx_i[e]],
// rho = sqrt(r.r + delta^2); the adjoint a_i is r_i (MSE) or r_i / rho (NORM).  No engine, no body model, no jfit state: the lists and
// the weights are host arrays, validated on the host (nothing is launched with a bad index), packed and copied into the head of the
// scratch on the stream; the call waits for that copy (one stream synchronisation, as jrr_jfit_norm_moments pays for its counts).
//
// Scratch:  head (vtx[17][128] int32 | counts[17] int32, padded | x[17][128] double) | per sample 64 doubles: a[c][i - 1] (48), r.r[i - 1]
//           (16) | the chunks' slabs, nc x 431 tiles x 256 doubles (nc <= 38: at most 32 MiB).
// k_jprice_resid    256 threads = 15 samples x 17 rows: thread (sample, row) forms q_row in double in list order; behind a barrier the
//                   threads of rows 1 .. 16 form r, r.r, rho and a and write them.  An empty row writes zeros; an empty pelvis row has q_0 = 0.
// k_jprice_partial  grid (14 tile blocks, nc sample chunks), 256 threads.  A vertex tile is 16 vertices: the 16 joints fill the M side of
//                   v_mfma_f64_16x16x4_f64 exactly.  A wave owns JP_TPW = 8 CONSECUTIVE tiles (a workgroup 32: 6144 contiguous bytes of
//                   one mesh), one 4-double accumulator per tile.  Per group of 4 samples and axis c: lane l holds
//                   A = a[s0 + (l >> 4)][c][l & 15] and B = (double) v[s0 + (l >> 4)][16 t + (l & 15)][c], straight from global memory
//                   (each lane's three axes are 12 contiguous bytes, a quad's 16 lanes 192); C/D: col = l & 15, row = (l >> 4) + 4 reg --
//                   the f64 map.  A sample behind the batch and a vertex behind 6890 enter as zero and are not loaded.
// k_jprice_finish   one workgroup per tile adds the chunks' slabs in chunk order and writes (or adds into) S, nothing behind element
//                   16 * 6890; one more workgroup per joint sums its scalars over the samples: thread p the samples p, p + 256, .. in
//                   order, then a tree of fixed shape over the 256 partial sums.
// No floating-point atomics, no scratch memory, plain vector stores: the output is a function of the meshes, the lists, x, mode, delta
// and the batch size alone; with accumulate, of the sequence of batch sizes.
#include "jrr_common.h"
#include "../../include/jrr.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace jrr {

constexpr int JP_CAP = JRR_JFIT_ROW_CAP;              // 128 entries a row
constexpr int JP_NJ = NH - 1;                         // 16 joints: the M side
constexpr int JP_TILES = (V + 15) / 16;               // 431, the last one with 10 live columns
constexpr int JP_TPW = 8;                             // tiles per wave
constexpr int JP_TPB = JP_TPW * 4;                    // 32 tiles per workgroup
constexpr int JP_THREADS = 256;
constexpr int JP_RS = 15;                             // samples per workgroup of the residual launch: 15 * 17 = 255 threads
constexpr int JP_SD = 64;                             // doubles per sample: a[3][16], r.r[16]
constexpr int JP_MAX_CHUNKS = 38;                     // 38 slabs of 431 * 256 doubles: 31.99 MiB
constexpr int JP_MIN_ROWS = 8;                        // fewest samples per chunk (the last one may be shorter)
constexpr size_t JP_HEAD_VTX = 0, JP_HEAD_CNT = (size_t)NH * JP_CAP * 4, JP_HEAD_X = JP_HEAD_CNT + 128;
constexpr size_t JP_HEAD = JP_HEAD_X + (size_t)NH * JP_CAP * 8;

static_assert((size_t)JP_MAX_CHUNKS * JP_TILES * 256 * 8 <= ((size_t)32 << 20), "the slabs stay within 32 MiB");
static_assert(JP_HEAD_X % 8 == 0 && JP_HEAD % 8 == 0, "the doubles of the scratch are 8-byte aligned");
static_assert(JP_RS * NH <= JP_THREADS, "one thread per (sample, row)");
static_assert(JRR_JFIT_PRICE_DOUBLES == JP_NJ * V + JP_NJ * 4, "output layout");

typedef double jp_d4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) jp_f3 { float x, y, z; };

// chunks and samples per chunk (a multiple of 4: only the last chunk has a partial k group) for a batch
static inline void jp_chunks(int batch, int& nc, int& rpc) {
  const long long b = batch;                                         // (a batch near 2^31 must not overflow the roundings)
  long long n = (b + JP_MIN_ROWS - 1) / JP_MIN_ROWS;
  if (n > JP_MAX_CHUNKS) n = JP_MAX_CHUNKS;
  const long long r = (((b + n - 1) / n) + 3) & ~3ll;
  rpc = (int)r;
  nc = (int)((b + r - 1) / r);
}

__global__ __launch_bounds__(JP_THREADS) void k_jprice_resid(const float* __restrict__ verts, const float* __restrict__ gt, int batch,
                                                             const int* __restrict__ vtx, const int* __restrict__ cnt,
                                                             const double* __restrict__ x, int mode, double delta,
                                                             double* __restrict__ samples) {
  __shared__ double s_q[JP_RS * NH * 3];
  const int tid = threadIdx.x, sl = tid / NH, row = tid - sl * NH;
  const int s = (int)blockIdx.x * JP_RS + sl;
  const bool on = sl < JP_RS && s < batch;
  if (on) {
    const int c = min(max(cnt[row], 0), JP_CAP);
    const float* vs = verts + (size_t)s * V * 3;
    double q0 = 0.0, q1 = 0.0, q2 = 0.0;
    for (int e = 0; e < c; ++e) {
      const int u = min(max(vtx[row * JP_CAP + e], 0), V - 1);       // (validated on the host; the clamp costs nothing)
      const double w = x[row * JP_CAP + e];
      q0 += w * (double)vs[3 * u];
      q1 += w * (double)vs[3 * u + 1];
      q2 += w * (double)vs[3 * u + 2];
    }
    double* q = s_q + (sl * NH + row) * 3;
    q[0] = q0; q[1] = q1; q[2] = q2;
  }
  __syncthreads();
  if (!on || row == 0) return;
  double* o = samples + (size_t)s * JP_SD;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, rr = 0.0;
  if (cnt[row] > 0) {
    const double* q = s_q + (sl * NH + row) * 3;
    const double* p = s_q + (sl * NH) * 3;
    const float* g = gt + ((size_t)s * NH + row) * 3;
    const double r0 = q[0] - p[0] - (double)g[0] / 1000.0, r1 = q[1] - p[1] - (double)g[1] / 1000.0, r2 = q[2] - p[2] - (double)g[2] / 1000.0;
    rr = r0 * r0 + r1 * r1 + r2 * r2;
    if (mode == JRR_JFIT_PRICE_NORM) {
      const double rho = sqrt(rr + delta * delta);
      a0 = r0 / rho; a1 = r1 / rho; a2 = r2 / rho;
    } else {
      a0 = r0; a1 = r1; a2 = r2;
    }
  }
  o[row - 1] = a0;
  o[JP_NJ + row - 1] = a1;
  o[2 * JP_NJ + row - 1] = a2;
  o[3 * JP_NJ + row - 1] = rr;
}

__global__ __launch_bounds__(JP_THREADS) void k_jprice_partial(const float* __restrict__ verts, const double* __restrict__ samples, int batch,
                                                               int rpc, double* __restrict__ slabs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, l15 = lane & 15;
  const int t0 = ((int)blockIdx.x * 4 + wave) * JP_TPW;             // the wave's first tile
  if (t0 >= JP_TILES) return;                                        // uniform over the wave; no barrier in this kernel
  const int chunk = blockIdx.y, s_begin = chunk * rpc, s_end = (int)min((long long)s_begin + rpc, (long long)batch);
  // every load below is unconditional, from an address that exists (a lane behind the batch reads the chunk's first sample, a lane
  // behind the last vertex reads vertex 6889), and what must enter as zero is zeroed in registers: with a branch around each load the
  // compiler drains the load queue behind every one of them
  bool live[JP_TPW];                                                 // this lane's vertex of tile j exists
  int voff[JP_TPW];                                                  // its float offset in a mesh
#pragma unroll
  for (int j = 0; j < JP_TPW; ++j) {
    const int u = 16 * (t0 + j) + l15;
    live[j] = u < V;
    voff[j] = 3 * min(u, V - 1);
  }
  jp_d4 acc[JP_TPW];
#pragma unroll
  for (int j = 0; j < JP_TPW; ++j) acc[j] = jp_d4{0.0, 0.0, 0.0, 0.0};
  double a[3], an[3];
  jp_f3 b[JP_TPW], bn[JP_TPW];
  {
    const int sv = s_begin + q < s_end ? s_begin + q : s_begin;
    const double* ap = samples + (size_t)sv * JP_SD + l15;
    const float* vp = verts + (size_t)sv * V * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = ap[c * JP_NJ];
#pragma unroll
    for (int j = 0; j < JP_TPW; ++j) b[j] = *reinterpret_cast<const jp_f3*>(vp + voff[j]);
  }
  for (int s0 = s_begin; s0 < s_end; s0 += 4) {
    const bool ok = s0 + q < s_end;
    // the next group's operands, in flight under this group's products (behind the last group: the chunk's first sample again, unused)
    const int sn = s0 + 4 + q < s_end ? s0 + 4 + q : s_begin;
    const double* ap = samples + (size_t)sn * JP_SD + l15;
    const float* vp = verts + (size_t)sn * V * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) an[c] = ap[c * JP_NJ];
#pragma unroll
    for (int j = 0; j < JP_TPW; ++j) bn[j] = *reinterpret_cast<const jp_f3*>(vp + voff[j]);
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = ok ? a[c] : 0.0;
#pragma unroll
    for (int j = 0; j < JP_TPW; ++j) {
      const bool on = ok && live[j];
      acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], on ? (double)b[j].x : 0.0, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], on ? (double)b[j].y : 0.0, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[2], on ? (double)b[j].z : 0.0, acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = an[c];
#pragma unroll
    for (int j = 0; j < JP_TPW; ++j) b[j] = bn[j];
  }
#pragma unroll
  for (int j = 0; j < JP_TPW; ++j) {
    if (t0 + j < JP_TILES) {                                         // uniform over the wave
      double* o = slabs + ((size_t)chunk * JP_TILES + (t0 + j)) * 256;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[lane + 64 * r] = acc[j][r];     // element (row = (l >> 4) + 4 r, col = l & 15) at 16 row + col
    }
  }
}

__global__ __launch_bounds__(JP_THREADS) void k_jprice_finish(const double* __restrict__ slabs, const double* __restrict__ samples,
                                                              const int* __restrict__ cnt, int nc, int batch, double delta, int accumulate,
                                                              double* __restrict__ out) {
  const int t = blockIdx.x, el = threadIdx.x;
  if (t < JP_TILES) {
    const int row = el >> 4, u = 16 * t + (el & 15);
    if (u >= V) return;
    const double* p = slabs + (size_t)t * 256 + el;
    const size_t stride = (size_t)JP_TILES * 256;
    double sum = 0.0;
    int k = 0;
    for (; k + 8 <= nc; k += 8) {                                    // eight loads in flight, added in chunk order
      double v[8];
#pragma unroll
      for (int w = 0; w < 8; ++w) v[w] = p[(size_t)(k + w) * stride];
#pragma unroll
      for (int w = 0; w < 8; ++w) sum += v[w];
    }
    for (; k < nc; ++k) sum += p[(size_t)k * stride];
    double* o = out + (size_t)row * V + u;
    *o = accumulate ? *o + sum : sum;
    return;
  }
  // the scalars of joint j = t - JP_TILES + 1: thread p adds the samples p, p + 256, .. in order, then a tree over the 256 partial sums
  // whose shape is fixed -- a function of the batch alone
  __shared__ double s_part[3][JP_THREADS];
  const int j = t - JP_TILES;
  const bool has = cnt[j + 1] > 0;
  const double d2 = delta * delta;
  double s_rr = 0.0, s_rho = 0.0, s_abs = 0.0;
  if (has) {
    for (int s = el; s < batch; s += JP_THREADS) {
      const double rr = samples[(size_t)s * JP_SD + 3 * JP_NJ + j];
      s_rr += rr;
      s_rho += sqrt(rr + d2);
      s_abs += sqrt(rr);
    }
  }
  s_part[0][el] = s_rr;
  s_part[1][el] = s_rho;
  s_part[2][el] = s_abs;
  __syncthreads();
  for (int h = JP_THREADS / 2; h > 0; h >>= 1) {
    if (el < h) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s_part[k][el] += s_part[k][el + h];
    }
    __syncthreads();
  }
  if (el >= 4) return;
  const double v = el == 3 ? (has ? (double)batch : 0.0) : s_part[el][0];
  double* o = out + (size_t)JP_NJ * V + 4 * j + el;
  *o = accumulate ? *o + v : v;
}

}  // namespace jrr

using namespace jrr;

extern "C" size_t jrr_jfit_price_bytes(int batch, size_t* scratch_bytes) {
  if (scratch_bytes) *scratch_bytes = 0;
  if (batch < 1) return 0;
  int nc, rpc;
  jp_chunks(batch, nc, rpc);
  if (scratch_bytes) *scratch_bytes = JP_HEAD + (size_t)batch * JP_SD * 8 + (size_t)nc * JP_TILES * 256 * 8;
  return (size_t)JRR_JFIT_PRICE_DOUBLES * 8;
}

extern "C" int jrr_jfit_price(const float* verts, const float* gt_mm, int batch, const int32_t* vtx, const int32_t* counts, const double* x,
                              int mode, double delta_m, int accumulate, double* out, void* scratch, size_t scratch_bytes, void* stream) {
  const char* why = nullptr;
  if (!verts || !gt_mm || !vtx || !counts || !x || !out || !scratch) why = "verts, gt_mm, vtx, counts, x, out and scratch are required";
  if (!why && (((uintptr_t)verts | (uintptr_t)gt_mm) & 3) != 0) why = "verts and gt_mm must be 4-byte aligned";
  if (!why && (((uintptr_t)out | (uintptr_t)scratch) & 7) != 0) why = "out and scratch must be 8-byte aligned";
  if (!why && batch < 1) why = "batch must be 1 or more";
  if (!why && mode != JRR_JFIT_PRICE_MSE && mode != JRR_JFIT_PRICE_NORM) why = "mode must be JRR_JFIT_PRICE_MSE or JRR_JFIT_PRICE_NORM";
  if (!why && !(std::isfinite(delta_m) && delta_m >= 0.0)) why = "delta_m must be finite and not negative";
  if (!why && mode == JRR_JFIT_PRICE_NORM && !(delta_m > 0.0)) why = "delta_m must be positive in JRR_JFIT_PRICE_NORM mode";
  if (!why) {
    static thread_local unsigned char seen[V];                       // the row (+ 1) that listed the vertex last
    for (int u = 0; u < V; ++u) seen[u] = 0;
    int total = 0;
    for (int i = 0; i < NH && !why; ++i) {
      const int c = counts[i];
      if (c < 0 || c > JP_CAP) {
        why = "a count must lie in 0 .. 128";
        break;
      }
      total += c;
      for (int e = 0; e < c; ++e) {
        const int u = vtx[i * JP_CAP + e];
        if (u < 0 || u >= V) {
          why = "a listed vertex must lie in 0 .. 6889";
          break;
        }
        if (seen[u] == i + 1) {
          why = "a vertex is listed twice in its row";
          break;
        }
        seen[u] = (unsigned char)(i + 1);
      }
    }
    if (!why && total == 0) why = "no row has an entry";
  }
  if (why) {
    jrr_set_error("jrr_jfit_price: %s", why);
    return JRR_ERR_ARG;
  }
  int nc, rpc;
  jp_chunks(batch, nc, rpc);
  const size_t need = JP_HEAD + (size_t)batch * JP_SD * 8 + (size_t)nc * JP_TILES * 256 * 8;
  if (scratch_bytes < need) {
    jrr_set_error("jrr_jfit_price: the scratch needs the %zu bytes jrr_jfit_price_bytes gives for a batch of %d", need, batch);
    return JRR_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(scratch);
  // the lists and the weights, packed, in one copy; the wait behind it frees the packed copy (and the caller's arrays) before the
  // call returns, whatever the runtime does with pageable memory
  {
    static thread_local std::vector<char> head;
    head.assign(JP_HEAD, 0);
    for (int i = 0; i < NH; ++i) {
      memcpy(head.data() + JP_HEAD_VTX + (size_t)i * JP_CAP * 4, vtx + i * JP_CAP, (size_t)counts[i] * 4);
      memcpy(head.data() + JP_HEAD_X + (size_t)i * JP_CAP * 8, x + i * JP_CAP, (size_t)counts[i] * 8);
    }
    memcpy(head.data() + JP_HEAD_CNT, counts, (size_t)NH * 4);
    JRR_HIP(hipMemcpyAsync(base, head.data(), JP_HEAD, hipMemcpyHostToDevice, s));
    JRR_HIP(hipStreamSynchronize(s));
  }
  const int* d_vtx = reinterpret_cast<const int*>(base + JP_HEAD_VTX);
  const int* d_cnt = reinterpret_cast<const int*>(base + JP_HEAD_CNT);
  const double* d_x = reinterpret_cast<const double*>(base + JP_HEAD_X);
  double* d_samples = reinterpret_cast<double*>(base + JP_HEAD);
  double* d_slabs = d_samples + (size_t)batch * JP_SD;
  hipLaunchKernelGGL(k_jprice_resid, dim3((unsigned)((batch + JP_RS - 1) / JP_RS)), dim3(JP_THREADS), 0, s, verts, gt_mm, batch, d_vtx, d_cnt, d_x,
                     mode, delta_m, d_samples);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_jprice_partial, dim3((unsigned)((JP_TILES + JP_TPB - 1) / JP_TPB), (unsigned)nc), dim3(JP_THREADS), 0, s, verts,
                     reinterpret_cast<const double*>(d_samples), batch, rpc, d_slabs);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_jprice_finish, dim3((unsigned)(JP_TILES + JP_NJ)), dim3(JP_THREADS), 0, s, reinterpret_cast<const double*>(d_slabs),
                     reinterpret_cast<const double*>(d_samples), d_cnt, nc, batch, delta_m, accumulate ? 1 : 0, out);
  CHECK_LAUNCH();
  return JRR_OK;
}
