// The joint regressor's bookkeeping: its normalisation into the layouts the matrix kernels read (among them the JN block of the
// backward kernels' per-tile operand records, lbs_tile.h), the adjoint of that normalisation, and the J step over the regressor's
// support.  Nothing here touches a matrix core.
#include "jrr_common.h"
#include "kernels.h"
#include "lbs_tile.h"

namespace jrr {

// ------------------------------------------------------------------------------------------
// J_regressor normalisation (scripts/utils.py:87-92) into the tile layouts, and its adjoint
// ------------------------------------------------------------------------------------------
constexpr int JREG_THREADS = 1024;     // one block per regressor row: 6890 columns, 7 per thread
__global__ __launch_bounds__(JREG_THREADS) void k_jreg_rowsum(const float* __restrict__ J, const float* __restrict__ mask,
                                                               float* __restrict__ rowsum, int* __restrict__ sup_flag,
                                                               int32_t* __restrict__ step_inc) {
  __shared__ float red[JREG_THREADS];
  const int i = blockIdx.x;
  if (sup_flag && i == 0 && threadIdx.x == 0) *sup_flag = 1;      // k_jreg_support (two launches later) may clear it
  if (step_inc && i == 0 && threadIdx.x == 0) step_inc[0] += 1;   // the J step's Adam count (k_adam_flat, the launch before, used + 1)
  float acc = 0.f;
  for (int v = threadIdx.x; v < V; v += blockDim.x) {
    float x = J[(size_t)i * V + v];
    if (mask) x *= mask[(size_t)i * V + v];
    acc += fmaxf(x, 0.f);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = JREG_THREADS / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) rowsum[i] = red[0];
}

__global__ void k_jreg_tiles(const float* __restrict__ J, const float* __restrict__ mask,
                             const float* __restrict__ rowsum, float* __restrict__ Jn, float* __restrict__ Jn_vi,
                             float* __restrict__ Jn_iv, float* __restrict__ Jn_q, const int* __restrict__ p2v, int r16) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;   // over VT*32*32 (tile, vv, i)
  if (idx >= VT * 1024) return;
  const int vt = idx >> 10, vv = (idx >> 5) & 31, i = idx & 31;
  const int v = vt * 32 + vv;                  // row of the internal vertex order
  const int vo = (v < V) ? (p2v ? p2v[v] : v) : -1;   // the regressor column stored there
  float val = 0.f;
  if (i < NH && vo >= 0) {
    float x = J[(size_t)i * V + vo];
    if (mask) x *= mask[(size_t)i * V + vo];
    val = fmaxf(x, 0.f) / rowsum[i];
    Jn[(size_t)i * V + vo] = val;            // Jn keeps the regressor's own column order
  }
  Jn_vi[(size_t)vt * 1024 + vv * 32 + i] = val;
  Jn_q[((size_t)(v >> 2) * 32 + i) * 4 + (v & 3)] = val;      // vertex quads [VP/4][32][4]: A operand of k_gemm_q32
  // backward operand record: the role kernel's [i][32 v], or R16's JN [blk][s = i / 4][g = i % 4][m] (k_lbs_bwd16)
  if (r16) { if (i < 20) Jn_iv[(size_t)vt * TB_FLOATS + R16_JN + ((vv >> 4) * 5 + (i >> 2)) * 64 + (i & 3) * 16 + (vv & 15)] = val; }
  else if (i < NHP) Jn_iv[(size_t)vt * TB_FLOATS + TB_JN + i * 32 + vv] = val;
}

// ------------------------------------------------------------------------------------------
// J step over the regressor's SUPPORT (scripts/optimize.py:300-312).  dJ_raw = mask relu'(J mask) (dJn - <dJn, Jn>) / rowsum is
// exactly zero wherever J mask <= 0, and <dJn, Jn> only meets dJn where Jn > 0: the J step needs dJn -- a (17 x 6890) x B product
// over the 340 MB of stored vertices -- on the positive entries of J only (62 of 117 130 for the shipped checkpoint, and Adam
// never re-activates an entry: its gradient is zero while it is <= 0).  The same holds for the re-regression of the joints with
// the stepped regressor.  Both become gathers of a few vertex rows; rows with more than JSUP_CAP positive entries switch the
// whole step back to the dense products (flag = 0, decided on the device: no host synchronisation).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JREG_THREADS) void k_jreg_support(const float* __restrict__ Jn, const int* __restrict__ v2p, JSupport sup) {
  __shared__ int wcount[JREG_THREADS / 64];
  __shared__ int base;
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  for (int v0 = 0; v0 < V; v0 += JREG_THREADS) {            // ascending vertex order: deterministic lists
    const int v = v0 + threadIdx.x;
    const float w = (v < V) ? Jn[(size_t)i * V + v] : 0.f;
    const bool on = w > 0.f;
    const unsigned long long bal = __ballot(on);
    if (lane == 0) wcount[wave] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int q = 0; q < wave; ++q) off += wcount[q];
    off += __popcll(bal & ((1ull << lane) - 1ull));
    if (on && off < JSUP_CAP) { sup.col[i * JSUP_CAP + off] = v2p ? v2p[v] : v; sup.val[i * JSUP_CAP + off] = w; }
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int q = 0; q < JREG_THREADS / 64; ++q) t += wcount[q]; base += t; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    sup.cnt[i] = base < JSUP_CAP ? base : JSUP_CAP;
    if (base > JSUP_CAP) atomicMin(sup.flag, 0);            // (flag is set to 1 by k_jreg_rowsum, the launch before)
  }
}

// tmask[tile] = 1 for the 32-vertex tiles that hold a support entry: the J step's forward stores the vertices of those tiles only
__global__ __launch_bounds__(256) void k_jsup_tilemask(JSupport sup) {
  __shared__ int m[VT];
  for (int t = threadIdx.x; t < VT; t += 256) m[t] = 0;
  __syncthreads();
  for (int idx = threadIdx.x; idx < NH * JSUP_CAP; idx += 256) {
    const int i = idx / JSUP_CAP, e = idx % JSUP_CAP;
    if (e < sup.cnt[i]) m[sup.col[idx] >> 5] = 1;
  }
  __syncthreads();
  const bool known = sup.flag[JSUP_KNOWN] != 0;
  for (int t = threadIdx.x; t < VT; t += 256) {
    sup.tmask[t] = m[t];
    // the host has been told which tiles hold the support (and enqueues support-restricted work only): a J step can only shrink
    // it (ReLU' = 0 outside it) -- unless the caller changed J or the mask in place.  Loud, not silently wrong: sticky error word,
    // reported by the next jrr_j_support_info
    if (known && m[t] && !sup.tknown[t]) atomicOr(&sup.flag[JSUP_ERR], 1);
  }
  if (known && threadIdx.x == 0 && sup.flag[0] == 0) atomicOr(&sup.flag[JSUP_ERR], 2);
}
static int launch_jsup_tilemask(const JSupport& sup, hipStream_t s) {
  hipLaunchKernelGGL(k_jsup_tilemask, dim3(1), dim3(256), 0, s, sup);
  return 0;
}

// one workgroup per (row i, entry slot): dJn[i][row] = sum_b sum_r dj_r[i][b] verts_r[row][b]; fixed-order sums.
// (1024 threads: the sum over the poses is a chain of dependent load rounds -- 4 per thread at 4096 poses instead of 16: 17 -> ~6 us)
constexpr int JGS_THREADS = 1024;
__global__ __launch_bounds__(JGS_THREADS) void k_jgrad_sparse(JSupport sup, const float* __restrict__ dJT, const float* __restrict__ VTq,
                                                              float* __restrict__ dJn, int BP) {
  if (*sup.flag == 0) return;
  __shared__ float red[JGS_THREADS];
  const int i = blockIdx.x;
  for (int e = blockIdx.y; e < sup.cnt[i]; e += gridDim.y) {
    const int row = sup.col[i * JSUP_CAP + e];
    float acc = 0.f;
    for (int b = threadIdx.x; b < BP; b += JGS_THREADS) {          // padded poses carry dj = 0
#pragma unroll
      for (int r = 0; r < 3; ++r)
        acc = fmaf(dJT[(size_t)(r * NHP + i) * BP + b], VTq[(((size_t)r * (VP / 4) + (row >> 2)) * BP + b) * 4 + (row & 3)], acc);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = JGS_THREADS / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) dJn[(size_t)i * VP + row] = red[0];
    __syncthreads();
  }
}

// joints^T slab [3][32][BP] (rows i < 17) of the stored vertices with the current regressor: one thread per (pose, row i)
__global__ __launch_bounds__(256) void k_rejoints_sparse(JSupport sup, const float* __restrict__ VTq, float* __restrict__ out, int BP,
                                                         int32_t* __restrict__ step_inc) {
  if (step_inc && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) step_inc[0] += 1;      // before the early return
  if (*sup.flag == 0) return;
  const int b = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (b >= BP) return;
  float acc[3] = {0.f, 0.f, 0.f};
  const int n = sup.cnt[i];
  for (int e = 0; e < n; ++e) {
    const int row = sup.col[i * JSUP_CAP + e];
    const float w = sup.val[i * JSUP_CAP + e];
#pragma unroll
    for (int r = 0; r < 3; ++r) acc[r] = fmaf(w, VTq[(((size_t)r * (VP / 4) + (row >> 2)) * BP + b) * 4 + (row & 3)], acc[r]);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) out[(size_t)(r * 32 + i) * BP + b] = acc[r];
}

// The J step's gradient restricted to the regressor's support, for the data-parallel all-reduce: dJ (17 x 6890, file order of
// the columns) is exactly zero outside the support, so the ranks exchange [17][JSUP_CAP] floats instead of 468 520 bytes.
// The compact values come out of k_jreg_bwd (zeros behind the row's count); scatter: their way back into a zero-filled dJ.
__global__ __launch_bounds__(JSUP_CAP) void k_jsup_scatter(JSupport sup, const float* __restrict__ in, const int* __restrict__ p2v,
                                                           float* __restrict__ dJ) {
  const int i = blockIdx.x, e = threadIdx.x;
  if (e < sup.cnt[i]) { const int row = sup.col[i * JSUP_CAP + e]; dJ[(size_t)i * V + (p2v ? p2v[row] : row)] = in[i * JSUP_CAP + e]; }
}
int launch_jsup_scatter(const JSupport& sup, const float* in, const int* p2v, float* dJ, hipStream_t s) {
  hipLaunchKernelGGL(k_jsup_scatter, dim3(NH), dim3(JSUP_CAP), 0, s, sup, in, p2v, dJ);
  return 0;
}

int launch_jgrad_sparse(const JSupport& sup, const float* dJT, const float* VTq, float* dJn, int BP, hipStream_t s) {
  hipLaunchKernelGGL(k_jgrad_sparse, dim3(NH, 16), dim3(JGS_THREADS), 0, s, sup, dJT, VTq, dJn, BP);
  return 0;
}
int launch_rejoints_sparse(const JSupport& sup, const float* VTq, float* out, int BP, hipStream_t s, int32_t* step_inc) {
  hipLaunchKernelGGL(k_rejoints_sparse, dim3((BP + 255) / 256, NH), dim3(256), 0, s, sup, VTq, out, BP, step_inc);   // BP is a multiple of 128 only: round UP (the kernel guards b >= BP)
  return 0;
}

// dJ_raw = mask * relu'(J*mask) * (dJn - sum_v(dJn*Jn)) / rowsum      (dJn given as [17][ldn])
__global__ __launch_bounds__(JREG_THREADS) void k_jreg_bwd(const float* __restrict__ J, const float* __restrict__ mask,
                                                            const float* __restrict__ Jn, const float* __restrict__ rowsum,
                                                            const float* __restrict__ dJn, int ldn, float* __restrict__ dJ,
                                                            const int* __restrict__ v2p, JSupport sup, const int* __restrict__ p2v,
                                                            float* __restrict__ dJs) {
  __shared__ float red[JREG_THREADS];
  const int i = blockIdx.x;
  float acc = 0.f;
  // dJn comes in the internal vertex order (row v2p[v] holds column v; NULL = identity)
  for (int v = threadIdx.x; v < V; v += blockDim.x) acc += dJn[(size_t)i * ldn + (v2p ? v2p[v] : v)] * Jn[(size_t)i * V + v];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = JREG_THREADS / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const float dot = red[0], rs = rowsum[i];
  for (int v = threadIdx.x; v < V; v += blockDim.x) {
    float mk = mask ? mask[(size_t)i * V + v] : 1.f;
    float x = J[(size_t)i * V + v] * mk;
    float g = (x > 0.f) ? (dJn[(size_t)i * ldn + (v2p ? v2p[v] : v)] - dot) / rs * mk : 0.f;
    dJ[(size_t)i * V + v] = g;
  }
  // dJs (nullable): the same gradient on the regressor's support, [17][JSUP_CAP] with zeros behind the row's count -- the payload of
  // the data-parallel all-reduce (jrr_j_regressor_grad_support).  Entry e of the list is internal row col[e]; its vertex is p2v[col[e]].
  if (dJs) {
    const int n = sup.cnt[i];
    for (int e = threadIdx.x; e < JSUP_CAP; e += blockDim.x) {
      float g = 0.f;
      if (e < n) {
        const int row = sup.col[i * JSUP_CAP + e];
        const int vo = p2v ? p2v[row] : row;
        const float mk = mask ? mask[(size_t)i * V + vo] : 1.f;
        const float x = J[(size_t)i * V + vo] * mk;
        g = (x > 0.f) ? (dJn[(size_t)i * ldn + row] - dot) / rs * mk : 0.f;
      }
      dJs[i * JSUP_CAP + e] = g;
    }
  }
}

// ------------------------------------------------------------------------------------------
// The second half of the J step in ONE launch (scripts/optimize.py:312 `J_Regressor_optimizer.step()` + the re-normalisation of the
// next find_joints, scripts/utils.py:87-92): one workgroup per regressor row does what used to be five launches -- torch's Adam on
// the row (k_adam_flat), the engine's copy of the raw parameter, the row sum, the normalised row in all layouts (k_jreg_tiles) and the
// row's support list (k_jreg_support) -- with the arithmetic and the summation orders of those kernels (bit-identical results).  The
// gradient arrives dense (dJ) or on the OLD support lists (dJs, the all-reduced payload of jrr_j_step_apply_support: scattered through
// LDS, zero elsewhere -- what the dense gradient holds there).  The workgroup that finishes LAST increments the step counter (every
// workgroup read it at its start) and publishes the fits-the-lists flag.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JREG_THREADS) void k_jstep_update(JStepUpdate a) {
  __shared__ float red[JREG_THREADS];
  __shared__ float gl[V];
  __shared__ AdamScalars sc;
  __shared__ int wcount[JREG_THREADS / 64];
  __shared__ int base, islast;
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { sc = adam_scalars(a.step[0] + 1, a.lr, 0.9f, 0.999f, 1e-8f); base = 0; }
  if (a.dJs) {
    for (int v = tid; v < V; v += JREG_THREADS) gl[v] = 0.f;
    __syncthreads();
    if (tid < a.sup.cnt[i]) { const int row = a.sup.col[i * JSUP_CAP + tid]; gl[a.p2v ? a.p2v[row] : row] = a.dJs[i * JSUP_CAP + tid]; }
  }
  __syncthreads();
  const AdamScalars s = sc;
  constexpr int NK = (V + JREG_THREADS - 1) / JREG_THREADS;      // 7 columns per thread
  float x[NK];
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int v = tid + k * JREG_THREADS;
    x[k] = 0.f;
    if (v < V) {
      const size_t o = (size_t)i * V + v;
      const float g = a.dJs ? gl[v] : a.dJ[o];
      float mm = a.m[o], vv = a.v[o];
      const float pn = adam_update(a.J[o], g, mm, vv, s);
      a.J[o] = pn; a.m[o] = mm; a.v[o] = vv;
      a.Jraw[o] = pn;
      float mk = 1.f;
      if (a.mask) { mk = a.mask[o]; a.Jmask[o] = mk; }
      x[k] = fmaxf(pn * mk, 0.f);
      acc += x[k];
    }
  }
  red[tid] = acc;
  __syncthreads();
  for (int w = JREG_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  const float rs = red[0];
  if (tid == 0) a.rowsum[i] = rs;
  // the normalised row in every layout (k_jreg_tiles), then its support list in ascending FILE order of the vertices (k_jreg_support)
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int v = tid + k * JREG_THREADS;
    const float val = (v < V) ? x[k] / rs : 0.f;
    int r = 0;
    if (v < V) {
      r = a.v2p ? a.v2p[v] : v;                      // internal row of the vertex
      const int vt = r >> 5, vv = r & 31;
      a.Jn[(size_t)i * V + v] = val;
      a.Jn_vi[(size_t)vt * 1024 + vv * 32 + i] = val;
      a.Jn_q[((size_t)(r >> 2) * 32 + i) * 4 + (r & 3)] = val;
      if (a.r16) a.Jn_iv[(size_t)vt * TB_FLOATS + R16_JN + ((vv >> 4) * 5 + (i >> 2)) * 64 + (i & 3) * 16 + (vv & 15)] = val;
      else a.Jn_iv[(size_t)vt * TB_FLOATS + TB_JN + i * 32 + vv] = val;
    }
    const bool on = val > 0.f;
    const unsigned long long bal = __ballot(on);
    if (lane == 0) wcount[wave] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int q = 0; q < wave; ++q) off += wcount[q];
    off += __popcll(bal & ((1ull << lane) - 1ull));
    if (on && off < JSUP_CAP) { a.sup.col[i * JSUP_CAP + off] = r; a.sup.val[i * JSUP_CAP + off] = val; }
    __syncthreads();
    if (tid == 0) { int t = 0; for (int q = 0; q < JREG_THREADS / 64; ++q) t += wcount[q]; base += t; }
    __syncthreads();
  }
  if (tid == 0) {
    a.sup.cnt[i] = base < JSUP_CAP ? base : JSUP_CAP;
    if (base > JSUP_CAP) atomicAdd(&a.sync[1], 1);
    __threadfence();
    islast = atomicAdd(&a.sync[0], 1) == (int)gridDim.x - 1;
    if (islast) {
      __threadfence();
      *a.sup.flag = atomicAdd(&a.sync[1], 0) == 0 ? 1 : 0;
      a.step[0] += 1;
      a.sync[0] = 0; a.sync[1] = 0;
    }
  }
}
int launch_jstep_update(const JStepUpdate& a, hipStream_t s) {
  hipLaunchKernelGGL(k_jstep_update, dim3(NH), dim3(JREG_THREADS), 0, s, a);
  launch_jsup_tilemask(a.sup, s);
  return 0;
}

int launch_jreg_normalize(const float* J, const float* mask, float* rowsum, float* Jn, float* Jn_vi, float* Jn_iv,
                          float* Jn_q, const int* p2v, hipStream_t s, int r16, const int* v2p, const JSupport* sup, int32_t* step_inc) {
  hipLaunchKernelGGL(k_jreg_rowsum, dim3(NH), dim3(JREG_THREADS), 0, s, J, mask, rowsum, sup ? sup->flag : nullptr, step_inc);
  hipLaunchKernelGGL(k_jreg_tiles, dim3(VT * 1024 / 256), dim3(256), 0, s, J, mask, rowsum, Jn, Jn_vi, Jn_iv, Jn_q, p2v, r16);
  if (sup) {
    hipLaunchKernelGGL(k_jreg_support, dim3(NH), dim3(JREG_THREADS), 0, s, Jn, v2p, *sup);
    launch_jsup_tilemask(*sup, s);
  }
  return 0;
}

int launch_jreg_bwd(const float* J, const float* mask, const float* Jn, const float* rowsum, const float* dJn, int ldn,
                    float* dJ, const int* v2p, hipStream_t s, const JSupport* sup, const int* p2v, float* dJs) {
  const JSupport none{nullptr, nullptr, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(k_jreg_bwd, dim3(NH), dim3(JREG_THREADS), 0, s, J, mask, Jn, rowsum, dJn, ldn, dJ, v2p, sup ? *sup : none, p2v,
                     sup ? dJs : nullptr);
  return 0;
}

}  // namespace jrr
