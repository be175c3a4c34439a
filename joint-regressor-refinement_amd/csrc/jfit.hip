// The regressor fit (`--fit_regressor`): Adam steps of the J_regressor on a table of fixed meshes (scripts/optimize.py:300-312 with the
// SMPL forward taken out of the loop).  No engine, no body model; include/jrr.h (jrr_jfit_*) is the specification.
//
// State and cache: jfitk.h.
//
// k_jfit_prepare  one workgroup: the union by an LDS flag per vertex and a scan, the rows' lists by ballots in ascending vertex order.
// k_jfit_set_entries  one workgroup: the raw values of the listed entries from a dense array, Adam's moments and step counter to zero.
// k_jfit_gather   one workgroup per sample: the NS vertices and the ground truth into the sample's cache row.
// k_jfit_joints   one thread per (sample, joint): the forward half alone, sums in double.
// k_jfit_step     ONE launch per Adam step.  A workgroup owns chunks of JF_SPW = 32 consecutive samples of the minibatch (chunk w,
//   w + grid, ...).  A chunk is staged in LDS in runs of whole cache rows (contiguous in memory: coalesced 4-byte loads; all 32 rows
//   at once for the shipped support, fewer per pass for a wide one) and worked on from there:
//     forward    one thread per (sample, joint): joints = sum over the row's list of Jn * vertex, in double, rounded once;
//                (a row WITHOUT entries has no parameters: its joint is left out of the loss and of the adjoint)
//     adjoint    one thread per (sample, joint, axis): d = (j - j0) - gt / 1000, loss += d^2, a = d * 2 / (count * 51);
//                then joint 0 takes a0 - sum of all a;
//     gradient   one thread per listed ENTRY (replicated 4 or 2 times over interleaved samples when there are at most 64 / 128 of them):
//                dJn[entry] += a[sample][row] . vertex[sample][entry], in double, over the samples in order.
//   The workgroup leaves its sums as a slab of doubles and its loss; the workgroup that arrives LAST (integer atomic on a counter, the
//   __threadfence pattern of k_jstep_update) adds the slabs in workgroup order, rounds once, applies the adjoint of the normalisation
//   (k_jreg_bwd's formula) and torch's Adam (adam_scalars / adam_update) to every listed entry, and publishes the new raw values,
//   moments, normalised weights, the step counter and the loss.  No floating-point atomics: a result is a function of the inputs
//   and the minibatch size alone.
#include "jfitk.h"

namespace jrr {

constexpr int JF_STAGE = 7680;                        // floats of staged cache rows: 32 rows of the shipped support (237 floats each)
constexpr int JF_K = (JF_CAP + JF_THREADS - 1) / JF_THREADS;   // 9 entries per thread at most
constexpr int JF_PREP_THREADS = 1024;

static_assert(JF_STAGE >= 3 * JF_CAP + JF_GT + 1, "one cache row of the widest support must fit the staging area");
static_assert(JF_STAGE >= JF_CAP, "the last workgroup keeps dJn in the staging area");

// ---- prepare ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JF_PREP_THREADS) void k_jfit_prepare(const float* __restrict__ J, const float* __restrict__ mask, void* state) {
  __shared__ int s_rank[V];                           // 1 where some row is positive, then the vertex's position in the union
  __shared__ int s_part[JF_PREP_THREADS];
  __shared__ int s_cnt[NH], s_off[NH + 1];
  __shared__ int s_bad;
  const JfState st = jf_carve(state);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int v = tid; v < V; v += JF_PREP_THREADS) s_rank[v] = 0;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  // the rows' counts (a wave per row, ballots) and the union's flags
  for (int i = wave; i < NH; i += JF_PREP_THREADS / 64) {
    int n = 0;
    for (int v0 = 0; v0 < V; v0 += 64) {
      const int v = v0 + lane;
      bool on = false;
      if (v < V) {
        const size_t o = (size_t)i * V + v;
        on = J[o] * (mask ? mask[o] : 1.f) > 0.f;
        if (on) s_rank[v] = 1;                        // every writer stores the same value
      }
      n += __popcll(__ballot(on));
    }
    if (lane == 0) { s_cnt[i] = n; if (n > JSUP_CAP) s_bad = 1; }
  }
  __syncthreads();
  // exclusive scan of the flags: contiguous segments of 7 vertices per thread, the 1024 partial sums serially by thread 0
  constexpr int SEG = (V + JF_PREP_THREADS - 1) / JF_PREP_THREADS;
  int local = 0;
  for (int k = 0; k < SEG; ++k) { const int v = tid * SEG + k; if (v < V) local += s_rank[v]; }
  s_part[tid] = local;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < JF_PREP_THREADS; ++t) { const int x = s_part[t]; s_part[t] = run; run += x; }
    int o = 0;
    for (int i = 0; i < NH; ++i) { s_off[i] = o; o += min(s_cnt[i], JSUP_CAP); }
    s_off[NH] = o;
    const bool bad = s_bad != 0 || o == 0;
    st.head[JF_H_NS] = bad ? 0 : run;
    st.head[JF_H_E] = bad ? 0 : o;
    st.head[JF_H_STEP] = 0;
    st.head[JF_H_ERR] = s_bad ? 1 : 0;
    st.head[JF_H_ARRIVE] = 0;
    for (int i = 0; i < NH; ++i) { st.head[JF_H_CNT + i] = s_cnt[i]; st.head[JF_H_OFF + i] = s_off[i]; }
    st.head[JF_H_OFF + NH] = o;
  }
  __syncthreads();
  {
    int run = s_part[tid];
    for (int k = 0; k < SEG; ++k) {
      const int v = tid * SEG + k;
      if (v < V) {
        const int f = s_rank[v];
        s_rank[v] = run;
        if (f && run < JF_CAP) st.cols[run] = v;
        run += f;
      }
    }
  }
  __syncthreads();
  if (s_bad) return;                                  // uniform
  // the lists: row i's entries in ascending vertex order at off[i] ..
  for (int i = wave; i < NH; i += JF_PREP_THREADS / 64) {
    int base = s_off[i];
    double sum = 0.0;
    for (int v0 = 0; v0 < V; v0 += 64) {
      const int v = v0 + lane;
      bool on = false;
      float raw = 0.f, mk = 1.f;
      if (v < V) {
        const size_t o = (size_t)i * V + v;
        raw = J[o];
        mk = mask ? mask[o] : 1.f;
        on = raw * mk > 0.f;
      }
      const unsigned long long bal = __ballot(on);
      if (on) {
        const int idx = base + __popcll(bal & ((1ull << lane) - 1ull));
        st.pk[idx] = s_rank[v] | (i << 16);
        st.vtx[idx] = v;
        st.raw[idx] = raw;
        st.mk[idx] = mk;
        st.m[idx] = 0.f;
        st.v[idx] = 0.f;
        sum += (double)(raw * mk);
      }
      base += __popcll(bal);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float rs = (float)sum;
    if (lane == 0) reinterpret_cast<float*>(st.head)[JF_H_RS + i] = rs;
  }
}
// the normalised weights of a freshly prepared state (a launch of its own: it reads what other lanes of k_jfit_prepare stored)
__global__ __launch_bounds__(JF_THREADS) void k_jfit_normalise(void* state) {
  const JfState st = jf_carve(state);
  const int E = st.head[JF_H_E];
  const float* rs = reinterpret_cast<const float*>(st.head) + JF_H_RS;
  for (int idx = blockIdx.x * JF_THREADS + threadIdx.x; idx < E; idx += gridDim.x * JF_THREADS) {
    const int i = st.pk[idx] >> 16;
    st.jn[idx] = fmaxf(st.raw[idx] * st.mk[idx], 0.f) / rs[i];
  }
}

// ---- set_entries ------------------------------------------------------------------------------------------------------------------
// one workgroup, a wave per row, two entries per lane: the raw value of every listed entry from the dense array (zeros allowed), Adam's
// m = v = 0 and step 0, the rows' sums and the normalised weights as k_jfit_step's last workgroup leaves them
__global__ __launch_bounds__(JF_THREADS) void k_jfit_set_entries(void* state, const float* __restrict__ J) {
  __shared__ int s_bad;
  const JfState st = jf_carve(state);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = st.head[JF_H_E];
  if (E < 1 || E > JF_CAP) return;                    // not a prepared state: jrr_jfit_info reports it
  if (tid == 0) s_bad = 0;
  __syncthreads();
  float* rowsum = reinterpret_cast<float*>(st.head) + JF_H_RS;
  for (int i = wave; i < NH; i += JF_THREADS / 64) {
    const int b = min(max(st.head[JF_H_OFF + i], 0), E), n = min(min(st.head[JF_H_OFF + i + 1], E) - b, JSUP_CAP);
    if (n <= 0) continue;
    float xn[2] = {0.f, 0.f};
    double sum = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = lane + 64 * h;
      if (e < n) {
        const int idx = b + e;
        const float raw = J[(size_t)i * V + min((unsigned)st.vtx[idx], (unsigned)(V - 1))];
        st.raw[idx] = raw; st.m[idx] = 0.f; st.v[idx] = 0.f;
        xn[h] = fmaxf(raw * st.mk[idx], 0.f);
        sum += (double)xn[h];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float rs = (float)sum;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = lane + 64 * h;
      if (e < n) st.jn[b + e] = xn[h] / rs;           // (a row that sums to zero: NaN, the reference's 0/0, and the error word)
    }
    if (lane == 0) {
      rowsum[i] = rs;
      if (!(rs > 0.f)) s_bad = 1;                     // every writer stores the same value
    }
  }
  __syncthreads();
  if (tid == 0) {
    st.head[JF_H_STEP] = 0;
    st.head[JF_H_ARRIVE] = 0;
    st.head[JF_H_ERR] = (st.head[JF_H_ERR] & ~JF_ERR_ROWSUM) | (s_bad ? JF_ERR_ROWSUM : 0);
  }
}

// ---- gather -----------------------------------------------------------------------------------------------------------------------
// grid: one workgroup per sample
__global__ __launch_bounds__(JF_THREADS) void k_jfit_gather(void* state, const float* __restrict__ verts, const float* __restrict__ gt_mm,
                                                            float* __restrict__ cache, long long row0, int ns) {
  const JfState st = jf_carve(state);
  if (st.head[JF_H_NS] != ns) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&st.head[JF_H_ERR], 2);
    return;
  }
  const int b = blockIdx.x, RL = jf_row_floats(ns);
  const float* pv = verts + (size_t)b * V * 3;
  float* out = cache + (size_t)(row0 + b) * RL;
  for (int r = threadIdx.x; r < RL; r += JF_THREADS) {
    float x = 0.f;
    if (r < 3 * ns) {
      const int k = r / 3, c = r - k * 3;
      x = pv[min((unsigned)st.cols[k], (unsigned)(V - 1)) * 3 + c];
    } else if (r < 3 * ns + JF_GT) {
      x = gt_mm[(size_t)b * JF_GT + (r - 3 * ns)];
    }
    out[r] = x;
  }
}

// ---- joints -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JF_THREADS) void k_jfit_joints(void* state, const float* __restrict__ cache, long long begin, int count,
                                                            int ns, float* __restrict__ joints) {
  const JfState st = jf_carve(state);
  const float nanv = __int_as_float(0x7fc00000);
  const int item = blockIdx.x * JF_THREADS + threadIdx.x;
  if (item >= count * NH) return;
  const int s = item / NH, i = item - s * NH;
  float* o = joints + (size_t)item * 3;
  if (st.head[JF_H_NS] != ns) {
    if (item == 0) atomicOr(&st.head[JF_H_ERR], 2);
    o[0] = nanv; o[1] = nanv; o[2] = nanv;
    return;
  }
  const int E = min(st.head[JF_H_E], JF_CAP);
  const int b = min(max(st.head[JF_H_OFF + i], 0), E), e = min(st.head[JF_H_OFF + i + 1], E);
  const float* row = cache + (size_t)(begin + s) * jf_row_floats(ns);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int idx = b; idx < e; ++idx) {
    const double w = (double)st.jn[idx];
    const int p = min(st.pk[idx] & 0xffff, ns - 1) * 3;
    a0 += w * (double)row[p];
    a1 += w * (double)row[p + 1];
    a2 += w * (double)row[p + 2];
  }
  o[0] = e > b ? (float)a0 : nanv;
  o[1] = e > b ? (float)a1 : nanv;
  o[2] = e > b ? (float)a2 : nanv;
}

// ---- one Adam step ----------------------------------------------------------------------------------------------------------------
// grid: min(ceil(count / 32), JF_MAX_WG) workgroups of 256 threads; rows [row0, row0 + count) of the cache are the minibatch
__global__ __launch_bounds__(JF_THREADS) void k_jfit_step(void* state, const float* __restrict__ cache, long long row0, int count, int ns,
                                                          float lr, float* __restrict__ loss_out, float* __restrict__ grad_out) {
  __shared__ float s_stage[JF_STAGE];                 // 30 720 B: staged cache rows; dJn of the last workgroup
  __shared__ float s_jn[JF_CAP];                      //  8 704 B
  __shared__ int s_pk[JF_CAP];                        //  8 704 B
  __shared__ float s_j[JF_SPW * JF_GT];               //  6 528 B: joints of the staged samples
  __shared__ float s_a[JF_SPW * JF_GT];               //  6 528 B: their adjoints
  __shared__ double s_red[JF_THREADS];                //  2 048 B
  __shared__ int s_off[NH + 1];
  __shared__ AdamScalars s_sc;
  __shared__ int s_last;
  const JfState st = jf_carve(state);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float nanv = __int_as_float(0x7fc00000);
  const int E = st.head[JF_H_E];
  if (st.head[JF_H_NS] != ns || E < 1 || E > JF_CAP) {          // uniform over the launch: nobody touches the counter
    if (blockIdx.x == 0 && tid == 0) { atomicOr(&st.head[JF_H_ERR], 2); loss_out[0] = nanv; }
    return;
  }
  for (int idx = tid; idx < E; idx += JF_THREADS) { s_jn[idx] = st.jn[idx]; s_pk[idx] = st.pk[idx]; }
  if (tid <= NH) s_off[tid] = min(max(st.head[JF_H_OFF + tid], 0), E);
  const int RL = jf_row_floats(ns);
  const int sub = min(JF_SPW, JF_STAGE / RL);         // >= 1 (static_assert above)
  // the gradient phase: `nrep` replicas of the entry list, replica r takes the staged samples r, r + nrep, ...
  const int span = E <= 64 ? 64 : (E <= 128 ? 128 : JF_THREADS);
  const int nrep = JF_THREADS / span, rep = tid / span, lidx = tid & (span - 1);
  const float scale = 2.f / (float)((double)count * JF_GT);
  double acc[JF_K];
#pragma unroll
  for (int k = 0; k < JF_K; ++k) acc[k] = 0.0;
  double lsum = 0.0;
  __syncthreads();

  for (int c0 = (int)blockIdx.x * JF_SPW; c0 < count; c0 += (int)gridDim.x * JF_SPW) {
    const int cn = min(JF_SPW, count - c0);
    for (int s0 = 0; s0 < cn; s0 += sub) {
      const int sn = min(sub, cn - s0);
      const float* src = cache + (size_t)(row0 + c0 + s0) * RL;
      for (int x = tid; x < sn * RL; x += JF_THREADS) s_stage[x] = src[x];
      __syncthreads();
      // forward
      for (int item = tid; item < sn * NH; item += JF_THREADS) {
        const int s = item / NH, i = item - s * NH;
        const int b = s_off[i], e = s_off[i + 1];
        const float* vs = s_stage + s * RL;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int idx = b; idx < e; ++idx) {
          const double w = (double)s_jn[idx];
          const int p = (s_pk[idx] & 0xffff) * 3;
          a0 += w * (double)vs[p];
          a1 += w * (double)vs[p + 1];
          a2 += w * (double)vs[p + 2];
        }
        float* o = s_j + s * JF_GT + i * 3;      // (a row without entries: zeros; it is left out below)
        o[0] = (float)a0;
        o[1] = (float)a1;
        o[2] = (float)a2;
      }
      __syncthreads();
      // centring, loss, adjoint of the loss; a row without entries has no parameters: its joint is left out of both
      for (int item = tid; item < sn * JF_GT; item += JF_THREADS) {
        const int s = item / JF_GT, r = item - s * JF_GT, i = r / 3, c = r - i * 3;
        const bool empty = s_off[i + 1] == s_off[i];
        const float d = empty ? 0.f : (s_j[item] - s_j[s * JF_GT + c]) - s_stage[s * RL + 3 * ns + r] / 1000.f;
        lsum += (double)d * (double)d;
        s_a[item] = d * scale;
      }
      __syncthreads();
      // adjoint of the centring: joint 0 receives minus the sum of all joint adjoints
      for (int item = tid; item < sn * 3; item += JF_THREADS) {
        const int s = item / 3, c = item - s * 3;
        float t = 0.f;
        for (int i = 0; i < NH; ++i) t += s_a[s * JF_GT + i * 3 + c];
        s_a[s * JF_GT + c] -= t;
      }
      __syncthreads();
      // gradient with respect to the normalised entries
#pragma unroll
      for (int k = 0; k < JF_K; ++k) {
        const int idx = lidx + k * JF_THREADS;
        if (idx < E) {
          const int pk = s_pk[idx];
          const float* vs = s_stage + (pk & 0xffff) * 3;
          const float* as = s_a + (pk >> 16) * 3;
          double t = acc[k];
          for (int s = rep; s < sn; s += nrep) {
            const float* v3 = vs + s * RL;
            const float* a3 = as + s * JF_GT;
            t += (double)a3[0] * (double)v3[0];
            t += (double)a3[1] * (double)v3[1];
            t += (double)a3[2] * (double)v3[2];
          }
          acc[k] = t;
        }
      }
      __syncthreads();
    }
  }

  // the workgroup's slab (replicas added in order) and its loss
  double* slab = st.slab + (size_t)blockIdx.x * JF_CAP;
  if (nrep > 1) {
    s_red[tid] = acc[0];
    __syncthreads();
    if (rep == 0 && lidx < E) {
      double t = s_red[lidx];
      for (int r = 1; r < nrep; ++r) t += s_red[r * span + lidx];
      slab[lidx] = t;
    }
    __syncthreads();
  } else {
#pragma unroll
    for (int k = 0; k < JF_K; ++k) {
      const int idx = tid + k * JF_THREADS;
      if (idx < E) slab[idx] = acc[k];
    }
  }
  s_red[tid] = lsum;
  __syncthreads();
  for (int w = JF_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) s_red[tid] += s_red[tid + w];
    __syncthreads();
  }
  if (tid == 0) st.lpart[blockIdx.x] = s_red[0];
  __threadfence();
  __syncthreads();
  if (tid == 0) s_last = atomicAdd(&st.head[JF_H_ARRIVE], 1) == (int)gridDim.x - 1;
  __syncthreads();
  if (!s_last) return;
  __threadfence();

  // ---- the last workgroup: slabs in workgroup order, the adjoint of the normalisation, Adam, the new weights ----
  float* s_g = s_stage;
  const int nwg = (int)gridDim.x;
#pragma unroll 1
  for (int idx = tid; idx < E; idx += JF_THREADS) {
    double t = 0.0;
    for (int w = 0; w < nwg; ++w) t += st.slab[(size_t)w * JF_CAP + idx];
    s_g[idx] = (float)t;
  }
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < nwg; ++w) t += st.lpart[w];
    loss_out[0] = (float)(t / ((double)count * JF_GT));
    s_sc = adam_scalars(st.head[JF_H_STEP] + 1, lr, 0.9f, 0.999f, 1e-8f);
  }
  if (grad_out)
    for (int slot = tid; slot < JF_CAP; slot += JF_THREADS) grad_out[slot] = 0.f;
  __syncthreads();
  const AdamScalars sc = s_sc;
  float* rowsum = reinterpret_cast<float*>(st.head) + JF_H_RS;
  for (int i = wave; i < NH; i += JF_THREADS / 64) {            // a wave per row, two entries per lane
    const int b = s_off[i], n = min(s_off[i + 1] - b, JSUP_CAP);
    if (n <= 0) continue;
    double dd = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = lane + 64 * h;
      if (e < n) dd += (double)s_g[b + e] * (double)s_jn[b + e];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dd += __shfl_xor(dd, o);
    const float dot = (float)dd, rs = rowsum[i];
    float xn[2] = {0.f, 0.f};
    double sum = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = lane + 64 * h;
      if (e < n) {
        const int idx = b + e;
        const float mk = st.mk[idx], raw = st.raw[idx];
        const float g = (raw * mk > 0.f) ? (s_g[idx] - dot) / rs * mk : 0.f;
        float mm = st.m[idx], vv = st.v[idx];
        const float pn = adam_update(raw, g, mm, vv, sc);
        st.raw[idx] = pn; st.m[idx] = mm; st.v[idx] = vv;
        if (grad_out) grad_out[i * JSUP_CAP + e] = g;
        xn[h] = fmaxf(pn * mk, 0.f);
        sum += (double)xn[h];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float rsn = (float)sum;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = lane + 64 * h;
      if (e < n) st.jn[b + e] = xn[h] / rsn;
    }
    if (lane == 0) rowsum[i] = rsn;
  }
  if (tid == 0) { st.head[JF_H_STEP] += 1; st.head[JF_H_ARRIVE] = 0; }
}

// ---- scatter ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JF_THREADS) void k_jfit_scatter(const void* state, float* __restrict__ J, float* __restrict__ m, float* __restrict__ v) {
  const JfState st = jf_carve(const_cast<void*>(state));
  const int E = min(st.head[JF_H_E], JF_CAP);
  for (int idx = blockIdx.x * JF_THREADS + threadIdx.x; idx < E; idx += gridDim.x * JF_THREADS) {
    const int i = st.pk[idx] >> 16;
    const unsigned col = (unsigned)st.vtx[idx];
    if (i < 0 || i >= NH || col >= (unsigned)V) continue;
    const size_t o = (size_t)i * V + col;
    if (J) J[o] = st.raw[idx];
    if (m) m[o] = st.m[idx];
    if (v) v[o] = st.v[idx];
  }
}

}  // namespace jrr

using namespace jrr;

static int jf_read_info(const void* state, int32_t* info_host, hipStream_t s, int* err_word) {
  int32_t head[JF_H_CNT + NH];
  JRR_HIP(hipMemcpyAsync(head, state, sizeof(head), hipMemcpyDeviceToHost, s));
  JRR_HIP(hipStreamSynchronize(s));
  if (info_host) {
    for (int i = 0; i < JRR_JFIT_INFO; ++i) info_host[i] = 0;
    info_host[0] = head[JF_H_NS];
    info_host[1] = head[JF_H_E];
    info_host[2] = head[JF_H_STEP];
    for (int i = 0; i < NH; ++i) info_host[4 + i] = head[JF_H_CNT + i];
  }
  *err_word = head[JF_H_ERR];
  if (head[JF_H_NS] < 1 || head[JF_H_NS] > JF_CAP || head[JF_H_E] < 1 || head[JF_H_E] > JF_CAP) *err_word |= 4;
  return JRR_OK;
}

extern "C" size_t jrr_jfit_state_bytes(void) { return jf_state_bytes(); }
extern "C" size_t jrr_jfit_cache_bytes(int64_t n_rows, int ns) {
  if (n_rows < 0 || n_rows > INT32_MAX || ns < 1 || ns > JF_CAP) return 0;
  return (size_t)n_rows * jf_row_floats(ns) * 4;
}
extern "C" int jrr_jfit_prepare(const float* J_init, const float* mask, void* state, size_t state_bytes, int32_t* info_host, void* stream) {
  if (!J_init || !state || ((uintptr_t)state & 15) != 0 || (((uintptr_t)J_init | (uintptr_t)mask) & 3) != 0) {
    jrr_set_error("jrr_jfit_prepare: bad argument (J_init and state are required, state 16-byte aligned)");
    return JRR_ERR_ARG;
  }
  if (state_bytes < jf_state_bytes()) {
    jrr_set_error("jrr_jfit_prepare: the state needs jrr_jfit_state_bytes() = %zu bytes", jf_state_bytes());
    return JRR_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_jfit_prepare, dim3(1), dim3(JF_PREP_THREADS), 0, s, J_init, mask, state);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_jfit_normalise, dim3((JF_CAP + JF_THREADS - 1) / JF_THREADS), dim3(JF_THREADS), 0, s, state);
  CHECK_LAUNCH();
  int err = 0;
  const int rc = jf_read_info(state, info_host, s, &err);
  if (rc != JRR_OK) return rc;
  if (err & 1) {
    jrr_set_error("jrr_jfit_prepare: a row of J_init * mask has more than %d positive entries", (int)JSUP_CAP);
    return JRR_ERR_ARG;
  }
  if (err) {
    jrr_set_error("jrr_jfit_prepare: J_init * mask has no positive entry");
    return JRR_ERR_ARG;
  }
  return JRR_OK;
}
extern "C" int jrr_jfit_info(const void* state, int32_t* info_host, void* stream) {
  if (!state || !info_host || ((uintptr_t)state & 15) != 0) {
    jrr_set_error("jrr_jfit_info: bad argument");
    return JRR_ERR_ARG;
  }
  int err = 0;
  const int rc = jf_read_info(state, info_host, (hipStream_t)stream, &err);
  if (rc != JRR_OK) return rc;
  if (err) {
    jrr_set_error(err & JF_ERR_NS       ? "jrr_jfit_info: a call passed an ns that is not the prepared one"
                  : err & JF_ERR_ROWSUM ? "jrr_jfit_info: jrr_jfit_set_entries left a listed row without a positive entry"
                                        : "jrr_jfit_info: the state is not a prepared one");
    return JRR_ERR_ARG;
  }
  return JRR_OK;
}

extern "C" int jrr_jfit_gather(void* state, const float* verts, const float* gt_mm, int batch, void* cache, int64_t n_rows, int64_t row0,
                               int ns, void* stream) {
  const char* why = jf_check_cache(state, cache, n_rows, ns);
  if (!why && (!verts || !gt_mm || (((uintptr_t)verts | (uintptr_t)gt_mm) & 3) != 0)) why = "verts and gt_mm are required, 4-byte aligned";
  if (!why && (batch < 0 || row0 < 0 || row0 > n_rows || batch > n_rows - row0)) why = "rows [row0, row0 + batch) must lie inside the cache";
  if (why) {
    jrr_set_error("jrr_jfit_gather: %s", why);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  hipLaunchKernelGGL(k_jfit_gather, dim3((unsigned)batch), dim3(JF_THREADS), 0, (hipStream_t)stream, state, verts, gt_mm,
                     reinterpret_cast<float*>(cache), (long long)row0, ns);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_jfit_joints(void* state, const void* cache, int64_t n_rows, int64_t begin, int count, int ns, float* joints,
                               void* stream) {
  const char* why = jf_check_cache(state, cache, n_rows, ns);
  if (!why && (!joints || ((uintptr_t)joints & 3) != 0)) why = "joints is required, 4-byte aligned";
  if (!why && (count < 0 || begin < 0 || begin > n_rows || count > n_rows - begin)) why = "rows [begin, begin + count) must lie inside the cache";
  if (!why && (long long)count * NH > INT32_MAX) why = "count is too large for one call";
  if (why) {
    jrr_set_error("jrr_jfit_joints: %s", why);
    return JRR_ERR_ARG;
  }
  if (count == 0) return JRR_OK;
  hipLaunchKernelGGL(k_jfit_joints, dim3((unsigned)((count * NH + JF_THREADS - 1) / JF_THREADS)), dim3(JF_THREADS), 0, (hipStream_t)stream, state,
                     reinterpret_cast<const float*>(cache), (long long)begin, count, ns, joints);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_jfit_run(void* state, const void* cache, int64_t n_rows, int ns, int batch, int64_t first, int n_steps, float lr,
                            float* loss, float* grad, void* stream) {
  const char* why = jf_check_cache(state, cache, n_rows, ns);
  if (!why && (!loss || (((uintptr_t)loss | (uintptr_t)grad) & 3) != 0)) why = "loss is required; loss and grad 4-byte aligned";
  if (!why && (batch < 1 || n_steps < 0 || first < 0)) why = "batch >= 1, n_steps >= 0 and first >= 0";
  if (!why) {
    const int64_t nmb = (n_rows + batch - 1) / batch;
    if (first > nmb || n_steps > nmb - first) why = "minibatches [first, first + n_steps) must lie inside ceil(n_rows / batch)";
  }
  if (why) {
    jrr_set_error("jrr_jfit_run: %s", why);
    return JRR_ERR_ARG;
  }
  for (int k = 0; k < n_steps; ++k) {
    const int64_t row0 = (first + k) * (int64_t)batch;
    const int count = (int)((n_rows - row0 < batch) ? n_rows - row0 : batch);
    const int nwg = (count + JF_SPW - 1) / JF_SPW;
    hipLaunchKernelGGL(k_jfit_step, dim3((unsigned)(nwg < JF_MAX_WG ? nwg : JF_MAX_WG)), dim3(JF_THREADS), 0, (hipStream_t)stream, state,
                       reinterpret_cast<const float*>(cache), (long long)row0, count, ns, lr, loss + k,
                       (k == n_steps - 1) ? grad : (float*)nullptr);
  }
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_jfit_set_entries(void* state, const float* J, void* stream) {
  if (!state || !J || ((uintptr_t)state & 15) != 0 || ((uintptr_t)J & 3) != 0) {
    jrr_set_error("jrr_jfit_set_entries: bad argument (state 16-byte aligned and J are required)");
    return JRR_ERR_ARG;
  }
  hipLaunchKernelGGL(k_jfit_set_entries, dim3(1), dim3(JF_THREADS), 0, (hipStream_t)stream, state, J);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_jfit_scatter(const void* state, float* J, float* m, float* v, void* stream) {
  if (!state || ((uintptr_t)state & 15) != 0 || (((uintptr_t)J | (uintptr_t)m | (uintptr_t)v) & 3) != 0 || (!J && !m && !v)) {
    jrr_set_error("jrr_jfit_scatter: bad argument (state 16-byte aligned; one of J, m, v at least)");
    return JRR_ERR_ARG;
  }
  hipLaunchKernelGGL(k_jfit_scatter, dim3((JF_CAP + JF_THREADS - 1) / JF_THREADS), dim3(JF_THREADS), 0, (hipStream_t)stream, state, J, m, v);
  CHECK_LAUNCH();
  return JRR_OK;
}
