// Flat streaming kernels (one element, or one float4, per thread and grid stride): Adam over a flat tensor, the step counter, and the sums
// of partial slabs, alone and two in one launch.  (The slab sum that rides beside the per-joint MLP adjoint, k_dconv_bwd_reduce, is
// chain.hip's: it is built from the same dconv.h bodies as the composed kernels there.)
//
// Reference arithmetic restated here:
//   Adam                       torch.optim.Adam defaults, scripts/optimize.py:201-202,263-265
#include "jrr_common.h"
#include "kernels.h"

namespace jrr {

// ------------------------------------------------------------------------------------------
// Adam (torch single-tensor formula): m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ;
// p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps), bias corrections evaluated in double like
// torch's Python scalars.
// ------------------------------------------------------------------------------------------
// (AdamScalars / adam_scalars / adam_update: jrr_common.h -- shared with the fused J-step update of jreg.hip)
__global__ void k_adam_flat(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, size_t n, const int32_t* __restrict__ step, float lr, float beta1,
                            float beta2, float eps, int step_plus) {
  __shared__ AdamScalars sc;
  // step_plus = 1: the counter still holds the number of COMPLETED steps; a later launch of the same stream increments it (the J
  // step: k_jreg_rowsum -- one launch less than a separate increment kernel before this one)
  if (threadIdx.x == 0) sc = adam_scalars(step[0] + step_plus, lr, beta1, beta2, eps);
  __syncthreads();
  AdamScalars s = sc;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float mm = m[i], vv = v[i];
    p[i] = adam_update(p[i], g[i], mm, vv, s);
    m[i] = mm;
    v[i] = vv;
  }
}
int launch_adam_flat(float* p, const float* g, float* m, float* v, size_t n, const int32_t* step, float lr, float b1,
                     float b2, float eps, hipStream_t s, int step_plus) {
  int blocks = (int)((n + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_adam_flat, dim3(blocks), dim3(256), 0, s, p, g, m, v, n, step, lr, b1, b2, eps, step_plus);
  return 0;
}

__global__ void k_step_inc(int32_t* step) { step[0] += 1; }
int launch_step_inc(int32_t* step, hipStream_t s) {
  hipLaunchKernelGGL(k_step_inc, dim3(1), dim3(1), 0, s, step);
  return 0;
}

// out[i] (+)= sum_s P[s*stride + i]  (split-K / vertex-chunk partial slabs), float4-wide
__global__ void k_reduce_slabs(const f32x4* __restrict__ P, int nslab, size_t stride4, f32x4* __restrict__ out,
                               size_t n4, int accumulate) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 acc = P[i];
    for (int s = 1; s < nslab; ++s) acc += P[(size_t)s * stride4 + i];
    if (accumulate) acc += out[i];
    out[i] = acc;
  }
}
int launch_reduce_slabs(const float* P, int nslab, size_t stride, float* out, size_t n, hipStream_t s, int accumulate) {
  size_t n4 = n / 4;
  int blocks = (int)((n4 + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_reduce_slabs, dim3(blocks), dim3(256), 0, s, (const f32x4*)P, nslab, stride / 4, (f32x4*)out, n4,
                     accumulate);
  return 0;
}

// two independent slab sums in ONE launch (small batches: the dA^T slabs of k_lbs_bwd are too many for their consumer and get a
// sum of their own next to the dF^T one -- a launch costs ~4 us of stream time; batch 1024: 0.302 -> 0.292 ms per iteration):
// blocks [0, nb1) the first, the rest the second
__global__ void k_reduce_slabs2(const f32x4* __restrict__ P1, int nslab1, size_t stride1, f32x4* __restrict__ out1, size_t n1, int nb1,
                                const f32x4* __restrict__ P2, int nslab2, size_t stride2, f32x4* __restrict__ out2, size_t n2) {
  const bool first = (int)blockIdx.x < nb1;
  const f32x4* P = first ? P1 : P2;
  f32x4* out = first ? out1 : out2;
  const int nslab = first ? nslab1 : nslab2;
  const size_t stride4 = first ? stride1 : stride2, n4 = first ? n1 : n2;
  const size_t blk = first ? blockIdx.x : blockIdx.x - nb1, nb = first ? (size_t)nb1 : (size_t)gridDim.x - nb1;
  for (size_t i = blk * blockDim.x + threadIdx.x; i < n4; i += nb * blockDim.x) {
    f32x4 acc = P[i];
    for (int s = 1; s < nslab; ++s) acc += P[(size_t)s * stride4 + i];
    out[i] = acc;
  }
}
int launch_reduce_slabs2(const float* P1, int nslab1, size_t stride1, float* out1, size_t n1, const float* P2, int nslab2,
                         size_t stride2, float* out2, size_t n2, hipStream_t s) {
  int b1 = (int)((n1 / 4 + 255) / 256), b2 = (int)((n2 / 4 + 255) / 256);
  if (b1 > 2048) b1 = 2048;
  if (b2 > 2048) b2 = 2048;
  hipLaunchKernelGGL(k_reduce_slabs2, dim3(b1 + b2), dim3(256), 0, s, (const f32x4*)P1, nslab1, stride1 / 4, (f32x4*)out1, n1 / 4, b1,
                     (const f32x4*)P2, nslab2, stride2 / 4, (f32x4*)out2, n2 / 4);
  return 0;
}

}  // namespace jrr
