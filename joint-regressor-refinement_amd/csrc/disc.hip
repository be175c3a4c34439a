// Pose / shape discriminators (/root/reference/scripts/discriminator.py:7-74) -- the VALU parts.
// The two wide layers (768->1024, 1024->1024) and their adjoints run on the MFMA GEMM (gemm.hip);
// here: the per-joint shared MLP (1x1 convs 6->32->32) + 24 per-joint heads, the 1024->1 output
// layer with sigmoid and the MSE adjoint, their input-gradients, and the tiny shape MLP.
//
// Flat parameter vector = state_dict order (offsets in floats):
//   conv0.w 0 (32x6)  conv0.b 192  conv2.w 224 (32x32)  conv2.b 1248
//   linears.i.{w,b} 1280+33i (+32)          i = 0..23
//   fc0.w 2072 (1024x768)  fc0.b 788504  fc2.w 789528 (1024x1024)  fc2.b 1838104
//   fc4.w 1839128 (1x1024) fc4.b 1840152
#include "engine.h"
#include "dconv.h"

namespace jrr {


// per-(pose, joint) shared MLP; lane = pose, blockIdx.y = joint
__device__ __forceinline__ void joint_mlp(const float* __restrict__ P, const float x[6], float h1[32], float h2[32]) {
  const float* w0 = P + DP_CONV0_W;
  const float* b0 = P + DP_CONV0_B;
  const float* w2 = P + DP_CONV2_W;
  const float* b2 = P + DP_CONV2_B;
#pragma unroll
  for (int o = 0; o < 32; ++o) {
    float acc = b0[o];
#pragma unroll
    for (int c = 0; c < 6; ++c) acc = fmaf(w0[o * 6 + c], x[c], acc);
    h1[o] = fmaxf(acc, 0.f);
  }
#pragma unroll
  for (int o = 0; o < 32; ++o) {
    float acc = b2[o];
#pragma unroll
    for (int c = 0; c < 32; ++c) acc = fmaf(w2[o * 32 + c], h1[c], acc);
    h2[o] = fmaxf(acc, 0.f);
  }
}

// The LDS parameter image of the per-joint MLP kernels (layout CL_*), built ONCE per parameter upload (k_conv_image,
// jrr_engine_set_pose_disc).  Building it inside every workgroup -- gathers of conv0.w, two orientations of conv2.w, three
// dependent load rounds -- was 4.7 of k_dconv_fwd's 11.6 us (wall-clock stamps); copying the image is one round.
static_assert(CL_FLOATS % 4 == 0 && CL_FLOATS <= CONV_IMAGE_FLOATS, "image copied in 16-byte pieces");
__global__ void k_conv_image(const float* __restrict__ P, float* __restrict__ L) {
  for (int i = threadIdx.x; i < 256; i += blockDim.x) {
    const int c = i >> 5, o = i & 31;
    L[CL_W0P + i] = (c < 6) ? P[DP_CONV0_W + o * 6 + c] : 0.f;
  }
  for (int i = threadIdx.x; i < 32; i += blockDim.x) { L[CL_B0 + i] = P[DP_CONV0_B + i]; L[CL_B2 + i] = P[DP_CONV2_B + i]; }
  for (int i = threadIdx.x; i < 1024; i += blockDim.x) {
    const int o = i >> 5, c = i & 31;
    const float w = P[DP_CONV2_W + i];          // conv2.w[o][c]
    L[CL_W2 + i] = w;
    L[CL_W2T + c * 32 + o] = w;
    L[CL_W0A + i] = (c < 6) ? P[DP_CONV0_W + o * 6 + c] : 0.f;
  }
  for (int i = threadIdx.x; i < 24 * 33; i += blockDim.x) L[CL_WH + i] = P[DP_HEADS + i];
}
static int launch_conv_image(const float* P, float* img, hipStream_t s) {
  hipLaunchKernelGGL(k_conv_image, dim3(1), dim3(256), 0, s, P, img);
  return 0;
}
// stand-alone launches (operator-level entry points, outer-step paths): (BP / 32) * 6 workgroups of 4 waves
template <bool QUAD>
__global__ __launch_bounds__(256) void k_dconv_fwd(const float* __restrict__ img, const float* __restrict__ x6d,
                                                   float* __restrict__ H2T, float* __restrict__ out, int B, int BP) {
  __shared__ __attribute__((aligned(16))) float L[CL_FLOATS];
  dconv_fwd_body<QUAD>(L, blockIdx.x, img, x6d, H2T, out, B, BP);
}
template <bool QUAD>
__global__ __launch_bounds__(256) void k_dconv_bwd(const float* __restrict__ img, const float* __restrict__ x6d,
                                                   const float* __restrict__ dH2T, const float* __restrict__ gout,
                                                   float scale, float target, float* __restrict__ gx, int B, int BP,
                                                   float* __restrict__ sqj) {
  __shared__ __attribute__((aligned(16))) float L[CL_FLOATS];
  dconv_bwd_body<QUAD>(L, blockIdx.x, img, x6d, dH2T, gout, scale, target, gx, B, BP, sqj);
}
// output layer: z = fc4.w . a2 + fc4.b ; s = sigmoid(z) ; dz = scale (s - target) s (1-s) ;
// dA2T[n][b] = relu'(a2[n][b]) * w[n] * dz.  Block = 1024 threads = 16 waves x 64 poses,
// wave q handles n in [64q, 64q+64).
__global__ __launch_bounds__(1024) void k_disc_out(const float* __restrict__ P, const float* __restrict__ A2T,
                                                   float* __restrict__ out, float* __restrict__ dA2T,
                                                   const float* __restrict__ gout, float scale, float target, int B,
                                                   int BP, float* __restrict__ dz0, float* __restrict__ sq0) {
  __shared__ float red[16][64];
  __shared__ float dzs[64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int b = blockIdx.x * 64 + lane;
  const float* w = P + DP_FC4_W;
  float acc = 0.f;
  for (int n = q * 64; n < q * 64 + 64; ++n) acc = fmaf(w[n], A2T[(size_t)n * BP + b], acc);
  red[q][lane] = acc;
  __syncthreads();
  if (q == 0) {
    float z = P[DP_FC4_B];
#pragma unroll
    for (int i = 0; i < 16; ++i) z += red[i][lane];
    float s = sigmoidf(z);
    if (out && b < B) out[(size_t)b * 25] = s;
    if (sq0) sq0[b] = (b < B) ? (s - target) * (s - target) : 0.f;
    const float up = gout ? ((b < B) ? gout[(size_t)b * 25] : 0.f) : scale * (s - target);
    dzs[lane] = (b < B) ? up * s * (1.f - s) : 0.f;
    if (dz0) dz0[b] = dzs[lane];
  }
  __syncthreads();
  if (dA2T) {
    const float dz = dzs[lane];
    for (int n = q * 64; n < q * 64 + 64; ++n) {
      float a = A2T[(size_t)n * BP + b];
      dA2T[(size_t)n * BP + b] = (a > 0.f) ? w[n] * dz : 0.f;
    }
  }
}

// shape discriminator 10 -> 10 -> 5 -> 1 (discriminator.py:57-74): forward + input gradient of
// weight*mean((s-target)^2).  Params: w0 0 (10x10) b0 100 w2 110 (5x10) b2 160 w4 165 (1x5) b4 170
__global__ void k_shape_disc(const float* __restrict__ P, const float* __restrict__ betas, float* __restrict__ out,
                             float* __restrict__ gb, float scale, float target, int B, const float* __restrict__ gout,
                             float* __restrict__ sq) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float x[10], h1[10], h2[5];
#pragma unroll
  for (int i = 0; i < 10; ++i) x[i] = betas[(size_t)b * 10 + i];
#pragma unroll
  for (int o = 0; o < 10; ++o) {
    float acc = P[100 + o];
#pragma unroll
    for (int i = 0; i < 10; ++i) acc = fmaf(P[o * 10 + i], x[i], acc);
    h1[o] = fmaxf(acc, 0.f);
  }
#pragma unroll
  for (int o = 0; o < 5; ++o) {
    float acc = P[160 + o];
#pragma unroll
    for (int i = 0; i < 10; ++i) acc = fmaf(P[110 + o * 10 + i], h1[i], acc);
    h2[o] = fmaxf(acc, 0.f);
  }
  float z = P[170];
#pragma unroll
  for (int i = 0; i < 5; ++i) z = fmaf(P[165 + i], h2[i], z);
  const float s = sigmoidf(z);
  if (out) out[b] = s;
  if (sq) sq[b] = (s - target) * (s - target);
  if (!gb) return;
  const float dz = (gout ? gout[b] : scale * (s - target)) * s * (1.f - s);
  float dh2[5], dh1[10];
#pragma unroll
  for (int i = 0; i < 5; ++i) dh2[i] = (h2[i] > 0.f) ? dz * P[165 + i] : 0.f;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < 5; ++o) acc = fmaf(P[110 + o * 10 + i], dh2[o], acc);
    dh1[i] = (h1[i] > 0.f) ? acc : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < 10; ++o) acc = fmaf(P[o * 10 + i], dh1[o], acc);
    gb[(size_t)b * 10 + i] = acc;
  }
}

// ---- weight gradients (outer-step discriminator update, scripts/optimize.py:276-293) ----
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ void wave_atomic_add(float v, float* dst, int lane) {
  v = wave_sum(v);
  if (lane == 0) atomicAdd(dst, v);
}

// out[r] += sum_c M[r][c] * (vec ? vec[c] : 1)
__global__ void k_rowdot_accum(const float* __restrict__ M, int ld, const float* __restrict__ vec, float* __restrict__ out,
                               int cols) {
  __shared__ float red[256];
  const int r = blockIdx.x;
  float acc = 0.f;
  for (int c = threadIdx.x; c < cols; c += blockDim.x) acc += M[(size_t)r * ld + c] * (vec ? vec[c] : 1.f);
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[r] += red[0];
}

// per-joint MLP + head weight gradients.  One wave per (64 poses, joint): lane = pose runs the joint MLP forward
// and backward in registers; the outer products over the 64 poses (dW2 = dh2^T h1, dW0 = dh1^T x, the bias and head
// sums) are taken from LDS-staged copies with lane = (output row o, half of the columns) and written as ONE partial
// slab per wave -- no atomics; the caller reduces the slabs.
// dH2T = gradient arriving from fc0.
constexpr int CW_LD = 36;                      // LDS row stride in floats (16-byte aligned rows)
__global__ __launch_bounds__(64) void k_disc_conv_bwd_params(const float* __restrict__ P, const float* __restrict__ x6d,
                                                             const float* __restrict__ dH2T, const float* __restrict__ gout,
                                                             float scale, float target, float* __restrict__ slab_shared,
                                                             float* __restrict__ slab_heads, int B, int BP) {
  __shared__ __attribute__((aligned(16))) float Sa[64 * CW_LD];
  __shared__ __attribute__((aligned(16))) float Sb[64 * CW_LD];
  const int lane = threadIdx.x, b = blockIdx.x * 64 + lane, j = blockIdx.y;
  const int o_ = lane & 31, hf = lane >> 5;
  const bool ok = b < B;
  float aW2[16], aW0[3] = {0.f, 0.f, 0.f}, ab2 = 0.f, ab0 = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) aW2[k] = 0.f;
  {
    float x[6], h1[32], h2[32];
#pragma unroll
    for (int c = 0; c < 6; ++c) x[c] = ok ? x6d[((size_t)b * NJ + j) * 6 + c] : 0.f;
    joint_mlp(P, x, h1, h2);
    const float* wh = P + DP_HEADS + 33 * j;
    float z = wh[32];
#pragma unroll
    for (int o = 0; o < 32; ++o) z = fmaf(wh[o], h2[o], z);
    const float s = sigmoidf(z);
    const float dz = ok ? (gout ? gout[(size_t)b * 25 + 1 + j] : scale * (s - target)) * s * (1.f - s) : 0.f;
    float dh2[32], dh1[32];
#pragma unroll
    for (int o = 0; o < 32; ++o) {
      float g = dz * wh[o];
      if (ok) g += dH2T[(size_t)(j * 32 + o) * BP + b];
      dh2[o] = (ok && h2[o] > 0.f) ? g : 0.f;
    }
    const float* w2 = P + DP_CONV2_W;
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int o = 0; o < 32; ++o) acc = fmaf(w2[o * 32 + c], dh2[o], acc);
      dh1[c] = (h1[c] > 0.f) ? acc : 0.f;
    }
    // ---- head of joint j: dW[o] = sum_b dz h2[o], db = sum_b dz
#pragma unroll
    for (int o = 0; o < 32; ++o) Sa[lane * CW_LD + o] = dz * h2[o];
    Sa[lane * CW_LD + 32] = dz;
    __syncthreads();
    if (lane < 33) {
      float acc = 0.f;
      for (int bb = 0; bb < 64; ++bb) acc += Sa[bb * CW_LD + lane];
      slab_heads[(size_t)blockIdx.x * 792 + 33 * j + lane] = acc;
    }
    __syncthreads();
    // ---- conv2: dW2[o][c] += sum_b dh2[b][o] h1[b][c]; db2[o] += sum_b dh2[b][o]
#pragma unroll
    for (int o = 0; o < 32; ++o) { Sa[lane * CW_LD + o] = dh2[o]; Sb[lane * CW_LD + o] = h1[o]; }
    __syncthreads();
    for (int bb = 0; bb < 64; ++bb) {
      const float a = Sa[bb * CW_LD + o_];
      const f32x4* hr = reinterpret_cast<const f32x4*>(&Sb[bb * CW_LD + hf * 16]);
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) {
        const f32x4 r = hr[k4];
#pragma unroll
        for (int k = 0; k < 4; ++k) aW2[k4 * 4 + k] = fmaf(a, r[k], aW2[k4 * 4 + k]);
      }
      ab2 += a;
    }
    __syncthreads();
    // ---- conv0: dW0[o][c] += sum_b dh1[b][o] x[b][c]; db0[o] += sum_b dh1[b][o]
#pragma unroll
    for (int o = 0; o < 32; ++o) Sa[lane * CW_LD + o] = dh1[o];
#pragma unroll
    for (int c = 0; c < 6; ++c) Sb[lane * CW_LD + c] = x[c];
    __syncthreads();
    for (int bb = 0; bb < 64; ++bb) {
      const float a = Sa[bb * CW_LD + o_];
#pragma unroll
      for (int k = 0; k < 3; ++k) aW0[k] = fmaf(a, Sb[bb * CW_LD + hf * 3 + k], aW0[k]);
      ab0 += a;
    }
    __syncthreads();
  }
  float* slab = slab_shared + ((size_t)blockIdx.x * NJ + j) * 1280;
#pragma unroll
  for (int k = 0; k < 16; ++k) slab[DP_CONV2_W + o_ * 32 + hf * 16 + k] = aW2[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) slab[DP_CONV0_W + o_ * 6 + hf * 3 + k] = aW0[k];
  if (hf == 0) { slab[DP_CONV2_B + o_] = ab2; slab[DP_CONV0_B + o_] = ab0; }
}

// shape discriminator: forward, weight gradients of mean((s-target)^2), per-pose squared error
__global__ __launch_bounds__(64) void k_shape_disc_bwd_params(const float* __restrict__ P, const float* __restrict__ betas,
                                                              const float* __restrict__ gout, float scale, float target,
                                                              float* __restrict__ dP,
                                                              float* __restrict__ sqerr, int B) {
  const int lane = threadIdx.x, b = blockIdx.x * 64 + lane;
  const bool ok = b < B;
  float x[10], h1[10], h2[5];
#pragma unroll
  for (int i = 0; i < 10; ++i) x[i] = ok ? betas[(size_t)b * 10 + i] : 0.f;
#pragma unroll
  for (int o = 0; o < 10; ++o) {
    float acc = P[100 + o];
#pragma unroll
    for (int i = 0; i < 10; ++i) acc = fmaf(P[o * 10 + i], x[i], acc);
    h1[o] = fmaxf(acc, 0.f);
  }
#pragma unroll
  for (int o = 0; o < 5; ++o) {
    float acc = P[160 + o];
#pragma unroll
    for (int i = 0; i < 10; ++i) acc = fmaf(P[110 + o * 10 + i], h1[i], acc);
    h2[o] = fmaxf(acc, 0.f);
  }
  float z = P[170];
#pragma unroll
  for (int i = 0; i < 5; ++i) z = fmaf(P[165 + i], h2[i], z);
  const float s = sigmoidf(z);
  if (ok && sqerr) sqerr[b] = (s - target) * (s - target);
  const float dz = ok ? (gout ? gout[b] : scale * (s - target)) * s * (1.f - s) : 0.f;
  float dh2[5], dh1[10];
  wave_atomic_add(dz, dP + 170, lane);
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    wave_atomic_add(dz * h2[i], dP + 165 + i, lane);
    dh2[i] = (h2[i] > 0.f) ? dz * P[165 + i] : 0.f;
    wave_atomic_add(dh2[i], dP + 160 + i, lane);
  }
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < 5; ++o) {
      acc = fmaf(P[110 + o * 10 + i], dh2[o], acc);
      wave_atomic_add(dh2[o] * h1[i], dP + 110 + o * 10 + i, lane);
    }
    dh1[i] = (h1[i] > 0.f) ? acc : 0.f;
    wave_atomic_add(dh1[i], dP + 100 + i, lane);
  }
#pragma unroll
  for (int o = 0; o < 10; ++o)
#pragma unroll
    for (int i = 0; i < 10; ++i) wave_atomic_add(dh1[o] * x[i], dP + o * 10 + i, lane);
}

// sqerr[b] = sum_k (out[b][k] - target)^2
__global__ void k_sqerr_rows(const float* __restrict__ out, int ncol, float target, float* __restrict__ sqerr, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float acc = 0.f;
  for (int k = 0; k < ncol; ++k) { const float d = out[(size_t)b * ncol + k] - target; acc += d * d; }
  sqerr[b] = acc;
}

// out[b*25] = sigmoid(fc4.b + sum_t zpart[t][b])   (operator-level forward: the fc4 dot comes from the fc2 epilogue)
__global__ void k_disc_z_finish(const float* __restrict__ zpart, int nz, int ld, const float* __restrict__ zbias,
                                float* __restrict__ out, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float z = zbias[0];
  for (int t = 0; t < nz; ++t) z += zpart[(size_t)t * ld + b];
  out[(size_t)b * 25] = sigmoidf(z);
}
static int launch_disc_z_finish(const float* zpart, int nz, int ld, const float* zbias, float* out, int B, hipStream_t s) {
  hipLaunchKernelGGL(k_disc_z_finish, dim3((B + 255) / 256), dim3(256), 0, s, zpart, nz, ld, zbias, out, B);
  return 0;
}
// out[r][c] = w[r] * in[r][c]
__global__ void k_scale_rows(const float* __restrict__ in, const float* __restrict__ w, float* __restrict__ out, int rows, int cols) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)rows * cols) out[i] = w[i / cols] * in[i];
}
static int launch_scale_rows(const float* in, const float* w, float* out, int rows, int cols, hipStream_t s) {
  hipLaunchKernelGGL(k_scale_rows, dim3((unsigned)(((size_t)rows * cols + 255) / 256)), dim3(256), 0, s, in, w, out, rows, cols);
  return 0;
}

// out[b] = sum_r M[r][b]   (rows of a [rows][ld] pose-contiguous array)
__global__ void k_colsum(const float* __restrict__ M, int rows, int ld, float* __restrict__ out, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float acc = 0.f;
  for (int r = 0; r < rows; ++r) acc += M[(size_t)r * ld + b];
  out[b] = acc;
}
int launch_colsum(const float* M, int rows, int ld, float* out, int B, hipStream_t s) {
  hipLaunchKernelGGL(k_colsum, dim3((B + 255) / 256), dim3(256), 0, s, M, rows, ld, out, B);
  return 0;
}

static int launch_rowdot_accum(const float* M, int ld, const float* vec, float* out, int rows, int cols, hipStream_t s) {
  hipLaunchKernelGGL(k_rowdot_accum, dim3(rows), dim3(256), 0, s, M, ld, vec, out, cols);
  return 0;
}
// conv / per-joint-head weight gradients as partial slabs: shared [24 * BP/64][1280] (conv0 W,b | conv2 W,b in the
// DP_* order) and heads [BP/64][792]; the caller reduces them into the flat gradient
static int launch_disc_conv_bwd_params(const float* P, const float* x6d, const float* dH2T, const float* gout, float scale,
                                float target, float* slab_shared, float* slab_heads, int B, int BP, hipStream_t s) {
  hipLaunchKernelGGL(k_disc_conv_bwd_params, dim3(BP / 64, NJ), dim3(64), 0, s, P, x6d, dH2T, gout, scale, target, slab_shared,
                     slab_heads, B, BP);
  return 0;
}
static int launch_shape_disc_bwd_params(const float* P, const float* betas, const float* gout, float scale, float target,
                                 float* dparams, float* sqerr, int B, hipStream_t s) {
  hipLaunchKernelGGL(k_shape_disc_bwd_params, dim3((B + 63) / 64), dim3(64), 0, s, P, betas, gout, scale, target, dparams, sqerr, B);
  return 0;
}
static int launch_sqerr_rows(const float* out, int ncol, float target, float* sqerr, int B, hipStream_t s) {
  hipLaunchKernelGGL(k_sqerr_rows, dim3((B + 255) / 256), dim3(256), 0, s, out, ncol, target, sqerr, B);
  return 0;
}

// [rows][cols] -> [cols][rows]
__global__ void k_transpose(const float* __restrict__ in, float* __restrict__ out, int rows, int cols, int ldin, int ldout) {
  __shared__ float t[32][33];
  int c = blockIdx.x * 32 + threadIdx.x, r0 = blockIdx.y * 32;
  for (int i = threadIdx.y; i < 32; i += blockDim.y)
    if (r0 + i < rows && c < cols) t[i][threadIdx.x] = in[(size_t)(r0 + i) * ldin + c];
  __syncthreads();
  int r = r0 + threadIdx.x, c0 = blockIdx.x * 32;
  for (int i = threadIdx.y; i < 32; i += blockDim.y)
    if (c0 + i < cols && r < rows) out[(size_t)(c0 + i) * ldout + r] = t[threadIdx.x][i];
}

int launch_transpose(const float* in, float* out, int rows, int cols, hipStream_t s, int ldin, int ldout) {
  hipLaunchKernelGGL(k_transpose, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(32, 8), 0, s, in, out, rows, cols,
                     ldin ? ldin : cols, ldout ? ldout : rows);
  return 0;
}

int launch_disc_conv_fwd(const float* P, const float* x6d, float* H2T, float* out, int B, int BP, hipStream_t s, int quad) {
  if (quad) hipLaunchKernelGGL((k_dconv_fwd<true>), dim3((BP / 32) * 6), dim3(256), 0, s, P, x6d, H2T, out, B, BP);
  else hipLaunchKernelGGL((k_dconv_fwd<false>), dim3((BP / 32) * 6), dim3(256), 0, s, P, x6d, H2T, out, B, BP);
  return 0;
}
static int launch_disc_out(const float* P, const float* A2T, float* out, float* dA2T, const float* gout, float scale,
                    float target, int B, int BP, hipStream_t s, float* dz0 = nullptr, float* sq0 = nullptr) {
  hipLaunchKernelGGL(k_disc_out, dim3(BP / 64), dim3(1024), 0, s, P, A2T, out, dA2T, gout, scale, target, B, BP, dz0, sq0);
  return 0;
}
int launch_disc_conv_bwd(const float* P, const float* x6d, const float* dH2T, const float* gout, float scale,
                         float target, float* gx, int B, int BP, hipStream_t s, float* sqj, int quad) {
  if (quad) hipLaunchKernelGGL((k_dconv_bwd<true>), dim3((BP / 32) * 6), dim3(256), 0, s, P, x6d, dH2T, gout, scale, target, gx, B, BP, sqj);
  else hipLaunchKernelGGL((k_dconv_bwd<false>), dim3((BP / 32) * 6), dim3(256), 0, s, P, x6d, dH2T, gout, scale, target, gx, B, BP, sqj);
  return 0;
}
int launch_shape_disc(const float* P, const float* betas, float* out, float* gb, float scale, float target, int B,
                      hipStream_t s, const float* gout, float* sq) {
  hipLaunchKernelGGL(k_shape_disc, dim3((B + 63) / 64), dim3(64), 0, s, P, betas, out, gb, scale, target, B, gout, sq);
  return 0;
}

}  // namespace jrr

using namespace jrr;

extern "C" int jrr_engine_set_pose_disc(jrr_engine_t* e, const float* P, void* stream) {
  if (!e || !P) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  if (!(e->flags & JRR_FLAG_POSE_DISC)) { jrr_set_error("engine created without JRR_FLAG_POSE_DISC"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  JRR_HIP(hipMemcpyAsync(e->Pd, P, (size_t)DP_TOTAL * 4, hipMemcpyDeviceToDevice, s));
  launch_transpose(e->Pd + DP_FC0_W, e->W0T, 1024, 768, s);    // [out][in] -> [in][out]
  launch_transpose(e->Pd + DP_FC2_W, e->W2T, 1024, 1024, s);
  launch_scale_rows(e->Pd + DP_FC2_W, e->Pd + DP_FC4_W, e->W2s, 1024, 1024, s);   // row n of fc2.w times fc4.w[n]
  launch_to_quads(e->W0T, 1024, e->W0Tq, 768, 1024, s);                // A operands A[k][m] of the four loop GEMMs, in quads
  launch_to_quads(e->W2T, 1024, e->W2Tq, 1024, 1024, s);
  launch_to_quads(e->W2s, 1024, e->W2sq, 1024, 1024, s);
  launch_to_quads(e->Pd + DP_FC0_W, 768, e->W0q, 1024, 768, s);
  launch_conv_image(e->Pd, e->convL, s);
  CHECK_LAUNCH();
  e->have_pd = true;
  return JRR_OK;
}

extern "C" int jrr_engine_set_shape_disc(jrr_engine_t* e, const float* P, void* stream) {
  if (!e || !P) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  if (!(e->flags & JRR_FLAG_SHAPE_DISC)) { jrr_set_error("engine created without JRR_FLAG_SHAPE_DISC"); return JRR_ERR_STATE; }
  JRR_HIP(hipMemcpyAsync(e->Ps, P, (size_t)JRR_SHAPE_DISC_PARAMS * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  e->have_sd = true;
  return JRR_OK;
}

// ---- pose discriminator --------------------------------------------------------------------
// Six launches per forward + input gradient (scripts/discriminator.py:32-54 and its adjoint):
//   k_dconv_fwd (per-joint MLP, MFMA)  ->  fc0 GEMM (+bias, ReLU)  ->  fc2 GEMM (+bias, ReLU, the fc4 dot product
//   w4 . a2 as per-column partials in the epilogue; what it stores is relu'(a2) as 0 / 1: nothing else of a2 is read again)
//   ->  fc2 adjoint GEMM on that indicator (dz from the partial dots in the prologue multiplies the finished column sums
//   in the epilogue; fc2.w pre-scaled by w4: the rank-one output-layer adjoint is never materialised)  ->  fc0 adjoint
//   GEMM  ->  k_dconv_bwd.
// All four GEMMs: exact 128x64 tiles (512 workgroups at 4096 poses), 3-deep LDS-DMA ring.
// The loop path keeps every activation in quads [row/4][pose][4] (k_disc_gemm); the weight-gradient path of the outer
// step (disc_backward_params) needs row-major activations for its transposes / row sums and runs the row-major kernels.
// conv_done: the per-joint MLP already ran (fused into the chain-forward launch, launch_prep_fwd_dconv)
int jrr::disc_forward(jrr_engine* e, const float* x6d, float* out, hipStream_t s, bool quad, bool conv_done) {
  if (!conv_done) launch_disc_conv_fwd(e->convL, x6d, e->H2T, out, e->B, e->BP, s, quad ? 1 : 0);
  GemmArgs g;
  g.mask = nullptr; g.split_stride = 0; g.N = e->BP; g.ldb = e->BP; g.ldo = e->BP;
  g.A = quad ? e->W0Tq : e->W0T; g.lda = 1024; g.Bm = e->H2T; g.Out = e->A1T; g.bias = e->Pd + DP_FC0_B; g.M = 1024; g.K = 768;
  int rc = quad ? launch_disc_gemm_q(g, EPI_BIAS_RELU, 0, s) : launch_gemm_128x64(g, EPI_BIAS_RELU, 1, s);
  if (rc) return rc;
  g.A = quad ? e->W2Tq : e->W2T; g.lda = 1024; g.Bm = e->A1T; g.Out = e->A2T; g.bias = e->Pd + DP_FC2_B; g.M = 1024; g.K = 1024;
  if (!quad) return launch_gemm_128x64(g, EPI_BIAS_RELU, 1, s);
  g.dotw = e->Pd + DP_FC4_W; g.dot_out = e->zpart;
  return launch_disc_gemm_q(g, EPI_BIAS_RELU_DOT, 0, s);
}

// skip_conv: the caller runs the per-joint MLP adjoint itself (fused with the dF^T slab sum, launch_dconv_bwd_reduce)
int jrr::disc_backward_input(jrr_engine* e, const float* x6d, float* out, const float* gout, float scale, float target, float* gx,
                             hipStream_t s, float* sq, bool skip_conv) {
  GemmArgs g;
  g.bias = nullptr; g.split_stride = 0; g.N = e->BP; g.ldb = e->BP; g.ldo = e->BP;
  // dA1T[k][b] = relu'(A1T) * sum_n (fc4.w[n] fc2.w[n][k]) relu'(A2T[n][b]) dz[b]
  g.A = e->W2sq; g.lda = 1024; g.Bm = e->A2T; g.Out = e->dA1T; g.mask = e->A1T; g.M = 1024; g.K = 1024;
  g.zpart = e->zpart; g.nzpart = 16; g.zbias = e->Pd + DP_FC4_B; g.gout = gout; g.gout_ld = 25; g.scale = scale; g.target = target;
  g.nvalid = e->B; g.sq0 = sq; g.out0 = out; g.out0_ld = 25;
  int rc = launch_disc_gemm_q(g, EPI_MASK, 2, s);
  if (rc) return rc;
  // dH2T[k][b] = sum_n fc0.w[n][k] dA1T[n][b]
  GemmArgs h;
  h.bias = nullptr; h.split_stride = 0; h.N = e->BP; h.ldb = e->BP; h.ldo = e->BP;
  h.A = e->W0q; h.lda = 768; h.Bm = e->dA1T; h.Out = e->dH2T; h.mask = nullptr; h.M = 768; h.K = 1024;
  rc = launch_disc_gemm_q(h, EPI_STORE, 0, s);
  if (rc) return rc;
  if (!skip_conv) launch_disc_conv_bwd(e->convL, x6d, e->dH2T, gout, scale, target, gx, e->B, e->BP, s, sq, 1);
  return 0;
}

extern "C" int jrr_pose_disc_forward(jrr_engine_t* e, const float* x6d, float* out, void* stream) {
  if (!e || !x6d || !out) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  if (!e->have_pd) { jrr_set_error("pose discriminator not set"); return JRR_ERR_STATE; }
  hipStream_t s = (hipStream_t)stream;
  int rc = disc_forward(e, x6d, out, s);
  if (rc) return rc;
  launch_disc_z_finish(e->zpart, 16, e->BP, e->Pd + DP_FC4_B, out, e->B, s);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_pose_disc_backward_input(jrr_engine_t* e, const float* x6d, float weight, float target, float* dx,
                                            void* stream) {
  if (!e || !x6d || !dx) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  if (!e->have_pd) { jrr_set_error("pose discriminator not set"); return JRR_ERR_STATE; }
  const float scale = (float)(2.0 * (double)weight / ((double)e->bnorm * 25.0));
  int rc = disc_backward_input(e, x6d, nullptr, nullptr, scale, target, dx, (hipStream_t)stream);
  if (rc) return rc;
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_pose_disc_vjp_input(jrr_engine_t* e, const float* x6d, const float* gout, float* dx, void* stream) {
  if (!e || !x6d || !gout || !dx) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  if (!e->have_pd) { jrr_set_error("pose discriminator not set"); return JRR_ERR_STATE; }
  int rc = disc_backward_input(e, x6d, nullptr, gout, 0.f, 0.f, dx, (hipStream_t)stream);
  if (rc) return rc;
  CHECK_LAUNCH();
  return JRR_OK;
}

// weight gradients of the pose discriminator: either of the MSE against `target` (gout == NULL; scale = 2/(bnorm*25))
// or the vector-Jacobian product for an arbitrary upstream gradient gout (B,25)
static int disc_backward_params(jrr_engine* e, const float* x6d, const float* gout, float scale, float target, float* dP,
                                float* sqerr, hipStream_t s) {
  int rc = disc_forward(e, x6d, e->dsc, s, false);        // row-major activations for the transposes / row sums below
  if (rc) return rc;
  launch_disc_out(e->Pd, e->A2T, e->dsc, e->dA2T, gout, scale, target, e->B, e->BP, s, e->dz0);
  if (sqerr) launch_sqerr_rows(e->dsc, 25, target, sqerr, e->B, s);
  // fc4: dw[n] += sum_b A2T[n][b] dz0[b] ; db += sum_b dz0[b]
  launch_rowdot_accum(e->A2T, e->BP, e->dz0, dP + DP_FC4_W, 1024, e->BP, s);
  launch_rowdot_accum(e->dz0, e->BP, nullptr, dP + DP_FC4_B, 1, e->BP, s);
  // fc2: dW[n][k] += sum_b dA2T[n][b] A1T[k][b] (pose-major copies feed the K-major GEMM) ; db[n] += sum_b dA2T[n][b]
  launch_transpose(e->dA2T, e->TrA, 1024, e->BP, s);
  launch_transpose(e->A1T, e->TrB, 1024, e->BP, s);
  GemmArgs g;
  g.bias = nullptr; g.mask = nullptr; g.split_stride = 0;
  // the pose dimension is the reduction: split it so that the 64 output tiles become >= 512 workgroups; partial
  // slabs, then a wide accumulate-reduce into the flat gradient (deterministic, no atomics)
  const int wsplit = e->BP >= 4096 ? 8 : e->BP >= 1024 ? 4 : e->BP >= 256 ? 2 : 1;
  g.A = e->TrA; g.lda = 1024; g.Bm = e->TrB; g.ldb = 1024; g.Out = e->wgs; g.ldo = 1024; g.M = 1024; g.N = 1024; g.K = e->BP;
  g.split_stride = (size_t)1024 * 1024;
  rc = launch_gemm_128(g, EPI_STORE, wsplit, s);
  if (rc) return rc;
  launch_reduce_slabs(e->wgs, wsplit, (size_t)1024 * 1024, dP + DP_FC2_W, (size_t)1024 * 1024, s, 1);
  g.split_stride = 0;
  launch_rowdot_accum(e->dA2T, e->BP, nullptr, dP + DP_FC2_B, 1024, e->BP, s);
  // back through fc2
  g.A = e->Pd + DP_FC2_W; g.lda = 1024; g.Bm = e->dA2T; g.ldb = e->BP; g.Out = e->dA1T; g.ldo = e->BP; g.mask = e->A1T;
  g.M = 1024; g.N = e->BP; g.K = 1024;
  rc = launch_gemm_128x64(g, EPI_MASK, 1, s);
  if (rc) return rc;
  // fc0
  launch_transpose(e->dA1T, e->TrA, 1024, e->BP, s);
  launch_transpose(e->H2T, e->TrB, 768, e->BP, s);
  g.mask = nullptr;
  g.A = e->TrA; g.lda = 1024; g.Bm = e->TrB; g.ldb = 768; g.Out = e->wgs; g.ldo = 768; g.M = 1024; g.N = 768; g.K = e->BP;
  g.split_stride = (size_t)1024 * 768;
  rc = launch_gemm_128(g, EPI_STORE, wsplit, s);
  if (rc) return rc;
  launch_reduce_slabs(e->wgs, wsplit, (size_t)1024 * 768, dP + DP_FC0_W, (size_t)1024 * 768, s, 1);
  g.split_stride = 0;
  launch_rowdot_accum(e->dA1T, e->BP, nullptr, dP + DP_FC0_B, 1024, e->BP, s);
  g.A = e->Pd + DP_FC0_W; g.lda = 768; g.Bm = e->dA1T; g.ldb = e->BP; g.Out = e->dH2T; g.ldo = e->BP; g.M = 768; g.N = e->BP; g.K = 1024;
  rc = launch_gemm_128x64(g, EPI_STORE, 1, s);
  if (rc) return rc;
  {   // conv / head weight gradients: one slab per wave [pose group][joint][1280], reduced in two wide steps
      // (over the pose groups, then over the joints) into the flat gradient
    const int ng = e->BP / 64;
    float* slab_shared = e->wgs;
    float* slab_heads = slab_shared + (size_t)NJ * ng * 1280;
    float* tmp = slab_heads + (size_t)ng * 792;
    launch_disc_conv_bwd_params(e->Pd, x6d, e->dH2T, gout, scale, target, slab_shared, slab_heads, e->B, e->BP, s);
    launch_reduce_slabs(slab_shared, ng, (size_t)NJ * 1280, tmp, (size_t)NJ * 1280, s, 0);
    launch_reduce_slabs(tmp, NJ, 1280, dP + DP_CONV0_W, 1280, s, 1);
    launch_reduce_slabs(slab_heads, ng, 792, dP + DP_HEADS, 792, s, 1);
  }
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_pose_disc_backward_params(jrr_engine_t* e, const float* x6d, float target, float* dP, float* sqerr,
                                             void* stream) {
  if (!e || !x6d || !dP) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  if (!e->have_pd) { jrr_set_error("pose discriminator not set"); return JRR_ERR_STATE; }
  return disc_backward_params(e, x6d, nullptr, (float)(2.0 / ((double)e->bnorm * 25.0)), target, dP, sqerr, (hipStream_t)stream);
}

extern "C" int jrr_pose_disc_vjp_params(jrr_engine_t* e, const float* x6d, const float* gout, float* dP, void* stream) {
  if (!e || !x6d || !gout || !dP) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  if (!e->have_pd) { jrr_set_error("pose discriminator not set"); return JRR_ERR_STATE; }
  return disc_backward_params(e, x6d, gout, 0.f, 0.f, dP, nullptr, (hipStream_t)stream);
}

extern "C" int jrr_shape_disc_vjp_params(jrr_engine_t* e, const float* betas, const float* gout, float* dP, void* stream) {
  if (!e || !betas || !gout || !dP) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  if (!e->have_sd) { jrr_set_error("shape discriminator not set"); return JRR_ERR_STATE; }
  launch_shape_disc_bwd_params(e->Ps, betas, gout, 0.f, 0.f, dP, nullptr, e->B, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_shape_disc_backward_params(jrr_engine_t* e, const float* betas, float target, float* dP, float* sqerr,
                                              void* stream) {
  if (!e || !betas || !dP) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  if (!e->have_sd) { jrr_set_error("shape discriminator not set"); return JRR_ERR_STATE; }
  const float scale = (float)(2.0 / ((double)e->bnorm * 1.0));
  launch_shape_disc_bwd_params(e->Ps, betas, nullptr, scale, target, dP, sqerr, e->B, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_shape_disc_forward(jrr_engine_t* e, const float* betas, float* out, void* stream) {
  if (!e || !betas || !out) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  if (!e->have_sd) { jrr_set_error("shape discriminator not set"); return JRR_ERR_STATE; }
  launch_shape_disc(e->Ps, betas, out, nullptr, 0.f, 0.f, e->B, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_shape_disc_vjp_input(jrr_engine_t* e, const float* betas, const float* gout, float* dbetas, void* stream) {
  if (!e || !betas || !gout || !dbetas) return JRR_ERR_ARG;
  e->st.workspace_overwritten();
  if (!e->have_sd) { jrr_set_error("shape discriminator not set"); return JRR_ERR_STATE; }
  launch_shape_disc(e->Ps, betas, nullptr, dbetas, 0.f, 0.f, e->B, (hipStream_t)stream, gout);
  CHECK_LAUNCH();
  return JRR_OK;
}
