// The fit report (the reference's viz(), scripts/optimize.py:28-74, around its inner loop at :204-218 and :268-274):
//   render > 0.5, mask_rcnn > 0.8               scripts/optimize.py:35-42   (torch.where on float32 tensors: strict, fp32)
//   the disagreement map mask + render == 1      scripts/optimize.py:47-48
//   plt.scatter of the 2-D joints over it        scripts/optimize.py:61-64   (imshow: pixel (x, y) has its centre AT the integer coordinate)
//
// k_sil_compare: per pose the four pixel counts {render & mask, render | mask, render, mask} of the two thresholded images, from which
// the host takes the IoU.  Memory-bound (8 bytes per pixel, read once as float4); the sums are integers: wave shuffles, LDS integer
// atomics, then one integer atomic per count and workgroup -- the result does not depend on the order of the additions.
// k_fit_overlay: the picture of one pose, (size,size,3) uint8 ready for a PNG encoder: the image crop (or black) tinted by the
// agreement of render and mask, the joint discs on top.  One thread assembles four pixels of a row (12 bytes, three dword stores) from
// 16-byte loads of alpha, mask and the three image planes; the pose's joints wait in LDS.  Every operation is stated in include/jrr.h
// and rounded once (no product is fused into an addition), so a host restatement reproduces every byte.
#include "jrr_common.h"

namespace jrr {

constexpr int RP_THREADS = 256;
constexpr int SC_QUADS_PER_THREAD = 4;           // k_sil_compare: float4 pairs a thread reads when a pose has enough of them
constexpr int OV_MAX_SETS = 3, OV_JOINTS = 17;

#pragma clang fp contract(off)

// a product that is rounded BEFORE it meets an addition (as image.hip's): the empty asm keeps the compiler from fusing the two
__device__ __forceinline__ float rp_mul_rn(float a, float b) {
  float p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int off = warpSize >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// grid: batch * nblk workgroups, workgroup (b, k) strides over the nq = h * w / 4 quads of pose b
__global__ __launch_bounds__(RP_THREADS) void k_sil_compare(const float* __restrict__ alpha, const float* __restrict__ mask, int nq, int nblk,
                                                            float thr_r, float thr_m, int* __restrict__ counts) {
  __shared__ int s_c[3];
  const int tid = threadIdx.x, b = (int)blockIdx.x / nblk, k = (int)blockIdx.x - b * nblk;
  if (tid < 3) s_c[tid] = 0;
  __syncthreads();
  const float4* a4 = reinterpret_cast<const float4*>(alpha) + (size_t)b * nq;
  const float4* m4 = reinterpret_cast<const float4*>(mask) + (size_t)b * nq;
  int c_and = 0, c_r = 0, c_m = 0;
  for (int q = k * RP_THREADS + tid; q < nq; q += nblk * RP_THREADS) {
    const float4 a = a4[q], m = m4[q];
    const float av[4] = {a.x, a.y, a.z, a.w}, mv[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = av[i] > thr_r, t = mv[i] > thr_m;        // strict; false for NaN
      c_and += r & t; c_r += r; c_m += t;
    }
  }
  c_and = wave_sum(c_and); c_r = wave_sum(c_r); c_m = wave_sum(c_m);
  if ((tid & (warpSize - 1)) == 0) { atomicAdd(&s_c[0], c_and); atomicAdd(&s_c[1], c_r); atomicAdd(&s_c[2], c_m); }
  __syncthreads();
  if (tid < 4) {
    const int i = s_c[0], r = s_c[1], m = s_c[2];
    const int v = tid == 0 ? i : tid == 1 ? r + m - i : tid == 2 ? r : m;
    if (v) atomicAdd(counts + (size_t)b * 4 + tid, v);
  }
}

// counts [B][4] = {render & mask, render | mask, render, mask} pixel counts, ADDED to what counts holds; h * w % 4 == 0
static int launch_sil_compare(const float* alpha, const float* mask, int B, int h, int w, float thr_r, float thr_m, int32_t* counts, hipStream_t s) {
  const int nq = h * w / 4;
  const int per = RP_THREADS * SC_QUADS_PER_THREAD;
  const int want = (nq + per - 1) / per, nblk = want < 64 ? want : 64;
  hipLaunchKernelGGL(k_sil_compare, dim3((unsigned)(B * nblk)), dim3(RP_THREADS), 0, s, alpha, mask, nq, nblk, thr_r, thr_m, counts);
  return 0;
}

struct OverlayArgs {
  const float* alpha; const float* mask; const float* image;     // image nullable
  const float* mean; const float* stdv;                          // nullable (both or neither)
  const float* j2d; int n_sets;                                  // (n_sets, B, 17, 2)
  int B, size; float thr_r, thr_m, radius;
  uint8_t* rgb;
};

// background byte of an image value: clamp to [0, 1], scale, round half up
__device__ __forceinline__ int ov_byte(float x) { return (int)floorf(rp_mul_rn(fminf(fmaxf(x, 0.f), 1.f), 255.0f) + 0.5f); }

// grid: B * nblk workgroups; workgroup (b, k) owns quads [256 k, 256 k + 256) of pose b: a quad is four pixels of one row (size % 4 == 0)
__global__ __launch_bounds__(RP_THREADS) void k_fit_overlay(OverlayArgs a, int nblk) {
  __shared__ float s_j[OV_MAX_SETS * OV_JOINTS * 2];
  const int tid = threadIdx.x, b = (int)blockIdx.x / nblk, k = (int)blockIdx.x - b * nblk;
  const int S = a.size, qrow = S >> 2, nq = S * qrow;
  for (int i = tid; i < a.n_sets * OV_JOINTS * 2; i += RP_THREADS) {
    const int set = i / (OV_JOINTS * 2), e = i - set * (OV_JOINTS * 2);
    s_j[i] = a.j2d[((size_t)set * a.B + b) * (OV_JOINTS * 2) + e];
  }
  __syncthreads();
  const int q = k * RP_THREADS + tid;
  if (q >= nq) return;
  const int y = q / qrow, x0 = (q - y * qrow) * 4;
  const size_t pix = ((size_t)b * S + y) * S + x0;               // first of the four pixels in a (B,S,S) plane
  const float4 al = *reinterpret_cast<const float4*>(a.alpha + pix), mk = *reinterpret_cast<const float4*>(a.mask + pix);
  const float av[4] = {al.x, al.y, al.z, al.w}, mv[4] = {mk.x, mk.y, mk.z, mk.w};

  int bg[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (a.image != nullptr) {
      const float4 v4 = *reinterpret_cast<const float4*>(a.image + (((size_t)b * 3 + c) * S + y) * S + x0);
      float v[4] = {v4.x, v4.y, v4.z, v4.w};
      if (a.mean != nullptr) {
        const float sd = a.stdv[c], mu = a.mean[c];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = rp_mul_rn(v[i], sd) + mu;             // undo transforms.Normalize
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) bg[c][i] = ov_byte(v[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) bg[c][i] = 0;
    }
  }

  // joint discs: the last set that covers a pixel owns it
  int hit[4] = {-1, -1, -1, -1};
  const float r2 = a.radius * a.radius, fy = (float)y;
  for (int set = 0; set < a.n_sets; ++set)
    for (int j = 0; j < OV_JOINTS; ++j) {
      const float jx = s_j[(set * OV_JOINTS + j) * 2], jy = s_j[(set * OV_JOINTS + j) * 2 + 1];
      if (!(fabsf(jx) <= 3.0e38f) || !(fabsf(jy) <= 3.0e38f)) continue;         // NaN / infinite: draws nothing
      const float dy = fy - jy, dy2 = dy * dy;
      if (!(dy2 <= r2)) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float dx = (float)(x0 + i) - jx;
        if (dx * dx + dy2 <= r2) hit[i] = set;
      }
    }

  unsigned char o[12];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool r = av[i] > a.thr_r, m = mv[i] > a.thr_m;
    int c0 = bg[0][i], c1 = bg[1][i], c2 = bg[2][i];
    if (r || m) {             // render only: red, mask only: blue, both: green
      c0 = (c0 + ((r && !m) ? 255 : 0) + 1) >> 1;
      c1 = (c1 + ((r && m) ? 255 : 0) + 1) >> 1;
      c2 = (c2 + ((m && !r) ? 255 : 0) + 1) >> 1;
    }
    if (hit[i] == 0) { c0 = 0; c1 = 255; c2 = 0; }
    else if (hit[i] == 1) { c0 = 255; c1 = 255; c2 = 0; }
    else if (hit[i] == 2) { c0 = 255; c1 = 0; c2 = 255; }
    o[3 * i] = (unsigned char)c0; o[3 * i + 1] = (unsigned char)c1; o[3 * i + 2] = (unsigned char)c2;
  }
  unsigned* out = reinterpret_cast<unsigned*>(a.rgb + pix * 3);     // 12 bytes per quad: 4-byte aligned
#pragma unroll
  for (int d = 0; d < 3; ++d)
    out[d] = (unsigned)o[4 * d] | ((unsigned)o[4 * d + 1] << 8) | ((unsigned)o[4 * d + 2] << 16) | ((unsigned)o[4 * d + 3] << 24);
}

static int launch_fit_overlay(const float* alpha, const float* mask, const float* image, const float* mean, const float* stdv, const float* j2d,
                       int n_sets, int B, int size, float thr_r, float thr_m, float radius, uint8_t* rgb, hipStream_t s) {
  OverlayArgs a;
  a.alpha = alpha; a.mask = mask; a.image = image; a.mean = mean; a.stdv = stdv; a.j2d = j2d; a.n_sets = n_sets;
  a.B = B; a.size = size; a.thr_r = thr_r; a.thr_m = thr_m; a.radius = radius; a.rgb = rgb;
  const int nq = size * size / 4, nblk = (nq + RP_THREADS - 1) / RP_THREADS;
  hipLaunchKernelGGL(k_fit_overlay, dim3((unsigned)(B * nblk)), dim3(RP_THREADS), 0, s, a, nblk);
  return 0;
}

}  // namespace jrr

using namespace jrr;

/* the fit report: viz() of scripts/optimize.py:35-48 around the inner loop (:204-218, :268-274) */
extern "C" int jrr_silhouette_compare(const float* alpha, const float* mask, int batch, int h, int w, float thr_render, float thr_mask,
                                      int32_t* counts, void* stream) {
  if (!alpha || !mask || !counts || batch < 0 || batch > (1 << 24) || h <= 0 || w <= 0 || (long long)h * w > (1LL << 30)) {
    jrr_set_error("jrr_silhouette_compare: bad argument");
    return JRR_ERR_ARG;
  }
  if (((long long)h * w) % 4 != 0 || (((uintptr_t)alpha | (uintptr_t)mask) & 15) != 0 || ((uintptr_t)counts & 3) != 0) {
    jrr_set_error("jrr_silhouette_compare: %d x %d: h * w must be a multiple of 4 and the images 16-byte aligned", h, w);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  JRR_HIP(hipMemsetAsync(counts, 0, (size_t)batch * 4 * sizeof(int32_t), (hipStream_t)stream));
  launch_sil_compare(alpha, mask, batch, h, w, thr_render, thr_mask, counts, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_fit_overlay(const float* alpha, const float* mask, const float* image, const float* mean, const float* stdv,
                               const float* joints2d, int n_sets, int batch, int size, float thr_render, float thr_mask, float radius,
                               uint8_t* rgb, void* stream) {
  if (!alpha || !mask || !rgb || batch < 0 || batch > (1 << 24) || n_sets < 0 || n_sets > 3 || (n_sets > 0 && !joints2d) ||
      ((mean == nullptr) != (stdv == nullptr)) || (mean && !image)) {
    jrr_set_error("jrr_fit_overlay: bad argument");
    return JRR_ERR_ARG;
  }
  if (size < 4 || size > 256 || size % 4 != 0) {
    jrr_set_error("jrr_fit_overlay: size %d: a multiple of 4, at most 256", size);
    return JRR_ERR_ARG;
  }
  if ((((uintptr_t)alpha | (uintptr_t)mask | (uintptr_t)image) & 15) != 0 || ((uintptr_t)rgb & 3) != 0) {
    jrr_set_error("jrr_fit_overlay: alpha, mask and image must be 16-byte aligned, the output 4-byte aligned");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  launch_fit_overlay(alpha, mask, image, mean, stdv, joints2d, n_sets, batch, size, thr_render, thr_mask, radius, rgb, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}
