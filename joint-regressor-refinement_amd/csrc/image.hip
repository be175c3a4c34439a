// The image half of the dataset on device:
//   find_crop                         /root/reference/scripts/data.py:220-271  (similarity warp, theta = 0, through
//                                     scripts/sampling_helper.py:15-69 and grid_sample: bilinear, zero padding, align_corners=False)
//   mask_rcnn / 255, valid, corner    /root/reference/scripts/data.py:121,130-132
//   transforms.Normalize              /root/reference/scripts/optimize.py:141-142,164
//
// k_image_crop: uint8 HWC pixels in, float32 CHW crops out, one or two crop sizes from one launch.  Without rotation the warp is
// separable: output row i reads source rows y0(i), y0(i) + 1 and output column j reads source columns x0(j), x0(j) + 1.  A
// workgroup owns (sample, crop size, band of IC_ROWS output rows): it brings the column span of the 2 IC_ROWS source rows into LDS
// with 16-byte loads of the interleaved bytes, takes the four taps of every output value from LDS and stores float4 along the
// output row (a wave writes up to 1 KiB contiguous per instruction).  The position arithmetic repeats data.py's axis_taps() of the
// host side operation by operation, each one rounded once (mul_rn() keeps a product from being fused into the addition that follows), so that
// host and kernel agree on every tap index: the host uploads only the block of each frame that its crops can touch.
#include "jrr_common.h"

namespace jrr {

constexpr int IC_MAX_SIZE = 256;       // largest crop (pixels per side; sizes are multiples of 4)
constexpr int IC_MAX_ROI_W = 1024;     // widest block of a frame a sample may hand over (pixels; frames are cut to 1000 x 1000)
constexpr int IC_ROWS = 4;                        // output rows per workgroup
constexpr int IC_SLOTS = 2 * IC_ROWS;             // staged source rows
constexpr int IC_ROWBYTES = 3 * IC_MAX_ROI_W + 32;  // a span of IC_MAX_ROI_W pixels starting anywhere in a 16-byte chunk, rounded up to chunks
constexpr int IC_CHUNKS = IC_ROWBYTES / 16;
constexpr int IC_THREADS = 256;
static_assert(IC_ROWBYTES % 16 == 0, "whole 16-byte chunks");

#pragma clang fp contract(off)

struct Tap { int i0; float w0, w1; };

// a product that is rounded BEFORE it meets an addition: the empty asm keeps the compiler from fusing the two into one fma
__device__ __forceinline__ float mul_rn(float a, float b) {
  float p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}

// linspace(-1, 1, n)[i], torch's scalar formula (data.py linspace_pm1)
__device__ __forceinline__ float lin_pm1(int i, int n) {
  const float step = 2.f / (float)(n - 1);
  return i < n / 2 ? -1.f + mul_rn(step, (float)i) : 1.f - mul_rn(step, (float)(n - 1 - i));
}

// data.py axis_taps(): the taps i0, i0 + 1 of output index i along an axis of `extent` pixels; s = scale, t = s * (centre / s)
__device__ __forceinline__ Tap axis_tap(float s, float t, int i, int n, int extent) {
  const float g = mul_rn(s, lin_pm1(i, n)) + t;
  const float pos = (mul_rn(g + 1.f, (float)extent) - 1.f) / 2.f;
  Tap r;
  if (!(fabsf(pos) <= 3.0e38f)) { r.i0 = -2; r.w0 = 0.f; r.w1 = 0.f; return r; }     // NaN / infinite: the reference zeroes the crop
  const float f = floorf(pos);
  r.w1 = pos - f;
  r.w0 = (f + 1.f) - pos;
  r.i0 = (int)fminf(fmaxf(f, -2.f), (float)extent);
  if (r.i0 < 0 || r.i0 >= extent) r.w0 = 0.f;
  if (r.i0 + 1 < 0 || r.i0 + 1 >= extent) r.w1 = 0.f;
  return r;
}

__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }   // torch.maximum

struct ImageCropArgs {
  const uint8_t* pix; long long pix_bytes;
  const long long* desc;      // [B][8] {byte offset, row pitch, roi_y0, roi_x0, roi_h, roi_w, frame_H, frame_W}
  const float* bbox;          // [B][4] (min_y, min_x, max_y, max_x), 1000-unit convention
  const float* mean; const float* stdv;    // [3] each or NULL: (x - mean) / std on the first size
  float* out0; float* out1; int n0, n1;    // n1 = 0: one size
  int* status;
};

__global__ __launch_bounds__(IC_THREADS) void k_image_crop(ImageCropArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_rows[IC_SLOTS][IC_ROWBYTES];
  __shared__ float s_tab[256];                                   // value of a byte: p / 255, a true division
  __shared__ int s_cx[IC_MAX_SIZE];
  __shared__ float s_cw0[IC_MAX_SIZE], s_cw1[IC_MAX_SIZE];
  __shared__ int s_shift[IC_SLOTS];                              // byte of column `cl` inside a staged row; -1: the row is not in the block
  __shared__ long long s_src[IC_SLOTS];                          // first (16-byte aligned) byte of the staged row in the buffer
  __shared__ int s_nchunk[IC_SLOTS];

  const int tid = threadIdx.x, b = blockIdx.y;
  const int nb0 = a.n0 / IC_ROWS;
  const bool second = (int)blockIdx.x >= nb0;
  const int N = second ? a.n1 : a.n0;
  const int row0 = ((int)blockIdx.x - (second ? nb0 : 0)) * IC_ROWS;
  float* out = second ? a.out1 : a.out0;
  const bool norm = !second && a.mean != nullptr;
  int err = 0;

  // ---- the sample: descriptor (checked against the buffer before anything is read through it) and crop geometry ----
  const long long* d = a.desc + (size_t)b * 8;
  const long long off = d[0], pitch = d[1];
  long long ry0 = d[2], rx0 = d[3], rh = d[4], rw = d[5];
  const long long FH = d[6], FW = d[7];
  bool ok = off >= 0 && pitch >= 0 && ry0 >= 0 && rx0 >= 0 && rh >= 0 && rw >= 0 && FH > 0 && FW > 0 && FH <= (1 << 20) && FW <= (1 << 20) &&
            rw <= IC_MAX_ROI_W && ry0 + rh <= FH && rx0 + rw <= FW && off <= a.pix_bytes && pitch <= a.pix_bytes;
  if (ok && rh > 0 && rw > 0) ok = (rh == 1 || 3 * rw <= pitch) && off + (rh - 1) * pitch + 3 * rw <= a.pix_bytes;
  if (!ok) { err |= 2; rh = 0; rw = 0; }
  const int H = ok ? (int)FH : 1, W = ok ? (int)FW : 1;
  const int y_lo = (int)ry0, y_hi = (int)(ry0 + rh), x_lo = (int)rx0, x_hi = (int)(rx0 + rw);     // the block [y_lo, y_hi) x [x_lo, x_hi)

  const float* bb = a.bbox + (size_t)b * 4;
  const float mnx = (bb[1] - 500.f) / 500.f, mxx = (bb[3] - 500.f) / 500.f;
  const float mny = (bb[0] - 500.f) / 500.f, mxy = (bb[2] - 500.f) / 500.f;
  const float ax = (mnx + mxx) / 2.f, ay = (mny + mxy) / 2.f;
  const float s = max_nan(mxx - mnx, mxy - mny) / 2.f;
  const float tx = mul_rn(s, ax / s), ty = mul_rn(s, ay / s);

  // columns the band can touch, cut to the block: [cl, ch]
  const int xa = axis_tap(s, tx, 0, N, W).i0, xb = axis_tap(s, tx, N - 1, N, W).i0;
  const int cl = max(min(xa, xb), x_lo), ch = min(max(xa, xb) + 1, x_hi - 1);

  s_tab[tid] = (float)tid / 255.f;
  if (tid < N) {
    const Tap t = axis_tap(s, tx, tid, N, W);
    s_cx[tid] = t.i0; s_cw0[tid] = t.w0; s_cw1[tid] = t.w1;
  }
  if (tid < IC_SLOTS) {
    const int y = axis_tap(s, ty, row0 + (tid >> 1), N, H).i0 + (tid & 1);
    int shift = -1, nchunk = 0;
    long long src = 0;
    if (y >= y_lo && y < y_hi && ch >= cl) {
      const long long first = off + (long long)(y - y_lo) * pitch + 3LL * (cl - x_lo), last = first + 3LL * (ch - cl + 1);
      src = first & ~15LL;                                   // >= 0; src + 16 nchunk <= pix_bytes rounded up to 16 = pix_bytes
      shift = (int)(first - src);
      nchunk = (int)((last - src + 15) >> 4);                // <= IC_CHUNKS: the span is at most IC_MAX_ROI_W pixels
    }
    s_shift[tid] = shift; s_src[tid] = src; s_nchunk[tid] = nchunk;
  }
  __syncthreads();

  // ---- stage the source rows: 16 bytes per lane, consecutive lanes consecutive chunks ----
  for (int idx = tid; idx < IC_SLOTS * IC_CHUNKS; idx += IC_THREADS) {
    const int q = idx / IC_CHUNKS, c = idx - q * IC_CHUNKS;
    if (c < s_nchunk[q])
      *reinterpret_cast<uint4*>(&s_rows[q][16 * c]) = *reinterpret_cast<const uint4*>(a.pix + s_src[q] + 16LL * c);
  }
  __syncthreads();

  // ---- four output columns of one (row, channel) per task ----
  const int nq = N >> 2;
  for (int t = tid; t < IC_ROWS * 3 * nq; t += IC_THREADS) {
    const int r = t / (3 * nq), rem = t - r * 3 * nq, c = rem / nq, j4 = (rem - c * nq) * 4;
    const Tap ty_ = axis_tap(s, ty, row0 + r, N, H);
    const int sh0 = s_shift[2 * r], sh1 = s_shift[2 * r + 1];
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x0 = s_cx[j4 + k];
      const float wx0 = s_cw0[j4 + k], wx1 = s_cw1[j4 + k];
      const bool in0 = x0 >= cl && x0 <= ch, in1 = x0 + 1 >= cl && x0 + 1 <= ch;
      const int o0 = 3 * (x0 - cl) + c, o1 = o0 + 3;
      const float nw = mul_rn(ty_.w0, wx0), ne = mul_rn(ty_.w0, wx1), sw = mul_rn(ty_.w1, wx0), se = mul_rn(ty_.w1, wx1);
      // a tap of non-zero weight that the block does not hold: read nothing, tell the caller
      if ((nw != 0.f && !(in0 && sh0 >= 0)) || (ne != 0.f && !(in1 && sh0 >= 0)) || (sw != 0.f && !(in0 && sh1 >= 0)) ||
          (se != 0.f && !(in1 && sh1 >= 0)))
        err |= 1;
      const float p00 = (in0 && sh0 >= 0) ? s_tab[s_rows[2 * r][sh0 + o0]] : 0.f;
      const float p01 = (in1 && sh0 >= 0) ? s_tab[s_rows[2 * r][sh0 + o1]] : 0.f;
      const float p10 = (in0 && sh1 >= 0) ? s_tab[s_rows[2 * r + 1][sh1 + o0]] : 0.f;
      const float p11 = (in1 && sh1 >= 0) ? s_tab[s_rows[2 * r + 1][sh1 + o1]] : 0.f;
      float acc = mul_rn(p00, nw) + mul_rn(p01, ne);          // grid_sample's order: nw, ne, sw, se
      acc = acc + mul_rn(p10, sw);
      acc = acc + mul_rn(p11, se);
      if (norm) acc = (acc - a.mean[c]) / a.stdv[c];
      v[k] = acc;
    }
    float4 o; o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
    *reinterpret_cast<float4*>(out + (((size_t)b * 3 + c) * N + row0 + r) * N + j4) = o;
  }
  if (err) atomicOr(a.status, err);
}

// status bits of k_image_crop (ORed into *status, never cleared by the kernel): 1 = a tap of non-zero weight inside the frame but
// outside the sample's block (nothing is read there), 2 = a descriptor that does not fit the pixel buffer (the sample reads nothing)
// desc [B][8] = {byte offset, row pitch, roi_y0, roi_x0, roi_h, roi_w, frame_H, frame_W}; pix 16-byte aligned, pix_bytes % 16 == 0
static int launch_image_crop(const uint8_t* pix, size_t pix_bytes, const int64_t* desc, const float* bbox, int B, const float* mean,
                      const float* stdv, int n0, float* out0, int n1, float* out1, int* status, hipStream_t s) {
  ImageCropArgs a;
  a.pix = pix; a.pix_bytes = (long long)pix_bytes; a.desc = reinterpret_cast<const long long*>(desc); a.bbox = bbox;
  a.mean = mean; a.stdv = stdv; a.out0 = out0; a.out1 = out1; a.n0 = n0; a.n1 = n1; a.status = status;
  hipLaunchKernelGGL(k_image_crop, dim3((n0 + n1) / IC_ROWS, B), dim3(IC_THREADS), 0, s, a);
  return 0;
}

// mask_rcnn = mask / 255 as (B,1,h,w), valid[b] = mask[b,0,0] != 0 read BEFORE the 2 x 2 corner is zeroed (data.py:121,130-132)
__global__ __launch_bounds__(256) void k_mask_prepare(const uint8_t* __restrict__ in, float* __restrict__ out, int* __restrict__ valid, int B,
                                                      int h, int w) {
  const size_t per = (size_t)h * w, total = per * B;
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= total) return;
  uint8_t p[4];
  if (i + 4 <= total) {
    const uchar4 q = *reinterpret_cast<const uchar4*>(in + i);
    p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w;
  } else {
    for (int k = 0; k < 4; ++k) p[k] = i + k < total ? in[i + k] : 0;
  }
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const size_t e = i + k, bi = e / per, rem = e - bi * per;
    const int y = (int)(rem / w), x = (int)(rem - (size_t)y * w);
    if (rem == 0 && e < total) valid[bi] = p[k] != 0;
    v[k] = (y < 2 && x < 2) ? 0.f : (float)p[k] / 255.f;
  }
  if (i + 4 <= total) {
    float4 o; o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
    *reinterpret_cast<float4*>(out + i) = o;
  } else {
    for (int k = 0; k < 4 && i + k < total; ++k) out[i + k] = v[k];
  }
}

}  // namespace jrr

using namespace jrr;

/* find_crop on uint8 frames (scripts/data.py:220-271) and the mask preparation (scripts/data.py:121,130-132) */
extern "C" int jrr_image_crop(const uint8_t* pix, size_t pix_bytes, const int64_t* desc, const float* bboxes, int batch, const float* mean,
                              const float* stdv, int size0, float* out0, int size1, float* out1, int32_t* status, void* stream) {
  if (!pix || !desc || !bboxes || !out0 || !status || batch < 0 || batch > 65535 || (size1 != 0 && !out1) || ((mean == nullptr) != (stdv == nullptr))) {
    jrr_set_error("jrr_image_crop: bad argument");
    return JRR_ERR_ARG;
  }
  auto bad_size = [](int n) { return n < 4 || n > IC_MAX_SIZE || n % 4 != 0; };
  if (bad_size(size0) || (size1 != 0 && bad_size(size1))) {
    jrr_set_error("jrr_image_crop: crop sizes %d, %d: one or two sizes, multiples of 4, at most %d", size0, size1, IC_MAX_SIZE);
    return JRR_ERR_ARG;
  }
  if (((uintptr_t)pix & 15) != 0 || pix_bytes % 16 != 0 || pix_bytes == 0) {
    jrr_set_error("jrr_image_crop: the pixel buffer must be 16-byte aligned and a non-zero multiple of 16 bytes long");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  launch_image_crop(pix, pix_bytes, desc, bboxes, batch, mean, stdv, size0, out0, size1, out1, status, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_mask_prepare(const uint8_t* masks, int batch, int h, int w, float* out, int32_t* valid, void* stream) {
  if (!masks || !out || !valid || batch < 0 || h <= 0 || w <= 0 || (((uintptr_t)masks | (uintptr_t)out) & 15) != 0) {
    jrr_set_error("jrr_mask_prepare: bad argument");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  const size_t total = (size_t)batch * h * w;
  hipLaunchKernelGGL(k_mask_prepare, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, masks, out, valid, batch, h, w);
  CHECK_LAUNCH();
  return JRR_OK;
}
