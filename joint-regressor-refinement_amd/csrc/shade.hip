// The fit report's picture of the BODY (`--fit_report_mesh`): per-vertex normals and a shaded view of the mesh the rasteriser resolved.
// The reference had pytorch3d for this (a MeshRenderer with a Phong shader is what every SMPL fitting tool shows); the arithmetic here is
// the part of it a viewer needs: Meshes.verts_normals_packed, barycentric interpolation with clip_barycentric_coordinates at
// perspective_correct = False (pytorch3d 0.3.0's default), one directional light, two-sided.
//
// k_vertex_normals: one thread per (pose, vertex).  The faces of the vertex come from a CSR adjacency (ascending face index), their
//   unnormalised cross products are summed IN THAT ORDER -- no float atomics, the result is a function of the list alone -- and the sum
//   is divided by max(|sum|, 1e-6).  No valence limit: the loop runs over the vertex's whole list.  Per pose 82.7 KB of vertices are
//   gathered from L2 about 6 x 9 floats per vertex and 82.7 KB are written; memory-bound and tiny.
// k_mesh_shade: one thread assembles four pixels of a row, as k_fit_overlay does: a 16-byte load of pix_to_face and of the three image
//   planes, 12 output bytes as three dword stores, the optional depth (one float4) and normal (three float4) maps.  A covered pixel
//   gathers its face's 3 indices, 9 vertex and 9 normal floats.  ~7 % of the pixels of a 224 x 224 body are covered, in one cluster.
// Every operation is stated in include/jrr.h and rounded once, in the order written (no product is fused into a sum), so a host
// restatement follows it.  Every index read from device memory -- adjacency offsets, face indices, vertex indices, pix_to_face -- is
// checked against its array before it is used: nothing is read outside the arrays whatever the data.
#include "jrr_common.h"

namespace jrr {

constexpr int SH_THREADS = 256;
constexpr float SH_FINITE = 3.402823466e+38f;   // FLT_MAX: |x| <= SH_FINITE: neither NaN nor infinite

#pragma clang fp contract(off)

__device__ __forceinline__ bool sh_finite(float x) { return fabsf(x) <= SH_FINITE; }

// grid: ceil(B * V / 256) workgroups; thread i owns vertex i % V of pose i / V
__global__ __launch_bounds__(SH_THREADS) void k_vertex_normals(const float* __restrict__ verts, const int* __restrict__ faces,
                                                               const int* __restrict__ adj_offset, const int* __restrict__ adj_face,
                                                               float* __restrict__ normals, int B, int V, int F) {
  const long long idx = (long long)blockIdx.x * SH_THREADS + threadIdx.x;
  if (idx >= (long long)B * V) return;
  const int b = (int)(idx / V), v = (int)(idx - (long long)b * V);
  const float* p = verts + (size_t)b * V * 3;
  int beg = adj_offset[v], end = adj_offset[v + 1];
  beg = beg < 0 ? 0 : beg;
  end = end > 3 * F ? 3 * F : end;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int k = beg; k < end; ++k) {
    const int f = adj_face[k];
    if (f < 0 || f >= F) continue;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
    const float ax = p[3 * i0], ay = p[3 * i0 + 1], az = p[3 * i0 + 2];
    const float e1x = p[3 * i1] - ax, e1y = p[3 * i1 + 1] - ay, e1z = p[3 * i1 + 2] - az;
    const float e2x = p[3 * i2] - ax, e2y = p[3 * i2 + 1] - ay, e2z = p[3 * i2 + 2] - az;
    sx += e1y * e2z - e1z * e2y;
    sy += e1z * e2x - e1x * e2z;
    sz += e1x * e2y - e1y * e2x;
  }
  const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
  const float d = len < 1e-6f ? 1e-6f : len;                    // torch's clamp(min = 1e-6): a NaN stays a NaN (fmaxf would drop it)
  float* o = normals + (size_t)idx * 3;
  o[0] = sx / d; o[1] = sy / d; o[2] = sz / d;
}

struct ShadeArgs {
  const float* verts; const float* normals; const int* faces; const float* cam; const int* p2f;
  const float* image; const float* mean; const float* stdv;      // nullable; mean and stdv both or neither
  int B, V, F, size;
  float colour[3], opacity, ambient, light[3], background;
  uint8_t* rgb; float* depth; float* normal; int* status;        // depth, normal, status nullable
};

__device__ __forceinline__ float sh_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ int sh_byte(float x01) { return (int)floorf(x01 * 255.0f + 0.5f); }
// (p - a) x (b - a)
__device__ __forceinline__ float sh_edge(float px, float py, float ax, float ay, float bx, float by) {
  return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// grid: B * nblk workgroups; workgroup (b, k) owns quads [256 k, 256 k + 256) of pose b: a quad is four pixels of one row (size % 4 == 0)
__global__ __launch_bounds__(SH_THREADS) void k_mesh_shade(ShadeArgs a, int nblk) {
  const int tid = threadIdx.x, b = (int)blockIdx.x / nblk, k = (int)blockIdx.x - b * nblk;
  const int S = a.size, qrow = S >> 2, nq = S * qrow;
  const int q = k * SH_THREADS + tid;
  if (q >= nq) return;
  const int y = q / qrow, x0 = (q - y * qrow) * 4;
  const size_t pix = ((size_t)b * S + y) * S + x0;               // first of the four pixels in a (B,S,S) plane
  const int4 f4 = *reinterpret_cast<const int4*>(a.p2f + pix);
  const int fv[4] = {f4.x, f4.y, f4.z, f4.w};

  float bg[3][4];                                                // background value in [0, 1]
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (a.image != nullptr) {
      const float4 v4 = *reinterpret_cast<const float4*>(a.image + (((size_t)b * 3 + c) * S + y) * S + x0);
      float v[4] = {v4.x, v4.y, v4.z, v4.w};
      if (a.mean != nullptr) {
        const float sd = a.stdv[c], mu = a.mean[c];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = v[i] * sd + mu;       // undo transforms.Normalize (contraction is off: product rounded first)
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) bg[c][i] = sh_clamp01(v[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) bg[c][i] = sh_clamp01(a.background);
    }
  }

  const float fS = (float)S, foc = 5000.f / fS;
  const float py = 1.f - (float)(2 * y + 1) / fS;
  const float cx = a.cam[(size_t)b * 3], cy = a.cam[(size_t)b * 3 + 1], cz = a.cam[(size_t)b * 3 + 2];
  const float* vb = a.verts + (size_t)b * a.V * 3;
  const float* nb = a.normals + (size_t)b * a.V * 3;
  const float om_amb = 1.f - a.ambient, om_op = 1.f - a.opacity;

  unsigned char o[12];
  float dep[4], nrm[4][3];
  int bits = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int f = fv[i];
    float col[3] = {bg[0][i], bg[1][i], bg[2][i]};
    dep[i] = -1.f; nrm[i][0] = nrm[i][1] = nrm[i][2] = 0.f;
    if (f >= 0) {
      int i0 = 0, i1 = 0, i2 = 0;
      bool ok = f < a.F;
      if (ok) {
        i0 = a.faces[3 * f]; i1 = a.faces[3 * f + 1]; i2 = a.faces[3 * f + 2];
        ok = (unsigned)i0 < (unsigned)a.V && (unsigned)i1 < (unsigned)a.V && (unsigned)i2 < (unsigned)a.V;
      }
      if (!ok) bits |= 1;
      else {
        const int iv[3] = {i0, i1, i2};
        float pu[3], pv[3], Z[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const float* p = vb + 3 * iv[t];
          const float X = -2.f * p[0] + cx, Y = -2.f * p[1] + cy;
          Z[t] = 2.f * p[2] + cz;
          pu[t] = foc * X / Z[t]; pv[t] = foc * Y / Z[t];
        }
        const float area = sh_edge(pu[2], pv[2], pu[0], pv[0], pu[1], pv[1]);
        const bool fin = sh_finite(pu[0]) && sh_finite(pu[1]) && sh_finite(pu[2]) && sh_finite(pv[0]) && sh_finite(pv[1]) && sh_finite(pv[2]) &&
                         sh_finite(Z[0]) && sh_finite(Z[1]) && sh_finite(Z[2]);
        if (!fin || !(fabsf(area) > 1e-8f)) bits |= 2;
        else {
          const float px = 1.f - (float)(2 * (x0 + i) + 1) / fS;
          float w0 = fmaxf(sh_edge(px, py, pu[1], pv[1], pu[2], pv[2]) / area, 0.f);
          float w1 = fmaxf(sh_edge(px, py, pu[2], pv[2], pu[0], pv[0]) / area, 0.f);
          float w2 = fmaxf(sh_edge(px, py, pu[0], pv[0], pu[1], pv[1]) / area, 0.f);
          const float ws = fmaxf((w0 + w1) + w2, 1e-5f);
          w0 = w0 / ws; w1 = w1 / ws; w2 = w2 / ws;
          dep[i] = (w0 * Z[0] + w1 * Z[1]) + w2 * Z[2];
          const float* n0 = nb + 3 * i0; const float* n1 = nb + 3 * i1; const float* n2 = nb + 3 * i2;
          const float mx = (w0 * n0[0] + w1 * n1[0]) + w2 * n2[0];
          const float my = (w0 * n0[1] + w1 * n1[1]) + w2 * n2[1];
          const float mz = (w0 * n0[2] + w1 * n1[2]) + w2 * n2[2];
          float nx = -mx, ny = -my, nz = mz;                        // model -> view space: the projection's x / y flip
          const float len = fmaxf(sqrtf((nx * nx + ny * ny) + nz * nz), 1e-6f);
          nx = nx / len; ny = ny / len; nz = nz / len;
          nrm[i][0] = nx; nrm[i][1] = ny; nrm[i][2] = nz;
          const float I = a.ambient + om_amb * fabsf((nx * a.light[0] + ny * a.light[1]) + nz * a.light[2]);
#pragma unroll
          for (int c = 0; c < 3; ++c) col[c] = sh_clamp01((a.opacity * a.colour[c]) * I + om_op * bg[c][i]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[3 * i + c] = (unsigned char)sh_byte(col[c]);
  }
  unsigned* out = reinterpret_cast<unsigned*>(a.rgb + pix * 3);     // 12 bytes per quad: 4-byte aligned
#pragma unroll
  for (int d = 0; d < 3; ++d)
    out[d] = (unsigned)o[4 * d] | ((unsigned)o[4 * d + 1] << 8) | ((unsigned)o[4 * d + 2] << 16) | ((unsigned)o[4 * d + 3] << 24);
  if (a.depth != nullptr) *reinterpret_cast<float4*>(a.depth + pix) = make_float4(dep[0], dep[1], dep[2], dep[3]);
  if (a.normal != nullptr) {
    float4* n4 = reinterpret_cast<float4*>(a.normal + pix * 3);     // 48 bytes per quad: 16-byte aligned
    n4[0] = make_float4(nrm[0][0], nrm[0][1], nrm[0][2], nrm[1][0]);
    n4[1] = make_float4(nrm[1][1], nrm[1][2], nrm[2][0], nrm[2][1]);
    n4[2] = make_float4(nrm[2][2], nrm[3][0], nrm[3][1], nrm[3][2]);
  }
  if (bits != 0 && a.status != nullptr) atomicOr(a.status, bits);
}

static int launch_mesh_shade(const float* verts, const float* normals, const int32_t* faces, const float* cam, const int32_t* p2f, const float* image,
                      const float* mean, const float* stdv, int B, int V, int F, int size, const float* colour, float opacity, float ambient,
                      const float* light, float background, uint8_t* rgb, float* depth, float* normal, int32_t* status, hipStream_t s) {
  ShadeArgs a;
  a.verts = verts; a.normals = normals; a.faces = faces; a.cam = cam; a.p2f = p2f; a.image = image; a.mean = mean; a.stdv = stdv;
  a.B = B; a.V = V; a.F = F; a.size = size; a.opacity = opacity; a.ambient = ambient; a.background = background;
  for (int c = 0; c < 3; ++c) { a.colour[c] = colour[c]; a.light[c] = light[c]; }
  a.rgb = rgb; a.depth = depth; a.normal = normal; a.status = status;
  const int nq = size * size / 4, nblk = (nq + SH_THREADS - 1) / SH_THREADS;
  hipLaunchKernelGGL(k_mesh_shade, dim3((unsigned)(B * nblk)), dim3(SH_THREADS), 0, s, a, nblk);
  return 0;
}

}  // namespace jrr

using namespace jrr;

/* the fit report's shaded views (--fit_report_mesh): no engine, no body model */
extern "C" int jrr_vertex_normals(const float* verts, const int32_t* faces, const int32_t* adj_offset, const int32_t* adj_face, int batch,
                                  int n_verts, int n_faces, float* normals, void* stream) {
  if (!verts || !faces || !adj_offset || !adj_face || !normals || batch < 0 || n_verts < 1 || n_faces < 1 || n_faces > (1 << 28) ||
      (long long)batch * n_verts > (1LL << 30)) {
    jrr_set_error("jrr_vertex_normals: bad argument");
    return JRR_ERR_ARG;
  }
  if ((((uintptr_t)verts | (uintptr_t)faces | (uintptr_t)adj_offset | (uintptr_t)adj_face | (uintptr_t)normals) & 3) != 0) {
    jrr_set_error("jrr_vertex_normals: every array must be 4-byte aligned");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  const long long n = (long long)batch * n_verts;
  hipLaunchKernelGGL(k_vertex_normals, dim3((unsigned)((n + SH_THREADS - 1) / SH_THREADS)), dim3(SH_THREADS), 0, (hipStream_t)stream, verts, faces,
                     adj_offset, adj_face, normals, batch, n_verts, n_faces);
  CHECK_LAUNCH();
  return JRR_OK;
}
extern "C" int jrr_mesh_shade(const float* verts, const float* normals, const int32_t* faces, const float* cam, const int32_t* pix_to_face,
                              const float* image, const float* mean, const float* stdv, int batch, int n_verts, int n_faces, int size,
                              const float* colour_host, float opacity, float ambient, const float* light_host, float background,
                              uint8_t* rgb, float* depth, float* normal, int32_t* status, void* stream) {
  if (!verts || !normals || !faces || !cam || !pix_to_face || !colour_host || !light_host || !rgb || batch < 0 || batch > (1 << 24) ||
      n_verts < 1 || n_faces < 1 || n_faces > (1 << 28) || (long long)batch * n_verts > (1LL << 30) ||
      ((mean == nullptr) != (stdv == nullptr)) || (mean && !image)) {
    jrr_set_error("jrr_mesh_shade: bad argument");
    return JRR_ERR_ARG;
  }
  if (size < 4 || size > 256 || size % 4 != 0) {
    jrr_set_error("jrr_mesh_shade: size %d: a multiple of 4, at most 256", size);
    return JRR_ERR_ARG;
  }
  if ((((uintptr_t)pix_to_face | (uintptr_t)image | (uintptr_t)depth | (uintptr_t)normal) & 15) != 0 ||
      (((uintptr_t)verts | (uintptr_t)normals | (uintptr_t)faces | (uintptr_t)cam | (uintptr_t)rgb | (uintptr_t)status) & 3) != 0) {
    jrr_set_error("jrr_mesh_shade: pix_to_face, image, depth and normal must be 16-byte aligned, everything else 4-byte aligned");
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  launch_mesh_shade(verts, normals, faces, cam, pix_to_face, image, mean, stdv, batch, n_verts, n_faces, size, colour_host, opacity, ambient,
                    light_host, background, rgb, depth, normal, status, (hipStream_t)stream);
  CHECK_LAUNCH();
  return JRR_OK;
}
