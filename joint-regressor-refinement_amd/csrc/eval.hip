// MPJPE / Procrustes-aligned MPJPE on device:
//   evaluate                                   /root/reference/scripts/utils.py:117-145
//   batch_compute_similarity_transform_torch   /root/reference/scripts/eval_utils.py:7-58
// One pose per thread; the body is evalk.h's, shared with the per-joint kernel of evalrep.hip.
#include "jrr_common.h"
#include "evalk.h"

namespace jrr {

__global__ __launch_bounds__(64) void k_evaluate(const float* __restrict__ pred, const float* __restrict__ target_mm, float* __restrict__ err,
                           float* __restrict__ err_pa, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
#define JRR_EVAL_PLAIN_BEGIN float e = 0.f;
#define JRR_EVAL_PLAIN(i, d) e += d;
#define JRR_EVAL_PLAIN_END err[b] = e / NH;
#define JRR_EVAL_PA_BEGIN float epa = 0.f;
#define JRR_EVAL_PA(i, d) epa += d;
#define JRR_EVAL_PA_END err_pa[b] = epa / NH;
#define JRR_EVAL_BODY
#include "evalk.h"
#undef JRR_EVAL_BODY
#undef JRR_EVAL_PLAIN_BEGIN
#undef JRR_EVAL_PLAIN
#undef JRR_EVAL_PLAIN_END
#undef JRR_EVAL_PA_BEGIN
#undef JRR_EVAL_PA
#undef JRR_EVAL_PA_END
}

}  // namespace jrr

using namespace jrr;

extern "C" int jrr_evaluate(const float* pred, const float* target_mm, float* err, float* err_pa, int batch, void* stream) {
  if (!pred || !target_mm || !err || !err_pa || batch <= 0) return JRR_ERR_ARG;
  hipLaunchKernelGGL(k_evaluate, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream, pred, target_mm, err, err_pa, batch);
  CHECK_LAUNCH();
  return JRR_OK;
}
