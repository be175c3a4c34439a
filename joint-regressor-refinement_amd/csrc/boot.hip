// Paired bootstrap intervals of the evaluation report (`--eval_ci`): how sure the arrow of `before -> after` is.  Two launches, no
// engine, no body model; integers only behind the fp32 errors, so every word is a function of the inputs alone.
//
// k_paired_units     one pose per thread.  The four (batch,17) error arrays jrr_evaluate_joints wrote for the two regressors become four
//                    int64 sums S_c = sum_j rn(e_j * 2^24) (fixedpt.h: the expression of k_eval_accumulate) which are ADDED, with a 1, to
//                    the row of the pose's resampling unit (a video sequence, or the frame itself) by int64 atomics; the pose also
//                    counts as better / worse / tie in its group's row by INTEGER comparison of its after and before sums.  A pose that
//                    is bad for one regressor is out for both: the analysis is paired.
// k_bootstrap_sums   one wave per (replicate r, segment s).  A segment is a run [begin, begin + count) of unit rows (all units, or one
//                    group's); replicate r of it is the sum of count rows drawn with replacement.  Draw i is word i & 3 of
//                    Philox4x32-10 at counter (i >> 2, r, s, 0): lane l takes the Philox blocks l, l + 64, ..., four draws from one
//                    ten-round call, and keeps five private int64 sums; ONE xor tree over the 64 lanes; lane 0 stores the row.  Integer
//                    addition is associative, so the row does not depend on which lane took which block, on the grid, on rep_begin or
//                    on rep_count.  No atomics, no zeroing: every output word is stored exactly once.
//                    A draw is a 40-byte gather at a random row.  10^5 units are 4 MB -- one XCD's L2 -- so most gathers should be
//                    served there; the rest of the time is Philox: 40 32-bit multiplies (quarter rate) per four draws.
#include "jrr_common.h"
#include "fixedpt.h"
#include "acctab.h"
#include "../../include/jrr.h"

namespace jrr {

static_assert(JRR_BOOT_UNIT_ROW == 5 && JRR_BOOT_UNIT_COUNT == 4 && JRR_BOOT_WINS_ROW == 8 && JRR_BOOT_WINS_TRAILER == 3 &&
              JRR_BOOT_WINS_TRAILER_IGNORED == JRR_EVAL_ACC_TRAILER_IGNORED && JRR_BOOT_WINS_TRAILER_BAD_GROUP == JRR_EVAL_ACC_TRAILER_BAD_GROUP,
              "row layouts; the trailer of acctab.h and a third word");

constexpr int PU_THREADS = 64;

__global__ __launch_bounds__(PU_THREADS) void k_paired_units(const float* __restrict__ before, const float* __restrict__ before_pa,
                                                             const float* __restrict__ after, const float* __restrict__ after_pa,
                                                             const int* __restrict__ group, const int* __restrict__ unit, int n_groups,
                                                             int n_units, long long* __restrict__ units, long long* __restrict__ wins, int B) {
  const int b = blockIdx.x * PU_THREADS + threadIdx.x;
  if (b >= B) return;
  const int g = group[b];
  if (long long* t = acc_refused(wins, JRR_BOOT_WINS_ROW, n_groups, g)) { acc_add(t, 1); return; }
  const int u = unit[b];
  if (u < 0 || u >= n_units) { acc_add(acc_trailer(wins, JRR_BOOT_WINS_ROW, n_groups) + JRR_BOOT_WINS_TRAILER_BAD_UNIT, 1); return; }
  long long* wrow = acc_row(wins, JRR_BOOT_WINS_ROW, g);
  const float* src[4] = {before + (size_t)b * NH, before_pa + (size_t)b * NH, after + (size_t)b * NH, after_pa + (size_t)b * NH};
  long long S[4];
  bool good = true;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    long long s = 0;
    for (int i = 0; i < NH; ++i) {
      const float e = src[c][i];
      good = good && (e < ERR_CAP);                  // false for NaN
      s += err_fixed24(e);
    }
    S[c] = s;
  }
  if (!good) { acc_add(wrow + JRR_BOOT_WINS_BAD, 1); return; }
  long long* urow = acc_row(units, JRR_BOOT_UNIT_ROW, u);
  acc_add(urow + JRR_BOOT_UNIT_BEFORE, S[0]);
  acc_add(urow + JRR_BOOT_UNIT_BEFORE_PA, S[1]);
  acc_add(urow + JRR_BOOT_UNIT_AFTER, S[2]);
  acc_add(urow + JRR_BOOT_UNIT_AFTER_PA, S[3]);
  acc_add(urow + JRR_BOOT_UNIT_COUNT, 1);
  acc_add(wrow + JRR_BOOT_WINS_COUNT, 1);
  acc_add(wrow + (S[2] < S[0] ? JRR_BOOT_WINS_BETTER : (S[2] > S[0] ? JRR_BOOT_WINS_WORSE : JRR_BOOT_WINS_TIE)), 1);
  acc_add(wrow + (S[3] < S[1] ? JRR_BOOT_WINS_BETTER_PA : (S[3] > S[1] ? JRR_BOOT_WINS_WORSE_PA : JRR_BOOT_WINS_TIE_PA)), 1);
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC11): c <- ten rounds of c under key k
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = lo1;
    c[2] = n2;
    c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

constexpr int BS_THREADS = 256, BS_WAVES = BS_THREADS / 64;

// grid: ceil(pairs / 4) workgroups of 4 waves; wave w of the launch owns pair w = s * rep_count + (r - rep_begin): row w of out.
// jrr_bootstrap_sums has checked every segment against n_units and uploaded the checked words itself, so begin + draw < n_units.
__global__ __launch_bounds__(BS_THREADS) void k_bootstrap_sums(const long long* __restrict__ units, const int* __restrict__ segments,
                                                               unsigned key0, unsigned key1, int rep_begin, int rep_count, long long pairs,
                                                               long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long p = (long long)blockIdx.x * BS_WAVES + wave;
  if (p >= pairs) return;                            // the whole wave
  const int s = (int)(p / rep_count);
  const unsigned r = (unsigned)rep_begin + (unsigned)(p - (long long)s * rep_count);
  const int begin = segments[2 * s];
  const unsigned count = (unsigned)segments[2 * s + 1];
  const unsigned n_blocks = (count + 3u) >> 2;
  long long acc[JRR_BOOT_UNIT_ROW] = {0, 0, 0, 0, 0};
  for (unsigned blk = (unsigned)lane; blk < n_blocks; blk += 64u) {
    unsigned c[4] = {blk, r, (unsigned)s, 0u};
    philox4x32_10(c, key0, key1);
    const unsigned left = count - 4u * blk;          // >= 1: draws of this block that exist
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if ((unsigned)k < left) {
        const long long* row = units + ((size_t)begin + __umulhi(c[k], count)) * JRR_BOOT_UNIT_ROW;
#pragma unroll
        for (int q = 0; q < JRR_BOOT_UNIT_ROW; ++q) acc[q] += row[q];
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int q = 0; q < JRR_BOOT_UNIT_ROW; ++q) acc[q] += __shfl_xor(acc[q], o);
  }
  if (lane == 0) {
    long long* dst = out + (size_t)p * JRR_BOOT_UNIT_ROW;
#pragma unroll
    for (int q = 0; q < JRR_BOOT_UNIT_ROW; ++q) dst[q] = acc[q];
  }
}

}  // namespace jrr

using namespace jrr;

extern "C" int jrr_paired_units(const float* before, const float* before_pa, const float* after, const float* after_pa, const int32_t* group,
                                const int32_t* unit, int batch, int n_groups, int n_units, int64_t* units, int64_t* wins, void* stream) {
  if (!before || !before_pa || !after || !after_pa || !group || !unit || !units || !wins || batch < 0 ||
      !acc_aligned(units, wins)) {
    jrr_set_error("jrr_paired_units: bad argument");
    return JRR_ERR_ARG;
  }
  if (!acc_groups_ok(n_groups) || n_units < 1) {
    jrr_set_error("jrr_paired_units: n_groups %d: 1 .. %d, n_units %d: at least 1", n_groups, (int)JRR_EVAL_ACC_MAX_GROUPS, n_units);
    return JRR_ERR_ARG;
  }
  if (batch == 0) return JRR_OK;
  hipLaunchKernelGGL(k_paired_units, dim3((unsigned)((batch + PU_THREADS - 1) / PU_THREADS)), dim3(PU_THREADS), 0, (hipStream_t)stream, before,
                     before_pa, after, after_pa, group, unit, n_groups, n_units, reinterpret_cast<long long*>(units),
                     reinterpret_cast<long long*>(wins), batch);
  CHECK_LAUNCH();
  return JRR_OK;
}

extern "C" int jrr_bootstrap_sums(const int64_t* units, int n_units, const int32_t* segments_host, int32_t* segments, int n_seg,
                                  uint64_t seed, int rep_begin, int rep_count, int64_t* out, void* stream) {
  if (!units || !segments || !segments_host || !out || n_units < 0 || n_seg < 1 || n_seg > JRR_BOOT_MAX_SEGMENTS || rep_begin < 0 ||
      rep_count < 0 || (long long)rep_begin + rep_count > 0x7fffffffLL || (((uintptr_t)units | (uintptr_t)out) & 7) != 0 ||
      ((uintptr_t)segments & 3) != 0) {
    jrr_set_error("jrr_bootstrap_sums: bad argument (1 <= n_seg <= %d, replicates below 2^31, 8-byte aligned tables)", (int)JRR_BOOT_MAX_SEGMENTS);
    return JRR_ERR_ARG;
  }
  for (int s = 0; s < n_seg; ++s) {
    const long long begin = segments_host[2 * s], count = segments_host[2 * s + 1];
    if (count < 0) {
      jrr_set_error("jrr_bootstrap_sums: segment %d has the negative count %lld", s, count);
      return JRR_ERR_SEGMENT;
    }
    if (begin < 0 || begin + count > (long long)n_units) {
      jrr_set_error("jrr_bootstrap_sums: segment %d = [%lld, %lld) lies outside the table of %d units", s, begin, begin + count, n_units);
      return JRR_ERR_SEGMENT;
    }
  }
  const long long pairs = (long long)n_seg * rep_count;
  if (pairs == 0) return JRR_OK;
  const long long blocks = (pairs + BS_WAVES - 1) / BS_WAVES;
  if (blocks > 0x7fffffffLL) {
    jrr_set_error("jrr_bootstrap_sums: %lld (segment, replicate) pairs in one call; split the replicates", pairs);
    return JRR_ERR_ARG;
  }
  // the kernel reads the words that were checked above: the device copy is made here, from them
  JRR_HIP(hipMemcpyAsync(segments, segments_host, (size_t)n_seg * 2 * sizeof(int32_t), hipMemcpyHostToDevice, (hipStream_t)stream));
  hipLaunchKernelGGL(k_bootstrap_sums, dim3((unsigned)blocks), dim3(BS_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(units),
                     segments, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), rep_begin, rep_count, pairs,
                     reinterpret_cast<long long*>(out));
  CHECK_LAUNCH();
  return JRR_OK;
}
