// The fixed-point form of a per-joint error in the int64 report tables: rn(e * 2^24), units of 2^-24 m.  k_eval_accumulate
// (evalrep.hip, JRR_EVAL_ACC_SUM*) and k_paired_units (boot.hip, JRR_BOOT_UNIT_*) both call this one function, so a group's SUM words
// and the column sums of its bootstrap units are the same integers.  e * 2^24 is exact in fp32 (a power of two; e < 1.0e3f keeps it
// below 2^34), the rounding to an integer is to nearest, ties to even.
#pragma once
#include <hip/hip_runtime.h>

namespace jrr {

constexpr float ERR_CAP = 1.0e3f;                  // a value that fails e < ERR_CAP (NaN, inf, absurd) makes its pose bad

__device__ __forceinline__ long long err_fixed24(float e) { return __float2ll_rn(e * 16777216.f); }

}  // namespace jrr
