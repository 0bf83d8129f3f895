// Lane and arithmetic helpers of the pass kernels (gfx950 / CDNA4): the
// cross-lane sums of a 64-lane wave and the short fp64 sequences of the row phases.
#pragma once

#include "dlsa_internal.hpp"

namespace dlsa {

// Lane l and lane l ^ 16 (permlane16_swap), l and l ^ 32 (permlane32_swap):
// both operands are v, so the swapped pair (x, y) holds the two halves and
// x + y is the same sum, bitwise, in both lanes of the pair.
__device__ __forceinline__ double wv_xor16(double v) {
  const unsigned lo = __double2loint(v), hi = __double2hiint(v);
  const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  return __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
}
__device__ __forceinline__ double wv_xor32(double v) {
  const unsigned lo = __double2loint(v), hi = __double2hiint(v);
  const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
}
// Sum over the 64 / R lanes of one row of a row phase with R rows per wave
// (lanes l, l ^ R, l ^ 2R, ...) without LDS; every lane of the row ends with
// the bitwise-identical total (each step adds a commutative pair).  The l ^ 4
// step of R = 4 is kept as each pass had it: DPP4 adds row_ror 4 after the
// l ^ 8 step (cooperative), else __shfl_xor(v, 4) goes first (per-wave).
template <int R, bool DPP4 = false>
__device__ __forceinline__ double wv_row_sum(double v) {
  static_assert(R == 16 || R == 8 || R == 4, "16, 8 or 4 rows per wave");
  if constexpr (R == 4 && !DPP4) v += __shfl_xor(v, 4);
  if constexpr (R <= 8) v += dpp_f64<0x128>(v);          // row_ror 8: l ^ 8
  if constexpr (R == 4 && DPP4) v += dpp_f64<0x124>(v);  // row_ror 4
  v = wv_xor16(v);
  v = wv_xor32(v);
  return v;
}

// Sum over each aligned group of 8 lanes, the same total in all 8
__device__ __forceinline__ double ev_red8(double v) {
  v += dpp_f64<0xB1>(v);
  v += dpp_f64<0x4E>(v);
  v += dpp_f64<0x141>(v);
  return v;
}

__device__ __forceinline__ double wave_sum64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ double bcast_first(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// 1 / d for d in [1, 3]: hardware estimate + two Newton steps (~1 ulp; the
// library division's scaling / fix-up steps are for operands this never sees)
__device__ __forceinline__ double wv_rcp(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(r, fma(-d, r, 1.0), r);
  r = fma(r, fma(-d, r, 1.0), r);
  return r;
}

// log(t) for t in [1, 2] (t = 1 + exp(-|eta|): the softplus of the
// log-likelihood).  t -> t / 2 above sqrt 2, then log t = k ln 2 + 2 atanh(s),
// s = (t - 1) / (t + 1) in [-0.172, 0.172], by the odd series to s^19
// (truncation < 1e-17 relative).  A few ulps, against ~70 instructions of the
// double-double library log1p; log1p's extra accuracy for tiny arguments is
// not needed here: the terms are summed, so the absolute error (~1e-16 per
// row) is what counts.
__device__ __forceinline__ double wv_log12(double t) {
  const bool hi = t > 1.4142135623730951;
  const double u = hi ? 0.5 * t : t;
  const double s = (u - 1.0) * wv_rcp(u + 1.0);
  const double s2 = s * s;
  double q = 1.0 / 19.0;
  q = fma(q, s2, 1.0 / 17.0);
  q = fma(q, s2, 1.0 / 15.0);
  q = fma(q, s2, 1.0 / 13.0);
  q = fma(q, s2, 1.0 / 11.0);
  q = fma(q, s2, 1.0 / 9.0);
  q = fma(q, s2, 1.0 / 7.0);
  q = fma(q, s2, 1.0 / 5.0);
  q = fma(q, s2, 1.0 / 3.0);
  const double l = fma(2.0 * s * s2, q, 2.0 * s);
  return hi ? l + 0.6931471805599453094 : l;
}

}  // namespace dlsa
