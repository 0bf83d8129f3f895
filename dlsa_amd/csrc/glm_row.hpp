// The device-side statement of the GLM families' row expressions, beside
// FamilyRules (dlsa_internal.hpp) and tests/_glm_ref.py, and the layout of the
// per-row streams (y and the row extras) in the tail of a ring slot.  Values
// in, values out; the `if (valid && lane sums)` stays at the call site.
#pragma once

#include "dlsa_internal.hpp"
#include "wave_math.hpp"

namespace dlsa {

// Behind the X pieces of a slot: y, then each row extra in bit order (EX_OFS
// the offset, EX_WGT the prior weight), each kRowStreamRows doubles, one 4-byte
// LDS-DMA load per lane and block.
constexpr int kRowStreamRows = 32;
// bytes of the slot tail of a pass with n_extras row extras (the slot sizes)
constexpr int row_streams_bytes(int n_extras) { return (1 + n_extras) * kRowStreamRows * 8; }

template <int EX>
struct RowStreams {
  static constexpr bool OFS = (EX & EX_OFS) != 0, WGT = (EX & EX_WGT) != 0;
  static constexpr int NLD = 1 + ex_count(EX);  // loads per block beside X: y and the extras
  static constexpr int OFS_OFF = row_streams_bytes(0);  // byte offsets in the tail; y at 0
  static constexpr int WGT_OFF = row_streams_bytes(OFS ? 1 : 0);
  // ys: the tail (the block's y); row: the row of the block
  static __device__ __forceinline__ double offset(const double* ys, int row) {
    return ys[OFS_OFF / 8 + row];
  }
  // The weight is read as `valid ? ys[WGT_OFF / 8 + row] : 0.0`, one line in
  // each kernel (as a function it changes the spill count of two cooperative
  // kernels): a padded row's is the next partition's, possibly NaN, and
  // 0 * NaN would reach w, r and the sums.  Its offset and y need no select:
  // they stay behind the row phase's selects on `valid`.  An unweighted kernel
  // multiplies by the constant om = 1, which folds away.
};

// The reciprocal of 1 + exp(-|eta|), kept where each was measured: the library
// division, or wv_rcp.
enum : int { RCP_DIV = 0, RCP_NEWTON = 1 };

// Logistic link at eta = e: ea = exp(-|e|), mu, w = mu (1 - mu) without
// cancellation.  (The int8 producer, irls_oz_impl.hpp, takes sqrt(w) through
// the half angle and states these lines itself; simulate_y_kernel draws y from
// 1 / (1 + exp(-eta)), which the oracle restates bit for bit.)
struct LogisticLink { double ea, mu, w; };
template <int RCP>
__device__ __forceinline__ LogisticLink logistic_link(double e) {
  const double ea = exp(-fabs(e));
  const double inv = RCP == RCP_NEWTON ? wv_rcp(1.0 + ea) : 1.0 / (1.0 + ea);
  return {ea, e >= 0.0 ? inv : ea * inv, ea * inv * inv};
}

// The mean and the variance function of a row at eta = e, for the passes that
// take both as values (the score pass, score_pass_impl.hpp): the logistic
// link above with the library division; mu = w = exp(e) for the Poisson
// family.  The caller keeps a padded row's eta out (exp of it may overflow).
struct RowMean { double mu, w; };
template <int FAM>
__device__ __forceinline__ RowMean row_mean(double e) {
  if constexpr (FAM == FAMILY_POISSON) {
    const double mu = exp(e);
    return {mu, mu};
  } else {
    const LogisticLink k = logistic_link<RCP_DIV>(e);
    return {k.mu, k.w};
  }
}

// One row's term of the evaluation passes at eta = e; lg = lgamma(y + 1) is
// computed once per row by the caller (0 for the logistic family); om the
// prior weight (the constant 1 without one).
template <int FAM>
__device__ __forceinline__ double row_loglik(double e, double yv, double om, double lg) {
  if constexpr (FAM == FAMILY_POISSON)
    return om * (yv * e - exp(e) - lg);
  else
    return om * (yv * e - (fmax(e, 0.0) + log1p(exp(-fabs(e)))));
}

// One row's terms of the goodness-of-fit passes at eta = e: its deviance and
// its Pearson chi-square.  What depends on y alone is computed once per row
// by the caller, rc = row_gof_const(y): the Poisson family's log y (0 at
// y = 0, where the deviance is 2 omega mu), the logistic family's saturated
// term y log y + (1 - y) log(1 - y) with 0 log 0 = 0 (0 for 0/1 data, whose
// deviance is -2 omega l).  y is taken as given (the logistic family's in
// [0, 1], a grouped row's s / m with omega = m); outside it the terms are NaN.
struct RowGof { double dev, chi; };
template <int FAM>
__device__ __forceinline__ double row_gof_const(double yv) {
  if constexpr (FAM == FAMILY_POISSON)
    return yv == 0.0 ? 0.0 : log(yv);
  else
    return (yv == 0.0 ? 0.0 : yv * log(yv)) + (yv == 1.0 ? 0.0 : (1.0 - yv) * log1p(-yv));
}
// Poisson: d = 2 omega (y (log y - eta) - (y - mu)), chi = omega (y - mu)^2 / mu,
// formed as r (r / mu) with r = y - mu: r^2 alone overflows from eta = 355.
// Logistic: d = 2 omega (rc - (y eta - softplus(eta))), and with ea = exp(-|eta|)
// (y - mu)^2 / (mu (1 - mu)) = t^2 / ea, t = a + b ea, (a, b) = (y - 1, y) at
// eta >= 0 and (y, y - 1) below: 1 - mu is never formed.
//
// At saturation chi takes its limit, never 0 / 0 or inf / inf.  Logistic: a
// matched row (a = 0: y = 1 at eta >= 0, y = 0 below, so b = +-1) has t = +-ea
// and t / ea = +-1 exactly: chi = omega ea, without the cancellation of y (1 +
// ea) - 1 (digits lost from |eta| = 16, all of them from 37 on); once ea has
// underflowed to 0 (|eta| > 745.13) t = 0, which is selected to chi = 0 (and is
// 0 as well where a grouped y equals mu).  Any other row is t (t / ea), +inf
// once ea = 0; t^2 itself would underflow from |eta| = 373.  Poisson: y = 0 is
// omega mu (0 once mu has underflowed), mu = +inf (eta > 709.78) is +inf, y > 0
// over an underflowed mu is +inf.  The deviance needs no such care: its terms
// are sums, and it is +inf where mu is.
template <int FAM>
__device__ __forceinline__ RowGof row_gof(double e, double yv, double om, double rc) {
  if constexpr (FAM == FAMILY_POISSON) {
    const double mu = exp(e), r = yv - mu;
    const double chi = (yv == 0.0 || mu == HUGE_VAL) ? mu : r * (r / mu);
    return {2.0 * om * (yv * (rc - e) - r), om * chi};
  } else {
    const double ea = exp(-fabs(e));
    const double a = e >= 0.0 ? yv - 1.0 : yv, b = e >= 0.0 ? yv : yv - 1.0;
    const double t = fma(b, ea, a);
    const double chi = t == 0.0 ? 0.0 : t * (t / ea);
    return {2.0 * om * (rc - (yv * e - (fmax(e, 0.0) + log1p(ea)))), om * chi};
  }
}

}  // namespace dlsa
