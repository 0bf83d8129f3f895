// Step control of the per-partition Newton update, shared by the two solve
// kernels (newton_solve.hip: P <= 192 and the categorical path;
// wide_newton.hip: P <= 512).  Each kernel assembles H, g and the
// log-likelihood, publishes Sig_inv, and factors and solves in its own LDS
// layout; the state machine around those stages is here, once:
//   step_prelude   non-finite log-likelihood, step halving on a decrease;
//   factor_failed  a pivot that is not positive and finite;
//   step_update    theta += d, convergence / phase switch / stall escalation.
// Device code only.  NTHR = threads of the partition's workgroup.
#pragma once

#include <math.h>

#include "dlsa_internal.hpp"

namespace dlsa {

// Broadcast lane `l` (wave-uniform) of a double with two v_readlane: no LDS
// round trip (ds_bpermute) on the dependency chains of the small
// factorizations and solves.
__device__ __forceinline__ double bcast_f64(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// Stall detection of the approximate phases.  With an approximate Hessian H~
// and the exact gradient, Newton contracts at rate ~ ||I - H~^-1 H|| (about
// kappa 2^-8 for bf16): on an ill-conditioned design that rate nears 1 and
// the fit would crawl to max_iter.  Far from the MLE (Newton's damped phase)
// steps of similar size are normal whatever the Hessian precision, so
// evidence is only taken once the log-likelihood has gone quiet (the last
// step gained at most kStallDll (1 + |ll|)): there an approximate iteration
// "stalls" when its max |step| did not at least halve against the previous
// one, or when it backtracks; two stalls in a row move the partition one
// precision up (F32 -> escalate_to, F32X -> F64).  Returns the phase to
// continue in.
constexpr double kStallDll = 1e-5;
__device__ __forceinline__ int32_t escalate_phase(const SolveArgs& a, int32_t ph) {
  return ph == PHASE_F32 ? a.escalate_to : PHASE_F64;
}
__device__ __forceinline__ int32_t approx_stall_step(const SolveArgs& a, int k, int32_t ph,
                                                     bool stalled) {
  const int st = stalled ? a.stall[k] + 1 : 0;
  if (st >= 2) {
    a.stall[k] = 0;
    a.dm_prev[k] = 0.0;
    return escalate_phase(a, ph);
  }
  a.stall[k] = st;
  return ph;
}
// Approximate-phase iteration with a step of max |d| = dm (not yet below
// switch_tol): log-likelihood ll at the pass's point, llp at the previous one.
__device__ __forceinline__ int32_t approx_next_phase(const SolveArgs& a, int k, int32_t ph,
                                                     double dm, double ll, double llp) {
  if (!(ll - llp <= kStallDll * (1.0 + fabs(ll)))) {  // damped phase (or first iteration)
    a.stall[k] = 0;
    a.dm_prev[k] = 0.0;
    return ph;
  }
  const double dp = a.dm_prev[k];
  const int32_t nph = approx_stall_step(a, k, ph, dp > 0.0 && dm > 0.5 * dp);
  if (nph == ph) a.dm_prev[k] = dm;
  return nph;
}
// A backtracking approximate iteration: a stall only once the fit was quiet.
__device__ __forceinline__ int32_t approx_backtrack_phase(const SolveArgs& a, int k, int32_t ph) {
  return a.dm_prev[k] > 0.0 ? approx_stall_step(a, k, ph, true) : ph;
}

// A warm-start level that fails (separation, too few rows) only restarts the
// partition from theta = 0 on the next level (level_reset_kernel rewrites
// ll_prev and backtracks before that level reads them); a Poisson partition
// restarts from its start point (a.theta0: log mean y on the intercept).
template <int NTHR>
__device__ __forceinline__ void level_fail(const SolveArgs& a, int k, int it) {
  double* th = a.theta + (int64_t)k * a.P;
  for (int f = threadIdx.x; f < a.P; f += NTHR) th[f] = (f == 0 && a.theta0) ? a.theta0[k] : 0.0;
  if (threadIdx.x == 0) {
    a.phase[k] = PHASE_LEVEL_DONE;
    a.iters[k] = it + 1;
  }
}

// Given the pass's summed log-likelihood ll (llp: the previous point's):
// false when the iteration ends here (block-uniform).
//  - ll not finite: the level fails, or the partition ends NONFINITE --
//    except for Poisson after a step (it > 0, a previous point of this level
//    on record, backtracks < 40): there exp(eta) overflowed, an overshoot
//    like any other, and the previous step is halved;
//  - ll fell: halve the previous step (the role of sklearn's line search).
//    The threshold is above the fp32-log noise of mixed-mode
//    log-likelihoods; real overshoots of a Newton step lose far more than
//    1e-6 relative.
template <int NTHR>
__device__ __forceinline__ bool step_prelude(const SolveArgs& a, int k, int phase, int it,
                                             double ll, double llp) {
  const int tid = threadIdx.x, P = a.P;
  const bool can_halve = !a.eval_only && it > 0 && a.backtracks[k] < 40;
  const bool overshoot =  // Poisson: a non-finite ll after a step (llp: this level's last point)
      a.family == FAMILY_POISSON && !isfinite(ll) && can_halve && isfinite(llp);
  if (!isfinite(ll) && !overshoot) {
    if (a.subsample)
      level_fail<NTHR>(a, k, it);
    else if (tid == 0)
      a.status[k] = DLSA_STATUS_NONFINITE;
    return false;
  }
  if (overshoot || (can_halve && a.family != FAMILY_GAUSSIAN &&
                    ll < llp - 1e-6 * (1.0 + fabs(llp)))) {
    const int bt = a.backtracks[k] + 1;
    const double sc = ldexp(1.0, -bt);
    double* th = a.theta + (int64_t)k * P;
    const double* tp = a.theta_prev + (int64_t)k * P;
    const double* dp = a.delta_prev + (int64_t)k * P;
    for (int f = tid; f < P; f += NTHR) th[f] = tp[f] + sc * dp[f];
    if (tid == 0) {
      a.backtracks[k] = bt;
      a.iters[k] = it + 1;
      int ph = phase;
      if (!a.subsample && ph != PHASE_F64) {  // an approximate step that overshot
        ph = approx_backtrack_phase(a, k, ph);
        a.phase[k] = ph;
      }
      atomicAdd(&a.counters[ph], 1);
    }
    return false;
  }
  return true;
}

// The factorisation met a pivot that is not positive and finite: the level
// fails; a low-precision Hessian that lost definiteness has this point redone
// one precision up (bf16 -> fp32 -> fp64); an exact one is SINGULAR.
template <int NTHR>
__device__ __forceinline__ void factor_failed(const SolveArgs& a, int k, int phase, int it) {
  if (a.subsample) {
    level_fail<NTHR>(a, k, it);
    return;
  }
  if (threadIdx.x != 0) return;
  if (phase != PHASE_F64 && a.family != FAMILY_GAUSSIAN) {
    const int32_t ph = escalate_phase(a, phase);
    a.phase[k] = ph;
    a.iters[k] = it + 1;
    a.stall[k] = 0;
    a.dm_prev[k] = 0.0;
    atomicAdd(&a.counters[ph], 1);
  } else {
    a.status[k] = DLSA_STATUS_SINGULAR;
  }
}

// Update and convergence, given the solved step z[] and the gradient g[] in
// LDS (complete: a barrier lies behind their last write) and red, 3 NTHR / 64
// doubles of LDS nobody reads any more.  One block reduction of
// (max |d|, max |theta|, theta . g): xor butterfly inside the wave, then the
// waves in index order -- max |d| by every thread (the non-finite exits are
// block-uniform), the other two by thread 0, which writes the decision
// (all threads combining all three measured slower in the wide kernel).
// NEAR: count in counters[3] the PHASE_F32 partitions whose
// step is below kOzNearTol (the fused fit's Ozaki digit-scale record).
template <int NTHR, bool NEAR>
__device__ __forceinline__ void step_update(const SolveArgs& a, int k, int phase, int it,
                                            double ll, double llp, const double* z,
                                            const double* g, double* red) {
  constexpr int NW = NTHR / 64;
  const int tid = threadIdx.x, P = a.P;
  double* th = a.theta + (int64_t)k * P;
  double* tp = a.theta_prev + (int64_t)k * P;
  double* dp = a.delta_prev + (int64_t)k * P;
  double dm = 0.0, tm = 0.0, tg = 0.0;
  for (int f = tid; f < P; f += NTHR) {
    const double d = z[f];
    const double t0 = th[f];
    const double t1 = t0 + d;
    tp[f] = t0;
    dp[f] = d;
    th[f] = t1;
    dm = fmax(dm, fabs(d));
    tm = fmax(tm, fabs(t1));
    tg += t1 * g[f];
  }
  for (int o = 32; o > 0; o >>= 1) {
    dm = fmax(dm, __shfl_xor(dm, o));
    tm = fmax(tm, __shfl_xor(tm, o));
    tg += __shfl_xor(tg, o);
  }
  if ((tid & 63) == 0) {
    red[tid >> 6] = dm;
    red[NW + (tid >> 6)] = tm;
    red[2 * NW + (tid >> 6)] = tg;
  }
  __syncthreads();
  dm = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) dm = fmax(dm, red[w]);
  const bool finite = isfinite(dm);  // block-uniform
  if (!finite && !a.subsample) {
    // keep the last finite iterate (each thread restores the entries it
    // wrote): the status reports the failure and the combine step excludes
    // the partition
    for (int f = tid; f < P; f += NTHR) th[f] = tp[f];
  }
  if (!finite && a.subsample && a.family != FAMILY_GAUSSIAN) {
    level_fail<NTHR>(a, k, it);
    return;
  }
  if (tid != 0) return;
  tm = red[NW];
  tg = red[2 * NW];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    tm = fmax(tm, red[NW + w]);
    tg += red[2 * NW + w];
  }
  a.iters[k] = it + 1;
  if (a.family == FAMILY_GAUSSIAN) {
    // OLS: theta was 0, one Newton step is the closed form (X^T X)^-1 X^T y;
    // residual sum of squares = y^T y - theta^T X^T y = -2 ll(0) - theta . g
    a.loglik[k] = -2.0 * ll - tg;
    a.status[k] = finite ? DLSA_STATUS_OK : DLSA_STATUS_NONFINITE;
    a.phase[k] = PHASE_DONE;
    return;
  }
  a.ll_prev[k] = ll;
  a.backtracks[k] = 0;
  if (a.subsample) {
    if (dm <= a.level_tol * (1.0 + tm))
      a.phase[k] = PHASE_LEVEL_DONE;
    else
      atomicAdd(&a.counters[phase], 1);
    return;
  }
  if (!finite) {
    a.status[k] = DLSA_STATUS_NONFINITE;
    return;
  }
  int ph = phase;
  if (ph != PHASE_F64) {
    if (dm <= a.switch_tol * (1.0 + tm)) {
      ph = PHASE_F64;
    } else {
      ph = approx_next_phase(a, k, ph, dm, ll, llp);
      // near the switch: the next bf16 pass records the Ozaki digit scales
      if (NEAR && ph == PHASE_F32 && dm <= kOzNearTol * (1.0 + tm)) atomicAdd(&a.counters[3], 1);
    }
  } else if (dm <= a.tol * (1.0 + tm)) {
    a.status[k] = DLSA_STATUS_OK;
    a.phase[k] = PHASE_DONE;
    return;
  }
  a.phase[k] = ph;
  atomicAdd(&a.counters[ph], 1);
}

}  // namespace dlsa
