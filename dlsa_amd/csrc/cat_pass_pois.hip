// Poisson regression on the categorical-code layout: the pass and presence
// kernels without row extras, the routing over the four row-extras units, and
// the two small kernels that size the fixed-point grids on the device.
//
// The logistic grids are sized once per fit (fit_cat.hip cat_grids) from
// w <= 1/4 and |y - mu| <= 1.  Here w = mu = exp(eta) has no bound and moves
// with theta, so a grid kernel runs before every pass and bounds every row's
// eta at that pass's theta by the smaller of
//   A(theta) = [theta_0] + sum_j |theta_j| m~_j + sum_f max(0, max_l theta_fl)
//              + o_max                                            always valid;
//   M = log w'_max + [d_0] + sum_j |d_j| m~_j + sum_f max(0, max_l d_fl),
//       d = theta - theta', theta' and w'_max the point and the measured
//       largest omega mu of the partition's previous pass          valid when
//       that pass measured a finite w'_max > 0
// (m~_j bounds the standardised column j, a baseline code contributes 0, and
// in M the offset cancels: eta(theta) = eta(theta') + d . x, so omega mu moves
// by exp(d . x) row by row).  M bounds log(omega mu), the bins' own term, and
// not eta: with omega_max exp(A) it would be log mu'_max + log omega_max, but
// a heavy weight and a large mu on different rows would multiply in that
// bound (1e4 x 4e4 in tests/test_gpu_pois_cat.py::test_heavy_row_grid, 1.2e-8
// per entry of Sig_inv instead of the contract's 1e-10).  With w_hi =
// min(omega_max exp(A), exp(M)) the terms are bounded by w_hi (w, the pair
// cells), max(omega_max y_max, w_hi) (the residual) and w_hi m~_j (w x_j),
// and each grid is 2^floor(60 - log2(bound rmax)) as in cat_grids: every term
// stays below 2^50 and the factor 2 up to the rounding trick's 2^51 covers the
// rounding of eta_hi.  A bound that is not finite, or whose grid exponent is
// below -900, has no grid: hscale[0] = NaN, the pass publishes a NaN
// log-likelihood and the solve halves the step (or ends the partition
// NONFINITE where there is no step to halve); theta' and w'_max are kept for
// the retry.  Above +900 the clamped grid still keeps the terms small.
#include "cat_pois_impl.hpp"

namespace dlsa {

DLSA_CAT_POIS_UNIT(EX_NONE)

hipError_t launch_cat_pass_pois(const CatArgsPois& a, bool standardize, int n_chunks,
                                hipStream_t s) {
  switch (pass_extras(a)) {
    case EX_NONE: return launch_cat_pass_pois_unit<EX_NONE>(a, standardize, n_chunks, s);
    case EX_OFS: return launch_cat_pass_pois_unit<EX_OFS>(a, standardize, n_chunks, s);
    case EX_WGT: return launch_cat_pass_pois_unit<EX_WGT>(a, standardize, n_chunks, s);
    default: return launch_cat_pass_pois_unit<EX_OFS | EX_WGT>(a, standardize, n_chunks, s);
  }
}

hipError_t launch_cat_presence_pois(const CatArgsPois& a, int n_chunks, int32_t* counts,
                                    int32_t* bad, double* colmax, hipStream_t s) {
  switch (pass_extras(a)) {
    case EX_NONE:
      return launch_cat_presence_pois_unit<EX_NONE>(a, n_chunks, counts, bad, colmax, s);
    case EX_OFS:
      return launch_cat_presence_pois_unit<EX_OFS>(a, n_chunks, counts, bad, colmax, s);
    case EX_WGT:
      return launch_cat_presence_pois_unit<EX_WGT>(a, n_chunks, counts, bad, colmax, s);
    default:
      return launch_cat_presence_pois_unit<EX_OFS | EX_WGT>(a, n_chunks, counts, bad, colmax, s);
  }
}

// bounds[k] = {m~_0 .. m~_{q-1}, 0 .., o_max, omega_max, y_max} from the
// presence pass's per-chunk maxima: one thread per value.  A partition the
// mark kernel has ended MISSING_LEVEL after the pre-pass wrote its start point
// gets theta[k][0] = 0 back: the outputs of an ended partition are all zero.
__global__ __launch_bounds__(64) void cat_pois_bounds_kernel(const CatArgsPois a,
                                                             const int32_t* pcb,
                                                             const double* colmax,
                                                             double* bounds, double* theta,
                                                             const int32_t* status) {
  const int k = blockIdx.x, i = threadIdx.x;
  if (i == 0 && status[k] == DLSA_STATUS_MISSING_LEVEL) theta[(int64_t)k * a.P] = 0.0;
  if (i >= kCatPoisBounds) return;
  const int cb = pcb[k], ce = pcb[k + 1];
  const double* src = i < kCatQMax ? colmax + i
                      : i == kCatQMax ? a.omax : i == kCatQMax + 1 ? a.wmax : a.ymax;
  const int stride = i < kCatQMax ? kCatQMax : 1;
  double m = 0.0;  // (the maxima are >= 0)
  for (int c = cb; c < ce; ++c) m = fmax(m, src[(int64_t)c * stride]);
  if (i < kCatQMax) {
    if (i >= a.q)
      m = 0.0;
    else if (a.center)
      m = (m + fabs(a.center[i])) / fabs(a.scale[i]);  // the kernel sums w (x - c) / s
  } else if (i == kCatQMax + 1) {
    // no weights, or a partition the pre-pass has ended: omega_max = 1
    if (!a.row_weight || !(m > 0.0)) m = 1.0;
  }
  bounds[(int64_t)k * kCatPoisBounds + i] = m;
}

hipError_t launch_cat_pois_bounds(const CatArgsPois& a, const int32_t* pcb, int K,
                                  const double* colmax, double* bounds, double* theta,
                                  const int32_t* status, hipStream_t s) {
  if (K <= 0) return hipSuccess;
  static_assert(kCatPoisBounds <= 64, "one thread per bound");
  hipLaunchKernelGGL(cat_pois_bounds_kernel, dim3(K), dim3(64), 0, s, a, pcb, colmax, bounds,
                     theta, status);
  return hipGetLastError();
}

// One wave per partition.  Lane i < Qn takes parameter i of the numeric block,
// lane f < F factor f's largest level effect; the sums are butterflies in a
// fixed order, so the grids are the same bits run to run.
__global__ __launch_bounds__(64) void cat_pois_grid_kernel(const CatArgsPois a,
                                                           const double* bounds,
                                                           double* theta_snap, double* hscale,
                                                           double rmax) {
  const int k = blockIdx.x, lane = threadIdx.x;
  if (a.phase[k] != a.want_phase) return;
  const int P = a.P, ic = a.intercept, q = a.q, F = a.F;
  const double* th = a.theta + (int64_t)k * P;
  double* tp = theta_snap + (int64_t)k * P;
  const double* bd = bounds + (int64_t)k * kCatPoisBounds;
  // this lane's share of A - o_max and of M - log w'_max
  double sa = 0.0, sm = 0.0;
  if (lane < ic + q) {
    const double t = th[lane], d = t - tp[lane];
    if (lane < ic) {
      sa = t;
      sm = d;
    } else {
      const double m = bd[lane - ic];
      sa = fabs(t) * m;
      sm = fabs(d) * m;
    }
  }
  static_assert(kCatMaxFactors + kCatQMax <= 64, "a lane per numeric parameter and per factor");
  if (lane >= kCatQMax && lane - kCatQMax < F) {
    const int f = lane - kCatQMax;
    double ma = 0.0, mm = 0.0;  // the baseline level's 0
    for (int l = 0; l < a.nlev[f]; ++l) {
      const double t = th[a.doff[f] + l];
      ma = fmax(ma, t);
      mm = fmax(mm, t - tp[a.doff[f] + l]);
    }
    sa = ma;
    sm = mm;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    sa += __shfl_xor(sa, o);
    sm += __shfl_xor(sm, o);
  }
  const unsigned long long mb = a.mumax[k];
  const double om = bd[kCatQMax + 1], ym = bd[kCatQMax + 2];
  double w_hi = om * exp(sa + bd[kCatQMax]);  // omega_max exp(A)
  if (mb > 0ull && mb < 0x7FF0000000000000ull)
    w_hi = fmin(w_hi, exp(log(__longlong_as_double((long long)mb)) + sm));
  // lane 0: w and the pair cells, lane 1: the residual, lane 2 + j: w x_j
  double bound = w_hi;
  if (lane == 1) bound = fmax(om * ym, w_hi);
  if (lane >= 2 && lane < kCatQMax + 2) bound *= lane - 2 < q ? bd[lane - 2] : 0.0;
  bool ok = true;
  double grid = 1.0;
  if (lane < kCatQMax + 2) {
    ok = isfinite(bound * rmax);
    if (ok && bound > 0.0) {
      const int e = (int)floor(60.0 - log2(bound * rmax));
      ok = e >= -900;
      grid = ldexp(1.0, min(900, e));
    }
  }
  ok = __all(ok);
  const double no_grid = __longlong_as_double(0x7FF8000000000000ll);  // a quiet NaN
  if (lane < kCatQMax + 2)
    hscale[(int64_t)k * (kCatQMax + 2) + lane] = (!ok && lane == 0) ? no_grid : grid;
  if (!ok) return;  // theta' and w'_max stay those of the last measured pass
  for (int i = lane; i < P; i += 64) tp[i] = th[i];
  if (lane == 0) a.mumax[k] = 0ull;
}

hipError_t launch_cat_pois_grid(const CatArgsPois& a, int K, const double* bounds,
                                double* theta_snap, double* hscale, double rmax, hipStream_t s) {
  if (K <= 0) return hipSuccess;
  hipLaunchKernelGGL(cat_pois_grid_kernel, dim3(K), dim3(64), 0, s, a, bounds, theta_snap, hscale,
                     rmax);
  return hipGetLastError();
}

}  // namespace dlsa
