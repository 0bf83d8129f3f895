// Small kernels around the fused pass: fit state init/finalise, the local
// partition reduction (dlsa/dlsa.py:30-34 group-sum, done in HBM before the
// RCCL all-reduce) and the synthetic data generator.
#include <math.h>

#include "dlsa_internal.hpp"

namespace dlsa {

__global__ void fit_init_kernel(const int64_t* offsets, int K, int P, int start_phase,
                                double* theta, int32_t* phase, int32_t* backtracks,
                                int32_t* iters, int32_t* status, double* ll_prev,
                                double* sig_inv, double* loglik) {
  const int k = blockIdx.x;
  const bool empty = offsets[k + 1] <= offsets[k];
  for (int f = threadIdx.x; f < P; f += blockDim.x) theta[(int64_t)k * P + f] = 0.0;
  for (int e = threadIdx.x; e < P * P; e += blockDim.x) sig_inv[(int64_t)k * P * P + e] = 0.0;
  if (threadIdx.x == 0) {
    phase[k] = empty ? PHASE_DONE : start_phase;
    backtracks[k] = 0;
    iters[k] = 0;
    status[k] = empty ? DLSA_STATUS_EMPTY : STATUS_RUNNING;
    ll_prev[k] = -INFINITY;
    loglik[k] = 0.0;
  }
}

hipError_t launch_fit_init(const int64_t* offsets_dev, int K, int P, int start_phase,
                           double* theta, int32_t* phase, int32_t* backtracks, int32_t* iters,
                           int32_t* status, double* ll_prev, double* sig_inv, double* loglik,
                           hipStream_t s) {
  hipLaunchKernelGGL(fit_init_kernel, dim3(K), dim3(256), 0, s, offsets_dev, K, P, start_phase,
                     theta, phase, backtracks, iters, status, ll_prev, sig_inv, loglik);
  return hipGetLastError();
}

// Start of a warm-start level: running partitions re-enter the Newton loop
// (the log-likelihood scale changes with the row count), non-finite iterates
// restart from 0; counters[phase] = partitions running.
// theta0 (Poisson, else null): the restart value of parameter 0.
__global__ void level_reset_kernel(int K, int P, int start_phase, int32_t* phase,
                                   int32_t* status, double* ll_prev, int32_t* backtracks,
                                   double* theta, int32_t* counters, const double* theta0) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < K; k += gridDim.x * blockDim.x) {
    if (status[k] != STATUS_RUNNING) continue;
    bool finite = true;
    for (int f = 0; f < P; ++f) finite &= (bool)isfinite(theta[(int64_t)k * P + f]);
    if (!finite) {
      for (int f = 0; f < P; ++f) theta[(int64_t)k * P + f] = 0.0;
      if (theta0) theta[(int64_t)k * P] = theta0[k];
    }
    phase[k] = start_phase;
    ll_prev[k] = -INFINITY;
    backtracks[k] = 0;
    atomicAdd(&counters[start_phase], 1);
  }
}

hipError_t launch_level_reset(int K, int P, int start_phase, int32_t* phase, int32_t* status,
                              double* ll_prev, int32_t* backtracks, double* theta,
                              int32_t* counters, hipStream_t s, const double* theta0) {
  hipLaunchKernelGGL(level_reset_kernel, dim3((K + 255) / 256), dim3(256), 0, s, K, P,
                     start_phase, phase, status, ll_prev, backtracks, theta, counters, theta0);
  return hipGetLastError();
}

// What the pre-pass makes of a non-empty partition's sums: the status that
// ends it, or STATUS_RUNNING.  bad: a non-finite y, o or omega; mn: min over y
// and omega; sw = sum omega, swy = sum omega y, swe = sum omega exp(o) (sum
// omega without an offset; swy = swe = 0 for a family without a device start).
//   NONFINITE  a bad or negative entry, or a sum that is not finite
//   SINGULAR   sum omega = 0, or (Poisson) sum omega y = 0: no MLE
//   NONFINITE  (Poisson) sum omega exp(o) = 0 or a quotient that is not
//              finite: no finite start
// A partition with sum omega y = 0 and sum omega exp(o) = 0 (every exp(o)
// underflowed) meets both of the last two: the weighted entries report it
// SINGULAR, the unweighted ones NONFINITE, a documented difference between
// them that callers may rely on.
__device__ __forceinline__ int prepass_status(bool poisson, bool weighted, int bad, double mn,
                                              double sw, double swy, double swe) {
  if (bad || !(mn >= 0.0) || !isfinite(sw) || !isfinite(swy) || !isfinite(swe))
    return DLSA_STATUS_NONFINITE;
  const bool singular = !(sw > 0.0) || (poisson && !(swy > 0.0));
  const bool no_start = poisson && (!(swe > 0.0) || !isfinite(swy / swe));
  if (singular && no_start) return weighted ? DLSA_STATUS_SINGULAR : DLSA_STATUS_NONFINITE;
  return singular ? DLSA_STATUS_SINGULAR : no_start ? DLSA_STATUS_NONFINITE : STATUS_RUNNING;
}

// Pre-pass of a fit whose family starts from a device-computed point or that
// carries prior weights, after fit_init: one workgroup per partition sums
// omega, omega y and omega exp(o) in a fixed order (thread t takes rows t,
// t + 256, ...; xor butterfly inside the wave, then the four waves in index
// order: the same bits run to run) and takes min(y, omega) and a finiteness
// flag along.  eta_offset and row_weight may be null (wave-uniform): without
// weights omega is the literal 1, so omega y = y and omega exp(o) = exp(o)
// exactly; without an offset no exp is evaluated and sum omega exp(o) is sum
// omega (unweighted: the row count, which the fixed-order sum of ones gives
// exactly).  A partition that prepass_status ends gets that status and
// PHASE_DONE before any pass, with the zeroed outputs fit_init wrote;
// nothing per row is stored.
//   POISSON: with an intercept the fit starts at theta = (log(sum omega y /
//   sum omega exp(o)), 0, ..., 0), the MLE of the intercept-only (rate)
//   model: from theta = 0 a Newton step at mean y ~ 50 overshoots to eta ~
//   50.  Without an intercept the start stays theta = 0.  theta0[k] keeps the
//   start value of parameter 0 for the restarts (level_fail,
//   level_reset_kernel).
//   Otherwise (logistic, weighted): statuses only; y, eta_offset, theta and
//   theta0 are not touched and the start stays theta = 0.
template <bool POISSON>
__global__ __launch_bounds__(256) void fit_prepass_kernel(
    const double* y, const double* eta_offset, const double* row_weight, const int64_t* offsets,
    int P, int intercept, double* theta, double* theta0, int32_t* phase, int32_t* status) {
  __shared__ double ssw[4], sswy[4], sswe[4], smin[4];
  __shared__ int sbad[4];
  const int k = blockIdx.x;
  const int64_t r0 = offsets[k], r1 = offsets[k + 1];
  double sw = 0.0, swy = 0.0, swe = 0.0, mn = INFINITY;
  int bad = 0;
  for (int64_t i = r0 + threadIdx.x; i < r1; i += 256) {
    const double om = row_weight ? row_weight[i] : 1.0;
    bad |= !isfinite(om);
    sw += om;
    mn = fmin(mn, om);
    if constexpr (POISSON) {
      const double v = y[i];
      bad |= !isfinite(v);
      mn = fmin(mn, v);
      swy += om * v;
      if (eta_offset) {
        const double o = eta_offset[i];
        bad |= !isfinite(o);
        swe += om * exp(o);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sw += __shfl_xor(sw, o);
    swy += __shfl_xor(swy, o);
    swe += __shfl_xor(swe, o);
    mn = fmin(mn, __shfl_xor(mn, o));
    bad |= __shfl_xor(bad, o);
  }
  if ((threadIdx.x & 63) == 0) {
    ssw[threadIdx.x >> 6] = sw;
    sswy[threadIdx.x >> 6] = swy;
    sswe[threadIdx.x >> 6] = swe;
    smin[threadIdx.x >> 6] = mn;
    sbad[threadIdx.x >> 6] = bad;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  sw = ((ssw[0] + ssw[1]) + ssw[2]) + ssw[3];
  swy = ((sswy[0] + sswy[1]) + sswy[2]) + sswy[3];
  swe = ((sswe[0] + sswe[1]) + sswe[2]) + sswe[3];
  mn = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
  bad = sbad[0] | sbad[1] | sbad[2] | sbad[3];
  if constexpr (POISSON) {
    theta0[k] = 0.0;
    if (!eta_offset) swe = sw;
  }
  if (r1 <= r0) return;  // empty: fit_init's DLSA_STATUS_EMPTY stands
  const int st = prepass_status(POISSON, row_weight != nullptr, bad, mn, sw, swy, swe);
  if (st != STATUS_RUNNING) {
    status[k] = st;
    phase[k] = PHASE_DONE;
  } else if (POISSON && intercept) {
    const double t0 = log(swy / swe);
    theta0[k] = t0;
    theta[(int64_t)k * P] = t0;
  }
}

hipError_t launch_fit_prepass(int family, const double* y, const double* eta_offset,
                              const double* row_weight, const int64_t* offsets_dev, int K, int P,
                              int intercept, double* theta, double* theta0, int32_t* phase,
                              int32_t* status, hipStream_t s) {
  const bool start = family_rules(family).device_start;
  if (K <= 0 || (!start && !row_weight)) return hipSuccess;
  if (start)
    hipLaunchKernelGGL(fit_prepass_kernel<true>, dim3(K), dim3(256), 0, s, y, eta_offset,
                       row_weight, offsets_dev, P, intercept, theta, theta0, phase, status);
  else  // the weight check alone
    hipLaunchKernelGGL(fit_prepass_kernel<false>, dim3(K), dim3(256), 0, s, nullptr, nullptr,
                       row_weight, offsets_dev, 0, 0, nullptr, nullptr, phase, status);
  return hipGetLastError();
}

// Polish pass of a budget that ran out: every still-running partition gets
// one exact pass at the theta it returns, whose X^T W X is published as
// Sig_inv -- models.py:114,130 evaluate the weights at whatever coef sklearn
// stopped at.  counters[PHASE_F64] = partitions marked.
__global__ void polish_mark_kernel(int K, int32_t* phase, const int32_t* status,
                                   int32_t* counters) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < K; k += gridDim.x * blockDim.x) {
    if (status[k] != STATUS_RUNNING) continue;
    phase[k] = PHASE_F64;
    atomicAdd(&counters[PHASE_F64], 1);
  }
}

hipError_t launch_polish_mark(int K, int32_t* phase, const int32_t* status, int32_t* counters,
                              hipStream_t s) {
  hipLaunchKernelGGL(polish_mark_kernel, dim3((K + 255) / 256), dim3(256), 0, s, K, phase, status,
                     counters);
  return hipGetLastError();
}

// sig_inv_theta = Sig_inv @ theta (models.py:131); still-running -> MAXITER.
// Sig_inv_theta[k] = Sig_inv[k] theta[k].  Grid (K, ceil(P / 16)): wave w of
// workgroup (k, y) takes rows 16 y + w + 4 r; a row is read coalesced (lane
// j + 64 m) against theta in LDS and summed by a fixed butterfly, so the
// result is the same run to run.  (One thread per row walked its row with a
// P-long dependent chain of strided loads: 0.27 ms per fit at P = 500, K = 32.)
__global__ __launch_bounds__(256) void fit_finalize_kernel(int K, int P, const double* theta,
                                                           const double* sig_inv,
                                                           double* sig_inv_theta, int32_t* status) {
  __shared__ double th[DLSA_MAX_P];
  const int k = blockIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const double* S = sig_inv + (int64_t)k * P * P;
  for (int j = threadIdx.x; j < P; j += 256) th[j] = theta[(int64_t)k * P + j];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = 16 * blockIdx.y + wid + 4 * r;  // wave-uniform
    if (i >= P) break;
    const double* Si = S + (int64_t)i * P;
    double acc = 0.0;
    for (int j = lane; j < P; j += 64) acc = fma(Si[j], th[j], acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) sig_inv_theta[(int64_t)k * P + i] = acc;
  }
  if (blockIdx.y == 0 && threadIdx.x == 0 && status[k] == STATUS_RUNNING)
    status[k] = DLSA_STATUS_MAXITER;
}

hipError_t launch_fit_finalize(int K, int P, const double* theta, const double* sig_inv,
                               double* sig_inv_theta, int32_t* status, hipStream_t s) {
  if (K <= 0 || P <= 0) return hipSuccess;
  if (P > DLSA_MAX_P) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fit_finalize_kernel, dim3(K, (P + 15) / 16), dim3(256), 0, s, K, P, theta,
                     sig_inv, sig_inv_theta, status);
  return hipGetLastError();
}

// theta_rec[k] = theta[k] for the partitions whose phase is ph: the point at
// which the next bf16 pass records their Ozaki digit scales
// gate: null, or the snapshot is taken only if gate[0] > 0 (the pass it
// belongs to records max |z| under the same condition, PassArgs::zrec_gate)
__global__ void theta_snapshot_kernel(int K, int P, const int32_t* phase, int ph,
                                      const double* theta, double* theta_rec, const int32_t* gate) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)K * P) return;
  if (gate && gate[0] <= 0) return;
  if (phase[i / P] == ph) theta_rec[i] = theta[i];
}

hipError_t launch_theta_snapshot(int K, int P, const int32_t* phase, int ph, const double* theta,
                                 double* theta_rec, hipStream_t s, const int32_t* gate) {
  const int64_t n = (int64_t)K * P;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(theta_snapshot_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, K,
                     P, phase, ph, theta, theta_rec, gate);
  return hipGetLastError();
}

// out = [sum_k Sig_inv_k | sum_k Sig_inv_k theta_k | sum_k theta_k | K]
// One thread per output element, partitions summed in index order.  The
// loads run 16 partitions ahead of the (sequential, order-preserving) adds:
// one dependent HBM round trip per partition made this 0.47 ms at K = 1024,
// P = 100 (40 workgroups, latency-bound).
template <int U>
__device__ __forceinline__ double ordered_sum(const double* __restrict__ a, int64_t stride, int K) {
  double s = 0.0;
  int k = 0;
  for (; k + U <= K; k += U) {
    double v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(a + (int64_t)(k + u) * stride);
#pragma unroll
    for (int u = 0; u < U; ++u) s += v[u];
  }
  for (; k < K; ++k) s += a[(int64_t)k * stride];
  return s;
}

__global__ void reduce_partitions_kernel(const double* sig_inv, const double* sig_inv_theta,
                                         const double* theta, int K, int P, double* out) {
  const int64_t PP2 = (int64_t)P * P;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < PP2) {
    out[e] = ordered_sum<16>(sig_inv + e, PP2, K);
  } else if (e < PP2 + P) {
    out[e] = ordered_sum<16>(sig_inv_theta + (e - PP2), P, K);
  } else if (e < PP2 + 2 * P) {
    out[e] = ordered_sum<16>(theta + (e - PP2 - P), P, K);
  } else if (e == PP2 + 2 * P) {
    out[e] = (double)K;
  }
}

hipError_t launch_reduce_partitions(const double* sig_inv, const double* sig_inv_theta,
                                    const double* theta, int K, int P, double* out,
                                    hipStream_t s) {
  const int64_t n = (int64_t)P * P + 2 * P + 1;
  const int threads = 64;  // P = 100: 158 one-wave workgroups instead of 40
  const int blocks = (int)((n + threads - 1) / threads);
  hipLaunchKernelGGL(reduce_partitions_kernel, dim3(blocks), dim3(threads), 0, s, sig_inv,
                     sig_inv_theta, theta, K, P, out);
  return hipGetLastError();
}

// ---- synthetic data: counter-based splitmix64 streams -----------------------
// X[i, j] = u(seed, (row0 + i) * p + j) - 0.5, y[i] = u(seed ^ kYSalt, row0 + i) <
// sigmoid(sum_{j < floor(0.4 p)} X[i, j]).  oracle/dlsa_oracle.py:simulate_counter
// restates it bit for bit.
__device__ __forceinline__ double u01(uint64_t seed, uint64_t ctr) {
  uint64_t z = seed + (ctr + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * 0x1.0p-53;
}
constexpr uint64_t kYSalt = 0x5DEECE66Dull;

__global__ void simulate_x_kernel(double* X, int64_t n, int p, uint64_t seed, int64_t row0) {
  const int64_t total = n * p;
  const int64_t base = row0 * p;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x)
    X[e] = u01(seed, (uint64_t)(base + e)) - 0.5;
}

__global__ void simulate_y_kernel(const double* X, double* y, int64_t n, int p, uint64_t seed,
                                  int64_t row0) {
  const int p1 = (int)(p * 0.4);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    double eta = 0.0;
    for (int j = 0; j < p1; ++j) eta = eta + X[i * p + j];
    const double prob = 1.0 / (1.0 + exp(-eta));
    y[i] = u01(seed ^ kYSalt, (uint64_t)(row0 + i)) < prob ? 1.0 : 0.0;
  }
}

hipError_t launch_simulate(double* X, double* y, int64_t n, int p, uint64_t seed, int64_t row0,
                           hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(simulate_x_kernel, dim3(8192), dim3(256), 0, s, X, n, p, seed, row0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(simulate_y_kernel, dim3(4096), dim3(256), 0, s, X, y, n, p, seed, row0);
  return hipGetLastError();
}

}  // namespace dlsa
