// Log-likelihood evaluation pass: one streaming pass
// over X computing, per partition and per candidate coefficient vector b,
//   ll[k, b] = sum_i y_i eta_ib - log(1 + exp(eta_ib)),  eta_ib = x_i . beta_b
// -- the per-partition work of dlsa/models.py:151-225 logistic_model_eval
// (driven by dlsa/model_eval.py:10-42 over the AIC / BIC / WLSE / ONESHOT
// columns).  HBM-bound: X and y are read once for all candidates.
//
// Geometry: one 4-wave workgroup per chunk; 32-row blocks through the same
// shared LDS-DMA ring as the fused IRLS pass; 8 lanes per row, the candidate
// vectors in LDS.
#include "eval_pass_impl.hpp"

namespace dlsa {

int eval_slot_bytes(int p, int n_extras) { return eval_slot_bytes_impl(p, n_extras); }

hipError_t launch_loglik_eval(const EvalArgs& a, int family, int n_chunks, hipStream_t s) {
  const size_t lds = eval_lds_bytes(a);
  const FamilyRules rules = family_rules(family);
  if (a.eta_offset && !rules.offset) return hipErrorInvalidValue;
  // the family whose log-likelihood has a constant term has its own kernel
  auto kern = !rules.sums_ll_const ? loglik_eval_kernel<FAMILY_LOGISTIC>
              : a.eta_offset       ? loglik_eval_kernel<FAMILY_POISSON, EX_OFS>
                                   : loglik_eval_kernel<FAMILY_POISSON>;
  {
    hipError_t e = ensure_max_lds((const void*)kern, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3(n_chunks), dim3(256), lds, s, a);
  return hipGetLastError();
}

// ll[k, b] = sum of the chunk partials of partition k (fixed order)
__global__ void loglik_reduce_kernel(const double* partial, const int32_t* pcb, int K, int B,
                                     double* out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= K * B) return;
  const int k = e / B, b = e - k * B;
  double s = 0.0;
  for (int c = pcb[k]; c < pcb[k + 1]; ++c) s += partial[(int64_t)c * B + b];
  out[e] = s;
}

hipError_t launch_loglik_reduce(const double* partial, const int32_t* pcb, int K, int B,
                                double* out, hipStream_t s) {
  hipLaunchKernelGGL(loglik_reduce_kernel, dim3((K * B + 255) / 256), dim3(256), 0, s, partial,
                     pcb, K, B, out);
  return hipGetLastError();
}

}  // namespace dlsa
