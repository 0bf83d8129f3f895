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

// Checks the family's rules and routes on the row-extras mask, like
// launch_irls_coop; the weighted instantiations are eval_pass_wgt.hip's.
hipError_t launch_loglik_eval(const EvalArgsWgt& a, int family, int n_chunks, hipStream_t s) {
  const FamilyRules rules = family_rules(family);
  if (a.eta_offset && !rules.offset) return hipErrorInvalidValue;
  if (a.row_weight && !rules.weights) return hipErrorInvalidValue;
  const int ex = pass_extras(a);
  if (ex & EX_WGT) return launch_eval_unit_wgt(a, family, n_chunks, s);
  if (rules.sums_ll_const)  // the family whose log-likelihood has a constant term: its own kernel
    return ex & EX_OFS ? launch_eval_kernel<FAMILY_POISSON, EX_OFS>(a, n_chunks, s)
                       : launch_eval_kernel<FAMILY_POISSON, EX_NONE>(a, n_chunks, s);
  return launch_eval_kernel<FAMILY_LOGISTIC, EX_NONE>(a, n_chunks, s);
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
