// Log-likelihood evaluation pass with per-row prior weights: ll[k, b] = sum_i
// omega_i l_ib (the kernel template is eval_pass_impl.hpp; the unweighted
// instantiations are eval_pass.hip's).
#include "eval_pass_impl.hpp"

namespace dlsa {

hipError_t launch_loglik_eval_wgt(const EvalArgsWgt& a, int family, int n_chunks, hipStream_t s) {
  const size_t lds = eval_lds_bytes(a);
  const FamilyRules rules = family_rules(family);
  if (!a.row_weight || !rules.weights) return hipErrorInvalidValue;
  if (a.eta_offset && !rules.offset) return hipErrorInvalidValue;
  auto kern = !rules.sums_ll_const ? loglik_eval_kernel<FAMILY_LOGISTIC, EX_WGT>
              : a.eta_offset       ? loglik_eval_kernel<FAMILY_POISSON, EX_OFS | EX_WGT>
                                   : loglik_eval_kernel<FAMILY_POISSON, EX_WGT>;
  {
    hipError_t e = ensure_max_lds((const void*)kern, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3(n_chunks), dim3(256), lds, s, a);
  return hipGetLastError();
}

}  // namespace dlsa
