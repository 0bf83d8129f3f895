// Log-likelihood evaluation pass with per-row prior weights: ll[k, b] = sum_i
// omega_i l_ib (the kernel template is eval_pass_impl.hpp; the unweighted
// instantiations are eval_pass.hip's).
#include "eval_pass_impl.hpp"

namespace dlsa {

// (launch_loglik_eval has checked the family's rules; a.row_weight is set)
hipError_t launch_eval_unit_wgt(const EvalArgsWgt& a, int family, int n_chunks, hipStream_t s) {
  if (family_rules(family).sums_ll_const)
    return a.eta_offset ? launch_eval_kernel<FAMILY_POISSON, EX_OFS | EX_WGT>(a, n_chunks, s)
                        : launch_eval_kernel<FAMILY_POISSON, EX_WGT>(a, n_chunks, s);
  return launch_eval_kernel<FAMILY_LOGISTIC, EX_WGT>(a, n_chunks, s);
}

}  // namespace dlsa
