// Goodness-of-fit pass on the dense layout: per partition and candidate the
// residual deviance and the Pearson chi-square, per partition the rows with
// omega > 0 -- what a GLM summary prints beside the log-likelihood, and the
// numerator of the dispersion estimate phi = chi^2 / (n - P) that a
// quasi-likelihood fit divides its information matrix by.  The ring and the
// bytes per row are the log-likelihood pass's (gof_pass_impl.hpp beside
// eval_pass_impl.hpp); the row terms are row_gof (glm_row.hpp).  One kernel
// per family and row-extras mask the log-likelihood pass has.
#include "gof_pass_impl.hpp"

namespace dlsa {

hipError_t launch_gof_eval(const GofArgs& a, int family, int n_chunks, hipStream_t s) {
  const FamilyRules rules = family_rules(family);
  if (a.eta_offset && !rules.offset) return hipErrorInvalidValue;
  if (a.row_weight && !rules.weights) return hipErrorInvalidValue;
  const int ex = pass_extras(a);
  if (family == FAMILY_POISSON) switch (ex) {
      case EX_NONE: return launch_gof_kernel<FAMILY_POISSON, EX_NONE>(a, n_chunks, s);
      case EX_OFS: return launch_gof_kernel<FAMILY_POISSON, EX_OFS>(a, n_chunks, s);
      case EX_WGT: return launch_gof_kernel<FAMILY_POISSON, EX_WGT>(a, n_chunks, s);
      default: return launch_gof_kernel<FAMILY_POISSON, EX_OFS | EX_WGT>(a, n_chunks, s);
    }
  if (family != FAMILY_LOGISTIC) return hipErrorInvalidValue;
  return ex & EX_WGT ? launch_gof_kernel<FAMILY_LOGISTIC, EX_WGT>(a, n_chunks, s)
                     : launch_gof_kernel<FAMILY_LOGISTIC, EX_NONE>(a, n_chunks, s);
}

}  // namespace dlsa
