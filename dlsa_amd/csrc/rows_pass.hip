// Row diagnostics pass on the dense layout: per row eta, mu, the signed
// deviance and Pearson residuals and the leverage h = omega w x^T S^-1 x at
// one coefficient vector and one factor R of S^-1 per partition.  This unit
// holds the logistic kernels and the launcher; rows_pass_pois.hip the Poisson
// kernels (rows_pass_impl.hpp).
#include "rows_pass_impl.hpp"

namespace dlsa {

hipError_t launch_rows_pass(const RowsArgs& a, int family, int n_chunks, hipStream_t s) {
  const FamilyRules rules = family_rules(family);
  if (a.eta_offset && !rules.offset) return hipErrorInvalidValue;
  if (a.P < 1 || a.P > DLSA_MAX_P_FUSED) return hipErrorInvalidValue;
  if (a.leverage && !a.rfac) return hipErrorInvalidValue;
  if (family == FAMILY_POISSON) return launch_rows_unit_pois(a, n_chunks, s);
  if (family != FAMILY_LOGISTIC) return hipErrorInvalidValue;
  return launch_rows_family<FAMILY_LOGISTIC>(a, n_chunks, s,
                                             std::make_integer_sequence<int, kScoreMaxNT>{});
}

}  // namespace dlsa
