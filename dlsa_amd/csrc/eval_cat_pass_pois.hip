// Log-likelihood evaluation pass on the categorical-code layout, Poisson
// family (log link): the four row-extras instantiations of
// eval_cat_pass_impl.hpp (none, offset, prior weights, both).
#include "eval_cat_pass_impl.hpp"

namespace dlsa {

hipError_t launch_loglik_cat_pois(const EvalCatArgsPois& a, int n_chunks, hipStream_t s) {
  switch ((a.eta_offset ? EX_OFS : 0) | (a.row_weight ? EX_WGT : 0)) {
    case EX_NONE: return ec_launch_bp<FAMILY_POISSON, EX_NONE>(a, n_chunks, s);
    case EX_OFS: return ec_launch_bp<FAMILY_POISSON, EX_OFS>(a, n_chunks, s);
    case EX_WGT: return ec_launch_bp<FAMILY_POISSON, EX_WGT>(a, n_chunks, s);
    default: return ec_launch_bp<FAMILY_POISSON, EX_OFS | EX_WGT>(a, n_chunks, s);
  }
}

}  // namespace dlsa
