// Goodness-of-fit pass on the categorical-code layout, logistic family: per
// partition and candidate the deviance and the Pearson chi-square of the
// dummy-expanded design, read as the log-likelihood pass reads it (the
// instantiations of gof_cat_pass_impl.hpp, without and with prior weights).
#include "gof_cat_pass_impl.hpp"

namespace dlsa {

hipError_t launch_gof_cat(const GofCatArgs& a, int n_chunks, hipStream_t s) {
  return a.row_weight ? gc_launch_bp<FAMILY_LOGISTIC, EX_WGT>(a, n_chunks, s)
                      : gc_launch_bp<FAMILY_LOGISTIC, EX_NONE>(a, n_chunks, s);
}

}  // namespace dlsa
