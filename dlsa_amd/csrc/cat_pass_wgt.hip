// The categorical-code pass and presence pass with per-row prior weights
// (the kernel templates are cat_pass_impl.hpp's; the unweighted instantiations
// are cat_pass.hip's).  Same thread counts and LDS layout as the unweighted
// kernels: cat_layout and cat_lds_bytes do not look at the weights.
#include "cat_pass_impl.hpp"

namespace dlsa {

hipError_t launch_cat_pass_wgt(const CatArgsWgt& a, bool standardize, int n_chunks,
                               hipStream_t s) {
  if (!a.row_weight) return hipErrorInvalidValue;
  return launch_cat_pass_t<FAMILY_LOGISTIC, EX_WGT>(a, standardize, n_chunks, s);
}

hipError_t launch_cat_presence_wgt(const CatArgsWgt& a, int n_chunks, int32_t* counts,
                                   int32_t* bad, double* colmax, hipStream_t s) {
  if (!a.row_weight || !a.wmax) return hipErrorInvalidValue;
  return launch_cat_presence_t<true>(a, n_chunks, counts, bad, colmax, s);
}

}  // namespace dlsa
