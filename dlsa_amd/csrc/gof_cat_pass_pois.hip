// Goodness-of-fit pass on the categorical-code layout, Poisson family: the
// four row-extras instantiations (none, offset, prior weights, both) of the
// kernel of gof_cat_pass_impl.hpp.
#include "gof_cat_pass_impl.hpp"

namespace dlsa {

hipError_t launch_gof_cat_pois(const GofCatArgs& a, int n_chunks, hipStream_t s) {
  switch ((a.eta_offset ? EX_OFS : 0) | (a.row_weight ? EX_WGT : 0)) {
    case EX_NONE: return gc_launch_bp<FAMILY_POISSON, EX_NONE>(a, n_chunks, s);
    case EX_OFS: return gc_launch_bp<FAMILY_POISSON, EX_OFS>(a, n_chunks, s);
    case EX_WGT: return gc_launch_bp<FAMILY_POISSON, EX_WGT>(a, n_chunks, s);
    default: return gc_launch_bp<FAMILY_POISSON, EX_OFS | EX_WGT>(a, n_chunks, s);
  }
}

}  // namespace dlsa
