// Poisson regression on the categorical-code layout with a per-row offset:
// the pass and presence kernels of this row-extras mask (cat_pois_impl.hpp;
// the routing and the grid kernels are cat_pass_pois.hip's).
#include "cat_pois_impl.hpp"

namespace dlsa {

DLSA_CAT_POIS_UNIT(EX_OFS)

}  // namespace dlsa
