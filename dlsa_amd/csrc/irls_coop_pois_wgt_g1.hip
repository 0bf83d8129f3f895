// Poisson instantiations of the cooperative pass with per-row prior weights
// (IRLS weight omega w) for NT in {1, 2, 3, 4}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_pois_wgt_g1, FamPoisson, EX_WGT, 1, 2, 3, 4)

}  // namespace dlsa
