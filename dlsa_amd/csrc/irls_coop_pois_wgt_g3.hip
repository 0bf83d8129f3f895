// Poisson instantiations of the cooperative pass with per-row prior weights
// (IRLS weight omega w) for NT in {9, 10, 11, 12}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_pois_wgt_g3, FamPoisson, EX_WGT, 9, 10, 11, 12)

}  // namespace dlsa
