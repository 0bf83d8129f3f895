// Logistic instantiations of the cooperative pass with per-row prior weights
// (IRLS weight omega w, CM = 0 only) for NT in {5, 6, 7, 8}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_wgt_g2, FamLogistic, EX_WGT, 5, 6, 7, 8)

}  // namespace dlsa
