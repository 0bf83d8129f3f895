// Logistic instantiations of the cooperative pass with per-row prior weights
// (IRLS weight omega w, CM = 0 only) for NT in {9, 10, 11, 12}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_wgt_g3, FamLogistic, EX_WGT, 9, 10, 11, 12)

}  // namespace dlsa
