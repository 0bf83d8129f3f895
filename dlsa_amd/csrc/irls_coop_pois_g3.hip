// Poisson instantiations of the cooperative pass for NT in {9, 10, 11, 12}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_pois_g3, FamPoisson, EX_NONE, 9, 10, 11, 12)

}  // namespace dlsa
