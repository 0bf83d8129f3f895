// Poisson instantiations of the cooperative pass for NT in {5, 6, 7, 8}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_pois_g2, FamPoisson, EX_NONE, 5, 6, 7, 8)

}  // namespace dlsa
