// Poisson instantiations of the cooperative pass with a per-row offset
// (eta = x . theta + eta_offset) for NT in {1, 2, 3, 4}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_pois_ofs_g1, FamPoisson, EX_OFS, 1, 2, 3, 4)

}  // namespace dlsa
