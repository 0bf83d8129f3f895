// Poisson instantiations of the cooperative pass with a per-row offset
// (eta = x . theta + eta_offset) for NT in {5, 6, 7, 8}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_pois_ofs_g2, FamPoisson, EX_OFS, 5, 6, 7, 8)

}  // namespace dlsa
