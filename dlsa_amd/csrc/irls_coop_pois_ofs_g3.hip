// Poisson instantiations of the cooperative pass with a per-row offset
// (eta = x . theta + eta_offset) for NT in {9, 10, 11, 12}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_pois_ofs_g3, FamPoisson, EX_OFS, 9, 10, 11, 12)

}  // namespace dlsa
